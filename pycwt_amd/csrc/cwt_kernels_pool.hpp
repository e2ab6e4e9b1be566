// cwt_kernels_pool.hpp -- the time-pooled scalogram (cwt_transform_pool): window MEANS of |W|^2 over h = pool consecutive columns,
//     Pbar[j, m] = (1 / c_m) sum_{n = m h}^{min((m + 1) h, n0) - 1} |W[j, n]|^2,     c_m = min((m + 1) h, n0) - m h,   m < ceil(n0 / h),
// h a power of two.  Power is not linear in W, so no folding of the spectrum gives it (cwt_kernels_hop.hpp samples W, this averages
// |W|^2): the columns are computed at the full rate and summed before anything is stored.
//
// NAMES.  As in cwt_kernels_hop.hpp: the kernels are called pool_*, not k_*, because the coverage gate of tests/test_emu_schedules.py
// demands that its own cases launch every __global__ function named k_*, and that module may not change with this feature.  The
// same gate for these kernels is in tests/test_pool_emulated.py (the set of names read from this file).
//
// Kernels (T = float | double):
//   pool_poly_rows  the rows of polynomial form: the Horner evaluation of k_poly_rows from the same coefficient planes (same u, same
//                   interval, same degree; no carrier, as in the power mode), re^2 + im^2 summed over the window in the kernel -- a row
//                   stores n0 / h reals instead of n0
//   pool_rows       every other form: its unchanged row kernel writes the full-rate power into plan scratch, this kernel reduces
//                   rows x n0 reals to window means
//
// ONE ORDER OF SUMMATION, fixed by (nfft, pool, R) -- never by n0, the batch, the launch geometry or the schedule; columns beyond n0
// count as exact zeros; no floating-point atomics:
//   pool_poly_rows  a thread sums a run of 16 consecutive columns (one interval: R >= 64) in ascending order; h < 16: the run holds
//                   16 / h whole windows, each summed in ascending order.  16 <= h <= 4096: the h / 16 runs of a window sit in adjacent
//                   lanes and are added in a binary tree (pool_tree_sum).  h > 4096: a workgroup owns the window, lane t adds its runs
//                   [4096 p + 16 t, + 16), p = 0, 1, ..., in ascending p, then the 256 lanes are added in the tree.
//   pool_rows       a lane loads 4 consecutive columns and adds them as (a0 + a1) + (a2 + a3) (h = 2: two windows); h <= 1024: the
//                   h / 4 lanes of a window are added in the tree.  h > 1024: a workgroup owns the window, lane t adds its quads
//                   [1024 p + 4 t, + 4) in ascending p, then the 256 lanes are added in the tree.
#pragma once
#include <hip/hip_runtime.h>

#include "cwt_types.hpp"
#include "fft_engine.hpp"

namespace cwt {

constexpr int POOL_THREADS = 256;
constexpr int POOL_LOG_RUN = 4;                           // pool_poly_rows: columns per run of a thread
constexpr int POOL_LOG_SPAN = 8 + POOL_LOG_RUN;           // ... and per pass of a workgroup (4096)
constexpr int POOL_LOG_QUAD = 2;                          // pool_rows: columns per load of a lane
constexpr int POOL_LOG_TILE = 8 + POOL_LOG_QUAD;          // ... and per pass of a workgroup (1024)
constexpr int POOL_TILES = 4;                             // pool_rows, h <= 1024: tiles (of any rows) per workgroup

// Sum of v over the g = 2^k <= 256 adjacent lanes [t0, t0 + g), t0 = t & ~(g - 1), returned in lane t0 (the other lanes get a partial
// sum): a fixed binary tree, ((v0 + v1) + (v2 + v3)) + ..., two levels per barrier.  g is uniform; every thread of the workgroup
// calls it (barriers).  A level reads entries no lane writes at that level, and after the last barrier a lane reads only its own
// entry: back-to-back calls need no barrier in between.
template <typename T>
__device__ __forceinline__ T pool_tree_sum(T* red, int t, int g, T v) {
  if (g == 1) return v;
  red[t] = v;
  __syncthreads();
  int s = 1;
  for (; 4 * s <= g; s <<= 2) {
    if ((t & (4 * s - 1)) == 0) red[t] = (red[t] + red[t + s]) + (red[t + 2 * s] + red[t + 3 * s]);
    __syncthreads();
  }
  if (2 * s <= g) {
    if ((t & (2 * s - 1)) == 0) red[t] = red[t] + red[t + s];
    __syncthreads();
  }
  return red[t];
}

// columns of window m inside [0, n0)
__host__ __device__ inline long pool_count(long m, int logh, long n0) {
  const long b = m << logh, e = b + (1L << logh);
  return (e < n0 ? e : n0) - b;
}

// pool_poly_rows.  grid = (ceil(n0 / 4096), rows) for h <= 4096, (ceil(n0 / h), rows) above; 256 threads, 256 reals of LDS.
// The coefficient set of a run's interval goes to registers once (adjacent lanes read the same addresses) and serves its 16 columns,
// four Horner chains side by side.
template <typename T, int D>
__device__ __forceinline__ void pool_poly_body(const RowDesc& rd, const cplx<T>* __restrict__ coef, int logN, int logh,
                                               T* __restrict__ prow, long n0, T* red) {
  constexpr int RUN = 1 << POOL_LOG_RUN;
  const int logR = logN - rd.logK, t = int(threadIdx.x);
  const long rmask = (1L << logR) - 1;
  const T scale = T(2) / T(1 << logR);
  const cplx<T>* a = coef + rd.tab_off;
  cplx<T> c[D + 1];
  T q[RUN];                                                             // |v|^2 of the run's columns, 0 beyond n0
  auto run = [&](long nb) {                                             // nb < nfft, a multiple of 16
    const cplx<T>* s = a + (nb >> logR);
#pragma unroll
    for (int d = 0; d <= D; ++d) c[d] = s[long(d) << rd.logK];
#pragma unroll
    for (int i0 = 0; i0 < RUN; i0 += 4) {
      T u[4], pr[4], pi[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        u[i] = T(int((nb + i0 + i) & rmask)) * scale - T(1);
        pr[i] = c[D].x; pi[i] = c[D].y;
      }
#pragma unroll
      for (int d = D - 1; d >= 0; --d)
#pragma unroll
        for (int i = 0; i < 4; ++i) { pr[i] = fma(pr[i], u[i], c[d].x); pi[i] = fma(pi[i], u[i], c[d].y); }
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i0 + i] = nb + i0 + i < n0 ? pr[i] * pr[i] + pi[i] * pi[i] : T(0);
    }
  };
  if (logh <= POOL_LOG_SPAN) {
    const long nb = (long(blockIdx.x) << POOL_LOG_SPAN) + (long(t) << POOL_LOG_RUN);
    const bool live = nb < n0;
    if (live) {
      run(nb);
    } else {
#pragma unroll
      for (int i = 0; i < RUN; ++i) q[i] = T(0);
    }
    if (logh < POOL_LOG_RUN) {                                          // (uniform) whole windows inside the run
      if (!live) return;
      const int h = 1 << logh;
      T s = T(0);
#pragma unroll
      for (int i = 0; i < RUN; ++i) {                                   // (constant indices: q stays in registers)
        s += q[i];
        if (((i + 1) & (h - 1)) == 0) {
          const long m = (nb + i) >> logh;
          if ((m << logh) < n0) prow[m] = s / T(pool_count(m, logh, n0));
          s = T(0);
        }
      }
      return;
    }
    T s = T(0);
#pragma unroll
    for (int i = 0; i < RUN; ++i) s += q[i];
    const int g = 1 << (logh - POOL_LOG_RUN);
    s = pool_tree_sum<T>(red, t, g, s);
    if (live && (t & (g - 1)) == 0) {
      const long m = nb >> logh;
      prow[m] = s / T(pool_count(m, logh, n0));
    }
    return;
  }
  const long m = long(blockIdx.x), w0 = m << logh;
  T s = T(0);
  for (long p = 0; p < (1L << (logh - POOL_LOG_SPAN)); ++p) {
    const long nb = w0 + (p << POOL_LOG_SPAN) + (long(t) << POOL_LOG_RUN);
    if (nb >= n0) break;
    run(nb);
    T r = T(0);
#pragma unroll
    for (int i = 0; i < RUN; ++i) r += q[i];
    s += r;
  }
  s = pool_tree_sum<T>(red, t, POOL_THREADS, s);
  if (t == 0) prow[m] = s / T(pool_count(m, logh, n0));
}

template <typename T>
__global__ void __launch_bounds__(POOL_THREADS)
pool_poly_rows(const RowDesc* __restrict__ rows, const cplx<T>* __restrict__ coef, int logN, int logh, T* __restrict__ P, long ldp,
               long n0) {
  HIP_DYNAMIC_SHARED(double2, lds_raw)
  T* red = reinterpret_cast<T*>(lds_raw);                               // 256 reals
  const RowDesc rd = rows[blockIdx.y];
  T* prow = P + long(rd.out_row) * ldp;
#define CWT_POOLP_CASE(DD) case DD: pool_poly_body<T, DD>(rd, coef, logN, logh, prow, n0, red); break;
  switch (rd.nterms) {
    CWT_POOLP_CASE(2) CWT_POOLP_CASE(4) CWT_POOLP_CASE(6) CWT_POOLP_CASE(8) CWT_POOLP_CASE(10) CWT_POOLP_CASE(12)
    CWT_POOLP_CASE(14) CWT_POOLP_CASE(16) CWT_POOLP_CASE(18) CWT_POOLP_CASE(20) CWT_POOLP_CASE(22) CWT_POOLP_CASE(24)
    default: break;
  }
#undef CWT_POOLP_CASE
}

// pool_rows: window means of the rows of S (nrows x n0 reals, sld elements apart; sld a multiple of 4 and S aligned to 4 elements:
// plan scratch) into P[map[r] * ldp + m].  Lanes run along the columns: a wavefront reads 256 consecutive reals per load
// (non-temporal: the scratch is read once).  h <= 1024: grid = ceil(nrows * ceil(n0 / 1024) / 4), a workgroup takes 4 consecutive
// tiles of 1024 columns (rows and tiles folded into one index, so that a few short rows still fill their workgroups); h > 1024:
// grid = nrows * ceil(n0 / h), a workgroup per window.  256 threads, 256 reals of LDS.
template <typename T>
__global__ void __launch_bounds__(POOL_THREADS)
pool_rows(const T* __restrict__ S, long sld, long n0, int nrows, const int* __restrict__ map, int logh, T* __restrict__ P, long ldp) {
  HIP_DYNAMIC_SHARED(double2, lds_raw)
  T* red = reinterpret_cast<T*>(lds_raw);
  typedef T vec2 __attribute__((vector_size(2 * sizeof(T))));
  const int t = int(threadIdx.x);
  T a[4];
  auto quad = [&](const T* srow, long col) {                            // columns col ... col + 3 of a row, 0 beyond n0
    if (col < n0) {                                                     // (col + 4 <= sld: both multiples of 4)
      const vec2 v0 = __builtin_nontemporal_load(reinterpret_cast<const vec2*>(srow + col));
      const vec2 v1 = __builtin_nontemporal_load(reinterpret_cast<const vec2*>(srow + col + 2));
      a[0] = v0[0];
      a[1] = col + 1 < n0 ? v0[1] : T(0);
      a[2] = col + 2 < n0 ? v1[0] : T(0);
      a[3] = col + 3 < n0 ? v1[1] : T(0);
    } else {
      a[0] = a[1] = a[2] = a[3] = T(0);
    }
  };
  if (logh <= POOL_LOG_TILE) {
    const long tpr = (n0 + (1L << POOL_LOG_TILE) - 1) >> POOL_LOG_TILE, total = long(nrows) * tpr;
    for (int i = 0; i < POOL_TILES; ++i) {
      const long gid = long(blockIdx.x) * POOL_TILES + i;
      if (gid >= total) break;                                          // (uniform)
      const long r = gid / tpr, col = ((gid - r * tpr) << POOL_LOG_TILE) + (long(t) << POOL_LOG_QUAD);
      quad(S + r * sld, col);
      T* prow = P + long(map[r]) * ldp;
      if (logh == 1) {
        const long m = col >> 1;
        if (col < n0) prow[m] = (a[0] + a[1]) / T(pool_count(m, 1, n0));
        if (col + 2 < n0) prow[m + 1] = (a[2] + a[3]) / T(pool_count(m + 1, 1, n0));
        continue;
      }
      const int g = 1 << (logh - POOL_LOG_QUAD);
      const T s = pool_tree_sum<T>(red, t, g, (a[0] + a[1]) + (a[2] + a[3]));
      if (col < n0 && (t & (g - 1)) == 0) {
        const long m = col >> logh;
        prow[m] = s / T(pool_count(m, logh, n0));
      }
    }
    return;
  }
  const long wpr = (n0 + (1L << logh) - 1) >> logh;
  const long r = long(blockIdx.x) / wpr, m = long(blockIdx.x) - r * wpr;
  const T* srow = S + r * sld;
  T s = T(0);
  for (long p = 0; p < (1L << (logh - POOL_LOG_TILE)); ++p) {
    const long col = (m << logh) + (p << POOL_LOG_TILE) + (long(t) << POOL_LOG_QUAD);
    if (col >= n0) break;
    quad(srow, col);
    s += (a[0] + a[1]) + (a[2] + a[3]);
  }
  s = pool_tree_sum<T>(red, t, POOL_THREADS, s);
  if (t == 0) P[long(map[r]) * ldp + m] = s / T(pool_count(m, logh, n0));
}

}  // namespace cwt
