// cwt_kernels_shrink_grad.hpp -- the vector-Jacobian product of the thresholded inverse transform (cwt_icwt_shrink_adjoint).
//
// The forward (cwt_kernels_shrink.hpp) is y[n] = coeff sum_j w_j Re eta(W[j, n]; lambda_j), w_j = 1 / sqrt(s_j).  For the real
// cotangent gy[n] and t = (coeff w_j) gy[n], with W = a + ib, v = abs2_fma(W), l2 = lambda lambda, all in the plan's real type T:
//
//     mode        kept when                gr                         gi                     gl
//     0 hard      v > l2                   1                          0                      0
//     1 soft      f = 1 - q > 0            f + (q u) u                (q u) s                -u            r = sqrt(v), q = lambda / r,
//                                                                                                          u = a (1 / r), s = b (1 / r)
//     2 garrote   f = 1 - q > 0            f + (2 q) (a p)            (2 q) (b p)            -(2 lambda) p q = l2 / v, p = a / v
//
//     G[j, n] = t gr + i t gi  (dL/dRe W + i dL/dIm W: the convention of cwt_adjoint_rows),   glambda[j] = sum_n t gl.
//
// A dropped entry and v = 0 have gr = gi = gl = 0.  "Kept" is the forward's predicate on the forward's roundings (shrink_re: the
// same v, the same q, the same f), v == l2 included: the gradient of what the forward computed.  An entry with a NaN component or
// a NaN lambda has gr = gi = gl = NaN; a NaN gy[n] makes t NaN and with it column n of G and every glambda[j].  In modes -1
// (lambda NULL: the plain inverse, W is not read) and 0 the imaginary part is +0 (NaN for a NaN entry or lambda), not t 0.
//
// shgrad_rows: grid (slices of SHGRAD_SLICE columns, rows) x 256 threads.  One workgroup owns one row's slice, so lambda, l2 and
// coeff w_j are uniform; thread t handles the columns slice + t + 256 u, u < 8, all loads in flight before the first use.  W is
// read once (load_once), G is written with non-temporal stores; gy is read again by every row (it stays in cache or it does
// not: profiles/shrink_grad_bench.txt).  G may be W: an element is read and then written by the same thread, and nothing else
// reads it.
//
// ONE ORDER OF SUMMATION (as cwt_kernels_sgrad.hpp).  A thread adds its t gl in ascending order of u, the workgroup adds its threads
// in a fixed binary tree through LDS (workgroup barriers, no shuffles), shgrad_sum adds a row's slices in ascending order in
// double.  No atomics.  The bits of glambda[j] and of row j of G depend on (ncols, the row's data) only -- not on nrows, on the
// rows around it, on the stream or on how a caller splits the rows over calls.
//
// NAMES.  shgrad_*, not k_*, for the reason cwt_kernels_hop.hpp gives; gated in tests/test_shrink_grad_schedules_emulated.py.
#pragma once
#include <hip/hip_runtime.h>

#include "cwt_kernels_shrink.hpp"

namespace cwt {

constexpr int SHGRAD_THREADS = 256, SHGRAD_PER_THREAD = 8;
constexpr int SHGRAD_SLICE = SHGRAD_THREADS * SHGRAD_PER_THREAD;      // columns per workgroup

__host__ __device__ inline long shgrad_slices(long ncols) { return (ncols + SHGRAD_SLICE - 1) / SHGRAD_SLICE; }

// (gr, gi, gl) of one entry; MODE as above (MODE -1 never gets here)
template <typename T, int MODE>
__device__ __forceinline__ void shgrad_entry(const cplx<T> w, const T lam, const T lam2, T& gr, T& gi, T& gl) {
  const T v = abs2_fma(w);
  gr = gi = gl = T(0);
  if (v != v || lam != lam) { gr = gi = gl = v + lam; return; }
  if (!(v > T(0))) return;
  if (MODE == 0) {
    if (v > lam2) gr = T(1);
  } else if (MODE == 1) {
    const T r = shrink_sqrt(v), q = lam / r, f = T(1) - q;
    if (!(f > T(0))) return;
    const T ir = T(1) / r, u = w.x * ir, s = w.y * ir, qu = q * u;
    gr = f + qu * u;
    gi = qu * s;
    gl = -u;
  } else {
    const T q = lam2 / v, f = T(1) - q;
    if (!(f > T(0))) return;
    const T p = w.x / v, q2 = q + q;
    gr = f + q2 * (w.x * p);
    gi = q2 * (w.y * p);
    gl = -((lam + lam) * p);
  }
}

template <typename T>
__device__ __forceinline__ void store_once(cplx<T>* p, const T re, const T im) {
  typedef T vec2 __attribute__((vector_size(2 * sizeof(T))));
  vec2 v;
  v[0] = re;
  v[1] = im;
  __builtin_nontemporal_store(v, reinterpret_cast<vec2*>(p));
}

// W, G: the first of the launch's rows (row blockIdx.y at + blockIdx.y ld); w, lambda, partial likewise offset by the caller.
// SUM: partial[blockIdx.y * nslices + blockIdx.x] = the slice's sum of t gl.  W and G may be one buffer (no __restrict__).
template <typename T, int MODE, bool SUM>
__global__ void __launch_bounds__(SHGRAD_THREADS)
shgrad_rows(const cplx<T>* W, long ldw, long ncols, const T* __restrict__ w, const T* __restrict__ lambda, T coeff,
            const T* __restrict__ gy, cplx<T>* G, long ldg, long nslices, T* __restrict__ partial) {
  HIP_DYNAMIC_SHARED(double2, lds_raw)
  constexpr int U = SHGRAD_PER_THREAD;
  const int t = int(threadIdx.x);
  const long j = long(blockIdx.y), first = long(blockIdx.x) * SHGRAD_SLICE + t;
  const T c = coeff * w[j];
  const T lam = MODE >= 0 ? lambda[j] : T(0), lam2 = lam * lam;
  const cplx<T>* wrow = W + j * ldw;
  cplx<T>* grow = G + j * ldg;
  cplx<T> x[U];
  T g[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long n = first + long(u) * SHGRAD_THREADS;
    x[u] = mk<T>(T(0), T(0));
    g[u] = T(0);
    if (n < ncols) {
      if (MODE >= 0) x[u] = load_once<T>(wrow + n);
      g[u] = gy[n];
    }
  }
  T sum = T(0);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long n = first + long(u) * SHGRAD_THREADS;
    if (n < ncols) {
      const T tt = c * g[u];
      if (MODE < 0) {
        store_once<T>(grow + n, tt, T(0));
      } else {
        T gr, gi, gl;
        shgrad_entry<T, MODE>(x[u], lam, lam2, gr, gi, gl);
        store_once<T>(grow + n, tt * gr, MODE == 0 ? gi : tt * gi);
        if (SUM) sum += tt * gl;
      }
    }
  }
  if (SUM) {
    T* red = reinterpret_cast<T*>(lds_raw);                      // 256 sums
    red[t] = sum;
    __syncthreads();
    for (int s = 1; s < SHGRAD_THREADS; s <<= 1) {
      if ((t & (2 * s - 1)) == 0) red[t] = red[t] + red[t + s];
      __syncthreads();
    }
    if (t == 0) partial[j * nslices + long(blockIdx.x)] = red[0];
  }
}

// shgrad_sum: out[j] (+)= the sum of row j's slices in ascending order, in double.  One thread per row.
template <typename T>
__global__ void __launch_bounds__(SHGRAD_THREADS)
shgrad_sum(const T* __restrict__ partial, int nrows, long nslices, int accumulate, double* __restrict__ out) {
  const int j = int(blockIdx.x) * SHGRAD_THREADS + int(threadIdx.x);
  if (j >= nrows) return;
  const T* pp = partial + long(j) * nslices;
  double s = 0.0;
  for (long i = 0; i < nslices; ++i) s += double(pp[i]);
  out[j] = accumulate ? out[j] + s : s;
}

}  // namespace cwt
