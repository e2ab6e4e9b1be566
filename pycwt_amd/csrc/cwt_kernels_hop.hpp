// cwt_kernels_hop.hpp -- the decimated transform (cwt_transform_hop, cwt_adjoint_rows_hop): every h-th column of W without
// the other h - 1.
//
// Sampling in time is folding in frequency.  With N = nfft, h = hop (a power of two), M = N / h:
//     W[j, m h] = (1/N) sum_{k' < M} Z_j[k'] e^{+2 pi i k' m / M},     Z_j[k'] = sum_{r < h} xhat[k' + r M] F_j[k' + r M],
// F_j the filter of cwt_transform_rows (RowDesc::amp carries the 1/N).  A row costs one pass over its support band, one M-point
// inverse transform in a workgroup (M <= 4096) and M stores; nothing of rows x n0 elements exists.  The rows are the plain
// supports of the row table (RowLayout::base: signed bins [k_lo, k_lo + nband) inside [-N/2, N/2), the Nyquist bin -N/2 of a
// two-sided filter included, as k_small / k_pass_a see them through filtered_bin); no fast form is involved.
//
// NAMES.  Every other kernel of the library is called k_*; these three are called hop_* for one reason: the coverage gate of
// tests/test_emu_schedules.py lists the __global__ functions named k_* in csrc/*.hpp and demands that ITS OWN cases launch each of
// them, and that module may not change with this feature, whose kernels none of its cases can reach.  The same gate for these
// kernels is in tests/test_hop_emulated.py (every hop_* kernel of this file launched under every wavefront schedule, the set of
// names read from this file).  Whoever next may edit test_emu_schedules.py should add a hop case there and rename them k_hop_*.
//
// Kernels (T = float | double, WT the output scheme of fft_engine.hpp):
//   hop_fold       Z of the rows with MORE than `fuse_terms` aliases per folded bin, gridded over (slice of k', signal x row):
//                  bounded work per thread whatever the support (the smallest scales have nband ~ N/2, h aliases per bin)
//   hop_rows       the M-point inverse transform and the store of W / |W|^2 / (alpha Q) W; rows with at most `fuse_terms`
//                  aliases fold their band themselves (16 bins x terms filter values per thread), the others read Z
//   hop_adj_accum  the adjoint's accumulation: k_adj_accum reading spec_j[k mod M] -- the N-point transform of a row that is
//                  zero between its kept columns is its M-point transform, periodic in k
//
// ONE ORDER OF SUMMATION.  The h aliases of a folded bin are cut into S = 2^hop_log_slices(logN, logM) runs of consecutive r;
// a run is summed in ascending r, the runs are added in ascending order.  hop_fold gives a run to a thread and adds the runs
// through LDS, hop_rows walks the runs itself: both call hop_slice_sum and add its results in the same order, and S depends
// on (N, M) alone -- a signal's bits do not depend on the batch around it, on the launch geometry or on `fuse_terms`.
#pragma once
#include <hip/hip_runtime.h>

#include "cwt_types.hpp"
#include "fft_engine.hpp"

namespace cwt {

constexpr int HOP_LOG_POINTS = 12;     // complex points per workgroup of hop_rows: 2^(12 - logM) rows of M points, 256 threads
constexpr int HOP_FOLD_THREADS = 256;  // hop_fold: 2^logTK folded bins x S runs of aliases

// hop_fold covers min(M, 64) consecutive folded bins per workgroup (lanes along k': the reads of xhat are contiguous) ...
__host__ __device__ inline int hop_log_tk(int logM) { return logM < 6 ? logM : 6; }
// ... and cuts the h aliases of a bin into this many runs (4 for M >= 64, up to 16 at M = 16; never more than h)
__host__ __device__ inline int hop_log_slices(int logN, int logM) {
  const int logS = 8 - hop_log_tk(logM), logh = logN - logM;
  return logS < logh ? logS : logh;
}

// sum of xhat[k] F[k] over the unsigned bins k = kp (mod M), kb <= k < ke, inside the row's band, in ascending k: first the
// non-negative signed bins (k < N/2), then the negative ones (k >= N/2 stands for k - N)
template <typename T>
__device__ __forceinline__ cplx<T> hop_slice_sum(const cplx<T>* __restrict__ xhat, const RowDesc& rd, const Mother& mo, int kp,
                                                 int logN, int logM, int kb, int ke) {
  const int N = 1 << logN, M = 1 << logM;
  const int khi = rd.k_lo + rd.nband;
  T sr = T(0), si = T(0);
  {
    int a = rd.k_lo > 0 ? rd.k_lo : 0, b = khi > 0 ? khi : 0;
    a = a > kb ? a : kb;
    b = b < ke ? b : ke;
    for (int k = kp + (((a - kp + M - 1) >> logM) << logM); k < b; k += M) {
      const cplx<T> v = filter_value<T>(xhat[k], rd, mo, k);
      sr += v.x; si += v.y;
    }
  }
  {
    int a = N + (rd.k_lo < 0 ? rd.k_lo : 0), b = N + (khi < 0 ? khi : 0);
    a = a > kb ? a : kb;
    b = b < ke ? b : ke;
    for (int k = kp + (((a - kp + M - 1) >> logM) << logM); k < b; k += M) {
      const cplx<T> v = filter_value<T>(xhat[k], rd, mo, k - N);
      sr += v.x; si += v.y;
    }
  }
  return mk<T>(sr, si);
}

// Z[kp] of one row: the runs in ascending order (what hop_fold computes with one thread per run)
template <typename T>
__device__ __forceinline__ cplx<T> hop_fold_bin(const cplx<T>* __restrict__ xhat, const RowDesc& rd, const Mother& mo, int kp,
                                                int logN, int logM) {
  const int logS = hop_log_slices(logN, logM), span = 1 << (logN - logS);
  cplx<T> z = hop_slice_sum<T>(xhat, rd, mo, kp, logN, logM, kp, kp + span);
  for (int s = 1; s < (1 << logS); ++s) {
    const cplx<T> v = hop_slice_sum<T>(xhat, rd, mo, kp, logN, logM, kp + s * span, kp + (s + 1) * span);
    z.x += v.x; z.y += v.y;
  }
  return z;
}

// aliases per folded bin of a row (an upper bound: the band is one run of nband consecutive signed bins)
__host__ __device__ inline int hop_terms(int nband, int logM) { return (nband + (1 << logM) - 1) >> logM; }

// hop_fold: grid = (M / TK, signals of the chunk x rows) x 256 threads, 256 complex of LDS.  Thread (run s, bin kk) sums its run;
// the threads of run 0 add the runs and write Z[(signal * nrows + row) * M + k'].  Rows that hop_rows folds itself leave at once.
template <typename T>
__global__ void __launch_bounds__(HOP_FOLD_THREADS)
hop_fold(const cplx<T>* __restrict__ xhat, long xhat_ld, const RowDesc* __restrict__ rows, int nrows, Mother mo, int logN,
         int logM, int fuse_terms, cplx<T>* __restrict__ Z) {
  HIP_DYNAMIC_SHARED(double2, lds_raw)
  cplx<T>* red = reinterpret_cast<cplx<T>*>(lds_raw);
  const int b = int(blockIdx.y) / nrows, row = int(blockIdx.y) - b * nrows;
  const RowDesc rd = rows[row];
  if (hop_terms(rd.nband, logM) <= fuse_terms) return;            // (uniform: the whole workgroup)
  const int logTK = hop_log_tk(logM), logS = hop_log_slices(logN, logM), span = 1 << (logN - logS);
  const int t = int(threadIdx.x), kk = t & ((1 << logTK) - 1), s = t >> logTK;
  const int kp = (int(blockIdx.x) << logTK) + kk;
  const cplx<T>* xh = xhat + long(b) * xhat_ld;
  cplx<T> v = mk<T>(T(0), T(0));
  if (s < (1 << logS)) v = hop_slice_sum<T>(xh, rd, mo, kp, logN, logM, kp + s * span, kp + (s + 1) * span);
  red[t] = v;
  __syncthreads();
  if (s != 0) return;
  cplx<T> z = red[kk];
  for (int i = 1; i < (1 << logS); ++i) {
    const cplx<T> w = red[(i << logTK) + kk];
    z.x += w.x; z.y += w.y;
  }
  Z[(long(blockIdx.y) << logM) + kp] = z;
}

// hop_rows: 2^(12 - LOGM) rows per workgroup (256 threads), row g = signal g / nrows of the chunk, table row g % nrows.
// M >= 256: the compile-time engine in the ROWS layout (lanes along the column index: loads of Z and stores of the output
// run in segments of M / 16 elements; M <= 1024 needs no workgroup barrier); shorter rows: the run-time engine.
// Only columns m < ncols_h are written; `out` is the chunk's first row, ld its leading dimension (Q's too, weighted mode).
template <typename T, int LOGM, typename WT>
__global__ void __launch_bounds__(1 << (HOP_LOG_POINTS - 4))
hop_rows(const cplx<T>* __restrict__ xhat, long xhat_ld, const cplx<T>* __restrict__ Z, const RowDesc* __restrict__ rows,
         int nrows, int total, Mother mo, const cplx<T>* __restrict__ tw, int logN, int fuse_terms, out_arg_t<WT> out, long ld,
         long ncols_h) {
  HIP_DYNAMIC_SHARED(double2, lds_raw)
  T* lds = reinterpret_cast<T*>(lds_raw);
  constexpr int LOGTB = HOP_LOG_POINTS - LOGM, LOGNT = LOGM - 4, NT = 1 << LOGNT;
  const int j = int(threadIdx.x) & (NT - 1), t = int(threadIdx.x) >> LOGNT;
  const int g = (int(blockIdx.x) << LOGTB) + t;
  const bool live = g < total;
  const int b = live ? g / nrows : 0, jr = live ? g - b * nrows : 0;
  T re[16], im[16];
  long orow = 0;
  if (live) {
    const RowDesc rd = rows[jr];
    orow = long(b) * nrows + rd.out_row;
    if (hop_terms(rd.nband, LOGM) <= fuse_terms) {
      const cplx<T>* xh = xhat + long(b) * xhat_ld;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const cplx<T> v = hop_fold_bin<T>(xh, rd, mo, j + (e << LOGNT), logN, LOGM);
        re[e] = v.x; im[e] = v.y;
      }
    } else {
      const cplx<T>* z = Z + (long(g) << LOGM) + j;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const cplx<T> v = z[e << LOGNT];
        re[e] = v.x; im[e] = v.y;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) { re[e] = T(0); im[e] = T(0); }
  }
  if constexpr (LOGM >= 8) {
    ct::Fft<T, LOGM, LOGTB, false> f;
    f.t = t; f.j = j;
    f.run(re, im, lds, tw);
  } else {
    Geo<T, false> geo;
    geo.logL = LOGM; geo.logTB = LOGTB; geo.t = t; geo.j = j;
    wg_ifft<T, false>(re, im, lds, geo, tw);
  }
  if (!live) return;
  out_ptr_t<WT> wrow = out + orow * ld;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const long m = j + (e << LOGNT);
    if (m < ncols_h) store_w<T>(wrow + m, re[e], im[e]);
  }
}

// hop_adj_accum: k_adj_accum for input rows that are zero between their kept columns -- spec holds their M-point transforms
// (cnt x M), read at k mod M.  acc[k] += sum_r F_r[k]/N conj(spec[r][k mod M]) over the chunk's rows in table order, bins inside
// a row's support only; one thread per bin, no atomics.  grid = N / 256, 256 threads.
template <typename T>
__global__ void __launch_bounds__(256)
hop_adj_accum(const cplx<T>* __restrict__ spec, const RowDesc* __restrict__ rows, int cnt, Mother mo, int logN, int logM,
              cplx<T>* __restrict__ acc) {
  const int N = 1 << logN, k = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (k >= N) return;
  const int ks = signed_bin(k, N), km = k & ((1 << logM) - 1);
  T sr = T(0), si = T(0);
  for (int r = 0; r < cnt; ++r) {
    const RowDesc rd = rows[r];
    if (unsigned(ks - rd.k_lo) >= unsigned(rd.nband)) continue;
    const cplx<T> x = spec[(long(r) << logM) + km];
    const cplx<T> v = filter_value<T>(mk<T>(x.x, -x.y), rd, mo, ks);
    sr += v.x; si += v.y;
  }
  const cplx<T> a = acc[k];
  acc[k] = mk<T>(a.x + sr, a.y + si);
}

}  // namespace cwt
