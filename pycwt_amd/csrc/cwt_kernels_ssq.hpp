// cwt_kernels_ssq.hpp -- the synchrosqueezed transform (cwt_spectrum_derivative, cwt_ssq_reassign): W reassigned along frequency
// by its own instantaneous frequency (Daubechies, Lu and Wu 2011).  Two steps beside the row kernels, which stay as they are:
//   dW[j, n] = (1/N) sum_k (i w_k xhat[k]) F_j[k] e^{2 pi i k n / N}   the time derivative of W: cwt_transform_rows on the spectrum
//                                                                     of the derivative signal -- exact, no finite difference
//   S[k, n]  = sum_{j kept, k(j, n) = k} w_j W[j, n]                   every entry added into the row of ITS frequency
// with, per entry (T = the plan's real type; the first three lines in T, every operation rounded once -- no fused multiply-add --
// so that a host can restate the decisions bit for bit),
//   a2  = Re W^2 + Im W^2
//   q   = (Im dW Re W - Re dW Im W) / a2                               = Im(dW / W), radians per time unit
//   pos = (log2(q) - log2(2 pi f_lo)) / dv       (in double)           position on the grid f_k = f_lo 2^(k dv), 0 <= k < nf
//   k   = floor(pos + 0.5)
// kept iff a2 > gamma^2 (compared in double), q > 0 and finite, 0 <= k < nf.  Zeros, NaN (in W or in dW), negative instantaneous
// frequencies and entries outside the grid are dropped.
//
// NAMES.  As in cwt_kernels_hop.hpp / _pool.hpp: the kernels are called ssq_*, not k_*, because the coverage gate of
// tests/test_emu_schedules.py demands that its own cases launch every __global__ function named k_*, and that module may not change
// with this feature.  The same gate for these kernels is in tests/test_ssq_schedules_emulated.py (the names read from this file).
//
// Kernels (T = float | double):
//   ssq_spec_deriv  yhat[k] = i w_k xhat[k], w_k = 2 pi signed_bin(k) / (N dt) formed in double; the Nyquist bin N / 2 is written
//                   as 0 (the derivative of a real signal stays real).  One thread per bin, reads its bin before it writes it:
//                   may run in place
//   ssq_zero        columns < ncols of the nf rows of S set to 0 (the call with accumulate = 0)
//   ssq_reassign    one thread per column n, lanes along n -- k_icwt's layout: 128-thread workgroups, non-temporal loads of W and dW
//                   (read once), 8 rows in flight.  The thread walks j ascending and keeps the CURRENT cell S[k, n] in registers:
//                   loaded when the bin changes, entries added in order, stored when the bin changes and at the end.  The
//                   arithmetic is exactly S[k, n] += w_j W[j, n] per kept entry in ascending j, whatever the split of the rows over
//                   calls (a stored cell is reloaded with its bits).  One thread owns a column: no atomics, no LDS, no traffic
//                   between lanes.  Rows next to each other near a ridge share a bin, so the cell traffic is small beside the
//                   2 x 16 B (complex128) read per entry.
#pragma once
#include <hip/hip_runtime.h>

#include "cwt_types.hpp"
#include "fft_engine.hpp"

namespace cwt {

template <typename T>
__global__ void ssq_spec_deriv(const cplx<T>* xhat, int N, double w1, cplx<T>* yhat) {
  const int k = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= N) return;
  const cplx<T> x = xhat[k];
  const int sk = k < (N >> 1) ? k : k - N;
  const double w = w1 * double(sk);                                   // w1 = 2 pi / (N dt)
  yhat[k] = 2 * k == N ? mk<T>(T(0), T(0)) : mk<T>(T(-w * double(x.y)), T(w * double(x.x)));
}

template <typename T>
__global__ void ssq_zero(cplx<T>* __restrict__ S, long ldt, long ncols) {
  const long n = long(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n < ncols) S[long(blockIdx.y) * ldt + n] = mk<T>(T(0), T(0));
}

// One entry (v = W[j, n], d = dW[j, n]) in two steps, shared with the kernel of cwt_kernels_ssq_grad.hpp that also records the bins:
//   ssq_bin   the decision: the bin k of a kept entry, -1 of a dropped one
//   ssq_add   the accumulation of a kept entry (weight wj) into the column whose first element is col; cur = the bin of the cell
//             held in acc (-1: none yet)
template <typename T>
__device__ __forceinline__ int ssq_bin(const cplx<T> v, const cplx<T> d, double g2, double l0, double inv_dv, int nf) {
#pragma clang fp contract(off)
  const T rr = v.x * v.x, ii = v.y * v.y;
  const T a2 = rr + ii;
  const T p1 = d.y * v.x, p2 = d.x * v.y;
  const T q = (p1 - p2) / a2;
  if (!(double(a2) > g2) || !(q > T(0))) return -1;                   // (a NaN fails either comparison)
  const double kf = floor((log2(double(q)) - l0) * inv_dv + 0.5);
  if (!(kf >= 0.0 && kf < double(nf))) return -1;                     // (q = inf ends here)
  return int(kf);
}

template <typename T>
__device__ __forceinline__ void ssq_add(const cplx<T> v, const T wj, const int k, cplx<T>* col, long ldt, int& cur, cplx<T>& acc) {
#pragma clang fp contract(off)
  if (k != cur) {
    if (cur >= 0) col[long(cur) * ldt] = acc;
    acc = col[long(k) * ldt];
    cur = k;
  }
  const T tr = wj * v.x, ti = wj * v.y;
  acc.x += tr;
  acc.y += ti;
}

// The walk of one thread down its column (W, dW, col and bcol point at the column's first element): rows ascending, SSQ_INFLIGHT
// rows in flight, the current cell in registers.  BINS: bcol[j ldb] = the bin of entry j as int16, -1 for a dropped one (2 B
// written beside the 2 x 16 B read; nf <= 32767 is the caller's business); without BINS bcol is not touched.
constexpr int SSQ_THREADS = 128, SSQ_INFLIGHT = 8;
template <typename T, bool BINS>
__device__ __forceinline__ void ssq_column(const cplx<T>* __restrict__ W, const cplx<T>* __restrict__ dW, long ld, int nrows,
                                           const T* __restrict__ w, double g2, double l0, double inv_dv, int nf, cplx<T>* col,
                                           long ldt, short* bcol, long ldb) {
  constexpr int U = SSQ_INFLIGHT;
  int cur = -1;
  cplx<T> acc = mk<T>(T(0), T(0));
  int j = 0;
  for (; j + U <= nrows; j += U) {
    cplx<T> v[U], d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = load_once<T>(W + long(j + u) * ld);
      d[u] = load_once<T>(dW + long(j + u) * ld);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = ssq_bin<T>(v[u], d[u], g2, l0, inv_dv, nf);
      if (BINS) __builtin_nontemporal_store(short(k), bcol + long(j + u) * ldb);
      if (k >= 0) ssq_add<T>(v[u], w[j + u], k, col, ldt, cur, acc);
    }
  }
  for (; j < nrows; ++j) {
    const cplx<T> v = load_once<T>(W + long(j) * ld), d = load_once<T>(dW + long(j) * ld);
    const int k = ssq_bin<T>(v, d, g2, l0, inv_dv, nf);
    if (BINS) __builtin_nontemporal_store(short(k), bcol + long(j) * ldb);
    if (k >= 0) ssq_add<T>(v, w[j], k, col, ldt, cur, acc);
  }
  if (cur >= 0) col[long(cur) * ldt] = acc;
}

template <typename T>
__global__ void __launch_bounds__(SSQ_THREADS)
ssq_reassign(const cplx<T>* __restrict__ W, const cplx<T>* __restrict__ dW, long ld, long ncols, int nrows,
             const T* __restrict__ w, double g2, double l0, double inv_dv, int nf, cplx<T>* S, long ldt) {
  const long n = long(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n >= ncols) return;
  ssq_column<T, false>(W + n, dW + n, ld, nrows, w, g2, l0, inv_dv, nf, S + n, ldt, nullptr, 0);
}

}  // namespace cwt
