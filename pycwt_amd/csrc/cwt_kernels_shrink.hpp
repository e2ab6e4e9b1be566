// cwt_kernels_shrink.hpp -- the thresholded inverse transform (cwt_icwt_shrink): TC98 eq. 11 over the SHRUNK coefficients,
//   out[n] = coeff sum_j Re eta(W[j, n]; lambda_j) w_j,     w_j = 1 / sqrt(s_j),
// with, per entry, v = abs2_fma(W) (cwt_kernels_select.hpp: the same rounding the selection ordered the entries by) and
// l2 = lambda lambda, both in the plan's real type T:
//   mode 0 hard      eta = W if v > l2, else 0
//   mode 1 soft      eta = W max(0, 1 - lambda / sqrt(v))
//   mode 2 garrote   eta = W max(0, 1 - l2 / v)
// v = 0 gives 0; lambda = 0 keeps everything; lambda = +inf drops the row; a NaN entry (v is NaN) or a NaN lambda gives NaN.  sqrt
// and the divisions are the correctly rounded ones.
//
// shrink_icwt is k_icwt (cwt_kernels_callers.hpp) with eta in front of the product: one thread per column, 128-thread workgroups,
// 8 rows in flight, non-temporal loads (W is read once), the same 8 accumulators folded in the same order.  With every lambda = 0
// in hard mode the factor is a selection of Re W itself, so the sums are those of k_icwt bit for bit.  The name: as in
// cwt_kernels_select.hpp, not k_*.
#pragma once
#include <hip/hip_runtime.h>

#include "cwt_kernels_select.hpp"

namespace cwt {

__device__ __forceinline__ double shrink_sqrt(const double v) { return __builtin_sqrt(v); }
__device__ __forceinline__ float shrink_sqrt(const float v) { return __builtin_sqrtf(v); }

template <typename T>
__device__ __forceinline__ T shrink_re(const cplx<T> w, const T lam, const T lam2, const int mode) {
  const T v = abs2_fma(w);
  if (v != v) return v;
  if (lam != lam) return lam;
  if (!(v > T(0))) return T(0);
  if (mode == 0) return v > lam2 ? w.x : T(0);
  const T f = mode == 1 ? T(1) - lam / shrink_sqrt(v) : T(1) - lam2 / v;
  return f > T(0) ? w.x * f : T(0);                          // (lambda = inf: f is -inf or NaN, never > 0)
}

template <typename T>
__global__ void __launch_bounds__(ICWT_THREADS)
shrink_icwt(const cplx<T>* __restrict__ W, long ldw, long ncols, int nrows, const T* __restrict__ w, const T* __restrict__ lambda,
            int mode, T coeff, T* __restrict__ out) {
  const long n = long(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n >= ncols) return;
  constexpr int U = ICWT_INFLIGHT;
  T acc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = T(0);
  int j = 0;
  for (; j + U <= nrows; j += U) {
    cplx<T> v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = load_once<T>(W + long(j + u) * ldw + n);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const T lam = lambda[j + u];
      acc[u] += shrink_re<T>(v[u], lam, lam * lam, mode) * w[j + u];
    }
  }
  for (; j < nrows; ++j) {
    const cplx<T> v = load_once<T>(W + long(j) * ldw + n);
    const T lam = lambda[j];
    acc[0] += shrink_re<T>(v, lam, lam * lam, mode) * w[j];
  }
  out[n] = coeff * (((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7])));
}

}  // namespace cwt
