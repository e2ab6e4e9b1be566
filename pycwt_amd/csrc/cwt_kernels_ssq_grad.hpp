// cwt_kernels_ssq_grad.hpp -- the gradient of the synchrosqueezed transform (cwt_ssq_reassign_bins, cwt_ssq_gather).
// Given the bin k(j, n) of every entry, T[k, n] = sum_{kept j, k(j, n) = k} w_j W[j, n] is linear in W, and k(j, n) and the keep /
// drop decision are piecewise constant in W, dW and gamma: almost everywhere the derivative runs through the values of W alone,
//   gW[j, n] = w_j gT[k(j, n), n]   for a kept entry,   0 for a dropped one
// (torch's convention for a map that is complex-linear in W with real weights; the derivative with respect to dW is zero).  The
// forward records the bins (int16, 2 B per entry, -1 = dropped), the backward gathers along frequency through them: neither W nor
// dW is held or recomputed.
//
// NAMES.  The kernels are called ssqg_* and live in this file: tests/test_ssq_schedules_emulated.py demands that the kernels of
// cwt_kernels_ssq.hpp are exactly the three it launches, and tests/test_emu_schedules.py that its own cases launch everything
// named k_*.  The gate of these kernels is in tests/test_ssq_grad_schedules_emulated.py, which reads the names from this file.
//
// Kernels (T = float | double):
//   ssqg_reassign_bins  ssq_reassign (the same walk, decision and accumulation: ssq_column of cwt_kernels_ssq.hpp, so the same
//                       bits of S) that also stores bins[j, n]: one non-temporal 2-B store per entry beside the 2 x 16 B read
//   ssqg_gather         G[j, n] = w_j gT[bins[j, n], n], +0 by selection where the bin is negative or >= nf (nothing outside gT
//                       is read).  Lanes along n, 128-thread workgroups; a thread owns SSQG_STRETCH consecutive rows of its
//                       column (blockIdx.y numbers the stretches): it loads their bins first (non-temporal, read once), then walks
//                       the rows ascending with the last cell of gT in registers, reloaded only when the bin changes -- near a
//                       ridge neighbouring rows share a bin.  One product per component in T; no atomics, no LDS, every element
//                       of G written by one thread: the same bits on every run.  All element offsets are long.
#pragma once
#include <hip/hip_runtime.h>

#include "cwt_kernels_ssq.hpp"

namespace cwt {

template <typename T>
__global__ void __launch_bounds__(SSQ_THREADS)
ssqg_reassign_bins(const cplx<T>* __restrict__ W, const cplx<T>* __restrict__ dW, long ld, long ncols, int nrows,
                   const T* __restrict__ w, double g2, double l0, double inv_dv, int nf, cplx<T>* S, long ldt,
                   short* __restrict__ bins, long ldb) {
  const long n = long(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n >= ncols) return;
  ssq_column<T, true>(W + n, dW + n, ld, nrows, w, g2, l0, inv_dv, nf, S + n, ldt, bins + n, ldb);
}

constexpr int SSQG_THREADS = 128, SSQG_STRETCH = 8;
template <typename T>
__global__ void __launch_bounds__(SSQG_THREADS)
ssqg_gather(const cplx<T>* __restrict__ gT, long ldt, int nf, const short* __restrict__ bins, long ldb,
            const T* __restrict__ w, int nrows, long ncols, cplx<T>* __restrict__ G, long ldg, int stretch0) {
#pragma clang fp contract(off)
  const long n = long(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n >= ncols) return;
  constexpr int R = SSQG_STRETCH;
  const long j0 = (long(stretch0) + long(blockIdx.y)) * R;
  int k[R];
#pragma unroll
  for (int u = 0; u < R; ++u) k[u] = j0 + u < nrows ? int(__builtin_nontemporal_load(bins + (j0 + u) * ldb + n)) : -1;
  int cur = -1;
  cplx<T> cell = mk<T>(T(0), T(0));
#pragma unroll
  for (int u = 0; u < R; ++u) {
    if (j0 + u >= nrows) break;
    cplx<T> g = mk<T>(T(0), T(0));
    if (k[u] >= 0 && k[u] < nf) {
      if (k[u] != cur) {
        cur = k[u];
        cell = gT[long(cur) * ldt + n];
      }
      const T wj = w[j0 + u];
      g = mk<T>(wj * cell.x, wj * cell.y);
    }
    G[(j0 + u) * ldg + n] = g;
  }
}

}  // namespace cwt
