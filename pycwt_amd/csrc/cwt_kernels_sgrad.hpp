// cwt_kernels_sgrad.hpp -- gradients of the transform with respect to its scales and to Morlet's f0 (cwt_adjoint_rows_scales).
//
// The filter of row j is F_j[k] = amp_j g(a_j k) with amp_j ~ sqrt(s_j) and a_j = 2 pi s_j / (N dt) (RowDesc, filter_value), so its
// derivative with respect to ln s_j -- and, for Morlet, to f0 -- is the filter itself times a real polynomial in f = a_j k:
//
//     mother       g(f)                      q(f) = (dF/d ln s) / F      r(f) = (dF/d f0) / F
//     Morlet(f0)   e^{-(f - f0)^2 / 2}       1/2 - f (f - f0)            f - f0
//     Paul(m)      f^m e^{-f},  f > 0        1/2 + m - f                 0
//     DOG(m)       f^m e^{-f^2 / 2}          1/2 + m - f^2               0
//
// With L = Re sum conj(G) W and term_j[k] = (F_j[k] / N) conj(DFT_N(pad G_j)[k]) -- what k_adj_accum adds into the accumulator --
//     dL/d ln s_j = Re sum_{k in band_j} q(a_j k) term_j[k] xhat[k],      dL/d f0 = sum_j Re sum_k r(a_j k) term_j[k] xhat[k]:
// one reduction over each row's band, on the spectra of G that the general path of the adjoint holds anyway (spec_j[k mod M] for
// the decimated adjoint, as hop_adj_accum reads them).  The support of a row is the forward's (bins below the plan's accuracy
// target of the filter's peak are dropped, in value and in gradient alike).
//
// NAMES.  sgrad_*, not k_*, for the reason cwt_kernels_hop.hpp gives: the coverage gate of tests/test_emu_schedules.py lists the
// __global__ functions named k_* and demands that its own cases launch each of them.  The same gate for these kernels is in
// tests/test_scale_grad_emulated.py (the set of names read from this file).
//
// Kernels (T = float | double):
//   sgrad_partial  grid (slices of the band, rows of the chunk) x 256 threads: the two sums over one slice of a row's band
//   sgrad_sum      one thread per row: the slices, then the signals, in double
//
// ONE ORDER OF SUMMATION.  A slice is SGRAD_SLICE consecutive band positions i (signed bin k_lo + i); thread t of the workgroup sums
// the positions t, t + 256, ... of the slice in ascending order, the workgroup adds its threads in a fixed binary tree through
// LDS (workgroup barriers, no shuffles), sgrad_sum adds a row's slices in ascending order and then the signals in ascending
// order.  No atomics.  The bits of a row's result depend on (N, M, the row's band) and the order of the signals only -- not on the
// chunk of rows the launch covers, on the rows around it or on the stream.
#pragma once
#include <hip/hip_runtime.h>

#include "cwt_types.hpp"
#include "fft_engine.hpp"

namespace cwt {

constexpr int SGRAD_THREADS = 256;
constexpr int SGRAD_SLICE = 2048;      // band positions per workgroup of sgrad_partial: 8 per thread

__host__ __device__ inline int sgrad_slices(int nband) { return (nband + SGRAD_SLICE - 1) / SGRAD_SLICE; }

// sgrad_partial: partial[((signal * nrows + row_first + blockIdx.y) * nslices + blockIdx.x) * 2 + {0, 1}] = the q and the r sum of
// slice blockIdx.x of row blockIdx.y of the chunk.  spec: the chunk's spectra of G (cnt x M, M = N without hop), xhat: the
// signal's N-point spectrum, `partial` already offset to the signal.  Workgroups beyond the row's band leave at once.
template <typename T>
__global__ void __launch_bounds__(SGRAD_THREADS)
sgrad_partial(const cplx<T>* __restrict__ spec, const cplx<T>* __restrict__ xhat, const RowDesc* __restrict__ rows, Mother mo,
              int logN, int logM, int row_first, int nslices, T* __restrict__ partial) {
  HIP_DYNAMIC_SHARED(double2, lds_raw)
  cplx<T>* red = reinterpret_cast<cplx<T>*>(lds_raw);             // 256 x (q sum, r sum)
  const RowDesc rd = rows[blockIdx.y];
  const int i0 = int(blockIdx.x) * SGRAD_SLICE;
  if (i0 >= rd.nband) return;                                     // (uniform: the whole workgroup)
  const int t = int(threadIdx.x), nmask = (1 << logN) - 1, mmask = (1 << logM) - 1;
  const int iend = rd.nband - i0 < SGRAD_SLICE ? rd.nband : i0 + SGRAD_SLICE;
  const cplx<T>* sp = spec + (long(blockIdx.y) << logM);
  T sq = T(0), sr = T(0);
  for (int i = i0 + t; i < iend; i += SGRAD_THREADS) {
    const int ks = rd.k_lo + i, k = ks & nmask;
    const cplx<T> x = sp[k & mmask];
    const cplx<T> v = filter_value<T>(mk<T>(x.x, -x.y), rd, mo, ks);      // term_j[k], as k_adj_accum forms it
    const cplx<T> xh = xhat[k];
    const T re = v.x * xh.x - v.y * xh.y;
    const T f = T(rd.a) * T(ks);
    T q, r = T(0);
    if (mo.kind == MOTHER_MORLET) {
      r = f - T(mo.p);
      q = T(0.5) - f * r;
    } else if (mo.kind == MOTHER_PAUL) {
      q = T(0.5) + T(mo.m) - f;
    } else {
      q = T(0.5) + T(mo.m) - f * f;
    }
    sq += q * re;
    sr += r * re;
  }
  red[t] = mk<T>(sq, sr);
  __syncthreads();
  for (int s = 1; s < SGRAD_THREADS; s <<= 1) {
    if ((t & (2 * s - 1)) == 0) { const cplx<T> a = red[t], b = red[t + s]; red[t] = mk<T>(a.x + b.x, a.y + b.y); }
    __syncthreads();
  }
  if (t == 0) {
    T* o = partial + (long(row_first + int(blockIdx.y)) * nslices + long(blockIdx.x)) * 2;
    o[0] = red[0].x;
    o[1] = red[0].y;
  }
}

// sgrad_sum: out[row][{0, 1}] (+)= sum over the signals (ascending) of the sum over the row's slices (ascending), in double.
// partial: nbatch x nrows x nslices x 2.  grid = nrows / 256.
template <typename T>
__global__ void __launch_bounds__(SGRAD_THREADS)
sgrad_sum(const T* __restrict__ partial, const RowDesc* __restrict__ rows, int nrows, int nbatch, int nslices, int accumulate,
          double* __restrict__ out) {
  const int j = int(blockIdx.x) * SGRAD_THREADS + int(threadIdx.x);
  if (j >= nrows) return;
  const int ns = sgrad_slices(rows[j].nband);
  double tq = 0.0, tr = 0.0;
  for (int b = 0; b < nbatch; ++b) {
    const T* pp = partial + (long(b) * nrows + j) * long(nslices) * 2;
    double q = 0.0, r = 0.0;
    for (int s = 0; s < ns; ++s) { q += double(pp[2 * s]); r += double(pp[2 * s + 1]); }
    tq = b ? tq + q : q;
    tr = b ? tr + r : r;
  }
  out[2 * j] = accumulate ? out[2 * j] + tq : tq;
  out[2 * j + 1] = accumulate ? out[2 * j + 1] + tr : tr;
}

}  // namespace cwt
