// cwt_kernels_select.hpp -- exact order statistics of every row of a matrix (cwt_row_order_statistics): out[j, i] = the ranks[i]-th
// smallest of v[j, n], n < ncols, with v = A[j, n] (a real matrix) or v = fma(re, re, im im) of the complex entry (abs2_fma: the ONE
// place that forms it, shared by every pass here and by cwt_kernels_shrink.hpp, so that no two passes see two roundings of an entry).
//
// ORDER.  A value is ordered by its key, the usual order-preserving map of the IEEE bit pattern to an unsigned integer of the same
// width (negative: all bits flipped; else: the sign bit set); every NaN, whatever its sign bit, takes the largest key and so sorts
// after +inf.  -0.0 sorts directly below +0.0.  The result is the value whose key the selection ends on: a value of the row itself
// (a canonical quiet NaN where the rank lies beyond the row's non-NaN count).
//
// METHOD.  Most-significant-digit radix select on the keys, digits of SEL_DIGIT = 11 bits (fp64: 11 11 11 11 11 9, fp32: 11 11 10),
// all rows and all ranks of the call side by side, without a look from the host.  Per (row, rank) a SelState: the resolved leading
// bits of the key (prefix), how many, the rank k among the candidates (the entries whose key starts with the prefix) and their
// count.  A ROUND is two launches:
//   sel_hist   grid (pieces of a row, rows).  Reads its piece of the row once and, per rank of the row,
//                ACTIVE   counts the next digit of every candidate: LDS histogram (integer atomicAdd; a thread first merges the run of
//                         equal digits it meets -- the first digit of continuous data is nearly one value), then the non-zero bins
//                         added into the row's global histogram (integer atomicAdd: the counts are exact whatever the order)
//                COMPACT  appends every candidate's key to the rank's buffer of SEL_CAP keys (a counter per rank; the ORDER in the
//                         buffer depends on the schedule, the SET does not, and nothing downstream depends on the order)
//              Ranks of a row whose states agree (same prefix, same status) share one histogram / buffer -- that of the first such
//              rank, the LEADER: the two middle ranks of a median cost one rank's work until their prefixes part.  A workgroup whose
//              row has every rank DONE returns at once.
//   sel_pick   one workgroup per row, rank after rank.
//                ACTIVE   finds the digit that holds k (three-level sum over the 2048 bins), appends it to the prefix, k -= the count
//                         below it; all bits resolved: DONE, out = the value of the key (the row of identical values ends here, after
//                         key width / digit width rounds); else at most SEL_CAP candidates left: COMPACT
//                COMPACT  (its buffer was filled by this round's sel_hist) takes the keys into LDS and runs the remaining digits
//                         there; DONE
//              and clears the histograms it used.
// A row of at most SEL_CAP columns starts COMPACT: one round.  Longer rows: continuous data narrows to <= SEL_CAP candidates in two
// digits (the first digit of an fp64 key is sign and exponent only), so the normal case is two counting reads and the compaction
// read; the launches of the later rounds find every rank DONE.  The worst case is key width / digit width reads.
//
// NAMES.  As in cwt_kernels_hop.hpp / _pool.hpp / _ssq.hpp: the kernels are called sel_*, not k_*, because the coverage gate of
// tests/test_emu_schedules.py lists the kernels named k_*; the gate for these is in tests/test_shrink_schedules_emulated.py.
#pragma once
#include <hip/hip_runtime.h>

#include <limits>

#include "cwt_types.hpp"

namespace cwt {

// |w|^2 as ONE fused multiply-add on top of one rounded product
__device__ __forceinline__ double abs2_fma(const cplx<double> w) { return __builtin_fma(w.x, w.x, w.y * w.y); }
__device__ __forceinline__ float abs2_fma(const cplx<float> w) { return __builtin_fmaf(w.x, w.x, w.y * w.y); }

constexpr int SEL_DIGIT = 11, SEL_BINS = 1 << SEL_DIGIT, SEL_THREADS = 256, SEL_CAP = 2048, SEL_MAX_RANKS = 8, SEL_INFLIGHT = 4;
enum { SEL_ACTIVE = 0, SEL_COMPACT = 1, SEL_DONE = 2 };

struct SelState {
  unsigned long long prefix;   // the resolved leading bits of the key, in place; the bits below them 0
  unsigned long long k;        // the wanted rank among the candidates
  unsigned long long cand;     // candidates: entries of the row whose key starts with the prefix
  int resolved;                // leading bits resolved
  int status;                  // SEL_ACTIVE | SEL_COMPACT | SEL_DONE
  unsigned fill;               // keys appended to the rank's buffer so far
  unsigned pad;
};
struct SelRanks { long long r[SEL_MAX_RANKS]; };

template <typename T> struct sel_traits;
template <> struct sel_traits<float> { typedef unsigned key; static constexpr int bits = 32; };
template <> struct sel_traits<double> { typedef unsigned long long key; static constexpr int bits = 64; };
template <typename T> constexpr int sel_rounds() { return (sel_traits<T>::bits + SEL_DIGIT - 1) / SEL_DIGIT; }

template <typename T>
__device__ __forceinline__ typename sel_traits<T>::key sel_to_key(const T v) {
  typedef typename sel_traits<T>::key K;
  constexpr K sign = K(1) << (sel_traits<T>::bits - 1);
  if (v != v) return ~K(0);                                            // every NaN: the largest key (no other value maps to it)
  K b;
  __builtin_memcpy(&b, &v, sizeof(K));
  return (b & sign) ? K(~b) : K(b | sign);
}

template <typename T>
__device__ __forceinline__ T sel_from_key(const typename sel_traits<T>::key k) {
  typedef typename sel_traits<T>::key K;
  constexpr K sign = K(1) << (sel_traits<T>::bits - 1);
  if (k == ~K(0)) return std::numeric_limits<T>::quiet_NaN();
  const K b = (k & sign) ? K(k ^ sign) : K(~k);
  T v;
  __builtin_memcpy(&v, &b, sizeof(K));
  return v;
}

// the value of entry i of a matrix of reals, or of complex numbers (CPLX); read once per pass: non-temporal
template <typename T, bool CPLX>
__device__ __forceinline__ T sel_value(const void* A, const long i) {
  if (CPLX) {
    typedef T vec2 __attribute__((vector_size(2 * sizeof(T))));
    const vec2 w = __builtin_nontemporal_load(static_cast<const vec2*>(A) + i);
    return abs2_fma(mk<T>(w[0], w[1]));
  }
  return __builtin_nontemporal_load(static_cast<const T*>(A) + i);
}

// key starts with the `resolved` leading bits of prefix
template <typename K>
__device__ __forceinline__ bool sel_match(const K key, const K prefix, const int resolved) {
  return resolved == 0 || ((key ^ prefix) >> (int(sizeof(K)) * 8 - resolved)) == 0;
}
// the digit after the `resolved` leading bits (the last digit of a key is narrower: it takes the low bits that are left)
template <typename K>
__device__ __forceinline__ int sel_width(const int resolved) {
  const int left = int(sizeof(K)) * 8 - resolved;
  return left < SEL_DIGIT ? left : SEL_DIGIT;
}
template <typename K>
__device__ __forceinline__ unsigned sel_digit(const K key, const int resolved) {
  const int w = sel_width<K>(resolved);
  return unsigned(key >> (int(sizeof(K)) * 8 - resolved - w)) & ((1u << w) - 1u);
}

// the leader of rank r of a row: the first rank whose state agrees (DONE ranks have none: -1)
__device__ __forceinline__ int sel_leader(const SelState* s, const int r) {
  if (s[r].status == SEL_DONE) return -1;
  for (int q = 0; q < r; ++q)
    if (s[q].status == s[r].status && s[q].resolved == s[r].resolved && s[q].prefix == s[r].prefix) return q;
  return r;
}

template <typename T>                                        // (T: instantiated beside the launches of its precision; unused)
__global__ void sel_init(SelState* st, const int nrows, const int nranks, const SelRanks ranks, const long ncols) {
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= nrows * nranks) return;
  SelState s;
  s.prefix = 0;
  s.k = (unsigned long long)ranks.r[i % nranks];
  s.cand = (unsigned long long)ncols;
  s.resolved = 0;
  s.status = ncols <= SEL_CAP ? SEL_COMPACT : SEL_ACTIVE;
  s.fill = 0;
  s.pad = 0;
  st[i] = s;
}

// st: rows x nranks states; hist: rows x nranks x SEL_BINS counts (zero on entry); cbuf: rows x nranks x SEL_CAP keys.
// LDS: nranks x SEL_BINS counts.
template <typename T, bool CPLX>
__global__ void __launch_bounds__(SEL_THREADS)
sel_hist(const void* __restrict__ A, const long ld, const long ncols, const int nranks, SelState* st, unsigned* hist,
         typename sel_traits<T>::key* cbuf) {
  typedef typename sel_traits<T>::key K;
  HIP_DYNAMIC_SHARED(double2, lds_raw)
  unsigned* lh = reinterpret_cast<unsigned*>(lds_raw);
  const long row = blockIdx.y;
  SelState* s = st + row * nranks;
  // the ranks this read serves: the leaders of the row
  K prefix[SEL_MAX_RANKS];
  int resolved[SEL_MAX_RANKS], mode[SEL_MAX_RANKS];          // mode: -1 = nothing to do for this rank
  bool any = false, counting = false;
#pragma unroll
  for (int r = 0; r < SEL_MAX_RANKS; ++r) {
    mode[r] = -1;
    prefix[r] = 0;
    resolved[r] = 0;
    if (r < nranks && sel_leader(s, r) == r) {
      mode[r] = s[r].status;
      prefix[r] = K(s[r].prefix);
      resolved[r] = s[r].resolved;
      any = true;
      counting = counting || mode[r] == SEL_ACTIVE;
    }
  }
  if (!any) return;                                          // (uniform over the workgroup: before any barrier)
  const int tid = int(threadIdx.x);
  if (counting) {
    for (int b = tid; b < nranks * SEL_BINS; b += SEL_THREADS) lh[b] = 0;
    __syncthreads();
  }
  // this workgroup's piece of the row: whole strides of the workgroup
  const long per = ((ncols + gridDim.x - 1) / gridDim.x + SEL_THREADS - 1) / SEL_THREADS * SEL_THREADS;
  const long c0 = long(blockIdx.x) * per, c1 = c0 + per < ncols ? c0 + per : ncols;
  int run_digit[SEL_MAX_RANKS];
  unsigned run[SEL_MAX_RANKS];
#pragma unroll
  for (int r = 0; r < SEL_MAX_RANKS; ++r) { run_digit[r] = 0; run[r] = 0; }
  for (long n0 = c0 + tid; n0 < c1; n0 += long(SEL_INFLIGHT) * SEL_THREADS) {
    T v[SEL_INFLIGHT];
#pragma unroll
    for (int u = 0; u < SEL_INFLIGHT; ++u) {
      const long n = n0 + long(u) * SEL_THREADS;
      v[u] = n < c1 ? sel_value<T, CPLX>(A, row * ld + n) : T(0);
    }
#pragma unroll
    for (int u = 0; u < SEL_INFLIGHT; ++u) {
      if (n0 + long(u) * SEL_THREADS >= c1) continue;
      const K key = sel_to_key<T>(v[u]);
#pragma unroll
      for (int r = 0; r < SEL_MAX_RANKS; ++r) {
        if (mode[r] < 0 || !sel_match<K>(key, prefix[r], resolved[r])) continue;
        if (mode[r] == SEL_ACTIVE) {
          const int d = int(sel_digit<K>(key, resolved[r]));
          if (d != run_digit[r]) {
            if (run[r]) atomicAdd(&lh[r * SEL_BINS + run_digit[r]], run[r]);
            run_digit[r] = d;
            run[r] = 0;
          }
          ++run[r];
        } else {
          const unsigned at = atomicAdd(&s[r].fill, 1u);
          if (at < unsigned(SEL_CAP)) cbuf[(row * nranks + r) * SEL_CAP + at] = key;      // (always: the counts are exact)
        }
      }
    }
  }
  if (!counting) return;
#pragma unroll
  for (int r = 0; r < SEL_MAX_RANKS; ++r)
    if (mode[r] == SEL_ACTIVE && run[r]) atomicAdd(&lh[r * SEL_BINS + run_digit[r]], run[r]);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SEL_MAX_RANKS; ++r) {
    if (mode[r] != SEL_ACTIVE) continue;
    for (int b = tid; b < SEL_BINS; b += SEL_THREADS) {
      const unsigned c = lh[r * SEL_BINS + b];
      if (c) atomicAdd(&hist[(row * nranks + r) * SEL_BINS + b], c);
    }
  }
}

// The digit of the SEL_BINS counts h (global or LDS) that holds rank k: thread 0 leaves it in res[0] and the count below it in
// below[0].  part: SEL_THREADS + 16 counts of LDS.  Ends on a barrier (res, below readable; part free again).
__device__ __forceinline__ void sel_find_digit(const unsigned* h, const unsigned long long k, unsigned* part, unsigned* res,
                                               unsigned long long* below) {
  constexpr int PER = SEL_BINS / SEL_THREADS, GROUP = 16;
  const int tid = int(threadIdx.x);
  unsigned sum = 0;
  for (int b = 0; b < PER; ++b) sum += h[tid * PER + b];
  part[tid] = sum;
  __syncthreads();
  if (tid < SEL_THREADS / GROUP) {
    unsigned g = 0;
    for (int i = 0; i < GROUP; ++i) g += part[tid * GROUP + i];
    part[SEL_THREADS + tid] = g;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long acc = 0;
    int g = 0, t, b;
    while (g < SEL_THREADS / GROUP - 1 && acc + part[SEL_THREADS + g] <= k) acc += part[SEL_THREADS + g++];
    t = g * GROUP;
    while (t < g * GROUP + GROUP - 1 && acc + part[t] <= k) acc += part[t++];
    b = t * PER;
    while (b < t * PER + PER - 1 && acc + h[b] <= k) acc += h[b++];
    res[0] = unsigned(b);
    below[0] = acc;
  }
  __syncthreads();
}

template <typename T>
constexpr size_t sel_pick_lds() {
  return SEL_CAP * sizeof(typename sel_traits<T>::key) + sizeof(unsigned long long) + (SEL_BINS + SEL_THREADS + 16 + 2) * sizeof(unsigned);
}

template <typename T>
__global__ void __launch_bounds__(SEL_THREADS)
sel_pick(const int nranks, SelState* st, unsigned* hist, const typename sel_traits<T>::key* cbuf, T* out, const long ldo) {
  typedef typename sel_traits<T>::key K;
  constexpr int BITS = sel_traits<T>::bits;
  HIP_DYNAMIC_SHARED(double2, lds_raw)                       // sel_pick_lds<T>() bytes: keys | below | lh | part | res
  K* keys = reinterpret_cast<K*>(lds_raw);
  unsigned long long* below = reinterpret_cast<unsigned long long*>(keys + SEL_CAP);
  unsigned* lh = reinterpret_cast<unsigned*>(below + 1);
  unsigned* part = lh + SEL_BINS;
  unsigned* res = part + SEL_THREADS + 16;
  const long row = blockIdx.x;
  const int tid = int(threadIdx.x);
  SelState* s = st + row * nranks;
  // the row's states as the round's sel_hist saw them (a leader's state changes before its followers are served)
  SelState old[SEL_MAX_RANKS];
  int lead[SEL_MAX_RANKS];
#pragma unroll
  for (int r = 0; r < SEL_MAX_RANKS; ++r) {
    lead[r] = -1;
    if (r < nranks) { old[r] = s[r]; lead[r] = sel_leader(s, r); }
  }
  __syncthreads();                                           // every thread has read the states before thread 0 writes one
#pragma unroll
  for (int r = 0; r < SEL_MAX_RANKS; ++r) {
    if (r >= nranks || lead[r] < 0) continue;                // (uniform over the workgroup)
    K prefix = K(old[r].prefix);
    unsigned long long k = old[r].k, cand = old[r].cand;
    int resolved = old[r].resolved, status = old[r].status;
    if (status == SEL_ACTIVE) {
      const unsigned* h = hist + (row * nranks + lead[r]) * SEL_BINS;
      sel_find_digit(h, k, part, res, below);
      const int w = sel_width<K>(resolved);
      prefix |= K(res[0]) << (BITS - resolved - w);
      k -= below[0];
      cand = h[res[0]];
      resolved += w;
      status = resolved == BITS ? SEL_DONE : cand <= (unsigned long long)SEL_CAP ? SEL_COMPACT : SEL_ACTIVE;
    } else {
      const int n = int(old[lead[r]].fill < unsigned(SEL_CAP) ? old[lead[r]].fill : unsigned(SEL_CAP));
      const K* src = cbuf + (row * nranks + lead[r]) * SEL_CAP;
      for (int i = tid; i < n; i += SEL_THREADS) keys[i] = src[i];
      while (resolved < BITS) {
        for (int b = tid; b < SEL_BINS; b += SEL_THREADS) lh[b] = 0;
        __syncthreads();                                     // (also: keys is loaded)
        for (int i = tid; i < n; i += SEL_THREADS)
          if (sel_match<K>(keys[i], prefix, resolved)) atomicAdd(&lh[sel_digit<K>(keys[i], resolved)], 1u);
        __syncthreads();
        sel_find_digit(lh, k, part, res, below);
        const int w = sel_width<K>(resolved);
        prefix |= K(res[0]) << (BITS - resolved - w);
        k -= below[0];
        cand = lh[res[0]];
        resolved += w;
        __syncthreads();                                     // lh, res and below are read before the next digit rewrites them
      }
      status = SEL_DONE;
    }
    if (tid == 0) {
      SelState t;
      t.prefix = prefix; t.k = k; t.cand = cand; t.resolved = resolved; t.status = status; t.fill = 0; t.pad = 0;
      s[r] = t;
      if (status == SEL_DONE) out[row * ldo + r] = sel_from_key<T>(prefix);
    }
    __syncthreads();                                         // keys / res / below are free for the next rank
  }
  // the histograms of this round, cleared for the next
#pragma unroll
  for (int r = 0; r < SEL_MAX_RANKS; ++r)
    if (r < nranks && lead[r] == r && old[r].status == SEL_ACTIVE)
      for (int b = tid; b < SEL_BINS; b += SEL_THREADS) hist[(row * nranks + r) * SEL_BINS + b] = 0;
}

}  // namespace cwt
