// abi.hip -- the exported C functions of libcwt_hip.so (include/cwt_hip.h has the contract and the reference lines each entry
// point stands in for).  Argument checks, the row-table cache lookups, dispatch on the plan's precision into the launches of
// launch_impl.hpp (compiled in launch_f64.hip / launch_f32.hip); the few small kernels launched directly from here
// (spectrum range, cross spectrum, time mean, coherence histogram) are instantiated in this file.
#include "launch_impl.hpp"

using namespace cwtd;
using namespace cwt;

namespace {
// Calls f(T()) with T = the plan's element type (double or float): each launch is written once.
template <class F>
int by_precision(const cwt_plan* p, F&& f) {
  if (p->prec == 64) return f(double());
  return f(float());
}

// What a table-building entry point asks for; a field left at its default is not used by that entry point.  The rows come
// from scales (row b * nrows + j of a batch of nbatch signals at scales[j]; wavelet.py:94, 102), from explicit filter
// parameters a / amp_re / amp_im, or from a filter bank of the caller's (tab_klo / tab_nband, mother = MOTHER_TABLE).
struct TableCall {
  int kind = -1;                          // cache key kind: 0 ... 3, one per kind of entry point (none shares another's tables);
  std::vector<double> head;               // -1 = never cached; head: the key's values after the kind
  int nbatch = 1, nrows = 0;              // signals, rows per signal
  const double* scales = nullptr;
  double dt = 0;
  int64_t ldw = 0, ncols = 0;             // the output W
  RowRequest rows;                        // (its nrows, and a / amp_* of a call by scales, are filled in by prepare_table)
};

// Makes the row table of call c current: the cached one of the same call, or a new one.  A new table gets the side tables
// of whatever forms it contains: decided here from the table alone, never by the entry point (commit 026261b).
int prepare_table(cwt_plan* p, const TableCall& c) {
  const int total = c.nbatch * c.nrows;
  if (total < 1 || total > p->max_rows) return fail(CWT_EINVAL, "nrows must be in [1, max_rows]");
  if (c.ncols < 1 || c.ncols > p->N || c.ldw < c.ncols) return fail(CWT_EINVAL, "need 1 <= ncols <= nfft and ldw >= ncols");
  if (c.rows.spec_ld != 0 && c.rows.spec_ld < p->N) return fail(CWT_EINVAL, "spec_ld must be 0 (shared) or >= nfft");
  if (c.scales && (!(c.dt > 0) || !std::isfinite(c.dt))) return fail(CWT_EINVAL, "dt must be positive");
  std::vector<double> key;                        // [kind, head..., the rows' arguments]
  if (c.kind >= 0) {
    key = c.scales ? call_key(c.kind, {}, {{c.scales, c.nrows}})
                   : call_key(c.kind, {}, {{c.rows.a, total}, {c.rows.amp_re, total}, {c.rows.amp_im, total}});
    key.insert(key.begin() + 1, c.head.begin(), c.head.end());
  }
  if (!select_table(p, key)) {
    double cre = 0, cim = 0;
    // the mother id and order of every call but a filter bank of the caller's (whose id is MOTHER_TABLE)
    int rc = c.rows.tab_klo ? CWT_OK : mother_constant(c.rows.mother, c.rows.param, &cre, &cim);
    if (rc) return rc;
    RowRequest r = c.rows;                        // (a / amp_*: the call's own, or made here)
    r.nrows = total;
    std::vector<double> va, vr, vi;
    if (c.scales) {
      const double w1 = 2.0 * 3.14159265358979323846 * (1.0 / (double(p->N) * c.dt));  // ftfreqs[1], wavelet.py:94
      va.resize(total); vr.resize(total); vi.resize(total);
      for (int j = 0; j < total; ++j) {
        const double s = c.scales[j % c.nrows];
        if (!(s > 0) || !std::isfinite(s)) return fail(CWT_EINVAL, "scales must be positive and finite");
        va[j] = s * w1;
        const double norm = std::sqrt(s * w1 * double(p->N));                         // wavelet.py:102
        vr[j] = norm * cre;
        vi[j] = norm * cim;
      }
      r.a = va.data(); r.amp_re = vr.data(); r.amp_im = vi.data();
    } else if (!r.a) {                                // a filter bank of the caller's holds the amplitudes
      va.assign(total, 1.0);
      vi.assign(total, 0.0);
      r.a = r.amp_re = va.data(); r.amp_im = vi.data();
    }
    rc = build_row_table(p, r);
    if (!rc) rc = upload_row_table(p, key);
    const Mother mo = mother_of(r.mother, r.param);
    if (!rc) rc = by_precision(p, [&](auto t) {
      using T = decltype(t);
      int r = p->rt->n_ols ? fill_ols_tables<T>(p, mo) : CWT_OK;
      if (!r && p->rt->n_aols) r = fill_aols_tables<T>(p, mo);
      if (!r && p->rt->poly_rtab_elems) r = fill_poly_tables<T>(p);
      return r;
    });
    if (rc) { p->rt->key.clear(); return rc; }
  }
  set_split(p);
  return CWT_OK;
}

// The rows of a call by scales (every table-building entry point but cwt_filter_rows and cwt_transform_rows_table)
TableCall scale_rows(int mother, double param, double dt, const double* scales, int nrows, int64_t ldw, int64_t ncols) {
  TableCall c;
  c.rows.mother = mother; c.rows.param = param;
  c.dt = dt;
  c.scales = scales;
  c.nrows = nrows;
  c.ldw = ldw;
  c.ncols = ncols;
  return c;
}

// Row table of cwt_transform / cwt_transform_rows / cwt_plan_classify
int prepare_rows_table(cwt_plan* p, bool have_signal, int mother, double param, double dt, const double* scales,
                       int nrows, int64_t ldw, int64_t ncols) {
  TableCall c = scale_rows(mother, param, dt, scales, nrows, ldw, ncols);
  c.kind = 0;
  c.head = {p->tolerance, double(mother), param, dt, double(nrows), have_signal ? 1.0 : 0.0, double(ncols)};
  c.rows.ols_ncols = have_signal ? ncols : 0;
  c.rows.out_ncols = ncols;
  return prepare_table(p, c);
}

// Every row of the current row table, as a call of its own; power: the rows' power instead of W (all the call decides)
int queue_rows(cwt_plan* p, const void* xhat_dev, const Mother& mo, int nrows, void* W_dev, int64_t ldw, int64_t ncols,
               int power = 0) {
  Call call;
  call.power = power;
  DrainOnFailure drain(p);
  return drain.done(by_precision(p, [&](auto t) { return rows_impl<decltype(t)>(p, call, xhat_dev, mo, nrows, W_dev, ldw, ncols); }));
}

std::mutex g_pinned_mutex;
std::map<uintptr_t, size_t> g_pinned;

bool is_pinned(const void* ptr, size_t bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
  std::lock_guard<std::mutex> lock(g_pinned_mutex);
  auto it = g_pinned.upper_bound(a);
  if (it == g_pinned.begin()) return false;
  --it;
  return a >= it->first && a + bytes <= it->first + it->second;
}

// Cost model of one rank's step, microseconds at N = 2^20: per kernel class a fixed part (launch ramp and tail; for the
// overlap-save classes the block spectra of that tile size) + a per-row part.  Fitted to the per-class launch durations of
// bench.py on BASELINE configs 2 / 3 (profiles/r03_per_class.txt) and the per-rank runs of profiles/r03_shards.txt; the
// overlap-save, band-passed and polynomial terms of fp64 refitted (least squares) to the 15 per-rank runs of
// profiles/r04_shards.txt.
struct ShardCost { double fwd, tp_fixed, tp_row, k2048_fixed, k2048_row, ols_fixed, ols_row, olsh_fixed, olsh_row, nar_fixed, nar_row, nar_term,
                   aols_fixed, aols_row, poly_fixed, poly_row, poly_coef; };
constexpr ShardCost kShardCost64 = {30.0, 18.0, 9.8, 30.0, 6.1, 22.0, 3.25, 44.0, 3.2, 8.0, 2.85, 0.9, 38.0, 2.9, 12.5, 2.67, 2.7};
constexpr ShardCost kShardCost32 = {27.0, 14.0, 5.3, 8.0, 5.4, 28.0, 2.3, 20.0, 1.9, 4.0, 1.75, 0.55, 40.0, 2.3, 22.0, 1.4, 1.1};

// Estimated step time of a rank that owns rows [lo, hi) (codes as cwt_plan_row_classes reports them).  nscale = transform
// length / 2^20: per-row parts scale with it, per-launch parts do not; chunk = rows per two-pass launch pair.
double shard_cost(const int* codes, int lo, int hi, const ShardCost& c, double nscale, int chunk) {
  double total = 0;
  bool seen_tp = false, seen_big = false, seen_ols = false, seen_olsh = false, seen_nar = false, seen_aols = false, seen_poly = false;
  int n_tp = 0;
  for (int i = lo; i < hi; ++i) {
    const int kind = codes[i] / 10000, logk = (codes[i] / 100) % 100, terms = codes[i] % 100;
    if (kind == 3) { ++n_tp; if (!seen_tp) { seen_tp = true; total += c.tp_fixed; } total += c.tp_row * nscale; }
    else if (kind == 2) { if (!seen_big) { seen_big = true; total += c.k2048_fixed; } total += c.k2048_row * nscale; }
    else if (kind == 4) { if (!seen_ols) { seen_ols = true; total += c.ols_fixed; } total += c.ols_row * nscale; }
    else if (kind == 5) {
      // (round 6: the rows of the narrow block supports are the ones with the long halos -- less of every block kept, and those on
      // 8192-point blocks come in a second launch behind their own block spectra: +10 % [measured per rank, profiles/r06_shards.txt])
      if (!seen_olsh) { seen_olsh = true; total += c.olsh_fixed; }
      total += c.olsh_row * nscale * (logk <= 8 ? 1.10 : 1.0);
    }
    else if (kind == 7) {
      // stage 2 per row (a little more per degree) + the row's share of stage 1: (D + 1) K' coefficients, priced at the
      // measured 2.2 us (fp64) of a K' = 16384, D = 8 row (profiles/r04_shards.txt)
      if (!seen_poly) { seen_poly = true; total += c.poly_fixed; }
      // (round 6, per (K', degree) class, profiles/r06_sessions.txt session r: the rows slow down with K' -- more coefficient sets per
      // workgroup -- beyond what their share of stage 1 says: +5 % at K' = 1024, +12 % at 2048 / 4096, +10 % above)
      const double kprime = logk >= 13 ? 0.10 : logk >= 11 ? 0.12 : logk == 10 ? 0.05 : 0.0;
      total += c.poly_row * nscale * (1.0 + 0.015 * std::max(0, terms - 8) + kprime);
      total += c.poly_coef * double((terms + 1) << logk) / double(9 << 14);
    }
    else if (kind == 6) { if (!seen_aols) { seen_aols = true; total += c.aols_fixed * std::max(nscale, 0.5); } total += c.aols_row * nscale; }
    else {
      if (!seen_nar) { seen_nar = true; total += c.nar_fixed; }
      const double per = c.nar_row * nscale;
      total += per;
      if (kind == 1) {                      // longer transforms per residue, shorter store segments
        const int K = 1 << logk;
        total += per * (K >= 1024 ? 0.25 : K >= 512 ? 0.13 : K >= 32 ? 0.05 : -0.05);
        if (terms > 1) total += nscale * c.nar_term * (terms - 1);
      }
    }
  }
  if (n_tp > chunk) total += c.tp_fixed * ((n_tp - 1) / chunk);
  if (seen_tp || seen_big || seen_nar || seen_aols || seen_poly) total += c.fwd * std::max(nscale, 0.5);   // some row needs the spectrum
  return total;
}
}  // namespace

// =============================================================================================
// ---- hardware queues ---------------------------------------------------------------------------------------------------
// A long transform runs on four streams (the caller's + three side streams).  The runtime multiplexes ALL streams of the
// process onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default) in the order they were created; two of the plan's
// streams that land on ONE queue execute in submission order and the overlap the schedule was built for is gone [measured:
// fp32 Paul 0.600 -> 0.618 / 0.637 ms with one / two idle streams created before the plan, fp64 Morlet 0.935 -> 0.952;
// the config-3 blocks of a default bench run, whose plans come after a dozen others, 6-10 % slower than alone].  HIP has no
// query for a stream's queue, so the plan MEASURES it: a one-thread kernel on stream a waits (bounded: 200 us) for a flag that
// a one-thread kernel on stream b sets; submitted in that order, b can only get through if it sits on another queue.  A side
// stream that shares a queue with the caller's stream or with an earlier side stream is parked (kept alive, idle, so that the
// runtime's least-used-queue choice moves on) and replaced.  Once per plan and caller's stream, ~0.3 ms; only for transforms
// long enough to use the side streams.  Option "queue_probe" = 0 turns it off.
#if defined(CWT_HIP_EMULATED)
int cwtd::ensure_distinct_queues(cwt_plan*) { return CWT_OK; }     // (the CPU stand-in of the tests runs kernels in launch order)
#else
__global__ void k_queue_probe_wait(int* flag, int* seen, long long ticks) {
  const long long t0 = wall_clock64();                              // 100 MHz
  int s = 0, turns = 0;
  do {
    s = __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    if (!s) __builtin_amdgcn_s_sleep(16);                           // ~0.5 us
  } while (!s && wall_clock64() - t0 < ticks && ++turns < 20000);   // (the turn count bounds the wait whatever the clock does)
  *seen = s;
}
__global__ void k_queue_probe_set(int* flag) { __hip_atomic_store(flag, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }

// true: kernels of a and b run side by side (different hardware queues)
static int queues_differ(cwt_plan* p, hipStream_t a, hipStream_t b, bool* differ) {
  HIPCHECK(hipMemsetAsync(p->probe_dev, 0, 2 * sizeof(int), a));
  HIPCHECK(hipEventRecord(p->ev_probe, a));
  HIPCHECK(hipStreamWaitEvent(b, p->ev_probe, 0));
  hipLaunchKernelGGL(k_queue_probe_wait, dim3(1), dim3(1), 0, a, p->probe_dev, p->probe_dev + 1, 20000LL);
  hipLaunchKernelGGL(k_queue_probe_set, dim3(1), dim3(1), 0, b, p->probe_dev);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(a));
  HIPCHECK(hipStreamSynchronize(b));
  int h[2] = {0, 0};
  HIPCHECK(hipMemcpy(h, p->probe_dev, sizeof(h), hipMemcpyDeviceToHost));
  *differ = h[1] != 0;
  return CWT_OK;
}

int cwtd::ensure_distinct_queues(cwt_plan* p) {
  if (!p->queue_probe) return CWT_OK;
  // one probe per caller's stream (a caller that alternates between two streams does not pay 0.3 ms per call), remembered for
  // the last few; never while the caller's stream is being captured (the probe synchronises)
  for (hipStream_t s : p->probed_streams) if (s == p->stream) return CWT_OK;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(p->stream, &cap) != hipSuccess) (void)hipGetLastError();
  else if (cap != hipStreamCaptureStatusNone) return CWT_OK;
  if (!p->probe_dev && hipMalloc(reinterpret_cast<void**>(&p->probe_dev), 2 * sizeof(int)) != hipSuccess)
    return fail(CWT_ENOMEM, "device allocation failed");
  if (!p->ev_probe) HIPCHECK(hipEventCreateWithFlags(&p->ev_probe, hipEventDisableTiming));
  static const bool verbose = std::getenv("CWT_QUEUE_PROBE_VERBOSE") != nullptr;
  hipStream_t* mine[3] = {&p->side[1], &p->side[0], &p->side2};     // by the work they carry: overlap-save chain first
  hipStream_t fixed[4] = {p->stream, nullptr, nullptr, nullptr};
  bool replaced = false;
  for (int i = 0; i < 3; ++i) {
    for (int attempt = 0;; ++attempt) {
      bool ok = true;
      for (int j = 0; j <= i && ok; ++j) {
        const int rc = queues_differ(p, fixed[j], *mine[i], &ok);
        if (rc) return rc;
      }
      if (ok || attempt == 8 || p->spacers.size() >= 16) {          // (a busy GPU can make a probe time out: the parked streams are capped)
        if (verbose) std::fprintf(stderr, "[cwt] side stream %d: %s after %d replacement(s)\n", i, ok ? "own hardware queue" : "still shares a queue", attempt);
        break;
      }
      p->spacers.push_back(*mine[i]);                               // idle from here on; destroyed with the plan
      HIPCHECK(create_side_stream(mine[i]));
      ++p->queue_collisions;
      replaced = true;
    }
    fixed[i + 1] = *mine[i];
  }
  if (replaced) p->probed_streams.clear();                          // what was measured against the old side streams is stale
  if (p->probed_streams.size() >= 8) p->probed_streams.erase(p->probed_streams.begin());
  p->probed_streams.push_back(p->stream);
  p->queues_probed = true;
  p->probed_main = p->stream;
  return CWT_OK;
}
#endif


extern "C" {

const char* cwt_backend(void) { return CWT_BACKEND_NAME; }
const char* cwt_last_error(void) { return g_err.c_str(); }

int cwt_device_count(int* count) {
  if (!count) return fail(CWT_EINVAL, "count is NULL");
  *count = 0;
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) { *count = 0; return fail(CWT_ENODEV, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
  return CWT_OK;
}

// Events that only order streams (fork / join of the side streams): no timestamps.  CWT_EVENT_TIMING=1 creates them with
// timestamps as before round 6 (A/B of the hand-over latency).
static hipError_t order_event(hipEvent_t* e) {
  static const bool timing = [] { const char* v = std::getenv("CWT_EVENT_TIMING"); return v && std::atoi(v) != 0; }();
  return timing ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming);
}

int cwt_plan_create(cwt_plan** plan, int device, int64_t nfft, int precision, int max_rows) {
  if (!plan) return fail(CWT_EINVAL, "plan is NULL");
  *plan = nullptr;
  if (precision != 32 && precision != 64) return fail(CWT_EINVAL, "precision must be 32 or 64");
  if (nfft < 2 || nfft > (int64_t(1) << 24) || (nfft & (nfft - 1)))
    return fail(CWT_EINVAL, "nfft must be a power of two in [2, 2^24]");
  if (max_rows < 1) return fail(CWT_EINVAL, "max_rows must be >= 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(CWT_ENODEV, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(CWT_EINVAL, "device index out of range");
  HIPCHECK(hipSetDevice(device));
  cwt_plan* p = new cwt_plan();
  p->device = device;
  p->N = nfft;
  p->logN = ilog2(nfft);
  p->prec = precision;
  p->max_rows = max_rows;
  p->log_wg_points = precision == 64 ? 13 : 14;
  p->narrow_terms = precision == 64 ? 4 : 8;      // see the cost table in classify_row
  p->serial_rows = precision == 64 ? 2 : 0;       // [measured, round 6: c2 -1 %, fp64 Paul -5.7 %; fp32 DOG +-0, fp32 Paul +1.4 %]
  if (const char* e = std::getenv("CWT_TOLERANCE")) {   // default accuracy target of plans created from here on
    const double t = std::atof(e);
    if (t > 0 && t <= 1e-2) p->tolerance = t;
  }
  if (const char* e = std::getenv("CWT_QUEUE_PROBE")) p->queue_probe = std::atoi(e) != 0;   // (diagnostic: plans the caller does not create itself)
  int rc = by_precision(p, [&](auto t) {
    const int r = build_tables<decltype(t)>(p);
    return r ? r : set_func_attrs<decltype(t)>();
  });
  for (int i = 0; i < 2 && !rc; ++i) {
    if (create_side_stream(&p->side[i]) != hipSuccess ||
        order_event(&p->ev_a[i]) != hipSuccess || order_event(&p->ev_b[i]) != hipSuccess)
      rc = fail(CWT_EHIP, "cannot create side streams/events");
  }
  if (!rc && order_event(&p->ev_fork) != hipSuccess) rc = fail(CWT_EHIP, "cannot create event");
  if (!rc && order_event(&p->ev_ols) != hipSuccess) rc = fail(CWT_EHIP, "cannot create event");
  if (!rc && (create_side_stream(&p->side2) != hipSuccess || order_event(&p->ev_big) != hipSuccess))
    rc = fail(CWT_EHIP, "cannot create side streams/events");
  p->narrow_mix = precision == 64;
  p->ols_big = precision == 32;                   // measured: +2.5 % (fp32 DOG), +-0 at one GPU and -3 % per rank of 8 in fp64
  for (auto& t : p->slots) {
    // (+ max_rows / 3 + 4: pseudo-rows -- the mask of the k_aols rows, one per signal of a batch)
    if (!rc && hipMalloc(reinterpret_cast<void**>(&t.rows_dev), table_capacity(max_rows) * sizeof(RowDesc)) != hipSuccess)
      rc = fail(CWT_ENOMEM, "row table allocation failed");
    if (!rc && hipHostMalloc(reinterpret_cast<void**>(&t.rows_pinned), table_capacity(max_rows) * sizeof(RowDesc)) != hipSuccess)
      rc = fail(CWT_ENOMEM, "pinned row table allocation failed");
    if (!rc && hipEventCreate(&t.uploaded) != hipSuccess) rc = fail(CWT_EHIP, "cannot create event");
  }
  if (!rc && hipMalloc(&p->weights_dev, size_t(max_rows) * sizeof(double)) != hipSuccess)
    rc = fail(CWT_ENOMEM, "weights allocation failed");
  for (int i = 0; i < 2; ++i) {
    if (!rc && hipHostMalloc(&p->weights_pinned[i], size_t(max_rows) * sizeof(double)) != hipSuccess)
      rc = fail(CWT_ENOMEM, "pinned weights allocation failed");
    if (!rc && hipEventCreate(&p->weights_ev[i]) != hipSuccess) rc = fail(CWT_EHIP, "cannot create event");
  }
  if (rc) { cwt_plan_destroy(p); return rc; }
  *plan = p;
  return CWT_OK;
}

int cwt_plan_destroy(cwt_plan* p) {
  if (!p) return CWT_OK;
  (void)hipSetDevice(p->device);
  (void)hipStreamSynchronize(p->stream);
  for (int i = 0; i < 2; ++i) {
    if (p->side[i]) { (void)hipStreamSynchronize(p->side[i]); (void)hipStreamDestroy(p->side[i]); }
    if (p->ev_a[i]) (void)hipEventDestroy(p->ev_a[i]);
    if (p->ev_b[i]) (void)hipEventDestroy(p->ev_b[i]);
  }
  if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
  if (p->ev_ols) (void)hipEventDestroy(p->ev_ols);
  if (p->side2) { (void)hipStreamSynchronize(p->side2); (void)hipStreamDestroy(p->side2); }
  for (hipStream_t sp : p->spacers) (void)hipStreamDestroy(sp);
  if (p->ev_probe) (void)hipEventDestroy(p->ev_probe);
  if (p->probe_dev) (void)hipFree(p->probe_dev);
  if (p->ev_big) (void)hipEventDestroy(p->ev_big);
  for (auto& t : p->timed) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
  for (auto e : p->free_events) (void)hipEventDestroy(e);
  void* bufs[] = {p->tw_all, p->twn_lo, p->weights_dev, p->Z, p->xs, p->xm, p->xsa, p->pcoef, p->pband, p->range_dev, p->hx, p->hxhat, p->hW,
                  p->bs_khat[0], p->bs_khat[1], p->bs_a, p->bs_spec, p->bs_par, p->adj_spec, p->adj_acc, p->hop_z, p->sgrad_part, p->pool_s, p->sel, p->shgrad_part};
  for (void* b : bufs) if (b) (void)hipFree(b);
  for (auto& t : p->slots) {
    if (t.gt_dev) (void)hipFree(t.gt_dev);
    if (t.agt_dev) (void)hipFree(t.agt_dev);
    if (t.prt_dev) (void)hipFree(t.prt_dev);
    if (t.rows_dev) (void)hipFree(t.rows_dev);
    if (t.rows_pinned) (void)hipHostFree(t.rows_pinned);
    if (t.uploaded) (void)hipEventDestroy(t.uploaded);
    if (t.adj_dev) (void)hipFree(t.adj_dev);
    if (t.adj_pinned) (void)hipHostFree(t.adj_pinned);
    if (t.adj_uploaded) (void)hipEventDestroy(t.adj_uploaded);
    if (t.pool_dev) (void)hipFree(t.pool_dev);
    if (t.pool_pinned) (void)hipHostFree(t.pool_pinned);
    if (t.pool_uploaded) (void)hipEventDestroy(t.pool_uploaded);
  }
  if (p->hstage) (void)hipHostFree(p->hstage);
  for (int i = 0; i < 2; ++i) {
    if (p->weights_pinned[i]) (void)hipHostFree(p->weights_pinned[i]);
    if (p->weights_ev[i]) (void)hipEventDestroy(p->weights_ev[i]);
  }
  delete p;
  return CWT_OK;
}

int cwt_plan_set_stream(cwt_plan* p, void* hip_stream) {
  if (!p) return fail(CWT_EINVAL, "plan is NULL");
  HIPCHECK(hipStreamSynchronize(p->stream));
  p->stream = static_cast<hipStream_t>(hip_stream);
  return CWT_OK;
}

int cwt_plan_set_option(cwt_plan* p, const char* key, int64_t value) {
  if (!p || !key) return fail(CWT_EINVAL, "plan/key is NULL");
  const std::string k(key);
  auto pow2 = [](int64_t v) { return v > 0 && (v & (v - 1)) == 0; };
  const std::string left = " belonged to a measured-and-rejected variant or a diagnostic that has left the sources "
                           "(EXPERIMENTS.md has its measurements)";
  for (const char* gone : {"overlap", "pass_b_prefetch", "pass_b_small", "stamps", "ols_tile", "ols_fwd_real", "sched", "narrow_wave",
                           "graph", "serial_s1_once", "fft_aside_small", "aols_small_b", "coef_small", "ols_big4_min_halo",
                           "ols_big4_max_halo"})
    if (k == gone) return fail(CWT_EINVAL, "option " + k + left);
  // (values of kept options that selected such a variant fail the same way: an old script must not change schedule silently)
  if ((k == "serial_rows" && (value == 1 || value == 3)) || (k == "ols_big" && value == 2))
    return fail(CWT_EINVAL, k + " = " + std::to_string(value) + left);
  for (auto& t : p->slots) t.key.clear();   // the classification depends on the options
  struct Restore {   // a rejected geometry leaves every geometry-affecting field as it was
    cwt_plan* p; int lmax, wg, logk, nmax;
    ~Restore() {
      if (check_geometry(p) != CWT_OK) { p->loglmax = lmax; p->log_wg_points = wg; p->force_logk = logk; p->narrow_max_logk = nmax; }
    }
  } restore{p, p->loglmax, p->log_wg_points, p->force_logk, p->narrow_max_logk};
  if (k == "chunk_rows") { if (value < 0) return fail(CWT_EINVAL, "chunk_rows >= 0"); p->chunk_rows = int(value); }
  else if (k == "narrow") p->narrow = value != 0;
  else if (k == "narrow_max_k") { if (!pow2(value) || value < 16 || value > 4096) return fail(CWT_EINVAL, "narrow_max_k: power of two in [16,4096]"); p->narrow_max_logk = ilog2(value); }
  else if (k == "lmax") { if (!pow2(value) || value < 16 || value > 4096) return fail(CWT_EINVAL, "lmax: power of two in [16,4096]"); p->loglmax = ilog2(value); }
  else if (k == "wg_points") { if (!pow2(value) || value < 256 || value > 16384) return fail(CWT_EINVAL, "wg_points: power of two in [256,16384]"); p->log_wg_points = ilog2(value); }
  else if (k == "profile") p->profile = value != 0;
  else if (k == "ct") p->use_ct = value != 0;
  else if (k == "band_pass_a") p->band_pass_a = value != 0;
  else if (k == "overlap_narrow") p->overlap_narrow = value != 0;
  else if (k == "narrow_big") p->narrow_big = value != 0;
  else if (k == "narrow_mix") p->narrow_mix = value != 0;
  else if (k == "two_pass_logk") { if (value < 0 || value > 12) return fail(CWT_EINVAL, "two_pass_logk in [0,12] (0 = default)"); p->force_logk = int(value); }
  else if (k == "big_tiles") p->big_tiles = value != 0;
  else if (k == "narrow_small") p->narrow_small = value != 0;
  else if (k == "pass_a_small") p->pass_a_small = value != 0;
  else if (k == "narrow_terms") { if (value < 1 || value > 16) return fail(CWT_EINVAL, "narrow_terms in [1,16]"); p->narrow_terms = int(value); }
  else if (k == "ols") p->ols = value != 0;
  else if (k == "host_direct") p->host_direct = value != 0;
  else if (k == "aols") p->aols = value != 0;
  else if (k == "aols_zc") p->aols_zc = value != 0;
  else if (k == "aols_long") p->aols_long = value != 0;
  else if (k == "poly") p->poly = value != 0;
  else if (k == "poly_carrier") p->poly_carrier = value != 0;
  else if (k == "poly_cheb") p->poly_cheb = value != 0;
  else if (k == "poly_degree") { if (value < 2 || value > POLY_MAX_DEGREE) return fail(CWT_EINVAL, "poly_degree in [2, 24]"); p->poly_degree = int(value); }
  else if (k == "queue_probe") { p->queue_probe = value != 0; }
  else if (k == "adjoint_poly") p->adjoint_poly = value != 0;
  else if (k == "hop_fuse_terms") { if (value < 0 || value > 65536) return fail(CWT_EINVAL, "hop_fuse_terms in [0, 65536]"); p->hop_fuse_terms = int(value); }
  else if (k == "poly_chunk_mb") { if (value < 0 || value > 4096) return fail(CWT_EINVAL, "poly_chunk_mb in [0, 4096] (0 = one chunk)"); p->poly_chunk_mb = int(value); }
  else if (k == "poly_xcd") p->poly_xcd = value != 0;
  else if (k == "poly_max_logk") { if (value < 8 || value > 14) return fail(CWT_EINVAL, "poly_max_logk in [8, 14]"); p->poly_max_logk = int(value); }
  else if (k == "poly_min_logn") { if (value < 14 || value > 24) return fail(CWT_EINVAL, "poly_min_logn in [14, 24]"); p->poly_min_logn = int(value); }
  else if (k == "aols_min_rows") { if (value < 1 || value > 65536) return fail(CWT_EINVAL, "aols_min_rows >= 1"); p->aols_min_rows = int(value); }
  else if (k == "ols_side") p->ols_side = value != 0;
  else if (k == "ols_big") { if (value < 0 || value > 1) return fail(CWT_EINVAL, "ols_big: 0 or 1 (blocks of two tiles)"); p->ols_big = int(value); }
  else if (k == "ols_min_logn") { if (value < 15 || value > 24) return fail(CWT_EINVAL, "ols_min_logn in [15, 24]"); p->ols_min_logn = int(value); }
  else if (k == "ols_small_max_halo") { if (value < 0 || value > 1024 || (value & 63)) return fail(CWT_EINVAL, "ols_small_max_halo: multiple of 64 in [0, 1024]"); p->ols_small_max_halo = int(value); }
  else if (k == "ols_small_big") p->ols_small_big = value != 0;
  else if (k == "ols_big_min_halo") { if (value < 64 || value > 8192) return fail(CWT_EINVAL, "ols_big_min_halo in [64, 8192]"); p->ols_big_min_halo = int(value); }
  else if (k == "ols_early") p->ols_early = value != 0;
  else if (k == "serial_rows") { if (value != 0 && value != 2) return fail(CWT_EINVAL, "serial_rows: 0 or 2"); p->serial_rows = int(value); }
  else if (k == "ols_max_halo") { if (value < 0 || value > 4096 || (value & 63)) return fail(CWT_EINVAL, "ols_max_halo: multiple of 64 in [0, 4096]"); p->ols_max_halo = int(value); }
  else if (k == "ols_fwd_weight") { if (value < 0 || value > 1000) return fail(CWT_EINVAL, "ols_fwd_weight: percent of a row, 0..1000"); p->ols_fwd_weight = double(value) / 100.0; }
  else if (k == "tolerance_neglog10") {   // integer alias of cwt_plan_set_tolerance for option sweeps: 10^-value; 0 = default
    if (value < 0 || value > 18) return fail(CWT_EINVAL, "tolerance_neglog10 in [0, 18]");
    p->tolerance = value ? std::pow(10.0, -double(value)) : 0.0;
  }
  else if (k == "big_terms") { if (value < 1 || value > 8) return fail(CWT_EINVAL, "big_terms in [1,8]"); p->big_terms = int(value); }
  else return fail(CWT_EINVAL, "unknown option " + k);
  return check_geometry(p);
}

int cwt_plan_set_tolerance(cwt_plan* p, double rel_tol) {
  if (!p) return fail(CWT_EINVAL, "plan is NULL");
  if (!(rel_tol >= 0) || rel_tol > 1e-2) return fail(CWT_EINVAL, "tolerance must be in [0, 1e-2] (0 = default)");
  p->tolerance = rel_tol;     // (part of the row tables' cache key: a loop whose measured target flips between two values -- Monte-Carlo
  return CWT_OK;              // surrogates near a threshold of the automatic mode -- keeps both tables; a rebuild at N = 2^23 is 1.6 s)
}

int cwt_plan_set_auto_tolerance(cwt_plan* p, double target) {
  if (!p) return fail(CWT_EINVAL, "plan is NULL");
  if (!(target >= 0) || target > 1e-2) return fail(CWT_EINVAL, "target must be in [0, 1e-2] (0 = off)");
  p->auto_target = target;
  return CWT_OK;
}

int cwt_spectrum_range(cwt_plan* p, const void* xhat_dev, int64_t n, double* max_abs, double* rms_abs, double* floor_abs) {
  if (!p || !xhat_dev || !max_abs || !rms_abs || !floor_abs) return fail(CWT_EINVAL, "NULL argument");
  if (n < 1) return fail(CWT_EINVAL, "n must be >= 1");
  HIPCHECK(hipSetDevice(p->device));
  constexpr int kOut = SPECTRUM_SLOTS, kGroupsMax = 512;
  if (!p->range_dev && hipMalloc(reinterpret_cast<void**>(&p->range_dev), size_t(kGroupsMax + 1) * kOut * sizeof(double)) != hipSuccess)
    return fail(CWT_ENOMEM, "device allocation failed");
  // slices of at least 4096 bins, at most two workgroups per CU
  const int groups = int(std::max<int64_t>(1, std::min<int64_t>(kGroupsMax, n / 4096)));
  double* part = p->range_dev + kOut;
  by_precision(p, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_spectrum_range<T>), dim3(groups), dim3(256), (256 + kOut + 2) * sizeof(double), p->stream,
                       static_cast<const cplx<T>*>(xhat_dev), long(n), part);
    return CWT_OK;
  });
  hipLaunchKernelGGL((k_spectrum_fold<0>), dim3(1), dim3(192), 0, p->stream, part, groups, p->range_dev);
  HIPCHECK(hipGetLastError());
  double h[kOut] = {0};
  HIPCHECK(hipMemcpyAsync(h, p->range_dev, sizeof(h), hipMemcpyDeviceToHost, p->stream));
  HIPCHECK(hipStreamSynchronize(p->stream));
  *max_abs = std::sqrt(h[0]);
  *rms_abs = std::sqrt(h[1] / double(n));
  // The quietest stretch of the positive half at the resolution of a row's pass band: quarter-octave windows (single bins
  // below bin 4), each pooled with its two neighbours (3/4 octave ~ the 1-sigma band of the narrowest built-in filter).
  // Every bin from 1 to n/2 - 1 belongs to a window, so neither a quiet low end (a high-passed signal) nor a notch of
  // 3/4 octave or more escapes; a narrower notch does not take a row's energy away.
  std::vector<double> e, cnt;
  for (int w = 0; w < SPECTRUM_WINDOWS; ++w) {
    const int64_t lo = spectrum_window_lo(w), hi = std::min<int64_t>(spectrum_window_lo(w + 1), n / 2);
    if (hi <= lo) continue;
    e.push_back(h[2 + w]);
    cnt.push_back(double(hi - lo));
  }
  double fl = -1;
  for (size_t i = 0; i < e.size(); ++i) {
    double es = e[i], cs = cnt[i];
    if (i > 0) { es += e[i - 1]; cs += cnt[i - 1]; }
    if (i + 1 < e.size()) { es += e[i + 1]; cs += cnt[i + 1]; }
    const double r = std::sqrt(es / cs);
    if (fl < 0 || r < fl || r != r) fl = r;
  }
  *floor_abs = fl >= 0 ? fl : *rms_abs;
  return CWT_OK;
}

// The filter-relative tolerance that keeps `target` relative to every row's own peak for a spectrum of dynamic range
// D = max|xhat| / floor (cwt_spectrum_range): the truncation error of a row can reach tolerance * D / 4 (cwt_hip.h); white
// noise has D ~ 5 ... 7, up to ~20 when one of the few-bin windows at the low end happens to be quiet (which then costs half
// a decade of tolerance, not accuracy); a power of sqrt(10) (calls with like spectra share one cached row table), never
// looser than the target, never below round-off.  A spectrum with an empty stretch or a non-finite bin: round-off.
static double auto_tolerance_of(const cwt_plan* p, double target, double mx, double fl) {
  const double round_off = default_tolerance(p);
  double tol = target;
  if (!(fl > 0) || !std::isfinite(mx)) return round_off;
  const double excess = (mx / fl) / 8.0;
  if (excess > 1.0) tol = std::pow(10.0, 0.5 * std::floor(2.0 * std::log10(target / excess)));
  return std::max(tol, round_off);
}

int cwt_plan_auto_tolerance(cwt_plan* p, const void* xhat_dev, double target, double* rel_tol) {
  if (!p || !xhat_dev || !rel_tol) return fail(CWT_EINVAL, "NULL argument");
  if (!(target > 0) || target > 1e-2) return fail(CWT_EINVAL, "target must be in (0, 1e-2]");
  double mx = 0, rms = 0, fl = 0;
  const int rc = cwt_spectrum_range(p, xhat_dev, p->N, &mx, &rms, &fl);
  if (rc) return rc;
  p->last_range = fl > 0 ? mx / fl : std::numeric_limits<double>::infinity();
  *rel_tol = auto_tolerance_of(p, target, mx, fl);
  return CWT_OK;
}

int cwt_plan_get_tolerance(cwt_plan* p, double* rel_tol) {
  if (!p || !rel_tol) return fail(CWT_EINVAL, "NULL argument");
  *rel_tol = p->tolerance > 0 ? p->tolerance : default_tolerance(p);
  return CWT_OK;
}

int cwt_plan_sync(cwt_plan* p) {
  if (!p) return fail(CWT_EINVAL, "plan is NULL");
  HIPCHECK(hipStreamSynchronize(p->stream));
  return CWT_OK;
}

int cwt_device_memory(int device, size_t* free_bytes, size_t* total_bytes) {
  if (!free_bytes || !total_bytes) return fail(CWT_EINVAL, "NULL argument");
  HIPCHECK(hipSetDevice(device));
  HIPCHECK(hipMemGetInfo(free_bytes, total_bytes));
  return CWT_OK;
}
int cwt_device_synchronize(int device) {
  HIPCHECK(hipSetDevice(device));
  HIPCHECK(hipDeviceSynchronize());
  return CWT_OK;
}
int cwt_malloc(int device, void** ptr, size_t bytes) {
  if (!ptr) return fail(CWT_EINVAL, "ptr is NULL");
  HIPCHECK(hipSetDevice(device));
  if (hipMalloc(ptr, bytes) != hipSuccess) return fail(CWT_ENOMEM, "hipMalloc failed");
  return CWT_OK;
}
int cwt_free(int device, void* ptr) {
  HIPCHECK(hipSetDevice(device));
  HIPCHECK(hipFree(ptr));
  return CWT_OK;
}
int cwt_memcpy_h2d(cwt_plan* p, void* dst, const void* src, size_t bytes) {
  if (!p) return fail(CWT_EINVAL, "plan is NULL");
  HIPCHECK(hipSetDevice(p->device));
  HIPCHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, p->stream));
  HIPCHECK(hipStreamSynchronize(p->stream));
  return CWT_OK;
}
int cwt_memcpy_d2h(cwt_plan* p, void* dst, const void* src, size_t bytes) {
  if (!p) return fail(CWT_EINVAL, "plan is NULL");
  HIPCHECK(hipSetDevice(p->device));
  return copy_d2h(p, dst, src, bytes);
}

int cwt_forward_fft(cwt_plan* p, const void* x_dev, int64_t n0, void* xhat_dev) {
  if (!p || !x_dev || !xhat_dev) return fail(CWT_EINVAL, "NULL argument");
  if (n0 < 1 || n0 > p->N) return fail(CWT_EINVAL, "n0 must be in [1, nfft]");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) { return fft_rows_impl<decltype(t), IN_REAL>(p, x_dev, 0, 1, n0, xhat_dev, p->stream); });
}



// cwt_transform_rows and cwt_transform_rows_power: one row table (the output is not part of its key)
static int transform_rows_entry(cwt_plan* p, const void* xhat_dev, int mother, double param, double dt, const double* scales,
                                int nrows, void* W_dev, int64_t ldw, int64_t ncols, int power) {
  if (!p || !xhat_dev || !scales || !W_dev) return fail(CWT_EINVAL, "NULL argument");
  HIPCHECK(hipSetDevice(p->device));
  int rc = prepare_rows_table(p, false, mother, param, dt, scales, nrows, ldw, ncols);
  if (!rc && p->logN >= 18 && !p->profile) rc = ensure_distinct_queues(p);
  if (rc) return rc;
  return queue_rows(p, xhat_dev, mother_of(mother, param), nrows, W_dev, ldw, ncols, power);
}

int cwt_transform_rows(cwt_plan* p, const void* xhat_dev, int mother, double param, double dt,
                       const double* scales, int nrows, void* W_dev, int64_t ldw, int64_t ncols) {
  return transform_rows_entry(p, xhat_dev, mother, param, dt, scales, nrows, W_dev, ldw, ncols, 0);
}

int cwt_transform_rows_power(cwt_plan* p, const void* xhat_dev, int mother, double param, double dt,
                             const double* scales, int nrows, void* P_dev, int64_t ldp, int64_t ncols) {
  return transform_rows_entry(p, xhat_dev, mother, param, dt, scales, nrows, P_dev, ldp, ncols, 1);
}

// The transpose of cwt_transform_rows.  The row table is the one cwt_transform builds for the same scales and ncols (the forward of a
// training step has classified and cached it already); the rows of form P may go through the transpose of that form.
int cwt_adjoint_rows(cwt_plan* p, const void* G_dev, int nbatch, int64_t g_batch_ld, int64_t ldg, int64_t ncols, int mother,
                     double param, double dt, const double* scales, int nrows, void* xbar_dev, int64_t xbar_ld, int accumulate) {
  if (!p || !G_dev || !scales || !xbar_dev) return fail(CWT_EINVAL, "NULL argument");
  if (mother == MOTHER_TABLE) return fail(CWT_EINVAL, "adjoint: a built-in mother is needed (a filter bank has no adjoint here)");
  if (nbatch < 1) return fail(CWT_EINVAL, "nbatch must be >= 1");
  if (ncols < 1 || ncols > p->N || ldg < ncols || xbar_ld < ncols) return fail(CWT_EINVAL, "need 1 <= ncols <= nfft, ldg >= ncols, xbar_ld >= ncols");
  if (nbatch > 1 && (g_batch_ld < int64_t(nrows) * ldg)) return fail(CWT_EINVAL, "g_batch_ld must be >= nrows * ldg");
  HIPCHECK(hipSetDevice(p->device));
  const int rc = prepare_rows_table(p, true, mother, param, dt, scales, nrows, ncols, ncols);
  if (rc) return rc;
  return by_precision(p, [&](auto t) {
    return adjoint_impl<decltype(t)>(p, G_dev, nbatch, g_batch_ld, ldg, ncols, mother_of(mother, param), nrows, xbar_dev, xbar_ld,
                                     accumulate, nullptr);
  });
}

// The weights of a *_weighted call: Q (reals of the plan's precision, laid out as the output G) and alpha
struct Weights { const void* q; double alpha; };

// What a transform entry point decides about its call: the output (W, its power, or W under the weights *wq) and, for a batch, the
// elements between its signals
static Call call_of(int power, const Weights* wq, int64_t x_ld = 0) {
  Call call;
  call.ols_x_ld = x_ld;
  call.power = power;
  if (wq) { call.weighted = 1; call.q = wq->q; call.alpha = wq->alpha; }
  return call;
}

// Q and G of a weighted call: nbatch * nrows rows of ld elements each, neither NULL, not overlapping
static int check_weights(const cwt_plan* p, const Weights& wq, const void* G_dev, int nbatch, int nrows, int64_t ld, int64_t ncols) {
  if (!wq.q) return fail(CWT_EINVAL, "NULL argument");
  if (ncols < 1 || ld < ncols) return fail(CWT_EINVAL, "weighted output: need 1 <= ncols <= ld");
  if (nbatch < 1 || nrows < 1) return fail(CWT_EINVAL, "weighted output: need nbatch >= 1 and nrows >= 1");
  const size_t elems = (size_t(nbatch) * size_t(nrows) - 1) * size_t(ld) + size_t(ncols), es = p->esize();
  const uintptr_t q0 = reinterpret_cast<uintptr_t>(wq.q), g0 = reinterpret_cast<uintptr_t>(G_dev);
  if (q0 < g0 + elems * 2 * es && g0 < q0 + elems * es) return fail(CWT_EINVAL, "weighted output: Q and G overlap");
  return CWT_OK;
}

static int transform_entry(cwt_plan* p, const void* x_dev, int64_t n0, int mother, double param, double dt,
                           const double* scales, int nrows, void* xhat_dev, void* W_dev, int64_t ldw, int64_t ncols, int power,
                           const Weights* wq = nullptr) {
  if (!p || !x_dev || !scales || !W_dev) return fail(CWT_EINVAL, "NULL argument");
  if (n0 < 1 || n0 > p->N) return fail(CWT_EINVAL, "n0 must be in [1, nfft]");
  if (wq) if (int rc = check_weights(p, *wq, W_dev, 1, nrows, ldw, ncols)) return rc;
  HIPCHECK(hipSetDevice(p->device));
  int rc = prepare_rows_table(p, true, mother, param, dt, scales, nrows, ldw, ncols);
  if (!rc && p->logN >= 18 && !p->profile) rc = ensure_distinct_queues(p);     // (transforms that use the side streams)
  if (rc) return rc;
  // the caller does not want the spectrum: computed (into plan scratch) only if some row needs it
  const bool only_ols = !xhat_dev && p->rt->n_ols == nrows;      // every row is an overlap-save row on the real signal
  if (!xhat_dev && !only_ols) {
    rc = grow(&p->hxhat, &p->hxhat_bytes, size_t(p->N) * 2 * p->esize(), p->stream);
    if (rc) return rc;
    xhat_dev = p->hxhat;
  }
  const Mother mo = mother_of(mother, param);
  const Call call = call_of(power, wq);
  DrainOnFailure drain(p);
  return drain.done(by_precision(p, [&](auto t) {
    return transform_impl<decltype(t)>(p, call, x_dev, n0, xhat_dev, mo, nrows, W_dev, ldw, ncols);
  }));
}

int cwt_transform(cwt_plan* p, const void* x_dev, int64_t n0, int mother, double param, double dt,
                  const double* scales, int nrows, void* xhat_dev, void* W_dev, int64_t ldw, int64_t ncols) {
  return transform_entry(p, x_dev, n0, mother, param, dt, scales, nrows, xhat_dev, W_dev, ldw, ncols, 0);
}

int cwt_transform_power(cwt_plan* p, const void* x_dev, int64_t n0, int mother, double param, double dt,
                        const double* scales, int nrows, void* xhat_dev, void* P_dev, int64_t ldp, int64_t ncols) {
  return transform_entry(p, x_dev, n0, mother, param, dt, scales, nrows, xhat_dev, P_dev, ldp, ncols, 1);
}

// G = (alpha Q) W: the row kernels of cwt_transform under a real weight per element (the cotangent of W that a weight on |W|^2
// induces); the row table and the schedule are those of cwt_transform / cwt_transform_power for the same scales
int cwt_transform_weighted(cwt_plan* p, const void* x_dev, int64_t n0, int mother, double param, double dt, const double* scales,
                           int nrows, void* xhat_dev, const void* Q_dev, double alpha, void* G_dev, int64_t ld, int64_t ncols) {
  const Weights wq{Q_dev, alpha};
  if (!Q_dev) return fail(CWT_EINVAL, "NULL argument");
  return transform_entry(p, x_dev, n0, mother, param, dt, scales, nrows, xhat_dev, G_dev, ld, ncols, 0, &wq);
}

int cwt_transform_rows_batch(cwt_plan* p, const void* xhat_dev, int nbatch, int64_t xhat_ld, int mother,
                             double param, double dt, const double* scales, int nrows, void* W_dev,
                             int64_t ldw, int64_t ncols) {
  if (!p || !xhat_dev || !scales || !W_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nbatch < 1 || nrows < 1 || int64_t(nbatch) * nrows > p->max_rows)
    return fail(CWT_EINVAL, "need nbatch*nrows <= max_rows");
  if (xhat_ld < p->N) return fail(CWT_EINVAL, "xhat_ld must be >= nfft");
  HIPCHECK(hipSetDevice(p->device));
  // W is treated as one (nbatch*nrows) x ldw matrix: row b*nrows + j = scale j of signal b
  TableCall c = scale_rows(mother, param, dt, scales, nrows, ldw, ncols);
  c.kind = 2;
  c.head = {p->tolerance, double(mother), param, dt, double(nbatch), double(xhat_ld), double(nrows)};
  c.nbatch = nbatch;
  c.rows.rows_per_signal = nrows; c.rows.spec_ld = xhat_ld;
  const int rc = prepare_table(p, c);
  if (rc) return rc;
  return queue_rows(p, xhat_dev, mother_of(mother, param), nbatch * nrows, W_dev, ldw, ncols);
}

static int transform_batch_entry(cwt_plan* p, const void* x_dev, int nbatch, int64_t x_ld, int64_t n0, int mother,
                                 double param, double dt, const double* scales, int nrows, void* xhat_dev, void* W_dev,
                                 int64_t ldw, int64_t ncols, int power, const Weights* wq = nullptr) {
  if (!p || !x_dev || !scales || !xhat_dev || !W_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nbatch < 1 || nrows < 1 || int64_t(nbatch) * nrows > p->max_rows)
    return fail(CWT_EINVAL, "need nbatch*nrows <= max_rows");
  if (wq) if (int rc = check_weights(p, *wq, W_dev, nbatch, nrows, ldw, ncols)) return rc;
  if (n0 < 1 || n0 > p->N || x_ld < n0) return fail(CWT_EINVAL, "need 1 <= n0 <= nfft and x_ld >= n0");
  HIPCHECK(hipSetDevice(p->device));
  // as cwt_transform_rows_batch, with the signals at hand: time-compact rows may take the overlap-save form
  TableCall c = scale_rows(mother, param, dt, scales, nrows, ldw, ncols);
  c.kind = 3;
  c.head = {p->tolerance, double(mother), param, dt, double(nbatch), double(nrows), double(ncols)};
  c.nbatch = nbatch;
  c.rows.rows_per_signal = nrows; c.rows.spec_ld = p->N;
  c.rows.ols_ncols = c.rows.out_ncols = ncols;
  int rc = prepare_table(p, c);
  if (rc) return rc;
  const Mother mo = mother_of(mother, param);
  const Call call = call_of(power, wq, x_ld);
  DrainOnFailure drain(p);
  rc = by_precision(p, [&](auto t) { return fft_rows_impl<decltype(t), IN_REAL>(p, x_dev, x_ld, nbatch, n0, xhat_dev, p->stream); });
  if (rc) return rc;
  return drain.done(by_precision(p, [&](auto t) {
    return rows_impl<decltype(t)>(p, call, xhat_dev, mo, nbatch * nrows, W_dev, ldw, ncols, x_dev, n0);
  }));
}

int cwt_transform_batch(cwt_plan* p, const void* x_dev, int nbatch, int64_t x_ld, int64_t n0, int mother,
                        double param, double dt, const double* scales, int nrows, void* xhat_dev, void* W_dev,
                        int64_t ldw, int64_t ncols) {
  return transform_batch_entry(p, x_dev, nbatch, x_ld, n0, mother, param, dt, scales, nrows, xhat_dev, W_dev, ldw, ncols, 0);
}

int cwt_transform_batch_power(cwt_plan* p, const void* x_dev, int nbatch, int64_t x_ld, int64_t n0, int mother,
                              double param, double dt, const double* scales, int nrows, void* xhat_dev, void* P_dev,
                              int64_t ldp, int64_t ncols) {
  return transform_batch_entry(p, x_dev, nbatch, x_ld, n0, mother, param, dt, scales, nrows, xhat_dev, P_dev, ldp, ncols, 1);
}

int cwt_transform_batch_weighted(cwt_plan* p, const void* x_dev, int nbatch, int64_t x_ld, int64_t n0, int mother, double param,
                                 double dt, const double* scales, int nrows, void* xhat_dev, const void* Q_dev, double alpha,
                                 void* G_dev, int64_t ld, int64_t ncols) {
  const Weights wq{Q_dev, alpha};
  if (!Q_dev) return fail(CWT_EINVAL, "NULL argument");
  return transform_batch_entry(p, x_dev, nbatch, x_ld, n0, mother, param, dt, scales, nrows, xhat_dev, G_dev, ld, ncols, 0, &wq);
}

// ---- decimated output: every hop-th column (cwt_hip.h) -------------------------------------------------------------------------
// The checks every hop entry point shares, before anything is queued; *logM = log2(nfft / hop)
static int check_hop(const cwt_plan* p, int nbatch, int nrows, int64_t n0, int64_t hop, int64_t ld, int64_t ncols_h, int* logM) {
  if (nbatch < 1 || nrows < 1 || int64_t(nbatch) * nrows > p->max_rows) return fail(CWT_EINVAL, "need nbatch*nrows <= max_rows");
  if (nrows > kMaxGridY) return fail(CWT_EINVAL, "decimated transform: at most 32768 scales per call");   // (gridDim.y of hop_fold)
  if (n0 < 1 || n0 > p->N) return fail(CWT_EINVAL, "n0 must be in [1, nfft]");
  if (hop < 2 || (hop & (hop - 1))) return fail(CWT_EINVAL, "hop must be a power of two >= 2");
  const int64_t M = p->N / hop;
  if (hop > p->N || M < 16 || M > 4096) return fail(CWT_EINVAL, "nfft / hop must be in [16, 4096] (longer decimated rows are not built)");
  if (ncols_h != (n0 + hop - 1) / hop) return fail(CWT_EINVAL, "ncols_h must be ceil(n0 / hop)");
  if (ld < ncols_h) return fail(CWT_EINVAL, "ld must be >= ncols_h");
  *logM = ilog2(M);
  return CWT_OK;
}

static int transform_hop_entry(cwt_plan* p, const void* x_dev, int nbatch, int64_t x_ld, int64_t n0, int mother, double param,
                               double dt, const double* scales, int nrows, int64_t hop, void* xhat_dev, int64_t xhat_ld, int output,
                               void* out_dev, const void* Q_dev, double alpha, int64_t ld, int64_t ncols_h, bool from_signal) {
  if (!p || !scales || !out_dev || (from_signal ? !x_dev : !xhat_dev)) return fail(CWT_EINVAL, "NULL argument");
  if (mother == MOTHER_TABLE) return fail(CWT_EINVAL, "decimated transform: a built-in mother is needed");
  if (output < 0 || output > (from_signal ? 2 : 1)) return fail(CWT_EINVAL, from_signal ? "output must be 0 (W), 1 (power) or 2 (weighted)" : "output must be 0 (W) or 1 (power)");
  int logM = 0;
  if (int rc = check_hop(p, nbatch, nrows, n0, hop, ld, ncols_h, &logM)) return rc;
  if (from_signal && nbatch > 1 && x_ld < n0) return fail(CWT_EINVAL, "x_ld must be >= n0");
  if (!from_signal && xhat_ld < p->N && nbatch > 1) return fail(CWT_EINVAL, "xhat_ld must be >= nfft");
  if (output == 2) {
    const Weights wq{Q_dev, alpha};
    if (int rc = check_weights(p, wq, out_dev, nbatch, nrows, ld, ncols_h)) return rc;
  }
  HIPCHECK(hipSetDevice(p->device));
  // the table of cwt_transform for these scales and n0 columns (the output and the hop are not part of its key)
  int rc = prepare_rows_table(p, true, mother, param, dt, scales, nrows, n0, n0);
  if (rc) return rc;
  if (from_signal && !xhat_dev) {                          // the caller has no use for the spectra: plan scratch
    rc = grow(&p->hxhat, &p->hxhat_bytes, size_t(nbatch) * size_t(p->N) * 2 * p->esize(), p->stream);
    if (rc) return rc;
    xhat_dev = p->hxhat;
  }
  if (from_signal) xhat_ld = p->N;
  const Mother mo = mother_of(mother, param);
  const Weights wq{Q_dev, alpha};
  const Call call = call_of(output == 1, output == 2 ? &wq : nullptr);
  DrainOnFailure drain(p);
  return drain.done(by_precision(p, [&](auto t) {
    return transform_hop_impl<decltype(t)>(p, call, from_signal ? x_dev : nullptr, nbatch, x_ld, n0, xhat_dev, xhat_ld, mo, nrows, logM,
                                           out_dev, ld, ncols_h);
  }));
}

int cwt_transform_hop(cwt_plan* p, const void* x_dev, int nbatch, int64_t x_ld, int64_t n0, int mother, double param, double dt,
                      const double* scales, int nrows, int64_t hop, void* xhat_dev, int output, void* out_dev, const void* Q_dev,
                      double alpha, int64_t ld, int64_t ncols_h) {
  return transform_hop_entry(p, x_dev, nbatch, x_ld, n0, mother, param, dt, scales, nrows, hop, xhat_dev, 0, output, out_dev, Q_dev,
                             alpha, ld, ncols_h, true);
}

int cwt_transform_rows_hop(cwt_plan* p, const void* xhat_dev, int nbatch, int64_t xhat_ld, int64_t n0, int mother, double param,
                           double dt, const double* scales, int nrows, int64_t hop, int output, void* out_dev, int64_t ld,
                           int64_t ncols_h) {
  return transform_hop_entry(p, nullptr, nbatch, 0, n0, mother, param, dt, scales, nrows, hop, const_cast<void*>(xhat_dev), xhat_ld,
                             output, out_dev, nullptr, 0.0, ld, ncols_h, false);
}

int cwt_adjoint_rows_hop(cwt_plan* p, const void* G_dev, int nbatch, int64_t g_batch_ld, int64_t ldg, int64_t ncols_h, int64_t hop,
                         int64_t n0, int mother, double param, double dt, const double* scales, int nrows, void* xbar_dev,
                         int64_t xbar_ld, int accumulate) {
  if (!p || !G_dev || !scales || !xbar_dev) return fail(CWT_EINVAL, "NULL argument");
  if (mother == MOTHER_TABLE) return fail(CWT_EINVAL, "adjoint: a built-in mother is needed (a filter bank has no adjoint here)");
  int logM = 0;
  if (int rc = check_hop(p, nbatch, nrows, n0, hop, ldg, ncols_h, &logM)) return rc;
  if (xbar_ld < n0) return fail(CWT_EINVAL, "xbar_ld must be >= n0");
  if (nbatch > 1 && g_batch_ld < int64_t(nrows) * ldg) return fail(CWT_EINVAL, "g_batch_ld must be >= nrows * ldg");
  HIPCHECK(hipSetDevice(p->device));
  const int rc = prepare_rows_table(p, true, mother, param, dt, scales, nrows, n0, n0);
  if (rc) return rc;
  return by_precision(p, [&](auto t) {
    return adjoint_hop_impl<decltype(t)>(p, G_dev, nbatch, g_batch_ld, ldg, ncols_h, logM, n0, mother_of(mother, param), nrows, xbar_dev,
                                         xbar_ld, accumulate, nullptr);
  });
}

// ---- time-pooled scalogram: window means of |W|^2 (cwt_hip.h) --------------------------------------------------------------------
int cwt_transform_pool(cwt_plan* p, const void* x_dev, int nbatch, int64_t x_ld, int64_t n0, int mother, double param, double dt,
                       const double* scales, int nrows, int64_t pool, void* xhat_dev, void* P_dev, int64_t ldp, int64_t ncols_p) {
  if (!p || !x_dev || !scales || !P_dev) return fail(CWT_EINVAL, "NULL argument");
  if (mother == MOTHER_TABLE) return fail(CWT_EINVAL, "pooled transform: a built-in mother is needed");
  if (nbatch < 1 || nrows < 1 || int64_t(nbatch) * nrows > p->max_rows) return fail(CWT_EINVAL, "need nbatch*nrows <= max_rows");
  if (n0 < 1 || n0 > p->N) return fail(CWT_EINVAL, "n0 must be in [1, nfft]");
  if (nbatch > 1 && x_ld < n0) return fail(CWT_EINVAL, "x_ld must be >= n0");
  if (pool < 2 || (pool & (pool - 1)) || pool > p->N) return fail(CWT_EINVAL, "pool must be a power of two in [2, nfft]");
  if (ncols_p != (n0 + pool - 1) / pool) return fail(CWT_EINVAL, "ncols_p must be ceil(n0 / pool)");
  if (ldp < ncols_p) return fail(CWT_EINVAL, "ldp must be >= ncols_p");
  HIPCHECK(hipSetDevice(p->device));
  // the table of cwt_transform / cwt_transform_power for these scales and n0 columns (neither the output nor the pool is part of its key)
  int rc = prepare_rows_table(p, true, mother, param, dt, scales, nrows, n0, n0);
  if (!rc && p->logN >= 18 && !p->profile) rc = ensure_distinct_queues(p);
  if (rc) return rc;
  const bool only_ols = !xhat_dev && p->rt->n_ols == nrows;      // no row needs a spectrum
  if (!xhat_dev && !only_ols) {                                  // the caller has no use for the spectra: one signal's, in plan scratch
    rc = grow(&p->hxhat, &p->hxhat_bytes, size_t(p->N) * 2 * p->esize(), p->stream);
    if (rc) return rc;
  }
  const Mother mo = mother_of(mother, param);
  const int logh = ilog2(pool);
  DrainOnFailure drain(p);
  if (xhat_dev || only_ols)
    return drain.done(by_precision(p, [&](auto t) {
      return transform_pool_impl<decltype(t)>(p, x_dev, nbatch, x_ld, n0, xhat_dev, mo, nrows, logh, P_dev, ldp);
    }));
  for (int b = 0; b < nbatch && !rc; ++b)                        // (every signal's spectrum through the same scratch, in stream order)
    rc = by_precision(p, [&](auto t) {
      using T = decltype(t);
      return transform_pool_impl<T>(p, static_cast<const T*>(x_dev) + size_t(b) * size_t(x_ld), 1, 0, n0, p->hxhat, mo, nrows, logh,
                                    static_cast<T*>(P_dev) + size_t(b) * size_t(nrows) * size_t(ldp), ldp);
    });
  return drain.done(rc);
}

// cwt_adjoint_rows (hop = 1) or cwt_adjoint_rows_hop with the gradients with respect to the scales and f0 beside xbar: the checks of
// those two, the same row table, every row through the general path (sgrad_partial reads the spectra it forms).
int cwt_adjoint_rows_scales(cwt_plan* p, const void* G_dev, int nbatch, int64_t g_batch_ld, int64_t ldg, int64_t ncols, int64_t hop,
                            int64_t n0, const void* xhat_dev, int64_t xhat_ld, int mother, double param, double dt, const double* scales,
                            int nrows, void* xbar_dev, int64_t xbar_ld, int accumulate, double* sgrad_dev) {
  if (!p || !G_dev || !scales || !xhat_dev || !sgrad_dev) return fail(CWT_EINVAL, "NULL argument");
  if (mother == MOTHER_TABLE) return fail(CWT_EINVAL, "adjoint: a built-in mother is needed (a filter bank has no adjoint here)");
  int logM = 0;
  if (hop == 1) {
    if (nbatch < 1 || nrows < 1) return fail(CWT_EINVAL, "need nbatch >= 1 and nrows >= 1");
    if (n0 < 1 || n0 > p->N || ncols != n0 || ldg < ncols) return fail(CWT_EINVAL, "hop = 1: need 1 <= ncols = n0 <= nfft and ldg >= ncols");
  } else if (int rc = check_hop(p, nbatch, nrows, n0, hop, ldg, ncols, &logM)) {
    return rc;
  }
  if (xbar_dev && xbar_ld < n0) return fail(CWT_EINVAL, "xbar_ld must be >= n0");
  if (nbatch > 1 && g_batch_ld < int64_t(nrows) * ldg) return fail(CWT_EINVAL, "g_batch_ld must be >= nrows * ldg");
  if (nbatch > 1 && xhat_ld < p->N) return fail(CWT_EINVAL, "xhat_ld must be >= nfft");
  HIPCHECK(hipSetDevice(p->device));
  const int rc = prepare_rows_table(p, true, mother, param, dt, scales, nrows, n0, n0);
  if (rc) return rc;
  const cwtd::ScaleGrad sg{xhat_dev, xhat_ld, sgrad_dev};
  return by_precision(p, [&](auto t) {
    if (hop == 1)
      return adjoint_impl<decltype(t)>(p, G_dev, nbatch, g_batch_ld, ldg, ncols, mother_of(mother, param), nrows, xbar_dev, xbar_ld,
                                       accumulate, &sg);
    return adjoint_hop_impl<decltype(t)>(p, G_dev, nbatch, g_batch_ld, ldg, ncols, logM, n0, mother_of(mother, param), nrows, xbar_dev,
                                         xbar_ld, accumulate, &sg);
  });
}

int cwt_transform_rows_table(cwt_plan* p, const void* xhat_dev, const void* table_dev, const int* k_lo,
                             const int* nband, int nrows, void* W_dev, int64_t ldw, int64_t ncols) {
  if (!p || !xhat_dev || !table_dev || !k_lo || !nband || !W_dev) return fail(CWT_EINVAL, "NULL argument");
  HIPCHECK(hipSetDevice(p->device));
  TableCall c;                                           // (kind -1: explicit filter banks are not cached)
  c.nrows = nrows;
  c.rows.tab_klo = k_lo; c.rows.tab_nband = nband;
  c.ldw = ldw;
  c.ncols = ncols;
  const int rc = prepare_table(p, c);
  if (rc) return rc;
  Mother mo = mother_of(MOTHER_TABLE, 0.0);
  mo.table = table_dev;
  return queue_rows(p, xhat_dev, mo, nrows, W_dev, ldw, ncols);
}

int cwt_fft_rows(cwt_plan* p, const void* in_dev, int in_complex, int nrows, int64_t in_ld, int64_t ncols_in,
                 void* spec_dev) {
  if (!p || !in_dev || !spec_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1) return fail(CWT_EINVAL, "nrows must be >= 1");
  if (ncols_in < 1 || ncols_in > p->N || in_ld < ncols_in) return fail(CWT_EINVAL, "need 1 <= ncols_in <= nfft and in_ld >= ncols_in");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    using T = decltype(t);
    return in_complex ? fft_rows_impl<T, IN_CPLX>(p, in_dev, in_ld, nrows, ncols_in, spec_dev, p->stream)
                      : fft_rows_impl<T, IN_REAL>(p, in_dev, in_ld, nrows, ncols_in, spec_dev, p->stream);
  });
}

int cwt_filter_rows(cwt_plan* p, const void* spec_dev, int64_t spec_ld, int mother, double param,
                    const double* a, const double* amp_re, const double* amp_im, int nrows, void* W_dev,
                    int64_t ldw, int64_t ncols) {
  if (!p || !spec_dev || !a || !amp_re || !amp_im || !W_dev) return fail(CWT_EINVAL, "NULL argument");
  HIPCHECK(hipSetDevice(p->device));
  TableCall c;
  c.kind = 1;
  c.head = {p->tolerance, double(mother), param, double(spec_ld), double(nrows)};
  c.rows.mother = mother; c.rows.param = param;
  c.nrows = nrows;
  c.rows.a = a; c.rows.amp_re = amp_re; c.rows.amp_im = amp_im;
  c.ldw = ldw;
  c.ncols = ncols;
  c.rows.spec_ld = spec_ld;
  const int rc = prepare_table(p, c);
  if (rc) return rc;
  return queue_rows(p, spec_dev, mother_of(mother, param), nrows, W_dev, ldw, ncols);
}

int cwt_wct_products(cwt_plan* p, const void* W1_dev, const void* W2_dev, const double* scales, int nrows,
                     int64_t ld, int64_t ncols, void* P_dev, void* C_dev, void* angle_dev) {
  if (!p || !W1_dev || !W2_dev || !scales || !P_dev || !C_dev || !angle_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || nrows > p->max_rows || ncols < 1 || ld < ncols) return fail(CWT_EINVAL, "bad shape");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    return wct_products_impl<decltype(t)>(p, W1_dev, W2_dev, scales, nrows, ld, ncols, P_dev, C_dev, angle_dev);
  });
}

int cwt_cross_spectrum(cwt_plan* p, const void* W1_dev, const void* W2_dev, int nrows, int64_t ld, int64_t ncols,
                       void* out_dev) {
  if (!p || !W1_dev || !W2_dev || !out_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || nrows > 65535 || ncols < 1 || ld < ncols) return fail(CWT_EINVAL, "bad shape");
  HIPCHECK(hipSetDevice(p->device));
  const dim3 grid(unsigned((ncols + 255) / 256), unsigned(nrows));
  return by_precision(p, [&](auto t) {
    using T = decltype(t);
    return timed_launch(p, KC_ELEMENTWISE, [&] {
      hipLaunchKernelGGL((k_cross_spectrum<T>), grid, dim3(256), 0, p->stream, static_cast<const cplx<T>*>(W1_dev),
                         static_cast<const cplx<T>*>(W2_dev), long(ld), long(ncols), static_cast<cplx<T>*>(out_dev));
    }, p->stream);
  });
}

int cwt_boxcar_scales(cwt_plan* p, const void* in_dev, int nrows, int64_t ld, int64_t ncols, const double* win,
                      int nwin, void* out_dev) {
  if (!p || !in_dev || !win || !out_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || ncols < 1 || ld < ncols || nwin < 1 || nwin > p->max_rows) return fail(CWT_EINVAL, "bad shape");
  if (in_dev == out_dev) return fail(CWT_EINVAL, "boxcar cannot run in place");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) { return boxcar_impl<decltype(t)>(p, in_dev, nrows, ld, ncols, win, nwin, out_dev); });
}

int cwt_wct_coherence(cwt_plan* p, const void* S_dev, const void* S12_dev, int nrows, int64_t ld, int64_t ncols,
                      void* out_dev) {
  if (!p || !S_dev || !S12_dev || !out_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || ncols < 1 || ld < ncols) return fail(CWT_EINVAL, "bad shape");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) { return coherence_impl<decltype(t)>(p, S_dev, S12_dev, nrows, ld, ncols, out_dev); });
}


int cwt_reduce_scales(cwt_plan* p, const void* W_dev, int64_t ldw, int64_t ncols, int nrows,
                      const double* weights, int power, double coeff, void* out_dev) {
  if (!p || !W_dev || !weights || !out_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || nrows > p->max_rows) return fail(CWT_EINVAL, "nrows must be in [1, max_rows]");
  if (ncols < 1 || ldw < ncols) return fail(CWT_EINVAL, "need ncols >= 1 and ldw >= ncols");
  if (power < 0 || power > 2) return fail(CWT_EINVAL, "power must be 0, 1 or 2");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    using T = decltype(t);
    if (power == 2) {                                  // W_dev is a real power matrix (cwt_transform_power)
      int rc = upload_reals<T>(p, weights, nrows);
      if (rc) return rc;
      return timed_launch(p, KC_ICWT, [&] {
        hipLaunchKernelGGL((k_icwt_real<T>), dim3(unsigned((ncols + ICWT_THREADS - 1) / ICWT_THREADS)), dim3(ICWT_THREADS), 0,
                           p->stream, static_cast<const T*>(W_dev), long(ldw), long(ncols), nrows,
                           static_cast<const T*>(p->weights_dev), T(coeff), static_cast<T*>(out_dev));
      }, p->stream);
    }
    return power ? reduce_scales_impl<T, true>(p, W_dev, ldw, ncols, nrows, weights, coeff, out_dev)
                 : reduce_scales_impl<T, false>(p, W_dev, ldw, ncols, nrows, weights, coeff, out_dev);
  });
}

int cwt_icwt_reduce(cwt_plan* p, const void* W_dev, int64_t ldw, int64_t ncols, int nrows,
                    const double* scales, double coeff, void* out_dev) {
  if (!p || !scales) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || nrows > p->max_rows) return fail(CWT_EINVAL, "nrows must be in [1, max_rows]");
  std::vector<double> w(nrows);
  for (int j = 0; j < nrows; ++j) {
    if (!(scales[j] > 0)) return fail(CWT_EINVAL, "scales must be positive");
    w[j] = 1.0 / std::sqrt(scales[j]);
  }
  return cwt_reduce_scales(p, W_dev, ldw, ncols, nrows, w.data(), 0, coeff, out_dev);
}

int cwt_icwt_shrink(cwt_plan* p, const void* W_dev, int64_t ldw, int64_t ncols, int nrows, const double* scales,
                    const void* lambda_dev, int mode, double coeff, void* out_dev) {
  if (!p || !W_dev || !scales || !lambda_dev || !out_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || nrows > p->max_rows) return fail(CWT_EINVAL, "nrows must be in [1, max_rows]");
  if (ncols < 1 || ldw < ncols) return fail(CWT_EINVAL, "need ncols >= 1 and ldw >= ncols");
  if (mode < 0 || mode > 2) return fail(CWT_EINVAL, "mode must be 0 (hard), 1 (soft) or 2 (garrote)");
  std::vector<double> w(nrows);
  for (int j = 0; j < nrows; ++j) {
    if (!(scales[j] > 0)) return fail(CWT_EINVAL, "scales must be positive");
    w[j] = 1.0 / std::sqrt(scales[j]);
  }
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    return icwt_shrink_impl<decltype(t)>(p, W_dev, ldw, ncols, nrows, w.data(), lambda_dev, mode, coeff, out_dev);
  });
}

int cwt_icwt_shrink_adjoint(cwt_plan* p, const void* W_dev, int64_t ldw, int64_t ncols, int nrows, const double* scales,
                            const void* lambda_dev, int mode, double coeff, const void* gy_dev, void* G_dev, int64_t ldg,
                            double* glambda_dev, int accumulate) {
  if (!p || !W_dev || !scales || !gy_dev || !G_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || nrows > p->max_rows) return fail(CWT_EINVAL, "nrows must be in [1, max_rows]");
  if (ncols < 1 || ldw < ncols || ldg < ncols) return fail(CWT_EINVAL, "need ncols >= 1, ldw >= ncols and ldg >= ncols");
  if (mode < 0 || mode > 2) return fail(CWT_EINVAL, "mode must be 0 (hard), 1 (soft) or 2 (garrote)");
  if (glambda_dev && !lambda_dev) return fail(CWT_EINVAL, "glambda_dev needs lambda_dev");
  std::vector<double> w(nrows);
  for (int j = 0; j < nrows; ++j) {
    if (!(scales[j] > 0)) return fail(CWT_EINVAL, "scales must be positive");
    w[j] = 1.0 / std::sqrt(scales[j]);
  }
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    return icwt_shrink_adjoint_impl<decltype(t)>(p, W_dev, ldw, ncols, nrows, w.data(), lambda_dev, mode, coeff, gy_dev, G_dev, ldg,
                                                 glambda_dev, accumulate);
  });
}

int cwt_row_order_statistics(cwt_plan* p, const void* A_dev, int is_complex, int64_t ld, int64_t ncols, int nrows,
                             const int64_t* ranks, int nranks, void* out_dev, int64_t ldo) {
  if (!p || !A_dev || !ranks || !out_dev) return fail(CWT_EINVAL, "NULL argument");
  if (is_complex != 0 && is_complex != 1) return fail(CWT_EINVAL, "is_complex must be 0 or 1");
  if (nrows < 1 || ncols < 1 || ld < ncols) return fail(CWT_EINVAL, "need nrows >= 1, ncols >= 1 and ld >= ncols");
  if (nranks < 1 || nranks > SEL_MAX_RANKS) return fail(CWT_EINVAL, "nranks must be in [1, 8]");
  if (ldo < nranks) return fail(CWT_EINVAL, "need ldo >= nranks");
  for (int i = 0; i < nranks; ++i)
    if (ranks[i] < 0 || ranks[i] >= ncols) return fail(CWT_EINVAL, "ranks must be in [0, ncols)");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    return order_statistics_impl<decltype(t)>(p, A_dev, is_complex, ld, ncols, nrows, ranks, nranks, out_dev, ldo);
  });
}

int cwt_time_mean_power(cwt_plan* p, const void* W_dev, int64_t ldw, int64_t ncols, int nrows, void* out_dev) {
  if (!p || !W_dev || !out_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || ncols < 1 || ldw < ncols) return fail(CWT_EINVAL, "bad shape");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    using T = decltype(t);
    return timed_launch(p, KC_ICWT, [&] {
      hipLaunchKernelGGL((k_time_mean<T>), dim3(nrows), dim3(256), 256 * sizeof(double), p->stream,
                         static_cast<const cplx<T>*>(W_dev), long(ldw), long(ncols), static_cast<T*>(out_dev));
    }, p->stream);
  });
}

int cwt_time_mean_real(cwt_plan* p, const void* P_dev, int64_t ldp, int64_t ncols, int nrows, void* out_dev) {
  if (!p || !P_dev || !out_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || ncols < 1 || ldp < ncols) return fail(CWT_EINVAL, "bad shape");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    using T = decltype(t);
    return timed_launch(p, KC_ICWT, [&] {
      hipLaunchKernelGGL((k_time_mean_real<T>), dim3(nrows), dim3(256), 256 * sizeof(double), p->stream,
                         static_cast<const T*>(P_dev), long(ldp), long(ncols), static_cast<T*>(out_dev));
    }, p->stream);
  });
}

int cwt_abs2(cwt_plan* p, const void* W_dev, int64_t ldw, int64_t ncols, int nrows, void* P_dev, int64_t ldp) {
  if (!p || !W_dev || !P_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || ncols < 1 || ldw < ncols || ldp < ncols) return fail(CWT_EINVAL, "bad shape");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    using T = decltype(t);
    return timed_launch(p, KC_ELEMENTWISE, [&] {
      for (int r0 = 0; r0 < nrows; r0 += kMaxGridY)
        hipLaunchKernelGGL((k_abs2<T>), dim3(unsigned((ncols + 255) / 256), unsigned(std::min(kMaxGridY, nrows - r0))), dim3(256), 0,
                           p->stream, static_cast<const cplx<T>*>(W_dev) + size_t(r0) * size_t(ldw), long(ldw), long(ncols),
                           static_cast<T*>(P_dev) + size_t(r0) * size_t(ldp), long(ldp));
    }, p->stream);
  });
}

int cwt_spectrum_derivative(cwt_plan* p, const void* xhat_dev, double dt, void* yhat_dev) {
  if (!p || !xhat_dev || !yhat_dev) return fail(CWT_EINVAL, "NULL argument");
  if (!(dt > 0) || !std::isfinite(dt)) return fail(CWT_EINVAL, "dt must be positive");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) { return spectrum_derivative_impl<decltype(t)>(p, xhat_dev, dt, yhat_dev); });
}

// what cwt_ssq_reassign refuses (cwt_ssq_reassign_bins: the same, then its own)
static int ssq_reassign_check(cwt_plan* p, const void* W_dev, const void* dW_dev, int64_t ld, int64_t ncols, int nrows,
                              const double* weights, double gamma, double f_lo, double dv, int nf, void* T_dev, int64_t ldt) {
  if (!p || !W_dev || !dW_dev || !weights || !T_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || nrows > p->max_rows) return fail(CWT_EINVAL, "nrows must be in [1, max_rows]");
  if (ncols < 1 || ld < ncols || ldt < ncols) return fail(CWT_EINVAL, "need ncols >= 1, ld >= ncols and ldt >= ncols");
  if (nf < 1) return fail(CWT_EINVAL, "nf must be >= 1");
  if (!std::isfinite(gamma) || !std::isfinite(f_lo) || !std::isfinite(dv) || gamma < 0 || !(f_lo > 0) || !(dv > 0))
    return fail(CWT_EINVAL, "need finite gamma >= 0, f_lo > 0 and dv > 0");
  const size_t cs = 2 * p->esize();
  const size_t in_bytes = ((size_t(nrows) - 1) * size_t(ld) + size_t(ncols)) * cs;
  const size_t out_bytes = ((size_t(nf) - 1) * size_t(ldt) + size_t(ncols)) * cs;
  const uintptr_t t0 = reinterpret_cast<uintptr_t>(T_dev);
  for (const void* in : {W_dev, dW_dev}) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(in);
    if (a < t0 + out_bytes && t0 < a + in_bytes) return fail(CWT_EINVAL, "T overlaps W or dW");
  }
  return CWT_OK;
}

int cwt_ssq_reassign(cwt_plan* p, const void* W_dev, const void* dW_dev, int64_t ld, int64_t ncols, int nrows,
                     const double* weights, double gamma, double f_lo, double dv, int nf, void* T_dev, int64_t ldt,
                     int accumulate) {
  const int rc = ssq_reassign_check(p, W_dev, dW_dev, ld, ncols, nrows, weights, gamma, f_lo, dv, nf, T_dev, ldt);
  if (rc) return rc;
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    return ssq_reassign_impl<decltype(t)>(p, W_dev, dW_dev, ld, ncols, nrows, weights, gamma, f_lo, dv, nf, T_dev, ldt, accumulate,
                                          nullptr, 0);
  });
}

// [a, a + na) and [b, b + nb) share a byte
static bool blocks_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

int cwt_ssq_reassign_bins(cwt_plan* p, const void* W_dev, const void* dW_dev, int64_t ld, int64_t ncols, int nrows,
                          const double* weights, double gamma, double f_lo, double dv, int nf, void* T_dev, int64_t ldt,
                          int accumulate, void* bins_dev, int64_t ldb) {
  const int rc = ssq_reassign_check(p, W_dev, dW_dev, ld, ncols, nrows, weights, gamma, f_lo, dv, nf, T_dev, ldt);
  if (rc) return rc;
  if (!bins_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nf > 32767) return fail(CWT_EINVAL, "the map of bins is int16: nf must be <= 32767");
  if (ldb < ncols) return fail(CWT_EINVAL, "need ldb >= ncols");
  const size_t cs = 2 * p->esize();
  const size_t in_bytes = ((size_t(nrows) - 1) * size_t(ld) + size_t(ncols)) * cs;
  const size_t out_bytes = ((size_t(nf) - 1) * size_t(ldt) + size_t(ncols)) * cs;
  const size_t bin_bytes = ((size_t(nrows) - 1) * size_t(ldb) + size_t(ncols)) * sizeof(int16_t);
  if (blocks_overlap(bins_dev, bin_bytes, W_dev, in_bytes) || blocks_overlap(bins_dev, bin_bytes, dW_dev, in_bytes) ||
      blocks_overlap(bins_dev, bin_bytes, T_dev, out_bytes))
    return fail(CWT_EINVAL, "bins overlaps W, dW or T");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    return ssq_reassign_impl<decltype(t)>(p, W_dev, dW_dev, ld, ncols, nrows, weights, gamma, f_lo, dv, nf, T_dev, ldt, accumulate,
                                          bins_dev, ldb);
  });
}

int cwt_ssq_gather(cwt_plan* p, const void* gT_dev, int64_t ldt, int nf, const void* bins_dev, int64_t ldb, const double* weights,
                   int nrows, int64_t ncols, void* G_dev, int64_t ldg) {
  if (!p || !gT_dev || !bins_dev || !weights || !G_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || nrows > p->max_rows) return fail(CWT_EINVAL, "nrows must be in [1, max_rows]");
  if (ncols < 1 || ldt < ncols || ldb < ncols || ldg < ncols)
    return fail(CWT_EINVAL, "need ncols >= 1, ldt >= ncols, ldb >= ncols and ldg >= ncols");
  if (nf < 1 || nf > 32767) return fail(CWT_EINVAL, "nf must be in [1, 32767]");
  const size_t cs = 2 * p->esize();
  const size_t g_bytes = ((size_t(nrows) - 1) * size_t(ldg) + size_t(ncols)) * cs;
  const size_t t_bytes = ((size_t(nf) - 1) * size_t(ldt) + size_t(ncols)) * cs;
  const size_t bin_bytes = ((size_t(nrows) - 1) * size_t(ldb) + size_t(ncols)) * sizeof(int16_t);
  if (blocks_overlap(G_dev, g_bytes, gT_dev, t_bytes) || blocks_overlap(G_dev, g_bytes, bins_dev, bin_bytes))
    return fail(CWT_EINVAL, "G overlaps gT or bins");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    return ssq_gather_impl<decltype(t)>(p, gT_dev, ldt, nf, bins_dev, ldb, weights, nrows, ncols, G_dev, ldg);
  });
}

int cwt_coherence_histogram(cwt_plan* p, const void* r2_dev, int64_t ld, int nrows, const int64_t* lo_dev,
                            const int64_t* hi_dev, int64_t max_span, int nbins, uint64_t* hist_dev) {
  if (!p || !r2_dev || !lo_dev || !hi_dev || !hist_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1 || ld < 1 || nbins < 1 || nbins > 16384 || max_span < 0) return fail(CWT_EINVAL, "bad shape");
  if (max_span == 0) return CWT_OK;
  HIPCHECK(hipSetDevice(p->device));
  static_assert(sizeof(long) == sizeof(int64_t) && sizeof(unsigned long long) == sizeof(uint64_t), "LP64 expected");
  const unsigned gx = unsigned(std::min<int64_t>(512, (max_span + 4095) / 4096));   // >= 16 columns per thread
  const size_t lds = size_t(nbins) * sizeof(unsigned);
  return by_precision(p, [&](auto t) {
    using T = decltype(t);
    return timed_launch(p, KC_ELEMENTWISE, [&] {
      for (int r0 = 0; r0 < nrows; r0 += kMaxGridY)               // (gridDim.y is limited to 65535: slabs of rows)
        hipLaunchKernelGGL((k_coherence_hist<T>), dim3(gx, unsigned(std::min(kMaxGridY, nrows - r0))), dim3(256), lds, p->stream,
                           static_cast<const T*>(r2_dev) + size_t(r0) * size_t(ld), long(ld),
                           reinterpret_cast<const long*>(lo_dev) + r0, reinterpret_cast<const long*>(hi_dev) + r0, nbins,
                           reinterpret_cast<unsigned long long*>(hist_dev) + size_t(r0) * size_t(nbins));
    }, p->stream);
  });
}


int cwt_random_normal(cwt_plan* p, uint64_t seed, uint64_t offset, int64_t n, double scale, void* out_dev) {
  if (!p || !out_dev) return fail(CWT_EINVAL, "NULL argument");
  if (n < 1) return fail(CWT_EINVAL, "n must be >= 1");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) { return random_normal_impl<decltype(t)>(p, seed, offset, n, scale, out_dev); });
}

int cwt_ar1_filter(cwt_plan* p, const void* e_dev, int64_t tau, int64_t n, double g, void* out_dev) {
  if (!p || !e_dev || !out_dev) return fail(CWT_EINVAL, "NULL argument");
  if (n < 1 || tau < 0) return fail(CWT_EINVAL, "need n >= 1 and tau >= 0");
  if (!(std::fabs(g) < 1.0)) return fail(CWT_EINVAL, "the AR(1) coefficient must be inside (-1, 1)");
  if (e_dev == out_dev) return fail(CWT_EINVAL, "the filter cannot run in place");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) { return ar1_filter_impl<decltype(t)>(p, e_dev, tau, n, g, out_dev); });
}

int cwt_forward_fft_n(cwt_plan* p, const void* x_dev, int64_t n0, void* xhat_dev) {
  if (!p || !x_dev || !xhat_dev) return fail(CWT_EINVAL, "NULL argument");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) { return forward_fft_n_impl<decltype(t)>(p, x_dev, n0, xhat_dev); });
}

int cwt_transform_rows_n(cwt_plan* p, const void* xhat_dev, int64_t n0, int mother, double param, double dt,
                         const double* scales, int nrows, void* W_dev, int64_t ldw) {
  if (!p || !xhat_dev || !scales || !W_dev) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 1) return fail(CWT_EINVAL, "nrows must be >= 1");
  if (ldw < n0) return fail(CWT_EINVAL, "ldw must be >= n0");
  if (!(dt > 0) || !std::isfinite(dt)) return fail(CWT_EINVAL, "dt must be positive");
  if (mother < MOTHER_MORLET || mother > MOTHER_DOG) return fail(CWT_EINVAL, "unknown mother id");
  HIPCHECK(hipSetDevice(p->device));
  return by_precision(p, [&](auto t) {
    return transform_rows_n_impl<decltype(t)>(p, xhat_dev, n0, mother, param, dt, scales, nrows, W_dev, ldw);
  });
}

// The plan's page-locked staging buffer of cwt_execute_host (allocated on first use)
constexpr size_t kHostStage = size_t(4) << 20;
static int ensure_hstage(cwt_plan* p) {
  if (p->hstage_bytes >= kHostStage) return CWT_OK;
  if (hipHostMalloc(&p->hstage, kHostStage) != hipSuccess) return fail(CWT_ENOMEM, "pinned staging allocation failed");
  p->hstage_bytes = kHostStage;
  return CWT_OK;
}

// Page-locked host buffers handed out by cwt_host_malloc (start -> bytes): cwt_execute_host lets the kernels of a short
// transform write W straight into such a buffer.

int cwt_host_malloc(void** ptr_host, size_t bytes) {
  if (!ptr_host || !bytes) return fail(CWT_EINVAL, "NULL argument or zero size");
  void* q = nullptr;
  // (portable + mapped: a buffer serves the plans of every device of the process, whichever was current when it was made)
  if (hipHostMalloc(&q, bytes, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return fail(CWT_ENOMEM, "page-locked allocation failed"); }
  { std::lock_guard<std::mutex> lock(g_pinned_mutex); g_pinned[reinterpret_cast<uintptr_t>(q)] = bytes; }
  *ptr_host = q;
  return CWT_OK;
}

int cwt_host_free(void* ptr_host) {
  if (!ptr_host) return CWT_OK;
  {
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    auto it = g_pinned.find(reinterpret_cast<uintptr_t>(ptr_host));
    if (it == g_pinned.end()) return fail(CWT_EINVAL, "not a cwt_host_malloc buffer");
    g_pinned.erase(it);
  }
  HIPCHECK(hipHostFree(ptr_host));
  return CWT_OK;
}

// cwt_execute_host and cwt_execute_host_power: the same two host paths, for an output of ow = 2 (W) or 1 (power) reals per element
static int execute_host_entry(cwt_plan* p, const void* x_host, int64_t n0, int mother, double param, double dt,
                              const double* scales, int nrows, void* W_host, void* xhat_host, int power) {
  if (!p || !x_host || !scales) return fail(CWT_EINVAL, "NULL argument");
  if (n0 < 1 || n0 > p->N) return fail(CWT_EINVAL, "n0 must be in [1, nfft]");
  HIPCHECK(hipSetDevice(p->device));
  const size_t es = p->esize(), ow = power ? 1 : 2;
  // A transform that fits one workgroup per row (the reference's canonical 504-point call: 4 KB in, 0.8 MB out) is all
  // latency, and copy operations are the larger part of it.  Here it has none: the forward FFT reads the signal from the
  // plan's page-locked staging buffer, the row kernel writes W over PCIe itself -- into W_host when that is a
  // cwt_host_malloc buffer, else into the staging buffer (then one memcpy) -- and only the spectrum (nfft values) is
  // copied.  45 us against 83 at 504 x 97, fp64 [measured, profiles/r04_latency.txt; tools/microbench/host_latency.cpp].
  if (W_host && p->host_direct && !p->profile && p->logN > 3 && p->logN <= p->loglmax) {
    const size_t in_b = (size_t(n0) * es + 255) & ~size_t(255), xh_b = size_t(p->N) * 2 * es;
    const size_t w_b = size_t(nrows) * size_t(n0) * ow * es;
    const bool w_direct = is_pinned(W_host, w_b);
    if (in_b + xh_b + (w_direct ? 0 : w_b) <= kHostStage) {
      int rc = ensure_hstage(p);
      if (rc) return rc;
      if (p->auto_target > 0) p->tolerance = default_tolerance(p);   // (round-off costs such transforms nothing: no need to look)
      rc = grow(&p->hxhat, &p->hxhat_bytes, xh_b, p->stream);
      if (rc) return rc;
      char* stage = static_cast<char*>(p->hstage);
      std::memcpy(stage, x_host, size_t(n0) * es);
      void* W_out = w_direct ? W_host : stage + in_b + xh_b;
      rc = transform_entry(p, stage, n0, mother, param, dt, scales, nrows, p->hxhat, W_out, n0, n0, power);
      if (rc) return rc;
      if (xhat_host) HIPCHECK(hipMemcpyAsync(stage + in_b, p->hxhat, xh_b, hipMemcpyDeviceToHost, p->stream));
      HIPCHECK(hipStreamSynchronize(p->stream));
      if (xhat_host) std::memcpy(xhat_host, stage + in_b, xh_b);
      if (!w_direct) std::memcpy(W_host, W_out, w_b);
      return CWT_OK;
    }
  }
  int rc = grow(&p->hx, &p->hx_bytes, size_t(n0) * es, p->stream);
  if (!rc) rc = grow(&p->hxhat, &p->hxhat_bytes, size_t(p->N) * 2 * es, p->stream);
  if (!rc && W_host) rc = grow(&p->hW, &p->hW_bytes, size_t(nrows) * size_t(n0) * ow * es, p->stream);
  if (rc) return rc;
  // Small calls (the reference's canonical 504-point series: 4 KB in, 0.7 MB out) are all latency: a copy to or from pageable
  // memory makes the runtime stage and synchronise on its own, once per copy.  They go through ONE page-locked buffer of the
  // plan instead -- memcpy in, three asynchronous copies, one synchronisation, memcpy out.
  const size_t in_b = size_t(n0) * es, xh_b = xhat_host ? size_t(p->N) * 2 * es : 0;
  const size_t w_b = W_host ? size_t(nrows) * size_t(n0) * ow * es : 0;
  const bool staged = in_b + xh_b + w_b <= kHostStage;
  char* stage = nullptr;
  if (staged) {
    rc = ensure_hstage(p);
    if (rc) return rc;
    stage = static_cast<char*>(p->hstage);
    std::memcpy(stage, x_host, in_b);
    HIPCHECK(hipMemcpyAsync(p->hx, stage, in_b, hipMemcpyHostToDevice, p->stream));
  } else {
    HIPCHECK(hipMemcpyAsync(p->hx, x_host, in_b, hipMemcpyHostToDevice, p->stream));
  }
  if (W_host && p->auto_target > 0 && p->logN <= p->loglmax) {
    // single-workgroup transforms compute every bin of every row anyway: round-off costs nothing, no need to look
    p->tolerance = default_tolerance(p);
  } else if (W_host && p->auto_target > 0) {
    // accuracy target of THIS call = auto_target / (dynamic range of its spectrum relative to white noise), a power of
    // ten (so that calls with like spectra share one cached row table), never looser than the target itself
    rc = cwt_forward_fft(p, p->hx, n0, p->hxhat);
    double tol = 0;
    if (!rc) rc = cwt_plan_auto_tolerance(p, p->hxhat, p->auto_target, &tol);
    if (rc) return rc;
    p->tolerance = tol;
  }
  if (W_host) rc = transform_entry(p, p->hx, n0, mother, param, dt, scales, nrows, p->hxhat, p->hW, n0, n0, power);
  else rc = cwt_forward_fft(p, p->hx, n0, p->hxhat);
  if (rc) return rc;
  if (staged) {
    if (xh_b) HIPCHECK(hipMemcpyAsync(stage + in_b, p->hxhat, xh_b, hipMemcpyDeviceToHost, p->stream));
    if (w_b) HIPCHECK(hipMemcpyAsync(stage + in_b + xh_b, p->hW, w_b, hipMemcpyDeviceToHost, p->stream));
    HIPCHECK(hipStreamSynchronize(p->stream));
    if (xh_b) std::memcpy(xhat_host, stage + in_b, xh_b);
    if (w_b) std::memcpy(W_host, stage + in_b + xh_b, w_b);
    return CWT_OK;
  }
  if (xhat_host)
    HIPCHECK(hipMemcpyAsync(xhat_host, p->hxhat, size_t(p->N) * 2 * es, hipMemcpyDeviceToHost, p->stream));
  if (W_host) return copy_d2h(p, W_host, p->hW, size_t(nrows) * size_t(n0) * ow * es);
  HIPCHECK(hipStreamSynchronize(p->stream));
  return CWT_OK;
}

int cwt_execute_host(cwt_plan* p, const void* x_host, int64_t n0, int mother, double param, double dt,
                     const double* scales, int nrows, void* W_host, void* xhat_host) {
  return execute_host_entry(p, x_host, n0, mother, param, dt, scales, nrows, W_host, xhat_host, 0);
}

int cwt_execute_host_power(cwt_plan* p, const void* x_host, int64_t n0, int mother, double param, double dt,
                           const double* scales, int nrows, void* P_host, void* xhat_host) {
  return execute_host_entry(p, x_host, n0, mother, param, dt, scales, nrows, P_host, xhat_host, 1);
}

int cwt_plan_timings(cwt_plan* p, int cap, const char** names, double* total_ms, int* launches, int* n) {
  if (!p || !n) return fail(CWT_EINVAL, "NULL argument");
  HIPCHECK(hipStreamSynchronize(p->stream));
  double tot[KC_COUNT] = {0};
  int cnt[KC_COUNT] = {0};
  for (auto& t : p->timed) {
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, t.a, t.b));
    tot[t.cls] += ms;
    cnt[t.cls]++;
    p->free_events.push_back(t.a);
    p->free_events.push_back(t.b);
  }
  p->timed.clear();
  int k = 0;
  for (int c = 0; c < KC_COUNT; ++c) {
    if (!cnt[c]) continue;
    if (k < cap) {
      if (names) names[k] = kClassNames[c];
      if (total_ms) total_ms[k] = tot[c];
      if (launches) launches[k] = cnt[c];
    }
    ++k;
  }
  *n = k;
  return CWT_OK;
}

int cwt_plan_row_classes(cwt_plan* p, int* codes, int cap, int* n) {
  if (!p || !n) return fail(CWT_EINVAL, "NULL argument");
  const int total = int(p->rt->table.size());
  const int n_aux = p->rt->aux_first >= 0 ? p->rt->aols_nbatch : 0;
  *n = total - n_aux;
  if (!codes) return CWT_OK;
  for (int i = 0; i < total; ++i) {
    const RowDesc& rd = p->rt->table[i];
    // 0 single-workgroup, 1 band-limited, 2 band-limited K = 2048, 3 two-pass, 4 overlap-save, 5 overlap-save on half-size tiles
    const int small_end = p->rt->ols_first + (p->rt->ols_grp[0].logp != p->rt->ols_grp[1].logp ? p->rt->ols_grp[0].nrows : 0);
    if (n_aux && i >= p->rt->aux_first && i < p->rt->aux_first + n_aux) continue;      // the mask pseudo-rows of the k_aols rows
    // ... 6 overlap-save on the band-passed complex signal (rows clipped at Nyquist)
    // 7 band-limited row in polynomial form (logK = log2 of its interval count, nterms = its degree)
    const int kind = i < p->rt->n_small ? 0 : i < p->rt->wide_first ? (rd.logK == 11 ? 2 : 1) : i < p->rt->ols_first ? 3 :
                     i >= p->rt->poly_first ? 7 : i >= p->rt->aols_first ? 6 : i < small_end ? 5 : 4;
    if (rd.out_row >= 0 && rd.out_row < cap) codes[rd.out_row] = kind * 10000 + rd.logK * 100 + rd.nterms;
  }
  return CWT_OK;
}

int cwt_plan_classify(cwt_plan* p, int mother, double param, double dt, const double* scales, int nrows, int64_t ncols,
                      int with_signal, int* codes) {
  if (!p || !scales || !codes) return fail(CWT_EINVAL, "NULL argument");
  HIPCHECK(hipSetDevice(p->device));
  int rc = prepare_rows_table(p, with_signal != 0, mother, param, dt, scales, nrows, ncols, ncols);
  if (rc) return rc;
  int n = 0;
  return cwt_plan_row_classes(p, codes, nrows, &n);
}


int cwt_shard_codes(const int* codes, int nrows, int precision, double nscale, int chunk_rows, int world, int* first,
                    int* count) {
  if (!codes || !first || !count) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 0 || world < 1 || (precision != 32 && precision != 64) || !(nscale > 0) || chunk_rows < 1)
    return fail(CWT_EINVAL, "bad shard arguments");
  const ShardCost& c = precision == 64 ? kShardCost64 : kShardCost32;
  const int n = nrows;
  std::vector<int> bounds(size_t(world) + 1, n);
  bounds[0] = 0;
  if (world > 1 && n > 0) {
    // largest shard minimised by bisection on the limit: greedy fill of contiguous shards (cost is monotone in hi)
    auto cuts_for = [&](double limit, std::vector<int>* out) {
      int lo = 0;
      for (int r = 0; r < world; ++r) {
        int a = lo, b = n;
        while (a < b) {
          const int m = (a + b + 1) / 2;
          if (shard_cost(codes, lo, m, c, nscale, chunk_rows) <= limit) a = m; else b = m - 1;
        }
        const int hi = lo < n ? std::max(a, lo + 1) : lo;
        if (out) (*out)[size_t(r) + 1] = std::min(hi, n);
        lo = std::min(hi, n);
      }
      return lo >= n;
    };
    double lo_t = 0, hi_t = shard_cost(codes, 0, n, c, nscale, chunk_rows);
    for (int it = 0; it < 40; ++it) {
      const double mid = 0.5 * (lo_t + hi_t);
      if (cuts_for(mid, nullptr)) hi_t = mid; else lo_t = mid;
    }
    cuts_for(hi_t, &bounds);
    bounds[size_t(world)] = n;
    // the greedy fill leaves the slack in the last shard and may strand one or two rows of a kernel class in a shard:
    // move every boundary by up to 4 rows where that lowers the larger of the two neighbouring shards
    for (int pass = 0; pass < 3; ++pass)
      for (int i = 1; i < world; ++i) {
        const int lo = bounds[size_t(i) - 1], hi = bounds[size_t(i) + 1];
        int best = bounds[size_t(i)];
        double best_cost = -1;
        for (int b = std::max(lo, bounds[size_t(i)] - 4); b <= std::min(hi, bounds[size_t(i)] + 4); ++b) {
          const double cost = std::max(shard_cost(codes, lo, b, c, nscale, chunk_rows), shard_cost(codes, b, hi, c, nscale, chunk_rows));
          if (best_cost < 0 || cost < best_cost - 1e-9) { best = b; best_cost = cost; }
        }
        bounds[size_t(i)] = best;
      }
  }
  for (int r = 0; r < world; ++r) { first[r] = bounds[size_t(r)]; count[r] = bounds[size_t(r) + 1] - bounds[size_t(r)]; }
  return CWT_OK;
}

int cwt_shard_cost(const int* codes, int nrows, int precision, double nscale, int chunk_rows, double* cost_us) {
  if (!codes || !cost_us) return fail(CWT_EINVAL, "NULL argument");
  if (nrows < 0 || (precision != 32 && precision != 64) || !(nscale > 0) || chunk_rows < 1)
    return fail(CWT_EINVAL, "bad shard arguments");
  *cost_us = shard_cost(codes, 0, nrows, precision == 64 ? kShardCost64 : kShardCost32, nscale, chunk_rows);
  return CWT_OK;
}

int cwt_plan_balanced_shards(cwt_plan* p, int mother, double param, double dt, const double* scales, int nrows,
                             int64_t ncols, int world, int* first, int* count) {
  if (!p || !scales || !first || !count) return fail(CWT_EINVAL, "NULL argument");
  std::vector<int> codes(size_t(std::max(nrows, 1)));
  int rc = cwt_plan_classify(p, mother, param, dt, scales, nrows, ncols, 1, codes.data());
  if (rc) return rc;
  return cwt_shard_codes(codes.data(), nrows, p->prec, double(p->N) / double(1 << 20), chunk_rows_of(p), world, first, count);
}

int cwt_plan_last_split(cwt_plan* p, int counts[6]) {
  if (!p || !counts) return fail(CWT_EINVAL, "NULL argument");
  for (int i = 0; i < 6; ++i) counts[i] = p->split[i];
  return CWT_OK;
}

int cwt_plan_last_split8(cwt_plan* p, int counts[8]) {
  if (!p || !counts) return fail(CWT_EINVAL, "NULL argument");
  for (int i = 0; i < 8; ++i) counts[i] = p->split[i];
  return CWT_OK;
}

}  // extern "C"
