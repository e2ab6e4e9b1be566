// TEST INFRASTRUCTURE ONLY -- fiber scheduler behind tests/emu/hip/hip_runtime.h.
//
// A workgroup is a set of fibers; a fiber parks at a workgroup barrier (__syncthreads) or at a wave barrier
// (__builtin_amdgcn_wave_barrier).  The interval between two workgroup barriers is an EPOCH.  Schedules:
//   lockstep       every live fiber in thread order, again and again; both barriers just end a fiber's turn.  A wave
//                  barrier therefore orders ALL waves of the workgroup, and a fiber always finds the work of the lower
//                  thread ids done: two things the hardware does not promise.
//   waves          one wavefront (64 consecutive linear thread ids) at a time: its fibers run, passing their wave barriers as
//                  soon as every live fiber of the wave is parked, until all of them wait at the workgroup barrier or have
//                  finished; only then the next wave starts.  Legal on the hardware, and the worst case for code that leans on
//                  a wave barrier between waves.  Waves 0, 1, ... and lanes 0 ... 63.
//   waves-reverse  the same with the waves from last to first and the lanes from 63 to 0.
//   waves-seeded   the same with a permutation of the waves and of the lanes of each wave, redrawn every epoch from a
//                  counter-based generator keyed by (seed, workgroup, epoch): reproducible whichever OS thread runs the workgroup.
// Under the wave schedules the LDS of a workgroup starts as all-ones bytes (NaN), not as what the previous one left there.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <mutex>
#include <numeric>
#include <set>
#include <string>

namespace hipemu {
thread_local Ctx* cur = nullptr;

namespace {
constexpr size_t kStack = 96 * 1024;

struct Worker {
  std::vector<ucontext_t> fibers;
  std::vector<Ctx> ctx;
  std::unique_ptr<char[]> stacks;        // not zero-filled: a fiber touches the few pages of its stack that it uses
  size_t stacks_size = 0;
  std::vector<char> smem;
  ucontext_t sched;
};

thread_local const std::function<void()>* g_body = nullptr;

void trampoline() {
  (*g_body)();
  cur->done = true;
  swapcontext(cur->self, cur->sched);
}

struct Schedule { int kind; unsigned seed; };
std::atomic<int> g_kind{HIPEMU_LOCKSTEP};
std::atomic<unsigned> g_seed{0};

void run_lockstep(Worker& w, unsigned nt) {
  unsigned alive = nt;
  while (alive) {
    unsigned finished = 0;
    for (unsigned t = 0; t < nt; ++t) {
      if (w.ctx[t].done) continue;
      cur = &w.ctx[t];
      swapcontext(&w.sched, &w.fibers[t]);
      if (w.ctx[t].done) ++finished;
    }
    alive -= finished;
    if (finished && alive) {
      fprintf(stderr, "hipemu: %u threads left a block early while %u still run (barrier divergence)\n",
              finished, alive);
      abort();
    }
  }
}

// counter-based generator: splitmix64's finaliser over (key, counter)
inline uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
void permute(unsigned* v, unsigned n, uint64_t key, uint64_t& counter) {      // Fisher-Yates
  for (unsigned i = n; i > 1; --i) std::swap(v[i - 1], v[mix64(key ^ mix64(counter++)) % i]);
}

void run_waves(Worker& w, unsigned nt, Schedule sch, char* smem, size_t shmem, uint64_t block_id) {
  constexpr unsigned kWave = 64;
  const unsigned nw = (nt + kWave - 1) / kWave;
  memset(smem, 0xFF, shmem);
  std::vector<unsigned> worder(nw), lorder(nt);                 // waves in their order; the thread ids of wave v at lorder[64 v ...]
  unsigned alive = nt;
  for (uint64_t epoch = 0; alive; ++epoch) {
    std::iota(worder.begin(), worder.end(), 0u);
    std::iota(lorder.begin(), lorder.end(), 0u);
    if (sch.kind == HIPEMU_WAVES_REVERSE) {
      std::reverse(worder.begin(), worder.end());
      for (unsigned v = 0; v < nw; ++v) std::reverse(lorder.begin() + v * kWave, lorder.begin() + std::min(nt, (v + 1) * kWave));
    } else if (sch.kind == HIPEMU_WAVES_SEEDED) {
      const uint64_t key = mix64(mix64(mix64(sch.seed) ^ block_id) ^ epoch);
      uint64_t counter = 0;
      permute(worder.data(), nw, key, counter);
      for (unsigned v = 0; v < nw; ++v) permute(lorder.data() + v * kWave, std::min(nt, (v + 1) * kWave) - v * kWave, key, counter);
    }
    unsigned finished = 0;
    for (unsigned v : worder) {
      const unsigned* lanes = lorder.data() + v * kWave;
      const unsigned nl = std::min(nt, (v + 1) * kWave) - v * kWave;
      for (;;) {
        for (unsigned i = 0; i < nl; ++i) {
          Ctx& c = w.ctx[lanes[i]];
          if (c.done || c.park != kReady) continue;
          cur = &c;
          swapcontext(&w.sched, &w.fibers[lanes[i]]);
          if (c.done) ++finished;
        }
        unsigned at_wave = 0, at_block = 0;
        for (unsigned i = 0; i < nl; ++i) {
          const Ctx& c = w.ctx[lanes[i]];
          if (!c.done) (c.park == kAtWave ? at_wave : at_block) += 1;
        }
        if (!at_wave) break;                                     // the wave waits at the workgroup barrier, or is through
        if (at_block) {
          fprintf(stderr, "hipemu: wave %u: %u threads wait at a wave barrier while %u wait at the workgroup barrier "
                  "(wave barrier divergence)\n", v, at_wave, at_block);
          abort();
        }
        for (unsigned i = 0; i < nl; ++i) w.ctx[lanes[i]].park = kReady;
      }
    }
    alive -= finished;
    if (finished && alive) {
      fprintf(stderr, "hipemu: %u threads left a block early while %u still run (barrier divergence)\n",
              finished, alive);
      abort();
    }
    for (unsigned t = 0; t < nt; ++t) w.ctx[t].park = kReady;
  }
}

void run_block(Worker& w, Schedule sch, dim3 grid, dim3 block, size_t shmem, unsigned bx, unsigned by,
               const std::function<void()>& body) {
  const unsigned nt = block.x * block.y * block.z;
  if (w.fibers.size() < nt) {
    w.fibers.resize(nt);
    w.ctx.resize(nt);
  }
  if (w.stacks_size < size_t(nt) * kStack) {
    w.stacks_size = size_t(nt) * kStack;
    w.stacks.reset(new char[w.stacks_size]);
  }
  if (w.smem.size() < shmem + 64) w.smem.resize(shmem + 64);
  char* smem = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(w.smem.data()) + 63) & ~uintptr_t(63));
  g_body = &body;
  for (unsigned t = 0; t < nt; ++t) {
    Ctx& c = w.ctx[t];
    c.tid = dim3(t % block.x, (t / block.x) % block.y, t / (block.x * block.y));
    c.bid = dim3(bx, by, 0);
    c.bdim = block;
    c.gdim = grid;
    c.smem = smem;
    c.self = &w.fibers[t];
    c.sched = &w.sched;
    c.done = false;
    c.park = kReady;
    getcontext(&w.fibers[t]);
    w.fibers[t].uc_stack.ss_sp = w.stacks.get() + size_t(t) * kStack;
    w.fibers[t].uc_stack.ss_size = kStack;
    w.fibers[t].uc_link = &w.sched;
    makecontext(&w.fibers[t], trampoline, 0);
  }
  if (sch.kind == HIPEMU_LOCKSTEP) run_lockstep(w, nt);
  else run_waves(w, nt, sch, smem, shmem, uint64_t(by) * grid.x + bx);
  cur = nullptr;
}
}  // namespace

namespace {
std::mutex g_log_mutex;
std::set<std::string> g_launched;
}  // namespace

void launch(const char* name, dim3 grid, dim3 block, size_t shmem, const std::function<void()>& body) {
  {
    std::lock_guard<std::mutex> lock(g_log_mutex);
    g_launched.insert(name);
  }
  const Schedule sch{g_kind.load(), g_seed.load()};
  const unsigned nblocks = grid.x * grid.y;
  unsigned nthreads = std::thread::hardware_concurrency();
  if (nthreads == 0) nthreads = 4;
  if (nthreads > nblocks) nthreads = nblocks;
  std::atomic<unsigned> next{0};
  auto work = [&]() {
    Worker w;
    for (;;) {
      unsigned b = next.fetch_add(1);
      if (b >= nblocks) break;
      run_block(w, sch, grid, block, shmem, b % grid.x, b / grid.x, body);
    }
  };
  if (nthreads <= 1) {
    work();
  } else {
    std::vector<std::thread> pool;
    for (unsigned i = 0; i < nthreads; ++i) pool.emplace_back(work);
    for (auto& t : pool) t.join();
  }
}
}  // namespace hipemu

double hipemu_now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

int hipemu_set_schedule(int kind, unsigned seed) {
  if (kind < HIPEMU_LOCKSTEP || kind > HIPEMU_WAVES_SEEDED) return -1;
  hipemu::g_kind.store(kind);
  hipemu::g_seed.store(seed);
  return 0;
}
void hipemu_get_schedule(int* kind, unsigned* seed) {
  *kind = hipemu::g_kind.load();
  *seed = hipemu::g_seed.load();
}
void hipemu_clear_launched() {
  std::lock_guard<std::mutex> lock(hipemu::g_log_mutex);
  hipemu::g_launched.clear();
}
size_t hipemu_launched(char* buf, size_t size) {
  std::lock_guard<std::mutex> lock(hipemu::g_log_mutex);
  std::string all;
  for (const std::string& s : hipemu::g_launched) all += s + "\n";
  if (buf && size) {
    const size_t n = std::min(size - 1, all.size());
    memcpy(buf, all.data(), n);
    buf[n] = 0;
  }
  return all.size() + 1;
}

namespace {
// CWT_EMU_SCHEDULE at load time; a value that is none of the four is an error, not a silent lockstep run
struct ScheduleFromEnv {
  ScheduleFromEnv() {
    const char* e = std::getenv("CWT_EMU_SCHEDULE");
    if (!e || !*e) return;
    const std::string v(e);
    char* end = nullptr;
    if (v == "lockstep") hipemu_set_schedule(HIPEMU_LOCKSTEP, 0);
    else if (v == "waves") hipemu_set_schedule(HIPEMU_WAVES, 0);
    else if (v == "waves-reverse") hipemu_set_schedule(HIPEMU_WAVES_REVERSE, 0);
    else if (v.rfind("waves-seeded:", 0) == 0 && v.size() > 13 &&
             (hipemu_set_schedule(HIPEMU_WAVES_SEEDED, unsigned(strtoul(e + 13, &end, 10))), *end == 0)) {}
    else {
      fprintf(stderr, "hipemu: CWT_EMU_SCHEDULE=%s is not lockstep | waves | waves-reverse | waves-seeded:<n>\n", e);
      abort();
    }
  }
} g_schedule_from_env;
}  // namespace
