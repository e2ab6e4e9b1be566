// ssq_gather.hip -- the shape of ssqg_gather (pycwt_amd/csrc/cwt_kernels_ssq_grad.hpp) measured alone: G[j, n] = w_j gT[bins[j, n], n]
// over 256 x 2^20 entries in double, for stretches of R rows per thread, workgroups of THREADS lanes along n, plain or non-temporal
// stores of G, and three maps: uniformly random bins (every entry changes cell), all dropped (bins read, zeros written), one bin
// for all (one cell per stretch).  Beside them a plain fill of G (the write stream alone).  Medians of 20 alternated rounds.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/microbench/ssq_gather.hip -o tools/microbench/ssq_gather && tools/microbench/ssq_gather
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(e)                                                                             \
  do {                                                                                       \
    hipError_t e_ = (e);                                                                     \
    if (e_ != hipSuccess) {                                                                  \
      std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(e_));                           \
      std::exit(1);                                                                          \
    }                                                                                        \
  } while (0)

typedef double vec2 __attribute__((vector_size(16)));

template <int R, int THREADS, bool NT>
__global__ void __launch_bounds__(THREADS)
gather(const vec2* __restrict__ gT, long ldt, int nf, const short* __restrict__ bins, long ldb, const double* __restrict__ w, int nrows,
       long ncols, vec2* __restrict__ G, long ldg) {
  const long n = long(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n >= ncols) return;
  const long j0 = long(blockIdx.y) * R;
  int k[R];
#pragma unroll
  for (int u = 0; u < R; ++u) k[u] = j0 + u < nrows ? int(__builtin_nontemporal_load(bins + (j0 + u) * ldb + n)) : -1;
  int cur = -1;
  vec2 cell = {0.0, 0.0};
#pragma unroll
  for (int u = 0; u < R; ++u) {
    if (j0 + u >= nrows) break;
    vec2 g = {0.0, 0.0};
    if (k[u] >= 0 && k[u] < nf) {
      if (k[u] != cur) {
        cur = k[u];
        cell = gT[long(cur) * ldt + n];
      }
      g = cell * w[j0 + u];
    }
    if (NT) __builtin_nontemporal_store(g, G + (j0 + u) * ldg + n);
    else G[(j0 + u) * ldg + n] = g;
  }
}

__global__ void fill(vec2* __restrict__ G, long ld, long ncols) {
  const long n = long(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n < ncols) G[long(blockIdx.y) * ld + n] = vec2{0.0, 0.0};
}

struct Variant {
  const char* name;
  void (*launch)(const vec2*, int, const short*, const double*, int, long, vec2*);
};

template <int R, int THREADS, bool NT>
void launch(const vec2* gT, int nf, const short* bins, const double* w, int rows, long N, vec2* G) {
  hipLaunchKernelGGL((gather<R, THREADS, NT>), dim3(unsigned((N + THREADS - 1) / THREADS), unsigned((rows + R - 1) / R)), dim3(THREADS), 0, 0, gT,
                     N, nf, bins, N, w, rows, N, G, N);
}

int main() {
  const long N = 1 << 20;
  const int rows = 256, nf = 256, reps = 20;
  vec2 *gT, *G;
  short* maps[3];
  double* w;
  CHECK(hipMalloc(&gT, size_t(nf) * N * 16));
  CHECK(hipMalloc(&G, size_t(rows) * N * 16));
  CHECK(hipMalloc(&w, rows * 8));
  CHECK(hipMemset(gT, 0, size_t(nf) * N * 16));
  std::vector<double> wh(rows, 0.5);
  CHECK(hipMemcpy(w, wh.data(), rows * 8, hipMemcpyHostToDevice));
  std::vector<short> h(size_t(rows) * N);
  const char* map_names[3] = {"random", "dropped", "one bin"};
  unsigned long long s = 88172645463325252ull;
  for (int m = 0; m < 3; ++m) {
    for (auto& v : h) {
      s ^= s << 13, s ^= s >> 7, s ^= s << 17;
      v = m == 0 ? short(s % nf) : m == 1 ? short(-1) : short(7);
    }
    CHECK(hipMalloc(&maps[m], h.size() * 2));
    CHECK(hipMemcpy(maps[m], h.data(), h.size() * 2, hipMemcpyHostToDevice));
  }
  const Variant vs[] = {{"R 8  T 128 plain", launch<8, 128, false>},  {"R 8  T 128 nt   ", launch<8, 128, true>},
                        {"R 8  T 256 plain", launch<8, 256, false>},  {"R 8  T 256 nt   ", launch<8, 256, true>},
                        {"R 4  T 128 plain", launch<4, 128, false>},  {"R 4  T 128 nt   ", launch<4, 128, true>},
                        {"R 16 T 128 plain", launch<16, 128, false>}, {"R 16 T 128 nt   ", launch<16, 128, true>},
                        {"R 2  T 256 plain", launch<2, 256, false>},  {"R 1  T 256 plain", launch<1, 256, false>}};
  const int nv = int(sizeof(vs) / sizeof(vs[0]));
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a));
  CHECK(hipEventCreate(&b));
  std::vector<std::vector<float>> t(nv * 3 + 1);
  for (int r = -3; r < reps; ++r) {
    for (int i = 0; i <= nv * 3; ++i) {
      CHECK(hipEventRecord(a, 0));
      if (i == nv * 3) hipLaunchKernelGGL(fill, dim3(unsigned(N / 256), rows), dim3(256), 0, 0, G, N, N);
      else vs[i / 3].launch(gT, nf, maps[i % 3], w, rows, N, G);
      CHECK(hipEventRecord(b, 0));
      CHECK(hipEventSynchronize(b));
      float ms;
      CHECK(hipEventElapsedTime(&ms, a, b));
      if (r >= 0) t[i].push_back(ms);
    }
  }
  auto med = [](std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return 0.5f * (v[v.size() / 2] + v[(v.size() - 1) / 2]);
  };
  std::printf("ssqg_gather shapes, 256 x 2^20 entries, double, 256 bins; median ms of %d alternated rounds\n%-18s", reps, "variant");
  for (int m = 0; m < 3; ++m) std::printf(" %10s", map_names[m]);
  std::printf("\n");
  for (int v = 0; v < nv; ++v) {
    std::printf("%-18s", vs[v].name);
    for (int m = 0; m < 3; ++m) std::printf(" %10.3f", med(t[v * 3 + m]));
    std::printf("\n");
  }
  std::printf("%-18s %10.3f   (4.29 GB of zeros, one element per thread)\n", "plain fill of G", med(t[nv * 3]));
  return 0;
}
