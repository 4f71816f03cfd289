// Tuning aid: the design of aivc_pair_sad_u8 that was NOT taken (experiments/scene_cut.md).  A workgroup owns a byte range of
// the plane and walks the frames: every thread keeps its chunks of frame t - 1 in registers and the loads of the next D - 1
// frames in flight, so every byte of the clip is loaded exactly once; one partial per wavefront and pair, no fold here (the
// host adds them when it checks the sums).  Aligned 1080p planes only; the product kernel's grid runs over (stripe, pair)
// and leaves the second read of a plane to the cache (csrc/scene.hip).
// Prints, per (chunks per thread V, ring depth D): workgroups, ms per walk warm (20 walks back to back, median of 7 windows)
// and cold (a single walk behind a 1 GiB fill, median of 7), TB/s, and whether the sums equal the host's.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/sad_walk_probe.hip -o sad_walk_probe ; run: ./sad_walk_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#define CHECK(x)                                                                    \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) {                                                         \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));    \
      exit(1);                                                                      \
    }                                                                               \
  } while (0)

typedef uint32_t chunk_t __attribute__((ext_vector_type(4)));
typedef const chunk_t __attribute__((address_space(1))) *chunk_ptr;

__device__ __forceinline__ uint32_t sad16(const chunk_t &x, const chunk_t &y, uint32_t acc) {
  acc = __builtin_amdgcn_sad_u8(x.x, y.x, acc);
  acc = __builtin_amdgcn_sad_u8(x.y, y.y, acc);
  acc = __builtin_amdgcn_sad_u8(x.z, y.z, acc);
  return __builtin_amdgcn_sad_u8(x.w, y.w, acc);
}

// thread (block b, tid) owns chunks (b * V + k) * 256 + tid, k < V.  partials: [n - 1][gridDim.x * 4] uint32 (one per wavefront)
template <int V, int D>
__global__ void __launch_bounds__(256) walk_kernel(const uint8_t *const *__restrict__ planes, int n, size_t nvec,
                                                   uint32_t *__restrict__ partials) {
  size_t idx[V];
  bool in[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    idx[k] = ((size_t)blockIdx.x * V + k) * 256 + threadIdx.x;
    in[k] = idx[k] < nvec;
  }
  chunk_t ring[D][V];
  auto load = [&](int slot, int f) {
    chunk_ptr p = (chunk_ptr)planes[f < n ? f : n - 1];  // (behind the clip: a load that is never summed)
#pragma unroll
    for (int k = 0; k < V; ++k) ring[slot][k] = in[k] ? p[idx[k]] : chunk_t{0u, 0u, 0u, 0u};
  };
#pragma unroll
  for (int d = 0; d < D; ++d) load(d, d);
  const size_t row = (size_t)gridDim.x * 4;
  for (int f0 = 1; f0 < n; f0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {  // frame f = f0 + d sits in slot (d + 1) % D, frame f - 1 in slot d
      const int f = f0 + d;
      if (f >= n) break;
      uint32_t s = 0;
#pragma unroll
      for (int k = 0; k < V; ++k) s = sad16(ring[d][k], ring[(d + 1) % D][k], s);
      load(d, f + D - 1);  // slot d (frame f - 1) is free now
#pragma unroll
      for (int sh = 32; sh >= 1; sh >>= 1) s += __shfl_down(s, sh, 64);
      if ((threadIdx.x & 63) == 0) partials[(size_t)(f - 1) * row + blockIdx.x * 4 + (threadIdx.x >> 6)] = s;
    }
  }
}

template <int V, int D>
static void run(const uint8_t *const *d_table, const std::vector<uint64_t> &want, int n, size_t len, uint8_t *flush, size_t flush_bytes) {
  const size_t nvec = len / 16;
  const int blocks = (int)((nvec + 256 * V - 1) / (256 * V));
  const size_t row = (size_t)blocks * 4;
  uint32_t *d_part;
  CHECK(hipMalloc(&d_part, (size_t)(n - 1) * row * 4));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  auto timed = [&](int calls) {
    CHECK(hipEventRecord(e0));
    for (int c = 0; c < calls; ++c) hipLaunchKernelGGL((walk_kernel<V, D>), dim3(blocks), dim3(256), 0, 0, d_table, n, nvec, d_part);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    return ms / calls;
  };
  std::vector<float> warm, cold;
  for (int r = 0; r < 8; ++r) {  // (the first round warms up and is dropped)
    const float w = timed(20);
    CHECK(hipMemsetAsync(flush, r, flush_bytes));
    const float c = timed(1);
    if (r) warm.push_back(w), cold.push_back(c);
  }
  std::vector<uint32_t> part((size_t)(n - 1) * row);
  CHECK(hipMemcpy(part.data(), d_part, part.size() * 4, hipMemcpyDeviceToHost));
  bool ok = true;
  for (int p = 0; p < n - 1; ++p) {
    uint64_t s = 0;
    for (size_t j = 0; j < row; ++j) s += part[(size_t)p * row + j];
    ok = ok && s == want[p];
  }
  std::sort(warm.begin(), warm.end());
  std::sort(cold.begin(), cold.end());
  const double bytes = (double)n * len;
  printf("V=%d D=%d workgroups=%d warm_ms=%.4f cold_ms=%.4f warm_TBps=%.2f cold_TBps=%.2f sums_%s\n", V, D, blocks, warm[warm.size() / 2],
         cold[cold.size() / 2], bytes / (warm[warm.size() / 2] * 1e-3) / 1e12, bytes / (cold[cold.size() / 2] * 1e-3) / 1e12,
         ok ? "ok" : "WRONG");
  CHECK(hipFree(d_part));
}

int main() {
  const int n = 129;
  const size_t len = (size_t)1920 * 1080;
  std::vector<std::vector<uint8_t>> host(n, std::vector<uint8_t>(len));
  uint32_t x = 12345u;
  for (auto &p : host)
    for (auto &b : p) b = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
  std::vector<uint64_t> want(n - 1, 0);
  for (int p = 0; p < n - 1; ++p)
    for (size_t j = 0; j < len; ++j) want[p] += (uint64_t)abs((int)host[p + 1][j] - (int)host[p][j]);
  std::vector<const uint8_t *> table(n);
  for (int p = 0; p < n; ++p) {
    uint8_t *d;
    CHECK(hipMalloc(&d, len));
    CHECK(hipMemcpy(d, host[p].data(), len, hipMemcpyHostToDevice));
    table[p] = d;
  }
  const uint8_t **d_table;
  CHECK(hipMalloc(&d_table, n * sizeof(void *)));
  CHECK(hipMemcpy(d_table, table.data(), n * sizeof(void *), hipMemcpyHostToDevice));
  const size_t flush_bytes = (size_t)1 << 30;
  uint8_t *flush;
  CHECK(hipMalloc(&flush, flush_bytes));
  run<1, 2>(d_table, want, n, len, flush, flush_bytes);
  run<1, 4>(d_table, want, n, len, flush, flush_bytes);
  run<1, 8>(d_table, want, n, len, flush, flush_bytes);
  run<2, 4>(d_table, want, n, len, flush, flush_bytes);
  run<2, 8>(d_table, want, n, len, flush, flush_bytes);
  run<4, 4>(d_table, want, n, len, flush, flush_bytes);
  return 0;
}
