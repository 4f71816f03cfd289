// Tuning aid: the design of aivc_resize_u8 that was NOT taken (experiments/resize.md).  One launch: a workgroup owns 16 output
// rows x 256 output columns of a plane, runs the horizontal pass over the input rows its output rows need into LDS (rounded
// to uint8, as the contract wants) and the vertical pass out of LDS, so the intermediate never leaves the CU -- at the price
// of the rows two neighbouring tiles both need (38 input rows per 16 output rows for 2:1 bicubic, 42 for lanczos), which are
// staged and filtered twice.  The product runs two launches with the intermediate in a
// global buffer (csrc/resize.hip).  Aligned planes of one clip only; the tap loops are the product's.
// KNOWN DEFECT: on the device its bytes differ from the host's statement (about half of them in the 2:1 bicubic case) although the
// same source is right when run on a CPU, a thread per work-item; the cause has not been found.  Its times measure the design's
// amount of work, nothing more.  PROBE_VERBOSE=1 prints where the planes differ and checks a plain one-thread-per-sample kernel.
// Prints, per case (2160p -> 1080p and 1080p -> 2160p luma, bicubic and lanczos, 129 planes): ms per clip (median of 7 windows
// behind a warm-up), TB/s over input + output bytes, and whether plane 0 and the last plane equal the host's statement.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/resize_fused_probe.hip -o resize_fused_probe ; run: ./resize_fused_probe
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#define CHECK(x)                                                                 \
  do {                                                                           \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) {                                                      \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(1);                                                                   \
    }                                                                            \
  } while (0)

constexpr int TX = 64, TY = 4, COLS = 4, ROWS = 4, TILE_W = TX * COLS, TILE_H = TY * ROWS;
constexpr int MAX_IN_ROWS = 64;  // input rows of a tile (42 for 2:1 lanczos)
typedef uint32_t chunk_t __attribute__((ext_vector_type(4)));
typedef int32_t int4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t lds_load4(const uint8_t *lds, uint32_t at) {  // any alignment, out of two aligned words
  const uint32_t *w = (const uint32_t *)lds + (at >> 2);
  return __builtin_amdgcn_alignbyte(w[1], w[0], at & 3u);
}
__device__ __forceinline__ uint32_t clip8(int32_t acc) {
  const int32_t v = acc >> 22;
  return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// planes: n aligned planes back to back; tables in the layout of include/aivc_hip_resize.h.  grid (tiles_y * n, tiles_x).
// LDS: in_rows * lds_pitch bytes of staged input, then in_rows * TILE_W bytes of the horizontal pass's result.
__global__ void __launch_bounds__(TX *TY) fused_kernel(const uint8_t *__restrict__ planes, int h_in, int w_in, int h_out, int w_out,
                                                        int tiles_y, const int32_t *__restrict__ xb, const int32_t *__restrict__ xk,
                                                        int x_taps, int xpitch, int lds_pitch, const int32_t *__restrict__ yb,
                                                        const int32_t *__restrict__ yk, int ypitch, int in_rows,
                                                        uint8_t *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint8_t *mid = lds + (size_t)in_rows * lds_pitch;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const size_t p = blockIdx.x / (unsigned)tiles_y;
  const int y0 = (int)(blockIdx.x - p * (unsigned)tiles_y) * TILE_H, x0 = blockIdx.y * TILE_W;
  const int yl = min(y0 + TILE_H - 1, h_out - 1), xl = min(x0 + TILE_W - 1, w_out - 1);
  const int r0 = yb[2 * y0], nr = yb[2 * yl] + yb[2 * yl + 1] - r0;  // input rows r0 ... r0 + nr - 1, nr <= in_rows
  const int s0 = xb[2 * x0], need = min(xb[2 * xl] + x_taps, w_in) - s0;
  const uint8_t *src = planes + p * (size_t)h_in * w_in;
  for (int rr = ty; rr < nr; rr += TY) {  // (planes and rows are 16-byte aligned here: w_in % 16 == 0)
    const uint8_t *g = src + (size_t)(r0 + rr) * w_in + s0;
    const int sh = (int)((uintptr_t)g & 15), nch = (sh + need + 15) >> 4;
    const chunk_t *a = (const chunk_t *)(g - sh);
    chunk_t *l = (chunk_t *)(lds + (size_t)rr * lds_pitch);
    for (int c = tx; c < nch; c += TX) l[c] = a[c];
  }
  __syncthreads();
  const int xq = x0 + tx * COLS;
  int off[COLS];
#pragma unroll
  for (int j = 0; j < COLS; ++j) off[j] = xb[2 * min(xq + j, w_out - 1)] - s0;
  const bool kin = xq < xpitch;
  for (int g0 = ty * ROWS; g0 < nr; g0 += TY * ROWS) {  // four rows at a time, as the product's horizontal pass
    int32_t acc[ROWS][COLS];
    int shift[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      shift[r] = (int)((uintptr_t)(src + (size_t)(r0 + min(g0 + r, nr - 1)) * w_in + s0) & 15);
#pragma unroll
      for (int j = 0; j < COLS; ++j) acc[r][j] = 1 << 21;
    }
    for (int k = 0; k < x_taps; k += 4) {
      int4_t kq[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) kq[t] = kin ? *(const int4_t *)(xk + (size_t)(k + t) * xpitch + xq) : int4_t{0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const uint32_t at = (uint32_t)(min(g0 + r, nr - 1) * lds_pitch + shift[r] + k);
#pragma unroll
        for (int j = 0; j < COLS; ++j) {
          const uint32_t v = lds_load4(lds, at + off[j]);
          int32_t a = acc[r][j];
          a += __mul24((int)(v & 255u), kq[0][j]);
          a += __mul24((int)((v >> 8) & 255u), kq[1][j]);
          a += __mul24((int)((v >> 16) & 255u), kq[2][j]);
          acc[r][j] = a + __mul24((int)(v >> 24), kq[3][j]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
      if (g0 + r < nr)
        *(uint32_t *)(mid + (size_t)(g0 + r) * TILE_W + tx * COLS) =
            clip8(acc[r][0]) | clip8(acc[r][1]) << 8 | clip8(acc[r][2]) << 16 | clip8(acc[r][3]) << 24;
  }
  __syncthreads();
  if (xq >= w_out) return;  // (w_out % 4 == 0 here)
  uint8_t *d = out + p * (size_t)h_out * w_out;
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int y = y0 + ty * ROWS + r;
    if (y >= h_out) break;
    const int first = yb[2 * y] - r0, count = yb[2 * y + 1];
    int32_t acc[COLS] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
    for (int k = 0; k < count; ++k) {
      const uint32_t v = *(const uint32_t *)(mid + (size_t)(first + k) * TILE_W + tx * COLS);
      const int32_t kk = yk[(size_t)k * ypitch + y];
#pragma unroll
      for (int j = 0; j < COLS; ++j) acc[j] += __mul24((int)((v >> (8 * j)) & 255u), kk);
    }
    *(uint32_t *)(d + (size_t)y * w_out + xq) = clip8(acc[0]) | clip8(acc[1]) << 8 | clip8(acc[2]) << 16 | clip8(acc[3]) << 24;
  }
}

// the plainest form of one pass, a thread per output sample: a second opinion on the device (PROBE_VERBOSE)
__global__ void plain_pass_kernel(const uint8_t *in, size_t rows, int n_in, int n_out, const int32_t *b, const int32_t *k, int pitch,
                                  uint8_t *out, size_t in_rs, size_t in_cs, size_t out_rs, size_t out_cs) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * n_out) return;
  const size_t r = i / n_out;
  const int xx = (int)(i - r * n_out);
  int32_t acc = 1 << 21;
  for (int t = 0; t < b[2 * xx + 1]; ++t) acc += in[r * in_rs + (size_t)(b[2 * xx] + t) * in_cs] * k[(size_t)t * pitch + xx];
  out[r * out_rs + xx * out_cs] = (uint8_t)clip8(acc);
}

// ---- the host's statement of one axis (aivc_amd/resize.py: axis_tables, device_tables) ------------------------------------------
static double sinc(double x) { return x == 0.0 ? 1.0 : sin(x * M_PI) / (x * M_PI); }
static double bicubic(double x) {
  const double a = -0.5;
  x = fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
static double lanczos(double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0; }

struct Axis {
  int n_in, n_out, taps, pitch, span, max_rows;
  std::vector<int32_t> bounds, coeffs;  // [n_out][2], [taps][pitch]
};
static Axis make_axis(int n_in, int n_out, bool lan, int tile) {
  Axis a{n_in, n_out, 0, (n_out + 3) & ~3, 0, 0, std::vector<int32_t>(2 * (size_t)n_out), {}};
  const double scale = (double)n_in / n_out, fs = std::max(scale, 1.0), support = (lan ? 3.0 : 2.0) * fs, ss = 1.0 / fs;
  std::vector<std::vector<int32_t>> rows(n_out);
  for (int xx = 0; xx < n_out; ++xx) {
    const double c = (xx + 0.5) * scale;
    const int xmin = std::max((int)(c - support + 0.5), 0), xmax = std::min((int)(c + support + 0.5), n_in) - xmin;
    std::vector<double> k(xmax);
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += k[x] = (lan ? lanczos : bicubic)((x + xmin - c + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
      const double w = ww != 0.0 ? k[x] / ww : k[x];
      rows[xx].push_back(w < 0 ? (int)(-0.5 + w * (1 << 22)) : (int)(0.5 + w * (1 << 22)));
    }
    a.bounds[2 * xx] = xmin, a.bounds[2 * xx + 1] = xmax;
    a.taps = std::max(a.taps, xmax);
  }
  a.taps = (a.taps + 3) & ~3;
  a.coeffs.assign((size_t)a.taps * a.pitch, 0);
  for (int xx = 0; xx < n_out; ++xx)
    for (size_t k = 0; k < rows[xx].size(); ++k) a.coeffs[k * a.pitch + xx] = rows[xx][k];
  for (int x0 = 0; x0 < n_out; x0 += tile) {
    const int xl = std::min(x0 + tile, n_out) - 1;
    a.span = std::max(a.span, a.bounds[2 * xl] + a.taps - a.bounds[2 * x0]);
    a.max_rows = std::max(a.max_rows, a.bounds[2 * xl] + a.bounds[2 * xl + 1] - a.bounds[2 * x0]);
  }
  return a;
}
static std::vector<uint8_t> host_pass(const std::vector<uint8_t> &in, int rows, const Axis &a) {  // along the rows of [rows][n_in]
  std::vector<uint8_t> out((size_t)rows * a.n_out);
  for (int r = 0; r < rows; ++r)
    for (int xx = 0; xx < a.n_out; ++xx) {
      int32_t acc = 1 << 21;
      for (int k = 0; k < a.bounds[2 * xx + 1]; ++k)
        acc += in[(size_t)r * a.n_in + a.bounds[2 * xx] + k] * a.coeffs[(size_t)k * a.pitch + xx];
      out[(size_t)r * a.n_out + xx] = (uint8_t)std::min(std::max(acc >> 22, 0), 255);
    }
  return out;
}
static std::vector<uint8_t> transpose(const std::vector<uint8_t> &in, int rows, int cols) {
  std::vector<uint8_t> out(in.size());
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) out[(size_t)c * rows + r] = in[(size_t)r * cols + c];
  return out;
}

template <class T>
static T *upload(const std::vector<T> &v) {
  T *d;
  CHECK(hipMalloc(&d, v.size() * sizeof(T)));
  CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

static void run(int n, int h_in, int w_in, int h_out, int w_out, bool lan) {
  const Axis ax = make_axis(w_in, w_out, lan, TILE_W), ay = make_axis(h_in, h_out, lan, TILE_H);
  const int lds_pitch = (ax.span + 34) & ~15, in_rows = ay.max_rows;
  const size_t lds_bytes = (size_t)in_rows * (lds_pitch + TILE_W);
  if (in_rows > MAX_IN_ROWS || lds_bytes > 65536) {
    printf("%dx%d -> %dx%d %s: %d input rows, %zu bytes of LDS: not run\n", w_in, h_in, w_out, h_out, lan ? "lanczos" : "bicubic", in_rows,
           lds_bytes);
    return;
  }
  const size_t len = (size_t)h_in * w_in, olen = (size_t)h_out * w_out;
  std::vector<uint8_t> host(len * n);
  uint32_t x = 12345u;
  for (size_t i = 0; i < len; ++i) host[i] = (uint8_t)((i % w_in + 2 * (i / w_in)) % 200 + ((x = x * 1664525u + 1013904223u) >> 26));
  for (int p = 1; p < n; ++p) {  // plane p: plane 0 rotated by 97 p bytes
    const size_t s = (size_t)97 * p;
    std::copy(host.begin() + s, host.begin() + len, host.begin() + p * len);
    std::copy(host.begin(), host.begin() + s, host.begin() + p * len + (len - s));
  }
  uint8_t *d_in = upload(host), *d_out;
  CHECK(hipMalloc(&d_out, olen * n));
  int32_t *xb = upload(ax.bounds), *xk = upload(ax.coeffs), *yb = upload(ay.bounds), *yk = upload(ay.coeffs);
  const int tiles_y = (h_out + TILE_H - 1) / TILE_H, tiles_x = (w_out + TILE_W - 1) / TILE_W;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::vector<float> ms;
  for (int r = 0; r < 8; ++r) {  // (the first window warms up and is dropped)
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL(fused_kernel, dim3(tiles_y * n, tiles_x), dim3(TX, TY), lds_bytes, 0, d_in, h_in, w_in, h_out, w_out, tiles_y, xb, xk,
                       ax.taps, ax.pitch, lds_pitch, yb, yk, ay.pitch, in_rows, d_out);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float t;
    CHECK(hipEventElapsedTime(&t, e0, e1));
    if (r) ms.push_back(t);
  }
  bool ok = true;
  std::vector<uint8_t> got(olen);
  for (int p : {0, n - 1}) {
    std::vector<uint8_t> plane(host.begin() + p * len, host.begin() + (p + 1) * len);
    const auto mid = host_pass(plane, h_in, ax);                                              // [h_in][w_out]
    const auto want = transpose(host_pass(transpose(mid, h_in, w_out), w_out, ay), w_out, h_out);  // [h_out][w_out]
    CHECK(hipMemcpy(got.data(), d_out + p * olen, olen, hipMemcpyDeviceToHost));
    ok = ok && got == want;
    if (got != want && getenv("PROBE_VERBOSE")) {
      uint8_t *t1, *t2;  // plane p through the plain kernel: rows, then columns
      CHECK(hipMalloc(&t1, (size_t)h_in * w_out));
      CHECK(hipMalloc(&t2, olen));
      hipLaunchKernelGGL(plain_pass_kernel, dim3((unsigned)(((size_t)h_in * w_out + 255) / 256)), dim3(256), 0, 0, d_in + p * len, (size_t)h_in,
                         w_in, w_out, xb, xk, ax.pitch, t1, (size_t)w_in, (size_t)1, (size_t)w_out, (size_t)1);
      hipLaunchKernelGGL(plain_pass_kernel, dim3((unsigned)((olen + 255) / 256)), dim3(256), 0, 0, t1, (size_t)w_out, h_in, h_out, yb, yk,
                         ay.pitch, t2, (size_t)1, (size_t)w_out, (size_t)1, (size_t)w_out);
      std::vector<uint8_t> plain(olen);
      CHECK(hipMemcpy(plain.data(), t2, olen, hipMemcpyDeviceToHost));
      printf("  plane %d: plain kernel == host %d, plain kernel == fused %d\n", p, (int)(plain == want), (int)(plain == got));
      CHECK(hipFree(t1));
      CHECK(hipFree(t2));
      size_t nd = 0, first = olen;
      for (size_t i = 0; i < olen; ++i)
        if (got[i] != want[i]) {
          if (first == olen) first = i;
          ++nd;
        }
      printf("  plane %d: %zu of %zu bytes differ, first at row %zu column %zu: %d against %d\n", p, nd, olen, first / w_out, first % w_out,
             got[first], want[first]);
    }
  }
  std::sort(ms.begin(), ms.end());
  const double med = ms[ms.size() / 2];
  printf("%dx%d -> %dx%d %s n=%d in_rows=%d lds=%zu ms=%.3f (min %.3f max %.3f) TBps=%.3f planes_%s\n", w_in, h_in, w_out, h_out,
         lan ? "lanczos" : "bicubic", n, in_rows, lds_bytes, med, ms.front(), ms.back(), (double)(len + olen) * n / (med * 1e-3) / 1e12,
         ok ? "ok" : "WRONG");
  for (void *q : {(void *)d_in, (void *)d_out, (void *)xb, (void *)xk, (void *)yb, (void *)yk}) CHECK(hipFree(q));
}

int main() {
  const int n = 129;
  for (bool lan : {false, true}) {
    run(n, 2160, 3840, 1080, 1920, lan);
    run(n, 1080, 1920, 2160, 3840, lan);
  }
  return 0;
}
