// ufr_common.h -- shared helpers of libufr_hip.so (gfx950 only).  No longer host-only: the device helpers that more than one kernel file uses (`ufr::dev`, at the end) live here, once.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/ufr_hip.h"

namespace ufr {

// Thread-local message returned by ufr_last_error().
char* err_buf();
int fail(int code, const char* fmt, ...);

inline hipStream_t as_stream(ufr_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// hipFuncAttributeMaxDynamicSharedMemorySize of `fn` raised to >= `bytes` on the CURRENT device: remembered per (kernel,
// device) under a mutex -- a process may drive several devices and several host threads (capi.hip).  hipSuccess when nothing
// had to be done.
hipError_t ensure_dynamic_lds(const void* fn, size_t bytes);

// Build manifest (capi.hip, `ufr_build_manifest()`): every translation unit registers, at load, the checksum of the sources it was
// COMPILED FROM (its .hip + every header of this directory + include/ufr_hip.h; the Makefile passes it as -DUFR_TU_SUM).  _lib.py recomputes the
// checksums from the tree and refuses a library that holds an object built from other sources.
void register_tu(const char* name, const char* sum);
struct TuRegistrar {
  TuRegistrar(const char* name, const char* sum) { register_tu(name, sum); }
};

// Post-launch check: launch-configuration errors surface here; nothing is synchronised.
inline int launched(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(UFR_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return UFR_OK;
}

constexpr int kWave = 64;           // CDNA4 wavefront
constexpr int kNumCU = 256;         // MI355X
constexpr int kMaxLds = 160 * 1024; // bytes of LDS per CU / per workgroup

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// Grid size for grid-stride elementwise kernels: enough workgroups to fill 256 CUs x 8.
inline int stream_grid(long n, int block) {
  long g = (n + block - 1) / block;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

// 16-byte alignment of every pointer given: the test in front of each float4 / bf16x8 kernel form
template <class... P>
inline bool aligned16(const P*... p) { return ((... | reinterpret_cast<uintptr_t>(p)) & 15) == 0; }

// ---- per-item metrics: the ONE scheme of ufr_sweep_metrics, ufr_eval_metrics, ufr_global_metrics and ufr_validation_metrics ---------
// A grid of (slots, K) workgroups of 256 threads, slots = metric_slots(work of one item, 256): workgroup (s, k) walks the elements
// s * 256 + t, + slots * 256, ... of item k with float64 sums per thread, `dev::store_partial` reduces them (block_sum) into the
// workgroup's partial in the workspace, and a finalize launch of K workgroups adds the `slots` partials of its item, thread t < slots
// partial t (`dev::item_totals`).  slots follows from the sizes alone, so every sum has a fixed order: no float atomics, two runs are
// bit-identical.  The workspace holds `stride` partials per item: kMetricSlots (sweep, eval, global) or slots itself (validation).
constexpr int kMetricSlots = 128;   // workgroups (= partials) per item at most
inline int metric_slots(long work, int block) {
  const int s = ceil_div(work, block);
  return s > kMetricSlots ? kMetricSlots : s;
}
// the two checks every metrics entry makes of its result rows and its workspace; `what` is the entry's name in its messages
inline int check_result_rows(const char* what, int row0, int K, int rows) {
  if (!(row0 >= 0 && rows > 0 && (long)row0 + K <= rows))
    return fail(UFR_EINVAL, "%s: rows %d .. %ld leave the result buffer of %d rows", what, row0, (long)row0 + K - 1, rows);
  return UFR_OK;
}
inline int check_workspace(const char* what, long ws_elems, long need) {
  if (!(ws_elems >= need)) return fail(UFR_EINVAL, "%s: workspace of %ld doubles, %ld needed", what, ws_elems, need);
  return UFR_OK;
}

// correlation_vec.hip: 0 = launched, 1 = shape not covered (use the general fast path), <0 = error
int corr_fwd_vec_launch(const float* in1, const float* in2, float* out, int B, int C, int H, int W, int P,
                        int DP, float scale, float slope, hipStream_t st);
int corr_bwd_vec_launch(const float* in1, const float* in2, const float* gout, float* gin1, float* gin2,
                        int B, int C, int H, int W, int P, int DP, hipStream_t st);

// correlation_mfma.hip: both adjoints on the fp32 matrix cores; same return convention
int corr_bwd_mfma_launch(const float* in1, const float* in2, const float* gout, float* gin1, float* gin2,
                         int B, int C, int H, int W, int P, int DP, hipStream_t st);

// attack.hip: *loss += sum of the n workgroup partials, in a fixed order (one wave)
void loss_finalize_launch(const float* partials, int n, float* loss, hipStream_t st);

// ---- device helpers shared by the kernel files (each file names what it uses: `using ufr::dev::split3;`) ---------------------------
namespace dev {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// The three-plane split, the numerical contract of every kernel on bf16 planes: v = a + b + c exactly, round to nearest even at
// every step (igemm.py's _split3 is the host's statement of it).
__device__ __forceinline__ void split3(float v, __bf16& a, __bf16& b, __bf16& c) {
  a = (__bf16)v;
  const float r1 = v - (float)a;
  b = (__bf16)r1;
  c = (__bf16)(r1 - (float)b);
}

// eight consecutive channels of one pixel of three planes <-> float32 (16-byte accesses)
__device__ __forceinline__ void load_planes8(const __bf16* p, long plane_stride, float v[8]) {
  const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
  const bf16x8 b = *reinterpret_cast<const bf16x8*>(p + plane_stride);
  const bf16x8 c = *reinterpret_cast<const bf16x8*>(p + 2 * plane_stride);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = ((float)a[j] + (float)b[j]) + (float)c[j];
}
__device__ __forceinline__ void store_planes8(__bf16* p, long plane_stride, const float v[8]) {
  bf16x8 q0, q1, q2;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 x, y, z;
    split3(v[j], x, y, z);
    q0[j] = x; q1[j] = y; q2[j] = z;
  }
  *reinterpret_cast<bf16x8*>(p) = q0;
  *reinterpret_cast<bf16x8*>(p + plane_stride) = q1;
  *reinterpret_cast<bf16x8*>(p + 2 * plane_stride) = q2;
}
__device__ __forceinline__ void load_f8(const float* p, float v[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// one LDS-DMA: 16 bytes per lane from `src` (per lane) to `lds_wave_base + 16 * lane` (the base must be wave-uniform)
__device__ __forceinline__ void glds16(const __bf16* src, __bf16* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(src, lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }
__device__ __forceinline__ float signf(float v) { return (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : 0.f); }  // torch.sign (NaN -> 0)
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ int floor_div(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
__device__ __forceinline__ int ceil_div_i(int a, int b) { return -floor_div(-a, b); }

// One axis of the window cone (window.hip's ufr_cone_window / ufr_attack_place and patch_sweep.hip's window table run the same
// statements; the tests compare their tables bit for bit): [lo, hi] (input pixels, inclusive) -> window origin / needed extent in
// pixels.  Cone of an interval through conv(k, s, p): outputs o with [s*o - p, s*o - p + k - 1] meeting it.
__device__ inline void cone_axis(int lo, int hi, int size, const ufr_cone_chain& ch, int win, int* origin, int* need) {
  int total = 1;
  for (int l = 0; l < ch.n_layers; ++l) total *= ch.stride[l];
  const int cells = size / total;          // window grid = cells of the deepest level
  if (hi < lo) { *origin = 0; *need = 0; return; }
  int need_lo = INT_MAX, need_hi = -1, n = size, jump = 1, t = 0;
  for (int l = 0; l < ch.n_layers; ++l) {
    const int k = ch.kernel[l], s = ch.stride[l], p = ch.pad[l];
    const int n_out = (n + 2 * p - k) / s + 1;
    lo = max(ceil_div_i(lo + p - (k - 1), s), 0);
    hi = min(floor_div(hi + p, s), n_out - 1);
    n = n_out; jump *= s;
    while (t < ch.n_taps && ch.tap_layer[t] == l) {
      const int per = total / jump;        // cells of this level per window-grid cell
      need_lo = min(need_lo, floor_div(lo - ch.tap_margin[t], per));
      need_hi = max(need_hi, floor_div(hi + ch.tap_margin[t], per));
      ++t;
    }
  }
  need_lo = max(need_lo, 0); need_hi = min(need_hi, cells - 1);
  const int cnt = need_hi - need_lo + 1, wcells = win / total;
  int o = need_lo - max(wcells - cnt, 0) / 2;
  o = min(max(o, 0), max(cells - wcells, 0));
  *origin = o * total; *need = cnt * total;
}

// the sum over a workgroup of BLOCK threads in a fixed order, returned to every thread (`lds`: BLOCK / 64 doubles)
template <int BLOCK>
__device__ inline double block_sum(double v, double* lds) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();                                            // the previous use of lds is over
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < BLOCK / 64; ++i) t += lds[i];
  return t;
}

// the per-item metrics scheme (above): the partial of workgroup (blockIdx.x, k) is WIDTH doubles, the first N of them sums.
// store_partial: this thread's N sums -> the workgroup's partial, which is returned (thread 0 may add to it)
template <int BLOCK, int N, int WIDTH = N>
__device__ inline double* store_partial(const double* sum, double* lds, double* __restrict__ part, int k, int stride) {
  double* __restrict__ mine = part + ((long)k * stride + blockIdx.x) * WIDTH;
  for (int q = 0; q < N; ++q) {
    const double t = block_sum<BLOCK>(sum[q], lds);
    if (threadIdx.x == 0) mine[q] = t;
  }
  return mine;
}
// item_totals: t[0..N) = the sums over the `slots` partials of item k, thread i < slots adding partial i (every thread gets them)
template <int BLOCK, int N, int WIDTH = N>
__device__ inline void item_totals(const double* __restrict__ part, int k, int stride, int slots, double* lds, double* t) {
  const bool mine = (int)threadIdx.x < slots;
  const double* __restrict__ p = part + ((long)k * stride + (mine ? threadIdx.x : 0)) * WIDTH;
  for (int q = 0; q < N; ++q) t[q] = block_sum<BLOCK>(mine ? p[q] : 0.0, lds);
}

// ---- shared by patch_sweep.hip, patch_eval.hip and global_eval.hip -------------------------------------------------------------------
// attack.hip's paste_placed_kernel, do_clamp = 1: (1-m)*img and m*patch are rounded separately, then added (no fma)
__device__ __forceinline__ float paste_clamped(float img, float m, float pv, float lo, float hi) {
  const float mp = m * pv, om = 1.0f - m;
  return clampf(om * img + mp, lo, hi);
}

// torch's upsample_bilinear2d, align_corners = False, size given (aten/src/ATen/native/UpSample.h area_pixel_compute_source_index):
//   src = max(scale * (dst + 0.5) - 0.5, 0), scale = in / out;  i0 = (int)src;  i1 = i0 + (i0 < in - 1);  l1 = src - i0
// in float64: with in == out the source is dst itself and l1 = 0
__device__ __forceinline__ void bilinear_source(int dst, double scale, int in, int& i0, int& i1, double& l1) {
  const double src = fmax(scale * ((double)dst + 0.5) - 0.5, 0.0);
  i0 = min((int)src, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (double)i0;
}

__device__ __forceinline__ double bilinear(double v00, double v01, double v10, double v11, double ly, double lx) {
  const double hy = 1.0 - ly, hx = 1.0 - lx;
  return hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
}

// Ground-truth pixel p = yg * Wg + xg of an Hg x Wg grid -> the four taps of an H x W prediction resized to it (sy = H / Hg,
// sx = W / Wg): rows y0 / y1 at offsets r0 / r1, columns x0 / x1, weights ly / lx of the second row / column
struct FlowTaps {
  int yg, xg, y0, y1, x0, x1;
  double ly, lx;
  long r0, r1;
};
__device__ __forceinline__ FlowTaps flow_taps(long p, int Wg, double sy, double sx, int H, int W) {
  FlowTaps s;
  s.yg = (int)(p / Wg);
  s.xg = (int)(p - (long)s.yg * Wg);
  bilinear_source(s.yg, sy, H, s.y0, s.y1, s.ly);
  bilinear_source(s.xg, sx, W, s.x0, s.x1, s.lx);
  s.r0 = (long)s.y0 * W;
  s.r1 = (long)s.y1 * W;
  return s;
}
// one plane of the prediction at those taps
__device__ __forceinline__ double sample(const float* __restrict__ f, const FlowTaps& s) {
  return bilinear((double)f[s.r0 + s.x0], (double)f[s.r0 + s.x1], (double)f[s.r1 + s.x0], (double)f[s.r1 + s.x1], s.ly, s.lx);
}

// One pixel: the length of (du, dv), the error vector as the caller's reference forms it (losses.py:29-30: ground truth - rescaled
// prediction; perturb_model.py:46-47: rescaled prediction - ground truth), and torch's cosine_similarity of (gu, gv) and (fu, fv):
// each vector divided by max(its norm, eps) first, then the dot product
__device__ __forceinline__ void epe_cos(double du, double dv, double gu, double gv, double fu, double fv, double& epe, double& cs) {
  epe = sqrt(du * du + dv * dv);
  const double ng = fmax(sqrt(gu * gu + gv * gv), 1e-8), nf = fmax(sqrt(fu * fu + fv * fv), 1e-8);
  cs = (gu / ng) * (fu / nf) + (gv / ng) * (fv / nf);
}

// A canvas that is 0 outside an h x w rectangle at (oy, ox) of the frame and `s` (rows of sw floats) inside it, at frame rows
// y0 / y1 and columns x0 / x1 (already inside the frame): which taps fall into the rectangle, and the canvas resized at them
struct Corners {
  int i0, i1, j0, j1;
  bool a0, a1, b0, b1, any;
};
__device__ __forceinline__ Corners corners(int y0, int y1, int x0, int x1, int oy, int ox, int h, int w) {
  Corners q;
  q.i0 = y0 - oy; q.i1 = y1 - oy; q.j0 = x0 - ox; q.j1 = x1 - ox;
  q.a0 = (unsigned)q.i0 < (unsigned)h; q.a1 = (unsigned)q.i1 < (unsigned)h;
  q.b0 = (unsigned)q.j0 < (unsigned)w; q.b1 = (unsigned)q.j1 < (unsigned)w;
  q.any = (q.a0 || q.a1) && (q.b0 || q.b1);
  return q;
}
__device__ __forceinline__ double resized_canvas(const float* __restrict__ s, int sw, const Corners& q, double ly, double lx) {
  const double v00 = q.a0 && q.b0 ? (double)s[q.i0 * sw + q.j0] : 0.0, v01 = q.a0 && q.b1 ? (double)s[q.i0 * sw + q.j1] : 0.0;
  const double v10 = q.a1 && q.b0 ? (double)s[q.i1 * sw + q.j0] : 0.0, v11 = q.a1 && q.b1 ? (double)s[q.i1 * sw + q.j1] : 0.0;
  return bilinear(v00, v01, v10, v11, ly, lx);
}

}  // namespace dev
}  // namespace ufr

#if defined(UFR_TU_NAME) && defined(UFR_TU_SUM)
namespace {
const ufr::TuRegistrar ufr_tu_registrar(UFR_TU_NAME, UFR_TU_SUM);
}
#endif

#define UFR_REQUIRE(cond, ...) \
  do {                         \
    if (!(cond)) return ufr::fail(UFR_EINVAL, __VA_ARGS__); \
  } while (0)
