// ufr_common.h -- shared helpers of libufr_hip.so (gfx950 only).  No longer host-only: the device helpers that more than one kernel file uses (`ufr::dev`, at the end) live here, once.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdarg>
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
// COMPILED FROM (its .hip + this header + include/ufr_hip.h; the Makefile passes it as -DUFR_TU_SUM).  _lib.py recomputes the
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

// ---- shared by patch_sweep.hip and patch_eval.hip ---------------------------------------------------------------------------------
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
