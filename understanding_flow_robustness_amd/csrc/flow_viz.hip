// flow_viz.hip -- the figures of the patch analyses (gfx950): the Middlebury colour coding of flowutils/flowlib.py:269-306 and
// :469-566, and the six-panel strip `viz###.jpg` of patch_attacks/test_patch.py:467-621 and test_moving_patch.py:529-654.
//   ufr_flow_to_image   flow [K,2,H,W] -> uint8 [K,H,W,3]: launch A finds each item's largest radius in float32 (the dtype the
//                       reference's `u**2 + v**2`, sqrt and max run in), launch B codes the colours in float64, statement for
//                       statement in the reference's order;
//   ufr_eval_blend_gt, ufr_sweep_blend_gt   the ground truth that ufr_eval_metrics / ufr_sweep_metrics scored, written out
//                       (patch_eval_dev.h);
//   ufr_viz_ranges      per item the record of eight floats the strip needs: the ranges of both normalised frames, the largest
//                       radius of the resized ground truth and the three flows' own maxima;
//   ufr_viz_strip       the strip, uint8 [K,H,6W,3], one launch; 12 bytes per four pixels when W % 4 == 0.
// The reference does, per item: seven D2H copies, four float64 numpy passes of flow_to_image over the frame, a cv2.resize, a cv2.erode
// and a concatenation of six float64 images.  Maxima are order-independent, nothing here adds floats: two runs give the same bytes.
#include <cfloat>

#include "patch_eval_dev.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSlots = ufr::kMetricSlots;
constexpr int kWheel = 55;                 // rows of make_color_wheel (flowlib.py:513-566)
constexpr int kMaxima = 8;                 // lo_tgt, hi_tgt, lo_ref, hi_ref, maxrad_gt, max |flow|, max |adv_flow|, max |adv_flow - flow|
constexpr int kRecord = UFR_VIZ_RECORD;    // those eight, then the ground-truth panel's own maximum once more: slot 4 is the `maxr` of
                                           // panels 3-6 and a caller may replace it, slot 8 stays what panel 6's flow_to_image finds itself
constexpr float kUnknown = 1e7f;           // UNKNOWN_FLOW_THRESH
constexpr double kPi = 3.141592653589793;  // np.pi

using ufr::aligned16;
using ufr::dev::eval_ground_truth;
using ufr::dev::eval_item;
using ufr::dev::EvalItem;
using ufr::dev::FlowTaps;
using ufr::dev::flow_taps;
using ufr::dev::sweep_ground_truth;

struct Wheel {
  double c[kWheel * 3];                    // wheel / 255, row-major: by value in the kernel arguments
};

// the maximum over a workgroup of kBlock threads, returned to every thread (`lds`: kBlock / 64 floats); exact in any order
__device__ inline float block_max(float v, float* lds) {
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  __syncthreads();                                            // the previous use of lds is over
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = lds[0];
  for (int i = 1; i < kBlock / 64; ++i) t = fmaxf(t, lds[i]);
  return t;
}

// flowlib.py:283-293: an unknown pixel counts as (0, 0); float32 products, sum and a correctly rounded square root
__device__ __forceinline__ bool unknown(float u, float v) { return fabsf(u) > kUnknown || fabsf(v) > kUnknown; }
__device__ __forceinline__ float radius(float u, float v) { return unknown(u, v) ? 0.f : sqrtf(u * u + v * v); }
// Python's max(maxr, own): the first unless the second is larger
__device__ __forceinline__ double denominator(float maxr, float own) { return (double)(own > maxr ? own : maxr) + DBL_EPSILON; }

// flowlib.py:298-306 and compute_color (:469-510) for one pixel, float64 in the reference's order.  A NaN is outside the contract
// (the reference's cast of NaN to uint8 is undefined): the wheel index is clamped and the byte is 0.
__device__ __forceinline__ void flow_color(float uf, float vf, double den, const double* __restrict__ wheel, unsigned char rgb[3]) {
  if (unknown(uf, vf)) {
    rgb[0] = rgb[1] = rgb[2] = 0;
    return;
  }
  const double u = (double)uf / den, v = (double)vf / den;
  const double rad = sqrt(u * u + v * v);
  const double a = atan2(-v, -u) / kPi;
  const double fk = (a + 1.0) / 2.0 * (double)(kWheel - 1) + 1.0;
  const double k0f = floor(fk);
  int k0 = (int)k0f;
  k0 = k0 < 1 ? 1 : (k0 > kWheel ? kWheel : k0);
  const int k1 = k0 + 1 == kWheel + 1 ? 1 : k0 + 1;
  const double f = fk - k0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double col = (1.0 - f) * wheel[(k0 - 1) * 3 + c] + f * wheel[(k1 - 1) * 3 + c];
    col = rad <= 1.0 ? 1.0 - rad * (1.0 - col) : col * 0.75;
    const double b = floor(255.0 * col);
    rgb[c] = b >= 0.0 && b <= 255.0 ? (unsigned char)(int)b : (unsigned char)0;
  }
}

__device__ __forceinline__ void load_wheel(const Wheel& wheel, double* lds) {
  for (int t = threadIdx.x; t < kWheel * 3; t += kBlock) lds[t] = wheel.c[t];
}

// four pixels' bytes as three words: the 12-byte store of the V = 4 forms (`dst` is 4-byte aligned)
struct Bytes12 {
  unsigned a, b, c;
};
__device__ __forceinline__ void store12(unsigned char* dst, const unsigned char b[12]) {
  Bytes12 w;
  w.a = (unsigned)b[0] | ((unsigned)b[1] << 8) | ((unsigned)b[2] << 16) | ((unsigned)b[3] << 24);
  w.b = (unsigned)b[4] | ((unsigned)b[5] << 8) | ((unsigned)b[6] << 16) | ((unsigned)b[7] << 24);
  w.c = (unsigned)b[8] | ((unsigned)b[9] << 8) | ((unsigned)b[10] << 16) | ((unsigned)b[11] << 24);
  *reinterpret_cast<Bytes12*>(dst) = w;
}
template <int V>
__device__ __forceinline__ void store_pixels(unsigned char* dst, const unsigned char* b) {
  if constexpr (V == 4) {
    store12(dst, b);
  } else {
    dst[0] = b[0]; dst[1] = b[1]; dst[2] = b[2];
  }
}
template <int V>
__device__ __forceinline__ void load_floats(const float* __restrict__ src, float* v) {
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(src);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = src[0];
  }
}

// ---- ufr_flow_to_image ---------------------------------------------------------------------------------------------------------------
// launch A, grid (slots, K): workgroup (s, k) takes the maximum radius over the pixels s * 256 + t, + slots * 256, ... of item k
__global__ __launch_bounds__(kBlock) void flow_max_kernel(const float* __restrict__ flow, long HW, float* __restrict__ part) {
  __shared__ float lds[kBlock / 64];
  const int k = blockIdx.y;
  const float* __restrict__ u = flow + (long)k * 2 * HW;
  const float* __restrict__ v = u + HW;
  float m = 0.f;
  for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < HW; p += (long)gridDim.x * kBlock) m = fmaxf(m, radius(u[p], v[p]));
  m = block_max(m, lds);
  if (threadIdx.x == 0) part[(long)k * kSlots + blockIdx.x] = m;
}

// launch B, grid (x, K): every workgroup takes its item's maximum from the `slots` partials, then walks groups of V pixels
template <int V>
__global__ __launch_bounds__(kBlock) void flow_color_kernel(const float* __restrict__ flow, const float* __restrict__ maxr,
                                                            const float* __restrict__ part, int slots, const Wheel wheel, long HW,
                                                            unsigned char* __restrict__ out) {
  __shared__ double wl[kWheel * 3];
  __shared__ float lds[kBlock / 64];
  const int k = blockIdx.y;
  load_wheel(wheel, wl);
  const float own = block_max((int)threadIdx.x < slots ? part[(long)k * kSlots + threadIdx.x] : 0.f, lds);   // syncs: wl is visible
  const double den = denominator(maxr != nullptr ? maxr[k] : -1.f, own);
  const float* __restrict__ u = flow + (long)k * 2 * HW;
  const float* __restrict__ v = u + HW;
  unsigned char* __restrict__ o = out + (long)k * HW * 3;
  for (long q = (long)blockIdx.x * kBlock + threadIdx.x; q < HW / V; q += (long)gridDim.x * kBlock) {
    float uu[V], vv[V];
    load_floats<V>(u + q * V, uu);
    load_floats<V>(v + q * V, vv);
    unsigned char b[3 * V];
#pragma unroll
    for (int j = 0; j < V; ++j) flow_color(uu[j], vv[j], den, wl, b + 3 * j);
    store_pixels<V>(o + q * V * 3, b);
  }
}

// ---- ufr_eval_blend_gt ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void eval_blend_gt_kernel(const float* __restrict__ gt, const float* __restrict__ m_tgt,
                                                               const float* __restrict__ m_ref, const float* __restrict__ flow,
                                                               const int* __restrict__ places, int H, int W, int Hg, int Wg, int sh,
                                                               int sw, int patch_flow, double zy, double zx, float* __restrict__ out) {
  const int k = blockIdx.y;
  const long HWg = (long)Hg * Wg;
  const int plane = sh * sw;
  const EvalItem it = eval_item(gt, m_tgt, m_ref, flow, places, k, HWg, plane);
  const double sy = (double)H / (double)Hg, sx = (double)W / (double)Wg;
  float* __restrict__ o = out + (long)k * 3 * HWg;
  for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < HWg; p += (long)gridDim.x * kBlock) {
    const FlowTaps s = flow_taps(p, Wg, sy, sx, H, W);
    double g[3], ga[3];
    eval_ground_truth(it, p, HWg, s, H, W, plane, sw, patch_flow, zy, zx, g, ga);
    o[p] = (float)ga[0];
    o[HWg + p] = (float)ga[1];
    o[2 * HWg + p] = (float)ga[2];
  }
}

// grid (x, K): position k of a chunk of the sweep
__global__ __launch_bounds__(kBlock) void sweep_blend_gt_kernel(const float* __restrict__ gt, const float* __restrict__ mask_p,
                                                                const int* __restrict__ origins, int H, int W, int Hg, int Wg, int ph,
                                                                int pw, double patch_valid, float* __restrict__ out) {
  const int k = blockIdx.y;
  const long HWg = (long)Hg * Wg;
  const double sy = (double)H / (double)Hg, sx = (double)W / (double)Wg;
  const int oy = origins[2 * k], ox = origins[2 * k + 1];
  float* __restrict__ o = out + (long)k * 3 * HWg;
  for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < HWg; p += (long)gridDim.x * kBlock) {
    const FlowTaps s = flow_taps(p, Wg, sy, sx, H, W);
    double g[3];
    sweep_ground_truth(gt, p, HWg, mask_p, oy, ox, ph, pw, patch_valid, s, g);
    o[p] = (float)g[0];
    o[HWg + p] = (float)g[1];
    o[2 * HWg + p] = (float)g[2];
  }
}

// ---- the strip -------------------------------------------------------------------------------------------------------------------------
// cv2.INTER_NEAREST: source index = min(floor(dst * (src / dst)), src - 1), the ratio in float64
__device__ __forceinline__ int nearest(int dst, double ratio, int src) {
  const int i = (int)floor((double)dst * ratio);
  return i < src - 1 ? i : src - 1;
}
// pixel (y, x) of the ground-truth panel before colour coding (test_patch.py:507-522): resized, u * (W / Wg), v * (H / Hg) in float32,
// an unknown pixel zeroed -- the script zeroes it in the array it hands to flow_to_image, so this panel shows it white, not black
struct GtPanel {
  const float* __restrict__ gu;
  const float* __restrict__ gv;
  int Hg, Wg;
  double ry, rx;
  float fu, fv;
};
__device__ __forceinline__ GtPanel gt_panel(const float* __restrict__ g, int k, int H, int W, int Hg, int Wg) {
  GtPanel t;
  t.gu = g + (long)k * 3 * Hg * Wg;
  t.gv = t.gu + (long)Hg * Wg;
  t.Hg = Hg; t.Wg = Wg;
  t.ry = (double)Hg / (double)H; t.rx = (double)Wg / (double)W;
  t.fu = (float)((double)W / (double)Wg); t.fv = (float)((double)H / (double)Hg);
  return t;
}
__device__ __forceinline__ void gt_pixel(const GtPanel& t, int y, int x, float& u, float& v) {
  const long src = (long)nearest(y, t.ry, t.Hg) * t.Wg + nearest(x, t.rx, t.Wg);
  u = t.gu[src] * t.fu;
  v = t.gv[src] * t.fv;
  if (unknown(u, v)) u = v = 0.f;
}
// custom_transforms.Normalize(0.5, 0.5) in float32
__device__ __forceinline__ float normalized(float x) { return (x - 0.5f) / 0.5f; }

// grid (slots, K): the eight maxima of item k over the frame pixels s * 256 + t, + slots * 256, ... (a minimum as -max(-x))
__global__ __launch_bounds__(kBlock) void viz_ranges_kernel(const float* __restrict__ adv_tgt, const float* __restrict__ adv_ref,
                                                            const float* __restrict__ flow, const float* __restrict__ adv_flow,
                                                            const float* __restrict__ g, int H, int W, int Hg, int Wg,
                                                            float* __restrict__ part) {
  __shared__ float lds[kBlock / 64];
  const int k = blockIdx.y;
  const long HW = (long)H * W;
  const float* __restrict__ ft = adv_tgt + (long)k * 3 * HW;
  const float* __restrict__ fr = adv_ref + (long)k * 3 * HW;
  const float* __restrict__ cu = flow + (long)k * 2 * HW;
  const float* __restrict__ au = adv_flow + (long)k * 2 * HW;
  const GtPanel t = gt_panel(g, k, H, W, Hg, Wg);
  float m[kMaxima] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.f, 0.f, 0.f, 0.f};
  for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < HW; p += (long)gridDim.x * kBlock) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = normalized(ft[c * HW + p]), b = normalized(fr[c * HW + p]);
      m[0] = fmaxf(m[0], -a); m[1] = fmaxf(m[1], a);
      m[2] = fmaxf(m[2], -b); m[3] = fmaxf(m[3], b);
    }
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    float u, v;
    gt_pixel(t, y, x, u, v);
    m[4] = fmaxf(m[4], radius(u, v));
    const float c0 = cu[p], c1 = cu[HW + p], a0 = au[p], a1 = au[HW + p];
    m[5] = fmaxf(m[5], radius(c0, c1));
    m[6] = fmaxf(m[6], radius(a0, a1));
    m[7] = fmaxf(m[7], radius(a0 - c0, a1 - c1));
  }
  float* __restrict__ mine = part + ((long)k * kSlots + blockIdx.x) * kMaxima;
  for (int q = 0; q < kMaxima; ++q) {
    const float r = block_max(m[q], lds);
    if (threadIdx.x == 0) mine[q] = r;
  }
}

// grid K: one workgroup takes the maxima over the `slots` partials of its item and writes the record
__global__ __launch_bounds__(kBlock) void viz_ranges_finalize_kernel(const float* __restrict__ part, int slots,
                                                                     float* __restrict__ record) {
  __shared__ float lds[kBlock / 64];
  const int k = blockIdx.x;
  const bool mine = (int)threadIdx.x < slots;
  const float* __restrict__ p = part + ((long)k * kSlots + (mine ? threadIdx.x : 0)) * kMaxima;
  for (int q = 0; q < kMaxima; ++q) {
    const float r = block_max(mine ? p[q] : -INFINITY, lds);
    if (threadIdx.x == 0) {
      record[k * kRecord + q] = q == 0 || q == 2 ? -r : r;
      if (q == 4) record[k * kRecord + kMaxima] = r;
    }
  }
}

// grid (x, K): a group is V pixels of one row of one panel; idx = (y * 6 + panel) * (W / V) + xq
template <int V>
__global__ __launch_bounds__(kBlock) void viz_strip_kernel(const float* __restrict__ adv_tgt, const float* __restrict__ adv_ref,
                                                           const float* __restrict__ flow, const float* __restrict__ adv_flow,
                                                           const float* __restrict__ g, const float* __restrict__ record,
                                                           const Wheel wheel, int H, int W, int Hg, int Wg,
                                                           unsigned char* __restrict__ out) {
  __shared__ double wl[kWheel * 3];
  load_wheel(wheel, wl);
  __syncthreads();
  const int k = blockIdx.y;
  const long HW = (long)H * W;
  const int Wv = W / V;
  const float* __restrict__ rec = record + (long)k * kRecord;
  const float maxrad_gt = rec[4];
  const GtPanel t = gt_panel(g, k, H, W, Hg, Wg);
  unsigned char* __restrict__ o = out + (long)k * HW * 18;
  const long groups = (long)H * 6 * Wv;
  for (long idx = (long)blockIdx.x * kBlock + threadIdx.x; idx < groups; idx += (long)gridDim.x * kBlock) {
    const int y = (int)(idx / (6 * Wv));
    const int rem = (int)(idx - (long)y * 6 * Wv);
    const int panel = rem / Wv, x0 = (rem - panel * Wv) * V;
    const long p = (long)y * W + x0;
    unsigned char b[3 * V];
    if (panel < 2) {
      // test_patch.py:481-489, :556-560, :617-619: Normalize, tensor2array's rule on the image's own range, (uint8)(255 * (double)a)
      const float* __restrict__ src = (panel == 0 ? adv_tgt : adv_ref) + (long)k * 3 * HW + p;
      const bool as_is = rec[2 * panel] >= 0.f && rec[2 * panel + 1] <= 1.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float x[V];
        load_floats<V>(src + c * HW, x);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float n = normalized(x[j]);
          const float a = as_is ? n : 0.5f + n * 0.5f;
          const double w = 255.0 * (double)a;                       // a frame outside [0, 1] is outside the contract: saturated
          b[3 * j + c] = w >= 0.0 ? (w < 256.0 ? (unsigned char)(int)w : (unsigned char)255) : (unsigned char)0;
        }
      }
    } else if (panel < 5) {
      // :532-552: flow_to_image(., maxrad_gt) of the flow, the attacked flow and their float32 difference
      float u[V], v[V];
      const float* __restrict__ cu = flow + (long)k * 2 * HW + p;
      const float* __restrict__ au = adv_flow + (long)k * 2 * HW + p;
      if (panel == 2) {
        load_floats<V>(cu, u);
        load_floats<V>(cu + HW, v);
      } else {
        load_floats<V>(au, u);
        load_floats<V>(au + HW, v);
        if (panel == 4) {
          float cu_[V], cv_[V];
          load_floats<V>(cu, cu_);
          load_floats<V>(cu + HW, cv_);
#pragma unroll
          for (int j = 0; j < V; ++j) { u[j] = u[j] - cu_[j]; v[j] = v[j] - cv_[j]; }
        }
      }
      const double den = denominator(maxrad_gt, rec[3 + panel]);
#pragma unroll
      for (int j = 0; j < V; ++j) flow_color(u[j], v[j], den, wl, b + 3 * j);
    } else {
      // :507-529: the scored ground truth, resized, colour coded with its own maximum, then cv2.erode's 3 x 3 minimum with positions
      // outside the image ignored: the column minima of the V + 2 columns around the group first, then three of them per pixel
      const double den = denominator(maxrad_gt, rec[kMaxima]);
      unsigned char col[V + 2][3];
#pragma unroll
      for (int j = 0; j < V + 2; ++j) {
        col[j][0] = col[j][1] = col[j][2] = 255;
        const int x = x0 - 1 + j;
        if (x < 0 || x >= W) continue;
        for (int dy = -1; dy <= 1; ++dy) {
          const int yy = y + dy;
          if (yy < 0 || yy >= H) continue;
          float u, v;
          unsigned char rgb[3];
          gt_pixel(t, yy, x, u, v);
          flow_color(u, v, den, wl, rgb);
#pragma unroll
          for (int c = 0; c < 3; ++c) col[j][c] = rgb[c] < col[j][c] ? rgb[c] : col[j][c];
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const unsigned char m01 = col[j][c] < col[j + 1][c] ? col[j][c] : col[j + 1][c];
          b[3 * j + c] = m01 < col[j + 2][c] ? m01 : col[j + 2][c];
        }
    }
    store_pixels<V>(o + ((long)y * 6 * W + (long)panel * W + x0) * 3, b);
  }
}

int wheel_from_host(const char* what, const double* wheel, Wheel* w) {
  for (int i = 0; i < kWheel * 3; ++i) {
    UFR_REQUIRE(wheel[i] >= 0.0 && wheel[i] <= 255.0, "%s: colour wheel entry %d = %g (0 .. 255)", what, i, wheel[i]);
    w->c[i] = wheel[i] / 255.0;                                       // compute_color: tmp[k] / 255
  }
  return UFR_OK;
}

}  // namespace

extern "C" long ufr_flow_to_image_workspace_floats(int K) { return K < 1 ? -1 : (long)K * kSlots; }

extern "C" int ufr_flow_to_image(const float* flow, const float* maxr, const double* wheel, unsigned char* out, int K, int H, int W,
                                 float* ws, long ws_elems, ufr_stream_t stream) {
  UFR_REQUIRE(flow && wheel && out && ws, "flow to image: null pointer argument");
  UFR_REQUIRE(K > 0 && K <= 65535 && H > 0 && W > 0, "flow to image: bad shape K=%d H=%d W=%d", K, H, W);
  UFR_REQUIRE((long)H * W < (1L << 30), "flow to image: too many pixels");
  if (int rc = ufr::check_workspace("flow to image", ws_elems, ufr_flow_to_image_workspace_floats(K))) return rc;
  Wheel w;
  if (int rc = wheel_from_host("flow to image", wheel, &w)) return rc;
  hipStream_t st = ufr::as_stream(stream);
  const long HW = (long)H * W;
  const int slots = ufr::metric_slots(HW, kBlock);
  flow_max_kernel<<<dim3(slots, K), kBlock, 0, st>>>(flow, HW, ws);
  if (int rc = ufr::launched("flow_max_kernel")) return rc;
  if (W % 4 == 0 && aligned16(flow) && (reinterpret_cast<uintptr_t>(out) & 3) == 0)
    flow_color_kernel<4><<<dim3(ufr::stream_grid(HW / 4, kBlock), K), kBlock, 0, st>>>(flow, maxr, ws, slots, w, HW, out);
  else
    flow_color_kernel<1><<<dim3(ufr::stream_grid(HW, kBlock), K), kBlock, 0, st>>>(flow, maxr, ws, slots, w, HW, out);
  return ufr::launched("flow_color_kernel");
}

extern "C" int ufr_eval_blend_gt(const float* gt, const float* m_tgt, const float* m_ref, const float* flow, const int* places,
                                 const int* places_host, float* g, int K, int H, int W, int Hg, int Wg, int sh, int sw,
                                 int ignore_mask_flow, ufr_stream_t stream) {
  UFR_REQUIRE(gt && m_tgt && places && g, "eval blend gt: null pointer argument");
  UFR_REQUIRE(places_host, "eval blend gt: the placements are needed on the host too (every record is checked before the launch)");
  UFR_REQUIRE(K > 0 && K <= 65535 && H > 0 && W > 0 && Hg > 0 && Wg > 0 && sh > 0 && sw > 0,
              "eval blend gt: bad shape K=%d H=%d W=%d Hg=%d Wg=%d sh=%d sw=%d", K, H, W, Hg, Wg, sh, sw);
  UFR_REQUIRE(sh <= H && sw <= W, "eval blend gt: the %dx%d slot is larger than the %dx%d frame", sh, sw, H, W);
  UFR_REQUIRE((long)H * W < (1L << 30) && (long)Hg * Wg < (1L << 30) && (long)K * 3 * sh * sw < (1L << 30),
              "eval blend gt: too many pixels");
  UFR_REQUIRE(ignore_mask_flow == 0 || ignore_mask_flow == 1, "eval blend gt: ignore_mask_flow = %d (0 or 1)", ignore_mask_flow);
  if (int rc = ufr::check_eval_places("eval blend gt", places_host, K, m_ref != nullptr ? 2 : 1, H, W, sh, sw)) return rc;
  const int patch_flow = flow != nullptr ? 2 : (ignore_mask_flow ? 0 : 1);
  const double zy = Hg > 1 ? (double)(H - 1) / (double)(Hg - 1) : 1.0, zx = Wg > 1 ? (double)(W - 1) / (double)(Wg - 1) : 1.0;
  eval_blend_gt_kernel<<<dim3(ufr::stream_grid((long)Hg * Wg, kBlock), K), kBlock, 0, ufr::as_stream(stream)>>>(
      gt, m_tgt, m_ref, flow, places, H, W, Hg, Wg, sh, sw, patch_flow, zy, zx, g);
  return ufr::launched("eval_blend_gt_kernel");
}

extern "C" int ufr_sweep_blend_gt(const float* gt, const float* mask_p, const int* origins, const int* origins_host, float* g, int K,
                                  int H, int W, int Hg, int Wg, int ph, int pw, int valid_in_patch, ufr_stream_t stream) {
  UFR_REQUIRE(gt && mask_p && g, "sweep blend gt: null pointer argument");
  UFR_REQUIRE(origins && origins_host, "sweep blend gt: null pointer argument (a patch needs its origins, on the device and the host)");
  UFR_REQUIRE(K > 0 && K <= 65535 && H > 0 && W > 0 && Hg > 0 && Wg > 0, "sweep blend gt: bad shape K=%d H=%d W=%d Hg=%d Wg=%d", K, H,
              W, Hg, Wg);
  UFR_REQUIRE((long)H * W < (1L << 30) && (long)Hg * Wg < (1L << 30), "sweep blend gt: too many pixels");
  UFR_REQUIRE(valid_in_patch == 0 || valid_in_patch == 1, "sweep blend gt: valid_in_patch = %d (0 or 1)", valid_in_patch);
  UFR_REQUIRE(ph > 0 && pw > 0, "sweep blend gt: bad shape ph=%d pw=%d", ph, pw);
  UFR_REQUIRE(ph <= H && pw <= W && (long)3 * ph * pw < (1L << 30), "sweep blend gt: the %dx%d patch is larger than the %dx%d frame", ph,
              pw, H, W);
  if (int rc = ufr::check_sweep_origins("sweep blend gt", origins_host, K, H, W, ph, pw)) return rc;
  sweep_blend_gt_kernel<<<dim3(ufr::stream_grid((long)Hg * Wg, kBlock), K), kBlock, 0, ufr::as_stream(stream)>>>(
      gt, mask_p, origins, H, W, Hg, Wg, ph, pw, (double)valid_in_patch, g);
  return ufr::launched("sweep_blend_gt_kernel");
}

extern "C" long ufr_viz_workspace_floats(int K) { return K < 1 ? -1 : (long)K * kSlots * kMaxima; }

namespace {
int check_strip(const char* what, const float* adv_tgt, const float* adv_ref, const float* flow, const float* adv_flow, const float* g,
                int K, int H, int W, int Hg, int Wg) {
  UFR_REQUIRE(adv_tgt && adv_ref && flow && adv_flow && g, "%s: null pointer argument", what);
  UFR_REQUIRE(K > 0 && K <= 65535 && H > 0 && W > 0, "%s: bad shape K=%d H=%d W=%d", what, K, H, W);
  UFR_REQUIRE(Hg > 0 && Wg > 0, "%s: a ground truth without its sizes (Hg=%d Wg=%d)", what, Hg, Wg);
  UFR_REQUIRE((long)H * W < (1L << 26) && (long)Hg * Wg < (1L << 30), "%s: too many pixels", what);
  return UFR_OK;
}
}  // namespace

extern "C" int ufr_viz_ranges(const float* adv_tgt, const float* adv_ref, const float* flow, const float* adv_flow, const float* g, int K,
                              int H, int W, int Hg, int Wg, float* ws, long ws_elems, float* record, ufr_stream_t stream) {
  if (int rc = check_strip("viz ranges", adv_tgt, adv_ref, flow, adv_flow, g, K, H, W, Hg, Wg)) return rc;
  UFR_REQUIRE(ws && record, "viz ranges: null pointer argument");
  if (int rc = ufr::check_workspace("viz ranges", ws_elems, ufr_viz_workspace_floats(K))) return rc;
  hipStream_t st = ufr::as_stream(stream);
  const int slots = ufr::metric_slots((long)H * W, kBlock);
  viz_ranges_kernel<<<dim3(slots, K), kBlock, 0, st>>>(adv_tgt, adv_ref, flow, adv_flow, g, H, W, Hg, Wg, ws);
  if (int rc = ufr::launched("viz_ranges_kernel")) return rc;
  viz_ranges_finalize_kernel<<<K, kBlock, 0, st>>>(ws, slots, record);
  return ufr::launched("viz_ranges_finalize_kernel");
}

extern "C" int ufr_viz_strip(const float* adv_tgt, const float* adv_ref, const float* flow, const float* adv_flow, const float* g,
                             const float* record, const double* wheel, unsigned char* out, int K, int H, int W, int Hg, int Wg,
                             ufr_stream_t stream) {
  if (int rc = check_strip("viz strip", adv_tgt, adv_ref, flow, adv_flow, g, K, H, W, Hg, Wg)) return rc;
  UFR_REQUIRE(record && wheel && out, "viz strip: null pointer argument");
  Wheel w;
  if (int rc = wheel_from_host("viz strip", wheel, &w)) return rc;
  hipStream_t st = ufr::as_stream(stream);
  const long HW = (long)H * W;
  if (W % 4 == 0 && aligned16(adv_tgt, adv_ref, flow, adv_flow) && (reinterpret_cast<uintptr_t>(out) & 3) == 0)
    viz_strip_kernel<4><<<dim3(ufr::stream_grid(6 * HW / 4, kBlock), K), kBlock, 0, st>>>(adv_tgt, adv_ref, flow, adv_flow, g, record, w,
                                                                                        H, W, Hg, Wg, out);
  else
    viz_strip_kernel<1><<<dim3(ufr::stream_grid(6 * HW, kBlock), K), kBlock, 0, st>>>(adv_tgt, adv_ref, flow, adv_flow, g, record, w, H,
                                                                                    W, Hg, Wg, out);
  return ufr::launched("viz_strip_kernel");
}
