// patch_eval_dev.h -- the scored ground truth of the patch evaluation (test_patch.py:420-457) and of the location sweep
// (test_moving_patch.py:414-432), once each: ufr_eval_metrics (patch_eval.hip) and ufr_sweep_metrics (patch_sweep.hip) score it
// without storing it, ufr_eval_blend_gt and ufr_sweep_blend_gt (flow_viz.hip) write it for the figure.  Scorer and writer call the
// same device function, so the panel shows what was scored.  (The way convex_upsample_dev.h is shared.)
#pragma once
#include "ufr_common.h"

namespace ufr {
namespace dev {

constexpr int kEvalPlace = 8;          // places[k] = {y_tgt, x_tgt, h_tgt, w_tgt, y_ref, x_ref, h_ref, w_ref}

// What one item of a chunk brings to a ground-truth pixel: the slots of its records and where they lie in the frame
struct EvalItem {
  const float* __restrict__ gk;        // ground truth [3,Hg,Wg]
  const float* __restrict__ mt;        // first-frame mask slot [3,sh,sw]
  const float* __restrict__ mr;        // second-frame mask slot, or nullptr
  const float* __restrict__ fl;        // flow slot, or nullptr
  int yt, xt, ht, wt, yr, xr, hr, wr;
};

__device__ __forceinline__ EvalItem eval_item(const float* __restrict__ gt, const float* __restrict__ m_tgt,
                                              const float* __restrict__ m_ref, const float* __restrict__ flow,
                                              const int* __restrict__ places, int k, long HWg, int plane) {
  EvalItem it;
  it.gk = gt + (long)k * 3 * HWg;
  it.mt = m_tgt + (long)k * 3 * plane;
  it.mr = m_ref != nullptr ? m_ref + (long)k * 3 * plane : nullptr;
  it.fl = flow != nullptr ? flow + (long)k * 3 * plane : nullptr;
  const int* __restrict__ pl = places + (long)k * kEvalPlace;
  it.yt = pl[0]; it.xt = pl[1]; it.ht = pl[2]; it.wt = pl[3];
  it.yr = it.xr = it.hr = it.wr = 0;
  if (it.mr != nullptr) { it.yr = pl[4]; it.xr = pl[5]; it.hr = pl[6]; it.wr = pl[7]; }
  return it;
}

// Ground-truth pixel p with the taps `s` of the frame-sized arrays resized to it: g = gt' = (1 - mr) * gt, ga = (1 - mt) * gt' +
// mt * f (include/ufr_hip.h, ufr_eval_metrics).  patch_flow: 0 = (0, 0, 0), 1 = (0, 0, 1), 2 = the flow slot; zy / zx: scipy's zoom
// factors (H - 1) / (Hg - 1), (W - 1) / (Wg - 1)
__device__ __forceinline__ void eval_ground_truth(const EvalItem& it, long p, long HWg, const FlowTaps& s, int H, int W, int plane,
                                                  int sw, int patch_flow, double zy, double zx, double g[3], double ga[3]) {
  g[0] = (double)it.gk[p]; g[1] = (double)it.gk[HWg + p]; g[2] = (double)it.gk[2 * HWg + p];
  if (it.mr != nullptr) {                                                         // test_patch.py:430-446: occluded by the moved patch
    const Corners q = corners(s.y0, s.y1, s.x0, s.x1, it.yr, it.xr, it.hr, it.wr);
    if (q.any) {
#pragma unroll
      for (int c = 0; c < 3; ++c) g[c] = (1.0 - resized_canvas(it.mr + c * plane, sw, q, s.ly, s.lx)) * g[c];
    }
  }
  ga[0] = g[0]; ga[1] = g[1]; ga[2] = g[2];
  const Corners q = corners(s.y0, s.y1, s.x0, s.x1, it.yt, it.xt, it.ht, it.wt);
  if (q.any) {
    double f[3] = {0.0, 0.0, patch_flow == 1 ? 1.0 : 0.0};
    if (patch_flow == 2) {
      // scipy.ndimage.zoom, order 1, mode='constant' (placement.hip): a source outside [0, n - 1] on either axis gives 0
      const double cy = zy * (double)s.yg, cx = zx * (double)s.xg;
      if (!(cy < 0.0 || cy > (double)(H - 1) || cx < 0.0 || cx > (double)(W - 1))) {
        const int fy0 = (int)floor(cy), fx0 = (int)floor(cx);
        const double ty = cy - (double)fy0, tx = cx - (double)fx0;
        const int fy1 = fy0 + 1 < H ? fy0 + 1 : fy0, fx1 = fx0 + 1 < W ? fx0 + 1 : fx0;
        const double wy1 = fy0 + 1 < H ? ty : 0.0, wx1 = fx0 + 1 < W ? tx : 0.0, wy0 = 1.0 - ty, wx0 = 1.0 - tx;
        const Corners z = corners(fy0, fy1, fx0, fx1, it.yt, it.xt, it.ht, it.wt);
        if (z.any) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float* __restrict__ fc = it.fl + c * plane;
            double v = (z.a0 && z.b0 ? (double)fc[z.i0 * sw + z.j0] : 0.0) * (wy0 * wx0);
            v += (z.a0 && z.b1 ? (double)fc[z.i0 * sw + z.j1] : 0.0) * (wy0 * wx1);
            v += (z.a1 && z.b0 ? (double)fc[z.i1 * sw + z.j0] : 0.0) * (wy1 * wx0);
            v += (z.a1 && z.b1 ? (double)fc[z.i1 * sw + z.j1] : 0.0) * (wy1 * wx1);
            f[c] = v;
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double m = resized_canvas(it.mt + c * plane, sw, q, s.ly, s.lx);
      ga[c] = (1.0 - m) * g[c] + m * f[c];                                        // test_patch.py:455-457
    }
  }
}

// The sweep's ground truth at pixel p: g = (1 - m) * gt + m * (0, 0, patch_valid), m the canvas mask (mask_p [3,ph,pw] at (oy, ox),
// 0 elsewhere) resized to the ground truth's grid at the taps `s`; gt itself when mask_p is null (test_moving_patch.py:430-432)
__device__ __forceinline__ void sweep_ground_truth(const float* __restrict__ gt, long p, long HWg, const float* __restrict__ mask_p,
                                                   int oy, int ox, int ph, int pw, double patch_valid, const FlowTaps& s, double g[3]) {
  g[0] = (double)gt[p]; g[1] = (double)gt[HWg + p]; g[2] = (double)gt[2 * HWg + p];
  if (mask_p != nullptr) {
    // the canvas mask at the (already clamped) source rows / columns: mask_p inside the rectangle, 0 outside
    const Corners q = corners(s.y0, s.y1, s.x0, s.x1, oy, ox, ph, pw);
    if (q.any) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double m = resized_canvas(mask_p + (long)c * ph * pw, pw, q, s.ly, s.lx);
        g[c] = (1.0 - m) * g[c] + m * (c == 2 ? patch_valid : 0.0);
      }
    }
  }
}

}  // namespace dev

// every origin of a chunk of the sweep against the frame (host; before any launch; the callers have checked ph <= H, pw <= W)
inline int check_sweep_origins(const char* what, const int* origins_host, int K, int H, int W, int ph, int pw) {
  for (int k = 0; k < K; ++k)
    if (!(origins_host[2 * k] >= 0 && origins_host[2 * k] <= H - ph && origins_host[2 * k + 1] >= 0 && origins_host[2 * k + 1] <= W - pw))
      return fail(UFR_EINVAL, "%s: placement %d = (%d, %d) of the %dx%d patch leaves the %dx%d frame", what, k, origins_host[2 * k],
                  origins_host[2 * k + 1], ph, pw, H, W);
  return UFR_OK;
}

// every placement record of a chunk against its slot and the frame (host; before any launch)
inline int check_eval_places(const char* what, const int* places_host, int K, int records, int H, int W, int sh, int sw) {
  for (int k = 0; k < K; ++k)
    for (int r = 0; r < records; ++r) {
      const int* p = places_host + (long)k * dev::kEvalPlace + 4 * r;
      if (!(p[2] >= 1 && p[2] <= sh && p[3] >= 1 && p[3] <= sw))
        return fail(UFR_EINVAL, "%s: item %d, frame %d: the %dx%d record does not fit its %dx%d slot", what, k, r, p[2], p[3], sh, sw);
      if (!(p[0] >= 0 && p[0] <= H - p[2] && p[1] >= 0 && p[1] <= W - p[3]))
        return fail(UFR_EINVAL, "%s: item %d, frame %d: placement (%d, %d) of the %dx%d patch leaves the %dx%d frame", what, k, r,
                    p[0], p[1], p[2], p[3], H, W);
    }
  return UFR_OK;
}

}  // namespace ufr
