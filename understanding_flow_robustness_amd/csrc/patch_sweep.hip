// patch_sweep.hip -- the patch location sweep of patch_attacks/test_moving_patch.py:299-445 (gfx950): the finished patch is moved
// over ONE clean frame pair and the end-point error / cosine similarity against the blended ground truth is recorded per position.
// Two streaming entries serve a chunk of K positions:
//   ufr_sweep_paste    the K adversarial pairs from the one clean pair -- as canvases [K,3,H,W], or, for the windowed prefix, only
//                      the window around each position's patch (the window table of ufr_cone_window first, then the windows);
//   ufr_sweep_metrics  resized prediction, resized canvas mask, blended ground truth, both metrics and their weighted means in one
//                      pass over the ground-truth pixels; float64 throughout, the per-item metrics scheme of ufr_common.h.
// The reference does, per position: three canvas-sized host arrays, one H2D copy, five torch operators for the paste, a bilinear
// resize of the mask, five for the blend, two metric calls that each end in `.item()`.
#include <climits>

#include "patch_eval_dev.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSlots = ufr::kMetricSlots;
constexpr int kSums = 3;               // valid * epe, valid * cos, valid
constexpr int kWinInts = 8;            // win[k] = {y0, x0, need_h, need_w, ymin, ymax, xmin, xmax} (window.hip)

using ufr::aligned16;
using ufr::dev::cone_axis;
using ufr::dev::paste_clamped;      // attack.hip's paste_placed_kernel, do_clamp = 1

// ---- canvas form: idx runs over [K,3,H,W] in units of V floats; the clean pair is [3,H,W] ---------------------------------------
template <int V>
__global__ __launch_bounds__(kBlock) void sweep_paste_canvas_kernel(const float* __restrict__ tgt, const float* __restrict__ ref,
                                                                    const float* __restrict__ patch_p, const float* __restrict__ mask_p,
                                                                    const int* __restrict__ origins, float* __restrict__ adv_tgt,
                                                                    float* __restrict__ adv_ref, long total, int H, int W, int ph,
                                                                    int pw, float lo, float hi) {
  const long HW = (long)H * W, CHW = 3 * HW;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const long idx = q * V;
    const int k = (int)(idx / CHW);
    const long src = idx - (long)k * CHW;
    const int c = (int)(src / HW);
    const long pix = src - (long)c * HW;
    const int y = (int)(pix / W), x = (int)(pix - (long)y * W);
    const int i = y - origins[2 * k], j0 = x - origins[2 * k + 1];
    float t[V], r[V];
    if constexpr (V == 4) {
      const float4 tv = *reinterpret_cast<const float4*>(tgt + src), rv = *reinterpret_cast<const float4*>(ref + src);
      t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
      r[0] = rv.x; r[1] = rv.y; r[2] = rv.z; r[3] = rv.w;
    } else {
      t[0] = tgt[src];
      r[0] = ref[src];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int j = j0 + v;
      float m = 0.f, pv = 0.f;
      if ((unsigned)i < (unsigned)ph && (unsigned)j < (unsigned)pw) {
        const int e = (c * ph + i) * pw + j;
        m = mask_p[e];
        pv = patch_p[e];
      }
      t[v] = paste_clamped(t[v], m, pv, lo, hi);
      r[v] = paste_clamped(r[v], m, pv, lo, hi);
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(adv_tgt + idx) = make_float4(t[0], t[1], t[2], t[3]);
      *reinterpret_cast<float4*>(adv_ref + idx) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
      adv_tgt[idx] = t[0];
      adv_ref[idx] = r[0];
    }
  }
}

// ---- window form, first launch: the window table (window.hip's cone_axis: ufr_common.h) -----------------------------------------

// One workgroup: the box of mask_p != 0 (all channels), then per position the table ufr_cone_window computes from the canvas mask,
// whose box is origin + that box (the host has checked that every placement lies inside the frame).
__global__ __launch_bounds__(kBlock) void sweep_window_table_kernel(const float* __restrict__ mask_p, const int* __restrict__ origins,
                                                                    int* __restrict__ win, int K, int H, int W, int ph, int pw,
                                                                    const ufr_cone_chain ch, int win_h, int win_w) {
  __shared__ int box[4];       // imin, imax, jmin, jmax
  const int tid = threadIdx.x, n = 3 * ph * pw, plane = ph * pw;
  if (tid == 0) { box[0] = INT_MAX; box[1] = -1; box[2] = INT_MAX; box[3] = -1; }
  __syncthreads();
  int imin = INT_MAX, imax = -1, jmin = INT_MAX, jmax = -1;
  for (int e = tid; e < n; e += kBlock) {
    if (mask_p[e] != 0.f) {
      const int r = e % plane, i = r / pw, j = r - i * pw;
      imin = min(imin, i); imax = max(imax, i); jmin = min(jmin, j); jmax = max(jmax, j);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    imin = min(imin, __shfl_xor(imin, o)); imax = max(imax, __shfl_xor(imax, o));
    jmin = min(jmin, __shfl_xor(jmin, o)); jmax = max(jmax, __shfl_xor(jmax, o));
  }
  if ((tid & 63) == 0 && imax >= 0) {      // integer min / max in LDS: exact in any order
    atomicMin(&box[0], imin); atomicMax(&box[1], imax); atomicMin(&box[2], jmin); atomicMax(&box[3], jmax);
  }
  __syncthreads();
  for (int k = tid; k < K; k += kBlock) {
    const int oy = origins[2 * k], ox = origins[2 * k + 1];
    int ymin = INT_MAX, ymax = -1, xmin = INT_MAX, xmax = -1;
    if (box[1] >= 0) { ymin = oy + box[0]; ymax = oy + box[1]; xmin = ox + box[2]; xmax = ox + box[3]; }
    int* w = win + k * kWinInts;
    w[4] = ymin; w[5] = ymax; w[6] = xmin; w[7] = xmax;
    int o0, o1, n0, n1;
    cone_axis(ymin, ymax, H, ch, win_h, &o0, &n0);
    cone_axis(xmin, xmax, W, ch, win_w, &o1, &n1);
    w[0] = o0; w[1] = o1; w[2] = n0; w[3] = n1;
  }
}

// ---- window form, second launch: xw [2K,3,wh,ww] = windows of the K pasted first frames, then of the K pasted second frames -------
// q runs over [K,3,wh,ww] in units of V floats; both frames of a position leave the same thread (one mask / patch lookup).
template <int V>
__global__ __launch_bounds__(kBlock) void sweep_paste_window_kernel(const float* __restrict__ tgt, const float* __restrict__ ref,
                                                                    const float* __restrict__ patch_p, const float* __restrict__ mask_p,
                                                                    const int* __restrict__ origins, const int* __restrict__ win,
                                                                    float* __restrict__ xw, long total, int K, int H, int W, int wh,
                                                                    int ww, int ph, int pw, float lo, float hi) {
  const long HW = (long)H * W, whw = (long)wh * ww, half = (long)K * 3 * whw;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const long e = q * V;
    const int k = (int)(e / (3 * whw));
    const long r = e - (long)k * 3 * whw;
    const int c = (int)(r / whw);
    const long wp = r - (long)c * whw;
    const int ii = (int)(wp / ww), jj = (int)(wp - (long)ii * ww);
    const int* w = win + k * kWinInts;
    // clamped like ufr_window_gather_pair: the window always lies inside the frame
    const int y0 = min(max(w[0], 0), H - wh), x0 = min(max(w[1], 0), W - ww);
    const int y = y0 + ii, x = x0 + jj;
    const long src = (long)c * HW + (long)y * W + x;
    const int i = y - origins[2 * k], j0 = x - origins[2 * k + 1];
    float t[V], s[V];
    if constexpr (V == 4) {          // x0 is a multiple of the chain's total stride (a multiple of 4, checked by the host) or W - ww
      const float4 tv = *reinterpret_cast<const float4*>(tgt + src), rv = *reinterpret_cast<const float4*>(ref + src);
      t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
      s[0] = rv.x; s[1] = rv.y; s[2] = rv.z; s[3] = rv.w;
    } else {
      t[0] = tgt[src];
      s[0] = ref[src];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int j = j0 + v;
      float m = 0.f, pv = 0.f;
      if ((unsigned)i < (unsigned)ph && (unsigned)j < (unsigned)pw) {
        const int pe = (c * ph + i) * pw + j;
        m = mask_p[pe];
        pv = patch_p[pe];
      }
      t[v] = paste_clamped(t[v], m, pv, lo, hi);
      s[v] = paste_clamped(s[v], m, pv, lo, hi);
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(xw + e) = make_float4(t[0], t[1], t[2], t[3]);
      *reinterpret_cast<float4*>(xw + half + e) = make_float4(s[0], s[1], s[2], s[3]);
    } else {
      xw[e] = t[0];
      xw[half + e] = s[0];
    }
  }
}

// ---- metrics ------------------------------------------------------------------------------------------------------------------
using ufr::dev::epe_cos;
using ufr::dev::FlowTaps;           // torch's upsample_bilinear2d, align_corners = False, in float64
using ufr::dev::flow_taps;
using ufr::dev::sample;
using ufr::dev::sweep_ground_truth;  // the canvas mask at the prediction's taps, the blend (patch_eval_dev.h)

// grid (slots, K): workgroup (s, k) walks the ground-truth pixels s * 256 + t, + slots * 256, ... of position k
__global__ __launch_bounds__(kBlock) void sweep_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                               const float* __restrict__ mask_p, const int* __restrict__ origins,
                                                               int H, int W, int Hg, int Wg, int ph, int pw, double patch_valid,
                                                               double* __restrict__ part) {
  __shared__ double lds[kBlock / 64];
  const int k = blockIdx.y;
  const long HW = (long)H * W, HWg = (long)Hg * Wg;
  const float* __restrict__ pu = pred + (long)k * 2 * HW;
  const float* __restrict__ pv = pu + HW;
  const double sy = (double)H / (double)Hg, sx = (double)W / (double)Wg;
  const double scale_u = (double)Wg / (double)W, scale_v = (double)Hg / (double)H;     // losses.py:27
  int oy = 0, ox = 0;
  if (mask_p != nullptr) { oy = origins[2 * k]; ox = origins[2 * k + 1]; }
  double sum[kSums] = {0.0, 0.0, 0.0};
  for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < HWg; p += (long)gridDim.x * kBlock) {
    const FlowTaps s = flow_taps(p, Wg, sy, sx, H, W);
    const double fu = sample(pu, s), fv = sample(pv, s);
    double g[3];
    sweep_ground_truth(gt, p, HWg, mask_p, oy, ox, ph, pw, patch_valid, s, g);       // test_moving_patch.py:430-432
    double epe, cs;                                                               // losses.py:29-30: the error against the rescaled
    epe_cos(g[0] - fu * scale_u, g[1] - fv * scale_v, g[0], g[1], fu, fv, epe, cs);  // prediction, the cosine with it as it is
    sum[0] += epe * g[2];
    sum[1] += cs * g[2];
    sum[2] += g[2];
  }
  ufr::dev::store_partial<kBlock, kSums>(sum, lds, part, k, kSlots);
}

// grid K: one workgroup adds the `slots` partials of its position in a fixed order
__global__ __launch_bounds__(kBlock) void sweep_metrics_finalize_kernel(const double* __restrict__ part, int slots,
                                                                        float* __restrict__ out) {
  __shared__ double lds[kBlock / 64];
  const int k = blockIdx.x;
  double t[kSums];
  ufr::dev::item_totals<kBlock, kSums>(part, k, kSlots, slots, lds, t);
  if (threadIdx.x == 0) {
    const double den = t[2] + 1e-8;                                               // losses.py:22
    out[2 * k] = (float)(t[0] / den);
    out[2 * k + 1] = (float)(t[1] / den);
  }
}

}  // namespace

extern "C" int ufr_sweep_paste(const float* tgt, const float* ref, const float* patch_p, const float* mask_p, const int* origins,
                               const int* origins_host, float* adv_tgt, float* adv_ref, int K, int H, int W, int ph, int pw, float lo,
                               float hi, const ufr_cone_chain* chain, int win_h, int win_w, int* win, float* xw, ufr_stream_t stream) {
  UFR_REQUIRE(tgt && ref && patch_p && mask_p && origins, "sweep paste: null pointer argument");
  UFR_REQUIRE(origins_host, "sweep paste: the origins are needed on the host too (every placement is checked before the launch)");
  UFR_REQUIRE(K > 0 && H > 0 && W > 0 && ph > 0 && pw > 0, "sweep paste: bad shape K=%d H=%d W=%d ph=%d pw=%d", K, H, W, ph, pw);
  UFR_REQUIRE(ph <= H && pw <= W, "sweep paste: the %dx%d patch is larger than the %dx%d frame", ph, pw, H, W);
  UFR_REQUIRE((long)K * 3 * H * W < (1L << 40) && (long)3 * ph * pw < (1L << 30), "sweep paste: too many pixels");
  UFR_REQUIRE(lo <= hi, "sweep paste: empty pixel range [%g, %g]", (double)lo, (double)hi);
  if (int rc = ufr::check_sweep_origins("sweep paste", origins_host, K, H, W, ph, pw)) return rc;
  hipStream_t st = ufr::as_stream(stream);
  if (win == nullptr) {
    UFR_REQUIRE(chain == nullptr && xw == nullptr, "sweep paste: a chain or window stack without the window table");
    UFR_REQUIRE(adv_tgt && adv_ref, "sweep paste: null pointer argument (canvas form: adv_tgt, adv_ref)");
    const long total = (long)K * 3 * H * W;
    if (W % 4 == 0 && aligned16(tgt, ref, adv_tgt, adv_ref))
      sweep_paste_canvas_kernel<4><<<ufr::stream_grid(total / 4, kBlock), kBlock, 0, st>>>(tgt, ref, patch_p, mask_p, origins, adv_tgt,
                                                                                         adv_ref, total / 4, H, W, ph, pw, lo, hi);
    else
      sweep_paste_canvas_kernel<1><<<ufr::stream_grid(total, kBlock), kBlock, 0, st>>>(tgt, ref, patch_p, mask_p, origins, adv_tgt,
                                                                                     adv_ref, total, H, W, ph, pw, lo, hi);
    return ufr::launched("sweep_paste_canvas_kernel");
  }
  UFR_REQUIRE(chain != nullptr, "sweep paste: the window form needs the chain");
  UFR_REQUIRE(xw != nullptr, "sweep paste: the window form needs the window stack xw");
  UFR_REQUIRE(chain->n_layers > 0 && chain->n_layers <= UFR_MAX_CONE_LAYERS && chain->n_taps > 0 &&
                  chain->n_taps <= UFR_MAX_CONE_LAYERS, "sweep paste: bad chain");
  int stride = 1;
  for (int l = 0; l < chain->n_layers; ++l) {
    UFR_REQUIRE(chain->kernel[l] > 0 && chain->stride[l] > 0 && chain->pad[l] >= 0, "sweep paste: bad layer %d", l);
    stride *= chain->stride[l];
  }
  for (int t = 0; t < chain->n_taps; ++t)
    UFR_REQUIRE(chain->tap_layer[t] >= 0 && chain->tap_layer[t] < chain->n_layers &&
                    (t == 0 || chain->tap_layer[t] >= chain->tap_layer[t - 1]) && chain->tap_margin[t] >= 0,
                "sweep paste: taps must be sorted by layer");
  UFR_REQUIRE(H % stride == 0 && W % stride == 0, "sweep paste: %dx%d is not a multiple of the chain stride %d", H, W, stride);
  UFR_REQUIRE(win_h > 0 && win_w > 0 && win_h % stride == 0 && win_w % stride == 0 && win_h <= H && win_w <= W,
              "sweep paste: window %dx%d must be a multiple of %d inside %dx%d", win_h, win_w, stride, H, W);
  sweep_window_table_kernel<<<1, kBlock, 0, st>>>(mask_p, origins, win, K, H, W, ph, pw, *chain, win_h, win_w);
  if (int rc = ufr::launched("sweep_window_table_kernel")) return rc;
  const long total = (long)K * 3 * win_h * win_w;
  // a window's first column is a multiple of the chain stride, or W - win_w when the clamp holds it inside the frame
  if (W % 4 == 0 && win_w % 4 == 0 && stride % 4 == 0 && aligned16(tgt, ref, xw))
    sweep_paste_window_kernel<4><<<ufr::stream_grid(total / 4, kBlock), kBlock, 0, st>>>(tgt, ref, patch_p, mask_p, origins, win, xw,
                                                                                       total / 4, K, H, W, win_h, win_w, ph, pw, lo, hi);
  else
    sweep_paste_window_kernel<1><<<ufr::stream_grid(total, kBlock), kBlock, 0, st>>>(tgt, ref, patch_p, mask_p, origins, win, xw, total,
                                                                                   K, H, W, win_h, win_w, ph, pw, lo, hi);
  return ufr::launched("sweep_paste_window_kernel");
}

extern "C" long ufr_sweep_metrics_workspace_doubles(int K) { return K < 1 ? -1 : (long)K * kSlots * kSums; }

extern "C" int ufr_sweep_metrics(const float* pred, const float* gt, const float* mask_p, const int* origins, const int* origins_host,
                                 int K, int H, int W, int Hg, int Wg, int ph, int pw, int valid_in_patch, double* ws, long ws_elems,
                                 float* out, int row0, int rows, ufr_stream_t stream) {
  UFR_REQUIRE(pred && gt && ws && out, "sweep metrics: null pointer argument");
  UFR_REQUIRE(K > 0 && K <= 65535 && H > 0 && W > 0 && Hg > 0 && Wg > 0, "sweep metrics: bad shape K=%d H=%d W=%d Hg=%d Wg=%d", K, H,
              W, Hg, Wg);
  UFR_REQUIRE((long)H * W < (1L << 30) && (long)Hg * Wg < (1L << 30), "sweep metrics: too many pixels");
  UFR_REQUIRE(valid_in_patch == 0 || valid_in_patch == 1, "sweep metrics: valid_in_patch = %d (0 or 1)", valid_in_patch);
  if (int rc = ufr::check_result_rows("sweep metrics", row0, K, rows)) return rc;
  if (int rc = ufr::check_workspace("sweep metrics", ws_elems, ufr_sweep_metrics_workspace_doubles(K))) return rc;
  if (mask_p != nullptr) {
    UFR_REQUIRE(origins && origins_host, "sweep metrics: null pointer argument (a patch needs its origins, on the device and the host)");
    UFR_REQUIRE(ph > 0 && pw > 0, "sweep metrics: bad shape ph=%d pw=%d", ph, pw);
    UFR_REQUIRE(ph <= H && pw <= W && (long)3 * ph * pw < (1L << 30), "sweep metrics: the %dx%d patch is larger than the %dx%d frame",
                ph, pw, H, W);
    if (int rc = ufr::check_sweep_origins("sweep metrics", origins_host, K, H, W, ph, pw)) return rc;
  }
  hipStream_t st = ufr::as_stream(stream);
  const int slots = ufr::metric_slots((long)Hg * Wg, kBlock);
  sweep_metrics_kernel<<<dim3(slots, K), kBlock, 0, st>>>(pred, gt, mask_p, origins, H, W, Hg, Wg, ph, pw, (double)valid_in_patch, ws);
  if (int rc = ufr::launched("sweep_metrics_kernel")) return rc;
  sweep_metrics_finalize_kernel<<<K, kBlock, 0, st>>>(ws, slots, out + 2L * row0);
  return ufr::launched("sweep_metrics_finalize_kernel");
}
