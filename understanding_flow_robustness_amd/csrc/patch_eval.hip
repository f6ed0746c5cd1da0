// patch_eval.hip -- the evaluation loop of patch_attacks/test_patch.py:242-466 (gfx950): a finished or hand-crafted patch is placed
// on every item of a validation set -- with `--different_pos` at another place, angle and scale in the second frame -- and the
// end-point error / cosine similarity of the clean and the attacked prediction are recorded per item.  Two streaming entries serve a
// chunk of K items, each with its own frames, ground truth and placement record (a slot in patch coordinates, include/ufr_hip.h):
//   ufr_eval_paste    the K adversarial pairs, one launch;
//   ufr_eval_metrics  resized predictions, resized canvas masks of both records, the occlusion of the ground truth by the second
//                     record, the patch's own flow resized by scipy's zoom rule, the blend and all four metrics in one pass over the
//                     ground-truth pixels; float64 throughout, the per-item metrics scheme of ufr_common.h.
// The reference does, per item: six canvas-sized host arrays and a canvas-sized flow, five H2D copies, ten torch operators for the
// pastes, two bilinear resizes, a scipy.ndimage.zoom of the canvas flow on the host, ten operators for the blends and four metric
// calls that each end in `.item()`.
#include "patch_eval_dev.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSlots = ufr::kMetricSlots;
constexpr int kSums = 6;               // clean: valid * epe, valid * cos, valid; attacked: the same three
constexpr int kPlace = ufr::dev::kEvalPlace;

using ufr::aligned16;
using ufr::dev::epe_cos;
using ufr::dev::eval_ground_truth;
using ufr::dev::eval_item;
using ufr::dev::EvalItem;
using ufr::dev::FlowTaps;
using ufr::dev::flow_taps;
using ufr::dev::paste_clamped;
using ufr::dev::sample;

// idx runs over [K,3,H,W] in units of V floats; the first frame takes record 0 of its item, the second frame record `second`
template <int V>
__global__ __launch_bounds__(kBlock) void eval_paste_kernel(const float* __restrict__ tgt, const float* __restrict__ ref,
                                                            const float* __restrict__ p_tgt, const float* __restrict__ m_tgt,
                                                            const float* __restrict__ p_ref, const float* __restrict__ m_ref,
                                                            const int* __restrict__ places, int second, float* __restrict__ adv_tgt,
                                                            float* __restrict__ adv_ref, long total, int H, int W, int sh, int sw,
                                                            float lo, float hi) {
  const long HW = (long)H * W, CHW = 3 * HW;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const long idx = q * V;
    const int k = (int)(idx / CHW);
    const long src = idx - (long)k * CHW;
    const int c = (int)(src / HW);
    const long pix = src - (long)c * HW;
    const int y = (int)(pix / W), x = (int)(pix - (long)y * W);
    const int* __restrict__ pl = places + (long)k * kPlace;
    const int* __restrict__ pr = pl + 4 * second;
    const int it = y - pl[0], jt0 = x - pl[1], ht = pl[2], wt = pl[3];
    const int ir = y - pr[0], jr0 = x - pr[1], hr = pr[2], wr = pr[3];
    const long slot = ((long)k * 3 + c) * sh * sw;
    float t[V], r[V];
    if constexpr (V == 4) {
      const float4 tv = *reinterpret_cast<const float4*>(tgt + idx), rv = *reinterpret_cast<const float4*>(ref + idx);
      t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
      r[0] = rv.x; r[1] = rv.y; r[2] = rv.z; r[3] = rv.w;
    } else {
      t[0] = tgt[idx];
      r[0] = ref[idx];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int jt = jt0 + v, jr = jr0 + v;
      float m = 0.f, pv = 0.f;
      if ((unsigned)it < (unsigned)ht && (unsigned)jt < (unsigned)wt) {
        const long e = slot + (long)it * sw + jt;
        m = m_tgt[e];
        pv = p_tgt[e];
      }
      t[v] = paste_clamped(t[v], m, pv, lo, hi);
      m = 0.f; pv = 0.f;
      if ((unsigned)ir < (unsigned)hr && (unsigned)jr < (unsigned)wr) {
        const long e = slot + (long)ir * sw + jr;
        m = m_ref[e];
        pv = p_ref[e];
      }
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

// ---- metrics ------------------------------------------------------------------------------------------------------------------
// losses.py:8-50 for one pixel: the end-point error against the rescaled prediction, the cosine with the prediction as it is
__device__ __forceinline__ void pixel_metrics(const double g[3], double fu, double fv, double scale_u, double scale_v, double* sum) {
  double epe, cs;
  epe_cos(g[0] - fu * scale_u, g[1] - fv * scale_v, g[0], g[1], fu, fv, epe, cs);
  sum[0] += epe * g[2];
  sum[1] += cs * g[2];
  sum[2] += g[2];
}

// grid (slots, K): workgroup (s, k) walks the ground-truth pixels s * 256 + t, + slots * 256, ... of item k
// the ground truth of a pixel: patch_eval_dev.h
__global__ __launch_bounds__(kBlock) void eval_metrics_kernel(const float* __restrict__ pred_clean, const float* __restrict__ pred_adv,
                                                              const float* __restrict__ gt, const float* __restrict__ m_tgt,
                                                              const float* __restrict__ m_ref, const float* __restrict__ flow,
                                                              const int* __restrict__ places, int H, int W, int Hg, int Wg, int sh,
                                                              int sw, int patch_flow, double zy, double zx, double* __restrict__ part) {
  __shared__ double lds[kBlock / 64];
  const int k = blockIdx.y;
  const long HW = (long)H * W, HWg = (long)Hg * Wg;
  const int plane = sh * sw;
  const float* __restrict__ cu = pred_clean + (long)k * 2 * HW;
  const float* __restrict__ cv = cu + HW;
  const float* __restrict__ au = pred_adv + (long)k * 2 * HW;
  const float* __restrict__ av = au + HW;
  const EvalItem it = eval_item(gt, m_tgt, m_ref, flow, places, k, HWg, plane);
  const double sy = (double)H / (double)Hg, sx = (double)W / (double)Wg;
  const double scale_u = (double)Wg / (double)W, scale_v = (double)Hg / (double)H;     // losses.py:27
  double sum[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < HWg; p += (long)gridDim.x * kBlock) {
    const FlowTaps s = flow_taps(p, Wg, sy, sx, H, W);
    const double pu = sample(cu, s), pv = sample(cv, s), qu = sample(au, s), qv = sample(av, s);
    double g[3], ga[3];
    eval_ground_truth(it, p, HWg, s, H, W, plane, sw, patch_flow, zy, zx, g, ga);
    pixel_metrics(g, pu, pv, scale_u, scale_v, sum);
    pixel_metrics(ga, qu, qv, scale_u, scale_v, sum + 3);
  }
  ufr::dev::store_partial<kBlock, kSums>(sum, lds, part, k, kSlots);
}

// grid K: one workgroup adds the `slots` partials of its item in a fixed order
__global__ __launch_bounds__(kBlock) void eval_metrics_finalize_kernel(const double* __restrict__ part, int slots,
                                                                       float* __restrict__ out) {
  __shared__ double lds[kBlock / 64];
  const int k = blockIdx.x;
  double t[kSums];
  ufr::dev::item_totals<kBlock, kSums>(part, k, kSlots, slots, lds, t);
  if (threadIdx.x == 0) {
    const double den = t[2] + 1e-8, den_adv = t[5] + 1e-8;                        // losses.py:22
    out[4 * k] = (float)(t[0] / den);                                             // epe, adv_epe, cos_sim, adv_cos_sim
    out[4 * k + 1] = (float)(t[3] / den_adv);
    out[4 * k + 2] = (float)(t[1] / den);
    out[4 * k + 3] = (float)(t[4] / den_adv);
  }
}

}  // namespace

extern "C" int ufr_eval_paste(const float* tgt, const float* ref, const float* p_tgt, const float* m_tgt, const float* p_ref,
                              const float* m_ref, const int* places, const int* places_host, float* adv_tgt, float* adv_ref, int K,
                              int H, int W, int sh, int sw, float lo, float hi, ufr_stream_t stream) {
  UFR_REQUIRE(tgt && ref && p_tgt && m_tgt && places && adv_tgt && adv_ref, "eval paste: null pointer argument");
  UFR_REQUIRE(places_host, "eval paste: the placements are needed on the host too (every record is checked before the launch)");
  UFR_REQUIRE((p_ref == nullptr) == (m_ref == nullptr), "eval paste: null pointer argument (a second-frame record is a patch AND a mask)");
  UFR_REQUIRE(K > 0 && H > 0 && W > 0 && sh > 0 && sw > 0, "eval paste: bad shape K=%d H=%d W=%d sh=%d sw=%d", K, H, W, sh, sw);
  UFR_REQUIRE(sh <= H && sw <= W, "eval paste: the %dx%d slot is larger than the %dx%d frame", sh, sw, H, W);
  UFR_REQUIRE((long)K * 3 * H * W < (1L << 40) && (long)K * 3 * sh * sw < (1L << 30), "eval paste: too many pixels");
  UFR_REQUIRE(lo <= hi, "eval paste: empty pixel range [%g, %g]", (double)lo, (double)hi);
  const int second = p_ref != nullptr ? 1 : 0;
  if (int rc = ufr::check_eval_places("eval paste", places_host, K, 1 + second, H, W, sh, sw)) return rc;
  if (!second) { p_ref = p_tgt; m_ref = m_tgt; }
  hipStream_t st = ufr::as_stream(stream);
  const long total = (long)K * 3 * H * W;
  if (W % 4 == 0 && aligned16(tgt, ref, adv_tgt, adv_ref))
    eval_paste_kernel<4><<<ufr::stream_grid(total / 4, kBlock), kBlock, 0, st>>>(tgt, ref, p_tgt, m_tgt, p_ref, m_ref, places, second,
                                                                               adv_tgt, adv_ref, total / 4, H, W, sh, sw, lo, hi);
  else
    eval_paste_kernel<1><<<ufr::stream_grid(total, kBlock), kBlock, 0, st>>>(tgt, ref, p_tgt, m_tgt, p_ref, m_ref, places, second,
                                                                           adv_tgt, adv_ref, total, H, W, sh, sw, lo, hi);
  return ufr::launched("eval_paste_kernel");
}

extern "C" long ufr_eval_metrics_workspace_doubles(int K) { return K < 1 ? -1 : (long)K * kSlots * kSums; }

extern "C" int ufr_eval_metrics(const float* pred_clean, const float* pred_adv, const float* gt, const float* m_tgt, const float* m_ref,
                                const float* flow, const int* places, const int* places_host, int K, int H, int W, int Hg, int Wg,
                                int sh, int sw, int ignore_mask_flow, double* ws, long ws_elems, float* out, int row0, int rows,
                                ufr_stream_t stream) {
  UFR_REQUIRE(pred_clean && pred_adv && gt && m_tgt && places && ws && out, "eval metrics: null pointer argument");
  UFR_REQUIRE(places_host, "eval metrics: the placements are needed on the host too (every record is checked before the launch)");
  UFR_REQUIRE(K > 0 && K <= 65535 && H > 0 && W > 0 && Hg > 0 && Wg > 0 && sh > 0 && sw > 0,
              "eval metrics: bad shape K=%d H=%d W=%d Hg=%d Wg=%d sh=%d sw=%d", K, H, W, Hg, Wg, sh, sw);
  UFR_REQUIRE(sh <= H && sw <= W, "eval metrics: the %dx%d slot is larger than the %dx%d frame", sh, sw, H, W);
  UFR_REQUIRE((long)H * W < (1L << 30) && (long)Hg * Wg < (1L << 30) && (long)K * 3 * sh * sw < (1L << 30),
              "eval metrics: too many pixels");
  UFR_REQUIRE(ignore_mask_flow == 0 || ignore_mask_flow == 1, "eval metrics: ignore_mask_flow = %d (0 or 1)", ignore_mask_flow);
  if (int rc = ufr::check_result_rows("eval metrics", row0, K, rows)) return rc;
  if (int rc = ufr::check_workspace("eval metrics", ws_elems, ufr_eval_metrics_workspace_doubles(K))) return rc;
  if (int rc = ufr::check_eval_places("eval metrics", places_host, K, m_ref != nullptr ? 2 : 1, H, W, sh, sw)) return rc;
  hipStream_t st = ufr::as_stream(stream);
  const int slots = ufr::metric_slots((long)Hg * Wg, kBlock);
  const int patch_flow = flow != nullptr ? 2 : (ignore_mask_flow ? 0 : 1);
  const double zy = Hg > 1 ? (double)(H - 1) / (double)(Hg - 1) : 1.0, zx = Wg > 1 ? (double)(W - 1) / (double)(Wg - 1) : 1.0;
  eval_metrics_kernel<<<dim3(slots, K), kBlock, 0, st>>>(pred_clean, pred_adv, gt, m_tgt, m_ref, flow, places, H, W, Hg, Wg, sh, sw,
                                                         patch_flow, zy, zx, ws);
  if (int rc = ufr::launched("eval_metrics_kernel")) return rc;
  eval_metrics_finalize_kernel<<<K, kBlock, 0, st>>>(ws, slots, out + 4L * row0);
  return ufr::launched("eval_metrics_finalize_kernel");
}
