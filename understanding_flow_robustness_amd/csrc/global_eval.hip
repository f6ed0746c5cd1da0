// global_eval.hip -- the evaluation of the global attacks (gfx950): global_attacks/perturb_main.py:466-812 runs, per validation item,
// a clean forward, the attack (or a fixed perturbation) and an attacked forward, and global_attacks/log_utils.py:226-528
// (`validate`) turns the noises, both predictions and the ground truth into the table of the paper.  Two streaming entries serve a
// chunk of K items:
//   ufr_global_apply    adv = clamp(image + noise, lo, hi) for both frames of the K pairs, one launch; the noise of one item may
//                       serve all of them (a universal perturbation);
//   ufr_global_metrics  the six flow metrics of `validate` (end-point error, L1 and cosine similarity of the clean and of the
//                       attacked prediction, each resized to the ground truth) and the four noise norms, one pass over the
//                       ground-truth pixels and one over the noise; float64 throughout, the per-item metrics scheme of ufr_common.h.
// The reference does, per item: five D2H copies, five `FloatTensor` uploads inside `validate`, six metric calls that each resize
// the prediction and end in `.item()`, and four numpy norms.
#include "ufr_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSlots = ufr::kMetricSlots;
// partials of one workgroup: [0..3] clean: w * epe, w * cos, sum |d| over non-NaN entries, their count; [4..7] attacked: the same;
// [8] sum of w; [9] sum |noise0|; [10] sum |noise1|; [11] max |noise0|; [12] max |noise1|
constexpr int kPart = 13;
constexpr int kSums = 11;
constexpr int kOut = 10;

using ufr::aligned16;
using ufr::dev::epe_cos;
using ufr::dev::FlowTaps;
using ufr::dev::flow_taps;
using ufr::dev::sample;

// numpy's max: a NaN stays
__device__ __forceinline__ double nan_max(double m, double a) { return (a > m || a != a) ? a : m; }

template <int BLOCK>
__device__ inline double block_max(double v, double* lds) {
  for (int off = 32; off > 0; off >>= 1) v = nan_max(v, __shfl_down(v, off, 64));
  __syncthreads();                                            // the previous use of lds is over
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = lds[0];
  for (int i = 1; i < BLOCK / 64; ++i) t = nan_max(t, lds[i]);
  return t;
}

// idx runs over [K,3,H,W] in units of V floats; CHW % V == 0, so a unit never leaves its item
template <int V>
__global__ __launch_bounds__(kBlock) void global_apply_kernel(const float* __restrict__ image0, const float* __restrict__ image1,
                                                              const float* __restrict__ noise0, const float* __restrict__ noise1,
                                                              float* __restrict__ adv0, float* __restrict__ adv1, long total, long CHW,
                                                              int broadcast, float lo, float hi) {
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const long idx = q * V;
    const long nidx = broadcast ? idx % CHW : idx;
    if constexpr (V == 4) {
      const float4 a = *reinterpret_cast<const float4*>(image0 + idx), b = *reinterpret_cast<const float4*>(image1 + idx);
      const float4 n = *reinterpret_cast<const float4*>(noise0 + nidx), m = *reinterpret_cast<const float4*>(noise1 + nidx);
      *reinterpret_cast<float4*>(adv0 + idx) = make_float4(fminf(fmaxf(a.x + n.x, lo), hi), fminf(fmaxf(a.y + n.y, lo), hi),
                                                           fminf(fmaxf(a.z + n.z, lo), hi), fminf(fmaxf(a.w + n.w, lo), hi));
      *reinterpret_cast<float4*>(adv1 + idx) = make_float4(fminf(fmaxf(b.x + m.x, lo), hi), fminf(fmaxf(b.y + m.y, lo), hi),
                                                           fminf(fmaxf(b.z + m.z, lo), hi), fminf(fmaxf(b.w + m.w, lo), hi));
    } else {
      adv0[idx] = fminf(fmaxf(image0[idx] + noise0[nidx], lo), hi);
      adv1[idx] = fminf(fmaxf(image1[idx] + noise1[nidx], lo), hi);
    }
  }
}

// perturb_model.py:38-99 for one pixel and one prediction (fu, fv), ALREADY rescaled: the error against it and the cosine with it;
// sum = (w * epe, w * cos, sum |d| over the non-NaN entries, their count)
__device__ __forceinline__ void pixel_metrics(double gu, double gv, double w, double fu, double fv, double* sum) {
  const double du = fu - gu, dv = fv - gv;
  double epe, cs;
  epe_cos(du, dv, gu, gv, fu, fv, epe, cs);
  sum[0] += epe * w;
  sum[1] += cs * w;
  const double au = fabs(du), av = fabs(dv);
  if (au == au) { sum[2] += au; sum[3] += 1.0; }
  if (av == av) { sum[2] += av; sum[3] += 1.0; }
}

// grid (slots, K): workgroup (s, k) walks the ground-truth pixels s * 256 + t, + slots * 256, ... of item k, then the noise
// elements of item k (of item 0 when one noise serves every item) in the same stride
__global__ __launch_bounds__(kBlock) void global_metrics_kernel(const float* __restrict__ pred_clean, const float* __restrict__ pred_adv,
                                                                const float* __restrict__ gt, const float* __restrict__ noise0,
                                                                const float* __restrict__ noise1, int gt_each, int noise_each, int C,
                                                                int H, int W, int Hg, int Wg, int vec, double* __restrict__ part) {
  __shared__ double lds[kBlock / 64];
  const int k = blockIdx.y;
  const long HW = (long)H * W, HWg = (long)Hg * Wg;
  const float* __restrict__ cu = pred_clean + (long)k * 2 * HW;
  const float* __restrict__ cv = cu + HW;
  const float* __restrict__ au = pred_adv + (long)k * 2 * HW;
  const float* __restrict__ av = au + HW;
  const float* __restrict__ gk = gt + (gt_each ? (long)k * C * HWg : 0L);
  const double sy = (double)H / (double)Hg, sx = (double)W / (double)Wg;
  const double scale_u = (double)Wg / (double)W, scale_v = (double)Hg / (double)H;     // perturb_model.py:44-45
  double sum[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double mx0 = 0.0, mx1 = 0.0;
  for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < HWg; p += (long)gridDim.x * kBlock) {
    const FlowTaps s = flow_taps(p, Wg, sy, sx, H, W);
    const double pu = sample(cu, s) * scale_u, pv = sample(cv, s) * scale_v;
    const double qu = sample(au, s) * scale_u, qv = sample(av, s) * scale_v;
    const double gu = (double)gk[p], gv = (double)gk[HWg + p];
    const double w = C == 3 ? (double)gk[2 * HWg + p] : 1.0;
    pixel_metrics(gu, gv, w, pu, pv, sum);
    pixel_metrics(gu, gv, w, qu, qv, sum + 4);
    sum[8] += w;
  }
  if (noise0 != nullptr) {
    const long CHW = 3 * HW;
    const float* __restrict__ n0 = noise0 + (noise_each ? (long)k * CHW : 0L);
    const float* __restrict__ n1 = noise1 + (noise_each ? (long)k * CHW : 0L);
    if (vec) {
      for (long q = (long)blockIdx.x * kBlock + threadIdx.x; q < CHW / 4; q += (long)gridDim.x * kBlock) {
        const float4 a = *reinterpret_cast<const float4*>(n0 + 4 * q), b = *reinterpret_cast<const float4*>(n1 + 4 * q);
        const double a4[4] = {fabs((double)a.x), fabs((double)a.y), fabs((double)a.z), fabs((double)a.w)};
        const double b4[4] = {fabs((double)b.x), fabs((double)b.y), fabs((double)b.z), fabs((double)b.w)};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          sum[9] += a4[v];
          sum[10] += b4[v];
          mx0 = nan_max(mx0, a4[v]);
          mx1 = nan_max(mx1, b4[v]);
        }
      }
    } else {
      for (long q = (long)blockIdx.x * kBlock + threadIdx.x; q < CHW; q += (long)gridDim.x * kBlock) {
        const double a = fabs((double)n0[q]), b = fabs((double)n1[q]);
        sum[9] += a;
        sum[10] += b;
        mx0 = nan_max(mx0, a);
        mx1 = nan_max(mx1, b);
      }
    }
  }
  double* __restrict__ mine = ufr::dev::store_partial<kBlock, kSums, kPart>(sum, lds, part, k, kSlots);
  const double t0 = block_max<kBlock>(mx0, lds);
  const double t1 = block_max<kBlock>(mx1, lds);
  if (threadIdx.x == 0) { mine[11] = t0; mine[12] = t1; }
}

// grid K: one workgroup adds the `slots` partials of its item in a fixed order
__global__ __launch_bounds__(kBlock) void global_metrics_finalize_kernel(const double* __restrict__ part, int slots, int C, double npix,
                                                                         double nframe, int with_noise, double* __restrict__ out) {
  __shared__ double lds[kBlock / 64];
  const int k = blockIdx.x;
  const bool mine = (int)threadIdx.x < slots;
  const double* __restrict__ p = part + ((long)k * kSlots + (mine ? threadIdx.x : 0)) * kPart;
  double t[kPart];
  ufr::dev::item_totals<kBlock, kSums, kPart>(part, k, kSlots, slots, lds, t);
  for (int q = kSums; q < kPart; ++q) t[q] = block_max<kBlock>(mine ? p[q] : 0.0, lds);
  if (threadIdx.x == 0) {
    double* __restrict__ o = out + (long)k * kOut;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    o[0] = with_noise ? t[11] : nan;                                              // eval_utils.lp_norm(p=0)
    o[1] = with_noise ? t[9] / nframe : nan;                                      // lp_norm(p=1, axis=-1) of the [H,W,3] view
    o[2] = with_noise ? t[12] : nan;
    o[3] = with_noise ? t[10] / nframe : nan;
    const double den = C == 3 ? t[8] + 1e-8 : npix;                               // perturb_model.py:49-54
    const double keep = C == 3 ? t[8] / (t[8] + 1e-8) : 1.0;                      // :94-99: l1 * valid summed, over sum(valid) + eps
    o[4] = t[0] / den;
    o[5] = t[4] / den;
    o[6] = t[2] / t[3] * keep;
    o[7] = t[6] / t[7] * keep;
    o[8] = t[1] / den;
    o[9] = t[5] / den;
  }
}

}  // namespace

extern "C" int ufr_global_apply(const float* image0, const float* image1, const float* noise0, const float* noise1, float* adv0,
                                float* adv1, int K, int Kn, int H, int W, float lo, float hi, ufr_stream_t stream) {
  UFR_REQUIRE(image0 && image1 && noise0 && noise1 && adv0 && adv1, "global apply: null pointer argument");
  UFR_REQUIRE(K > 0 && H > 0 && W > 0, "global apply: bad shape K=%d H=%d W=%d", K, H, W);
  UFR_REQUIRE(Kn == 1 || Kn == K, "global apply: %d noise items for %d images (1 or %d)", Kn, K, K);
  UFR_REQUIRE((long)K * 3 * H * W < (1L << 40), "global apply: too many pixels");
  UFR_REQUIRE(lo <= hi, "global apply: empty pixel range [%g, %g]", (double)lo, (double)hi);
  hipStream_t st = ufr::as_stream(stream);
  const long CHW = 3L * H * W, total = (long)K * CHW;
  const int broadcast = Kn == 1 && K > 1 ? 1 : 0;
  if (CHW % 4 == 0 && aligned16(image0, image1, noise0, noise1, adv0, adv1))
    global_apply_kernel<4><<<ufr::stream_grid(total / 4, kBlock), kBlock, 0, st>>>(image0, image1, noise0, noise1, adv0, adv1,
                                                                                 total / 4, CHW, broadcast, lo, hi);
  else
    global_apply_kernel<1><<<ufr::stream_grid(total, kBlock), kBlock, 0, st>>>(image0, image1, noise0, noise1, adv0, adv1, total, CHW,
                                                                             broadcast, lo, hi);
  return ufr::launched("global_apply_kernel");
}

extern "C" long ufr_global_metrics_workspace_doubles(int K) { return K < 1 ? -1 : (long)K * kSlots * kPart; }

extern "C" int ufr_global_metrics(const float* pred_clean, const float* pred_adv, const float* gt, const float* noise0,
                                  const float* noise1, int K, int Kg, int Kn, int C, int H, int W, int Hg, int Wg, double* ws,
                                  long ws_elems, double* out, int row0, int rows, ufr_stream_t stream) {
  UFR_REQUIRE(pred_clean && pred_adv && gt && ws && out, "global metrics: null pointer argument");
  UFR_REQUIRE((noise0 == nullptr) == (noise1 == nullptr), "global metrics: null pointer argument (both noises or neither)");
  UFR_REQUIRE(K > 0 && K <= 65535 && H > 0 && W > 0 && Hg > 0 && Wg > 0, "global metrics: bad shape K=%d H=%d W=%d Hg=%d Wg=%d", K, H, W,
              Hg, Wg);
  UFR_REQUIRE(Kg == 1 || Kg == K, "global metrics: %d ground truths for %d items (1 or %d)", Kg, K, K);
  UFR_REQUIRE(noise0 == nullptr || Kn == 1 || Kn == K, "global metrics: %d noise items for %d items (1 or %d)", Kn, K, K);
  UFR_REQUIRE(C == 2 || C == 3, "global metrics: %d ground-truth channels (2 or 3)", C);
  UFR_REQUIRE((long)H * W < (1L << 29) && (long)Hg * Wg < (1L << 29), "global metrics: too many pixels");
  if (int rc = ufr::check_result_rows("global metrics", row0, K, rows)) return rc;
  if (int rc = ufr::check_workspace("global metrics", ws_elems, ufr_global_metrics_workspace_doubles(K))) return rc;
  hipStream_t st = ufr::as_stream(stream);
  const long npix = (long)Hg * Wg, CHW = 3L * H * W;
  const int vec = noise0 != nullptr && CHW % 4 == 0 && aligned16(noise0, noise1) ? 1 : 0;
  // the workgroup count fixes the order of the sums: it follows from the sizes alone, never from the alignment that picks `vec`
  const long quads = noise0 != nullptr ? (CHW + 3) / 4 : 0;
  const int slots = ufr::metric_slots(quads > npix ? quads : npix, kBlock);
  global_metrics_kernel<<<dim3(slots, K), kBlock, 0, st>>>(pred_clean, pred_adv, gt, noise0, noise1, Kg == K ? 1 : 0, Kn == K ? 1 : 0, C,
                                                           H, W, Hg, Wg, vec, ws);
  if (int rc = ufr::launched("global_metrics_kernel")) return rc;
  global_metrics_finalize_kernel<<<K, kBlock, 0, st>>>(ws, slots, C, (double)npix, (double)H * (double)W, noise0 != nullptr ? 1 : 0,
                                                       out + (long)kOut * row0);
  return ufr::launched("global_metrics_finalize_kernel");
}
