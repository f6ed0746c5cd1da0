// train_loss.hip -- the two training losses of the reference's `flowNetC or pwc` branch (training/utils.py:68-222), value and the
// gradient of every prediction, in three launches whatever the frame size (gfx950):
//   1. gt_area_kernel:   gt_i = the mean of every (H/h_i) x (W/w_i) block of gt (/ div_flow), float64, all scales in one launch;
//                        per workgroup, how many elements / pixels of gt_i are not NaN (the counts depend on the ground truth only);
//   2. loss_grad_kernel: every workgroup adds the counts of its scale (integers: exact), then writes the gradient of its pixels
//                        and leaves its partial sums (loss term, the metrics of scale 0);
//   3. loss_finalize_kernel: one workgroup adds the partials in a fixed order and writes `out`.
// No float atomics: two runs are bit-identical.  The work reads a few megabytes; float64 arithmetic costs nothing here.
#include "ufr_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSlots = 256;            // workgroups (= partials) per scale and kernel at most
constexpr int kMaxS = UFR_TRAIN_LOSS_MAX_SCALES;
constexpr int kSums = 6;               // loss term, epe sum, epe count, < 1, < 3, < 5

struct Scales {
  int n;
  int h[kMaxS], w[kMaxS], ry[kMaxS], rx[kMaxS];
  int team[kMaxS];                     // lanes that share one block mean: a power of two <= 64
  int wg1[kMaxS + 1], wg2[kMaxS + 1];  // first workgroup of each scale in kernel 1 / kernel 2
  long off[kMaxS];                     // where gt_i starts in the workspace
  double weight[kMaxS];
};

__device__ inline int find_scale(const int* wg0, int n, int wg) {
  int s = 0;
  while (s + 1 < n && wg >= wg0[s + 1]) ++s;
  return s;
}

using ufr::dev::block_sum;          // the sum over the workgroup in a fixed order, returned to every thread

__global__ __launch_bounds__(kBlock) void gt_area_kernel(Scales sc, const float* __restrict__ gt, int B, int H, int W, double div_flow,
                                                         double* __restrict__ gtm, double* __restrict__ cnt) {
  __shared__ double lds[kBlock / 64];
  const int s = find_scale(sc.wg1, sc.n, blockIdx.x);
  const int nwg = sc.wg1[s + 1] - sc.wg1[s], wg = blockIdx.x - sc.wg1[s];
  const int h = sc.h[s], w = sc.w[s], ry = sc.ry[s], rx = sc.rx[s], T = sc.team[s];
  const long npix = (long)B * h * w;
  const int per = kBlock / T, lane = threadIdx.x & (T - 1), area = ry * rx;
  double* __restrict__ dst = gtm + sc.off[s];
  double n_elem = 0.0, n_pix = 0.0;
  for (long base = (long)wg * per; base < npix; base += (long)nwg * per) {       // uniform over the workgroup: the shuffles below
    const long p = base + threadIdx.x / T;
    const bool valid = p < npix;
    const long pc = valid ? p : 0;
    const int x = (int)(pc % w), y = (int)((pc / w) % h), b = (int)(pc / ((long)w * h));
    double m[2];
    for (int c = 0; c < 2; ++c) {
      const float* __restrict__ src = gt + (((long)b * 2 + c) * H + (long)y * ry) * W + (long)x * rx;
      double acc = 0.0;
      if (valid)
        for (int j = lane; j < area; j += T) acc += (double)src[(long)(j / rx) * W + (j % rx)];
      for (int off = T >> 1; off > 0; off >>= 1) acc += __shfl_down(acc, off, T);
      acc /= (double)area;
      if (div_flow > 1.0) acc /= div_flow;
      m[c] = acc;
    }
    if (valid && lane == 0) {
      dst[(((long)b * 2 + 0) * h + y) * w + x] = m[0];
      dst[(((long)b * 2 + 1) * h + y) * w + x] = m[1];
      const bool ok0 = m[0] == m[0], ok1 = m[1] == m[1];
      n_elem += (ok0 ? 1.0 : 0.0) + (ok1 ? 1.0 : 0.0);
      n_pix += (ok0 && ok1) ? 1.0 : 0.0;
    }
  }
  n_elem = block_sum<kBlock>(n_elem, lds);
  n_pix = block_sum<kBlock>(n_pix, lds);
  if (threadIdx.x == 0) {
    cnt[((long)s * kSlots + wg) * 2 + 0] = n_elem;
    cnt[((long)s * kSlots + wg) * 2 + 1] = n_pix;
  }
}

// the non-NaN count of scale s: the per-workgroup counts of kernel 1 are integers, their sum is exact in any order
__device__ inline double scale_count(const Scales& sc, int s, int kind, const double* __restrict__ cnt, double* lds) {
  const int n1 = sc.wg1[s + 1] - sc.wg1[s];
  double c = 0.0;
  for (int i = threadIdx.x; i < n1; i += kBlock) c += cnt[((long)s * kSlots + i) * 2 + kind];
  return block_sum<kBlock>(c, lds);
}

__global__ __launch_bounds__(kBlock) void loss_grad_kernel(Scales sc, ufr_train_loss_desc d, const double* __restrict__ gtm,
                                                           const double* __restrict__ cnt, double* __restrict__ part) {
  __shared__ double lds[kBlock / 64];
  const int s = find_scale(sc.wg2, sc.n, blockIdx.x);
  const int nwg = sc.wg2[s + 1] - sc.wg2[s], wg = blockIdx.x - sc.wg2[s];
  const int h = sc.h[s], w = sc.w[s];
  const long hw = (long)h * w, npix = (long)d.B * hw;
  const double count = scale_count(sc, s, d.kind, cnt, lds);
  const double gscale = count > 0.0 ? sc.weight[s] / count : 0.0;
  const double sx = (double)w / (double)d.W, sy = (double)h / (double)d.H;
  const float* __restrict__ pred = d.pred[s];
  float* __restrict__ grad = d.grad[s];
  const double* __restrict__ g = gtm + sc.off[s];
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double sum[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long p = (long)wg * kBlock + threadIdx.x; p < npix; p += (long)nwg * kBlock) {
    const long i0 = (p / hw) * 2 * hw + p % hw, i1 = i0 + hw;
    const double u0 = g[i0], u1 = g[i1];                       // the interpolated ground truth, before the scaling
    const double p0 = (double)pred[i0], p1 = (double)pred[i1];
    const double d0 = p0 - u0 * sx, d1 = p1 - u1 * sy;
    const bool nan0 = u0 != u0, nan1 = u1 != u1;
    double g0, g1, epe;
    if (d.kind == 0) {
      sum[0] += (nan0 ? 0.0 : fabs(d0)) + (nan1 ? 0.0 : fabs(d1));
      g0 = nan0 ? 0.0 : gscale * (d0 > 0.0 ? 1.0 : d0 < 0.0 ? -1.0 : d0);       // sign(); a NaN prediction stays a NaN
      g1 = nan1 ? 0.0 : gscale * (d1 > 0.0 ? 1.0 : d1 < 0.0 ? -1.0 : d1);
      epe = sqrt(d0 * d0 + d1 * d1);                           // against the scaled ground truth, no NaN filter
      if (s == 0) {
        sum[1] += epe;
        sum[2] += 1.0;
      }
    } else {
      const double e = sqrt(d0 * d0 + d1 * d1 + 1e-5);
      if (nan0 || nan1) {
        g0 = g1 = count > 0.0 ? nan : 0.0;                     // autograd's answer through the boolean mask; a skipped scale has none
      } else {
        sum[0] += e;
        g0 = gscale * d0 / e;
        g1 = gscale * d1 / e;
      }
      const double e0 = p0 - u0, e1 = p1 - u1;                 // against the unscaled ground truth, NaN entries dropped
      epe = sqrt(e0 * e0 + e1 * e1);
      if (s == 0 && epe == epe) {
        sum[1] += epe;
        sum[2] += 1.0;
      }
    }
    if (s == 0 && epe == epe) {
      sum[3] += epe < 1.0 ? 1.0 : 0.0;
      sum[4] += epe < 3.0 ? 1.0 : 0.0;
      sum[5] += epe < 5.0 ? 1.0 : 0.0;
    }
    grad[i0] = (float)g0;
    grad[i1] = (float)g1;
  }
  for (int k = 0; k < kSums; ++k) {
    const double t = block_sum<kBlock>(sum[k], lds);
    if (threadIdx.x == 0) part[((long)s * kSlots + wg) * kSums + k] = t;
  }
}

__global__ __launch_bounds__(kBlock) void loss_finalize_kernel(Scales sc, int kind, const double* __restrict__ cnt,
                                                               const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double lds[kBlock / 64];
  double loss = 0.0, metric[kSums - 1] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < sc.n; ++s) {
    const double count = scale_count(sc, s, kind, cnt, lds);
    const int n2 = sc.wg2[s + 1] - sc.wg2[s];                  // <= kSlots = kBlock: one partial per thread
    for (int k = 0; k < (s == 0 ? kSums : 1); ++k) {
      const double t = block_sum<kBlock>((int)threadIdx.x < n2 ? part[((long)s * kSlots + threadIdx.x) * kSums + k] : 0.0, lds);
      if (k == 0) {
        if (kind == 0 || count > 0.0) loss += sc.weight[s] * (t / count);        // kind 0: an empty mean is 0/0 = NaN, as in torch
      } else {
        metric[k - 1] = t;
      }
    }
  }
  if (threadIdx.x == 0) {
    out[0] = loss;
    for (int k = 0; k < kSums - 1; ++k) out[1 + k] = metric[k];
    out[6] = out[7] = 0.0;
  }
}

inline int team_of(int area) {
  int t = 1;
  while (t * 2 <= area && t < 64) t *= 2;
  return t;
}

inline int clamp_slots(long g) { return (int)(g < 1 ? 1 : g > kSlots ? kSlots : g); }

long gtm_doubles(int B, int nscale, const int* h, const int* w) {
  long total = 0;
  for (int i = 0; i < nscale; ++i) total += 2L * B * h[i] * w[i];
  return total;
}

}  // namespace

extern "C" long ufr_train_loss_workspace_doubles(int B, int nscale, const int* h, const int* w) {
  if (B < 1 || nscale < 1 || nscale > kMaxS || !h || !w) return -1;
  for (int i = 0; i < nscale; ++i)
    if (h[i] < 1 || w[i] < 1) return -1;
  return gtm_doubles(B, nscale, h, w) + (long)nscale * kSlots * (2 + kSums);
}

extern "C" int ufr_train_loss(const ufr_train_loss_desc* d, ufr_stream_t stream) {
  UFR_REQUIRE(d, "train loss: null descriptor");
  UFR_REQUIRE(d->nscale >= 1 && d->nscale <= kMaxS, "train loss: %d scales, 1 .. %d are served", d->nscale, kMaxS);
  UFR_REQUIRE(d->kind == 0 || d->kind == 1, "train loss: kind %d (0 = sequence_loss, 1 = multiscale_epe)", d->kind);
  UFR_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0, "train loss: ground truth of %d x 2 x %d x %d: sizes must be positive", d->B, d->H, d->W);
  UFR_REQUIRE(d->gt && d->out && d->ws, "train loss: null pointer (gt, out or ws)");
  Scales sc;
  sc.n = d->nscale;
  sc.wg1[0] = sc.wg2[0] = 0;
  long off = 0;
  for (int i = 0; i < d->nscale; ++i) {
    UFR_REQUIRE(d->h[i] > 0 && d->w[i] > 0, "train loss: scale %d is %d x %d: sizes must be positive", i, d->h[i], d->w[i]);
    UFR_REQUIRE(d->H % d->h[i] == 0 && d->W % d->w[i] == 0,
                "train loss: scale %d (%d x %d) does not divide the ground truth (%d x %d): only integer ratios are served", i, d->h[i],
                d->w[i], d->H, d->W);
    UFR_REQUIRE(d->pred[i] && d->grad[i], "train loss: null pointer (pred or grad of scale %d)", i);
    sc.h[i] = d->h[i]; sc.w[i] = d->w[i];
    sc.ry[i] = d->H / d->h[i]; sc.rx[i] = d->W / d->w[i];
    UFR_REQUIRE((long)sc.ry[i] * sc.rx[i] <= (1L << 24), "train loss: scale %d averages blocks of %d x %d", i, sc.ry[i], sc.rx[i]);
    sc.team[i] = team_of(sc.ry[i] * sc.rx[i]);
    const long npix = (long)d->B * d->h[i] * d->w[i];
    const int per = kBlock / sc.team[i];
    sc.wg1[i + 1] = sc.wg1[i] + clamp_slots((npix + 4L * per - 1) / (4L * per));
    sc.wg2[i + 1] = sc.wg2[i] + clamp_slots((npix + 2L * kBlock - 1) / (2L * kBlock));
    sc.off[i] = off;
    sc.weight[i] = d->weight[i];
    off += 2L * npix;
  }
  const long need = off + (long)d->nscale * kSlots * (2 + kSums);
  UFR_REQUIRE(d->ws_elems >= need, "train loss: the workspace holds %ld doubles, %ld are needed", d->ws_elems, need);
  double* gtm = d->ws;
  double* cnt = d->ws + off;
  double* part = cnt + (long)d->nscale * kSlots * 2;
  hipStream_t st = ufr::as_stream(stream);
  hipLaunchKernelGGL(gt_area_kernel, dim3(sc.wg1[sc.n]), dim3(kBlock), 0, st, sc, d->gt, d->B, d->H, d->W, d->div_flow, gtm, cnt);
  int rc = ufr::launched("gt_area_kernel");
  if (rc != UFR_OK) return rc;
  hipLaunchKernelGGL(loss_grad_kernel, dim3(sc.wg2[sc.n]), dim3(kBlock), 0, st, sc, *d, gtm, cnt, part);
  rc = ufr::launched("loss_grad_kernel");
  if (rc != UFR_OK) return rc;
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(kBlock), 0, st, sc, d->kind, cnt, part, d->out);
  return ufr::launched("loss_finalize_kernel");
}
