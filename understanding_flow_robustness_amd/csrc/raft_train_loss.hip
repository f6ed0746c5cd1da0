// raft_train_loss.hip -- RAFT's branch of the training loss (training/utils.py:162-222, the `else` branches) with the convex upsampling
// that feeds it (models/raft/raft.py:111-122) folded in, value and the gradient of every low-resolution flow and mask, in three launches
// whatever the number of predictions (gfx950):
//   1. raft_loss_main:     convex_up_fwd's decomposition (a workgroup = 32 coarse columns of one row, 8 sub-pixel lanes per column, 8
//                          passes: mask reads and grad_mask writes in 128-byte runs).  The workgroup loads its gt / valid tile ONCE (16 + 8
//                          values per thread, in registers) and loops over the predictions: neighbours of flow_i, softmax, up, the loss
//                          term, g_up (never stored), grad_mask, and the 18 per-coarse-pixel sums a[k][c] (registers + LDS, fixed order)
//                          into the workspace; per prediction one float64 loss partial, at the end the metric partials: one row per
//                          workgroup;
//   2. raft_loss_gather:   grad_flow_i[n,c,h',w'] = 8 * sum_k a_i[k][c] at (h'-ky+1, w'-kx+1), all predictions in one launch;
//   3. raft_loss_finalize: one workgroup adds the partial rows in ascending order and writes `out`.
// `up` is built from convex_upsample_dev.h's softmax9 / neighbours and the fmaf chain of convex_up_fwd: bit-equal to what
// ufr_convex_upsample_forward writes.  No float atomics; the number of workgroups and the order of every sum follow from the shape
// alone: two runs are bit-identical.  The pointer tables travel by value in the kernel arguments.
#include "convex_upsample_dev.h"

namespace {

constexpr int RL_W = 32;           // coarse columns per workgroup
constexpr int RL_NT = 256;         // 8 sub-pixels x 32 columns per pass, 8 passes
constexpr int kMaxP = UFR_RAFT_LOSS_MAX_PREDS;
constexpr int kMetrics = 5;        // epe sum, epe count, < 1, < 3, < 5

using ufr::dev::block_sum;
using ufr::dev::neighbours;
using ufr::dev::signf;
using ufr::dev::softmax9;

struct GradFlows { float* g[kMaxP]; };
struct Weights { double w[kMaxP]; };

// a_ws [npred,B,2,9,H,W]; part [workgroups, npred + kMetrics]
__global__ __launch_bounds__(RL_NT) void raft_loss_main(ufr_raft_sequence_loss_desc d, double total, double* __restrict__ a_ws,
                                                        double* __restrict__ part) {
  __shared__ float lds_a[8][18][RL_W];
  __shared__ double lds_sum[RL_NT / 64];
  const int H = d.H, W = d.W;
  const int wl = threadIdx.x & (RL_W - 1), sub = threadIdx.x / RL_W;       // sub: the sub-pixel column j; pass t: the sub-pixel row i
  const int w = blockIdx.x * RL_W + wl, h = blockIdx.y, n = blockIdx.z;
  const bool inside = w < W;
  const size_t plane = (size_t)H * W, fplane = 64 * plane;
  const int width = d.npred + kMetrics;
  double* __restrict__ row = part + (((size_t)n * H + h) * gridDim.x + blockIdx.x) * width;

  // the ground truth and the mask v of this thread's 8 pixels
  float g0[8], g1[8], vf[8];
  {
    const bool divide = d.div_flow > 1.0;
    const float df = (float)d.div_flow, mf = (float)d.max_flow;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      g0[t] = g1[t] = vf[t] = 0.f;
      if (inside) {
        const size_t o = (size_t)(8 * h + t) * (8 * W) + 8 * w + sub;
        float a = d.gt[((size_t)n * 2 + 0) * fplane + o], b = d.gt[((size_t)n * 2 + 1) * fplane + o];
        if (divide) { a /= df; b /= df; }
        bool v = d.valid[(size_t)n * fplane + o] >= 0.5f;
        if (d.exclude_large) v = v && sqrtf(a * a + b * b) < mf;
        g0[t] = a; g1[t] = b; vf[t] = v ? 1.f : 0.f;
      }
    }
  }

  double m_sum = 0.0, m_cnt = 0.0, m_1 = 0.0, m_3 = 0.0, m_5 = 0.0;
  for (int p = 0; p < d.npred; ++p) {
    const float gs = (float)(d.weight[p] / total);
    const bool last = p == d.npred - 1;
    float acc[18];
#pragma unroll
    for (int q = 0; q < 18; ++q) acc[q] = 0.f;
    double lsum = 0.0;
    if (inside) {
      float f0[9], f1[9];
      neighbours(d.flow[p] + ((size_t)n * 2 + 0) * plane, h, w, H, W, f0);
      neighbours(d.flow[p] + ((size_t)n * 2 + 1) * plane, h, w, H, W, f1);
      const float* __restrict__ mp = d.mask[p] + (size_t)n * 576 * plane + (size_t)h * W + w;
      float* __restrict__ gm = d.grad_mask[p] + (size_t)n * 576 * plane + (size_t)h * W + w;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int ij = t * 8 + sub;
        float s[9];
        softmax9(mp + (size_t)ij * plane, 64 * plane, s);
        float u0 = 0.f, u1 = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) { u0 = fmaf(s[k], f0[k], u0); u1 = fmaf(s[k], f1[k], u1); }
        const float e0 = u0 - g0[t], e1 = u1 - g1[t];
        lsum += (double)(vf[t] * fabsf(e0)) + (double)(vf[t] * fabsf(e1));  // a product: a NaN ground truth reaches the loss
        if (last && vf[t] != 0.f) {
          const float epe = sqrtf(e0 * e0 + e1 * e1);
          m_sum += (double)epe;
          m_cnt += 1.0;
          m_1 += epe < 1.f ? 1.0 : 0.0;
          m_3 += epe < 3.f ? 1.0 : 0.0;
          m_5 += epe < 5.f ? 1.0 : 0.0;
        }
        const float gu0 = gs * vf[t] * signf(e0), gu1 = gs * vf[t] * signf(e1);  // d loss / d up_p at this pixel
        float dk[9], dbar = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) { dk[k] = gu0 * f0[k] + gu1 * f1[k]; dbar = fmaf(s[k], dk[k], dbar); }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          gm[((size_t)k * 64 + ij) * plane] = s[k] * (dk[k] - dbar);          // softmax adjoint
          acc[k] = fmaf(s[k], gu0, acc[k]);
          acc[9 + k] = fmaf(s[k], gu1, acc[9 + k]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 18; ++q) lds_a[sub][q][wl] = acc[q];
    __syncthreads();
    double* __restrict__ a_out = a_ws + ((size_t)p * gridDim.z + n) * 18 * plane + (size_t)h * W;
    for (int e = threadIdx.x; e < 18 * RL_W; e += RL_NT) {
      const int q = e / RL_W, l = e % RL_W, ww = blockIdx.x * RL_W + l;
      if (ww >= W) continue;
      double v = 0.0;
#pragma unroll
      for (int g = 0; g < 8; ++g) v += (double)lds_a[g][q][l];
      a_out[(size_t)q * plane + ww] = v;
    }
    lsum = block_sum<RL_NT>(lsum, lds_sum);        // its barriers also end this prediction's reads of lds_a
    if (threadIdx.x == 0) row[p] = lsum;
  }
  const double m[kMetrics] = {m_sum, m_cnt, m_1, m_3, m_5};
#pragma unroll
  for (int k = 0; k < kMetrics; ++k) {
    const double t = block_sum<RL_NT>(m[k], lds_sum);
    if (threadIdx.x == 0) row[d.npred + k] = t;
  }
}

// grid (x, npred): prediction blockIdx.y, a grid-stride walk over its [B,2,H,W] elements
__global__ __launch_bounds__(256) void raft_loss_gather(GradFlows gf, const double* __restrict__ a_ws, int B, int H, int W) {
  const size_t plane = (size_t)H * W;
  const long total = (long)B * 2 * plane;
  const double* __restrict__ a_p = a_ws + (size_t)blockIdx.y * total * 9;
  float* __restrict__ out = gf.g[blockIdx.y];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int w = (int)(i % W), h = (int)((i / W) % H);
    const long nc = i / (long)plane;
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {                      // the coarse pixel whose k-th neighbour is (h, w)
      const int hh = h - (k / 3 - 1), ww = w - (k % 3 - 1);
      if (hh >= 0 && hh < H && ww >= 0 && ww < W) v += a_p[((size_t)nc * 9 + k) * plane + (size_t)hh * W + ww];
    }
    out[i] = (float)(8.0 * v);
  }
}

__global__ __launch_bounds__(RL_NT) void raft_loss_finalize(Weights wt, const double* __restrict__ part, long rows, int npred,
                                                            double total, double* __restrict__ out) {
  __shared__ double lds[RL_NT / 64];
  const int width = npred + kMetrics;
  double loss = 0.0;
  for (int q = 0; q < width; ++q) {
    double s = 0.0;
    for (long r = threadIdx.x; r < rows; r += RL_NT) s += part[r * width + q];
    s = block_sum<RL_NT>(s, lds);
    if (q < npred) loss += wt.w[q] * (s / total);
    else if (threadIdx.x == 0) out[1 + q - npred] = s;
  }
  if (threadIdx.x == 0) {
    out[0] = loss;
    out[6] = out[7] = 0.0;
  }
}

inline bool shape_ok(int B, int H, int W, int npred) {
  return B > 0 && B <= 65535 && H > 0 && H <= 65535 && W > 0 && npred >= 1 && npred <= kMaxP;
}

inline long groups(int B, int H, int W) { return (long)B * H * ufr::ceil_div(W, RL_W); }

}  // namespace

extern "C" long ufr_raft_sequence_loss_workspace_doubles(int B, int H, int W, int npred) {
  if (!shape_ok(B, H, W, npred)) return -1;
  return 18L * npred * B * H * W + groups(B, H, W) * (npred + kMetrics);
}

extern "C" int ufr_raft_sequence_loss(const ufr_raft_sequence_loss_desc* d, ufr_stream_t stream) {
  UFR_REQUIRE(d, "raft sequence loss: null descriptor");
  UFR_REQUIRE(d->npred >= 1 && d->npred <= kMaxP, "raft sequence loss: %d predictions, 1 .. %d are served", d->npred, kMaxP);
  UFR_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0, "raft sequence loss: a 1/8 grid of %d x %d x %d: sizes must be positive", d->B, d->H,
              d->W);
  UFR_REQUIRE(d->B <= 65535 && d->H <= 65535, "raft sequence loss: B = %d, H = %d: at most 65535 each", d->B, d->H);
  UFR_REQUIRE(d->gt && d->valid && d->ws && d->out, "raft sequence loss: null pointer (gt, valid, ws or out)");
  for (int i = 0; i < d->npred; ++i)
    UFR_REQUIRE(d->flow[i] && d->mask[i] && d->grad_flow[i] && d->grad_mask[i],
                "raft sequence loss: null pointer (flow, mask, grad_flow or grad_mask of prediction %d)", i);
  const long need = ufr_raft_sequence_loss_workspace_doubles(d->B, d->H, d->W, d->npred);
  UFR_REQUIRE(d->ws_elems >= need, "raft sequence loss: the workspace holds %ld doubles, %ld are needed", d->ws_elems, need);
  const long plane = (long)d->H * d->W, rows = groups(d->B, d->H, d->W);
  const double total = (double)d->B * 2.0 * 64.0 * (double)plane;
  double* a_ws = d->ws;
  double* part = d->ws + 18L * d->npred * d->B * plane;
  GradFlows gf;
  Weights wt;
  for (int i = 0; i < kMaxP; ++i) {
    gf.g[i] = i < d->npred ? d->grad_flow[i] : nullptr;
    wt.w[i] = i < d->npred ? d->weight[i] : 0.0;
  }
  hipStream_t st = ufr::as_stream(stream);
  hipLaunchKernelGGL(raft_loss_main, dim3(ufr::ceil_div(d->W, RL_W), d->H, d->B), dim3(RL_NT), 0, st, *d, total, a_ws, part);
  int rc = ufr::launched("raft_loss_main");
  if (rc != UFR_OK) return rc;
  hipLaunchKernelGGL(raft_loss_gather, dim3(ufr::stream_grid(2L * d->B * plane, 256), d->npred), dim3(256), 0, st, gf, a_ws, d->B,
                     d->H, d->W);
  rc = ufr::launched("raft_loss_gather");
  if (rc != UFR_OK) return rc;
  hipLaunchKernelGGL(raft_loss_finalize, dim3(1), dim3(RL_NT), 0, st, wt, part, rows, d->npred, total, d->out);
  return ufr::launched("raft_loss_finalize");
}
