// perturb_step.hip -- what MI-FGSM and input diversity add to the captured attack step (gfx950)
//   global_attacks/perturb_model.py:621-757 (__mifgsm): grad = mu * grad + (1 - mu) * g / sum|g|, step along sign(grad)
//   global_attacks/perturb_model.py:759-821 (__diverse_input): resize to (nh, nw) >= 90 %, zero-pad back, flow rescaled
// The reference runs these as ~20 elementwise torch operators per step with host RNG draws in between.  Here a step adds
//   ufr_diverse_forward   adv0, adv1, gt -> x0, x1, gt'  (+ the loss normaliser 1 / (sum valid' + 1e-8), :141-143)
//   ufr_diverse_backward  d loss / d x0, x1 -> d loss / d adv0, adv1   (a gather: no atomics)
//   ufr_abs_sums          sum |g0|, sum |g1|  (float64 partials, fixed order, float32 result on the device)
//   ufr_momentum_update   momentum + the update of universal.hip's per-sample branch, both frames
//   ufr_step_advance      the device-resident step index that selects the transform's row
// and the transform's parameters come from a device table drawn by the host before the first step, so a captured graph replays
// the whole attack without host work.  Plain stores only; every reduction order is a function of the shape.
#include <cstdint>

#include "ufr_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxPartials = 2048;         // workgroups of a launch: 8 per CU, the rest is a grid stride
constexpr long kPerGroup = 1024;           // elements per workgroup before the grid stops growing

using ufr::dev::clampf;
using ufr::dev::signf;

__host__ __device__ inline int groups_for(long n) {
  const long g = (n + kPerGroup - 1) / kPerGroup;
  return (int)(g < 1 ? 1 : g > kMaxPartials ? kMaxPartials : g);
}

// the workgroup's 256 values added by a fixed halving tree; the total is in lds[0] afterwards
__device__ inline void block_tree(double* lds) {
  __syncthreads();
  for (int half = kBlock / 2; half >= 1; half >>= 1) {
    if ((int)threadIdx.x < half) lds[threadIdx.x] += lds[threadIdx.x + half];
    __syncthreads();
  }
}

// ---- sum |g0|, sum |g1| --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void abs_sums_partial_kernel(const float* __restrict__ g0, const float* __restrict__ g1, long n,
                                                                  double* __restrict__ ws) {
  __shared__ double lds0[kBlock], lds1[kBlock];
  double a0 = 0.0, a1 = 0.0;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long)gridDim.x * kBlock) {
    a0 += (double)fabsf(g0[i]);
    a1 += (double)fabsf(g1[i]);
  }
  lds0[threadIdx.x] = a0;
  lds1[threadIdx.x] = a1;
  block_tree(lds0);
  block_tree(lds1);
  if (threadIdx.x == 0) {
    ws[2 * blockIdx.x] = lds0[0];
    ws[2 * blockIdx.x + 1] = lds1[0];
  }
}

// one wave: lane l adds partials l, l + 64, ... in ascending order, then the lanes by a fixed shuffle tree
__device__ inline double wave_sum(const double* __restrict__ p, int count, int stride) {
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += 64) s += p[(long)i * stride];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  return s;
}

__global__ __launch_bounds__(64) void abs_sums_finalize_kernel(const double* __restrict__ ws, int count, float* __restrict__ out) {
  const double s0 = wave_sum(ws, count, 2), s1 = wave_sum(ws + 1, count, 2);
  if (threadIdx.x == 0) {
    out[0] = (float)s0;
    out[1] = (float)s1;
  }
}

// ---- momentum + update ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void momentum_update_kernel(const float* __restrict__ img0, const float* __restrict__ img1,
                                                                 const float* __restrict__ g0, const float* __restrict__ g1,
                                                                 const float* __restrict__ sums, float* __restrict__ m0,
                                                                 float* __restrict__ m1, float* __restrict__ adv0,
                                                                 float* __restrict__ adv1, float* __restrict__ delta, long total,
                                                                 long CHW, float mu, float omm, float lr, float eps, float lo, float hi,
                                                                 int frames, float direction) {
  const float s0 = sums[0], s1 = sums[1];
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const long b = i / CHW, e = i - b * CHW;
    // mu * grad + (1 - mu) * g / sum|g|  (:673-678): product, product, quotient, sum, each rounded to float32
    const float n0 = __fadd_rn(__fmul_rn(mu, m0[i]), __fdiv_rn(__fmul_rn(omm, g0[i]), s0));
    const float n1 = __fadd_rn(__fmul_rn(mu, m1[i]), __fdiv_rn(__fmul_rn(omm, g1[i]), s1));
    m0[i] = n0;
    m1[i] = n1;
    const float d0 = (frames & 1) ? __fmul_rn(lr, signf(n0)) : 0.f;
    const float d1 = (frames & 2) ? __fmul_rn(lr, signf(n1)) : 0.f;
    const float a0 = clampf(__fadd_rn(adv0[i], direction * d0), lo, hi);
    const float a1 = clampf(__fadd_rn(adv1[i], direction * d1), lo, hi);
    const float i0 = img0[i], i1 = img1[i];
    const float z0 = clampf(__fsub_rn(a0, i0), -eps, eps), z1 = clampf(__fsub_rn(a1, i1), -eps, eps);
    adv0[i] = __fadd_rn(i0, z0);
    adv1[i] = __fadd_rn(i1, z1);
    delta[(b * 2 + 0) * CHW + e] = z0;            // [B,2,3,H,W]
    delta[(b * 2 + 1) * CHW + e] = z1;
  }
}

// ---- input diversity --------------------------------------------------------------------------------------------------------
struct Row {
  int apply, nh, nw, top, left;
};

// the step's row; a row that would leave the frame is treated as "do not apply" (the host check refuses it before the upload)
__device__ inline Row load_row(const int* __restrict__ table, int rows, const int* __restrict__ step, int H, int W) {
  Row r = {0, H, W, 0, 0};
  const int s = *step;
  if (s < 0 || s >= rows) return r;
  const int* t = table + (long)s * UFR_DIVERSE_COLS;
  const int ap = t[0], nh = t[1], nw = t[2], top = t[3], left = t[4];
  if (ap == 0 || nh < 1 || nh > H || nw < 1 || nw > W || top < 0 || left < 0 || top > H - nh || left > W - nw) return r;
  r.apply = 1; r.nh = nh; r.nw = nw; r.top = top; r.left = left;
  return r;
}

// torch's area_pixel_compute_source_index (align_corners False, not cubic) in float32: scale * (dst + 0.5) - 0.5, clamped at 0;
// i0 = the lower source index, ip = 1 when a second one exists, l1 = its weight
__device__ __forceinline__ void bilinear_source(float scale, int dst, int in_size, int& i0, int& ip, float& l1) {
  float s = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
  if (s < 0.f) s = 0.f;
  int i = (int)s;
  if (i > in_size - 1) i = in_size - 1;
  i0 = i;
  ip = (i < in_size - 1) ? 1 : 0;
  l1 = __fsub_rn(s, (float)i);
}

// torch's nearest_neighbor_compute_source_index: min(int(floor(dst * scale)), in_size - 1)
__device__ __forceinline__ int nearest_source(float scale, int dst, int in_size) {
  const int i = (int)floorf(__fmul_rn((float)dst, scale));
  return i < in_size - 1 ? i : in_size - 1;
}

__global__ __launch_bounds__(kBlock) void diverse_forward_kernel(const float* __restrict__ adv0, const float* __restrict__ adv1,
                                                                 const float* __restrict__ gt, float* __restrict__ x0,
                                                                 float* __restrict__ x1, float* __restrict__ gt_out, int B, int H, int W,
                                                                 int Cg, const int* __restrict__ table, int rows,
                                                                 const int* __restrict__ step, double* __restrict__ ws) {
  __shared__ double lds[kBlock];
  const Row r = load_row(table, rows, step, H, W);
  const long HW = (long)H * W, F = (long)B * 3 * HW, total = 2 * F + (long)B * Cg * HW;
  const float sh = __fdiv_rn((float)H, (float)r.nh), sw = __fdiv_rn((float)W, (float)r.nw);
  const float factor = (float)((double)r.nw / (double)W);              // float(n_width) / float(o_width), :815
  double valid = 0.0;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const bool frame = i < 2 * F;
    const long j = frame ? (i < F ? i : i - F) : i - 2 * F;            // element of its own tensor
    const float* __restrict__ src = frame ? (i < F ? adv0 : adv1) : gt;
    float* __restrict__ dst = frame ? (i < F ? x0 : x1) : gt_out;
    const long plane = j / HW, p = j - plane * HW;
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    float v;
    if (!r.apply) {
      v = src[j];
    } else {
      const int dy = y - r.top, dx = x - r.left;
      if (dy < 0 || dy >= r.nh || dx < 0 || dx >= r.nw) {
        v = 0.f;
      } else if (frame) {
        int h1, hp, w1, wp;
        float hl, wl;
        bilinear_source(sh, dy, H, h1, hp, hl);
        bilinear_source(sw, dx, W, w1, wp, wl);
        const float h0 = 1.f - hl, w0 = 1.f - wl;
        const float* __restrict__ q = src + plane * HW;
        const float a = q[(long)h1 * W + w1], b = q[(long)h1 * W + w1 + wp];
        const float c = q[(long)(h1 + hp) * W + w1], d = q[(long)(h1 + hp) * W + w1 + wp];
        v = h0 * (w0 * a + wl * b) + hl * (w0 * c + wl * d);
      } else {
        const int sy = nearest_source(sh, dy, H), sx = nearest_source(sw, dx, W);
        v = src[plane * HW + (long)sy * W + sx] * factor;
      }
    }
    dst[j] = v;
    if (!frame && Cg == 3 && plane % 3 == 2) valid += (double)v;
  }
  if (Cg == 3) {                          // uniform over the launch
    lds[threadIdx.x] = valid;
    block_tree(lds);
    if (threadIdx.x == 0) ws[blockIdx.x] = lds[0];
  }
}

__global__ __launch_bounds__(64) void diverse_scale_kernel(const double* __restrict__ ws, int count, float* __restrict__ scale_t) {
  const double s = wave_sum(ws, count, 1);
  if (threadIdx.x == 0) *scale_t = 1.0f / ((float)s + 1e-8f);           // loss.sum() / (valid.sum() + epsilon) in float32
}

// The adjoint of the frames' map.  Destination row dy reads source rows h1(dy) and h1(dy) + hp(dy) with weights 1 - l and l;
// h1 = floor(scale * (dy + 0.5) - 0.5) with scale >= 1, so the rows that reach source row sy lie within 1 of
// floor((sy + 0.5) / scale): the five rows within 2 are examined with the forward's own arithmetic (columns alike).
__device__ __forceinline__ void adjoint_weights(float scale, int s, int in_size, int out_size, int& d_lo, float (&w)[5]) {
  d_lo = (int)__fdiv_rn((float)s + 0.5f, scale) - 2;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int d = d_lo + k;
    float wk = 0.f;
    if (d >= 0 && d < out_size) {
      int i0, ip;
      float l1;
      bilinear_source(scale, d, in_size, i0, ip, l1);
      if (i0 == s) wk += 1.f - l1;
      if (i0 + ip == s) wk += l1;
    }
    w[k] = wk;
  }
}

__global__ __launch_bounds__(kBlock) void diverse_backward_kernel(const float* __restrict__ gx0, const float* __restrict__ gx1,
                                                                  float* __restrict__ g0, float* __restrict__ g1, int B, int H, int W,
                                                                  const int* __restrict__ table, int rows,
                                                                  const int* __restrict__ step) {
  const Row r = load_row(table, rows, step, H, W);
  const long HW = (long)H * W, F = (long)B * 3 * HW;
  const float sh = __fdiv_rn((float)H, (float)r.nh), sw = __fdiv_rn((float)W, (float)r.nw);
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < 2 * F; i += (long)gridDim.x * kBlock) {
    const long j = i < F ? i : i - F;
    const float* __restrict__ src = i < F ? gx0 : gx1;
    float* __restrict__ dst = i < F ? g0 : g1;
    if (!r.apply) {
      dst[j] = src[j];
      continue;
    }
    const long plane = j / HW, p = j - plane * HW;
    const int sy = (int)(p / W), sx = (int)(p - (long)sy * W);
    int y_lo, x_lo;
    float wy[5], wx[5];
    adjoint_weights(sh, sy, H, r.nh, y_lo, wy);
    adjoint_weights(sw, sx, W, r.nw, x_lo, wx);
    const float* __restrict__ q = src + plane * HW;
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky) {
      if (wy[ky] == 0.f) continue;                 // also every row outside [0, nh)
      const long row = (long)(y_lo + ky + r.top) * W + r.left;
      float line = 0.f;
#pragma unroll
      for (int kx = 0; kx < 5; ++kx)
        if (wx[kx] != 0.f) line += wx[kx] * q[row + x_lo + kx];
      acc += wy[ky] * line;
    }
    dst[j] = acc;
  }
}

__global__ void step_advance_kernel(int* __restrict__ step) { *step = *step + 1; }

bool shape_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && (long)B * 9 * H * W < (1L << 40); }

}  // namespace

extern "C" long ufr_abs_sums_workspace_doubles(long n) { return n < 1 ? -1 : 2L * groups_for(n); }

extern "C" int ufr_abs_sums(const float* g0, const float* g1, long n, double* ws, long ws_elems, float* out, ufr_stream_t stream) {
  UFR_REQUIRE(g0 && g1 && ws && out, "abs sums: null pointer argument");
  UFR_REQUIRE(n >= 1, "abs sums: %ld elements", n);
  const int groups = groups_for(n);
  UFR_REQUIRE(ws_elems >= 2L * groups, "abs sums: workspace of %ld doubles, %ld needed", ws_elems, 2L * groups);
  hipStream_t st = ufr::as_stream(stream);
  abs_sums_partial_kernel<<<groups, kBlock, 0, st>>>(g0, g1, n, ws);
  if (int rc = ufr::launched("abs_sums_partial_kernel")) return rc;
  abs_sums_finalize_kernel<<<1, 64, 0, st>>>(ws, groups, out);
  return ufr::launched("abs_sums_finalize_kernel");
}

extern "C" int ufr_momentum_update(const float* img0, const float* img1, const float* g0, const float* g1, const float* sums,
                                   float* m0, float* m1, float* adv0, float* adv1, float* delta, int B, int CHW, float mu,
                                   float one_minus_mu, float lr, float eps, float lo, float hi, int frames, int ascent,
                                   ufr_stream_t stream) {
  UFR_REQUIRE(img0 && img1 && g0 && g1 && sums && m0 && m1 && adv0 && adv1 && delta, "momentum update: null pointer argument");
  UFR_REQUIRE(B > 0 && CHW > 0 && frames >= 1 && frames <= 3, "momentum update: bad argument (B %d, CHW %d, frames %d)", B, CHW, frames);
  const long total = (long)B * CHW;
  momentum_update_kernel<<<ufr::stream_grid(total, kBlock), kBlock, 0, ufr::as_stream(stream)>>>(
      img0, img1, g0, g1, sums, m0, m1, adv0, adv1, delta, total, (long)CHW, mu, one_minus_mu, lr, eps, lo, hi, frames,
      ascent ? 1.0f : -1.0f);
  return ufr::launched("momentum_update_kernel");
}

extern "C" int ufr_diverse_table_check(const int* table_host, int rows, int H, int W) {
  UFR_REQUIRE(table_host != nullptr, "diverse table: null pointer argument");
  UFR_REQUIRE(rows >= 1 && H > 0 && W > 0, "diverse table: %d rows for frames of %d x %d", rows, H, W);
  for (int i = 0; i < rows; ++i) {
    const int* t = table_host + (long)i * UFR_DIVERSE_COLS;
    if (t[0] == 0) continue;
    const int nh = t[1], nw = t[2], top = t[3], left = t[4];
    UFR_REQUIRE(nh >= 1 && nh <= H && nw >= 1 && nw <= W, "diverse table: row %d resizes %d x %d frames to %d x %d (nh > H or nw > W is no down-scale)",
                i, H, W, nh, nw);
    UFR_REQUIRE(top >= 0 && left >= 0 && top <= H - nh && left <= W - nw,
                "diverse table: row %d places %d x %d at (%d, %d): top + nh > H or left + nw > W leaves the %d x %d frame", i, nh, nw,
                top, left, H, W);
  }
  return UFR_OK;
}

extern "C" long ufr_diverse_workspace_doubles(int B, int H, int W, int Cg) {
  if (!shape_ok(B, H, W) || (Cg != 2 && Cg != 3)) return -1;
  return Cg == 3 ? groups_for((long)B * (6 + Cg) * H * W) : 0;
}

extern "C" int ufr_diverse_forward(const float* adv0, const float* adv1, const float* gt, float* x0, float* x1, float* gt_out, int B,
                                   int H, int W, int Cg, const int* table, int rows, const int* step, float* scale_t, double* ws,
                                   long ws_elems, ufr_stream_t stream) {
  UFR_REQUIRE(adv0 && adv1 && gt && x0 && x1 && gt_out && table && step, "diverse forward: null pointer argument");
  UFR_REQUIRE(Cg == 2 || Cg == 3, "diverse forward: ground truth of %d channels (2, or 3 with a validity mask)", Cg);
  UFR_REQUIRE(shape_ok(B, H, W) && rows >= 1, "diverse forward: bad argument (B %d, H %d, W %d, rows %d)", B, H, W, rows);
  const int groups = groups_for((long)B * (6 + Cg) * H * W);
  if (Cg == 3) {
    UFR_REQUIRE(scale_t && ws, "diverse forward: null pointer argument (a validity mask needs scale_t and a workspace)");
    UFR_REQUIRE(ws_elems >= groups, "diverse forward: workspace of %ld doubles, %d needed", ws_elems, groups);
  }
  hipStream_t st = ufr::as_stream(stream);
  diverse_forward_kernel<<<groups, kBlock, 0, st>>>(adv0, adv1, gt, x0, x1, gt_out, B, H, W, Cg, table, rows, step, ws);
  if (int rc = ufr::launched("diverse_forward_kernel")) return rc;
  if (Cg == 3) {
    diverse_scale_kernel<<<1, 64, 0, st>>>(ws, groups, scale_t);
    return ufr::launched("diverse_scale_kernel");
  }
  return UFR_OK;
}

extern "C" int ufr_diverse_backward(const float* gx0, const float* gx1, float* g0, float* g1, int B, int H, int W, const int* table,
                                    int rows, const int* step, ufr_stream_t stream) {
  UFR_REQUIRE(gx0 && gx1 && g0 && g1 && table && step, "diverse backward: null pointer argument");
  UFR_REQUIRE(shape_ok(B, H, W) && rows >= 1, "diverse backward: bad argument (B %d, H %d, W %d, rows %d)", B, H, W, rows);
  UFR_REQUIRE(gx0 != g0 && gx1 != g1 && gx0 != g1 && gx1 != g0, "diverse backward: the gather cannot run in place");
  const long n = 2L * B * 3 * H * W;
  diverse_backward_kernel<<<ufr::stream_grid(n, kBlock), kBlock, 0, ufr::as_stream(stream)>>>(gx0, gx1, g0, g1, B, H, W, table, rows,
                                                                                             step);
  return ufr::launched("diverse_backward_kernel");
}

extern "C" int ufr_step_advance(int* step, ufr_stream_t stream) {
  UFR_REQUIRE(step != nullptr, "step advance: null pointer argument");
  step_advance_kernel<<<1, 1, 0, ufr::as_stream(stream)>>>(step);
  return ufr::launched("step_advance_kernel");
}
