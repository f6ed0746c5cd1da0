// warp_norm.hip -- FlowNet2's two HBM-bound helpers for gfx950:
//   Resample2d  (backward warp by a flow field)   models/resample2d_package/resample2d_kernel.cu
//   ChannelNorm (per-pixel L2 norm over channels) models/channelnorm_package/channelnorm_kernel.cu
// Both are pure streaming kernels: one thread per output PIXEL (not per element), so the flow
// vector / bilinear weights are computed once and reused for all channels, and every access of a
// wave is a 256-byte coalesced row segment of one channel plane.
#include "ufr_common.h"

namespace {

using ufr::dev::clampi;

// resample2d_kernel.cu:15-72.  Quirks kept: clamp with the OUTPUT's dims (:45-48); the four
// products are formed in double and rounded to float one by one (:52-55); nearest = floor(x+.5).
__global__ void resample2d_fwd(const float* __restrict__ img, const float* __restrict__ flow,
                               float* __restrict__ out, int B, int C, int Hi, int Wi, int H, int W,
                               int ksize, int bilinear) {
  const long npix = (long)B * H * W;
  const size_t plane_o = (size_t)H * W, plane_i = (size_t)Hi * Wi;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < npix;
       idx += (long)gridDim.x * blockDim.x) {
    int x, y, b;
    if (npix < (1L << 31)) {                      // 32-bit index arithmetic (three 64-bit divisions per pixel cost more than the taps)
      const unsigned ui = (unsigned)idx, uw = (unsigned)W, uh = (unsigned)H, row = ui / uw;
      x = (int)(ui - row * uw); b = (int)(row / uh); y = (int)(row - (unsigned)b * uh);
    } else {
      x = (int)(idx % W); y = (int)((idx / W) % H); b = (int)(idx / plane_o);
    }
    const size_t pix = (size_t)y * W + x;
    const float dx = flow[((size_t)b * 2 + 0) * plane_o + pix];
    const float dy = flow[((size_t)b * 2 + 1) * plane_o + pix];
    const float xf = (float)x + dx, yf = (float)y + dy;
    if (bilinear) {
      const float alpha = xf - floorf(xf), beta = yf - floorf(yf);
      const int xL = clampi((int)floorf(xf), 0, W - 1), xR = clampi((int)floorf(xf) + 1, 0, W - 1);
      const int yT = clampi((int)floorf(yf), 0, H - 1), yB = clampi((int)floorf(yf) + 1, 0, H - 1);
      const double wTL = (1. - alpha) * (1. - beta), wTR = (double)alpha * (1. - beta);
      const double wBL = (1. - alpha) * (double)beta, wBR = (double)alpha * (double)beta;
      for (int c = 0; c < C; ++c) {
        const float* im = img + ((size_t)b * C + c) * plane_i;
        float val = 0.f;
        for (int fy = 0; fy < ksize; ++fy)
          for (int fx = 0; fx < ksize; ++fx) {
            val += (float)(wTL * im[(size_t)(yT + fy) * Wi + xL + fx]);
            val += (float)(wTR * im[(size_t)(yT + fy) * Wi + xR + fx]);
            val += (float)(wBL * im[(size_t)(yB + fy) * Wi + xL + fx]);
            val += (float)(wBR * im[(size_t)(yB + fy) * Wi + xR + fx]);
          }
        out[((size_t)b * C + c) * plane_o + pix] = val;
      }
    } else {
      const int xN = clampi((int)floor((double)xf + 0.5), 0, W - 1);
      const int yN = clampi((int)floor((double)yf + 0.5), 0, H - 1);
      for (int c = 0; c < C; ++c)
        out[((size_t)b * C + c) * plane_o + pix] = img[((size_t)b * C + c) * plane_i + (size_t)yN * Wi + xN];
    }
  }
}

// resample2d_kernel.cu:75-125 (scatter to the image; weights use int() truncation, :105-106)
// fused with :127-198 (gradient wrt the flow; clamps with the flow's dims; channel 0 uses
// gamma = 1-frac(y), channel 1 gamma = 1-frac(x)).  gimg must be zero on entry.
__global__ void resample2d_bwd(const float* __restrict__ img, const float* __restrict__ flow,
                               const float* __restrict__ gout, float* __restrict__ gimg,
                               float* __restrict__ gflow, int B, int C, int Hi, int Wi, int H,
                               int W, int ksize) {
  const long npix = (long)B * H * W;
  const size_t plane_o = (size_t)H * W, plane_i = (size_t)Hi * Wi;
  const int krad = (ksize - 1) / 2;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < npix;
       idx += (long)gridDim.x * blockDim.x) {
    int x, y, b;
    if (npix < (1L << 31)) {                      // 32-bit index arithmetic (three 64-bit divisions per pixel cost more than the taps)
      const unsigned ui = (unsigned)idx, uw = (unsigned)W, uh = (unsigned)H, row = ui / uw;
      x = (int)(ui - row * uw); b = (int)(row / uh); y = (int)(row - (unsigned)b * uh);
    } else {
      x = (int)(idx % W); y = (int)((idx / W) % H); b = (int)(idx / plane_o);
    }
    const size_t pix = (size_t)y * W + x;
    const float dx = flow[((size_t)b * 2 + 0) * plane_o + pix];
    const float dy = flow[((size_t)b * 2 + 1) * plane_o + pix];
    const float xf = (float)x + dx, yf = (float)y + dy;
    // ---- wrt image
    {
      const float alpha = xf - (float)(int)xf, beta = yf - (float)(int)yf;
      const int xL = clampi((int)floorf(xf), 0, Wi - 1), xR = clampi((int)floorf(xf) + 1, 0, Wi - 1);
      const int yT = clampi((int)floorf(yf), 0, Hi - 1), yB = clampi((int)floorf(yf) + 1, 0, Hi - 1);
      for (int c = 0; c < C; ++c) {
        const float g = gout[((size_t)b * C + c) * plane_o + pix];
        float* gi = gimg + ((size_t)b * C + c) * plane_i;
        for (int fy = 0; fy < ksize; ++fy)
          for (int fx = 0; fx < ksize; ++fx) {
            atomicAdd(&gi[(size_t)(yT + fy) * Wi + xL + fx], (1 - alpha) * (1 - beta) * g);
            atomicAdd(&gi[(size_t)(yT + fy) * Wi + xR + fx], (alpha) * (1 - beta) * g);
            atomicAdd(&gi[(size_t)(yB + fy) * Wi + xL + fx], (1 - alpha) * (beta)*g);
            atomicAdd(&gi[(size_t)(yB + fy) * Wi + xR + fx], (alpha) * (beta)*g);
          }
      }
    }
    // ---- wrt flow
    {
      const int xL = clampi((int)floorf(xf), 0, W - 1), xR = clampi((int)floorf(xf) + 1, 0, W - 1);
      const int yT = clampi((int)floorf(yf), 0, H - 1), yB = clampi((int)floorf(yf) + 1, 0, H - 1);
      const float gx = 1 - (yf - floorf(yf));  // channel 0 (:183)
      const float gy = 1 - (xf - floorf(xf));  // channel 1 (:170)
      float o0 = 0.f, o1 = 0.f;
      for (int i = 0; i <= 2 * krad; ++i)
        for (int j = 0; j <= 2 * krad; ++j)
          for (int ch = 0; ch < C; ++ch) {
            const float g = gout[((size_t)b * C + ch) * plane_o + pix];
            const float* im = img + ((size_t)b * C + ch) * plane_i;
            const float tl = im[(size_t)(yT + j) * Wi + xL + i], tr = im[(size_t)(yT + j) * Wi + xR + i];
            const float bl = im[(size_t)(yB + j) * Wi + xL + i], br = im[(size_t)(yB + j) * Wi + xR + i];
            o0 += (gx)*g * tr;
            o0 -= (gx)*g * tl;
            o0 += (1 - gx) * g * br;
            o0 -= (1 - gx) * g * bl;
            o1 += (gy)*g * bl;
            o1 -= (gy)*g * tl;
            o1 += (1 - gy) * g * br;
            o1 -= (1 - gy) * g * tr;
          }
      gflow[((size_t)b * 2 + 0) * plane_o + pix] = o0;
      gflow[((size_t)b * 2 + 1) * plane_o + pix] = o1;
    }
  }
}

// ---- LDS-staged forms (kernel_size 1, bilinear, image and flow of one size: FlowNet2's only use) -----------------------
// Workgroup = an 8 x 32 tile of output pixels.  The tile's source pixels lie in the bounding box of its (clamped) sampling
// corners; when that box fits the LDS budget (smooth flow: tile + |flow| spread) the box of every channel is fetched ONCE
// with coalesced row reads and the 4*C bilinear taps of every pixel come from LDS -- instead of 4*C scattered global reads
// per pixel.  The adjoint with respect to the image is PRIVATISED: the tile's 4*C contributions per pixel are accumulated
// in an LDS copy of the box (ds_add_f32) and flushed with one global atomic per touched cell (the boxes of neighbouring
// tiles overlap), instead of 4*C global float atomics per pixel (resample2d_kernel.cu:118-121's scheme).  A box that does
// not fit (wild flow) falls back to the direct form, tile by tile; the arithmetic is identical either way.
constexpr int RS_TH = 8, RS_TW = 32;
constexpr int RS_FWD_MAX_AREA = 3 * RS_TH * RS_TW;

struct RsBox { int x0, y0, bw, bh; };

__device__ __forceinline__ RsBox rs_tile_box(int xL, int xR, int yT, int yB, bool live, int* red) {
  // red: 4 ints in LDS, initialised by the caller pattern below
  int mnx = live ? xL : (1 << 30), mxx = live ? xR : -(1 << 30), mny = live ? yT : (1 << 30), mxy = live ? yB : -(1 << 30);
  for (int off = 32; off > 0; off >>= 1) {
    mnx = min(mnx, __shfl_xor(mnx, off, 64)); mxx = max(mxx, __shfl_xor(mxx, off, 64));
    mny = min(mny, __shfl_xor(mny, off, 64)); mxy = max(mxy, __shfl_xor(mxy, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&red[0], mnx); atomicMax(&red[1], mxx); atomicMin(&red[2], mny); atomicMax(&red[3], mxy);
  }
  __syncthreads();
  RsBox bx;
  bx.x0 = red[0]; bx.y0 = red[2]; bx.bw = red[1] - red[0] + 1; bx.bh = red[3] - red[2] + 1;
  return bx;
}

__global__ __launch_bounds__(256) void resample2d_fwd_lds(const float* __restrict__ img, const float* __restrict__ flow,
                                                          float* __restrict__ out, int B, int C, int H, int W, int lds_floats) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  __shared__ int red[4];
  const int tid = threadIdx.x;
  if (tid == 0) { red[0] = 1 << 30; red[1] = -(1 << 30); red[2] = 1 << 30; red[3] = -(1 << 30); }
  __syncthreads();
  const int tiles_x = (W + RS_TW - 1) / RS_TW, tiles_y = (H + RS_TH - 1) / RS_TH;
  const int b = blockIdx.x / (tiles_x * tiles_y), tr = blockIdx.x - b * tiles_x * tiles_y;
  const int x = (tr % tiles_x) * RS_TW + (tid & (RS_TW - 1)), y = (tr / tiles_x) * RS_TH + tid / RS_TW;
  const bool live = x < W && y < H;
  const size_t plane = (size_t)H * W, pix = (size_t)(live ? y : 0) * W + (live ? x : 0);
  const float dx = live ? flow[((size_t)b * 2 + 0) * plane + pix] : 0.f;
  const float dy = live ? flow[((size_t)b * 2 + 1) * plane + pix] : 0.f;
  const float xf = (float)x + dx, yf = (float)y + dy;
  const float alpha = xf - floorf(xf), beta = yf - floorf(yf);
  const int xL = clampi((int)floorf(xf), 0, W - 1), xR = clampi((int)floorf(xf) + 1, 0, W - 1);
  const int yT = clampi((int)floorf(yf), 0, H - 1), yB = clampi((int)floorf(yf) + 1, 0, H - 1);
  const double wTL = (1. - alpha) * (1. - beta), wTR = (double)alpha * (1. - beta);
  const double wBL = (1. - alpha) * (double)beta, wBR = (double)alpha * (double)beta;
  const RsBox bx = rs_tile_box(xL, xR, yT, yB, live, red);
  // uniform.  Staging pays only while the box is not much larger than the tile (smooth flow): a box of more than
  // RS_FWD_MAX_AREA cells costs more coalesced reads than the 4 taps per pixel it saves (measured: profiles/r2_hbm_ops*).
  const bool staged = (long)C * bx.bw * bx.bh <= lds_floats && bx.bw * bx.bh <= RS_FWD_MAX_AREA;
  if (staged) {
    const int area = bx.bw * bx.bh;
    for (int r = tid >> 6; r < C * bx.bh; r += 4) {                   // one wave per box row: coalesced, no per-cell division
      const int c = r / bx.bh, ry = r - c * bx.bh;
      const float* src = img + ((size_t)b * C + c) * plane + (size_t)(bx.y0 + ry) * W + bx.x0;
      for (int rx = tid & 63; rx < bx.bw; rx += 64) rs_lds[c * area + ry * bx.bw + rx] = src[rx];
    }
    __syncthreads();
    if (live) {
      const int oTL = (yT - bx.y0) * bx.bw + xL - bx.x0, oTR = (yT - bx.y0) * bx.bw + xR - bx.x0;
      const int oBL = (yB - bx.y0) * bx.bw + xL - bx.x0, oBR = (yB - bx.y0) * bx.bw + xR - bx.x0;
      for (int c = 0; c < C; ++c) {
        const float* im = rs_lds + c * area;
        float val = 0.f;
        val += (float)(wTL * im[oTL]);
        val += (float)(wTR * im[oTR]);
        val += (float)(wBL * im[oBL]);
        val += (float)(wBR * im[oBR]);
        out[((size_t)b * C + c) * plane + pix] = val;
      }
    }
  } else if (live) {
    for (int c = 0; c < C; ++c) {
      const float* im = img + ((size_t)b * C + c) * plane;
      float val = 0.f;
      val += (float)(wTL * im[(size_t)yT * W + xL]);
      val += (float)(wTR * im[(size_t)yT * W + xR]);
      val += (float)(wBL * im[(size_t)yB * W + xL]);
      val += (float)(wBR * im[(size_t)yB * W + xR]);
      out[((size_t)b * C + c) * plane + pix] = val;
    }
  }
}

__global__ __launch_bounds__(256) void resample2d_bwd_lds(const float* __restrict__ img, const float* __restrict__ flow,
                                                          const float* __restrict__ gout, float* __restrict__ gimg,
                                                          float* __restrict__ gflow, int B, int C, int H, int W, int lds_floats) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];      // [C*area] image box | [C*area] gradient box
  __shared__ int red[4];
  const int tid = threadIdx.x;
  if (tid == 0) { red[0] = 1 << 30; red[1] = -(1 << 30); red[2] = 1 << 30; red[3] = -(1 << 30); }
  __syncthreads();
  const int tiles_x = (W + RS_TW - 1) / RS_TW, tiles_y = (H + RS_TH - 1) / RS_TH;
  const int b = blockIdx.x / (tiles_x * tiles_y), tr = blockIdx.x - b * tiles_x * tiles_y;
  const int x = (tr % tiles_x) * RS_TW + (tid & (RS_TW - 1)), y = (tr / tiles_x) * RS_TH + tid / RS_TW;
  const bool live = x < W && y < H;
  const size_t plane = (size_t)H * W, pix = (size_t)(live ? y : 0) * W + (live ? x : 0);
  const float dx = live ? flow[((size_t)b * 2 + 0) * plane + pix] : 0.f;
  const float dy = live ? flow[((size_t)b * 2 + 1) * plane + pix] : 0.f;
  const float xf = (float)x + dx, yf = (float)y + dy;
  const int xL = clampi((int)floorf(xf), 0, W - 1), xR = clampi((int)floorf(xf) + 1, 0, W - 1);
  const int yT = clampi((int)floorf(yf), 0, H - 1), yB = clampi((int)floorf(yf) + 1, 0, H - 1);
  // image adjoint: weights with int() truncation (resample2d_kernel.cu:105-106); flow adjoint: floor()
  const float alpha = xf - (float)(int)xf, beta = yf - (float)(int)yf;
  const float gx = 1 - (yf - floorf(yf)), gy = 1 - (xf - floorf(xf));
  const RsBox bx = rs_tile_box(xL, xR, yT, yB, live, red);
  const int area = bx.bw * bx.bh;
  const bool staged = 2L * C * area <= lds_floats;                     // uniform
  float o0 = 0.f, o1 = 0.f;
  if (staged) {
    float* gbox = rs_lds + C * area;
    for (int r = tid >> 6; r < C * bx.bh; r += 4) {                   // one wave per box row
      const int c = r / bx.bh, ry = r - c * bx.bh;
      const float* src = img + ((size_t)b * C + c) * plane + (size_t)(bx.y0 + ry) * W + bx.x0;
      for (int rx = tid & 63; rx < bx.bw; rx += 64) {
        rs_lds[c * area + ry * bx.bw + rx] = src[rx];
        gbox[c * area + ry * bx.bw + rx] = 0.f;
      }
    }
    __syncthreads();
    if (live) {
      const int oTL = (yT - bx.y0) * bx.bw + xL - bx.x0, oTR = (yT - bx.y0) * bx.bw + xR - bx.x0;
      const int oBL = (yB - bx.y0) * bx.bw + xL - bx.x0, oBR = (yB - bx.y0) * bx.bw + xR - bx.x0;
      for (int c = 0; c < C; ++c) {
        const float g = gout[((size_t)b * C + c) * plane + pix];
        float* gi = gbox + c * area;
        atomicAdd(&gi[oTL], (1 - alpha) * (1 - beta) * g);
        atomicAdd(&gi[oTR], (alpha) * (1 - beta) * g);
        atomicAdd(&gi[oBL], (1 - alpha) * (beta)*g);
        atomicAdd(&gi[oBR], (alpha) * (beta)*g);
        const float* im = rs_lds + c * area;
        const float tl = im[oTL], trv = im[oTR], bl = im[oBL], br = im[oBR];
        o0 += (gx)*g * trv; o0 -= (gx)*g * tl; o0 += (1 - gx) * g * br; o0 -= (1 - gx) * g * bl;
        o1 += (gy)*g * bl;  o1 -= (gy)*g * tl; o1 += (1 - gy) * g * br; o1 -= (1 - gy) * g * trv;
      }
    }
    __syncthreads();
    for (int r = tid >> 6; r < C * bx.bh; r += 4) {
      const int c = r / bx.bh, ry = r - c * bx.bh;
      float* dst = gimg + ((size_t)b * C + c) * plane + (size_t)(bx.y0 + ry) * W + bx.x0;
      for (int rx = tid & 63; rx < bx.bw; rx += 64) {
        const float v = gbox[c * area + ry * bx.bw + rx];
        if (v != 0.f) atomicAdd(&dst[rx], v);
      }
    }
  } else if (live) {
    for (int c = 0; c < C; ++c) {
      const float g = gout[((size_t)b * C + c) * plane + pix];
      float* gi = gimg + ((size_t)b * C + c) * plane;
      atomicAdd(&gi[(size_t)yT * W + xL], (1 - alpha) * (1 - beta) * g);
      atomicAdd(&gi[(size_t)yT * W + xR], (alpha) * (1 - beta) * g);
      atomicAdd(&gi[(size_t)yB * W + xL], (1 - alpha) * (beta)*g);
      atomicAdd(&gi[(size_t)yB * W + xR], (alpha) * (beta)*g);
      const float* im = img + ((size_t)b * C + c) * plane;
      const float tl = im[(size_t)yT * W + xL], trv = im[(size_t)yT * W + xR];
      const float bl = im[(size_t)yB * W + xL], br = im[(size_t)yB * W + xR];
      o0 += (gx)*g * trv; o0 -= (gx)*g * tl; o0 += (1 - gx) * g * br; o0 -= (1 - gx) * g * bl;
      o1 += (gy)*g * bl;  o1 -= (gy)*g * tl; o1 += (1 - gy) * g * br; o1 -= (1 - gy) * g * trv;
    }
  }
  if (live) {
    gflow[((size_t)b * 2 + 0) * plane + pix] = o0;
    gflow[((size_t)b * 2 + 1) * plane + pix] = o1;
  }
}

// channelnorm_kernel.cu:18-60
__global__ void channelnorm_fwd(const float* __restrict__ in, float* __restrict__ out, int B, int C,
                                long HW) {
  const long npix = (long)B * HW;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < npix;
       idx += (long)gridDim.x * blockDim.x) {
    const long b = idx / HW, p = idx - b * HW;
    const float* src = in + (size_t)b * C * HW + p;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
      const float v = src[(size_t)c * HW];
      acc += v * v;   // two roundings, as the reference (no fma contraction: see Makefile flags)
    }
    out[idx] = sqrtf(acc);
  }
}

// channelnorm_kernel.cu:63-96: g * x / (out + 1e-9), the division carried out in double (:93)
__global__ void channelnorm_bwd(const float* __restrict__ in, const float* __restrict__ out,
                                const float* __restrict__ gout, float* __restrict__ gin, int B,
                                int C, long HW) {
  const long npix = (long)B * HW;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < npix;
       idx += (long)gridDim.x * blockDim.x) {
    const long b = idx / HW, p = idx - b * HW;
    const double den = (double)out[idx] + 1e-9;
    const float g = gout[idx];
    const size_t base = (size_t)b * C * HW + p;
    for (int c = 0; c < C; ++c) {
      const size_t e = base + (size_t)c * HW;
      gin[e] = (float)((double)(g * in[e]) / den);
    }
  }
}

constexpr int RS_LDS_BYTES = 48 * 1024;         // per workgroup: three workgroups per CU

// UFR_RESAMPLE_LDS: unset / 1 = LDS-privatised adjoint, direct forward (one pixel per thread: a four-pixel-per-thread
// form with float4 flow / output accesses measured 0.136 vs 0.071 ms -- fewer, wider threads lose the gathers' locality) (the measured optimum: profiles/r2_hbm_ops_*: the
// forward's 12 taps per pixel are already served by L1 / L2, staging the box costs more than it saves -- 0.112 vs 0.071 ms
// at 8 x 448x1024 with a smooth flow -- while the adjoint's atomics drop 3x: 1.56 -> 0.50 ms); 0 = both direct; 2 = both LDS.
int rs_lds_mode() {
  const char* e = getenv("UFR_RESAMPLE_LDS");      // read per call: the tests switch it
  return e ? (e[0] == '0' ? 0 : (e[0] == '2' ? 2 : 1)) : 1;
}

void rs_raise_lds() {
  (void)ufr::ensure_dynamic_lds(reinterpret_cast<const void*>(resample2d_fwd_lds), RS_LDS_BYTES);
  (void)ufr::ensure_dynamic_lds(reinterpret_cast<const void*>(resample2d_bwd_lds), RS_LDS_BYTES);
}

}  // namespace

extern "C" int ufr_resample2d_forward(const float* input1, const float* input2, float* output,
                                      int B, int C, int Hi, int Wi, int H, int W, int kernel_size,
                                      int bilinear, ufr_stream_t stream) {
  UFR_REQUIRE(input1 && input2 && output, "resample2d forward: null pointer argument");
  UFR_REQUIRE(B > 0 && C > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0 && kernel_size >= 1,
              "resample2d forward: bad shape");
  const long npix = (long)B * H * W;
  if (kernel_size == 1 && bilinear && Hi == H && Wi == W && rs_lds_mode() == 2) {   // LDS-staged form (opt-in: see rs_lds_mode)
    const int tiles = B * ufr::ceil_div(H, RS_TH) * ufr::ceil_div(W, RS_TW);
    rs_raise_lds();
    resample2d_fwd_lds<<<tiles, 256, RS_LDS_BYTES, ufr::as_stream(stream)>>>(input1, input2, output, B, C, H, W, RS_LDS_BYTES / 4);
    return ufr::launched("resample2d_fwd_lds");
  }
  // one pixel per thread, every pixel's gathers in flight at once (the grid-stride form with 2048 workgroups serialised
  // seven dependent flow -> gather chains per thread: measured slower)
  const unsigned blocks = (unsigned)((npix + 255) / 256);
  hipLaunchKernelGGL(resample2d_fwd, dim3(blocks), dim3(256), 0,
                     ufr::as_stream(stream), input1, input2, output, B, C, Hi, Wi, H, W,
                     kernel_size, bilinear);
  return ufr::launched("resample2d_fwd");
}

extern "C" int ufr_resample2d_backward(const float* input1, const float* input2,
                                       const float* grad_output, float* grad_input1,
                                       float* grad_input2, int B, int C, int Hi, int Wi, int H,
                                       int W, int kernel_size, int bilinear, ufr_stream_t stream) {
  (void)bilinear;  // ignored by the reference backward as well
  UFR_REQUIRE(input1 && input2 && grad_output && grad_input1 && grad_input2,
              "resample2d backward: null pointer argument");
  UFR_REQUIRE(B > 0 && C > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0 && kernel_size >= 1,
              "resample2d backward: bad shape");
  hipStream_t st = ufr::as_stream(stream);
  hipError_t e = hipMemsetAsync(grad_input1, 0, sizeof(float) * (size_t)B * C * Hi * Wi, st);
  if (e != hipSuccess) return ufr::fail(UFR_ELAUNCH, "resample2d backward: memset: %s", hipGetErrorString(e));
  const long npix = (long)B * H * W;
  if (kernel_size == 1 && Hi == H && Wi == W && rs_lds_mode() >= 1) {
    const int tiles = B * ufr::ceil_div(H, RS_TH) * ufr::ceil_div(W, RS_TW);
    rs_raise_lds();
    resample2d_bwd_lds<<<tiles, 256, RS_LDS_BYTES, st>>>(input1, input2, grad_output, grad_input1, grad_input2, B, C, H, W,
                                                         RS_LDS_BYTES / 4);
    return ufr::launched("resample2d_bwd_lds");
  }
  hipLaunchKernelGGL(resample2d_bwd, dim3(ufr::stream_grid(npix, 256)), dim3(256), 0, st, input1,
                     input2, grad_output, grad_input1, grad_input2, B, C, Hi, Wi, H, W, kernel_size);
  return ufr::launched("resample2d_bwd");
}

extern "C" int ufr_channelnorm_forward(const float* input1, float* output, int B, int C, int H,
                                       int W, int norm_deg, ufr_stream_t stream) {
  (void)norm_deg;  // channelnorm_kernel.cu:53-59 always computes the L2 norm
  UFR_REQUIRE(input1 && output, "channelnorm forward: null pointer argument");
  UFR_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "channelnorm forward: bad shape");
  const long npix = (long)B * H * W;
  hipLaunchKernelGGL(channelnorm_fwd, dim3(ufr::stream_grid(npix, 256)), dim3(256), 0,
                     ufr::as_stream(stream), input1, output, B, C, (long)H * W);
  return ufr::launched("channelnorm_fwd");
}

extern "C" int ufr_channelnorm_backward(const float* input1, const float* output,
                                        const float* grad_output, float* grad_input1, int B, int C,
                                        int H, int W, int norm_deg, ufr_stream_t stream) {
  (void)norm_deg;
  UFR_REQUIRE(input1 && output && grad_output && grad_input1, "channelnorm backward: null pointer argument");
  UFR_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "channelnorm backward: bad shape");
  const long npix = (long)B * H * W;
  hipLaunchKernelGGL(channelnorm_bwd, dim3(ufr::stream_grid(npix, 256)), dim3(256), 0,
                     ufr::as_stream(stream), input1, output, grad_output, grad_input1, B, C,
                     (long)H * W);
  return ufr::launched("channelnorm_bwd");
}
