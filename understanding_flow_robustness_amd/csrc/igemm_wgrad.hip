// igemm_wgrad.hip -- the WEIGHT gradient of the convolutions igemm.hip runs forward and backward-data:
//   dW[n][c][ky][kx] = sum over (b, y, x) of gy[b, n, y, x] * x[b, c, y*sy + ky*dy - py, x*sx + kx*dx - px]   (zero outside [0,Hi) x [0,Wi))
// (dy, dx = the dilation: data, as in igemm.hip -- PWC-Net's context network runs 2, 4, 8 and 16)
// from two operands already in the plane layout (bf16 [3][chunks][M][32], v = p0 + p1 + p2 exactly), float32-accurate on the bf16
// matrix cores: the six plane products of igemm.hip, in its order (smallest first), accumulated in float32 by
// `v_mfma_f32_32x32x16_bf16`.
//
// The reduction runs over PIXELS -- the strided dimension of the layout (a pixel's 32 channels are the contiguous run).  Per tap
// the GEMM is  dW_tap[n][c] = sum_m G[m][n] * X_tap[m][c]:  the A operand is gy TRANSPOSED, the B operand is x as it lies, and both
// fragments of the 32x32x16 form want, per lane, eight consecutive k (= pixels) of ONE channel.  So a K tile of 32 pixels of either
// operand is staged as it lies in HBM -- rows of [pixel][32 channels], 64 bytes each -- and read back with `ds_read_b64_tr_b16`
// (4 pixels x 16 channels per 16-lane group, delivered channel-major): lane l of the wave gets channel l & 31, pixels
// 8 (l >> 5) + 0..7 of a 16-pixel k step from two reads.  A 32-lane half reads 4 whole rows = 256 contiguous bytes: no bank
// conflict.  Tap rows outside the frame and the pixels behind a slice's end are ZEROS WRITTEN TO LDS; they are never read from
// memory (with a dilation as large as the grid whole taps lie outside: their workgroups stage zeros only and write exact zeros).  The transposed reads sit in workgroup-uniform control flow (EXEC all ones).
//
// Workgroup = 256 threads, one (n tile, c tile, tap, pixel slice): 64 NB output channels x 64 input channels, four waves 2 x 2,
// a wave owns NB 32 x 32 blocks.  The next K tile's 16-byte pieces are fetched into registers before the current tile's MFMAs.
// Split over pixels: slice s of `splitm` writes its raw sums to slab s of the caller's workspace and a second kernel adds the slabs in
// ASCENDING slice order (and then onto dw when `accumulate`): no float atomics, bit-reproducible -- igemm.hip's split-K convention.
// db[n] = sum of gy over all pixels rides along: per slice a fixed-order float32 sum, the slices added by the same second kernel.
//
// ConvTranspose2d(., ., 4, 2, 1) is the same call with the operands swapped (x = the gradient on the fine grid, gy = the layer's input
// on the coarse grid, stride 2, padding 1): the result is the [in][out][4][4] layout torch keeps.
#include "ufr_common.h"

namespace {

using ufr::dev::bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int KT = 32;                                       // pixels per staged K tile
constexpr int XCH = 2;                                       // x chunks per workgroup (64 input channels)
constexpr int MAX_TAPS = 49;
constexpr int MAX_SPLIT = 256;
__device__ constexpr int PROD_G[6] = {2, 0, 1, 1, 0, 0};     // (gy plane, x plane) of each product, smallest first (igemm.hip PROD_A / PROD_B)
__device__ constexpr int PROD_X[6] = {0, 2, 1, 0, 1, 0};

struct WArgs {
  const __bf16* x; long x_plane_stride; int x_chunk0, C, CCH;      // CCH = chunks that hold the C channels
  const __bf16* g; long g_plane_stride; int g_chunk0, N, NCH;
  int B, Hi, Wi, Ho, Wo, kw, sy, sx, py, px, dy, dx, taps;
  int M, per;                        // pixels of the gy grid; pixels per slice (a multiple of KT)
  int tiles_c;
  float* out; long slab;             // direct: dw (slab = 0); split: the workspace and the floats of one slab
  float* db_out;                     // direct: db; split: workspace + N*C*taps (same slab stride); NULL = no bias gradient
  int accumulate;                    // direct launches only (the reduce kernel applies it otherwise)
};

// Eight consecutive k (pixels krow0 .. krow0 + 7 for lanes 0-31, + 8 for lanes 32-63) of channel (lane & 31) of a [pixel][32] tile:
// the A / B fragment of v_mfma_f32_32x32x16_bf16.  Group g = lane >> 4 reads the 4 x 16 block at rows 8 (g >> 1) (+ 4 for the second
// read), columns 16 (g & 1); lane 4q + p of the group supplies the address of row q, columns 4p .. 4p + 3.
__device__ __forceinline__ bf16x8 tr_fragment(const __bf16* tile, int krow0, int lane) {
  typedef __attribute__((address_space(3))) s16x4* lds_v4;
  const int g = lane >> 4, i = lane & 15;
  const __bf16* p = tile + (krow0 + (g >> 1) * 8 + (i >> 2)) * 32 + (g & 1) * 16 + (i & 3) * 4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)p);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p + 4 * 32));
  return __builtin_shufflevector(__builtin_bit_cast(bf16x4, lo), __builtin_bit_cast(bf16x4, hi), 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int NB>
__global__ __launch_bounds__(256) void wgrad_kernel(const WArgs a) {
  constexpr int GCH = 2 * NB, TILES = GCH + XCH, UNITS = 3 * TILES, PER_T = UNITS / 2;
  static_assert(UNITS % 2 == 0, "two staging halves");
  __shared__ __attribute__((aligned(16))) __bf16 lds[UNITS][KT * 32];      // unit = tile * 3 + plane; tiles: GCH of gy, then XCH of x
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wc = wave & 1;
  const int tc = blockIdx.x % a.tiles_c, tn = blockIdx.x / a.tiles_c;
  const int tap = blockIdx.y, ky = tap / a.kw, kx = tap - ky * a.kw;
  const int slice = blockIdx.z;
  const long m0l = (long)slice * a.per;
  const int m0 = (int)(m0l < a.M ? m0l : a.M), m1 = (int)(m0l + a.per < a.M ? m0l + a.per : a.M);
  // staging role: 16-byte piece `piece` of pixel row `prow`, every second unit
  const int piece = tid & 3, prow = (tid >> 2) & 31, half = tid >> 7;
  const int hw = a.Ho * a.Wo;
  const long Min = (long)a.B * a.Hi * a.Wi;
  bf16x8 st[PER_T];
  auto fetch = [&](int mt) {
    const int m = mt + prow;
    const bool live = m < m1;
    long xpix = -1;
    if (live) {
      const int b = m / hw, r = m - b * hw, y = r / a.Wo, xx = r - y * a.Wo;
      const int yi = y * a.sy + ky * a.dy - a.py, xi = xx * a.sx + kx * a.dx - a.px;
      if ((unsigned)yi < (unsigned)a.Hi && (unsigned)xi < (unsigned)a.Wi) xpix = ((long)b * a.Hi + yi) * a.Wi + xi;
    }
#pragma unroll
    for (int i = 0; i < PER_T; ++i) {
      const int u = half + 2 * i, tile = u / 3, pl = u - tile * 3;
      bf16x8 v = {};
      if (tile < GCH) {
        const int ch = tn * GCH + tile;
        if (live && ch < a.NCH)
          v = *reinterpret_cast<const bf16x8*>(a.g + pl * a.g_plane_stride + ((long)(a.g_chunk0 + ch) * a.M + m) * 32 + piece * 8);
      } else {
        const int ch = tc * XCH + (tile - GCH);
        if (xpix >= 0 && ch < a.CCH)
          v = *reinterpret_cast<const bf16x8*>(a.x + pl * a.x_plane_stride + ((long)(a.x_chunk0 + ch) * Min + xpix) * 32 + piece * 8);
      }
      st[i] = v;
    }
  };

  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;

  if (m0 < m1) fetch(m0);
  for (int mt = m0; mt < m1; mt += KT) {
    __syncthreads();                                   // every wave has read the previous tile's fragments
#pragma unroll
    for (int i = 0; i < PER_T; ++i) *reinterpret_cast<bf16x8*>(&lds[half + 2 * i][prow * 32 + piece * 8]) = st[i];
    __syncthreads();
    if (mt + KT < m1) fetch(mt + KT);                  // in flight under this tile's MFMAs
#pragma unroll
    for (int kk = 0; kk < KT / 16; ++kk) {
      bf16x8 fx[3], fg[NB][3];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        fx[p] = tr_fragment(lds[(GCH + wc) * 3 + p], kk * 16, lane);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) fg[nb][p] = tr_fragment(lds[(wn * NB + nb) * 3 + p], kk * 16, lane);
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int t = 0; t < 6; ++t)
          acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fg[nb][PROD_G[t]], fx[PROD_X[t]], acc[nb], 0, 0, 0);
    }
  }

  // C/D of the 32x32 forms: col = lane & 31 (the B column: input channel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (output channel)
  const int c = tc * (XCH * 32) + wc * 32 + (lane & 31);
  float* out = a.out + (long)slice * a.slab;
  if (c < a.C) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = (tn * GCH + wn * NB + nb) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (n < a.N) {
          float* o = out + ((long)n * a.C + c) * a.taps + tap;
          *o = acc[nb][r] + (a.accumulate ? *o : 0.f);
        }
      }
  }
}

// db[n] (or its slab partial) = sum of gy[n] over the slice's pixels: thread (pixel lane q, channel) adds pixels m0 + q, m0 + q + 8, ...
// in ascending order, then the eight pixel lanes are added in ascending order -- one fixed order, float32.
__global__ __launch_bounds__(256) void wgrad_bias_kernel(const WArgs a) {
  __shared__ float part[8][32];
  const int ch = blockIdx.x, slice = blockIdx.y, cl = threadIdx.x & 31, q = threadIdx.x >> 5;
  const long m0l = (long)slice * a.per;
  const int m0 = (int)(m0l < a.M ? m0l : a.M), m1 = (int)(m0l + a.per < a.M ? m0l + a.per : a.M);
  const __bf16* g = a.g + ((long)(a.g_chunk0 + ch) * a.M) * 32 + cl;
  float s = 0.f;
  for (int m = m0 + q; m < m1; m += 8) {
    const __bf16* p = g + (long)m * 32;
    s += ((float)p[0] + (float)p[a.g_plane_stride]) + (float)p[2 * a.g_plane_stride];
  }
  part[q][cl] = s;
  __syncthreads();
  const int n = ch * 32 + cl;
  if (q == 0 && n < a.N) {
    float v = part[0][cl];
#pragma unroll
    for (int i = 1; i < 8; ++i) v += part[i][cl];
    float* o = a.db_out + (long)slice * a.slab + n;
    *o = v + (a.accumulate ? *o : 0.f);
  }
}

// out[i] = (accumulate ? out[i] : 0) + (slab 0 + slab 1 + ... in ascending order, from zero)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* ws, long slab, int S, float* out, long n, int accumulate) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = 0.f;
    for (int s = 0; s < S; ++s) v += ws[s * slab + i];
    out[i] = accumulate ? out[i] + v : v;
  }
}

}  // namespace

extern "C" int ufr_igemm_wgrad_dilated(const ufr_igemm_wgrad_desc* d, int dy, int dx, ufr_stream_t stream) {
  UFR_REQUIRE(d, "igemm wgrad: null descriptor");
  UFR_REQUIRE(d->x && d->gy && d->dw, "igemm wgrad: null pointer (x, gy and dw are required)");
  UFR_REQUIRE(d->products == 6, "igemm wgrad: products must be 6 (the float32-accurate form is the only one), got %d", d->products);
  UFR_REQUIRE(d->kh > 0 && d->kw > 0, "igemm wgrad: bad kernel size %d x %d", d->kh, d->kw);
  UFR_REQUIRE((long)d->kh * d->kw <= MAX_TAPS, "igemm wgrad: %d x %d = %ld taps, at most %d are served", d->kh, d->kw,
              (long)d->kh * d->kw, MAX_TAPS);
  UFR_REQUIRE(d->B > 0 && d->Hi > 0 && d->Wi > 0 && d->Ho > 0 && d->Wo > 0, "igemm wgrad: bad grid");
  UFR_REQUIRE(d->sy > 0 && d->sx > 0 && d->py >= 0 && d->px >= 0, "igemm wgrad: bad stride / padding");
  UFR_REQUIRE(dy >= 1 && dx >= 1, "igemm wgrad: bad dilation %d x %d (at least 1)", dy, dx);
  UFR_REQUIRE(d->C > 0 && d->N > 0 && d->in_chunk0 >= 0 && d->g_chunk0 >= 0, "igemm wgrad: bad channel counts");
  const long Min = (long)d->B * d->Hi * d->Wi, M = (long)d->B * d->Ho * d->Wo;
  UFR_REQUIRE(Min < (1L << 30) && M < (1L << 30), "igemm wgrad: too many pixels");
  // the taps must stay inside int arithmetic and the frame's neighbourhood: the last output cell's last tap
  UFR_REQUIRE((long)(d->Ho - 1) * d->sy + (long)(d->kh - 1) * dy + 1 < (1L << 30) && (long)(d->Wo - 1) * d->sx + (long)(d->kw - 1) * dx + 1 < (1L << 30),
              "igemm wgrad: bad geometry (the last tap of the last output cell, dilation %d x %d, leaves int arithmetic)", dy, dx);
  const int CCH = (d->C + 31) / 32, NCH = (d->N + 31) / 32;
  if (d->x_plane_stride <= 0 || (long)(d->in_chunk0 + CCH) * Min * 32 > d->x_plane_stride)
    return ufr::fail(UFR_EINVAL, "igemm wgrad: chunks [%d, %d) leave the x planes operand (%ld chunks per plane)", d->in_chunk0,
                     d->in_chunk0 + CCH, d->x_plane_stride > 0 ? d->x_plane_stride / (Min * 32) : 0L);
  if (d->gy_plane_stride <= 0 || (long)(d->g_chunk0 + NCH) * M * 32 > d->gy_plane_stride)
    return ufr::fail(UFR_EINVAL, "igemm wgrad: chunks [%d, %d) leave the gy planes operand (%ld chunks per plane)", d->g_chunk0,
                     d->g_chunk0 + NCH, d->gy_plane_stride > 0 ? d->gy_plane_stride / (M * 32) : 0L);
  UFR_REQUIRE(d->splitm >= 1 && d->splitm <= MAX_SPLIT, "igemm wgrad: splitm must be 1 .. %d", MAX_SPLIT);
  const int taps = d->kh * d->kw;
  const long dw_elems = (long)d->N * d->C * taps, slab = dw_elems + (d->db ? d->N : 0);
  if (d->splitm > 1) {
    UFR_REQUIRE(d->ws, "igemm wgrad: null pointer (a split over pixels needs the workspace)");
    UFR_REQUIRE(d->ws_elems >= (long)d->splitm * slab, "igemm wgrad: the workspace holds %ld floats, %d slabs of %ld are needed", d->ws_elems,
                d->splitm, slab);
  }

  WArgs a;
  a.x = static_cast<const __bf16*>(d->x); a.x_plane_stride = d->x_plane_stride; a.x_chunk0 = d->in_chunk0; a.C = d->C; a.CCH = CCH;
  a.g = static_cast<const __bf16*>(d->gy); a.g_plane_stride = d->gy_plane_stride; a.g_chunk0 = d->g_chunk0; a.N = d->N; a.NCH = NCH;
  a.B = d->B; a.Hi = d->Hi; a.Wi = d->Wi; a.Ho = d->Ho; a.Wo = d->Wo; a.kw = d->kw;
  a.sy = d->sy; a.sx = d->sx; a.py = d->py; a.px = d->px; a.dy = dy; a.dx = dx; a.taps = taps;
  a.M = (int)M;
  a.per = (int)(((M + d->splitm - 1) / d->splitm + KT - 1) / KT * KT);
  a.tiles_c = (CCH + XCH - 1) / XCH;
  const bool split = d->splitm > 1;
  a.out = split ? d->ws : d->dw;
  a.slab = split ? slab : 0;
  a.db_out = d->db ? (split ? d->ws + dw_elems : d->db) : nullptr;
  a.accumulate = (!split && d->accumulate) ? 1 : 0;
  hipStream_t st = ufr::as_stream(stream);
  // 128 output channels per workgroup where the layer has them, 64 otherwise (conv_redir, the two-channel flow layers)
  const int nb = NCH > 2 ? 2 : 1;
  const dim3 grid((unsigned)(((NCH + 2 * nb - 1) / (2 * nb)) * a.tiles_c), (unsigned)taps, (unsigned)d->splitm);
  if (nb == 2) wgrad_kernel<2><<<grid, 256, 0, st>>>(a);
  else wgrad_kernel<1><<<grid, 256, 0, st>>>(a);
  int rc = ufr::launched("igemm_wgrad_kernel");
  if (rc != UFR_OK) return rc;
  if (d->db) {
    wgrad_bias_kernel<<<dim3((unsigned)NCH, (unsigned)d->splitm), 256, 0, st>>>(a);
    rc = ufr::launched("igemm_wgrad_bias_kernel");
    if (rc != UFR_OK) return rc;
  }
  if (!split) return UFR_OK;
  wgrad_reduce_kernel<<<ufr::stream_grid(dw_elems, 256), 256, 0, st>>>(d->ws, slab, d->splitm, d->dw, dw_elems, d->accumulate ? 1 : 0);
  rc = ufr::launched("igemm_wgrad_reduce_kernel");
  if (rc != UFR_OK || !d->db) return rc;
  wgrad_reduce_kernel<<<ufr::stream_grid(d->N, 256), 256, 0, st>>>(d->ws + dw_elems, slab, d->splitm, d->db, d->N, d->accumulate ? 1 : 0);
  return ufr::launched("igemm_wgrad_reduce_kernel (bias)");
}

extern "C" int ufr_igemm_wgrad(const ufr_igemm_wgrad_desc* d, ufr_stream_t stream) { return ufr_igemm_wgrad_dilated(d, 1, 1, stream); }
