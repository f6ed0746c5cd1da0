// correlation_planes.hip -- FlowNetC's cost volume (21 x 21 displacements, stride 2: correlation_cuda_kernel.cu:21-83 with
// models/submodules.py:124-138 `correlate` = / C and FlowNetC.py:139 LeakyReLU fused) on the bf16 matrix cores, reading the
// engine's chunk-major planes of both feature maps and writing conv3_1's input planes directly (flownetc_engine.py: `in31`
// chunks 1..14) -- no NCHW cost volume, no conversion pass.
//
// For one output row y and displacement row dy (source row y2 = y + 2(dy - 10)) the volume is a BANDED GEMM:
//     R[x, x'] = sum_c f1[c, y, x] * f2[c, y2, x'],      needed for x' - x in {-20, -18, ..., 20}
// Only same-parity columns meet, so a workgroup owns (sample, row, column parity): with i = x / 2, j = x' / 2 the band is
// |j - i| <= 10.  A wave owns 16 columns i and keeps its f1 fragments (256 channels x 3 planes = 96 VGPRs) for its whole
// life; per dy the source row's same-parity columns are streamed through LDS by LDS-DMA, one 32-channel chunk per stage,
// double-buffered (XOR-swizzled images like csrc/igemm.hip), and each wave multiplies its 16 columns against 3 tiles of 16 source columns
// (j in [i0 - 16, i0 + 32): 44 % of the MFMA work lands inside the band), float32 = six bf16 products.
// out channel d = dy * 21 + (j - i + 10); value = leaky(R / C).
//
// Three entry points: the full volume (ufr_corr_forward_planes), and two incremental forms for the later iterations of an
// attack call, when the features changed inside the prefix window only -- every row and displacement of the 64 columns around
// the window (ufr_corr_forward_planes_window: the full kernel on one column block, kept as the reference), and only the
// entries whose cell or source cell lies in the window's rectangle (ufr_corr_forward_planes_changed, what the engine runs:
// `corr_fwd_planes_changed_kernel` below, a quarter of the window form's time).  All three write the same bits.
#include "ufr_common.h"

namespace {

using ufr::dev::bf16x8;
using ufr::dev::f32x4;
using ufr::dev::glds16;
using ufr::dev::split3;

__device__ constexpr int PROD_A[6] = {2, 0, 1, 1, 0, 0};
__device__ constexpr int PROD_B[6] = {0, 2, 1, 0, 1, 0};
__device__ __attribute__((aligned(64))) unsigned corr_zero_page[16];

constexpr int P = 21, R = 10, KCH = 8;           // 21 displacements per axis, reach 10 same-parity columns, 8 chunks of 32 channels
constexpr int OT = 24;                            // per-wave output tile: 16 columns x 21 displacements, row stride 24 floats

// f1, f2: planes [3][KCH][M][32] (M = B*H*W); out: planes [3][out_chunks][M][32], channels written at chunk out_chunk0 + d / 32.
// grid = (column blocks, 2 parities, B*H); block = NW waves; ONE workgroup per CU is resident (5 waves x 165 VGPRs), so all
// overlap is built into the workgroup:
//  * a STAGE = one 32-channel chunk of one source row (3 planes x NJ columns x 64 B) fetched by LDS-DMA into one of THREE
//    buffers, two stages ahead of its use; the wave that issued a stage's DMA retires it with a COUNTED s_waitcnt vmcnt(n)
//    (n = its DMA instructions of the one younger stage) before a raw s_barrier, and the buffer is read in the next phase
//    (a __syncthreads() would drain every DMA in flight: cdna_hip_programming.md, "Pipelining across barriers");
//  * the nine B fragments of a stage are read in one batch, then 18 MFMAs;
//  * a displacement row's 16 x 21 results per wave go through a wave-private LDS tile and leave as dense 2-byte stores
//    (18 instructions instead of 36 quarter-full ones), BEFORE the stage's DMA is issued so the counted wait stays exact.
// Workgroup -> (row, parity, column block).  The hardware deals consecutive workgroups round-robin to the 8 XCDs, each with
// its own 4 MB L2; a row of f2 is read by the 2 x 21 workgroups of the rows around it, so neighbouring rows must land on the
// SAME XCD: XCD k takes the k-th eighth of the (row, parity, block) list (a bijection when 8 divides it).
// Displacement rows are independent, so every workgroup walks them in a ROTATED order chosen so that all rows y of one parity
// read the SAME source row at the same step (row y + 2 (dy - 10) with dy = (t - y / 2) mod 21 is 2 t - 20 or 2 t + 22 for
// every y): the workgroups resident on an XCD share each fetched row through its L2.
// (The single-wave-per-tile form of this kernel -- one wave keeps all 8 chunks' f1 fragments, 96 VGPRs, 8 barriers per
// displacement row -- measured 0.356 ms against 0.325 and was removed in round 3.)
// ---- the reduction is split over TWO waves per tile ---------------------------------------------------------------------
// 2 NW waves: wave (tile tw, half kh) keeps the f1 fragments of chunks 4 kh .. 4 kh + 3 (48 VGPRs instead of 96) and a
// stage carries one chunk of EACH half, so a displacement row takes 4 barriers instead of 8 with the same 18 MFMAs per
// wave and stage; the upper half's accumulators cross to the lower half's wave through LDS once per row.  With one
// workgroup per CU this doubles the waves that share its issue slots (3,3,2,2 per SIMD instead of 2,1,1,1): 0.356 -> 0.325 ms
// at 8 pairs.  (Five buffers / four stages in flight on the single-wave form measured SLOWER, 0.417 ms: the kernel is bound
// by instruction issue and LDS traffic per stage, not by bytes in flight.)
template <int NW>
constexpr int corr_planes_k2_lds_bytes() { return 3 * 2 * 3 * (16 * NW + 32) * 32 * 2 + NW * 16 * OT * 4 + NW * 64 * 12 * 4; }

template <int NW>
__global__ __launch_bounds__(128 * NW) void corr_fwd_planes_k2_kernel(const __bf16* __restrict__ f1, const __bf16* __restrict__ f2,
                                                                      long in_plane_stride, __bf16* __restrict__ out,
                                                                      long out_plane_stride, int out_chunk0, int B, int H, int W,
                                                                      float scale, float slope, const int* __restrict__ win,
                                                                      int win_div) {
  // win != nullptr: only the 16 NW same-parity columns starting 20 cells left of the sample's window (win[b*8+1] / win_div)
  // are recomputed -- the incremental forward of the attack: between iterations of a call the features change only inside
  // the prefix window, so the volume changes only within the correlation's reach of it; grid.x = 1 then.
  constexpr int NJ = 16 * NW + 32, NRB = NJ / 16;
  constexpr int PLANE = NJ * 32, HBUF = 3 * PLANE, BUF = 2 * HBUF;        // elements: plane, one half's chunk, a stage
  constexpr int KH = KCH / 2;                                             // chunks per half
  extern __shared__ __attribute__((aligned(16))) unsigned char corr_lds[];
  __bf16* lds = reinterpret_cast<__bf16*>(corr_lds);                     // [3 buffers][2 halves][3 planes][NJ * 32]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kh = wave >= NW ? 1 : 0, tw = wave - kh * NW;
  float* otile = reinterpret_cast<float*>(corr_lds + 3 * BUF * 2) + tw * 16 * OT;
  float* part = reinterpret_cast<float*>(corr_lds + 3 * BUF * 2 + NW * 16 * OT * 4) + (tw * 64 + lane) * 12;
  const int nblk = gridDim.x * gridDim.y * gridDim.z;                    // XCD-contiguous rows: see the notes above
  int item = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  if ((nblk & 7) == 0) item = (item & 7) * (nblk >> 3) + (item >> 3);
  const int bx = item % gridDim.x, par = (item / gridDim.x) % gridDim.y, by = item / (gridDim.x * gridDim.y);
  const int b = by / H, y = by - b * H;
  int i0 = bx * 16 * NW;
  if (win) i0 = min(max((win[b * 8 + 1] / win_div - 2 * R) >> 1, 0), max((W + 1) / 2 - 16 * NW, 0));
  const long M = (long)B * H * W;
  const long rowbase = ((long)b * H + y) * W;
  const int ai = i0 + 16 * tw + (lane & 15), ax = 2 * ai + par;
  const bool a_ok = ax < W;
  const __bf16* zero = reinterpret_cast<const __bf16*>(corr_zero_page);
  bf16x8 fa[KH][3];
#pragma unroll
  for (int i = 0; i < KH; ++i)
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const __bf16* src = a_ok ? f1 + p * in_plane_stride + ((long)(kh * KH + i) * M + rowbase + ax) * 32 + (lane >> 4) * 8 : zero;
      fa[i][p] = *reinterpret_cast<const bf16x8*>(src);
    }
  // staging plan: 2 NRB (half, row block) items per plane over 2 NW waves: item = wave + it * 2 NW
  const int srow_in = lane >> 2, spiece = lane & 3;
  int voff[2], sdst[2], shalf[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int itm = wave + it * 2 * NW, h = itm >= NRB ? 1 : 0, rb = itm - h * NRB, r = rb * 16 + srow_in;
    const int j = i0 - 16 + r, xs = 2 * j + par;
    voff[it] = (itm < 2 * NRB && j >= 0 && xs < W) ? xs * 32 + ((spiece ^ ((r >> 1) & 3)) << 3) : -1;
    sdst[it] = h * HBUF + rb * 16 * 32;
    shalf[it] = h;
  }
  const bool two = wave + 2 * NW < 2 * NRB;      // uniform: 6 (else 3) DMA instructions per stage
  const int frow = lane & 15;
  const int foff = frow * 32 + (((lane >> 4) ^ ((frow >> 1) & 3)) << 3);
  auto stage = [&](int dy, int sl, int buf) {    // chunks sl and KH + sl of source row y + 2 (dy - R) -> buffer `buf`
    const long rowoff = ((long)b * H + (y + 2 * (dy - R))) * W;
    __bf16* dst = lds + buf * BUF;
    {
      const __bf16* sbase = f2 + ((long)(shalf[0] * KH + sl) * M + rowoff) * 32;
#pragma unroll
      for (int p = 0; p < 3; ++p) glds16(voff[0] >= 0 ? sbase + p * in_plane_stride + voff[0] : zero, dst + sdst[0] + p * PLANE);
    }
    if (two) {
      const __bf16* sbase = f2 + ((long)(shalf[1] * KH + sl) * M + rowoff) * 32;
#pragma unroll
      for (int p = 0; p < 3; ++p) glds16(voff[1] >= 0 ? sbase + p * in_plane_stride + voff[1] : zero, dst + sdst[1] + p * PLANE);
    }
  };
  const int rot = (P - (y >> 1) % P) % P;        // rotated displacement order: see the notes above
  auto dy_at = [&](int t) { const int d = t + rot; return d >= P ? d - P : d; };
  auto row_ok = [&](int dy) { const int y2 = y + 2 * (dy - R); return y2 >= 0 && y2 < H; };
  auto next_valid = [&](int t) { do { ++t; } while (t < P && !row_ok(dy_at(t))); return t; };
  auto write_row = [&](int d_row, const f32x4 (&acc)[3], bool zeros) {
    if (!zeros) {
#pragma unroll
      for (int tt = 0; tt < 3; ++tt)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int il = (lane >> 4) * 4 + rg;
          const int dx = 16 * tt - 16 + (lane & 15) - il + R;
          if (dx >= 0 && dx < P) otile[il * OT + dx] = acc[tt][rg];
        }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const int e = lane + 64 * q;
      const int il = e / P, dx = e - il * P;
      const int x = 2 * (i0 + 16 * tw + il) + par;
      if (e < 16 * P && x < W) {
        float v = zeros ? 0.f : otile[il * OT + dx] * scale;
        v = v > 0.f ? v : v * slope;
        __bf16 p0, p1, p2;
        split3(v, p0, p1, p2);
        const int d = d_row * P + dx;
        __bf16* o = out + ((long)(out_chunk0 + (d >> 5)) * M + rowbase + x) * 32 + (d & 31);
        o[0] = p0;
        o[out_plane_stride] = p1;
        o[2 * out_plane_stride] = p2;
      }
    }
  };
  const f32x4 zacc[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  if (kh == 0)
    for (int d0 = 0; d0 < P; ++d0)
      if (!row_ok(d0)) write_row(d0, zacc, true);
  int t = next_valid(-1);
  if (t >= P) return;
  int cur = 0;
  stage(dy_at(t), 0, 0);
  stage(dy_at(t), 1, 1);
  if (two) asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  while (t < P) {
    const int dy = dy_at(t), tn = next_valid(t);
    f32x4 acc[3];
#pragma unroll
    for (int tt = 0; tt < 3; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sl = 0; sl < KH; ++sl) {            // unrolled: fa[] indexed statically
      const bool ahead = sl + 2 < KH || tn < P;  // the stage two ahead: (dy, sl + 2) or (next valid row, sl + 2 - KH)
      const int nxt = cur == 0 ? 2 : cur - 1;
      if (ahead) stage(sl + 2 < KH ? dy : dy_at(tn), (sl + 2) & (KH - 1), nxt);
      bf16x8 fb[3][3];
      const __bf16* bsrc = lds + cur * BUF + kh * HBUF + tw * 16 * 32 + foff;
#pragma unroll
      for (int tt = 0; tt < 3; ++tt)
#pragma unroll
        for (int p = 0; p < 3; ++p) fb[tt][p] = *reinterpret_cast<const bf16x8*>(bsrc + p * PLANE + tt * 16 * 32);
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int tt = 0; tt < 3; ++tt)
          acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[sl][PROD_A[q]], fb[tt][PROD_B[q]], acc[tt], 0, 0, 0);
      if (sl == KH - 1 && kh == 1) {              // upper half: hand the partial sums to the tile's lower-half wave
#pragma unroll
        for (int tt = 0; tt < 3; ++tt) *reinterpret_cast<f32x4*>(part + 4 * tt) = acc[tt];
      }
      if (ahead) {
        if (two) asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      cur = cur == 2 ? 0 : cur + 1;
      if (sl == KH - 1 && kh == 0) {              // lower half: add, then the row leaves (its stores precede the next DMA issue)
#pragma unroll
        for (int tt = 0; tt < 3; ++tt) {
          const f32x4 o = *reinterpret_cast<const f32x4*>(part + 4 * tt);
          acc[tt][0] += o[0]; acc[tt][1] += o[1]; acc[tt][2] += o[2]; acc[tt][3] += o[3];
        }
        write_row(dy, acc, false);
      }
    }
    t = tn;
  }
}

template <int NW>
int launch_corr_planes(const __bf16* a, const __bf16* b, long in_plane_stride, __bf16* o, long out_plane_stride, int out_chunk0,
                       int B, int H, int W, int ni, float scale, float slope, hipStream_t st, const int* win = nullptr,
                       int win_div = 1) {
  {                                              // above the default dynamic-LDS limit
    hipError_t e = ufr::ensure_dynamic_lds(reinterpret_cast<const void*>(corr_fwd_planes_k2_kernel<NW>), corr_planes_k2_lds_bytes<NW>());
    if (e != hipSuccess) return ufr::fail(UFR_ELAUNCH, "correlation (planes): %s", hipGetErrorString(e));
  }
  corr_fwd_planes_k2_kernel<NW><<<dim3(win ? 1 : ufr::ceil_div(ni, 16 * NW), 2, B * H), 128 * NW, corr_planes_k2_lds_bytes<NW>(), st>>>(
      a, b, in_plane_stride, o, out_plane_stride, out_chunk0, B, H, W, scale, slope, win, win_div);
  return UFR_OK;
}

// ---- the changed entries only ------------------------------------------------------------------------------------------
// Between the iterations of a call the features change only inside a rectangle of cells (the prefix window without its
// inexact rim: plane_layout.hip `window_features_kernel`), so out[d = (dy, dx), y, x] can change only where
//   (A) (y, x) lies in the rectangle, or (B) its source cell (y2, x2) = (y + 2 (dy - 10), x + 2 (dx - 10)) does.
// Per column parity the rectangle holds at most 12 columns, one 16-column tile S; everything they meet lies in the 32
// same-parity columns from 10 left of them, two tiles D.  A wave owns one pair of rows, for both column parities:
//   (A) row y of the rectangle:  S of f1's row y  against D of f2's row y2 -> the 21 dx of the rectangle's columns;
//   (B) row y2 of the rectangle: D of f1's row y  against S of f2's row y2 -> the dx whose source column is in the rectangle
//       (every y, the rectangle's rows too: their columns outside the rectangle are case B's alone; where both cases write
//       an entry they write the same bits).
// 2 of the window form's 6 tile products per (row, dy, parity), on 2 x (rows of the rectangle) instead of all H rows.
// The fragments are 16-byte plane reads straight into registers (`load_fragment`): nothing is reused inside a wave, so nothing
// is staged.  A cell's 32 channels are 64 B, so the same-parity columns of a fragment each sit in half a 128-byte line: a
// wave reads BOTH parities back to back and uses every line it fetches, and the four waves of a workgroup take four rows of
// the rectangle against ONE row of the other map (the D tiles, 2/3 of the lines).  Measured at 8 pairs of 48 x 160 cells, 16 x 16
// windows, beside the window form's 183 us: 46 us (kernel trace; 53 between two events).  One parity per wave and the 21 dy
// of one row per workgroup: 82 us between events; either form with the loads in the fragment's own lane order: 87 - 93 us;
// loads a stage ahead of the MFMAs, 3 or 4 waves per SIMD, stores of all 16 x 21 slots or only of the entries there are:
// no difference.
// An entry's arithmetic is the full kernel's: chunks 0-3 into one accumulator and 4-7 into another, six products per chunk in
// PROD order with f1 as A and f2 as B, lo + hi, x scale, LeakyReLU, split3 -- an MFMA result depends on its A row, its B column
// and its accumulator only, so the bits are those of corr_fwd_planes_k2_kernel whatever the tiles are made of.
constexpr int CH_WAVES = 4;                       // waves per workgroup = rows of the rectangle that share a row of the other map
constexpr int CH_MAX_CELLS = 23;                  // window width: 12 same-parity columns + 2 x 10 reach = 32

// 16 bytes per lane in load order (above) -> the MFMA fragment: lane (row, k group) takes the 16 bytes of lane 4 row + k group
__device__ __forceinline__ bf16x8 load_fragment(const __bf16* src, int perm) {
  typedef __attribute__((ext_vector_type(4))) int i32x4;
  i32x4 v = *reinterpret_cast<const i32x4*>(src);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = __builtin_amdgcn_ds_bpermute(perm, v[k]);
  return __builtin_bit_cast(bf16x8, v);
}

// rowS / rowD: pixel index of the first cell of the rectangle's row / of the other map's row; row1: of f1's row (the output's)
template <bool CASE_B>
__device__ __forceinline__ void corr_changed_rows(const __bf16* __restrict__ f1, const __bf16* __restrict__ f2, long in_plane_stride,
                                                  __bf16* __restrict__ out, long out_plane_stride, int out_chunk0, long M, int W,
                                                  float scale, float slope, long rowS, long rowD, long row1, int rx0, int rx1, int dy,
                                                  float* otile, int lane) {
  const __bf16* zero = reinterpret_cast<const __bf16*>(corr_zero_page);
  const int fr = lane & 15, g = lane >> 4;        // the lane's place in a fragment: tile row (a column of the map), k group
  // a lane LOADS piece lane & 3 of column lane >> 2, so that four neighbouring lanes read one cell's 64 bytes (in the
  // fragment's own order the 16 lanes of a group each read from another line: 87 us instead of 53), and the fragment is
  // put in order by a lane permutation
  const int lc = lane >> 2, perm = ((fr << 2) | g) << 2;
  const __bf16* baseS = (CASE_B ? f2 : f1) + rowS * 32 + (lane & 3) * 8;
  const __bf16* baseD = (CASE_B ? f1 : f2) + rowD * 32 + (lane & 3) * 8;
  int i_lo[2], n[2];                              // per parity: the rectangle's columns are 2 i + par, i in [i_lo, i_lo + n)
  bool s_ok[2], d_ok[2][2];
  const __bf16 *sp[2], *dp[2][2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    i_lo[par] = (rx0 - par + 1) >> 1;
    n[par] = ((rx1 - par + 1) >> 1) - i_lo[par];
    s_ok[par] = lc < n[par];
    sp[par] = baseS + (long)(2 * (i_lo[par] + lc) + par) * 32;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int u = i_lo[par] - R + 16 * t + lc, xu = 2 * u + par;
      d_ok[par][t] = u >= 0 && xu < W;
      dp[par][t] = baseD + (long)xu * 32;
    }
  }
  f32x4 acc[2][2][2];                             // [half of the reduction][parity][D tile]
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int par = 0; par < 2; ++par)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[h][par][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < KCH; ++c) {
    const long off = (long)c * M * 32;
    bf16x8 fs[2][3], fd[2][2][3];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int par = 0; par < 2; ++par)           // the two parities of a line, one after the other
        fs[par][p] = load_fragment(s_ok[par] ? sp[par] + p * in_plane_stride + off : zero, perm);
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int par = 0; par < 2; ++par)
          fd[par][t][p] = load_fragment(d_ok[par][t] ? dp[par][t] + p * in_plane_stride + off : zero, perm);
#pragma unroll
    for (int par = 0; par < 2; ++par)
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          f32x4& a = acc[c / (KCH / 2)][par][t];
          a = CASE_B ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd[par][t][PROD_A[q]], fs[par][PROD_B[q]], a, 0, 0, 0)
                     : __builtin_amdgcn_mfma_f32_16x16x32_bf16(fs[par][PROD_A[q]], fd[par][t][PROD_B[q]], a, 0, 0, 0);
        }
  }
  // through the wave's LDS tile [f1 column][dx], so that the 2-byte stores of a column's displacements are dense
  constexpr int ROWS = 32;                        // case B: f1 columns of the two D tiles
#pragma unroll
  for (int par = 0; par < 2; ++par) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const float v = acc[0][par][t][rg] + acc[1][par][t][rg];
        const int m = g * 4 + rg;                 // the result's A row, fr its B column
        const int il = CASE_B ? 16 * t + m : m;
        const int dx = CASE_B ? fr - il + 2 * R : 16 * t + fr - m;
        if (dx >= 0 && dx < P && (!CASE_B || fr < n[par])) otile[il * OT + dx] = v;
      }
    // only the entries there are: (column of the rectangle, dx) in case A, (f1 column, source column in the rectangle) in case B
    const int np = n[par], cnt = (CASE_B ? ROWS : P) * np;
    for (int e = lane; e < cnt; e += 64) {
      const int il = CASE_B ? e / np : e / P;
      const int dx = CASE_B ? e - il * np - il + 2 * R : e - il * P;
      const int i = CASE_B ? i_lo[par] - R + il : i_lo[par] + il, x = 2 * i + par;
      if (!CASE_B || (dx >= 0 && dx < P && i >= 0 && x < W)) {
        float v = otile[il * OT + dx] * scale;
        v = v > 0.f ? v : v * slope;
        __bf16 p0, p1, p2;
        split3(v, p0, p1, p2);
        const int d = dy * P + dx;
        __bf16* o = out + ((long)(out_chunk0 + (d >> 5)) * M + row1 + x) * 32 + (d & 31);
        o[0] = p0;
        o[out_plane_stride] = p1;
        o[2 * out_plane_stride] = p2;
      }
    }
  }
}

// grid = B x 2 cases x H rows of the other map x groups of CH_WAVES same-parity rows of the window: sized for the largest
// rectangle (a window in a frame corner), so a captured launch serves every placement; a wave whose row is not in its sample's
// rectangle, or not within the reach of the other map's row, leaves at once.
__global__ __launch_bounds__(64 * CH_WAVES, 3) void corr_fwd_planes_changed_kernel(
    const __bf16* __restrict__ f1, const __bf16* __restrict__ f2, long in_plane_stride, __bf16* __restrict__ out, long out_plane_stride,
    int out_chunk0, int B, int H, int W, float scale, float slope, const int* __restrict__ win, int level_stride, int wh, int ww,
    int margin) {
  __shared__ float tiles[CH_WAVES][32 * OT];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int groups = ((wh + 1) / 2 + CH_WAVES - 1) / CH_WAVES;
  int item = blockIdx.x;
  const int k = item % groups; item /= groups;
  const int yd = item % H; item /= H;
  const int case_b = item & 1, b = item >> 1;
  if (b >= B) return;
  // the rectangle: window_features_kernel's origin and rim rule
  const int wy0 = min(max(win[b * 8 + 0] / level_stride, 0), H - wh), wx0 = min(max(win[b * 8 + 1] / level_stride, 0), W - ww);
  const int ry0 = wy0 + (wy0 > 0 ? margin : 0), ry1 = wy0 + wh - (wy0 + wh < H ? margin : 0);
  const int rx0 = wx0 + (wx0 > 0 ? margin : 0), rx1 = wx0 + ww - (wx0 + ww < W ? margin : 0);
  const int ys = ry0 + ((ry0 ^ yd) & 1) + 2 * (k * CH_WAVES + wave);             // the rectangle's rows of yd's parity
  const int dy = (case_b ? ys - yd : yd - ys) / 2 + R;                           // source row - row = 2 (dy - R)
  if (ys >= ry1 || dy < 0 || dy >= P || rx1 <= rx0) return;
  const long M = (long)B * H * W;
  const long rowS = ((long)b * H + ys) * W, rowD = ((long)b * H + yd) * W;
  if (case_b)
    corr_changed_rows<true>(f1, f2, in_plane_stride, out, out_plane_stride, out_chunk0, M, W, scale, slope, rowS, rowD, rowD, rx0, rx1, dy,
                            tiles[wave], lane);
  else
    corr_changed_rows<false>(f1, f2, in_plane_stride, out, out_plane_stride, out_chunk0, M, W, scale, slope, rowS, rowD, rowS, rx0, rx1, dy,
                             tiles[wave], lane);
}

}  // namespace

extern "C" int ufr_corr_forward_planes(const void* f1_planes, const void* f2_planes, long in_plane_stride, void* out_planes,
                                       long out_plane_stride, int out_chunk0, int B, int C, int H, int W, int patch,
                                       int dilation_patch, float scale, float slope, ufr_stream_t stream) {
  UFR_REQUIRE(f1_planes && f2_planes && out_planes, "correlation (planes): null pointer");
  UFR_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H < 65536 && out_chunk0 >= 0, "correlation (planes): bad shape");
  if (C != 32 * KCH || patch != P || dilation_patch != 2)
    return ufr::fail(UFR_EUNSUPPORTED, "correlation (planes): built for FlowNetC's configuration (256 channels, patch 21, "
                                       "dilation_patch 2); got C=%d patch=%d dilation_patch=%d", C, patch, dilation_patch);
  const int ni = (W + 1) / 2;                    // same-parity columns of a row (parity 0; parity 1 has W / 2)
  hipStream_t st = ufr::as_stream(stream);
  const __bf16* a = static_cast<const __bf16*>(f1_planes);
  const __bf16* b = static_cast<const __bf16*>(f2_planes);
  __bf16* o = static_cast<__bf16*>(out_planes);
  const int waves = ufr::ceil_div(ni, 16);
  int rc;
  if (waves <= 2) rc = launch_corr_planes<2>(a, b, in_plane_stride, o, out_plane_stride, out_chunk0, B, H, W, ni, scale, slope, st);
  else if (waves <= 4 || waves > 5 * 2)                         // 4-wave blocks also tile rows wider than one block
    rc = launch_corr_planes<4>(a, b, in_plane_stride, o, out_plane_stride, out_chunk0, B, H, W, ni, scale, slope, st);
  else                                                          // 160 columns (FlowNetC @1280): one block per row and parity
    rc = launch_corr_planes<5>(a, b, in_plane_stride, o, out_plane_stride, out_chunk0, B, H, W, ni, scale, slope, st);
  if (rc != UFR_OK) return rc;
  return ufr::launched("corr_fwd_planes_kernel");
}

extern "C" int ufr_corr_forward_planes_window(const void* f1_planes, const void* f2_planes, long in_plane_stride, void* out_planes,
                                              long out_plane_stride, int out_chunk0, int B, int C, int H, int W, int patch,
                                              int dilation_patch, float scale, float slope, const int* win, int level_stride,
                                              int win_cells, ufr_stream_t stream) {
  UFR_REQUIRE(f1_planes && f2_planes && out_planes && win, "correlation (planes, window): null pointer");
  UFR_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H < 65536 && out_chunk0 >= 0 && level_stride > 0 && win_cells > 0,
              "correlation (planes, window): bad shape");
  if (C != 32 * KCH || patch != P || dilation_patch != 2 || win_cells + 4 * R > 63)
    return ufr::fail(UFR_EUNSUPPORTED, "correlation (planes, window): 256 channels, patch 21, dilation_patch 2, windows of at most "
                                       "23 cells; got C=%d patch=%d dilation_patch=%d cells=%d", C, patch, dilation_patch, win_cells);
  // 2 x 32 same-parity columns from 20 cells left of the window cover [x0 - 20, x0 + cells + 20): every cell whose cost
  // volume can have changed when the features changed inside the window only
  int rc = launch_corr_planes<2>(static_cast<const __bf16*>(f1_planes), static_cast<const __bf16*>(f2_planes), in_plane_stride,
                                 static_cast<__bf16*>(out_planes), out_plane_stride, out_chunk0, B, H, W, (W + 1) / 2, scale, slope,
                                 ufr::as_stream(stream), win, level_stride);
  if (rc != UFR_OK) return rc;
  return ufr::launched("corr_fwd_planes_k2_kernel (window)");
}

extern "C" int ufr_corr_forward_planes_changed(const void* f1_planes, const void* f2_planes, long in_plane_stride, void* out_planes,
                                               long out_plane_stride, int out_chunk0, int B, int C, int H, int W, int patch,
                                               int dilation_patch, float scale, float slope, const int* win, int level_stride,
                                               int win_cells_h, int win_cells_w, int margin, ufr_stream_t stream) {
  UFR_REQUIRE(f1_planes && f2_planes && out_planes && win, "correlation (planes, changed): null pointer");
  UFR_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H < 65536 && out_chunk0 >= 0 && level_stride > 0 && win_cells_h > 0 &&
                  win_cells_w > 0 && margin >= 0, "correlation (planes, changed): bad shape");
  if (C != 32 * KCH || patch != P || dilation_patch != 2 || win_cells_w > CH_MAX_CELLS)
    return ufr::fail(UFR_EUNSUPPORTED, "correlation (planes, changed): 256 channels, patch 21, dilation_patch 2, windows of at most "
                                       "%d cells across; got C=%d patch=%d dilation_patch=%d cells=%d", CH_MAX_CELLS, C, patch,
                     dilation_patch, win_cells_w);
  UFR_REQUIRE(win_cells_h <= H && win_cells_w <= W && 2 * margin <= win_cells_h && 2 * margin <= win_cells_w,
              "correlation (planes, changed): window %dx%d (margin %d) in a frame of %dx%d cells", win_cells_h, win_cells_w, margin, H, W);
  const int groups = ufr::ceil_div((win_cells_h + 1) / 2, CH_WAVES);
  corr_fwd_planes_changed_kernel<<<B * 2 * H * groups, 64 * CH_WAVES, 0, ufr::as_stream(stream)>>>(
      static_cast<const __bf16*>(f1_planes), static_cast<const __bf16*>(f2_planes), in_plane_stride, static_cast<__bf16*>(out_planes),
      out_plane_stride, out_chunk0, B, H, W, scale, slope, win, level_stride, win_cells_h, win_cells_w, margin);
  return ufr::launched("corr_fwd_planes_changed_kernel");
}
