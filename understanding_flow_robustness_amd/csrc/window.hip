// window.hip -- "cone of influence" windows for the patch attack (gfx950).
//
// patch_attacks/main.py:537-600 multiplies the image gradient by the patch mask and changes only the
// masked pixels between iterations.  For a purely convolutional encoder prefix (FlowNetC conv1-3,
// models/FlowNetC.py:96-104) that means
//   * backward: d loss/d patch only needs the encoder's adjoint inside the patch's forward cone, and
//   * forward (iterations >= 2 of one attack() call): encoder features outside the cone are unchanged.
// So the encoder runs on a small window around the patch; these kernels move data between the
// full-size tensors and the window at an origin that lives in DEVICE memory (a captured HIP graph
// follows new patch placements without re-capture):
//   ufr_cone_window    mask -> bounding box -> cone through the conv chain -> window origin
//   ufr_window_gather  full tensor -> window (optionally zeroing the inexact rim)
//   ufr_window_scatter window -> full tensor (optionally skipping the inexact rim)
// The "inexact rim": a zero-padded convolution on the window differs from the full-image one within
// `margin` cells of a window edge, except where that edge IS the image edge (same padding).
#include <climits>

#include "ufr_common.h"

namespace {

// win[n] = {y0, x0, need_h, need_w, ymin, ymax, xmin, xmax}; y0/x0/need_* in input pixels
constexpr int kWinInts = 8;

__global__ void bbox_init_kernel(int* __restrict__ win, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int* w = win + n * kWinInts;
  w[0] = w[1] = w[2] = w[3] = 0;
  w[4] = INT_MAX; w[5] = -1; w[6] = INT_MAX; w[7] = -1;
}

// grid (blocks, N): bounding box of mask != 0 over all channels of sample n
__global__ void bbox_kernel(const float* __restrict__ mask, long bstride, int C, int H, int W,
                            int* __restrict__ win) {
  const int n = blockIdx.y;
  const float* m = mask + (long)n * bstride;
  const long total = (long)C * H * W;
  int ymin = INT_MAX, ymax = -1, xmin = INT_MAX, xmax = -1;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    if (m[i] != 0.f) {
      const int r = (int)(i % ((long)H * W));
      const int y = r / W, x = r - y * W;
      ymin = min(ymin, y); ymax = max(ymax, y); xmin = min(xmin, x); xmax = max(xmax, x);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    ymin = min(ymin, __shfl_xor(ymin, o)); ymax = max(ymax, __shfl_xor(ymax, o));
    xmin = min(xmin, __shfl_xor(xmin, o)); xmax = max(xmax, __shfl_xor(xmax, o));
  }
  if ((threadIdx.x & 63) == 0 && ymax >= 0) {
    int* w = win + n * kWinInts;
    atomicMin(w + 4, ymin); atomicMax(w + 5, ymax); atomicMin(w + 6, xmin); atomicMax(w + 7, xmax);
  }
}

using ufr::dev::cone_axis;          // one axis of the window cone (ufr_common.h)
using ufr::dev::floor_div;

__global__ void cone_finalize_kernel(int* __restrict__ win, int N, int H, int W, ufr_cone_chain ch, int win_h,
                                     int win_w, float* __restrict__ overflow) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int* w = win + n * kWinInts;
  cone_axis(w[4], w[5], H, ch, win_h, w + 0, w + 2);
  cone_axis(w[6], w[7], W, ch, win_w, w + 1, w + 3);
  if ((w[2] > win_h || w[3] > win_w) && overflow) atomicAdd(overflow, 1.0f);
}

// One thread per window element.  GATHER: dst[n,c,i,j] = src[n,c,y0+i,x0+j] (0 on the inexact rim);
// SCATTER: dst[n,c,y0+i,x0+j] = src[n,c,i,j] (rim skipped).
template <bool GATHER>
__global__ void window_copy_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                   const int* __restrict__ win, int n_win, int C, int Hf, int Wf, int wh, int ww,
                                   int level_stride, int margin, long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int j = (int)(i % ww);
    long r = i / ww;
    const int ii = (int)(r % wh); r /= wh;
    const int c = (int)(r % C);
    const int n = (int)(r / C);
    const int* w = win + (n % n_win) * kWinInts;
    // clamped: an origin that was never computed cannot send the copy out of bounds
    const int y0 = min(max(w[0] / level_stride, 0), Hf - wh), x0 = min(max(w[1] / level_stride, 0), Wf - ww);
    const bool rim = (ii < margin && y0 > 0) || (ii >= wh - margin && y0 + wh < Hf) ||
                     (j < margin && x0 > 0) || (j >= ww - margin && x0 + ww < Wf);
    const long full = (((long)n * C + c) * Hf + (y0 + ii)) * Wf + (x0 + j);
    if (GATHER) dst[i] = rim ? 0.f : src[full];
    else if (!rim) dst[full] = src[i];
  }
}

// The window of a chunk-major float32 tensor [chunks][N * Hf * Wf][32] (the engine's gradient sums) as a chunk-major
// window tensor [chunks][N_dst * wh * ww][32], rim zeroed like window_copy_kernel<true>; images n >= N of dst are not touched.
__global__ void window_gather_chunks_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ win,
                                            int n_win, int N, int N_dst, int chunks, int Hf, int Wf, int wh, int ww, int level_stride,
                                            int margin, long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int q = (int)(i & 7);                      // float4 of the pixel's 32 channels
    long r = i >> 3;
    const int j = (int)(r % ww); r /= ww;
    const int ii = (int)(r % wh); r /= wh;
    const int n = (int)(r % N);
    const int ch = (int)(r / N);
    const int* w = win + (n % n_win) * kWinInts;
    const int y0 = min(max(w[0] / level_stride, 0), Hf - wh), x0 = min(max(w[1] / level_stride, 0), Wf - ww);
    const bool rim = (ii < margin && y0 > 0) || (ii >= wh - margin && y0 + wh < Hf) ||
                     (j < margin && x0 > 0) || (j >= ww - margin && x0 + ww < Wf);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!rim) v = *reinterpret_cast<const float4*>(src + (((long)ch * N * Hf + (long)n * Hf + y0 + ii) * Wf + x0 + j) * 32 + q * 4);
    *reinterpret_cast<float4*>(dst + (((long)ch * N_dst * wh + (long)n * wh + ii) * ww + j) * 32 + q * 4) = v;
  }
}

// Both frame stacks' windows in one launch (margin 0, pixels): xw [2N, C, wh, ww] = windows of a (images 0..N-1) and of b
// (images N..2N-1), as two window_copy_kernel<true> launches write them; `zero` (optional) receives 0.f.
__global__ void window_gather_pair_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ xw,
                                          const int* __restrict__ win, int N, int C, int Hf, int Wf, int wh, int ww, long total,
                                          float* __restrict__ zero) {
  if (zero != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *zero = 0.f;
  const long half = total >> 1;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long e = i < half ? i : i - half;
    const int j = (int)(e % ww);
    long r = e / ww;
    const int ii = (int)(r % wh); r /= wh;
    const int c = (int)(r % C);
    const int n = (int)(r / C);
    const int* w = win + n * kWinInts;
    const int y0 = min(max(w[0], 0), Hf - wh), x0 = min(max(w[1], 0), Wf - ww);
    const long full = (((long)n * C + c) * Hf + (y0 + ii)) * Wf + (x0 + j);
    xw[i] = (i < half ? a : b)[full];
  }
}

// ---- one attack() call's placement in one launch (ufr_attack_place) -------------------------------------------------------------
// Up to this many pairs' host origins travel as a kernel argument (no pageable host-to-device copy)
constexpr int kPlaceByValue = 64;
struct PlaceOrigins {
  int v[2 * kPlaceByValue];
};
struct PlaceArgs {
  const float *patch, *mask_p, *patch_init;
  float *patch_dst, *mask_dst, *init_dst, *loaded_dst, *state;
  const int* origins_src;      // device origins (nullptr: `by_value`)
  int *origins_dst, *win, *band_win;
  int B, H, W, ph, pw, has_chain, win_h, win_w, band_width, band_reach, corr_width, corr_reach;
};

// One workgroup: the patch-coordinate operands into the step's static buffers, state = 0, the bounding box of mask_p, and per pair
// the window table of ufr_cone_window (the canvas mask's box is origin + that box: the canvas holds mask_p at the origin, clipped
// to the frame) with the overflow count in state[3], plus the two band origins derived from the window's first column.
__global__ __launch_bounds__(1024) void attack_place_kernel(const PlaceArgs a, const PlaceOrigins by_value, const ufr_cone_chain ch) {
  __shared__ int box[4];       // imin, imax, jmin, jmax over mask_p != 0 (all channels)
  __shared__ int overflow;
  const int tid = threadIdx.x, n = 3 * a.ph * a.pw, plane = a.ph * a.pw;
  if (tid == 0) { box[0] = INT_MAX; box[1] = -1; box[2] = INT_MAX; box[3] = -1; overflow = 0; }
  __syncthreads();
  int imin = INT_MAX, imax = -1, jmin = INT_MAX, jmax = -1;
  for (int e = tid; e < n; e += blockDim.x) {
    const float m = a.mask_p[e], p = a.patch[e];
    a.mask_dst[e] = m;
    a.patch_dst[e] = p;
    a.init_dst[e] = a.patch_init[e];
    if (a.loaded_dst) a.loaded_dst[e] = p;
    if (m != 0.f) {
      const int r = e % plane, i = r / a.pw, j = r - i * a.pw;
      imin = min(imin, i); imax = max(imax, i); jmin = min(jmin, j); jmax = max(jmax, j);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    imin = min(imin, __shfl_xor(imin, o)); imax = max(imax, __shfl_xor(imax, o));
    jmin = min(jmin, __shfl_xor(jmin, o)); jmax = max(jmax, __shfl_xor(jmax, o));
  }
  if ((tid & 63) == 0 && imax >= 0) {
    atomicMin(&box[0], imin); atomicMax(&box[1], imax); atomicMin(&box[2], jmin); atomicMax(&box[3], jmax);
  }
  __syncthreads();
  for (int b = tid; b < a.B; b += blockDim.x) {
    const int oy = a.origins_src ? a.origins_src[2 * b] : by_value.v[2 * b];
    const int ox = a.origins_src ? a.origins_src[2 * b + 1] : by_value.v[2 * b + 1];
    a.origins_dst[2 * b] = oy;
    a.origins_dst[2 * b + 1] = ox;
    if (!a.has_chain) continue;
    int ymin = INT_MAX, ymax = -1, xmin = INT_MAX, xmax = -1;
    if (oy >= 0 && ox >= 0 && oy + a.ph <= a.H && ox + a.pw <= a.W) {
      if (box[1] >= 0) { ymin = oy + box[0]; ymax = oy + box[1]; xmin = ox + box[2]; xmax = ox + box[3]; }
    } else {
      // a device-resident placement that leaves the frame (not validated on the host): the canvas shows the part inside only
      for (int e = 0; e < n; ++e) {
        if (a.mask_p[e] == 0.f) continue;
        const int r = e % plane, i = r / a.pw, y = oy + i, x = ox + r - i * a.pw;
        if ((unsigned)y >= (unsigned)a.H || (unsigned)x >= (unsigned)a.W) continue;
        ymin = min(ymin, y); ymax = max(ymax, y); xmin = min(xmin, x); xmax = max(xmax, x);
      }
    }
    int* w = a.win + b * kWinInts;
    w[4] = ymin; w[5] = ymax; w[6] = xmin; w[7] = xmax;
    int o0, o1, n0, n1;
    cone_axis(ymin, ymax, a.H, ch, a.win_h, &o0, &n0);
    cone_axis(xmin, xmax, a.W, ch, a.win_w, &o1, &n1);
    w[0] = o0; w[1] = o1; w[2] = n0; w[3] = n1;
    if (n0 > a.win_h || n1 > a.win_w) atomicAdd(&overflow, 1);
    if (a.band_win != nullptr && a.band_width > 0) {   // band start: 32-pixel aligned, `reach` left of the window, inside the frame
      int* bw = a.band_win + b * kWinInts;
      bw[1] = min(max(floor_div(o1 - a.band_reach, 32) * 32, 0), a.W - a.band_width);
      if (a.corr_width > 0) bw[2] = min(max(o1 - a.corr_reach, 0), a.W - a.corr_width);
    }
  }
  __syncthreads();
  if (tid == 0) {
    a.state[0] = a.state[1] = a.state[2] = 0.f;
    a.state[3] = (float)overflow;
  }
}

int check_window(const char* what, int N, int C, int Hf, int Wf, int wh, int ww, int level_stride, int margin,
                 int n_win) {
  UFR_REQUIRE(N > 0 && C > 0 && Hf > 0 && Wf > 0, "%s: bad shape N=%d C=%d H=%d W=%d", what, N, C, Hf, Wf);
  UFR_REQUIRE(wh > 0 && ww > 0 && wh <= Hf && ww <= Wf, "%s: window %dx%d does not fit %dx%d", what, wh, ww, Hf, Wf);
  UFR_REQUIRE(level_stride > 0 && margin >= 0 && 2 * margin <= wh && 2 * margin <= ww, "%s: bad stride/margin", what);
  UFR_REQUIRE(n_win > 0 && n_win <= N, "%s: n_win=%d out of range", what, n_win);
  return UFR_OK;
}

}  // namespace

extern "C" int ufr_cone_window(const float* mask, int N, long mask_bstride, int C, int H, int W,
                               const ufr_cone_chain* chain, int win_h, int win_w, int* win, float* overflow,
                               ufr_stream_t stream) {
  UFR_REQUIRE(mask && chain && win, "cone_window: null pointer");
  UFR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "cone_window: bad shape N=%d C=%d H=%d W=%d", N, C, H, W);
  UFR_REQUIRE(chain->n_layers > 0 && chain->n_layers <= UFR_MAX_CONE_LAYERS && chain->n_taps > 0 &&
                  chain->n_taps <= UFR_MAX_CONE_LAYERS, "cone_window: bad chain");
  int total = 1;
  for (int l = 0; l < chain->n_layers; ++l) {
    UFR_REQUIRE(chain->kernel[l] > 0 && chain->stride[l] > 0 && chain->pad[l] >= 0, "cone_window: bad layer %d", l);
    total *= chain->stride[l];
  }
  for (int t = 0; t < chain->n_taps; ++t)
    UFR_REQUIRE(chain->tap_layer[t] >= 0 && chain->tap_layer[t] < chain->n_layers &&
                    (t == 0 || chain->tap_layer[t] >= chain->tap_layer[t - 1]) && chain->tap_margin[t] >= 0,
                "cone_window: taps must be sorted by layer");
  UFR_REQUIRE(H % total == 0 && W % total == 0, "cone_window: %dx%d is not a multiple of the chain stride %d", H, W, total);
  UFR_REQUIRE(win_h > 0 && win_w > 0 && win_h % total == 0 && win_w % total == 0 && win_h <= H && win_w <= W,
              "cone_window: window %dx%d must be a multiple of %d inside %dx%d", win_h, win_w, total, H, W);
  hipStream_t st = ufr::as_stream(stream);
  bbox_init_kernel<<<ufr::ceil_div(N, 64), 64, 0, st>>>(win, N);
  const long per = (long)C * H * W;
  dim3 grid(ufr::stream_grid(per, 256) > 256 ? 256 : ufr::stream_grid(per, 256), N);
  bbox_kernel<<<grid, 256, 0, st>>>(mask, mask_bstride, C, H, W, win);
  cone_finalize_kernel<<<ufr::ceil_div(N, 64), 64, 0, st>>>(win, N, H, W, *chain, win_h, win_w, overflow);
  return ufr::launched("cone_window");
}

static int check_chain(const char* what, const ufr_cone_chain* chain, int H, int W, int win_h, int win_w) {
  UFR_REQUIRE(chain->n_layers > 0 && chain->n_layers <= UFR_MAX_CONE_LAYERS && chain->n_taps > 0 &&
                  chain->n_taps <= UFR_MAX_CONE_LAYERS, "%s: bad chain", what);
  int total = 1;
  for (int l = 0; l < chain->n_layers; ++l) {
    UFR_REQUIRE(chain->kernel[l] > 0 && chain->stride[l] > 0 && chain->pad[l] >= 0, "%s: bad layer %d", what, l);
    total *= chain->stride[l];
  }
  for (int t = 0; t < chain->n_taps; ++t)
    UFR_REQUIRE(chain->tap_layer[t] >= 0 && chain->tap_layer[t] < chain->n_layers &&
                    (t == 0 || chain->tap_layer[t] >= chain->tap_layer[t - 1]) && chain->tap_margin[t] >= 0,
                "%s: taps must be sorted by layer", what);
  UFR_REQUIRE(H % total == 0 && W % total == 0, "%s: %dx%d is not a multiple of the chain stride %d", what, H, W, total);
  UFR_REQUIRE(win_h > 0 && win_w > 0 && win_h % total == 0 && win_w % total == 0 && win_h <= H && win_w <= W,
              "%s: window %dx%d must be a multiple of %d inside %dx%d", what, win_h, win_w, total, H, W);
  return UFR_OK;
}

extern "C" int ufr_attack_place(const float* patch, const float* mask_p, const float* patch_init, const int* origins,
                                const int* origins_host, float* patch_dst, float* mask_dst, float* init_dst, float* loaded_dst,
                                int* origins_dst, float* state, int B, int H, int W, int ph, int pw, const ufr_cone_chain* chain,
                                int win_h, int win_w, int* win, int* band_win, int band_width, int band_reach, int corr_width,
                                int corr_reach, ufr_stream_t stream) {
  UFR_REQUIRE(patch && mask_p && patch_init && patch_dst && mask_dst && init_dst && origins_dst && state,
              "attack place: null pointer argument");
  UFR_REQUIRE((origins != nullptr) != (origins_host != nullptr), "attack place: origins on the device OR on the host");
  UFR_REQUIRE(B > 0 && H > 0 && W > 0 && ph > 0 && pw > 0 && ph <= H && pw <= W && (long)3 * ph * pw < (1L << 30),
              "attack place: bad shape");
  if (origins_host)
    for (int b = 0; b < B; ++b)
      UFR_REQUIRE(origins_host[2 * b] >= 0 && origins_host[2 * b] + ph <= H && origins_host[2 * b + 1] >= 0 &&
                      origins_host[2 * b + 1] + pw <= W, "attack place: a placement leaves the frame");
  ufr_cone_chain ch = {};
  if (chain) {
    UFR_REQUIRE(win, "attack place: a chain needs the window table");
    if (int rc = check_chain("attack place", chain, H, W, win_h, win_w)) return rc;
    ch = *chain;
    if (band_win && band_width > 0) {
      UFR_REQUIRE(band_width <= W && band_reach >= 0, "attack place: band of %d columns does not fit %d", band_width, W);
      UFR_REQUIRE(corr_width >= 0 && corr_width <= W && corr_reach >= 0, "attack place: bad correlation band");
    }
  }
  hipStream_t st = ufr::as_stream(stream);
  PlaceOrigins by_value = {};
  const int* src = origins;
  if (origins_host) {
    if (B <= kPlaceByValue) {
      for (int i = 0; i < 2 * B; ++i) by_value.v[i] = origins_host[i];
    } else {                                   // too many pairs for a kernel argument: through the destination table itself
      if (hipMemcpyAsync(origins_dst, origins_host, sizeof(int) * 2 * B, hipMemcpyHostToDevice, st) != hipSuccess)
        return ufr::launched("attack place: origins copy");
      src = origins_dst;
    }
  }
  PlaceArgs a = {patch, mask_p, patch_init, patch_dst, mask_dst, init_dst, loaded_dst, state, src, origins_dst, win, band_win,
                 B, H, W, ph, pw, chain ? 1 : 0, win_h, win_w, band_width, band_reach, corr_width, corr_reach};
  attack_place_kernel<<<1, 1024, 0, st>>>(a, by_value, ch);
  return ufr::launched("attack_place_kernel");
}

extern "C" int ufr_window_gather_pair(const float* a, const float* b, float* xw, const int* win, float* zero, int N, int C, int Hs,
                                      int Ws, int wh, int ww, ufr_stream_t stream) {
  UFR_REQUIRE(a && b && xw && win, "window_gather_pair: null pointer");
  if (int rc = check_window("window_gather_pair", N, C, Hs, Ws, wh, ww, 1, 0, N)) return rc;
  const long total = 2L * N * C * wh * ww;
  window_gather_pair_kernel<<<ufr::stream_grid(total, 256), 256, 0, ufr::as_stream(stream)>>>(a, b, xw, win, N, C, Hs, Ws, wh, ww,
                                                                                               total, zero);
  return ufr::launched("window_gather_pair");
}

extern "C" int ufr_window_gather(const float* src, float* dst, const int* win, int n_win, int N, int C, int Hs,
                                 int Ws, int wh, int ww, int level_stride, int margin, ufr_stream_t stream) {
  UFR_REQUIRE(src && dst && win, "window_gather: null pointer");
  if (int rc = check_window("window_gather", N, C, Hs, Ws, wh, ww, level_stride, margin, n_win)) return rc;
  const long total = (long)N * C * wh * ww;
  window_copy_kernel<true><<<ufr::stream_grid(total, 256), 256, 0, ufr::as_stream(stream)>>>(
      src, dst, win, n_win, C, Hs, Ws, wh, ww, level_stride, margin, total);
  return ufr::launched("window_gather");
}

extern "C" int ufr_window_scatter(const float* src, float* dst, const int* win, int n_win, int N, int C, int Hd,
                                  int Wd, int wh, int ww, int level_stride, int margin, ufr_stream_t stream) {
  UFR_REQUIRE(src && dst && win, "window_scatter: null pointer");
  if (int rc = check_window("window_scatter", N, C, Hd, Wd, wh, ww, level_stride, margin, n_win)) return rc;
  const long total = (long)N * C * wh * ww;
  window_copy_kernel<false><<<ufr::stream_grid(total, 256), 256, 0, ufr::as_stream(stream)>>>(
      src, dst, win, n_win, C, Hd, Wd, wh, ww, level_stride, margin, total);
  return ufr::launched("window_scatter");
}

extern "C" int ufr_window_gather_chunks(const float* src, float* dst, const int* win, int n_win, int N, int N_dst, int chunks,
                                        int Hs, int Ws, int wh, int ww, int level_stride, int margin, ufr_stream_t stream) {
  UFR_REQUIRE(src && dst && win, "window_gather_chunks: null pointer");
  if (int rc = check_window("window_gather_chunks", N, chunks, Hs, Ws, wh, ww, level_stride, margin, n_win)) return rc;
  UFR_REQUIRE(N_dst >= N, "window_gather_chunks: destination holds %d images, source %d", N_dst, N);
  const long total = (long)chunks * N * wh * ww * 8;
  window_gather_chunks_kernel<<<ufr::stream_grid(total, 256), 256, 0, ufr::as_stream(stream)>>>(
      src, dst, win, n_win, N, N_dst, chunks, Hs, Ws, wh, ww, level_stride, margin, total);
  return ufr::launched("window_gather_chunks");
}
