// validation.hip -- the validation of the fine-tuning loop (gfx950): training/evaluate.py:270-392 (`validate_chairs`, `validate_sintel`,
// `validate_kitti`) pads every item with models/raft/utils/utils.py:7-30 (`InputPadder`), runs one batch-1 forward, copies the
// prediction to the host and keeps a per-pixel error array per item.  Two streaming entries serve a chunk of K items:
//   ufr_validation_pad      the replicate pad of both frames of the K pairs (and FlowNetC's division by 255), one launch, bit-equal to
//                           torch on this device;
//   ufr_validation_metrics  crops the padded-frame prediction in place and reduces the per-pixel errors of the three validators to
//                           eight float64 values per item: float32 per pixel with every operation rounded on its own (what the
//                           reference's threshold comparisons see), float64 sums, the per-item metrics scheme of ufr_common.h
//                           with `slots` partials per item in the workspace.
#include "ufr_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kCols = 8;               // UFR_VALIDATION_COLS

using ufr::aligned16;

// torch's device kernel for `x / 255.0` (a host scalar divisor) multiplies by the float32 reciprocal
__device__ __forceinline__ float scaled(float v, float inv) { return v * inv; }

// q runs over [K,3,Hp,Wp] in units of V floats of one output row (V = 4 needs Wp % 4 == 0); `src4` says that a unit whose four
// sources are interior columns may be read as one 16-byte load (W % 4 == 0, left % 4 == 0, aligned inputs)
template <int V, bool DIV>
__global__ __launch_bounds__(kBlock) void validation_pad_kernel(const float* __restrict__ image1, const float* __restrict__ image2,
                                                                float* __restrict__ out1, float* __restrict__ out2, long total, int H,
                                                                int W, int Hp, int Wp, int top, int left, int src4, float inv) {
  const int units = Wp / V;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const long row = q / units;                                  // (k * 3 + c) * Hp + yp
    const int xp = (int)(q - row * units) * V;
    const long plane = row / Hp;
    const int yp = (int)(row - plane * Hp);
    const int y = min(max(yp - top, 0), H - 1);
    const long src = (plane * H + y) * (long)W;
    const long dst = row * (long)Wp + xp;
    if constexpr (V == 4) {
      const int x0 = xp - left;
      float4 a, b;
      if (src4 && x0 >= 0 && x0 + 3 < W) {
        a = *reinterpret_cast<const float4*>(image1 + src + x0);
        b = *reinterpret_cast<const float4*>(image2 + src + x0);
      } else {
        const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1), xc = min(max(x0 + 2, 0), W - 1),
                  xd = min(max(x0 + 3, 0), W - 1);
        a = make_float4(image1[src + xa], image1[src + xb], image1[src + xc], image1[src + xd]);
        b = make_float4(image2[src + xa], image2[src + xb], image2[src + xc], image2[src + xd]);
      }
      if constexpr (DIV) {
        a = make_float4(scaled(a.x, inv), scaled(a.y, inv), scaled(a.z, inv), scaled(a.w, inv));
        b = make_float4(scaled(b.x, inv), scaled(b.y, inv), scaled(b.z, inv), scaled(b.w, inv));
      }
      *reinterpret_cast<float4*>(out1 + dst) = a;
      *reinterpret_cast<float4*>(out2 + dst) = b;
    } else {
      const int x = min(max(xp - left, 0), W - 1);
      const float a = image1[src + x], b = image2[src + x];
      out1[dst] = DIV ? scaled(a, inv) : a;
      out2[dst] = DIV ? scaled(b, inv) : b;
    }
  }
}

// sqrtf and `/` are the correctly rounded forms under hipcc's default (-fhip-fp32-correctly-rounded-divide-sqrt); the __fsqrt_rn
// intrinsic is NOT (it maps to the native, approximate square root unless OCML_BASIC_ROUNDED_OPERATIONS is defined).
// one entry of the reference's error array: the comparisons are numpy's (a NaN compares false), the sum takes the NaN
__device__ __forceinline__ void entry(float e, float mag, bool val, double* sum) {
  sum[0] += (double)e;
  sum[1] += 1.0;
  if (e < 1.0f) sum[2] += 1.0;
  if (e < 3.0f) sum[3] += 1.0;
  if (e < 5.0f) sum[4] += 1.0;
  if (val) {
    sum[5] += (double)e;
    sum[6] += 1.0;
    if (e > 3.0f && e / mag > 0.05f) sum[7] += 1.0;           // evaluate.py:381
  }
}

// grid (slots, K): workgroup (s, k) walks the ground-truth pixels s * 256 + t, + slots * 256, ... of item k and reads the
// prediction at (y + top, x + left) of its padded frame
__global__ __launch_bounds__(kBlock) void validation_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                    const float* __restrict__ valid, int Hp, int Wp, int top, int left,
                                                                    int H, int W, int mode, double* __restrict__ part) {
  __shared__ double lds[kBlock / 64];
  const int k = blockIdx.y;
  const long HW = (long)H * W, HWp = (long)Hp * Wp;
  const float* __restrict__ pu = pred + (long)k * 2 * HWp;
  const float* __restrict__ pv = pu + HWp;
  const float* __restrict__ gu = gt + (long)k * 2 * HW;
  const float* __restrict__ gv = gu + HW;
  const float* __restrict__ vk = valid != nullptr ? valid + (long)k * HW : nullptr;
  double sum[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < HW; p += (long)gridDim.x * kBlock) {
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const long pp = (long)(y + top) * Wp + (x + left);
    const float fu = pu[pp], fv = mode == 2 ? fu : pv[pp];
    const float a = gu[p], b = gv[p];
    const float du = fu - a, dv = fv - b;
    const float du2 = du * du, dv2 = dv * dv;
    const float a2 = a * a, b2 = b * b;
    const float mag = sqrtf(a2 + b2);                                // evaluate.py:375
    const bool val = vk == nullptr || vk[p] >= 0.5f;                      // :379
    if (mode == 0) {
      entry(sqrtf(du2 + dv2), mag, val, sum);                        // :290, :374
    } else {
      entry(sqrtf(du2), mag, val, sum);                              // :328: the sum runs over the batch axis of size 1
      entry(sqrtf(dv2), mag, val, sum);
    }
  }
  ufr::dev::store_partial<kBlock, kCols>(sum, lds, part, k, gridDim.x);
}

// grid K: one workgroup adds the `slots` partials of its item in a fixed order
__global__ __launch_bounds__(kBlock) void validation_metrics_finalize_kernel(const double* __restrict__ part, int slots,
                                                                             double* __restrict__ out) {
  __shared__ double lds[kBlock / 64];
  const int k = blockIdx.x;
  double t[kCols];
  ufr::dev::item_totals<kBlock, kCols>(part, k, slots, slots, lds, t);
  if (threadIdx.x == 0)
    for (int q = 0; q < kCols; ++q) out[(long)k * kCols + q] = t[q];
}

template <int V>
void launch_pad(bool div, const float* image1, const float* image2, float* out1, float* out2, long total, int H, int W, int Hp, int Wp,
                int top, int left, int src4, hipStream_t st) {
  const float inv = 1.0f / 255.0f;
  const int grid = ufr::stream_grid(total, kBlock);
  if (div)
    validation_pad_kernel<V, true><<<grid, kBlock, 0, st>>>(image1, image2, out1, out2, total, H, W, Hp, Wp, top, left, src4, inv);
  else
    validation_pad_kernel<V, false><<<grid, kBlock, 0, st>>>(image1, image2, out1, out2, total, H, W, Hp, Wp, top, left, src4, inv);
}

}  // namespace

extern "C" int ufr_validation_pad(const float* image1, const float* image2, float* out1, float* out2, int K, int H, int W, int top,
                                  int bottom, int left, int right, int divide_by_255, ufr_stream_t stream) {
  UFR_REQUIRE(image1 && image2 && out1 && out2, "validation pad: null pointer argument");
  UFR_REQUIRE(K > 0 && H > 0 && W > 0, "validation pad: bad shape K=%d H=%d W=%d", K, H, W);
  UFR_REQUIRE(top >= 0 && bottom >= 0 && left >= 0 && right >= 0, "validation pad: negative pad top=%d bottom=%d left=%d right=%d", top,
              bottom, left, right);
  UFR_REQUIRE((long)H + top + bottom < (1L << 20) && (long)W + left + right < (1L << 20), "validation pad: padded frame too large");
  const int Hp = H + top + bottom, Wp = W + left + right;
  UFR_REQUIRE((long)Hp * Wp <= (1L << 40) / 3 / K, "validation pad: too many pixels");
  hipStream_t st = ufr::as_stream(stream);
  const long total = (long)K * 3 * Hp * Wp;
  if (Wp % 4 == 0 && aligned16(out1, out2)) {
    const int src4 = W % 4 == 0 && left % 4 == 0 && aligned16(image1, image2) ? 1 : 0;
    launch_pad<4>(divide_by_255 != 0, image1, image2, out1, out2, total / 4, H, W, Hp, Wp, top, left, src4, st);
  } else {
    launch_pad<1>(divide_by_255 != 0, image1, image2, out1, out2, total, H, W, Hp, Wp, top, left, 0, st);
  }
  return ufr::launched("validation_pad_kernel");
}

extern "C" long ufr_validation_metrics_workspace_doubles(int K, int H, int W) {
  if (K < 1 || H < 1 || W < 1 || (long)H * W >= (1L << 29)) return -1;
  return (long)K * ufr::metric_slots((long)H * W, kBlock) * kCols;
}

extern "C" int ufr_validation_metrics(const float* pred, const float* gt, const float* valid, int K, int Hp, int Wp, int top, int left,
                                      int H, int W, int mode, double* ws, long ws_elems, double* out, int row0, int rows,
                                      ufr_stream_t stream) {
  UFR_REQUIRE(pred && gt && ws && out, "validation metrics: null pointer argument");
  UFR_REQUIRE(K > 0 && K <= 65535 && H > 0 && W > 0 && Hp > 0 && Wp > 0, "validation metrics: bad shape K=%d Hp=%d Wp=%d H=%d W=%d", K, Hp,
              Wp, H, W);
  UFR_REQUIRE((long)H * W < (1L << 29) && (long)Hp * Wp < (1L << 29), "validation metrics: too many pixels");
  UFR_REQUIRE(top >= 0 && left >= 0, "validation metrics: negative pad top=%d left=%d", top, left);
  UFR_REQUIRE((long)top + H <= Hp && (long)left + W <= Wp,
              "validation metrics: the crop of %d x %d at (%d, %d) leaves the padded frame of %d x %d", H, W, top, left, Hp, Wp);
  UFR_REQUIRE(mode >= 0 && mode <= 2, "validation metrics: mode %d (0 end-point, 1 per component, 2 channel 0 against both)", mode);
  if (int rc = ufr::check_result_rows("validation metrics", row0, K, rows)) return rc;
  if (int rc = ufr::check_workspace("validation metrics", ws_elems, ufr_validation_metrics_workspace_doubles(K, H, W))) return rc;
  hipStream_t st = ufr::as_stream(stream);
  const int slots = ufr::metric_slots((long)H * W, kBlock);      // from the sizes alone: it fixes the order of the sums
  validation_metrics_kernel<<<dim3(slots, K), kBlock, 0, st>>>(pred, gt, valid, Hp, Wp, top, left, H, W, mode, ws);
  if (int rc = ufr::launched("validation_metrics_kernel")) return rc;
  validation_metrics_finalize_kernel<<<K, kBlock, 0, st>>>(ws, slots, out + (long)kCols * row0);
  return ufr::launched("validation_metrics_finalize_kernel");
}
