// submission.hip -- what the test-server submissions of training/evaluate.py:201-267 need on the device (gfx950):
//   ufr_forward_interpolate  `forward_interpolate` of models/raft/utils/utils.py:33-59, the warm start of `create_sintel_submission`:
//                            every low-resolution flow vector is splatted forward to (x0 + dx, y0 + dy), the points that stay inside
//                            the grid are kept, and every grid pixel takes the flow of its nearest kept point (scipy's
//                            `griddata(method="nearest")` there, between a D2H and an H2D copy).  Here: an exact brute-force search,
//                            float64 positions and distances, one launch, nothing leaves the device.
//   ufr_flow_encode          the payload of the two file formats from the padded-frame prediction: the interleaved float32 of a
//                            `.flo` file (`writeFlow`) or the 16-bit codes of a KITTI flow map (`writeFlowKITTI`), cropped in place.
#include "ufr_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kStage = 1024;           // source points per LDS slice: 16 KiB of (x1, y1) pairs

// The SLICES lanes that share a target pixel are neighbours in one wave: lane = target * SLICES + slice.  Lane `slice` scans the
// source points slice, slice + SLICES, ... of every LDS slice in ascending index with a strict `<`, so within a lane the lowest
// index wins a tie; the lanes' (d2, index) pairs meet in a lexicographic minimum, which is associative and commutative: any
// SLICES gives the same bits.  An invalid point is staged as (+inf, +inf): its distance is +inf and never below the initial +inf.
template <int SLICES>
__global__ __launch_bounds__(kBlock) void forward_interpolate_kernel(const float* __restrict__ flow, float* __restrict__ out, int H,
                                                                     int W) {
  __shared__ double2 pts[kStage];
  constexpr int kTargets = kBlock / SLICES;
  const int HW = H * W;
  const float* __restrict__ fx = flow + (long)blockIdx.y * 2 * HW;
  const float* __restrict__ fy = fx + HW;
  const int slice = threadIdx.x % SLICES;
  const int target = blockIdx.x * kTargets + threadIdx.x / SLICES;     // (a tail workgroup's surplus lanes stage and search like the rest -- they
                                                                       //  take part in the barriers -- and only store nothing)
  const double gx = (double)(target % W), gy = (double)(target / W);
  double best = INFINITY;
  int best_i = -1;
  for (int base = 0; base < HW; base += kStage) {
    const int n = min(kStage, HW - base);
    __syncthreads();                                                   // the previous slice has been read
    for (int j = threadIdx.x; j < n; j += kBlock) {
      const int i = base + j;
      const double x1 = (double)(i % W) + (double)fx[i], y1 = (double)(i / W) + (double)fy[i];      // utils.py:39-40 in float64
      const bool valid = x1 > 0.0 && x1 < (double)W && y1 > 0.0 && y1 < (double)H;                   // :45 (a NaN compares false)
      pts[j] = valid ? make_double2(x1, y1) : make_double2(INFINITY, INFINITY);
    }
    __syncthreads();
    for (int j = slice; j < n; j += SLICES) {
      const double2 p = pts[j];
      const double ex = p.x - gx, ey = p.y - gy;
      const double d2 = ex * ex + ey * ey;                             // (no contraction: -ffp-contract=off)
      if (d2 < best) {
        best = d2;
        best_i = base + j;
      }
    }
  }
#pragma unroll
  for (int off = 1; off < SLICES; off <<= 1) {
    const double other = __shfl_xor(best, off, 64);
    const int other_i = __shfl_xor(best_i, off, 64);
    if (other < best || (other == best && other_i < best_i)) {
      best = other;
      best_i = other_i;
    }
  }
  if (slice == 0 && target < HW) {
    float* __restrict__ o = out + (long)blockIdx.y * 2 * HW + target;
    o[0] = best_i >= 0 ? fx[best_i] : __builtin_nanf("");              // no valid point at all: NaN, as scipy 1.15 answers
    o[HW] = best_i >= 0 ? fy[best_i] : __builtin_nanf("");
  }
}

// data_utils.writeFlowKITTI: (64 * x + 2^15).astype(uint16).  64 * x is exact in float32, the sum is rounded once, the cast
// truncates towards zero.  numpy's cast is undefined outside the target range; here it is DEFINED: below 0 and NaN -> 0,
// at or above 65536 -> 65535.
__device__ __forceinline__ unsigned short kitti_code(float x) {
  const float v = 64.0f * x + 32768.0f;
  if (!(v >= 0.0f)) return 0;
  if (v >= 65536.0f) return 65535;
  return (unsigned short)(int)v;
}

// p runs over the K * H * W cropped pixels; the prediction is read at (y + top, x + left) of its padded frame
template <int MODE>
__global__ __launch_bounds__(kBlock) void flow_encode_kernel(const float* __restrict__ pred, void* __restrict__ out, long total, int Hp,
                                                             int Wp, int top, int left, int H, int W) {
  const long HW = (long)H * W, HWp = (long)Hp * Wp;
  for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < total; p += (long)gridDim.x * kBlock) {
    const long k = p / HW;
    const int q = (int)(p - k * HW);
    const int y = q / W, x = q - y * W;
    const float* __restrict__ src = pred + k * 2 * HWp + (long)(y + top) * Wp + (x + left);
    const float u = src[0], v = src[HWp];
    if constexpr (MODE == 0) {
      float* __restrict__ o = static_cast<float*>(out) + 2 * p;
      o[0] = u;
      o[1] = v;
    } else {
      unsigned short* __restrict__ o = static_cast<unsigned short*>(out) + 3 * p;
      o[0] = kitti_code(u);
      o[1] = kitti_code(v);
      o[2] = 1;
    }
  }
}

}  // namespace

extern "C" int ufr_forward_interpolate_sliced(const float* flow, float* out, int B, int H, int W, int slices, ufr_stream_t stream) {
  UFR_REQUIRE(flow && out, "forward interpolate: null pointer argument");
  UFR_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "forward interpolate: bad shape B=%d H=%d W=%d", B, H, W);
  UFR_REQUIRE((long)H * W < (1L << 29), "forward interpolate: too many pixels (%d x %d)", H, W);
  UFR_REQUIRE(slices == 1 || slices == 4 || slices == 16, "forward interpolate: slices %d (1, 4 or 16)", slices);
  hipStream_t st = ufr::as_stream(stream);
  const int HW = H * W;
  const dim3 grid(ufr::ceil_div(HW, kBlock / slices), B);
  if (slices == 1)
    forward_interpolate_kernel<1><<<grid, kBlock, 0, st>>>(flow, out, H, W);
  else if (slices == 4)
    forward_interpolate_kernel<4><<<grid, kBlock, 0, st>>>(flow, out, H, W);
  else
    forward_interpolate_kernel<16><<<grid, kBlock, 0, st>>>(flow, out, H, W);
  return ufr::launched("forward_interpolate_kernel");
}

extern "C" int ufr_forward_interpolate(const float* flow, float* out, int B, int H, int W, ufr_stream_t stream) {
  return ufr_forward_interpolate_sliced(flow, out, B, H, W, UFR_FORWARD_INTERPOLATE_SLICES, stream);
}

extern "C" int ufr_flow_encode(const float* pred, void* out, int K, int Hp, int Wp, int top, int left, int H, int W, int mode,
                               ufr_stream_t stream) {
  UFR_REQUIRE(pred && out, "flow encode: null pointer argument");
  UFR_REQUIRE(K > 0 && H > 0 && W > 0 && Hp > 0 && Wp > 0, "flow encode: bad shape K=%d Hp=%d Wp=%d H=%d W=%d", K, Hp, Wp, H, W);
  UFR_REQUIRE((long)H * W < (1L << 29) && (long)Hp * Wp < (1L << 29), "flow encode: too many pixels");
  UFR_REQUIRE(top >= 0 && left >= 0, "flow encode: negative pad top=%d left=%d", top, left);
  UFR_REQUIRE((long)top + H <= Hp && (long)left + W <= Wp,
              "flow encode: the crop of %d x %d at (%d, %d) leaves the padded frame of %d x %d", H, W, top, left, Hp, Wp);
  UFR_REQUIRE(mode == 0 || mode == 1, "flow encode: mode %d (0 float32 u, v interleaved, 1 KITTI 16-bit codes)", mode);
  hipStream_t st = ufr::as_stream(stream);
  const long total = (long)K * H * W;
  const int grid = ufr::stream_grid(total, kBlock);
  if (mode == 0)
    flow_encode_kernel<0><<<grid, kBlock, 0, st>>>(pred, out, total, Hp, Wp, top, left, H, W);
  else
    flow_encode_kernel<1><<<grid, kBlock, 0, st>>>(pred, out, total, Hp, Wp, top, left, H, W);
  return ufr::launched("flow_encode_kernel");
}
