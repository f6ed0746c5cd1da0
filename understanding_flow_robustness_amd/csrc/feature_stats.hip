// feature_stats.hip -- per-image, per-channel sums of feature maps where the engine left them (gfx950).
//
// patch_attacks/test_patch_embeddings.py of the reference copies every feature map of a forward to the host and takes np.mean over
// its pixels.  Here a map is a chunk range of a planes buffer (bf16 [3][chunks][images * pixels][32]) or a small NCHW float32
// tensor (the five flows), and only [B][channels] float64 sums leave the device: a streaming read at 6 bytes per element, so the
// target is HBM bandwidth.
//
//   stage 1  one workgroup per (segment, image, chunk, pixel slab): 16-byte loads (8 channels of one pixel per lane, 64 pixels per
//            pass), float64 accumulators, the workgroup's 64 pixel rows added through LDS by a fixed halving tree -> 32 partials in `ws`
//            (NCHW: one workgroup per (segment, image, channel, slab), the lanes' sums added in ascending lane order)
//   stage 2  one thread per (segment, image, channel): its slabs added in ascending order -> the result matrix
//
// The slab count depends on the pixel count alone and both orders are fixed: no float atomics, two runs are bit-identical.  The
// parallelism comes from the slabs (conv1 at 384 x 1280 has 2 chunks but 122,880 pixels per frame: 2 x 60 workgroups per frame).
// The segment table reaches both kernels by value in the kernel arguments (csrc/optim.hip does the same): the statistics of a whole
// forward are two launches.
#include <cmath>
#include <cstdint>

#include "ufr_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRows = kBlock / 4;                  // pixels per pass: four lanes (8 channels each) share one pixel's 64 bytes
constexpr long kSlabPixels = 2048;          // (1024: 0.43 ms for FlowNetC's 28 maps of 8 pairs at 384 x 1280, 2048: 0.38, 4096: 0.37)
constexpr int kMaxSlabs = 128;
constexpr int kMaxSegs = UFR_FEATURE_STATS_MAX_SEGS;

struct StatsArgs {
  ufr_feature_stats_seg seg[kMaxSegs];
  long ws0[kMaxSegs];                              // first partial of each segment
  int wg0[kMaxSegs + 1];                           // first workgroup of each segment; wg0[nseg] = the grid
  int nseg;
};

__host__ __device__ inline int slabs_for(long pixels) {
  const long s = (pixels + kSlabPixels - 1) / kSlabPixels;
  return (int)(s < 1 ? 1 : s > kMaxSlabs ? kMaxSlabs : s);
}
// pixels of one slab: the image split evenly, in whole passes
__host__ __device__ inline long slab_len(long pixels, int slabs) { return ((pixels + slabs - 1) / slabs + kRows - 1) / kRows * kRows; }
// what a segment's images are cut into, and the partial sums each (unit, slab) leaves: 32-lane chunks (planes) or channels (NCHW)
__host__ __device__ inline int units_of(const ufr_feature_stats_seg& s) { return s.kind == 0 ? (s.channels + 31) / 32 : s.channels; }
__host__ __device__ inline int lanes_of(const ufr_feature_stats_seg& s) { return s.kind == 0 ? 32 : 1; }

__device__ inline int find_seg(const StatsArgs& a, int wg) {      // wave-uniform
  int lo = 0, hi = a.nseg;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (wg >= a.wg0[mid]) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ inline double bf16_bits(unsigned bits16) { return (double)__uint_as_float(bits16 << 16); }
// The float32 value in front of a LeakyReLU of slope s whose output is x = fl(y * s) < 0: among the five floats around
// fl(x / s), the one of smallest magnitude whose product with s rounds back to x (x is such a product, so one exists within an
// ulp of the quotient; fl(x / s) itself when none does).  The rule does not depend on how the quotient was rounded, and
// `Planes.load_nchw(slope=s)` maps the result back to the same planes bit for bit.
__device__ inline double undo_leaky(double x, float s) {
  if (s == 0.f || !(x < 0.0)) return x;
  const float xf = (float)x;                         // exact: x is the sum of three bf16 that came from one float32
  const float y0 = __fdiv_rn(xf, s);
  const int b0 = __float_as_int(y0);
#pragma unroll
  for (int d = -2; d <= 2; ++d) {
    const float cand = __int_as_float(b0 + d);
    if (__fmul_rn(cand, s) == xf) return (double)cand;
  }
  return (double)y0;
}

__global__ __launch_bounds__(kBlock) void feature_stats_partial_kernel(StatsArgs a, double* __restrict__ ws) {
  __shared__ double lds[kRows][33];
  const int si = find_seg(a, blockIdx.x);
  const ufr_feature_stats_seg& s = a.seg[si];
  const long pixels = s.pixels;
  const int slabs = slabs_for(pixels), units = units_of(s);
  const long len = slab_len(pixels, slabs);
  int w = blockIdx.x - a.wg0[si];
  const int slab = w % slabs;
  w /= slabs;
  const int unit = w % units, b = w / units;
  const long p_lo = (long)slab * len;
  const long p_hi = p_lo + len < pixels ? p_lo + len : pixels;
  const float unleaky = (float)s.unleaky;
  const int t = threadIdx.x;
  if (s.kind == 0) {
    const int q = t & 3, r = t >> 2;
    const long M = (long)s.images * pixels, stride = s.plane_stride;
    const uint16_t* __restrict__ base =
        static_cast<const uint16_t*>(s.src) + (((long)(s.chunk0 + unit) * M + (long)(s.image0 + b) * pixels) << 5) + q * 8;
    double acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0;
#pragma unroll 2
    for (long p = p_lo + r; p < p_hi; p += kRows) {
      const uint16_t* px = base + (p << 5);
      const uint4 v0 = *reinterpret_cast<const uint4*>(px);
      const uint4 v1 = *reinterpret_cast<const uint4*>(px + stride);
      const uint4 v2 = *reinterpret_cast<const uint4*>(px + 2 * stride);
      const unsigned w0[4] = {v0.x, v0.y, v0.z, v0.w}, w1[4] = {v1.x, v1.y, v1.z, v1.w}, w2[4] = {v2.x, v2.y, v2.z, v2.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // p0 + p1 + p2 is exact in float32, hence in float64, in any order
        const double lo = bf16_bits(w0[j] & 0xffffu) + bf16_bits(w1[j] & 0xffffu) + bf16_bits(w2[j] & 0xffffu);
        const double hi = bf16_bits(w0[j] >> 16) + bf16_bits(w1[j] >> 16) + bf16_bits(w2[j] >> 16);
        acc[2 * j] += undo_leaky(lo, unleaky);
        acc[2 * j + 1] += undo_leaky(hi, unleaky);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) lds[r][q * 8 + j] = acc[j];
    __syncthreads();
    // the 64 pixel rows of the workgroup, halved six times: row r += row r + half (a fixed pairing, hence a fixed order)
    for (int half = kRows / 2; half >= 1; half >>= 1) {
      if (r < half) {
#pragma unroll
        for (int j = 0; j < 8; ++j) lds[r][q * 8 + j] += lds[r + half][q * 8 + j];
      }
      __syncthreads();
    }
    if (t < 32) ws[a.ws0[si] + ((long)(b * units + unit) * slabs + slab) * 32 + t] = lds[0][t];
  } else {
    // NCHW float32 [images][tensor channels][pixels]; plane_stride = its element count
    const long cn = s.plane_stride / ((long)s.images * pixels);
    const float* __restrict__ x = static_cast<const float*>(s.src) + ((long)(s.image0 + b) * cn + s.chunk0 + unit) * pixels;
    double acc = 0.0;
    for (long p = p_lo + t; p < p_hi; p += kBlock) acc += undo_leaky((double)x[p], unleaky);
    double* flat = &lds[0][0];
    flat[t] = acc;
    __syncthreads();
    if (t == 0) {
      double sum = 0.0;
      for (int i = 0; i < kBlock; ++i) sum += flat[i];
      ws[a.ws0[si] + (long)(b * units + unit) * slabs + slab] = sum;
    }
  }
}

// one workgroup per segment; a thread per (image, channel) adds that entry's slabs in ascending order
__global__ __launch_bounds__(kBlock) void feature_stats_finalize_kernel(StatsArgs a, const double* __restrict__ ws, double* __restrict__ out,
                                                                        long out_stride) {
  const ufr_feature_stats_seg& s = a.seg[blockIdx.x];
  const int slabs = slabs_for(s.pixels), units = units_of(s), lanes = lanes_of(s);
  const double* __restrict__ part = ws + a.ws0[blockIdx.x];
  for (int e = threadIdx.x; e < s.B * s.channels; e += kBlock) {
    const int b = e / s.channels, c = e % s.channels;
    const int unit = c / lanes, lane = c % lanes;
    const double* p = part + (long)(b * units + unit) * slabs * lanes + lane;
    double sum = 0.0;
    for (int i = 0; i < slabs; ++i) sum += p[(long)i * lanes];
    out[(long)b * out_stride + s.out_col + c] = sum;
  }
}

// everything ufr_feature_stats refuses about the table itself; 0 = fine
int check_table(const ufr_feature_stats_seg* segs, int nseg) {
  UFR_REQUIRE(segs != nullptr, "feature stats: null pointer argument (segment table)");
  UFR_REQUIRE(nseg >= 1 && nseg <= kMaxSegs, "feature stats: %d segments (1 .. %d per call)", nseg, kMaxSegs);
  for (int i = 0; i < nseg; ++i) {
    const ufr_feature_stats_seg& s = segs[i];
    UFR_REQUIRE(s.src != nullptr, "feature stats: null pointer argument (segment %d)", i);
    UFR_REQUIRE(s.kind == 0 || s.kind == 1, "feature stats: segment %d has kind %d (0: planes, 1: NCHW float32)", i, s.kind);
    UFR_REQUIRE(s.pixels > 0 && s.pixels < (1L << 30) && s.images > 0 && s.images <= 65536 && s.B > 0 && s.channels > 0 &&
                    s.channels <= 65536 && s.chunk0 >= 0 && s.chunk0 <= 65536 && s.image0 >= 0 && s.plane_stride > 0,
                "feature stats: bad shape in segment %d (pixels=%ld images=%d image0=%d B=%d chunk0=%d channels=%d)", i, s.pixels,
                s.images, s.image0, s.B, s.chunk0, s.channels);
    UFR_REQUIRE((long)s.image0 + s.B <= s.images, "feature stats: images [%d, %ld) of segment %d leave its buffer of %d images", s.image0,
                (long)s.image0 + s.B, i, s.images);
    UFR_REQUIRE(std::isfinite(s.unleaky) && s.unleaky >= 0.0, "feature stats: segment %d has unleaky slope %g (0: none, else > 0)", i,
                s.unleaky);
    const long M = (long)s.images * s.pixels;
    if (s.kind == 0) {
      const int chunks = (s.channels + 31) / 32;
      UFR_REQUIRE((long)(s.chunk0 + chunks) * M * 32 <= s.plane_stride,
                  "feature stats: chunks [%d, %d) of segment %d leave the planes operand (%ld chunks per plane)", s.chunk0,
                  s.chunk0 + chunks, i, s.plane_stride / (M * 32));
      UFR_REQUIRE((reinterpret_cast<uintptr_t>(s.src) & 15u) == 0, "feature stats: the planes of segment %d are not 16-byte aligned", i);
    } else {
      UFR_REQUIRE((long)(s.chunk0 + s.channels) * M <= s.plane_stride,
                  "feature stats: channels [%d, %d) of segment %d leave the tensor (%ld channels)", s.chunk0, s.chunk0 + s.channels, i,
                  s.plane_stride / M);
    }
    UFR_REQUIRE(s.out_col >= 0, "feature stats: segment %d starts at column %ld of the result matrix", i, s.out_col);
  }
  return UFR_OK;
}

long seg_partials(const ufr_feature_stats_seg& s) { return (long)s.B * units_of(s) * slabs_for(s.pixels) * lanes_of(s); }

}  // namespace

extern "C" long ufr_feature_stats_workspace_doubles(const ufr_feature_stats_seg* segs, int nseg) {
  if (check_table(segs, nseg) != UFR_OK) return -1;
  long n = 0;
  for (int i = 0; i < nseg; ++i) n += seg_partials(segs[i]);
  return n;
}

extern "C" int ufr_feature_stats(const ufr_feature_stats_seg* segs, int nseg, double* ws, long ws_elems, double* out, int out_rows,
                                 long out_cols, long out_stride, ufr_stream_t stream) {
  UFR_REQUIRE(segs && ws && out, "feature stats: null pointer argument");
  if (int rc = check_table(segs, nseg)) return rc;
  UFR_REQUIRE(out_rows > 0 && out_cols > 0 && out_stride >= out_cols, "feature stats: result matrix of %d rows x %ld columns, row stride %ld",
              out_rows, out_cols, out_stride);
  StatsArgs a;
  long ws_need = 0, wgs = 0;
  for (int i = 0; i < nseg; ++i) {
    const ufr_feature_stats_seg& s = segs[i];
    UFR_REQUIRE(s.B <= out_rows, "feature stats: segment %d writes %d rows of a result matrix of %d", i, s.B, out_rows);
    UFR_REQUIRE(s.out_col <= out_cols - s.channels, "feature stats: the %d columns from %ld of segment %d leave the result matrix (%ld columns)",
                s.channels, s.out_col, i, out_cols);                 // (out_col + channels could leave `long`)
    a.seg[i] = s;
    a.ws0[i] = ws_need;
    a.wg0[i] = (int)wgs;
    ws_need += seg_partials(s);
    wgs += (long)s.B * units_of(s) * slabs_for(s.pixels);
    UFR_REQUIRE(wgs < (1L << 30), "feature stats: too many workgroups (%ld)", wgs);
  }
  a.wg0[nseg] = (int)wgs;
  a.nseg = nseg;
  UFR_REQUIRE(ws_elems >= ws_need, "feature stats: workspace of %ld doubles, %ld needed", ws_elems, ws_need);
  hipStream_t st = ufr::as_stream(stream);
  feature_stats_partial_kernel<<<(int)wgs, kBlock, 0, st>>>(a, ws);
  if (int rc = ufr::launched("feature_stats_partial_kernel")) return rc;
  feature_stats_finalize_kernel<<<nseg, kBlock, 0, st>>>(a, ws, out, out_stride);
  return ufr::launched("feature_stats_finalize_kernel");
}
