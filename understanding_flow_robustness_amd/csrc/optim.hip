// optim.hip -- the optimiser half of a fine-tuning step: torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW over many tensors
// (training/train.py:277-280 of the reference), gfx950.
//
// Memory-bound: the arithmetic needs 8 passes over the parameters (read g for the norm; read p, g, m, v; write p, m, v).  The
// segments reach the kernels BY VALUE in the kernel arguments (kSegs per launch, the way multi-tensor-apply does it): no device
// table, no copy, no allocation.  A segment of n elements gets min(ceil(n / 4096), 1024) workgroups which stride over it, so the
// number of launches grows with the number of tensors only, and the partition -- hence every sum -- is a function of the sizes alone:
// two runs are bit-identical.  16-byte accesses where the pointers of a segment share their offset modulo 16 bytes; the (at most
// three) elements before the first aligned address and after the last full vector are handled one by one.
#include <cstdint>

#include "ufr_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSegs = 48;                          // segments per launch: 48 x 40 bytes + the workgroup table < 4 KiB of arguments
constexpr long kElemsPerWg = 4096;                 // 256 lanes x float4 x 4 iterations before a segment gets another workgroup
constexpr int kMaxWgPerSeg = 1024;

struct SegArgs {
  ufr_adamw_seg seg[kSegs];
  int wg0[kSegs + 1];                              // first workgroup of each segment; wg0[nseg] = the grid
  int nseg;
};

struct StepConsts {
  double decay, b1, omb1, b2, omb2;                // 1 - lr*wd, beta1, 1 - beta1, beta2, 1 - beta2
  float step_size, bc2_sqrt, eps;                  // lr / bias1, sqrt(bias2), eps
};

inline int seg_workgroups(long n) {
  long g = (n + kElemsPerWg - 1) / kElemsPerWg;
  return (int)(g < 1 ? 1 : g > kMaxWgPerSeg ? kMaxWgPerSeg : g);
}

// wave-uniform: every lane of a workgroup asks for the same workgroup index
__device__ inline int find_seg(const SegArgs& a, int wg) {
  int lo = 0, hi = a.nseg;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (wg >= a.wg0[mid]) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ inline long head_elems(const void* p, long n) {
  const long h = (long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
  return h < n ? h : n;
}

__global__ __launch_bounds__(kBlock) void grad_sumsq_kernel(SegArgs a, double* __restrict__ partials) {
  __shared__ double lds[kBlock / 64];
  const int wg = blockIdx.x, s = find_seg(a, wg);
  const float* __restrict__ g = a.seg[s].g;
  const long n = a.seg[s].n;
  const int nwg = a.wg0[s + 1] - a.wg0[s], w = wg - a.wg0[s];
  const long head = head_elems(g, n), nvec = (n - head) >> 2, tail0 = head + (nvec << 2);
  const float4* __restrict__ gv = reinterpret_cast<const float4*>(g + head);
  double acc = 0.0;
  for (long i = (long)w * kBlock + threadIdx.x; i < nvec; i += (long)nwg * kBlock) {
    const float4 x = gv[i];
    acc += (double)x.x * x.x + (double)x.y * x.y + (double)x.z * x.z + (double)x.w * x.w;
  }
  if (w == 0) {                                     // at most three elements on either side
    if ((long)threadIdx.x < head) acc += (double)g[threadIdx.x] * g[threadIdx.x];
    const long t = tail0 + threadIdx.x;
    if (t < n) acc += (double)g[t] * g[t];
  }
  const double total = ufr::dev::block_sum<kBlock>(acc, lds);   // lane tree inside a wave, then the waves in ascending order
  if (threadIdx.x == 0) partials[wg] = total;
}

__global__ __launch_bounds__(kBlock) void grad_norm_finalize_kernel(const double* __restrict__ partials, long np, float max_norm,
                                                                    float* __restrict__ norm_out) {
  __shared__ double lds[kBlock];
  const long per = (np + kBlock - 1) / kBlock, lo = per * threadIdx.x, hi = lo + per < np ? lo + per : np;
  double acc = 0.0;
  for (long i = lo; i < hi; ++i) acc += partials[i];          // ascending inside a thread's range
  lds[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int i = 0; i < kBlock; ++i) total += lds[i];          // and the ranges in ascending order
    const double norm = sqrt(total);
    const double coef = (double)max_norm / (norm + 1e-6);
    norm_out[0] = (float)norm;
    norm_out[1] = coef > 1.0 ? 1.0f : (float)coef;             // a NaN stays a NaN, as torch.clamp(max=1) leaves it
  }
}

__device__ inline void adamw_one(float& p, float g, float& m, float& v, const StepConsts& k, double coef) {
  const double gp = coef * (double)g;
  const float mn = (float)(k.b1 * (double)m + k.omb1 * gp);
  const float vn = (float)(k.b2 * (double)v + k.omb2 * (gp * gp));
  const float denom = sqrtf(vn) / k.bc2_sqrt + k.eps;
  const float q = mn / denom;
  p = (float)((double)p * k.decay - (double)k.step_size * (double)q);
  m = mn;
  v = vn;
}

__global__ __launch_bounds__(kBlock) void adamw_step_kernel(SegArgs a, StepConsts k, const float* __restrict__ norm) {
  const int wg = blockIdx.x, s = find_seg(a, wg);
  float* __restrict__ p = a.seg[s].p;
  const float* __restrict__ g = a.seg[s].g;
  float* __restrict__ m = a.seg[s].m;
  float* __restrict__ v = a.seg[s].v;
  const long n = a.seg[s].n;
  const int nwg = a.wg0[s + 1] - a.wg0[s], w = wg - a.wg0[s];
  const double coef = norm ? (double)norm[1] : 1.0;
  const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u);
  const bool same = mis == (unsigned)(reinterpret_cast<uintptr_t>(g) & 15u) && mis == (unsigned)(reinterpret_cast<uintptr_t>(m) & 15u) &&
                    mis == (unsigned)(reinterpret_cast<uintptr_t>(v) & 15u);
  if (!same) {                                      // the pointers disagree about where a 16-byte line starts: one element at a time
    for (long i = (long)w * kBlock + threadIdx.x; i < n; i += (long)nwg * kBlock) {
      float pi = p[i], mi = m[i], vi = v[i];
      adamw_one(pi, g[i], mi, vi, k, coef);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
    return;
  }
  const long head = head_elems(p, n), nvec = (n - head) >> 2, tail0 = head + (nvec << 2);
  float4* __restrict__ pv = reinterpret_cast<float4*>(p + head);
  const float4* __restrict__ gv = reinterpret_cast<const float4*>(g + head);
  float4* __restrict__ mv = reinterpret_cast<float4*>(m + head);
  float4* __restrict__ vv = reinterpret_cast<float4*>(v + head);
  for (long i = (long)w * kBlock + threadIdx.x; i < nvec; i += (long)nwg * kBlock) {
    float4 pi = pv[i], mi = mv[i], vi = vv[i];
    const float4 gi = gv[i];
    adamw_one(pi.x, gi.x, mi.x, vi.x, k, coef);
    adamw_one(pi.y, gi.y, mi.y, vi.y, k, coef);
    adamw_one(pi.z, gi.z, mi.z, vi.z, k, coef);
    adamw_one(pi.w, gi.w, mi.w, vi.w, k, coef);
    pv[i] = pi; mv[i] = mi; vv[i] = vi;
  }
  if (w == 0) {
    long i = -1;
    if ((long)threadIdx.x < head) i = threadIdx.x;
    else if (tail0 + ((long)threadIdx.x - head) < n && (long)threadIdx.x - head < 4) i = tail0 + ((long)threadIdx.x - head);
    if (i >= 0) {
      float pi = p[i], mi = m[i], vi = v[i];
      adamw_one(pi, g[i], mi, vi, k, coef);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
  }
}

int check_segs(const char* what, const ufr_adamw_seg* segs, int nseg, bool all_pointers) {
  UFR_REQUIRE(nseg >= 0, "%s: nseg = %d is negative", what, nseg);
  UFR_REQUIRE(nseg == 0 || segs, "%s: null segment array with nseg = %d", what, nseg);
  for (int i = 0; i < nseg; ++i) {
    UFR_REQUIRE(segs[i].n >= 0, "%s: segment %d has n = %ld < 0", what, i, segs[i].n);
    if (segs[i].n == 0) continue;
    UFR_REQUIRE(segs[i].g && (!all_pointers || (segs[i].p && segs[i].m && segs[i].v)), "%s: segment %d has a null pointer with n = %ld",
                what, i, segs[i].n);
  }
  return UFR_OK;
}

// the next launch's worth of non-empty segments from segs[*next ..]; false when none are left
bool pack(const ufr_adamw_seg* segs, int nseg, int* next, SegArgs* a) {
  a->nseg = 0;
  a->wg0[0] = 0;
  while (*next < nseg && a->nseg < kSegs) {
    const ufr_adamw_seg& s = segs[(*next)++];
    if (s.n == 0) continue;
    a->seg[a->nseg] = s;
    a->wg0[a->nseg + 1] = a->wg0[a->nseg] + seg_workgroups(s.n);
    ++a->nseg;
  }
  return a->nseg > 0;
}

}  // namespace

extern "C" long ufr_grad_norm_partials(const ufr_adamw_seg* segs, int nseg) {
  if (nseg < 0 || (nseg > 0 && !segs)) return -1;
  long total = 0;
  for (int i = 0; i < nseg; ++i) {
    if (segs[i].n < 0) return -1;
    if (segs[i].n > 0) total += seg_workgroups(segs[i].n);
  }
  return total;
}

extern "C" int ufr_grad_norm(const ufr_adamw_seg* segs, int nseg, float max_norm, double* partials, long partial_elems,
                             float* norm_out, ufr_stream_t stream) {
  const int rc = check_segs("grad norm", segs, nseg, false);
  if (rc != UFR_OK) return rc;
  if (nseg == 0) return UFR_OK;
  UFR_REQUIRE(norm_out, "grad norm: null pointer (norm_out)");
  const long need = ufr_grad_norm_partials(segs, nseg);
  UFR_REQUIRE(partials || need == 0, "grad norm: null pointer (partials), %ld values are needed", need);
  UFR_REQUIRE(partial_elems >= need, "grad norm: partials holds %ld values, %ld are needed (one per workgroup)", partial_elems, need);
  hipStream_t st = ufr::as_stream(stream);
  SegArgs a;
  int next = 0;
  long done = 0;
  while (pack(segs, nseg, &next, &a)) {
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(a.wg0[a.nseg]), dim3(kBlock), 0, st, a, partials + done);
    const int lrc = ufr::launched("grad_sumsq_kernel");
    if (lrc != UFR_OK) return lrc;
    done += a.wg0[a.nseg];
  }
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(kBlock), 0, st, partials, done, max_norm, norm_out);
  return ufr::launched("grad_norm_finalize_kernel");
}

extern "C" int ufr_adamw_step(const ufr_adamw_seg* segs, int nseg, const ufr_adamw_hyper* h, const float* norm, ufr_stream_t stream) {
  const int rc = check_segs("adamw step", segs, nseg, true);
  if (rc != UFR_OK) return rc;
  UFR_REQUIRE(h, "adamw step: null pointer (hyperparameters)");
  UFR_REQUIRE(h->lr >= 0.0, "adamw step: lr = %g is negative", h->lr);
  UFR_REQUIRE(h->beta1 >= 0.0 && h->beta1 < 1.0, "adamw step: beta1 = %g is outside [0, 1)", h->beta1);
  UFR_REQUIRE(h->beta2 >= 0.0 && h->beta2 < 1.0, "adamw step: beta2 = %g is outside [0, 1)", h->beta2);
  UFR_REQUIRE(h->eps >= 0.0, "adamw step: eps = %g is negative", h->eps);
  UFR_REQUIRE(h->weight_decay >= 0.0, "adamw step: weight_decay = %g is negative", h->weight_decay);
  UFR_REQUIRE(h->bias1 > 0.0 && h->bias1 <= 1.0 && h->bias2 > 0.0 && h->bias2 <= 1.0,
              "adamw step: bias corrections (%g, %g) are outside (0, 1]", h->bias1, h->bias2);
  if (nseg == 0) return UFR_OK;
  StepConsts k;
  k.decay = 1.0 - h->lr * h->weight_decay;
  k.b1 = h->beta1; k.omb1 = 1.0 - h->beta1;
  k.b2 = h->beta2; k.omb2 = 1.0 - h->beta2;
  k.step_size = (float)(h->lr / h->bias1);
  k.bc2_sqrt = (float)sqrt(h->bias2);
  k.eps = (float)h->eps;
  hipStream_t st = ufr::as_stream(stream);
  SegArgs a;
  int next = 0;
  while (pack(segs, nseg, &next, &a)) {
    hipLaunchKernelGGL(adamw_step_kernel, dim3(a.wg0[a.nseg]), dim3(kBlock), 0, st, a, k, norm);
    const int lrc = ufr::launched("adamw_step_kernel");
    if (lrc != UFR_OK) return lrc;
  }
  return UFR_OK;
}
