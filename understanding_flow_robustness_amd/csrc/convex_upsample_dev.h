// convex_upsample_dev.h -- the per-element arithmetic of RAFT's convex upsampling (models/raft/raft.py:111-122), once: the softmax over
// the 9 mask channels of one sub-pixel and the 8x flow at the 3x3 coarse neighbours.  convex_upsample.hip (upsample_flow and its
// adjoint) and raft_train_loss.hip (the upsampling fused into the sequence loss) both build `up` from these two, followed by the same
// fmaf chain, so their results are bit-equal.
#pragma once
#include "ufr_common.h"

namespace ufr {
namespace dev {

__device__ __forceinline__ void softmax9(const float* __restrict__ m, size_t stride, float* s) {
  float mx = m[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) mx = fmaxf(mx, m[k * stride]);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) { s[k] = expf(m[k * stride] - mx); sum += s[k]; }
  const float inv = 1.0f / sum;
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] *= inv;
}

// 8 * flow at the 3x3 neighbours (zero padding, like F.unfold(padding=1))
__device__ __forceinline__ void neighbours(const float* __restrict__ flow_nc, int h, int w, int H, int W, float* f) {
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int hh = h + k / 3 - 1, ww = w + k % 3 - 1;
    f[k] = (hh >= 0 && hh < H && ww >= 0 && ww < W) ? 8.0f * flow_nc[hh * W + ww] : 0.f;
  }
}

}  // namespace dev
}  // namespace ufr
