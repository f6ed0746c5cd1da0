// raft_context_head.hip -- the context head of a RAFT without a separate context network (models/raft/raft.py:169-175):
//     cnet = conv_redir(fmap1);  net, inp = split(cnet, [hdim, cdim]);  net = tanh(net);  inp = relu(inp)
// as ONE kernel each way instead of four torch operators and two copies (the split's halves are strided views of cnet: the
// refinement engine wants both contiguous):
//     forward    ctx [B, Ct + Cr, HW]  ->  net [B, Ct, HW] = tanh(ctx[:, :Ct]),  inp [B, Cr, HW] = max(ctx[:, Ct:], 0)
//     backward   g_ctx [B, Ct + Cr, HW] = [ g_net * (1 - net * net) | g_inp where inp > 0, else 0 ]     (a NULL gradient = zeros)
// Streaming, one element of ctx per work item, blockIdx.y = the image: 16 bytes per lane when HW is a multiple of 4 and every tensor is 16-byte aligned
// (a channel row then starts on a float4 boundary, so a float4 never straddles the tanh | relu seam), one float per lane
// otherwise.  At one pair of 384 x 1280 frames (B = 1, 256 channels, HW = 48 * 160) that is 1920 workgroups of 256 lanes over
// 7.9 MB in and 7.9 MB out: 5.2 us forward, 6.7 us backward inside an attack iteration (3.0 / 3.5 TB/s); 8 pairs stream at the
// HBM roof (profiles/r8_raft_fnc_iteration_kernels.md).  tanhf is csrc/gru.hip's; 1 - t * t stays two roundings (-ffp-contract=off), torch's tanh_backward.
#include "ufr_common.h"

namespace {

// one float (V = float) or four (V = float4) per work item
template <typename V> struct Lanes;
template <> struct Lanes<float> {
  static constexpr int n = 1;
  __device__ static float get(const float& v, int) { return v; }
  __device__ static void set(float& v, int, float x) { v = x; }
};
template <> struct Lanes<float4> {
  static constexpr int n = 4;
  __device__ static float get(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
  __device__ static void set(float4& v, int k, float x) { (k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w) = x; }
};

// nt / nr: work items (of V) of one image's tanh half / relu half; blockIdx.y = the image (no division per item), the x
// dimension strides over the image's nt + nr items
template <typename V>
__global__ __launch_bounds__(256) void raft_context_split_fwd_kernel(const V* __restrict__ ctx, V* __restrict__ net, V* __restrict__ inp,
                                                                     long nt, long nr) {
  const long b = blockIdx.y;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nt + nr; e += (long)gridDim.x * blockDim.x) {
    const V v = ctx[b * (nt + nr) + e];
    V o;
    if (e < nt) {
#pragma unroll
      for (int k = 0; k < Lanes<V>::n; ++k) Lanes<V>::set(o, k, tanhf(Lanes<V>::get(v, k)));
      net[b * nt + e] = o;
    } else {
#pragma unroll
      for (int k = 0; k < Lanes<V>::n; ++k) {
        const float x = Lanes<V>::get(v, k);
        Lanes<V>::set(o, k, x < 0.0f ? 0.0f : x);              // (a NaN stays a NaN, like torch.relu)
      }
      inp[b * nr + (e - nt)] = o;
    }
  }
}

template <typename V>
__global__ __launch_bounds__(256) void raft_context_split_bwd_kernel(const V* __restrict__ net, const V* __restrict__ inp,
                                                                     const V* __restrict__ g_net, const V* __restrict__ g_inp,
                                                                     V* __restrict__ g_ctx, long nt, long nr) {
  const long b = blockIdx.y;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nt + nr; e += (long)gridDim.x * blockDim.x) {
    V o;
    if (e < nt) {
      if (g_net) {
        const V t = net[b * nt + e], g = g_net[b * nt + e];
#pragma unroll
        for (int k = 0; k < Lanes<V>::n; ++k) {
          const float tk = Lanes<V>::get(t, k);
          Lanes<V>::set(o, k, Lanes<V>::get(g, k) * (1.0f - tk * tk));
        }
      } else {
#pragma unroll
        for (int k = 0; k < Lanes<V>::n; ++k) Lanes<V>::set(o, k, 0.0f);
      }
    } else {
      if (g_inp) {
        const V y = inp[b * nr + (e - nt)], g = g_inp[b * nr + (e - nt)];
#pragma unroll
        for (int k = 0; k < Lanes<V>::n; ++k) Lanes<V>::set(o, k, Lanes<V>::get(y, k) > 0.0f ? Lanes<V>::get(g, k) : 0.0f);
      } else {
#pragma unroll
        for (int k = 0; k < Lanes<V>::n; ++k) Lanes<V>::set(o, k, 0.0f);
      }
    }
    g_ctx[b * (nt + nr) + e] = o;
  }
}

using ufr::aligned16;

}  // namespace

extern "C" int ufr_raft_context_split_forward(const float* ctx, float* net, float* inp, int B, int Ct, int Cr, long HW,
                                              ufr_stream_t stream) {
  UFR_REQUIRE(ctx && net && inp, "raft context split: null pointer");
  UFR_REQUIRE(B > 0 && B < 65536 && Ct > 0 && Cr > 0 && HW > 0, "raft context split: bad shape");
  const long nt = (long)Ct * HW, nr = (long)Cr * HW;
  if (HW % 4 == 0 && aligned16(ctx, net, inp)) {
    raft_context_split_fwd_kernel<float4><<<dim3(ufr::stream_grid((nt + nr) / 4, 256), B), 256, 0, ufr::as_stream(stream)>>>(
        reinterpret_cast<const float4*>(ctx), reinterpret_cast<float4*>(net), reinterpret_cast<float4*>(inp), nt / 4, nr / 4);
  } else {
    raft_context_split_fwd_kernel<float><<<dim3(ufr::stream_grid(nt + nr, 256), B), 256, 0, ufr::as_stream(stream)>>>(ctx, net, inp, nt, nr);
  }
  return ufr::launched("raft_context_split_fwd_kernel");
}

extern "C" int ufr_raft_context_split_backward(const float* net, const float* inp, const float* g_net, const float* g_inp, float* g_ctx,
                                               int B, int Ct, int Cr, long HW, ufr_stream_t stream) {
  UFR_REQUIRE(net && inp && g_ctx, "raft context split backward: null pointer");
  UFR_REQUIRE(B > 0 && B < 65536 && Ct > 0 && Cr > 0 && HW > 0, "raft context split backward: bad shape");
  const long nt = (long)Ct * HW, nr = (long)Cr * HW;
  if (HW % 4 == 0 && aligned16(net, inp, g_net, g_inp, g_ctx)) {
    raft_context_split_bwd_kernel<float4><<<dim3(ufr::stream_grid((nt + nr) / 4, 256), B), 256, 0, ufr::as_stream(stream)>>>(
        reinterpret_cast<const float4*>(net), reinterpret_cast<const float4*>(inp), reinterpret_cast<const float4*>(g_net),
        reinterpret_cast<const float4*>(g_inp), reinterpret_cast<float4*>(g_ctx), nt / 4, nr / 4);
  } else {
    raft_context_split_bwd_kernel<float><<<dim3(ufr::stream_grid(nt + nr, 256), B), 256, 0, ufr::as_stream(stream)>>>(net, inp, g_net, g_inp,
                                                                                                                     g_ctx, nt, nr);
  }
  return ufr::launched("raft_context_split_bwd_kernel");
}
