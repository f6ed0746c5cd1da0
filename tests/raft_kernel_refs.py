"""Plain torch restatements of what csrc/raft_update.hip and csrc/raft_norm.hip compute, on the engine's chunk-major layout
(activation planes bf16 [3][chunks][M][32], float32 tensors [chunks][M][32], M = B*H*W pixels in (image, y, x) order).  They
take and return ordinary tensors and compute in the dtype they are given: float64 for the gate arithmetic and the norm (the
truth the kernels are judged against; called with float32 tensors they are the float32 torch spelling the kernels' error is
measured by), float32 for everything a kernel must match bit for bit.  tests/test_raft_update_ref_cpu.py proves them against
F.conv2d, F.instance_norm, the SepConvGRU half-step and torch.autograd without a device."""
import ctypes

import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------------------------------- layout
def to_cm(x):
    """[B, C, H, W] (C a multiple of 32) -> chunk-major [C / 32][B*H*W][32]."""
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C // 32, 32).permute(1, 0, 2).contiguous()


def from_cm(t, B, H, W):
    """chunk-major [chunks][B*H*W][32] -> [B, chunks * 32, H, W]."""
    chunks = t.shape[0]
    return t.permute(1, 0, 2).reshape(B, H, W, chunks * 32).permute(0, 3, 1, 2).contiguous()


def split3(v):
    """float32 [...] -> bf16 [3, ...] with (p0 + p1) + p2 == v exactly (round to nearest even at every step): the kernels'
    store_planes8, the arithmetic of igemm._split3 keeping the shape."""
    v = v.float()
    p0 = v.to(torch.bfloat16)
    r1 = v - p0.float()
    p1 = r1.to(torch.bfloat16)
    p2 = (r1 - p1.float()).to(torch.bfloat16)
    return torch.stack((p0, p1, p2))


def merge3(p):
    """bf16 [3, ...] -> float32, added in the kernels' order (load_planes8)."""
    return (p[0].float() + p[1].float()) + p[2].float()


# ---------------------------------------------------------------------------------------------------- bit-exact group
def flow_patches(flow):
    """flow [B, 2, H, W] -> chunk-major [4][M][32]: channel k = tap * 2 + ch, tap = ky * 7 + kx holds flow[b, ch, y + ky - 3,
    x + kx - 3] (0 outside the frame), k < 98; channels 98..127 are zero.  A pure gather: exact in any dtype."""
    B, _, H, W = flow.shape
    cols = F.unfold(flow, 7, padding=3).view(B, 2, 49, H * W)           # [b][ch][tap][pixel]
    k98 = cols.permute(0, 3, 2, 1).reshape(B * H * W, 98)
    out = flow.new_zeros(B * H * W, 128)
    out[:, :98] = k98
    return out.view(B * H * W, 4, 32).permute(1, 0, 2).contiguous()


def convf1_weight_as_matrix(w):
    """Conv2d(2, N, 7, padding=3) weight [N, 2, 7, 7] -> [128, N] with row k = tap * 2 + ch (rows 98..127 zero):
    conv2d(flow, w) at a pixel is its 128 patch channels times this matrix."""
    N = w.shape[0]
    m = w.new_zeros(128, N)
    m[:98] = w.permute(2, 3, 1, 0).reshape(98, N)
    return m


def flow_rows(flow):
    """flow [B, 2, H, W] -> [M, 2]."""
    return flow.permute(0, 2, 3, 1).reshape(-1, 2)


def slab_sum(slabs):
    """[S][M][Npad] float32 -> [M][Npad]: from zeros, the slabs added in ascending order, in float32."""
    v = torch.zeros_like(slabs[0])
    for s in range(slabs.shape[0]):
        v = v + slabs[s]
    return v


def slab_preact(slabs, bias, addend, col0, nch):
    """The pre-activation the gate kernels read from a split-K launch's raw slabs [S][M][Npad]: columns col0 .. col0 + nch * 32 as
    a chunk-major float32 [nch][M][32], in this order of float32 additions: zeros, + slab 0, + slab 1, ..., + addend (chunk-major
    [nch][M][32] or None), + bias[column]."""
    M = slabs.shape[1]
    v = slab_sum(slabs)[:, col0:col0 + nch * 32].reshape(M, nch, 32).permute(1, 0, 2).contiguous()
    if addend is not None:
        v = v + addend
    return v + bias[col0:col0 + nch * 32].view(nch, 1, 32)


def leaky(v, slope):
    return torch.where(v > 0, v, v * slope)


def motion_finish_slabs(slabs, bias, N, slope, flow):
    """-> float32 chunk-major [4][M][32]: leaky(slab sum + bias) in columns < N, zeros in N..125, the flow in 126, 127."""
    M = slabs.shape[1]
    v = slab_sum(slabs)
    b = torch.zeros(128, dtype=torch.float32, device=slabs.device)
    b[:N] = bias[:N]
    v = leaky(v + b, torch.tensor(slope, dtype=torch.float32, device=slabs.device))
    v[:, N:] = 0.0
    v[:, 126:128] = flow_rows(flow)
    return v.view(M, 4, 32).permute(1, 0, 2).contiguous()


def coords_step(coords1, delta, coords0):
    """-> (coords1 after the step, the saved copy, flow)."""
    c = coords1 + delta if delta is not None else coords1.clone()
    return c, c.clone(), c - coords0


def grad_finalize(g, mask, slope):
    """g * LeakyReLU'(mask): g where mask > 0, g * slope elsewhere (float32)."""
    return torch.where(mask > 0, g, g * torch.tensor(slope, dtype=g.dtype, device=g.device))


# ---------------------------------------------------------------------------------------------------- SepConvGRU half-step
def gates_forward(zr_pre, h):
    """zr_pre [2 chunks][M][32] = [z | r] pre-activations, h [chunks][M][32] -> (sigmoid values [2 chunks][M][32], r * h)."""
    c = h.shape[0]
    zr = torch.sigmoid(zr_pre)
    return zr, zr[c:] * h


def blend_forward(q_pre, z, h):
    """-> (tanh values, (1 - z) h + z q)."""
    q = torch.tanh(q_pre)
    return q, (1 - z) * h + z * q


def blend_backward(q, z, h, g, acc=None):
    """q = tanh values, z = sigmoid values, g = d/d h'.  -> (g_q_pre, g_z, g_h, acc + g_q_pre or None)."""
    gq = g * z * (1 - q * q)
    return gq, g * q - g * h, g * (1 - z), (acc + gq if acc is not None else None)


def gates_backward(zr, h, g_z, g_rh, g_h, acc=None, consume=False):
    """zr = sigmoid values [z | r].  -> (g_zr_pre [2 chunks] = [g_z z (1 - z) | g_rh h r (1 - r)], g_h + g_rh r,
    acc + g_zr_pre or None, g_rh as it is left behind)."""
    c = h.shape[0]
    z, r = zr[:c], zr[c:]
    gzr = torch.cat((g_z * ((1 - z) * z), (g_rh * h) * ((1 - r) * r)))
    return gzr, g_h + g_rh * r, (acc + gzr if acc is not None else None), (torch.zeros_like(g_rh) if consume else g_rh)


# ---------------------------------------------------------------------------------------------------- instance norm
def _per_image(t, n):
    chunks, M, _ = t.shape
    return t.view(chunks, n, M // n, 32)


def _bcast(s):
    """[n][C] -> [chunks][n][1][32]."""
    n, C = s.shape
    return s.view(n, C // 32, 32).permute(1, 0, 2).unsqueeze(2)


def norm_stats(x, n, eps):
    """x chunk-major [chunks][n*HW][32] -> (mean [n][C], 1 / sqrt(biased variance + eps) [n][C]), two passes."""
    xi = _per_image(x, n)
    mean = xi.mean(2, keepdim=True)
    var = ((xi - mean) ** 2).mean(2, keepdim=True)
    flat = lambda s: s.squeeze(2).permute(1, 0, 2).reshape(n, -1)
    return flat(mean), flat(1.0 / torch.sqrt(var + eps))


def norm_xhat(x, n, mean=None, rstd=None):
    if mean is None:
        return x
    return ((_per_image(x, n) - _bcast(mean)) * _bcast(rstd)).reshape(x.shape)


def norm_forward(x, n, mean=None, rstd=None, res=None, relu1=True, relu2=True):
    """relu2(res + relu1((x - mean) * rstd)); mean = None: the folded-BatchNorm form (mean 0, rstd 1)."""
    v = norm_xhat(x, n, mean, rstd)
    if relu1:
        v = torch.relu(v)
    if res is not None:
        v = v + res
    if relu2:
        v = torch.relu(v)
    return v


def norm_backward(x, G, n, mean=None, rstd=None, outmask=None, relu1=True, pos=None):
    """g = G [outmask > 0] [xhat > 0 if relu1];  gz = rstd (g - mean_HW g - xhat mean_HW(g xhat)), and the two means [n][C] each;
    mean = None: gz = g, no statistics terms.  `pos` overrides [xhat > 0] (a mask taken from a kernel's own float32 xhat)."""
    xh = norm_xhat(x, n, mean, rstd)
    g = G
    if outmask is not None:
        g = g * (outmask > 0)
    if relu1:
        g = g * (pos if pos is not None else (xh > 0))
    if mean is None:
        return g, None, None
    gi, xi = _per_image(g, n), _per_image(xh, n)
    s0, s1 = gi.mean(2, keepdim=True), (gi * xi).mean(2, keepdim=True)
    gz = (_bcast(rstd) * (gi - s0 - xi * s1)).reshape(x.shape)
    flat = lambda s: s.squeeze(2).permute(1, 0, 2).reshape(n, -1)
    return gz, flat(s0), flat(s1)


# ---------------------------------------------------------------------------------------------------- device buffers of the GPU tests
DEV = "cuda:0"
SENT = 7.0
GUARD = 64                                       # float32 elements of sentinel on both sides of a float32 buffer (keeps 256-byte alignment)
LAUNCH_THREADS = 2048 * 256


def device_lib():
    from understanding_flow_robustness_amd import _lib as L
    return L, L.lib()


class F32:
    """A float32 device buffer between two sentinel guards."""

    def __init__(self, value=None, shape=None):
        shape = tuple(value.shape) if value is not None else tuple(shape)
        n = 1
        for s in shape:
            n *= s
        self.raw = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=DEV)
        self.t = self.raw[GUARD:GUARD + n].view(shape)
        if value is not None:
            self.t.copy_(value)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def guards_hold(self):
        return bool((self.raw[:GUARD] == SENT).all()) and bool((self.raw[-GUARD:] == SENT).all())


class PlaneBuf:
    """bf16 planes [3][total chunks][M][32] full of the sentinel; `own` = the chunk range the call under test may write."""

    def __init__(self, total, M, chunk0=0, values=None):
        self.t = torch.full((3, total, M, 32), SENT, dtype=torch.bfloat16, device=DEV)
        self.stride, self.chunk0, self.M = total * M * 32, chunk0, M
        if values is not None:
            self.t[:, chunk0:chunk0 + values.shape[0]] = split3(values)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def chunk_ptr(self, chunk):
        return ctypes.c_void_p(self.t.data_ptr() + chunk * self.M * 32 * 2)

    def own(self, n):
        return self.t[:, self.chunk0:self.chunk0 + n]

    def values(self, n):
        return merge3(self.own(n))

    def rest_holds(self, n):
        return bool((self.t[:, :self.chunk0] == SENT).all()) and bool((self.t[:, self.chunk0 + n:] == SENT).all())


def device_rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _rel(a, ref64):
    return float((a.double() - ref64).abs().max()) / max(float(ref64.abs().max()), 1e-300)


class Gate:
    """Collects (output, kernel error, torch float32 error) against float64, prints every figure, then asserts them all."""

    def __init__(self, what):
        self.what, self.rows = what, []

    def add(self, name, kernel, torch32, ref64):
        assert kernel.shape == ref64.shape == torch32.shape
        ek, et = _rel(kernel, ref64), _rel(torch32, ref64)
        print(f"raft_update_kernel_errors {self.what} {name}: kernel {ek:.3e}, torch float32 {et:.3e} (max-norm, of max |float64|)")
        self.rows.append((name, ek, et))

    def check(self):
        bad = [(n, ek, et) for n, ek, et in self.rows if not ek <= 3 * et]
        assert not bad, f"{self.what}: beyond three times the float32 torch error: {bad}"
