"""fp32 parity mode of the dense operators on the hand-written matrix-core kernels: split-bf16 products.

The golden-vector tests (and `bench.py --precision fp32`) run fp32 tensors, for which the 16-bit MFMA kernels have no
direct variant; until round 3 those calls went to the ROCm libraries (hipBLASLt / MIOpen / fused SDPA behind F.linear,
F.conv2d, scaled_dot_product_attention).  Here an fp32 operand is split into two bf16 terms, x = hi + lo with
hi = bf16(x), lo = bf16(x - hi) (16 significand bits, fp32's exponent range), and a product x.y is evaluated as
hi.hi' + hi.lo' + lo.hi' -- three bf16 MFMA products accumulated in fp32 INSIDE ONE launch by concatenating the terms
along the reduction index:
    Linear / conv forward, data gradient   [xh | xh | xl] . [wh | wl | wh]^T      (K -> 3K; conv: channels -> 3C per tap)
    weight gradient                        [gh ; gh ; gl]^T . [xh ; xl ; xh]      (rows T -> 3T; conv: batch -> 3B)
on csrc/mfma_gemm.hip's kernels with an fp32-result epilogue (rfn_gemm_nt_o32 / rfn_conv2d_nhwc_o32; the weight-gradient
kernel's result is fp32 anyway).  The dropped lo.lo' term and the second rounding leave ~2^-16 relative error per product
(fp32: 2^-24): far inside the 1e-3 parity bar of the goldens.  Three times the MFMA work of the 16-bit path; the operand
splits are one launch each (csrc/split3.hip), and attention runs on the fp32 matrix pipe itself (csrc/attn32.hip).
"""
import torch

from . import _lib, mfma
from ._tensor import ptr
from .params import derived

ENABLED = True
BF = torch.bfloat16


def usable(*ts):
    return ENABLED and mfma.ENABLED and all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in ts)


def split2(x):
    hi = x.to(BF)
    return hi, (x - hi.float()).to(BF)


_ORDER = {"hhl": 0, "hlh": 1}


def split3(x2, order, Kp, stack=False):
    """(rows, K) fp32, unit column stride -> the three bf16 terms `order` of its (hi, lo) split in ONE launch (csrc/split3.hip):
    side by side as (rows, 3 Kp), or stacked as (3 rows, Kp); columns K .. Kp - 1 are zero."""
    rows, K = x2.shape
    if x2.stride(1) != 1 or x2.stride(0) < K:
        x2 = x2.contiguous()
    out = torch.empty((3 * rows, Kp) if stack else (rows, 3 * Kp), dtype=BF, device=x2.device)
    _lib.call("rfn_split3_bf16", x2.device, ptr(x2), x2.stride(0), ptr(out), out.stride(0), rows * Kp if stack else Kp, rows, K,
              Kp, _ORDER[order])
    return out


def _cat_k(x, order, pad_to=64):
    """(rows, K) fp32 -> (rows, 3 Kp) bf16 = terms `order` of (hi, lo) side by side, each zero-padded to Kp = roundup(K, pad_to)."""
    return split3(x, order, -(-x.shape[1] // pad_to) * pad_to)


def gemm_nt(x, w, bias=None, res=None, act=0):
    """fp32 y[M, N] = res + act(x[M, K] @ w[N, K]^T + bias) through three bf16 products in one launch."""
    M, K = x.shape
    N = w.shape[0]
    Np = -(-N // 8) * 8
    x3 = _cat_k(x, "hhl")
    w3 = _cat_k(w, "hlh")
    if Np != N:
        w3 = torch.cat([w3, w3.new_zeros((Np - N, w3.shape[1]))])
        if bias is not None:
            bias = torch.cat([bias, bias.new_zeros(Np - N)])
    y = torch.empty((M, Np), dtype=torch.float32, device=x.device)
    if res is not None and Np != N:
        res = torch.nn.functional.pad(res, (0, Np - N))
    _lib.call("rfn_gemm_nt_o32", x.device, ptr(x3), ptr(w3), ptr(None if bias is None else bias.contiguous()),
              ptr(None if res is None else res.contiguous()), None, 0, int(act), ptr(y), M, Np, x3.shape[1], x3.stride(0),
              w3.stride(0), y.stride(0))
    return y if Np == N else y[:, :N]


def gemm_tn(g, x):
    """fp32 (N, K) = g[T, N]^T @ x[T, K]: the three products stacked along T on the split-T weight-gradient kernel."""
    N, K = g.shape[1], x.shape[1]
    g3 = split3(g, "hhl", -(-N // 64) * 64, stack=True)              # [gh ; gh ; gl]
    x3 = split3(x, "hlh", -(-K // 64) * 64, stack=True)              # [xh ; xl ; xh]
    part = mfma.gemm_tn(g3, x3)
    if part is None:
        raise RuntimeError("split32.gemm_tn: outside the weight-gradient kernel's domain")
    return part.sum(0)[:N, :K]


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        x2 = x.reshape(-1, x.shape[-1])
        ctx.save_for_backward(x2, weight)
        ctx.has_bias, ctx.xshape = bias is not None, x.shape
        return gemm_nt(x2, weight.view(weight.shape[0], -1), bias).view(x.shape[:-1] + (weight.shape[0],))

    @staticmethod
    def backward(ctx, gy):
        x2, weight = ctx.saved_tensors
        w2 = weight.view(weight.shape[0], -1)
        g2 = gy.reshape(-1, w2.shape[0]).float()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = gemm_nt(g2, w2.t().contiguous()).view(ctx.xshape)
        if ctx.needs_input_grad[1]:
            gw = gemm_tn(g2, x2).reshape(weight.shape)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = g2.sum(0)
        return gx, gw, gb


def linear(x, weight, bias=None):
    """F.linear for fp32 HIP tensors on the hand-written kernels (forward, input / weight / bias gradients)."""
    return _LinearFn.apply(x, weight, bias)


def matmul_nt(a, b):
    """a[M, K] @ b[N, K]^T with autograd (attention's two products)."""
    return _LinearFn.apply(a, b, None)


class _Attn32Fn(torch.autograd.Function):
    """softmax(scale q k^T) v per head of 64 on the fp32 matrix pipe (csrc/attn32.hip): one launch forward, two backward."""

    @staticmethod
    def forward(ctx, q, kv, heads, scale):
        B, N, C = q.shape
        Nkv = kv.shape[1]
        nqpad = -(-N // 128) * 128
        o = torch.empty_like(q)
        lse2 = torch.empty((B * heads, nqpad), dtype=torch.float32, device=q.device)
        _lib.call("rfn_attn32_fwd", q.device, ptr(q), q.stride(0), q.stride(1), ptr(kv), kv.stride(0), kv.stride(1), ptr(o),
                  o.stride(0), o.stride(1), ptr(lse2), B, heads, C // heads, N, Nkv, nqpad, float(scale))
        if q.requires_grad or kv.requires_grad:
            ctx.save_for_backward(q, kv, o, lse2)
            ctx.heads, ctx.scale = heads, scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, kv, o, lse2 = ctx.saved_tensors
        heads, scale = ctx.heads, ctx.scale
        B, N, C = q.shape
        Nkv = kv.shape[1]
        do = do.float()
        if do.stride() != o.stride():
            do = do.contiguous()
        dq = torch.empty_like(q)
        delta = torch.empty_like(lse2)
        # enough (key tile, query chunk) workgroups for 256 CUs; the chunks of a key tile add their partial sums with atomics
        tiles = -(-Nkv // 128) * B * heads
        chunks = max(1, min(-(-N // 32), -(-1024 // tiles)))
        dkv = (torch.zeros_like if chunks > 1 else torch.empty_like)(kv)
        _lib.call("rfn_attn32_bwd", q.device, ptr(q), q.stride(0), q.stride(1), ptr(kv), kv.stride(0), kv.stride(1), ptr(do),
                  ptr(o), o.stride(0), o.stride(1), ptr(lse2), ptr(delta), ptr(dq), dq.stride(0), dq.stride(1), ptr(dkv),
                  dkv.stride(0), dkv.stride(1), B, heads, C // heads, N, Nkv, lse2.shape[1], chunks, float(scale))
        return dq, dkv, None, None


def attention(q, kv, heads, scale):
    """q: (B, N, heads * D) fp32, kv: (B, Nkv, 2 * heads * D) fp32 (K then V, each (heads, D) per token: the layout of
    mix_transformer.py:147-149) -> (B, N, heads * D) = `(softmax(scale q k^T) v).transpose(1, 2).reshape(B, N, C)`; None
    outside the kernel's domain (head dimension 64 or 32, contiguous rows)."""
    B, N, C = q.shape
    if C not in (heads * 64, heads * 32) or kv.shape[2] != 2 * C or q.stride(2) != 1 or kv.stride(2) != 1 or q.stride(1) % 4 or kv.stride(1) % 4 \
            or q.stride(0) % 4 or kv.stride(0) % 4 or q.data_ptr() % 16 or kv.data_ptr() % 16:
        return None
    return _Attn32Fn.apply(q, kv, heads, scale)


# ---------------------------------------------------------------------------------------------------------------------
# convolution (groups == 1, square geometry)
# ---------------------------------------------------------------------------------------------------------------------
def _cp(C):
    """Channels per split term: C to a multiple of 8 -- of 32 above 64 channels, so that the 3 Cp channels of a pixel are a multiple
    of 32 and the 3 x 3 layers take the halo-tiled kernel (csrc/conv3x3.hip: 64-channel chunks, a last half chunk allowed); the
    decoders' first layers see 84-87 channels (uawarpc.py:136-160): 96, i.e. 9-14 % more products on those layers."""
    return -(-C // 32) * 32 if C > 64 else -(-C // 8) * 8


def _nhwc3(x, order):
    """NCHW-shaped fp32 -> (B, H, W, 3 Cp) bf16: the split terms `order` concatenated along the channels (Cp = _cp(C))."""
    xh = x.permute(0, 2, 3, 1)
    B, H, W, C = xh.shape
    Cp = _cp(C)
    # rows = pixels; a channels-last tensor (also a channel slice of one) has uniformly strided rows: no copy
    if not (xh.stride(3) == 1 and xh.stride(2) >= C and xh.stride(1) == W * xh.stride(2) and xh.stride(0) == H * xh.stride(1)):
        xh = xh.contiguous()
    rows = xh.as_strided((B * H * W, C), (xh.stride(2), 1))
    return split3(rows, order, Cp).view(B, H, W, 3 * Cp), Cp


def _w3(w, order):
    """(N, C, KH, KW) fp32 -> packed bf16 rows [n][(tap, 3 Cp)] with the split terms `order` per tap; N padded to 8."""
    N, C, KH, KW = w.shape
    Cp = _cp(C)
    hi, lo = split2(w)
    w3 = torch.zeros((N, 3 * Cp, KH, KW), dtype=BF, device=w.device)
    for i, which in enumerate(order):
        w3[:, i * Cp:i * Cp + C] = hi if which == "h" else lo
    packed = mfma.pack_conv_weight(w3, BF)
    Np = -(-N // 8) * 8
    if Np != N:
        packed = torch.cat([packed, packed.new_zeros((Np - N, packed.shape[1]))])
    return packed


def _wb(weight, bias):
    """(packed split weight, bias padded to the packed row count) of a convolution's forward: params.derived entries without a
    refill view, which stand until the parameter changes or a params.refresh() of a set that holds it.  The frozen matcher's
    decoders pack their ~60 weights per align() once; a trainable convolution re-packs once per step."""
    wp = derived(weight, ("split3", "hlh"), lambda t: _w3(t, "hlh"))
    if bias is None:
        return wp, None
    N, Np = bias.shape[0], wp.shape[0]
    if Np == N and bias.is_contiguous():
        return wp, bias
    return wp, derived(bias, ("split3_bias", Np), lambda t: torch.nn.functional.pad(t, (0, Np - N)).contiguous())


def cat_split(parts):
    """[(B, c_i, H, W) fp32 maps, any strides] -> ((B, H, W, 3 Cp) bf16 (hi, hi, lo) split of their channel concatenation, Cp, C) in
    one launch (csrc/split3.hip split3_cat_kernel); None outside its domain (more than 4 parts, more than 96 channels)."""
    import ctypes
    B, _, H, W = parts[0].shape
    C = sum(p.shape[1] for p in parts)
    Cp = _cp(C)
    if not (1 <= len(parts) <= 4 and Cp <= 96 and all(p.is_cuda and p.dtype == torch.float32 and p.dim() == 4
                                                      and p.shape[0] == B and tuple(p.shape[2:]) == (H, W) for p in parts)):
        return None
    n = len(parts)
    out = torch.empty((B, H, W, 3 * Cp), dtype=BF, device=parts[0].device)
    ptrs = (ctypes.c_void_p * n)(*[p.data_ptr() for p in parts])
    strides = (ctypes.c_long * (4 * n))(*[v for p in parts for v in p.stride()])
    chans = (ctypes.c_int * n)(*[p.shape[1] for p in parts])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    _lib.call("rfn_split3_cat_bf16", out.device, cast(ptrs), cast(strides), cast(chans), n, ptr(out), B, H, W, Cp)
    return out, Cp, C


def parts_ok(parts, weight):
    """The shapes conv2d_parts takes (gradient-free, int geometry: the caller's to see): at most 4 fp32 HIP maps of one
    (B, H, W), channels that add up to the filter's, within cat_split's 96 channels and the kernel's reduction length."""
    N, C, KH, KW = weight.shape
    B, hw = parts[0].shape[0], parts[0].shape[2:]
    return (1 <= len(parts) <= 4 and sum(p.shape[1] for p in parts) == C and _cp(C) <= 96 and 3 * _cp(C) * KH * KW // 8 < 65536
            and all(p.is_cuda and p.dtype == torch.float32 and p.dim() == 4 and p.shape[0] == B and p.shape[2:] == hw
                    for p in parts))


def conv2d_parts(parts, weight, bias=None, stride=1, padding=0, dilation=1, act=0):
    """conv2d(torch.cat(parts, 1), ...) for gradient-free fp32 HIP maps without materialising the concatenation: the parts are
    gathered, split and laid out channels-last in one pass (cat_split), then the one-launch split-bf16 convolution.  None outside
    the domain (the caller concatenates)."""
    if torch.is_grad_enabled() or not isinstance(stride, int) or not isinstance(padding, int) or not isinstance(dilation, int):
        return None
    N, C, KH, KW = weight.shape
    if sum(p.shape[1] for p in parts) != C or 3 * _cp(C) * KH * KW // 8 >= 65536:
        return None
    got = cat_split(parts)
    if got is None:
        return None
    x3, Cp, _ = got
    B, H, W = x3.shape[:3]
    wp, b = _wb(weight, bias)
    OH = (H + 2 * padding - dilation * (KH - 1) - 1) // stride + 1
    OW = (W + 2 * padding - dilation * (KW - 1) - 1) // stride + 1
    y = _conv_o32(x3, wp, b, B, H, W, 3 * Cp, wp.shape[0], KH, KW, stride, padding, dilation, act, False, (OH, OW))
    return y[..., :N].permute(0, 3, 1, 2)


def _conv_o32(x3, wp, bias, B, H, W, C, N, KH, KW, s, p, d, act, transposed, out_hw):
    """(H, W, C) = the convolution's INPUT side, N its output channels (C ABI of rfn_conv2d_nhwc_o32); the result has N
    channels (forward) or C channels (transposed = data gradient)."""
    oc = C if transposed else N
    y = torch.empty((B,) + tuple(out_hw) + (oc,), dtype=torch.float32, device=x3.device)
    _lib.call("rfn_conv2d_nhwc_o32", x3.device, ptr(x3), ptr(wp), ptr(bias), int(act), ptr(y), B, H, W, C, N, KH, KW, s, p, d,
              wp.stride(0), oc, 1 if transposed else 0)
    return y


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, s, p, d, act):
        N, C, KH, KW = weight.shape
        B, _, H, W = x.shape
        x3, Cp = _nhwc3(x, "hhl")
        Np = -(-N // 8) * 8
        wp, b = _wb(weight, bias)
        OH = (H + 2 * p - d * (KH - 1) - 1) // s + 1
        OW = (W + 2 * p - d * (KW - 1) - 1) // s + 1
        y = _conv_o32(x3, wp, b, B, H, W, 3 * Cp, Np, KH, KW, s, p, d, act, False, (OH, OW))
        ctx.save_for_backward(x, weight)
        ctx.conf, ctx.has_bias = (s, p, d), bias is not None
        assert act == 0 or not any(ctx.needs_input_grad), "activation epilogue: gradient-free callers only"
        return y[..., :N].permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        s, p, d = ctx.conf
        N, C, KH, KW = weight.shape
        B, _, H, W = x.shape
        gy = gy.float()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            g3, Np = _nhwc3(gy, "hhl")                                            # (B, OH, OW, 3 Np)
            wt = _w3(weight.permute(1, 0, 2, 3).contiguous(), "hlh")               # rows c, columns [tap][3 Np]
            Cp = wt.shape[0]
            dx = _conv_o32(g3, wt, None, B, H, W, Cp, 3 * Np, KH, KW, s, p, d, 0, True, (H, W))
            gx = dx[..., :C].permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            gh, gl = split2(gy.permute(0, 2, 3, 1))
            xh, xl = split2(x.permute(0, 2, 3, 1))
            Np, Cp = -(-N // 64) * 64, -(-C // 8) * 8
            g3 = torch.zeros((3 * B,) + gh.shape[1:3] + (Np,), dtype=BF, device=x.device)
            x3 = torch.zeros((3 * B, H, W, Cp), dtype=BF, device=x.device)
            for i, (a, b) in enumerate(((gh, xh), (gh, xl), (gl, xh))):
                g3[i * B:(i + 1) * B, ..., :N] = a
                x3[i * B:(i + 1) * B, ..., :C] = b
            Kp = -(-(KH * KW * Cp) // 64) * 64
            part = mfma.conv2d_nhwc_wgrad(g3, x3, KH, KW, Kp, s, p, d)
            if part is None:
                raise RuntimeError("split32.conv2d: outside the weight-gradient kernel's domain")
            gw = part.sum(0)[:N, :KH * KW * Cp].view(N, KH, KW, Cp)[..., :C].permute(0, 3, 1, 2)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gy.sum((0, 2, 3))
        return gx, gw, gb, None, None, None, None


def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1, act=0):
    """F.conv2d (groups 1, square geometry, power-of-two stride when a data gradient is needed) for fp32 HIP tensors; None
    when the geometry is outside the kernels' domain."""
    vals = []
    for v in (stride, padding, dilation):
        if isinstance(v, (tuple, list)):
            if v[0] != v[1]:
                return None
            v = v[0]
        if isinstance(v, str):
            return None
        vals.append(int(v))
    s, p, d = vals
    N, C, KH, KW = weight.shape
    if x.shape[1] != C or (x.requires_grad and torch.is_grad_enabled() and s & (s - 1)):
        return None
    if 3 * _cp(C) * KH * KW // 8 >= 65536 or 3 * _cp(N) * KH * KW // 8 >= 65536:
        return None
    return _Conv2dFn.apply(x, weight, bias, s, p, d, act)
