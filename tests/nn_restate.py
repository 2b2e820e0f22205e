"""float64 restatement of include/fbsmi_nn.h -- TEST INFRASTRUCTURE.

One function per entry point of the header, written from the formulas in its comments (not from fbs_amd/unet.py), in
plain torch float64 ops, on whatever device the arguments live on.  Each takes the arrays the kernel takes, in the
kernel's layouts: token-major activations, the (Cout, 3, 3, wstride) weight with `ci_off`, a channel slice of a wider
tensor as a strided view (the kernel's pointer + `xstride`), `accumulate`, and None wherever the kernel takes NULL.

Nothing is rounded here: for bfloat16 operands the caller passes the bfloat16-rounded values upcast to float64 (`f64`),
so the reference multiplies the numbers the kernel multiplies.  tests/test_nn_restate.py pins these functions against
torch's own float64 operators and oracle/unet_np.py without a GPU.
"""
import math

import torch
import torch.nn.functional as F


def f64(t):
    """A tensor's values, exactly, in float64 (None stays None)."""
    return None if t is None else t.detach().to(torch.float64)


def linear_attention(qkv, heads, dim_head=32):
    """fbsmi_nn_linear_attention: qkv (B, n, 3 * heads * dim_head), channel = which * heads * dim_head + head * dim_head + d
    -> out (B, n, heads * dim_head), channel = head * dim_head + e."""
    B, n, _ = qkv.shape
    q, k, v = qkv.reshape(B, n, 3, heads, dim_head).unbind(2)           # each (B, n, heads, dim_head)
    q = torch.softmax(q, dim=3) / math.sqrt(dim_head)                   # over the embedding
    k = torch.softmax(k, dim=1)                                         # over the tokens
    v = v / n
    ctx = torch.einsum("bnhd,bnhe->bhde", k, v)                         # context[d][e] = sum_n k[n][d] v[n][e]
    out = torch.einsum("bhde,bnhd->bnhe", ctx, q)                       # out[n][e] = sum_d context[d][e] q[n][d]
    return out.reshape(B, n, heads * dim_head)


def qkv_linear_attention(xn, w, heads, dim_head=32):
    """fbsmi_nn_qkv_linear_attention: xn (B, n, C), w (3 * heads * dim_head, C): qkv = xn W^T, then the core above."""
    return linear_attention(torch.matmul(xn, w.t()), heads, dim_head)


def qkv_logits(xn, w, heads, dim_head=32):
    """The q and k logits (B, n, heads * dim_head each) the kernel above forms: for the tests that constrain them."""
    qkv = torch.matmul(xn, w.t())
    hd = heads * dim_head
    return qkv[..., :hd], qkv[..., hd:2 * hd]


def conv3x3(x, w, ci_off, bias, y=None, accumulate=False):
    """fbsmi_nn_conv3x3.  x: (B, H, W, Cin) -- the slice itself, e.g. wide[..., c0:c0 + Cin] (any strides: that view is the
    kernel's pointer and xstride); w: (Cout, 3, 3, wstride), of which channels ci_off .. ci_off + Cin multiply this slice;
    bias (Cout) or None; y (B, H, W, Cout): what accumulate adds to.
      out[b, i, j, :] = [y[b, i, j, :] +] bias + sum_{di, dj, c} w[:, di + 1, dj + 1, ci_off + c] x[b, i + di, j + dj, c]"""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))                                   # zero padding 1 on the two image axes
    out = torch.zeros((B, H, W, Cout), dtype=x.dtype, device=x.device)
    for ti in range(3):
        for tj in range(3):
            out = out + torch.matmul(xp[:, ti:ti + H, tj:tj + W, :], w[:, ti, tj, ci_off:ci_off + Cin].t())
    if bias is not None:
        out = out + bias
    if accumulate:
        out = out + y
    return out


def conv3x3_supported(H, W, Cin, Cout):
    """fbsmi_nn_conv3x3_supported, from the header's sentence: W < 248 at Cin = 64, W <= 100 at Cin = 128."""
    if H < 1 or W < 1 or Cin not in (64, 128) or Cout < 64 or Cout % 64 != 0:
        return 0
    return 1 if (W < 248 if Cin == 64 else W <= 100) else 0


def conv3x3_tile_rule(W, Cin, cfg=None):
    """The tile shape the dispatcher takes for rows of W pixels and slices of Cin channels, from the rule in the comment
    above conv3x3_shape in fbsmi_nn.hip: 8 waves when the staged range fits beside the weights in 160 KB of LDS (and in the
    threads' staging registers), else 6, else 4; one block of 32 pixels per wave; cfg = "<waves><pixel blocks>" overrides.
    -> dict(nw, mb, tile, lds, cap) or None (no shape: FBSMI_ERR_UNSUPPORTED).  cap = workgroups launched at most."""
    ck = Cin // 16
    nco = 64 if ck == 4 else 32

    def lds_of(nw, mb):
        return 16 * (9 * ck * 2 * nco + (32 * mb * nw + 2 * W + 3) * (2 * ck + 1))

    def fits(nw, mb):
        return lds_of(nw, mb) <= 160 * 1024 and (32 * mb * nw + 2 * W + 2) * 2 * ck <= (12 if nw >= 6 else 24) * 64 * nw

    nw, mb = 8, 1
    if not fits(nw, mb):
        nw = 6
    if not fits(nw, mb):
        nw = 4
    if cfg is not None:
        nw, mb = int(cfg[0]), int(cfg[1])
    if nw not in (4, 6, 8) or mb not in (1, 2) or (nw == 6 and mb != 1) or not fits(nw, mb):
        return None
    lds = lds_of(nw, mb)
    return dict(nw=nw, mb=mb, tile=32 * mb * nw, lds=lds, cap=256 * ((160 * 1024) // lds))


def proj64(a, b, w, bias, ln_scale, eps, residual):
    """fbsmi_nn_proj64: y = [LN_c]( a Wa^T [+ b Wb^T] [+ bias] ) [* ln_scale] [+ residual]; a (npix, Ca), b (npix, Cb) or
    None, w (64, Ca + Cb), bias / ln_scale (64) or None, residual (npix, 64) or None."""
    Ca = a.shape[1]
    y = torch.matmul(a, w[:, :Ca].t())
    if b is not None:
        y = y + torch.matmul(b, w[:, Ca:].t())
    if bias is not None:
        y = y + bias
    if ln_scale is not None:
        mean = y.mean(dim=1, keepdim=True)
        var = ((y - mean) ** 2).mean(dim=1, keepdim=True)
        y = (y - mean) / torch.sqrt(var + eps) * ln_scale
    if residual is not None:
        y = y + residual
    return y


def groupnorm_silu(x, groups, gamma, beta, eps, scale=None, shift=None, xbias=None, residual=None, rbias=None):
    """fbsmi_nn_groupnorm_silu: x (B, n, C); gamma, beta, xbias, rbias (C); scale, shift (B, C); residual (B, n, C).
    rbias without a residual is ignored, as the header says."""
    B, n, C = x.shape
    xx = x if xbias is None else x + xbias
    g = xx.reshape(B, n, groups, C // groups)
    mean = g.mean(dim=(1, 3), keepdim=True)
    var = ((g - mean) ** 2).mean(dim=(1, 3), keepdim=True)              # biased
    z = ((g - mean) / torch.sqrt(var + eps)).reshape(B, n, C) * gamma + beta
    if scale is not None:
        z = z * (1.0 + scale[:, None, :]) + shift[:, None, :]
    y = z / (1.0 + torch.exp(-z))                                       # silu
    if residual is not None:
        y = y + residual
        if rbias is not None:
            y = y + rbias
    return y


def channel_layernorm(x, scale, eps, residual=None, xbias=None):
    """fbsmi_nn_channel_layernorm: x (rows, C), scale (C), xbias (C) or None, residual (rows, C) or None."""
    xx = x if xbias is None else x + xbias
    mean = xx.mean(dim=1, keepdim=True)
    var = ((xx - mean) ** 2).mean(dim=1, keepdim=True)
    y = (xx - mean) / torch.sqrt(var + eps) * scale
    return y if residual is None else y + residual


def bias_add(y, bias):
    """fbsmi_nn_bias_add: y (rows, C) + bias (C)."""
    return y + bias


def pixel_shuffle(x, s, bias=None):
    """fbsmi_nn_pixel_shuffle: x (B, H, W, s * s * c) [+ bias (s * s * c)] -> (B, s * H, s * W, c),
    'b h w (h2 w2 c) -> b (h h2) (w w2) c'."""
    B, H, W, C = x.shape
    c = C // (s * s)
    xx = x if bias is None else x + bias
    return xx.reshape(B, H, W, s, s, c).permute(0, 1, 3, 2, 4, 5).reshape(B, H * s, W * s, c)
