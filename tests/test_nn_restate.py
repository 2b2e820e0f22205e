"""tests/nn_restate.py (the float64 restatement of include/fbsmi_nn.h that tests/test_gpu_nn_edges.py compares the kernels
with) pinned without a GPU against torch's float64 operators and oracle/unet_np.py, and the argument validation of the
nine fbsmi_nn_* entry points: every answer checked here is given on the host, before any HIP call."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_restate as R

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


# ------------------------------------------------------------------------------------------------
# (a) the restatement against torch float64 and the numpy oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout,xs,c0,ws,ci_off", [(2, 3, 4, 8, 5, 8, 0, 8, 0), (1, 1, 5, 6, 4, 16, 8, 20, 9),
                                                          (3, 4, 1, 4, 3, 12, 4, 4, 0)])
def test_conv3x3_restatement(B, H, W, Cin, Cout, xs, c0, ws, ci_off):
    """F.conv2d (cross-correlation, padding 1) on the slice's channels; a strided slice of a wider tensor, ci_off / wstride,
    bias None, accumulate; oracle/unet_np.conv2d on the same numbers."""
    from oracle import unet_np
    wide = _rand(B, H, W, xs, seed=1)
    w = _rand(Cout, 3, 3, ws, seed=2)
    bias = _rand(Cout, seed=3)
    y0 = _rand(B, H, W, Cout, seed=4)
    x = wide[..., c0:c0 + Cin]
    wk = w[..., ci_off:ci_off + Cin]                                          # (Cout, 3, 3, Cin)
    want = F.conv2d(x.permute(0, 3, 1, 2), wk.permute(0, 3, 1, 2), bias, padding=1).permute(0, 2, 3, 1)
    _close(R.conv3x3(x, w, ci_off, bias), want)
    _close(R.conv3x3(x, w, ci_off, None), want - bias)
    _close(R.conv3x3(x, w, ci_off, bias, y0, accumulate=True), want + y0)
    _close(R.conv3x3(x, w, ci_off, bias, y0, accumulate=False), want)
    onp = unet_np.conv2d(x.numpy(), wk.permute(1, 2, 3, 0).numpy(), bias.numpy(), pad=1)   # kernel (kh, kw, in, out)
    _close(R.conv3x3(x, w, ci_off, bias), torch.from_numpy(onp))


def test_conv3x3_supported_and_tile_rule_restatement():
    """The header's sentence (W < 248 at Cin = 64, W <= 100 at Cin = 128) and the dispatcher's rule agree with each other, and
    the rule gives the tile shapes test_gpu_nn_edges.py's table expects."""
    for Cin in (64, 128):
        for W in range(1, 300):
            assert R.conv3x3_supported(4, W, Cin, 64) == (R.conv3x3_tile_rule(W, Cin) is not None)
    assert R.conv3x3_supported(0, 8, 64, 64) == 0 and R.conv3x3_supported(8, 8, 32, 64) == 0 and R.conv3x3_supported(8, 8, 64, 96) == 0
    table = [(128, 36, 8), (128, 37, 6), (128, 47, 6), (128, 48, 4), (128, 100, 4), (64, 183, 8), (64, 184, 6), (64, 191, 6),
             (64, 192, 4), (64, 247, 4)]
    for Cin, W, nw in table:
        assert R.conv3x3_tile_rule(W, Cin)["nw"] == nw
    t = R.conv3x3_tile_rule(8, 64)
    assert (t["nw"], t["tile"], t["cap"]) == (8, 256, 256)                    # 65 536 pixels per round


@pytest.mark.parametrize("Ca,Cb", [(8, 0), (6, 10)])
@pytest.mark.parametrize("ln,bias,res", [(True, True, True), (False, False, False), (True, False, False), (False, True, True)])
def test_proj64_restatement(Ca, Cb, ln, bias, res):
    """F.linear on the concatenation, F.layer_norm over the channels (no bias), the residual; oracle/unet_np.layer_norm."""
    from oracle import unet_np
    npix = 7
    a, b = _rand(npix, Ca, seed=1), (_rand(npix, Cb, seed=2) if Cb else None)
    w = _rand(64, Ca + Cb, seed=3)
    bs = _rand(64, seed=4) if bias else None
    sc = _rand(64, seed=5) if ln else None
    rs = _rand(npix, 64, seed=6) if res else None
    y = F.linear(a if b is None else torch.cat([a, b], dim=1), w, bs)
    if ln:
        _close(F.layer_norm(y, (64,), sc, None, 1e-5), torch.from_numpy(unet_np.layer_norm(y.numpy(), sc.numpy(), 1e-5)))
        y = F.layer_norm(y, (64,), sc, None, 1e-5)
    if res:
        y = y + rs
    _close(R.proj64(a, b, w, bs, sc, 1e-5, rs), y)


@pytest.mark.parametrize("heads,n,B", [(1, 1, 1), (3, 5, 2), (4, 9, 1)])
def test_linear_attention_restatement(heads, n, B):
    """The einsum form of LinearAttention on NCHW-style (b, h, d, n) tensors, and the numpy oracle's lines for the same block;
    the fused to_qkv form is the 1x1 convolution in front of it."""
    from oracle import unet_np
    dh, hd = 32, heads * 32
    qkv = _rand(B, n, 3 * hd, seed=heads + n) * 2.0
    q, k, v = (t.reshape(B, n, heads, dh) for t in qkv.chunk(3, dim=2))
    qs, ks = torch.softmax(q, dim=-1) / math.sqrt(dh), torch.softmax(k, dim=-3)
    ctx = torch.einsum("bnhd,bnhe->bhde", ks, v / n)
    want = torch.einsum("bhde,bnhd->bhen", ctx, qs).permute(0, 3, 1, 2).reshape(B, n, hd)
    _close(R.linear_attention(qkv, heads), want)
    qn, kn, vn = (t.numpy() for t in (q, k, v))                               # oracle/unet_np.py attnblock, linear branch
    ctx_np = np.einsum("bnhd,bnhe->bhde", unet_np.softmax(kn, -3), vn / n)
    out_np = np.einsum("bhde,bnhd->bhen", ctx_np, unet_np.softmax(qn, -1) / math.sqrt(dh)).transpose(0, 3, 1, 2).reshape(B, n, hd)
    _close(R.linear_attention(qkv, heads), torch.from_numpy(out_np))
    Cx = 6
    xn, w = _rand(B, n, Cx, seed=7), _rand(3 * hd, Cx, seed=8)
    conv = F.conv2d(xn.permute(0, 2, 1)[..., None], w[:, :, None, None])[..., 0].permute(0, 2, 1)   # the 1x1 convolution
    _close(R.qkv_linear_attention(xn, w, heads), R.linear_attention(conv, heads))
    ql, kl = R.qkv_logits(xn, w, heads)
    _close(ql, conv[..., :hd])
    _close(kl, conv[..., hd:2 * hd])


@pytest.mark.parametrize("C,groups", [(16, 2), (24, 1), (8, 8)])
@pytest.mark.parametrize("mod,xb,res,rb", [(True, True, True, True), (False, False, False, False), (True, False, True, False),
                                          (False, True, False, True)])
def test_groupnorm_silu_restatement(C, groups, mod, xb, res, rb):
    """F.group_norm (biased variance) on (B, C, n) + the modulation + F.silu + residual + rbias; rbias without a residual is
    ignored; oracle/unet_np.group_norm and swish."""
    from oracle import unet_np
    B, n, eps = 2, 5, 1e-6
    x = _rand(B, n, C, seed=1) * 2 + 0.7
    gamma, beta = _rand(C, seed=2), _rand(C, seed=3)
    scale, shift = (_rand(B, C, seed=4), _rand(B, C, seed=5)) if mod else (None, None)
    xbias = _rand(C, seed=6) if xb else None
    resid = _rand(B, n, C, seed=7) if res else None
    rbias = _rand(C, seed=8) if rb else None
    xx = x + xbias if xb else x
    z = F.group_norm(xx.permute(0, 2, 1), groups, gamma, beta, eps).permute(0, 2, 1)
    _close(z, torch.from_numpy(unet_np.group_norm(xx.reshape(B, n, 1, C).numpy(), gamma.numpy(), beta.numpy(), groups, eps)).reshape(B, n, C))
    if mod:
        z = z * (1 + scale[:, None, :]) + shift[:, None, :]
    y = F.silu(z)
    _close(y, torch.from_numpy(unet_np.swish(z.numpy())))
    if res:
        y = y + resid + (rbias if rb else 0.0)
    _close(R.groupnorm_silu(x, groups, gamma, beta, eps, scale, shift, xbias, resid, rbias), y)


@pytest.mark.parametrize("xb,res", [(False, False), (True, False), (False, True), (True, True)])
def test_channel_layernorm_restatement(xb, res):
    from oracle import unet_np
    rows, Cc = 6, 16
    x, scale = _rand(rows, Cc, seed=1) * 3 + 1, _rand(Cc, seed=2)
    xbias = _rand(Cc, seed=3) if xb else None
    resid = _rand(rows, Cc, seed=4) if res else None
    xx = x + xbias if xb else x
    y = F.layer_norm(xx, (Cc,), scale, None, 1e-5)
    _close(y, torch.from_numpy(unet_np.layer_norm(xx.numpy(), scale.numpy(), 1e-5)))
    _close(R.channel_layernorm(x, scale, 1e-5, resid, xbias), y + resid if res else y)


@pytest.mark.parametrize("s,c", [(1, 8), (2, 8), (3, 16)])
def test_bias_add_and_pixel_shuffle_restatement(s, c):
    """The einops pattern 'b h w (h2 w2 c) -> b (h h2) (w w2) c' element by element, and oracle/unet_np.pixel_shuffle."""
    from oracle import unet_np
    B, H, W = 2, 3, 5
    x, bias = _rand(B, H, W, s * s * c, seed=s), _rand(s * s * c, seed=9)
    got = R.pixel_shuffle(x, s, bias)
    assert got.shape == (B, s * H, s * W, c)
    want = torch.empty_like(got)
    for h2 in range(s):
        for w2 in range(s):
            ch = (h2 * s + w2) * c
            want[:, h2::s, w2::s, :] = x[..., ch:ch + c] + bias[ch:ch + c]
    assert torch.equal(got, want)
    assert torch.equal(R.pixel_shuffle(x, s, None), torch.from_numpy(unet_np.pixel_shuffle(x.numpy(), s)))
    y = _rand(7, 24, seed=3)
    b2 = _rand(24, seed=4)
    assert torch.equal(R.bias_add(y, b2), y + b2.view(1, 24))


# ------------------------------------------------------------------------------------------------
# (b) argument validation.  Every call below is answered before the first HIP call (the pointers are host memory that no
# kernel may ever see): each case was read against the checks at the top of its entry point in fbsmi_nn.hip.
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from fbs_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def P():
    buf = C.create_string_buffer(4096)                                        # a non-NULL pointer; never dereferenced
    return C.addressof(buf), buf


def _expect(L, rc, code, name):
    assert rc == code, (name, rc, L.fbsmi_last_error())
    if code != OK:
        assert name.encode() in L.fbsmi_last_error(), L.fbsmi_last_error()


def test_validation_linear_attention(L, P):
    p, f = P[0], L.fbsmi_nn_linear_attention
    for args in [(None, p, 0, 1, 4, 1, 32), (p, None, 0, 1, 4, 1, 32), (p, p, 0, 1, 0, 1, 32), (p, p, 2, 1, 4, 1, 32),
                 (p, p, -1, 1, 4, 1, 32), (p, p, 0, -1, 4, 1, 32), (p, p, 0, 1, 4, 0, 32)]:
        _expect(L, f(*args, None), ERR_ARG, "nn_linear_attention")
    for dh in (16, 31, 64):
        _expect(L, f(p, p, 0, 1, 4, 1, dh, None), ERR_UNSUPPORTED, "nn_linear_attention")
    _expect(L, f(p, p, 1, 65536, 4, 1, 32, None), ERR_UNSUPPORTED, "nn_linear_attention")
    _expect(L, f(p, p, 0, 0, 4, 1, 32, None), OK, "nn_linear_attention")
    _expect(L, f(p, p, 1, 0, 1, 4, 32, None), OK, "nn_linear_attention")


def test_validation_qkv_linear_attention(L, P):
    p, f = P[0], L.fbsmi_nn_qkv_linear_attention
    for args in [(None, p, p, 1, 4, 64, 1, 32), (p, None, p, 1, 4, 64, 1, 32), (p, p, None, 1, 4, 64, 1, 32),
                 (p, p, p, 1, 0, 64, 1, 32), (p, p, p, -1, 4, 64, 1, 32), (p, p, p, 1, 4, 64, 0, 32)]:
        _expect(L, f(*args, None), ERR_ARG, "nn_qkv_linear_attention")
    _expect(L, f(p, p, p, 1, 4, 64, 1, 16, None), ERR_UNSUPPORTED, "nn_qkv_linear_attention")
    for Cx in (8, 24, 48, 96, 256):
        _expect(L, f(p, p, p, 1, 4, Cx, 1, 32, None), ERR_UNSUPPORTED, "nn_qkv_linear_attention")
    for Cx in (16, 32, 64, 128):
        _expect(L, f(p, p, p, 0, 4, Cx, 4, 32, None), OK, "nn_qkv_linear_attention")


def test_validation_conv3x3_and_its_supported_query(L, P):
    p, f, q = P[0], L.fbsmi_nn_conv3x3, L.fbsmi_nn_conv3x3_supported
    #      x  xstride w wstride ci_off bias y acc B H W Cin Cout
    good = [p, 64, p, 64, 0, p, p, 0, 1, 4, 4, 64, 64]

    def with_(**kw):
        names = ["x", "xstride", "w", "wstride", "ci_off", "bias", "y", "acc", "B", "H", "W", "Cin", "Cout"]
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    for kw in [dict(x=None), dict(w=None), dict(y=None), dict(B=-1), dict(H=0), dict(W=0),
               dict(xstride=56), dict(xstride=127, Cin=128), dict(xstride=68),          # narrower than the slice; misaligned
               dict(ci_off=4, wstride=72), dict(ci_off=-8), dict(wstride=68), dict(wstride=120, ci_off=64),
               dict(wstride=56)]:
        _expect(L, f(*with_(**kw), None), ERR_ARG, "nn_conv3x3")
    for kw in [dict(Cin=32, xstride=32, wstride=32), dict(Cout=96), dict(Cout=0), dict(Cin=128, xstride=128, wstride=128, W=101),
               dict(Cin=128, xstride=128, wstride=128, W=101, B=0), dict(W=248), dict(W=248, B=0), dict(B=1 << 20, H=32, W=33)]:
        _expect(L, f(*with_(**kw), None), ERR_UNSUPPORTED, "nn_conv3x3")
    # the query and the entry point give one answer per shape; an empty batch of a supported shape is OK and launches nothing
    for Cin, W, sup in [(128, 100, 1), (128, 101, 0), (64, 247, 1), (64, 248, 0)]:
        assert q(8, W, Cin, 64) == sup == R.conv3x3_supported(8, W, Cin, 64)
        rc = f(*with_(Cin=Cin, xstride=Cin, wstride=Cin, W=W, H=8, B=0), None)
        _expect(L, rc, OK if sup else ERR_UNSUPPORTED, "nn_conv3x3")
    for Cin in (64, 128):
        for W in (1, 36, 37, 47, 48, 183, 184, 191, 192):
            assert q(3, W, Cin, 128) == R.conv3x3_supported(3, W, Cin, 128)
    assert q(8, 8, 32, 64) == 0 and q(8, 8, 64, 96) == 0 and q(0, 8, 64, 64) == 0 and q(8, 0, 64, 64) == 0
    _expect(L, f(*with_(B=0, bias=None), None), OK, "nn_conv3x3")


def test_validation_proj64(L, P):
    p, f = P[0], L.fbsmi_nn_proj64
    for args in [(None, 64, None, 0, p, p, p, 1e-5, p, p, 8), (p, 64, None, 0, None, p, p, 1e-5, p, p, 8),
                 (p, 64, None, 0, p, p, p, 1e-5, p, None, 8), (p, 64, None, 64, p, p, p, 1e-5, p, p, 8),
                 (p, 64, None, 0, p, p, p, 1e-5, p, p, -1)]:
        _expect(L, f(*args, None), ERR_ARG, "nn_proj64")
    for Ca, Cb in [(128, 64), (32, 0), (64, 32), (96, 0), (64, 128), (0, 64)]:
        _expect(L, f(p, Ca, p, Cb, p, None, None, 0.0, None, p, 8, None), ERR_UNSUPPORTED, "nn_proj64")
    for Ca, Cb in [(64, 0), (128, 0), (64, 64)]:
        _expect(L, f(p, Ca, p if Cb else None, Cb, p, None, None, 0.0, None, p, 0, None), OK, "nn_proj64")


def test_validation_groupnorm_silu(L, P):
    """33 groups is FBSMI_ERR_UNSUPPORTED, not FBSMI_ERR_ARG: it is a valid GroupNorm the kernel has no room for (32 group
    statistics in LDS), the same kind of answer as C = 384 -- and the one fbs_amd._lib.call turns into the
    NotImplementedError a dispatcher may fall back on.  groups < 1 is a bad argument."""
    p, f = P[0], L.fbsmi_nn_groupnorm_silu
    #       x  y dtype B  n  C  groups gamma beta eps scale shift xbias residual rbias
    good = [p, p, 0, 1, 4, 64, 8, p, p, 1e-6, p, p, p, p, p]

    def with_(**kw):
        names = ["x", "y", "dtype", "B", "n", "C", "groups", "gamma", "beta", "eps", "scale", "shift", "xbias", "residual", "rbias"]
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    for kw in [dict(x=None), dict(y=None), dict(gamma=None), dict(beta=None), dict(n=0), dict(B=-1), dict(dtype=2), dict(dtype=-1),
               dict(scale=None), dict(shift=None), dict(groups=0), dict(C=0)]:
        _expect(L, f(*with_(**kw), None), ERR_ARG, "nn_groupnorm_silu")
    for kw in [dict(C=384), dict(C=264, groups=33), dict(C=2112, groups=33), dict(C=64, groups=16), dict(C=72, groups=8),
               dict(C=4096), dict(C=192)]:
        _expect(L, f(*with_(**kw), None), ERR_UNSUPPORTED, "nn_groupnorm_silu")
    for kw in [dict(B=0), dict(B=0, scale=None, shift=None, xbias=None, residual=None, rbias=None), dict(B=0, C=256, groups=32)]:
        _expect(L, f(*with_(**kw), None), OK, "nn_groupnorm_silu")


def test_validation_channel_layernorm(L, P):
    p, f = P[0], L.fbsmi_nn_channel_layernorm
    for args in [(None, p, 0, 4, 64, p, 1e-5, None, None), (p, None, 0, 4, 64, p, 1e-5, None, None),
                 (p, p, 0, 4, 64, None, 1e-5, None, None), (p, p, 2, 4, 64, p, 1e-5, None, None),
                 (p, p, 0, -1, 64, p, 1e-5, None, None), (p, p, 0, 4, 4, p, 1e-5, None, None)]:
        _expect(L, f(*args, None), ERR_ARG, "nn_channel_layernorm")
    for Cx in (24, 1024, 12, 96, 520):
        _expect(L, f(p, p, 0, 4, Cx, p, 1e-5, None, None, None), ERR_UNSUPPORTED, "nn_channel_layernorm")
    for Cx in (8, 512):
        _expect(L, f(p, p, 1, 0, Cx, p, 1e-5, p, p, None), OK, "nn_channel_layernorm")


def test_validation_bias_add_and_pixel_shuffle(L, P):
    p, f = P[0], L.fbsmi_nn_bias_add
    for args in [(None, 0, 4, 8, p), (p, 0, 4, 8, None), (p, 0, -1, 8, p), (p, 0, 4, 12, p), (p, 0, 4, 0, p), (p, 2, 4, 8, p)]:
        _expect(L, f(*args, None), ERR_ARG, "nn_bias_add")
    _expect(L, f(p, 0, 0, 24, p, None), OK, "nn_bias_add")
    g = L.fbsmi_nn_pixel_shuffle
    for args in [(None, p, 0, 1, 2, 2, 8, 2, p), (p, None, 0, 1, 2, 2, 8, 2, p), (p, p, 3, 1, 2, 2, 8, 2, p), (p, p, 0, -1, 2, 2, 8, 2, p),
                 (p, p, 0, 1, 0, 2, 8, 2, p), (p, p, 0, 1, 2, 0, 8, 2, p), (p, p, 0, 1, 2, 2, 12, 2, p), (p, p, 0, 1, 2, 2, 0, 2, p),
                 (p, p, 0, 1, 2, 2, 8, 0, p)]:
        _expect(L, g(*args, None), ERR_ARG, "nn_pixel_shuffle")
    _expect(L, g(p, p, 1, 0, 2, 3, 24, 3, None, None), OK, "nn_pixel_shuffle")
