"""The score-network kernels of fbs_amd/csrc/fbsmi_nn.hip, called through the C ABI (include/fbsmi_nn.h) on device tensors
and compared with tests/nn_restate.py -- the float64 restatement of the header, itself pinned in tests/test_nn_restate.py --
over every output element, at the smallest shapes that enter each tile shape, loop round and mask of the kernels.

Tolerances.  The bfloat16 matrix-core kernels keep the per-element bounds of tests/test_unet.py (they follow from one
bfloat16 rounding of a float32 accumulation), now against float64 on the same bfloat16-rounded operands.  The float32
kernels (linear_attention, groupnorm_silu, channel_layernorm with dtype 0) are held to the accuracy of the eager torch
float32 operators they replaced: per case the largest error of those operators against float64 is measured, and the
kernel's largest error may be 4 times that (another summation order), with a floor of 2^-21 of the output's largest
magnitude (where torch happens to be exact).  With dtype 1 the bound is that plus 2^-8 |want| for the one rounding of the
output.  No bound is derived from a kernel's own output.  Every output is written into a buffer with guard bands that must
come back untouched, and starts as NaN so that an element the kernel skipped fails the comparison."""
import math

import pytest
import torch
import torch.nn.functional as F

import nn_restate as R

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
_GUARD = 1024


def _call(name, *args):
    from fbs_amd import _lib
    return _lib.call(name, *args)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dt(dtype):
    return 0 if dtype == F32 else 1


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _out(dev, shape, dtype, init=None):
    """An output tensor inside a buffer with guard bands (checked by _guards_ok); NaN (or `init`) to start with."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * _GUARD,), 3.0, dtype=dtype, device=dev)
    view = buf[_GUARD:_GUARD + n].view(shape)
    if init is None:
        view.fill_(float("nan"))
    else:
        view.copy_(init)
    return view, buf


def _guards_ok(buf):
    return bool((buf[:_GUARD] == 3.0).all()) and bool((buf[-_GUARD:] == 3.0).all())


def _f32_bound(eager32, want):
    """(bound, torch's error): 4 x the largest error of the eager float32 operators, floor 2^-21 max |want|."""
    err_t = (eager32.double() - want).abs().max().item()
    return max(4.0 * err_t, 2.0 ** -21 * want.abs().max().item()), err_t


def _check_f32_family(got, want, eager32, dtype, what):
    """float32: max error <= bound.  bfloat16: every element within 2^-8 |want| + bound."""
    bound, err_t = _f32_bound(eager32, want)
    err = (got.double() - want).abs()
    print(f"MEASURED {what} dtype={'f32' if dtype == F32 else 'bf16'} torch_f32_err={err_t:.3e} kernel_err={err.max().item():.3e} "
          f"bound={bound:.3e} max_want={want.abs().max().item():.3e}")
    if dtype == F32:
        assert bool((err <= bound).all()), (what, err.max().item(), bound, err_t)
    else:
        assert bool((err <= 2.0 ** -8 * want.abs() + bound).all()), (what, err.max().item(), bound, err_t)


# ================================================================================================
# conv3x3
# ================================================================================================
def _conv_case(dev, B, H, W, Cin, Cout, seed, xs=None, c0=0, ws=None, ci_off=0, bias=True, accumulate=False):
    """One call of fbsmi_nn_conv3x3 on random bfloat16 data against the restatement, every element."""
    xs = Cin if xs is None else xs
    ws = Cin if ws is None else ws
    assert c0 + Cin <= xs and ci_off + Cin <= ws                    # what the kernel reads stays inside the tensors
    g = _gen(seed)
    wide = _randn(g, B, H, W, xs).to(BF).to(dev)
    w = (_randn(g, Cout, 3, 3, ws) / (3 * Cin ** 0.5)).to(BF).to(dev)
    bs = _randn(g, Cout).to(dev) if bias else None
    y0 = _randn(g, B, H, W, Cout).to(BF).to(dev) if accumulate else None
    y, buf = _out(dev, (B, H, W, Cout), BF, init=y0)
    _call("fbsmi_nn_conv3x3", wide.data_ptr() + 2 * c0, xs, w.data_ptr(), ws, ci_off, _ptr(bs), y.data_ptr(), 1 if accumulate else 0,
          B, H, W, Cin, Cout, _st())
    want = R.conv3x3(R.f64(wide)[..., c0:c0 + Cin], R.f64(w), ci_off, R.f64(bs), R.f64(y0), accumulate)
    if accumulate:      # y0 stands for an earlier slice: one more bfloat16 rounding of a partial sum (tests/test_unet.py)
        tol = 2.0 ** -8 * want.abs() + 2.0 ** -9 * 2.0 * want.abs().max() + 4e-3
    else:
        tol = 2.0 ** -8 * want.abs() + 1e-3
    err = (y.double() - want).abs()
    assert _guards_ok(buf)
    assert bool((err <= tol).all()), (err.max().item(), int((~(err <= tol)).sum()))


@pytest.mark.parametrize("Cin,W,waves,B,H,Cout", [(128, 36, 8, 2, 3, 64), (128, 37, 6, 2, 3, 64), (128, 47, 6, 1, 3, 128),
                                                 (128, 48, 4, 2, 2, 64), (128, 100, 4, 1, 3, 64), (64, 183, 8, 1, 2, 64),
                                                 (64, 184, 6, 2, 2, 64), (64, 191, 6, 1, 3, 128), (64, 192, 4, 1, 3, 64),
                                                 (64, 247, 4, 1, 3, 64)])
def test_conv3x3_every_tile_shape_the_dispatcher_chooses(dev, monkeypatch, Cin, W, waves, B, H, Cout):
    """k_conv3x3<CK, NB, NW, 1> for NW = 8, 6, 4 at both slice widths, at the row widths where conv3x3_shape changes its
    answer (the 6-wave instantiations <8,1,6,1> and <4,2,6,1> and the widths at the LDS limit, W = 100 / 247, are launched
    by nothing else).  Rows this wide make every tile straddle image rows, and the last tile is ragged."""
    from fbs_amd import _lib
    monkeypatch.delenv("FBSMI_CONV_CFG", raising=False)
    rule = R.conv3x3_tile_rule(W, Cin)
    assert rule is not None and rule["nw"] == waves and rule["mb"] == 1
    assert _lib.lib().fbsmi_nn_conv3x3_supported(H, W, Cin, Cout) == 1
    assert (B * H * W) % rule["tile"] != 0
    _conv_case(dev, B, H, W, Cin, Cout, seed=1000 + W + Cin)


@pytest.mark.parametrize("Cin", [64, 128])
@pytest.mark.parametrize("cfg", ["82", "42"])
def test_conv3x3_two_pixel_blocks_per_wave(dev, monkeypatch, cfg, Cin):
    """The MB = 2 instantiations (k_conv3x3<.,.,8,2> and <.,.,4,2>: two accumulator rows per wave sharing every weight
    fragment, a park region of 64 rows per wave) through the documented FBSMI_CONV_CFG knob at W = 14; where the shape does
    not fit 160 KB of LDS (8 waves x 64 pixels at 128 channels) the call must say FBSMI_ERR_UNSUPPORTED and launch nothing."""
    from fbs_amd import _lib
    monkeypatch.setenv("FBSMI_CONV_CFG", cfg)
    B, H, W, Cout = 3, 14, 14, 64
    rule = R.conv3x3_tile_rule(W, Cin, cfg)
    if rule is None:
        assert (cfg, Cin) == ("82", 128)
        x = torch.zeros((B, H, W, Cin), dtype=BF, device=dev)
        w = torch.zeros((Cout, 3, 3, Cin), dtype=BF, device=dev)
        y, buf = _out(dev, (B, H, W, Cout), BF)
        L = _lib.lib()
        assert L.fbsmi_nn_conv3x3_supported(H, W, Cin, Cout) == 0
        rc = L.fbsmi_nn_conv3x3(x.data_ptr(), Cin, w.data_ptr(), Cin, 0, None, y.data_ptr(), 0, B, H, W, Cin, Cout, _st())
        assert rc == -3 and b"nn_conv3x3" in L.fbsmi_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all()) and _guards_ok(buf)
        return
    assert rule["mb"] == 2 and rule["nw"] == int(cfg[0]) and (B * H * W) % rule["tile"] != 0 and B * H * W > rule["tile"]
    _conv_case(dev, B, H, W, Cin, Cout, seed=82 + Cin)


@pytest.mark.parametrize("Cin", [64, 128])
def test_conv3x3_second_round_of_the_persistent_tile_loop(dev, monkeypatch, Cin):
    """More tiles than workgroups: the grid is capped at 256 * floor(160 KB / lds) workgroups, each walks tiles t, t +
    gridDim.x, ... and fetches the next tile's input into registers while it multiplies this one.  The smallest batch of
    8 x 8 images with cap * tile pixels plus one full and one ragged tile: workgroup 0 takes a second, full tile, workgroup 1
    a second, ragged one, every other workgroup finds its prefetch guard false."""
    monkeypatch.delenv("FBSMI_CONV_CFG", raising=False)
    rule = R.conv3x3_tile_rule(8, Cin)
    tile, cap = rule["tile"], rule["cap"]
    assert rule["nw"] == 8 and tile == 256 and cap == 256
    npix = cap * tile + tile + 64
    B = npix // 64
    assert B * 64 == npix and B == 1029
    ntiles = (npix + tile - 1) // tile
    assert ntiles > cap and ntiles == cap + 2 and npix % tile != 0        # the precondition: a second round, full + ragged
    _conv_case(dev, B, 8, 8, Cin, 64, seed=4242 + Cin)


@pytest.mark.parametrize("Cin", [64, 128])
@pytest.mark.parametrize("what", ["column", "row", "straddle", "xstride", "ci_off", "accumulate", "nobias", "all"])
def test_conv3x3_layout_edges(dev, monkeypatch, Cin, what):
    """column: H > 1, W = 1 (every horizontal tap is padding); row: H = 1 (every vertical tap is); straddle: 40 images of
    3 x 3, a tile covers 28 of them; xstride: a slice in the middle of a wider tensor; ci_off: a slice in the middle of a
    wider weight; accumulate: onto a known non-zero y; nobias: bias = NULL; all: everything at once."""
    monkeypatch.delenv("FBSMI_CONV_CFG", raising=False)
    kw = dict(column=dict(B=3, H=5, W=1), row=dict(B=3, H=1, W=7), straddle=dict(B=40, H=3, W=3),
              xstride=dict(B=2, H=4, W=5, xs=Cin + 128, c0=64), ci_off=dict(B=2, H=4, W=5, ws=Cin + 192, ci_off=64),
              accumulate=dict(B=2, H=6, W=5, accumulate=True), nobias=dict(B=2, H=4, W=5, bias=False),
              all=dict(B=5, H=7, W=9, xs=Cin + 72, c0=8, ws=Cin + 40, ci_off=24, accumulate=True, bias=False))[what]
    _conv_case(dev, Cin=Cin, Cout=128 if what == "all" else 64, seed=77 + Cin, **kw)


@pytest.mark.parametrize("Cin", [64, 128])
def test_conv3x3_single_pixels_and_single_taps_exactly(dev, monkeypatch, Cin):
    """Five 5 x 6 images with one non-zero pixel each (the four corners, one interior position) and a weight that is non-zero
    in one tap only, for each of the nine taps.  Pixel values in {-1, 0, 1}, weights in {-2 .. 2}: every output is an integer
    of magnitude <= 256, exact in float32 and in bfloat16, so the comparison is equality -- a transposed, mirrored or shifted
    tap, or a border test on the wrong side, moves a value to another pixel and fails outright."""
    monkeypatch.delenv("FBSMI_CONV_CFG", raising=False)
    H, W, Cout = 5, 6, 64
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (2, 3)]
    c = torch.arange(Cin)
    x = torch.zeros(len(spots), H, W, Cin)
    for b, (i, j) in enumerate(spots):
        x[b, i, j] = ((c + b) % 3 - 1).float()
    wt = (((torch.arange(Cout)[:, None] + 2 * c[None, :]) % 5) - 2).float()              # (Cout, Cin), rows differ
    x16 = x.to(BF).to(dev)
    for tap in range(9):
        w = torch.zeros(Cout, 3, 3, Cin)
        w[:, tap // 3, tap % 3] = wt
        w16 = w.to(BF).to(dev)
        y, buf = _out(dev, (len(spots), H, W, Cout), BF)
        _call("fbsmi_nn_conv3x3", x16.data_ptr(), Cin, w16.data_ptr(), Cin, 0, None, y.data_ptr(), 0, len(spots), H, W, Cin, Cout, _st())
        want = R.conv3x3(R.f64(x16), R.f64(w16), 0, None)
        assert want.abs().max().item() <= 256 and bool((want == want.round()).all())
        di, dj = tap // 3 - 1, tap % 3 - 1                                                # out[i, j] takes x[i + di, j + dj]
        for b, (i, j) in enumerate(spots):
            oi, oj = i - di, j - dj
            nz = want[b].abs().sum(dim=2).nonzero().tolist()
            assert nz == ([[oi, oj]] if (0 <= oi < H and 0 <= oj < W) else []), (tap, b, nz)
        assert _guards_ok(buf)
        assert torch.equal(y.double(), want), (tap, (y.double() - want).abs().max().item())


# ================================================================================================
# proj64
# ================================================================================================
def _proj_case(dev, chans, npix, ln, bias, res, seed):
    g = _gen(seed)
    Ca, Cb = chans[0], (chans[1] if len(chans) > 1 else 0)
    a = _randn(g, npix, Ca).to(BF).to(dev)
    b = _randn(g, npix, Cb).to(BF).to(dev) if Cb else None
    w = (_randn(g, 64, Ca + Cb) / (Ca + Cb) ** 0.5).to(BF).to(dev)
    bs = _randn(g, 64).to(dev) if bias else None
    sc = (0.5 + torch.rand(64, generator=g)).to(dev) if ln else None
    rs = _randn(g, npix, 64).to(BF).to(dev) if res else None
    y, buf = _out(dev, (npix, 64), BF)
    _call("fbsmi_nn_proj64", a.data_ptr(), Ca, _ptr(b), Cb, w.data_ptr(), _ptr(bs), _ptr(sc), 1e-5, _ptr(rs), y.data_ptr(), npix, _st())
    want = R.proj64(R.f64(a), R.f64(b), R.f64(w), R.f64(bs), R.f64(sc), 1e-5, R.f64(rs))
    err = (y.double() - want).abs()
    assert _guards_ok(buf)
    assert bool((err <= 2.0 ** -7 * want.abs() + 2e-2).all()), (chans, npix, ln, bias, res, err.max().item())


@pytest.mark.parametrize("chans", [(64,), (128,), (64, 64)])
def test_proj64_every_option_at_the_tile_edges(dev, chans):
    """k_proj64<4,0>, <8,0>, <4,4>, each with and without the LayerNorm (the LN template flag), the bias and the residual,
    at pixel counts around the 32-pixel wave tile and the 128-pixel workgroup: a lone pixel (31 lanes clamped to it), a ragged
    last tile whose dead lanes must not be stored, idle waves of the last workgroup."""
    for npix in (1, 31, 32, 33, 127, 128, 129):
        for k in range(8):
            _proj_case(dev, chans, npix, bool(k & 1), bool(k & 2), bool(k & 4), seed=100 * npix + k + sum(chans))


@pytest.mark.parametrize("chans,ln,res", [((128,), True, True), ((64, 64), False, False)])
def test_proj64_second_grid_round(dev, chans, ln, res):
    """2048 * 128 + 133 pixels: the grid is capped at 2048 workgroups of 4 waves x 32 pixels, so waves of workgroups 0 and 1
    take a second tile (t += gridDim.x * 4), the last of them ragged (5 of 32 pixels)."""
    npix = 2048 * 128 + 133
    assert (npix + 31) // 32 > 2048 * 4 and npix % 32 != 0
    _proj_case(dev, chans, npix, ln, True, res, seed=9 + sum(chans))


# ================================================================================================
# qkv_linear_attention
# ================================================================================================
def _qkv_case(dev, x, w, heads):
    B, n, Cx = x.shape
    x16, w16 = x.to(BF).to(dev).contiguous(), w.to(BF).to(dev).contiguous()
    y, buf = _out(dev, (B, n, heads * 32), BF)
    _call("fbsmi_nn_qkv_linear_attention", x16.data_ptr(), w16.data_ptr(), y.data_ptr(), B, n, Cx, heads, 32, _st())
    want = R.qkv_linear_attention(R.f64(x16), R.f64(w16), heads)
    err = (y.double() - want).abs().max().item()
    assert _guards_ok(buf)
    assert bool(torch.isfinite(y).all()) and err <= 2e-2 * want.abs().max().item(), (B, n, Cx, heads, err, want.abs().max().item())
    return R.qkv_logits(R.f64(x16), R.f64(w16), heads)


@pytest.mark.parametrize("Cx", [16, 32, 64, 128])
def test_qkv_linear_attention_channels_heads_and_token_counts(dev, Cx):
    """k_qkv_linear_attention<1, 2, 4, 8>; heads 1 (three idle waves), 4, 5 (a second head round with one active wave) and 8;
    token counts 1, 31, 33, 65 (a ragged last 32-token block: rows past n are loaded as zeros and masked) and 32."""
    for heads in (1, 4, 5, 8):
        for n in (1, 31, 32, 33, 65):
            g = _gen(Cx * 1000 + heads * 100 + n)
            _qkv_case(dev, _randn(g, 2, n, Cx), _randn(g, 3 * heads * 32, Cx) / Cx ** 0.5, heads)


@pytest.mark.parametrize("n", [33, 65])
@pytest.mark.parametrize("which", ["k", "q"])
def test_qkv_linear_attention_padding_rows_do_not_leak(dev, which, n):
    """The masks of the ragged token block.  Activations |randn| + 1 (all >= 1) and k-rows of w all <= -2: every real k-logit
    is <= -128, while a padding row's (x = 0) is exactly 0.  Were pass 1's `t0 + row_of(i) < n` test missing, the running max
    would be 0 and every exp(k - 0) underflows float32: Z = 0, the output NaN or inf; were pass 2's missing, a padding row's
    exp(0 - max) = inf lands in Z.  which = q is the mirror image for the q softmax (its running max starts from the first
    logit, not from 0)."""
    Cx, heads, B = 64, 5, 2
    g = _gen(n + (0 if which == "k" else 500))
    x = _randn(g, B, n, Cx).abs() + 1.0
    w = _randn(g, 3 * heads * 32, Cx) / Cx ** 0.5
    rows = slice(heads * 32, 2 * heads * 32) if which == "k" else slice(0, heads * 32)
    w[rows] = -(2.0 + 0.5 * _randn(g, heads * 32, Cx).abs())
    ql, kl = _qkv_case(dev, x, w, heads)
    lg = kl if which == "k" else ql
    assert lg.max().item() <= -20.0 and lg.max().item() <= -110.0       # the second: exp(logit - 0) is 0 in float32


def test_qkv_linear_attention_wide_logits(dev):
    """q and k logits spread over more than +-30: the online max / exp of both softmaxes far from the order-1 logits of the
    other cases."""
    Cx, heads = 64, 4
    for n in (33, 65):
        g = _gen(3000 + n)
        x = _randn(g, 2, n, Cx)
        w = _randn(g, 3 * heads * 32, Cx) / Cx ** 0.5
        w[:2 * heads * 32] *= 15.0
        ql, kl = _qkv_case(dev, x, w, heads)
        for lg in (ql, kl):
            assert lg.min().item() < -30.0 and lg.max().item() > 30.0


# ================================================================================================
# linear_attention
# ================================================================================================
def _la_case(dev, qkv, heads, dtype, what):
    B, n, _ = qkv.shape
    q = qkv.to(dtype).to(dev).contiguous()
    y, buf = _out(dev, (B, n, heads * 32), dtype)
    _call("fbsmi_nn_linear_attention", q.data_ptr(), y.data_ptr(), _dt(dtype), B, n, heads, 32, _st())
    want = R.linear_attention(R.f64(q), heads)
    eager = R.linear_attention(q.float(), heads)          # the same torch operators in float32: the eager path
    assert _guards_ok(buf)
    _check_f32_family(y, want, eager, dtype, what)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("heads,B", [(1, 1), (4, 3), (1, 3), (4, 1)])
def test_linear_attention_token_counts(dev, dtype, heads, B):
    """k_linear_attention<float / bfloat16>: n = 1, 7 (tokens < the 8 token groups of pass 1: empty groups merge with
    (-inf, 0)), 8, 9, 63, 64, 65 (the `nn < n` guards of the 64-token chunks of passes 2 and 3), 129 (three chunks)."""
    for n in (1, 7, 8, 9, 63, 64, 65, 129):
        g = _gen(heads * 1000 + B * 100 + n)
        _la_case(dev, _randn(g, B, n, 3 * heads * 32), heads, dtype, f"linear_attention random heads={heads} B={B} n={n}")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("kind", ["k_negative", "q_negative", "wide"])
def test_linear_attention_hard_logits(dev, dtype, kind):
    """All k (or q) logits <= -20, and logits uniform over +-30, at token counts with a ragged last chunk: a guard that let a
    token past n into the max or the sums (0 where it is staged as such) would dominate logits this negative."""
    heads, B = 4, 3
    for n in (7, 9, 65, 129):
        g = _gen(n + len(kind))
        qkv = _randn(g, B, n, 3, heads * 32)
        if kind == "k_negative":
            qkv[:, :, 1] = -(20.0 + 5.0 * qkv[:, :, 1].abs())
        elif kind == "q_negative":
            qkv[:, :, 0] = -(20.0 + 5.0 * qkv[:, :, 0].abs())
        else:
            qkv[:, :, :2] = 60.0 * torch.rand(B, n, 2, heads * 32, generator=g) - 30.0
        if kind != "wide":
            assert qkv[:, :, 1 if kind == "k_negative" else 0].to(dtype).max().item() <= -20.0
        _la_case(dev, qkv.reshape(B, n, 3 * heads * 32), heads, dtype, f"linear_attention {kind} n={n}")


# ================================================================================================
# groupnorm_silu
# ================================================================================================
def _eager_gn(x, groups, gamma, beta, eps, scale, shift, xbias, residual, rbias):
    """The float32 torch operators the kernel replaced."""
    xx = x if xbias is None else x + xbias
    z = F.group_norm(xx.transpose(1, 2), groups, gamma, beta, eps).transpose(1, 2)
    if scale is not None:
        z = z * (1.0 + scale[:, None, :]) + shift[:, None, :]
    y = F.silu(z)
    if residual is not None:
        y = y + residual
        if rbias is not None:
            y = y + rbias
    return y


def _gn_case(dev, x, groups, dtype, what, g, mod=True, xb=True, res=True, rb=True, gamma=None, beta=None, scale=None, shift=None,
             eps=1e-6):
    B, n, Cx = x.shape
    xd = x.to(dtype).to(dev).contiguous()
    gamma = (1.0 + 0.3 * _randn(g, Cx) if gamma is None else gamma).to(dev)
    beta = (0.3 * _randn(g, Cx) if beta is None else beta).to(dev)
    if mod:
        scale = (0.3 * _randn(g, B, Cx) if scale is None else scale).to(dev)
        shift = (0.3 * _randn(g, B, Cx) if shift is None else shift).to(dev)
    else:
        scale = shift = None
    xbias = (0.5 * _randn(g, Cx)).to(dev) if xb else None
    resid = _randn(g, B, n, Cx).to(dtype).to(dev) if res else None
    rbias = _randn(g, Cx).to(dev) if rb else None
    y, buf = _out(dev, (B, n, Cx), dtype)
    _call("fbsmi_nn_groupnorm_silu", xd.data_ptr(), y.data_ptr(), _dt(dtype), B, n, Cx, groups, gamma.data_ptr(), beta.data_ptr(), eps,
          _ptr(scale), _ptr(shift), _ptr(xbias), _ptr(resid), _ptr(rbias), _st())
    want = R.groupnorm_silu(R.f64(xd), groups, R.f64(gamma), R.f64(beta), eps, R.f64(scale), R.f64(shift), R.f64(xbias), R.f64(resid),
                            R.f64(rbias))
    eager = _eager_gn(xd.float(), groups, gamma, beta, eps, scale, shift, xbias, None if resid is None else resid.float(), rbias)
    assert _guards_ok(buf)
    _check_f32_family(y, want, eager, dtype, what)


def _gn_ns(Cx):
    lanes = 256 // (Cx // 8)
    return lanes, sorted({m for m in (1, lanes - 1, lanes, 4 * lanes - 1, 4 * lanes, 4 * lanes + 1, 9 * lanes + 3) if m >= 1})


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("Cx,groups", [(64, 8), (128, 8), (512, 8), (2048, 8), (256, 32), (64, 1)])
def test_groupnorm_silu_channel_layouts_and_token_counts(dev, dtype, Cx, groups):
    """k_groupnorm_silu with 1 to 32 token lanes (lanes = 256 / (C / 8)) and 1, 8 or 32 slots per group.  n < lanes: token
    lanes without a token enter the group merge with count 0; n = 4 lanes - 1, 4 lanes, 4 lanes + 1: the boundary of the
    four-vector unrolled loop of both passes and its remainder loop; 9 lanes + 3: two unrolled rounds and a ragged rest."""
    lanes, ns = _gn_ns(Cx)
    for n in ns:
        g = _gen(Cx + groups + n)
        _gn_case(dev, 2.0 * _randn(g, 2, n, Cx) + 0.7, groups, dtype, f"groupnorm random C={Cx} groups={groups} n={n}", g)


@pytest.mark.parametrize("dtype", [F32, BF])
def test_groupnorm_silu_every_null_pattern(dev, dtype):
    """scale + shift, xbias, residual and rbias each given or NULL (16 patterns), rbias with a NULL residual included: the
    header says it is ignored."""
    Cx, groups = 128, 8
    n = 4 * (256 // (Cx // 8)) + 1
    for k in range(16):
        g = _gen(160 + k)
        _gn_case(dev, 2.0 * _randn(g, 2, n, Cx) + 0.7, groups, dtype, f"groupnorm nulls pattern={k}", g,
                 mod=bool(k & 1), xb=bool(k & 2), res=bool(k & 4), rb=bool(k & 8))


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("Cx,groups", [(64, 8), (512, 8), (256, 32), (64, 1)])
@pytest.mark.parametrize("kind", ["offset", "constant", "saturate"])
def test_groupnorm_silu_hard_inputs(dev, dtype, kind, Cx, groups):
    """offset: every group sits 100 standard deviations from zero (+100 / -100 by group), what a sum-of-squares variance
    loses and the Welford / Chan merge must not; constant: group 0 is the constant 1.5 (variance exactly 0: eps alone sets
    the scale, the output is silu(beta ...)); saturate: shift = +-90 by channel, so SiLU's expf(-z) overflows to inf on one
    side (z / inf = -0 for a true value of -7e-38) and underflows on the other."""
    lanes, _ = _gn_ns(Cx)
    n, B = 9 * lanes + 3, 2
    g = _gen(Cx + groups + len(kind))
    x = _randn(g, B, n, Cx)
    kw = {}
    if kind == "offset":
        sign = 1.0 - 2.0 * (torch.arange(groups) % 2).float()
        x = x + (100.0 * sign).repeat_interleave(Cx // groups)
    elif kind == "constant":
        x[:, :, :Cx // groups] = 1.5
        kw = dict(xb=False)
    else:
        kw = dict(scale=torch.zeros(B, Cx), shift=(90.0 * (1.0 - 2.0 * (torch.arange(Cx) % 2).float())).repeat(B, 1).contiguous())
    _gn_case(dev, x, groups, dtype, f"groupnorm {kind} C={Cx} groups={groups}", g, **kw)


# ================================================================================================
# channel_layernorm
# ================================================================================================
def _ln_case(dev, x, dtype, what, g, xb, res):
    rows, Cx = x.shape
    xd = x.to(dtype).to(dev).contiguous()
    scale = (0.5 + torch.rand(Cx, generator=g)).to(dev)
    xbias = (0.5 * _randn(g, Cx)).to(dev) if xb else None
    resid = _randn(g, rows, Cx).to(dtype).to(dev) if res else None
    y, buf = _out(dev, (rows, Cx), dtype)
    _call("fbsmi_nn_channel_layernorm", xd.data_ptr(), y.data_ptr(), _dt(dtype), rows, Cx, scale.data_ptr(), 1e-5, _ptr(resid), _ptr(xbias), _st())
    want = R.channel_layernorm(R.f64(xd), R.f64(scale), 1e-5, R.f64(resid), R.f64(xbias))
    xx = xd.float() if xbias is None else xd.float() + xbias
    eager = F.layer_norm(xx, (Cx,), scale, None, 1e-5)
    if resid is not None:
        eager = eager + resid.float()
    assert _guards_ok(buf)
    _check_f32_family(y, want, eager, dtype, what)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("Cx", [8, 16, 64, 512])
def test_channel_layernorm_lane_groups_and_row_counts(dev, dtype, Cx):
    """k_channel_layernorm with L = C / 8 = 1, 2, 8, 64 lanes per row (0 to 6 xor-shuffle steps; 64: a row is a whole wave);
    rows = 1, one less than / exactly / one more than a workgroup's 256 / L rows (dead rows shuffle along and must not
    store), 1000; xbias and residual given and NULL."""
    per = 256 // (Cx // 8)
    for rows in sorted({1, per - 1, per, per + 1, 1000} - {0}):
        for k in range(4):
            g = _gen(Cx * 10 + rows + k)
            _ln_case(dev, 2.0 * _randn(g, rows, Cx) + 0.7, dtype, f"layernorm random C={Cx} rows={rows}", g, bool(k & 1), bool(k & 2))


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("Cx", [8, 16, 64, 512])
def test_channel_layernorm_hard_rows(dev, dtype, Cx):
    """Rows 100 standard deviations from zero (the first row of each of two workgroups) and a constant row (variance 0: the
    output is exactly the residual) among ordinary ones."""
    per = 256 // (Cx // 8)
    rows = per + 3
    g = _gen(Cx + 5)
    x = _randn(g, rows, Cx)
    x[0] += 100.0
    x[per] -= 100.0
    x[1] = 1.5
    _ln_case(dev, x, dtype, f"layernorm hard rows C={Cx}", g, False, True)


# ================================================================================================
# bias_add, pixel_shuffle
# ================================================================================================
@pytest.mark.parametrize("dtype", [F32, BF])
def test_bias_add_and_pixel_shuffle_exactly(dev, dtype):
    """One addition per element: float32 must equal the correctly rounded sum, bfloat16 the bfloat16 rounding of the float32
    sum.  s = 1, 2, 3 and c = 8, 24 (one and three vectors per output pixel), H != W, vector counts that are no multiple of the
    256-thread workgroup (one ragged workgroup up to twelve), bias given and NULL."""
    B, H, W = 3, 5, 7
    for s in (1, 2, 3):
        for c in (8, 24):
            for with_bias in (True, False):
                g = _gen(100 * s + c + int(with_bias))
                x = _randn(g, B, H, W, s * s * c).to(dtype).to(dev)
                bias = _randn(g, s * s * c).to(dev) if with_bias else None
                assert (B * H * s * W * s * (c // 8)) % 256 != 0
                y, buf = _out(dev, (B, s * H, s * W, c), dtype)
                _call("fbsmi_nn_pixel_shuffle", x.data_ptr(), y.data_ptr(), _dt(dtype), B, H, W, c, s, _ptr(bias), _st())
                want = R.pixel_shuffle(R.f64(x), s, R.f64(bias)).float().to(dtype)
                assert _guards_ok(buf)
                assert torch.equal(y, want), (s, c, with_bias)
    for rows, Cx in ((37, 8), (1000, 24), (1, 8), (255, 24)):
        g = _gen(rows + Cx)
        y0 = _randn(g, rows, Cx).to(dtype).to(dev)
        bias = _randn(g, Cx).to(dev)
        assert (rows * (Cx // 8)) % 256 != 0
        y, buf = _out(dev, (rows, Cx), dtype, init=y0)
        _call("fbsmi_nn_bias_add", y.data_ptr(), _dt(dtype), rows, Cx, bias.data_ptr(), _st())
        want = R.bias_add(R.f64(y0), R.f64(bias)).float().to(dtype)
        assert _guards_ok(buf)
        assert torch.equal(y, want), (rows, Cx)
