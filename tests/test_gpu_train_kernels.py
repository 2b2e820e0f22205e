"""GPU: the trainer's kernels (fbs_amd/csrc/fbsmi_train.hip) against tests/train_restate.py -- bit for bit against the
float32 restatements of include/fbsmi.h, within 1e-5 relative of the float64 restatements of the reference's formulas.

Row lengths: both sides of the pair draw (odd D), of the 16-byte path (multiples of 8 or not), one past a workgroup's
share of a row (2048 + 1) and one past the point where a row's 64 workgroups start looping (64 * 2048 + 1)."""
import numpy as np
import pytest
import torch

import train_restate as R
from helpers import bits

pytestmark = pytest.mark.gpu

DS = [1, 2, 3, 63, 64, 65, 257, 784, 2049, 64 * 2048 + 1]
BS = [1, 2, 5]
REL = 1e-5


def _t(a, dev):
    a = np.array(a)                                   # a writable copy: the shared cases are read-only
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)


def _bf16_np(t):
    """a bfloat16 device tensor -> the float32 values it holds"""
    return t.float().cpu().numpy()


@pytest.mark.parametrize("D", DS)
def test_noise_equals_the_restatement(dev, D):
    from fbs_amd.sdes.losses import dsm_noise_batched
    c = R.case(D)
    data = _t(c["data"], dev)
    for B in BS:
        keys, F, sq = _t(c["keys"][:B], dev), _t(c["F"][:B], dev), _t(c["sq"][:B], dev)
        for tag, idx in (("xt", None), ("xt_idx", _t(R.IDX[:B], dev))):
            want = c[tag][:B]
            got = dsm_noise_batched(data, idx, keys, F, sq, torch.float32).cpu().numpy()
            assert np.array_equal(bits(got), bits(want)), (B, tag)
            got16 = _bf16_np(dsm_noise_batched(data, idx, keys, F, sq, torch.bfloat16))
            assert np.array_equal(bits(got16), bits(R.bf16_round_full(want))), (B, tag, "bf16")


def _loss_case(c, B, mode, dt16):
    """(net float32 values, e, x0, xt, idx) of the first B rows; mode 1 reads the gathered layout."""
    net = (c["net16"] if dt16 else c["net"])[:B]
    if mode == 0:
        return net, c["xi"][:B], c["data"][:B], c["xt"][:B], None
    idx = R.IDX[:B]
    xt = c["xt_idx"][:B]
    return net, R.stored_noise_f32(xt, c["data"], idx, c["F"], c["sq"]), c["x0_idx"][:B], xt, idx


def _run_loss(dev, c, B, mode, dt16, rows=slice(None), gc=None):
    from fbs_amd.sdes.losses import dsm_loss_batched
    net, e, x0, xt, idx = _loss_case(c, B, mode, dt16)
    sel = lambda a: np.ascontiguousarray(a[:B][rows])
    nb = sel(net).shape[0]
    F, sq = sel(c["F"]), sel(c["sq"])
    gc = (2.0 * sq.astype(np.float64) / (nb * c["D"])).astype(np.float32) if gc is None else gc
    net_d = _t(sel(net), dev).to(torch.bfloat16 if dt16 else torch.float32)
    if mode == 0:
        loss, dnet, S = dsm_loss_batched(net_d, 0, _t(sel(c["keys"]), dev), None, None, None, None, _t(sq, dev), _t(gc, dev),
                                         want_rows=True)
    else:
        loss, dnet, S = dsm_loss_batched(net_d, 1, None, _t(sel(xt), dev), _t(c["data"], dev), _t(sel(idx), dev), _t(F, dev),
                                         _t(sq, dev), _t(gc, dev), want_rows=True)
    return (loss.cpu().numpy(), dnet.float().cpu().numpy(), S.cpu().numpy(),
            dict(net=sel(net), e=sel(e), x0=sel(x0), xt=sel(xt), F=F, sq=sq, gc=gc, inv=np.float32(1.0 / (nb * c["D"]))))


@pytest.mark.parametrize("dt16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1], ids=["drawn", "stored"])
@pytest.mark.parametrize("D", DS)
def test_loss_equals_the_restatements(dev, D, mode, dt16):
    c = R.case(D)
    for B in BS:
        loss, dnet, S, w = _run_loss(dev, c, B, mode, dt16)
        wS, wloss, wd = R.loss_f32(w["net"], w["e"], w["sq"], w["gc"], w["inv"])
        if dt16:
            wd = R.bf16_round_full(wd)
        assert np.array_equal(bits(S), bits(wS)), B
        assert np.array_equal(bits(loss), bits(np.array([wloss], np.float32))), B
        assert np.array_equal(bits(dnet), bits(wd)), B
        # the reference's formula in float64: mode 0 on the exact x_t = F x0 + sq xi, mode 1 on the stored float32 x_t
        xt64 = (w["F"][:, None].astype(np.float64) * w["x0"] + w["sq"][:, None].astype(np.float64) * w["e"]) if mode == 0 \
            else w["xt"]
        ref = R.loss_f64(w["net"], xt64, w["x0"], w["F"], w["sq"])
        rel = abs(float(loss[0]) - ref) / ref
        print(f"D={D} B={B} mode={mode} bf16={dt16}: loss {float(loss[0]):.9g} float64 {ref:.9g} rel {rel:.2e}")
        assert rel < REL, (B, rel)


@pytest.mark.parametrize("dt16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [3, 64, 784, 2049])
def test_stored_loss_without_idx_reads_row_b_of_data(dev, D, dt16):
    """mode 1 with idx NULL: x0 of row b is row b of data (the other stored-point cases gather through idx)."""
    from fbs_amd.sdes.losses import dsm_loss_batched
    c = R.case(D)
    for B in BS:
        net = (c["net16"] if dt16 else c["net"])[:B]
        F, sq = c["F"][:B], c["sq"][:B]
        gc, inv = (2.0 * sq.astype(np.float64) / (B * D)).astype(np.float32), np.float32(1.0 / (B * D))
        xt = c["xt"][:B]                                              # noised from rows 0 .. B - 1
        e = R.stored_noise_f32(xt, c["data"], None, F, sq)
        loss, dnet, S = dsm_loss_batched(_t(net, dev).to(torch.bfloat16 if dt16 else torch.float32), 1, None, _t(xt, dev),
                                         _t(c["data"], dev), None, _t(F, dev), _t(sq, dev), _t(gc, dev), want_rows=True)
        wS, wloss, wd = R.loss_f32(net, e, sq, gc, inv)
        assert np.array_equal(bits(S.cpu().numpy()), bits(wS)), B
        assert np.array_equal(bits(loss.cpu().numpy()), bits(np.array([wloss], np.float32))), B
        assert np.array_equal(bits(dnet.float().cpu().numpy()), bits(R.bf16_round_full(wd) if dt16 else wd)), B
        ref = R.loss_f64(net, xt, c["data"][:B], F, sq)
        assert abs(float(loss[0]) - ref) / ref < REL, B


@pytest.mark.parametrize("mode", [0, 1], ids=["drawn", "stored"])
@pytest.mark.parametrize("D", [3, 784, 2049, 64 * 2048 + 1])
def test_a_row_does_not_depend_on_the_batch(dev, D, mode):
    """Row b at B = 5 has the bits of row b at B = 1 (given the same gc[b], which carries the batch size): S_b and dnet."""
    c = R.case(D)
    _, dnet5, S5, w5 = _run_loss(dev, c, 5, mode, False)
    for b in (0, 3, 4):
        _, dnet1, S1, _ = _run_loss(dev, c, 5, mode, False, rows=slice(b, b + 1), gc=w5["gc"][b:b + 1])
        assert np.array_equal(bits(S1), bits(S5[b:b + 1])), b
        assert np.array_equal(bits(dnet1), bits(dnet5[b:b + 1])), b


@pytest.mark.parametrize("n", [1, 3, 2047, 2048, 2049, 256 * 2048 + 1, 4096 * 2048 + 2049])
def test_sqnorm_is_the_canonical_tree(dev, oracle, n):
    from fbs_amd.train import sqnorm
    x = np.random.default_rng(n).normal(size=n).astype(np.float32)
    got = sqnorm(_t(x, dev)).cpu().numpy()
    assert np.array_equal(bits(got), bits(np.array([oracle.tree_sum(x * x)], np.float32)))
    xo = _t(np.concatenate([np.zeros(1, np.float32), x]), dev)[1:]       # a base that is not 16-byte aligned
    assert xo.data_ptr() % 16 == 4 and np.array_equal(bits(sqnorm(xo).cpu().numpy()), bits(got))


def _rel(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want)))


@pytest.mark.parametrize("clip", ["off", "active", "inactive"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1025])
def test_adam_ema_step_follows_optax(dev, n, clip):
    """Five consecutive steps, ema_mode 2, 0, 2, 0, 1, each compared from the GPU's own previous state: the update
    p_new - p and m, v, ema within 1e-5 relative of the float64 restatement.  p, m, v, ema are of order one (kept away from
    zero) and g is seeded normal, so nothing compared is a near-cancellation; the learning rate is 4 so that the update is
    of the order of p itself: with a small rate, p_new - p would mostly measure the rounding of p_new to float32."""
    from fbs_amd.train import adam_ema_step, sqnorm
    rng = np.random.default_rng(10 * n + len(clip))
    away = lambda a: (np.sign(a) * (0.5 + np.abs(a))).astype(np.float32)
    p, ema = (away(rng.normal(size=n)) for _ in range(2))
    # |m| in [2, 3]: over the five steps 0.9 m + 0.1 g, with |0.1 g| mostly below 0.4, then never comes near zero
    m = (np.sign(rng.normal(size=n)) * (2.0 + rng.uniform(size=n))).astype(np.float32)
    v = (0.5 + rng.uniform(size=n)).astype(np.float32)
    lr, b1, b2, eps, decay = 4.0, 0.9, 0.999, 1e-8, 0.99
    pd, md, vd, ed = (_t(a, dev) for a in (p, m, v, ema))
    for count, mode in enumerate([2, 0, 2, 0, 1]):      # the copy last: a blend then always starts from an ema of order one
        g = rng.normal(size=n).astype(np.float32)
        gnorm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        max_norm = {"off": None, "active": 0.5 * gnorm, "inactive": 2.0 * gnorm}[clip]
        p0, m0, v0, e0 = (t.cpu().numpy() for t in (pd, md, vd, ed))
        gd = _t(g, dev)
        gn2 = None if max_norm is None else sqnorm(gd)
        adam_ema_step(pd, gd, md, vd, ed, lr, b1, b2, eps, count, gn2, 1.0 if max_norm is None else max_norm, mode, decay)
        g64 = g.astype(np.float64) if max_norm is None else R.clip_by_global_norm_f64(g, float(np.float32(max_norm)))
        if clip == "active":
            assert np.linalg.norm(g64) < 0.51 * gnorm
        if clip == "inactive":
            assert np.array_equal(g64, g.astype(np.float64))
        wp, wm, wv = R.adam_f64(p0, g64, m0, v0, float(np.float32(lr)), float(np.float32(b1)), float(np.float32(b2)),
                                float(np.float32(eps)), count)
        p1, m1, v1, e1 = (t.cpu().numpy() for t in (pd, md, vd, ed))
        assert _rel(p1.astype(np.float64) - p0, wp - p0) < REL, (count, "update")
        assert _rel(m1, wm) < REL and _rel(v1, wv) < REL, count
        we = R.ema_f64(e0, wp, mode, float(np.float32(decay)))
        if mode == 0:
            assert np.array_equal(bits(e1), bits(e0)), count
        elif mode == 1:
            assert np.array_equal(bits(e1), bits(p1)), count
        else:
            assert _rel(e1, we) < REL, count
