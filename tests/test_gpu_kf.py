"""GPU: the fused Kalman-filter conditional sampler (fbsmi_kf_*, LGKalman, samplers.kalman_conditional_sampler,
examples/toy_kf.py) against the float32 restatement of the header's specification (tests/kf_restate.py) on the same keys,
bit for bit; the law of the draw; and the fused bootstrap filter's likelihood estimate against the exact value."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from helpers import toy_gp, toy_2d, toy_4d, toy_31, oracle_model_from
import kf_restate as R
from test_kf_tables import LADDER

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64   # floats of NaN on either side of every output


def _np(t):
    return t.detach().cpu().numpy()


def _eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    x, y = a.view(np.uint32), b.view(np.uint32)
    bad = np.flatnonzero(x.ravel() != y.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first {bad[:4]}: {a.ravel()[bad[:4]]} vs {b.ravel()[bad[:4]]}"


MODELS = {"2d": (toy_2d, 30), "4d": (toy_4d, 30), "31": (toy_31, 30), "gp17": (lambda: toy_gp(17), 10),
          "gp20v7": (lambda: toy_gp(20, dv=7), 10), "gp128": (lambda: toy_gp(128), 4), "gp100": (lambda: toy_gp(100), 200)}
MODELS.update({name: (make, 6) for name, make in LADDER.items()})      # the width ladder of tests/test_kf_tables.py
_BRIDGES, _WANT = {}, {}
NKEYS = 33


def _setup(name, dev):
    """The bridge of a named toy on ts = linspace(0, 2, T + 1) (shared by the tests: handles are cached on it)."""
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    if name not in _BRIDGES:
        make, T = MODELS[name]
        toy = make()
        ts = np.linspace(0, 2, T + 1)
        br = fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(-0.5, 1.0), ts, toy["du"], device=dev)
        _BRIDGES[name] = (toy, ts, br)
    return _BRIDGES[name]


def _keys(O, name):
    return O.split(O.PRNGKey(51), NKEYS)[:17 if name == "gp100" else NKEYS]


def _want(O, name, br, toy):
    """The restatement's batch on the model's keys, computed once and shared: sample b depends on keys[b] only."""
    if name not in _WANT:
        from fbs_amd.lg_kalman import kalman_model
        st = kalman_model(br)
        _WANT[name] = R.want(O, oracle_model_from(O, br), st.host, st.tables64, _keys(O, name), toy["y0"])
    return _WANT[name]


def _guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _untouched(buf, what):
    b = _np(buf)
    assert np.isnan(b[:GUARD]).all() and np.isnan(b[-GUARD:]).all(), f"{what}: a guard band was written"


def _sample_guarded(h, br, keys, y0, dev):
    """fbsmi_kf_sample and both views through the C ABI into guarded buffers -> dict of numpy arrays."""
    from fbs_amd import _lib, ops
    B = len(keys)
    kt = torch.from_numpy(np.asarray(keys, np.uint32).view(np.int32).copy()).to(dev)
    y0t = torch.from_numpy(np.asarray(y0, f32)).to(dev)
    shapes = dict(samples=(B, br.du), means=(B, br.du), loglik=(B,), vs=(B, br.T + 1, br.dv), m_=(B, br.du))
    bufs = {k: _guarded(int(np.prod(s)), dev) for k, s in shapes.items()}
    ptr = lambda k: bufs[k][1].data_ptr()
    _lib.call("fbsmi_kf_sample", h.h, kt.data_ptr(), y0t.data_ptr(), ptr("samples"), ptr("means"), ptr("loglik"), ops._stream())
    _lib.call("fbsmi_kf_view", h.h, 0, ptr("vs"), None, ops._stream())
    _lib.call("fbsmi_kf_view", h.h, 1, ptr("m_"), None, ops._stream())
    torch.cuda.synchronize()
    for k in shapes:
        _untouched(bufs[k][0], k)
    return {k: _np(bufs[k][1]).reshape(shapes[k]) for k in shapes}


# ---- 1. bit equality ----------------------------------------------------------------------------------------------------
PARITY = [(m, B) for m in ("2d", "4d", "31", "gp17", "gp20v7", "gp128") for B in (1, 15, 16, 17, 33)] + [("gp100", 17)]
# NQu = NQv = 1, 3, 4 (63, 64), 5 (65, 80), 6, 7 and the pairs (8, 1), (5, 3), (1, 3), (3, 5), (2, 6), (1, 8): every count
# 3..6 on either side, both "second row tile on some waves only" flags mixed, dv > du, the fallback loads (row tile 0, the
# last column group again) with NQu != NQv; one workgroup with one live sample, and two
PARITY += [(m, B) for m in LADDER for B in (1, 17)]


@pytest.mark.parametrize("name,B", PARITY, ids=[f"{m}-B{B}" for m, B in PARITY])
def test_bit_equality_with_the_restatement(name, B, oracle, dev):
    toy, ts, br = _setup(name, dev)
    want = _want(oracle, name, br, toy)
    h = br.kalman_handle(B)
    assert h is br.kalman_handle(B) and h.C == B
    got = _sample_guarded(h, br, _keys(oracle, name)[:B], toy["y0"], dev)
    for k in ("vs", "m_", "means", "loglik", "samples"):
        _eq(got[k], want[k][:B], f"{k} {name} B={B}")
    assert np.isfinite(got["samples"]).all() and np.isfinite(got["loglik"]).all()


# ---- 2. filter(vs) against sample, the Python layer, ragged batches -----------------------------------------------------------
@pytest.mark.parametrize("name", ["4d", "gp20v7", "gp80v33", "rand33v80"])
def test_filter_on_the_sampled_paths_and_ragged_batches(name, oracle, dev):
    from fbs_amd import _lib, ops
    toy, ts, br = _setup(name, dev)
    want = _want(oracle, name, br, toy)
    keys = _keys(oracle, name)
    h = br.kalman_handle(17)
    samples, means, ll = h.sample(keys[:17], toy["y0"], return_moments=True)
    _eq(_np(samples), want["samples"][:17], "samples")
    v = h.views()
    _eq(_np(v["vs"]), want["vs"][:17], "vs view")
    # the filter alone on those paths, through guarded outputs
    mb, lb = _guarded(17 * br.du, dev), _guarded(17, dev)
    _lib.call("fbsmi_kf_filter", h.h, v["vs"].data_ptr(), mb[1].data_ptr(), lb[1].data_ptr(), ops._stream())
    torch.cuda.synchronize()
    _untouched(mb[0], "filter means")
    _untouched(lb[0], "filter loglik")
    _eq(_np(mb[1]).reshape(17, br.du), _np(means), "filter means")
    _eq(_np(lb[1]), _np(ll), "filter loglik")
    fm, fl = h.filter(v["vs"])
    _eq(_np(fm), _np(means), "LGKalman.filter means")
    _eq(_np(fl), _np(ll), "LGKalman.filter loglik")
    _eq(_np(h.views()["m_"]), want["m_"][:17], "m_ view after filter")
    # a ragged batch runs on the bridge's handle of that size; one key of shape (2,); one path of shape (T+1, dv)
    part = h.sample(keys[:3], toy["y0"])
    assert part.shape == (3, br.du) and h.views()["vs"].shape[0] == 3 and ("kalman", 3) in br._sweeps
    _eq(_np(part), want["samples"][:3], "ragged samples")
    _eq(_np(h.sample(keys[4], toy["y0"])), want["samples"][4:5], "one key")
    pm, pl = h.filter(v["vs"][5])
    _eq(_np(pm), want["means"][5:6], "one path: mean")
    _eq(_np(pl), want["loglik"][5:6], "one path: loglik")
    with pytest.raises(ValueError):
        h.sample(keys[:18], toy["y0"])
    assert h.cov_T.shape == (br.du, br.du) and h.cov_T.dtype == np.float64


# ---- 3. chunking ------------------------------------------------------------------------------------------------------------
def test_chunking_does_not_change_results(oracle, dev):
    from fbs_amd import samplers
    toy, ts, br = _setup("4d", dev)
    want = _want(oracle, "4d", br, toy)
    keys = _keys(oracle, "4d")
    one = samplers.kalman_conditional_sampler(keys, toy["y0"], br, return_moments=True)
    two = samplers.kalman_conditional_sampler(keys, toy["y0"], br, return_moments=True, _bound=16 * (br.T + 1) * br.dv)
    assert ("kalman", 33) in br._sweeps and ("kalman", 16) in br._sweeps and ("kalman", 1) in br._sweeps   # 16, 16, 1
    for a, b, k in zip(one, two, ("samples", "means", "loglik")):
        assert a.shape == want[k].shape
        _eq(_np(b), _np(a), f"chunked {k}")
        _eq(_np(a), want[k], k)
    assert samplers.kalman_conditional_sampler(keys[:2], toy["y0"], br).shape == (2, br.du)


# ---- 4. the law of the draw ---------------------------------------------------------------------------------------------------
def test_law_of_the_draw(oracle, dev):
    toy, ts, br = _setup("4d", dev)
    B = 4096
    keys = oracle.split(oracle.PRNGKey(52), B)
    h = br.kalman_handle(B)
    samples, means, ll = h.sample(keys, toy["y0"], return_moments=True)
    from fbs_amd.lg_kalman import kalman_model
    Lt = kalman_model(br).tables64["Lt"]
    resid = (_np(samples).astype(np.float64) - _np(means).astype(np.float64))          # = zz @ chol = Lt^T zz
    w = np.linalg.solve(Lt.T, resid.T).T                                                # Lt^{-T} (x - mean)
    mean, var = w.mean(axis=0), w.var(axis=0, ddof=1)
    print(f"whitened residuals, B = {B}: mean {mean}, variance {var}; bounds {4 / np.sqrt(B):.4f}, {4 * np.sqrt(2 / B):.4f}")
    assert np.all(np.abs(mean) <= 4 / np.sqrt(B)) and np.all(np.abs(var - 1) <= 4 * np.sqrt(2 / B))
    assert np.isfinite(_np(ll)).all()


# ---- 5. the fused filter's likelihood estimate against the exact value -----------------------------------------------------------
def test_fused_filter_likelihood_against_the_exact_value(oracle, dev):
    from fbs_amd import samplers
    toy, ts, br = _setup("2d", dev)
    N, B = 4096, 64
    keys = oracle.split(oracle.PRNGKey(53), B)
    _, nell = samplers.filter_conditional_sampler(keys, toy["y0"], ts, br.fwd_ys_sampler, br.ref_sampler,
                                                  br.transition_sampler, br.likelihood_logpdf, N, samplers.stratified,
                                                  return_nell=True)
    vs = br.filter_sampler_handle(N, "stratified", B).views()["vs"]
    means, loglik = br.kalman_handle(B).filter(vs)
    d = -_np(nell).astype(np.float64) - _np(loglik).astype(np.float64)
    se = d.std(ddof=1) / np.sqrt(B)
    print(f"fused filter N = {N}, B = {B}: mean(-nell - loglik) = {d.mean():+.2e}, sd {d.std(ddof=1):.4f}, standard error {se:.4f}")
    assert abs(d.mean()) <= 4 * se


# ---- 6. refusals that need a device ---------------------------------------------------------------------------------------------
def test_gaussian_sb_bridge_is_refused(dev):
    import fbs_amd
    rng = np.random.default_rng(0)
    A = rng.normal(size=(2, 2))
    sb = fbs_amd.GaussianSBBridge(np.zeros(2), np.eye(2), np.array([0.5, -0.5]), A @ A.T + np.eye(2), np.linspace(0, 1, 11),
                                  du=1, device=dev)
    with pytest.raises(NotImplementedError, match="GaussianSBBridge"):
        sb.kalman_handle(1)
    with pytest.raises(NotImplementedError, match="GaussianSBBridge"):
        fbs_amd.samplers.kalman_conditional_sampler(np.zeros((1, 2), np.uint32), np.zeros(1, f32), sb)


# ---- 7. the driver ----------------------------------------------------------------------------------------------------------------
def test_toy_kf_driver(tmp_path, oracle, dev):
    from fbs_amd import ops, samplers
    from fbs_amd.metrics import tabulate
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        spec = importlib.util.spec_from_file_location("toy_kf_driver", os.path.join(ROOT, "examples", "toy_kf.py"))
        tk = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tk)
        from _gp_toy import gp_setting
    finally:
        sys.path.remove(os.path.join(ROOT, "examples"))
    samples, gp_mean, gp_cov = tk.main(["--d", "4", "--nsamples", "40", "--batch", "16", "--quiet", "--outdir", str(tmp_path)])
    assert samples.shape == (40, 4) and np.isfinite(samples).all()
    path = os.path.join(str(tmp_path), "kf-const-666.npz")
    saved = np.load(path)
    assert set(saved.files) == {"samples", "gp_mean", "gp_cov"}
    _eq(saved["samples"], samples, "saved samples")
    stats = tabulate([path])
    assert stats and all(np.isfinite(m) for m, s in stats.values())
    g = gp_setting(tk.argparse.Namespace(id=666, d=4, sde="const"), dev)
    key, subkeys = g["key"], []
    for _ in range(40):
        key, subkey = ops.split(key)
        subkeys.append(subkey)
    direct = samplers.kalman_conditional_sampler(np.stack(subkeys), g["y0_t"], g["bridge"])
    _eq(samples, _np(direct), "driver samples")
