"""GPU: the fused Kalman sampler and smoother of the Gaussian SB toy (fbsmi_kf_set_em_forward, SBKalman, SBKalmanSmoother,
samplers.sb_kalman_conditional_sampler / sb_kalman_path_sampler, examples/toy_sb_kf.py) against the float32 restatement
(tests/sb_kf_restate.py) on the same keys, bit for bit; the observation paths against the SB filter sampler's; the law of
the draw; and the fused SB filter's likelihood estimate against the exact value."""
import argparse
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import sb_kf_restate as R
from sb_restate import sb_problem

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64   # floats of NaN on either side of every output
ERR_UNSUPPORTED = -3


def _np(t):
    return t.detach().cpu().numpy()


def _eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    x, y = a.view(np.uint32), b.view(np.uint32)
    bad = np.flatnonzero(x.ravel() != y.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first {bad[:4]}: {a.ravel()[bad[:4]]} vs {b.ravel()[bad[:4]]}"


_MODELS, _WANT = {}, {}


def _setup(du, dv, T, nsub, dev):
    """The SB bridge of tests/test_gpu_sb_filter_sampler.py::_setup: sb_problem cut to D = du + dv coordinates on
    ts = linspace(0, 1, T + 1), y0 and a proper prior, shared by the tests (handles are cached on the bridge)."""
    import fbs_amd
    k = (du, dv, T, nsub)
    if k not in _MODELS:
        D = du + dv
        m0, c0, m1, c1 = sb_problem((D + 1) // 2, 0)
        ts = np.linspace(0.0, 1.0, T + 1)
        br = fbs_amd.GaussianSBBridge(m0[:D], c0[:D, :D], m1[:D], c1[:D, :D], ts, du=du, sig=1.0, nsub=nsub, device=dev)
        rng = np.random.default_rng(1000 * du + dv)
        y0 = rng.normal(size=dv).astype(f32)
        A = rng.normal(size=(du, du))
        prior = (rng.normal(size=du).astype(f32), np.linalg.cholesky(A @ A.T / du + 0.5 * np.eye(du)).astype(f32))
        _MODELS[k] = (br, ts, y0, prior)
    return _MODELS[k]


def _keys(O, B, seed=41):
    return O.split(O.PRNGKey(seed), 17)[:B]


def _want(O, case, br, y0, prior, nkeys):
    """The restatement's batch on the case's first `nkeys` keys, computed once per (case, prior) at the largest batch the
    tests use and shared: sample b depends on keys[b] only."""
    from fbs_amd.gaussian_sb import sb_kalman_model, sb_kalman_smoother_model
    k = (case, prior is not None)
    if k not in _WANT or _WANT[k]["vs"].shape[0] < nkeys:
        kf, ks = sb_kalman_model(br), sb_kalman_smoother_model(br)
        h = br.em_host
        _WANT[k] = R.want(O, (h["M"], h["c"], h["ddt"], h["s"], br.nsub), kf.host, ks.host, kf.tables64, _keys(O, nkeys), y0, prior)
    return {n: v[:nkeys] for n, v in _WANT[k].items()}


def _guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _untouched(buf, what):
    b = _np(buf)
    assert np.isnan(b[:GUARD]).all() and np.isnan(b[-GUARD:]).all(), f"{what}: a guard band was written"


def _call_guarded(br, keys, y0, dev, shapes, run):
    from fbs_amd import ops
    kt = torch.from_numpy(np.asarray(keys, np.uint32).view(np.int32).copy()).to(dev)
    y0t = torch.from_numpy(np.asarray(y0, f32)).to(dev)
    bufs = {k: _guarded(int(np.prod(s)), dev) for k, s in shapes.items()}
    run(kt, y0t, lambda k: bufs[k][1].data_ptr(), ops._stream())
    torch.cuda.synchronize()
    for k in shapes:
        _untouched(bufs[k][0], k)
    return {k: _np(bufs[k][1]).reshape(shapes[k]) for k in shapes}


def _sample_guarded(h, br, keys, y0, dev):
    """fbsmi_kf_sample and both views through the C ABI into guarded buffers -> dict of numpy arrays."""
    from fbs_amd import _lib
    B = len(keys)
    shapes = dict(samples=(B, br.du), means=(B, br.du), loglik=(B,), vs=(B, br.T + 1, br.dv), m_=(B, br.du))

    def run(kt, y0t, ptr, st):
        _lib.call("fbsmi_kf_sample", h.h, kt.data_ptr(), y0t.data_ptr(), ptr("samples"), ptr("means"), ptr("loglik"), st)
        _lib.call("fbsmi_kf_view", h.h, 0, ptr("vs"), None, st)
        _lib.call("fbsmi_kf_view", h.h, 1, ptr("m_"), None, st)

    return _call_guarded(br, keys, y0, dev, shapes, run)


def _paths_guarded(h, br, keys, y0, dev):
    """fbsmi_kfs_sample and its three views through the C ABI into guarded buffers -> dict of numpy arrays."""
    from fbs_amd import _lib
    B = len(keys)
    shapes = dict(paths=(B, br.T + 1, br.du), loglik=(B,), vs=(B, br.T + 1, br.dv), m=(B, br.T + 1, br.du), r=(B, br.T, br.dv))

    def run(kt, y0t, ptr, st):
        _lib.call("fbsmi_kfs_sample", h.h, kt.data_ptr(), y0t.data_ptr(), ptr("paths"), ptr("loglik"), st)
        for which, k in enumerate(("vs", "m", "r")):
            _lib.call("fbsmi_kfs_view", h.h, which, ptr(k), None, st)

    return _call_guarded(br, keys, y0, dev, shapes, run)


# ---- 1. bit equality ----------------------------------------------------------------------------------------------------
# (du, dv, T, nsub, batch sizes, priors): one sample, a full tile of k_kf and one past it; du != dv both ways; D = 31, 32,
# 33 on either side of em_path_run's M chunk; one wave of the front against two; four waves with two workgroups of k_kf,
# one of them with a single live sample; T = 1 and nsub = 1; T = 1025, one past the intervals whose keys stay in LDS.
PARITY = [(1, 1, 6, 3, (1, 16, 17), (False,)),
          (3, 3, 20, 10, (3,), (False, True)),
          (5, 7, 8, 4, (2,), (False,)),
          (7, 5, 8, 4, (2,), (False,)),
          (16, 15, 4, 2, (2,), (False,)),
          (16, 16, 4, 2, (2,), (False,)),
          (17, 16, 4, 2, (2,), (False,)),
          (32, 32, 4, 2, (2,), (False,)),
          (33, 32, 4, 3, (2,), (False,)),
          (128, 128, 3, 2, (17,), (False,)),
          (3, 3, 1, 1, (2,), (False,)),
          (1, 1, 1025, 1, (2,), (False,))]
PARITY = [(du, dv, T, nsub, B, p) for du, dv, T, nsub, Bs, ps in PARITY for B in Bs for p in ps]


@pytest.mark.parametrize("case", PARITY, ids=["-".join(str(x) for x in c[:5]) + f"-{'proper' if c[5] else 'heuristic'}"
                                             for c in PARITY])
def test_bit_equality_with_the_restatement(case, oracle, dev):
    du, dv, T, nsub, B, proper = case
    br, ts, y0, prior = _setup(du, dv, T, nsub, dev)
    prior = prior if proper else None
    want = _want(oracle, case[:4], br, y0, prior, max(B, 17 if case[:4] == (1, 1, 6, 3) else B))
    keys = _keys(oracle, B)
    h = br.sb_kalman_handle(B, prior)
    assert h is br.sb_kalman_handle(B, prior) and h.C == B, "handles are cached by the size and the prior's bytes"
    got = _sample_guarded(h, br, keys, y0, dev)
    for k in ("vs", "m_", "means", "loglik", "samples"):
        _eq(got[k], want[k][:B], f"{k} {case}")
    assert np.isfinite(got["samples"]).all() and np.isfinite(got["loglik"]).all()
    hs = br.sb_kalman_smoother_handle(B, prior)
    assert hs is br.sb_kalman_smoother_handle(B, prior) and hs.C == B
    gs = _paths_guarded(hs, br, keys, y0, dev)
    for k in ("vs", "m", "r", "paths"):
        _eq(gs[k], want[k][:B], f"smoother {k} {case}")
    _eq(gs["loglik"], want["sloglik"][:B], f"smoother loglik {case}")
    _eq(gs["paths"][:, T], got["samples"], "paths[:, T] against the sampler's draw")
    _eq(gs["loglik"], got["loglik"], "the smoother's loglik against the sampler's")


# ---- 2. the observation paths are the filter sampler's ---------------------------------------------------------------------
@pytest.mark.parametrize("proper", [False, True])
def test_same_observation_paths_as_the_filter_sampler(proper, oracle, dev):
    br, ts, y0, prior = _setup(3, 3, 20, 10, dev)
    prior = prior if proper else None
    B = 5
    keys = _keys(oracle, B, 43)
    fs = br.sb_filter_sampler_handle(64, "stratified", B, prior)
    fs.sample(keys, y0)
    fvs = _np(fs.views()["vs"])
    h = br.sb_kalman_handle(B, prior)
    h.sample(keys, y0)
    _eq(_np(h.views()["vs"]), fvs, "vs of the Kalman handle against the filter sampler's")
    hs = br.sb_kalman_smoother_handle(B, prior)
    hs.sample(keys, y0)
    _eq(_np(hs.views()["vs"]), fvs, "vs of the smoother handle against the filter sampler's")


# ---- 3. filter(vs) against sample, the Python layer, ragged batches -----------------------------------------------------------
@pytest.mark.parametrize("proper", [False, True])
def test_sample_then_filter_and_ragged_batches(proper, oracle, dev):
    br, ts, y0, prior = _setup(3, 3, 20, 10, dev)
    prior = prior if proper else None
    B = 5
    keys = _keys(oracle, B)
    want = _want(oracle, (3, 3, 20, 10), br, y0, prior, B)
    h = br.sb_kalman_handle(B, prior)
    samples, means, ll = h.sample(keys, y0, return_moments=True)
    _eq(_np(samples), want["samples"], "samples")
    v = h.views()
    _eq(_np(v["vs"]), want["vs"], "vs view")
    fm, fl = h.filter(v["vs"])
    _eq(_np(fm), _np(means), "filter means on the sampled paths")
    _eq(_np(fl), _np(ll), "filter loglik on the sampled paths")
    _eq(_np(h.views()["m_"]), want["m_"], "m_ view after filter")
    # a ragged batch runs on the bridge's handle of that size and the same prior; one key of shape (2,)
    part = h.sample(keys[:3], y0)
    assert part.shape == (3, br.du) and h.views()["vs"].shape[0] == 3 and h._last is br.sb_kalman_handle(3, prior)
    _eq(_np(part), want["samples"][:3], "ragged samples")
    _eq(_np(h.sample(keys[4], y0)), want["samples"][4:5], "one key")
    with pytest.raises(ValueError):
        h.sample(_keys(oracle, B + 1), y0)
    assert h.cov_T.shape == (br.du, br.du) and h.cov_T.dtype == np.float64
    # the smoother alike
    hs = br.sb_kalman_smoother_handle(B, prior)
    paths, sl = hs.sample(keys, y0, return_loglik=True)
    _eq(_np(paths), want["paths"], "paths")
    _eq(_np(sl), _np(ll), "smoother loglik")
    on = hs.sample_on(keys, hs.views()["vs"])
    _eq(_np(on), want["paths"], "sample_on the sampled paths")
    part = hs.sample(keys[:3], y0)
    assert part.shape == (3, br.T + 1, br.du) and hs._last is br.sb_kalman_smoother_handle(3, prior)
    _eq(_np(part), want["paths"][:3], "ragged paths")
    _eq(_np(hs.sample(keys[4], y0)), want["paths"][4:5], "one key: path")
    with pytest.raises(ValueError):
        hs.sample(_keys(oracle, B + 1), y0)
    assert hs.cov_s.shape == (br.T + 1, br.du, br.du)


def test_the_prior_is_part_of_the_cache_key(dev):
    br, ts, y0, prior = _setup(3, 3, 20, 10, dev)
    other = (prior[0] + f32(1), prior[1])
    for make in (br.sb_kalman_handle, br.sb_kalman_smoother_handle):
        a, b = make(2), make(2, prior)
        assert a is not b and make(2, other) is not b and a.prior is None
        assert make(2, (prior[0].astype(np.float64), prior[1].copy())) is b
    assert br.sb_kalman_handle(2) is not br.sb_kalman_smoother_handle(2)


# ---- 4. chunking ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proper", [False, True])
def test_chunking_does_not_change_results(proper, oracle, dev):
    from fbs_amd import samplers
    br, ts, y0, prior = _setup(3, 3, 20, 10, dev)
    prior = prior if proper else None
    keys = _keys(oracle, 5)
    want = _want(oracle, (3, 3, 20, 10), br, y0, prior, 5)
    one = samplers.sb_kalman_conditional_sampler(keys, y0, br, prior, return_moments=True)
    two = samplers.sb_kalman_conditional_sampler(keys, y0, br, prior, return_moments=True, _bound=2 * (br.T + 1) * br.dv)
    for a, b, k in zip(one, two, ("samples", "means", "loglik")):        # chunks of 2, 2, 1
        _eq(_np(b), _np(a), f"chunked {k}")
        _eq(_np(a), want[k], k)
    assert samplers.sb_kalman_conditional_sampler(keys[:2], y0, br, prior).shape == (2, br.du)
    p1 = samplers.sb_kalman_path_sampler(keys, y0, br, prior, return_moments=True)
    p2 = samplers.sb_kalman_path_sampler(keys, y0, br, prior, return_moments=True, _bound=2 * (br.T + 1) * br.dv)
    for a, b, k in zip(p1, p2, ("paths", "smoothed means", "loglik")):
        _eq(_np(b), _np(a), f"chunked {k}")
    _eq(_np(p1[0]), want["paths"], "paths")
    _eq(_np(p1[2]), want["loglik"], "path sampler loglik")
    assert p1[1].shape == (5, br.T + 1, br.du)
    _eq(_np(p1[1][:, br.T]), want["means"], "the smoothed mean at T is the filtering mean")
    pk = None if prior is None else (prior[0].tobytes(), prior[1].tobytes())
    for size in (5, 2, 1):
        assert ("sb_kalman", size, pk) in br._sweeps and ("sb_kalman_smoother", size, pk) in br._sweeps


# ---- 5. the law of the draw ---------------------------------------------------------------------------------------------------
def test_law_of_the_draw(oracle, dev):
    from fbs_amd.gaussian_sb import sb_kalman_model
    br, ts, y0, prior = _setup(3, 3, 20, 10, dev)
    B = 4096
    keys = oracle.split(oracle.PRNGKey(52), B)
    samples, means, ll = br.sb_kalman_handle(B).sample(keys, y0, return_moments=True)
    Lt = sb_kalman_model(br).tables64["Lt"]
    resid = _np(samples).astype(np.float64) - _np(means).astype(np.float64)             # = zz @ chol = Lt^T zz
    w = np.linalg.solve(Lt.T, resid.T).T                                                # Lt^{-T} (x - mean)
    mean, var = w.mean(axis=0), w.var(axis=0, ddof=1)
    print(f"whitened residuals, B = {B}: mean {mean}, variance {var}; bounds {4 / np.sqrt(B):.4f}, {4 * np.sqrt(2 / B):.4f}")
    assert np.all(np.abs(mean) <= 4 / np.sqrt(B)) and np.all(np.abs(var - 1) <= 4 * np.sqrt(2 / B))
    assert np.isfinite(_np(ll)).all()


# ---- 6. the fused SB filter's likelihood estimate against the exact value ----------------------------------------------------
def test_fused_filter_likelihood_against_the_exact_value(oracle, dev):
    br, ts, y0, prior = _setup(1, 1, 6, 3, dev)
    N, B = 4096, 64
    keys = oracle.split(oracle.PRNGKey(53), B)
    fs = br.sb_filter_sampler_handle(N, "stratified", B)
    _, nell = fs.sample(keys, y0, return_nell=True)
    means, loglik = br.sb_kalman_handle(B).filter(fs.views()["vs"])
    d = -_np(nell).astype(np.float64) - _np(loglik).astype(np.float64)
    se = d.std(ddof=1) / np.sqrt(B)
    print(f"fused SB filter N = {N}, B = {B}: mean(-nell - loglik) = {d.mean():+.2e}, sd {d.std(ddof=1):.4f}, standard error {se:.4f}")
    assert abs(d.mean()) <= 4 * se


# ---- 7. refusals of the C ABI that need a device --------------------------------------------------------------------------------
def test_c_level_refusals(oracle, dev):
    import fbs_amd
    from fbs_amd import _lib, ops
    from fbs_amd.gaussian_sb import sb_kalman_model, sb_kalman_smoother_model
    from fbs_amd.sdes import StationaryConstLinearSDE
    from helpers import toy_2d
    sb, ts, y0, prior = _setup(3, 3, 8, 3, dev)
    L = _lib.lib()
    kt = torch.from_numpy(np.asarray(_keys(oracle, 2), np.uint32).view(np.int32).copy()).to(dev)
    y0t = torch.from_numpy(y0).to(dev)
    out = torch.empty((2, sb.T + 1, sb.du), dtype=torch.float32, device=dev)
    # an SB-table handle without the setter answers as before
    h = C.c_void_p()
    _lib.call("fbsmi_kf_create", C.byref(sb_kalman_model(sb)), 2, C.byref(h))
    try:
        assert L.fbsmi_kf_sample(h, kt.data_ptr(), y0t.data_ptr(), out.data_ptr(), None, None, ops._stream()) == ERR_UNSUPPORTED
        assert b"kf_sample" in L.fbsmi_last_error() and b"forward transition" in L.fbsmi_last_error()
    finally:
        L.fbsmi_kf_destroy(h)
    hs = C.c_void_p()
    _lib.call("fbsmi_kfs_create", C.byref(sb_kalman_smoother_model(sb)), 2, C.byref(hs))
    try:
        assert L.fbsmi_kfs_sample(hs, kt.data_ptr(), y0t.data_ptr(), out.data_ptr(), None, ops._stream()) == ERR_UNSUPPORTED
        assert b"kfs_sample" in L.fbsmi_last_error()
    finally:
        L.fbsmi_kfs_destroy(hs)
    # a handle with an exact forward transition (F, sqQ not all zero) refuses the setter
    toy = toy_2d()
    lg = fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(-0.5, 1.0), np.linspace(0, 2, 9), 1,
                                      device=dev)
    assert not hasattr(lg, "sb_kalman_handle")
    for handle, fn, name in ((lg.kalman_handle(2), L.fbsmi_kf_set_em_forward, b"kf_set_em_forward"),
                             (lg.kalman_smoother_handle(2), L.fbsmi_kfs_set_em_forward, b"kf_set_em_forward")):
        assert fn(handle.h, C.byref(sb.em_struct), None, None) == ERR_UNSUPPORTED and name in L.fbsmi_last_error()
    with pytest.raises(NotImplementedError, match="exact forward transition"):
        _lib.call("fbsmi_kf_set_em_forward", lg.kalman_handle(2).h, C.byref(sb.em_struct), None, None)
    # and the refused handle still serves its own model
    assert lg.kalman_handle(2).sample(_keys(oracle, 2), toy["y0"]).shape == (2, 1)
    # the inherited handles keep refusing the SB bridge
    with pytest.raises(NotImplementedError, match="GaussianSBBridge"):
        sb.kalman_handle(1)
    with pytest.raises(NotImplementedError, match="GaussianSBBridge"):
        sb.kalman_smoother_handle(1)


# ---- 8. the driver ----------------------------------------------------------------------------------------------------------------
def test_toy_sb_kf_driver(tmp_path, dev):
    from fbs_amd import ops, samplers
    from fbs_amd.metrics import tabulate
    ex = os.path.join(ROOT, "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    spec = importlib.util.spec_from_file_location("toy_sb_kf_driver", os.path.join(ex, "toy_sb_kf.py"))
    tk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tk)
    for x0 in ("heuristic", "proper"):
        argv = ["--d", "3", "--nsamples", "40", "--x0", x0, "--quiet", "--outdir", str(tmp_path)]
        samples, gp_mean, gp_cov = tk.main(argv + ["--batch", "16"])
        assert samples.shape == (40, 3) and np.isfinite(samples).all()
        path = os.path.join(str(tmp_path), f"kf-{x0}-666.npz")
        saved = np.load(path)
        assert set(saved.files) == {"samples", "gp_mean", "gp_cov"}
        _eq(saved["samples"], samples, "saved samples")
        stats = tabulate([path])
        assert stats and all(np.isfinite(m) for m, s in stats.values())
        g = tk.sb_setting(argparse.Namespace(id=666, d=3, fused=True), dev)
        key, subkeys = g.key, []
        for _ in range(40):
            key, subkey = ops.split(key)
            subkeys.append(subkey)
        prior = (g.gp_mean, np.linalg.cholesky(g.gp_cov)) if x0 == "proper" else None
        direct = samplers.sb_kalman_conditional_sampler(np.stack(subkeys), g.y0, g.bridge, x0_prior=prior)
        _eq(samples, _np(direct), f"driver samples ({x0})")
        smoothed = tk.main(argv + ["--batch", "40", "--smoother"])[0]
        _eq(smoothed, samples, f"--smoother draws the same samples ({x0})")
        assert set(np.load(os.path.join(str(tmp_path), f"kfs-{x0}-666.npz")).files) == {"samples", "gp_mean", "gp_cov", "path_mean",
                                                                                        "path_var"}
