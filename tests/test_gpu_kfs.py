"""GPU: the fused Kalman smoother and path sampler (fbsmi_kfs_*, LGKalmanSmoother, samplers.kalman_path_sampler,
gibbs_init(method='kalman'), examples/toy_kf.py --smoother) against the float32 restatement of the header's specification
(tests/kfs_restate.py) on the same keys, bit for bit; parity with the filter engine; the law of the draw; and the fused
particle smoother against the exact smoothing law."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from helpers import toy_31, toy_4d, toy_gp, oracle_model_from
import kfs_restate as KR
from test_gpu_kf import MODELS, _eq, _guarded, _keys, _np, _setup, _untouched
from test_kf_tables import LADDER
from test_kfs_tables import check_whitened_paths, particle_smoother_inputs

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# T = 1 (no step behind the first, nothing to ping-pong) and T * du odd (the padded random_bits layout of xi)
MODELS.update({"4d-T1": (toy_4d, 1), "gp17-T1": (lambda: toy_gp(17), 1), "31-T5": (toy_31, 5)})
_WANT = {}


def _want(O, name, br, toy):
    """The restatement's batch on the model's keys -- sample, and smooth on the sampled vs -- computed once and shared."""
    if name not in _WANT:
        from fbs_amd.lg_kalman import kalman_smoother_model
        st = kalman_smoother_model(br)
        kf = st.kf_struct
        w = KR.want(O, oracle_model_from(O, br), kf.host, st.host, kf.tables64, _keys(O, name), toy["y0"])
        w["smeans"] = KR.smooth_restated(kf.host, st.host, kf.tables64, w["vs"])["smeans"]
        _WANT[name] = w
    return _WANT[name]


def _call_guarded(h, br, entry, keys, arg, dev):
    """One fbsmi_kfs_* call and the three views through the C ABI into guarded buffers -> dict of numpy arrays.
    entry 'sample' (arg y0), 'sample_on' (arg vs) or 'smooth' (arg vs, keys unused)."""
    from fbs_amd import _lib, ops
    B, T = h.C, br.T
    at = torch.from_numpy(np.ascontiguousarray(np.asarray(arg, f32))).to(dev)
    shapes = dict(paths=(B, T + 1, br.du), loglik=(B,), vs=(B, T + 1, br.dv), m=(B, T + 1, br.du), r=(B, T, br.dv))
    bufs = {k: _guarded(int(np.prod(s)), dev) for k, s in shapes.items()}
    ptr = lambda k: bufs[k][1].data_ptr()
    if entry == "smooth":
        _lib.call("fbsmi_kfs_smooth", h.h, at.data_ptr(), ptr("paths"), ptr("loglik"), ops._stream())
    else:
        kt = torch.from_numpy(np.asarray(keys, np.uint32).view(np.int32).copy()).to(dev)
        _lib.call("fbsmi_kfs_" + entry, h.h, kt.data_ptr(), at.data_ptr(), ptr("paths"), ptr("loglik"), ops._stream())
    for which, k in enumerate(("vs", "m", "r")):
        _lib.call("fbsmi_kfs_view", h.h, which, ptr(k), None, ops._stream())
    torch.cuda.synchronize()
    for k in shapes:
        _untouched(bufs[k][0], f"{entry} {k}")
    return {k: _np(bufs[k][1]).reshape(shapes[k]) for k in shapes}


# ---- 1. bit equality ----------------------------------------------------------------------------------------------------
PARITY = [(m, B) for m in ("2d", "4d", "31", "gp17", "gp20v7", "gp128") for B in (1, 15, 16, 17, 33)] + [("gp100", 17)]
PARITY += [(m, B) for m in LADDER for B in (1, 17)]
PARITY += [("4d-T1", 17), ("gp17-T1", 17), ("31-T5", 17)]


@pytest.mark.parametrize("name,B", PARITY, ids=[f"{m}-B{B}" for m, B in PARITY])
def test_bit_equality_with_the_restatement(name, B, oracle, dev):
    toy, ts, br = _setup(name, dev)
    want = _want(oracle, name, br, toy)
    keys = _keys(oracle, name)[:B]
    h = br.kalman_smoother_handle(B)
    assert h is br.kalman_smoother_handle(B) and h.C == B
    got = _call_guarded(h, br, "sample", keys, toy["y0"], dev)
    for k in ("vs", "m", "r", "loglik", "paths"):
        _eq(got[k], want[k][:B], f"sample: {k} {name} B={B}")
    assert np.isfinite(got["paths"]).all() and np.isfinite(got["loglik"]).all()
    on = _call_guarded(h, br, "sample_on", keys, got["vs"], dev)
    for k in ("vs", "m", "r", "loglik", "paths"):
        _eq(on[k], want[k][:B], f"sample_on: {k} {name} B={B}")
    sm = _call_guarded(h, br, "smooth", None, got["vs"], dev)
    for k in ("vs", "m", "r", "loglik"):
        _eq(sm[k], want[k][:B], f"smooth: {k} {name} B={B}")
    _eq(sm["paths"], want["smeans"][:B], f"smooth: smeans {name} B={B}")


# ---- 2. parity with the filter engine, the Python layer, ragged batches, chunking ---------------------------------------------
@pytest.mark.parametrize("name", ["4d", "gp20v7", "gp80v33", "rand33v80"])
def test_parity_with_the_filter_engine_and_ragged_batches(name, oracle, dev):
    toy, ts, br = _setup(name, dev)
    want = _want(oracle, name, br, toy)
    keys = _keys(oracle, name)
    h, kf = br.kalman_smoother_handle(17), br.kalman_handle(17)
    paths, ll = h.sample(keys[:17], toy["y0"], return_loglik=True)
    samples, means, kll = kf.sample(keys[:17], toy["y0"], return_moments=True)
    _eq(_np(paths)[:, -1], _np(samples), "paths[:, T] against fbsmi_kf_sample")
    _eq(_np(ll), _np(kll), "loglik against fbsmi_kf_sample")
    _eq(_np(paths), want["paths"][:17], "paths")
    v = h.views()
    _eq(_np(v["vs"]), _np(kf.views()["vs"]), "vs against fbsmi_kf_sample")
    assert v["m"].shape == (17, br.T + 1, br.du) and v["r"].shape == (17, br.T, br.dv)
    sm, sll = h.smooth(v["vs"], return_loglik=True)
    fm, fl = kf.filter(v["vs"])
    _eq(_np(sll), _np(fl), "smooth loglik against fbsmi_kf_filter")
    _eq(_np(h.views()["m"])[:, -1], _np(fm), "view 1 at k = T against fbsmi_kf_filter")
    _eq(_np(sm), want["smeans"][:17], "smeans")
    _eq(_np(h.sample_on(keys[:17], v["vs"])), want["paths"][:17], "sample_on")
    # a ragged batch runs on the bridge's handle of that size; one key of shape (2,); one path of shape (T+1, dv)
    part = h.sample(keys[:3], toy["y0"])
    assert part.shape == (3, br.T + 1, br.du) and h.views()["vs"].shape[0] == 3 and ("kalman_smoother", 3) in br._sweeps
    _eq(_np(part), want["paths"][:3], "ragged paths")
    _eq(_np(h.sample(keys[4], toy["y0"])), want["paths"][4:5], "one key")
    _eq(_np(h.smooth(v["vs"][5])), want["smeans"][5:6], "one path: smeans")
    _eq(_np(h.sample_on(keys[5], v["vs"][5])), want["paths"][5:6], "one key, one path")
    with pytest.raises(ValueError):
        h.sample(keys[:18], toy["y0"])
    assert h.cov_s.shape == (br.T + 1, br.du, br.du) and h.cov_s.dtype == np.float64


def test_chunking_does_not_change_results(oracle, dev):
    from fbs_amd import samplers
    toy, ts, br = _setup("4d", dev)
    want = _want(oracle, "4d", br, toy)
    keys = _keys(oracle, "4d")
    one = samplers.kalman_path_sampler(keys, toy["y0"], br, return_moments=True)
    two = samplers.kalman_path_sampler(keys, toy["y0"], br, return_moments=True, _bound=16 * (br.T + 1) * br.du)
    for n in (33, 16, 1):                                                               # 16, 16, 1
        assert ("kalman_smoother", n) in br._sweeps
    for a, b, k in zip(one, two, ("paths", "smeans", "loglik")):
        assert a.shape == want[k].shape
        _eq(_np(b), _np(a), f"chunked {k}")
        _eq(_np(a), want[k], k)
    assert samplers.kalman_path_sampler(keys[:2], toy["y0"], br).shape == (2, br.T + 1, br.du)


# ---- 3. the law of the draw ---------------------------------------------------------------------------------------------------
def test_law_of_the_draw(oracle, dev):
    toy, ts, br = _setup("4d", dev)
    assert br.T == 30
    B = 4096
    keys = oracle.split(oracle.PRNGKey(52), B)
    h = br.kalman_smoother_handle(B)
    paths = _np(h.sample(keys, toy["y0"])).astype(np.float64)
    resid = paths - _np(h.smooth(h.views()["vs"])).astype(np.float64)
    from fbs_amd.lg_kalman import kalman_smoother_model
    st = kalman_smoother_model(br).tables64
    white = {}
    for k in (0, 14, 15, 30):
        white[k] = np.linalg.solve(np.linalg.cholesky(st["cov_s"][k]), resid[:, k].T).T
    for k in (0, 15, 30):
        mean, var = white[k].mean(axis=0), white[k].var(axis=0, ddof=1)
        print(f"step {k}, B = {B}: whitened mean {mean}, variance {var}; bounds {4 / np.sqrt(B):.4f}, {4 * np.sqrt(2 / B):.4f}")
        assert np.all(np.abs(mean) <= 4 / np.sqrt(B)) and np.all(np.abs(var - 1) <= 4 * np.sqrt(2 / B))
    # the lag-one cross moment of (14, 15), whitened by the two Cholesky factors, against J[14] cov_s[15] whitened alike
    got = white[14].T @ white[15] / B
    L14, L15 = np.linalg.cholesky(st["cov_s"][14]), np.linalg.cholesky(st["cov_s"][15])
    cross = st["J"][14] @ st["cov_s"][15]
    assert np.allclose(cross, st["cross"][14], rtol=0, atol=1e-14)
    wantx = np.linalg.solve(L14, np.linalg.solve(L15, cross.T).T)
    print(f"whitened lag-one cross moment (14, 15): worst difference {np.abs(got - wantx).max():.4f}, bound {4 / np.sqrt(B):.4f}")
    assert np.all(np.abs(got - wantx) <= 4 / np.sqrt(B))


# ---- 4. the fused particle smoother against the exact smoothing law --------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d", "4d"])
def test_fused_particle_smoother_against_the_exact_law(name, oracle, dev):
    """The inputs and keys of tests/test_kfs_tables.py's oracle test through the fused engines, which are bit-exact to the
    oracle: that test predicts the figures."""
    import fsamp_restate as FR
    toy, ts, (tab, pm, kt, st), om, vs, keys = particle_smoother_inputs(oracle, name)
    _, _, br = _setup(name, dev)
    assert br.T == 30
    n, Cn = 1024, len(keys)
    k3 = [oracle.split(key, 3) for key in keys]
    u0s = np.stack([FR.ref_restated(oracle, pm, oracle.split(k[2], 2)[0], vs[0], n) for k in k3])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vst = t(np.broadcast_to(vs, (Cn,) + vs.shape))
    _, _, filt = br.filter_handle(n, "bootstrap", "stratified", store_path=True, nchains=Cn).run(
        np.stack([k[2] for k in k3]), vst, t(u0s))
    traj = br.backsim_handle(n, "smoother", Cn).run(np.stack([k[1] for k in k3]), vst, filt)
    check_whitened_paths(_np(traj), kt, st, vs, f"{name}: fused particle smoother, {n} particles, {Cn} keys")


# ---- 5. gibbs_init(method='kalman') -----------------------------------------------------------------------------------------------
def test_gibbs_init_kalman(oracle, dev):
    from fbs_amd.samplers import gibbs_init
    toy, ts, br = _setup("4d", dev)
    om = oracle_model_from(oracle, br)
    key = oracle.PRNGKey(31)
    y0 = torch.from_numpy(toy["y0"]).to(dev)
    x0, us_star = gibbs_init(key, y0, (br.du,), ts, br.fwd_sampler, br.sde, br.unpack, br.transition_sampler,
                             br.transition_logpdf, br.likelihood_logpdf, 10, method='kalman', marg_y=False)
    k_fwd, k_bridge, k_u0, k_bf, k_fwd2, k_bwd = oracle.split(key, 6)
    path = oracle.lg_fwd_sampler(om, k_fwd, np.concatenate([np.zeros(br.du, f32), toy["y0"]]))
    vs = path[::-1, br.du:].copy()
    want = br.kalman_smoother_handle(1).sample_on(k_bf, torch.from_numpy(vs).to(dev))[0]
    assert us_star.shape == (br.T + 1, br.du) and x0.shape == (br.du,)
    _eq(_np(us_star), _np(want), "us_star")
    _eq(_np(x0), _np(want)[-1], "x0")
    from fbs_amd.lg_kalman import kalman_smoother_model
    st = kalman_smoother_model(br)
    w = KR.sample_on_restated(oracle, st.kf_struct.host, st.host, st.kf_struct.tables64, k_bf, vs[None])
    _eq(_np(us_star), w["paths"][0], "us_star against the restatement")
    with pytest.raises(NotImplementedError, match="LinearGaussianBridge"):
        gibbs_init(key, y0, (br.du,), ts, br.fwd_sampler, br.sde, lambda p: br.unpack(p), br.transition_sampler,
                   br.transition_logpdf, br.likelihood_logpdf, 10, method='kalman', marg_y=False)


# ---- 6. the driver ----------------------------------------------------------------------------------------------------------------
def test_toy_kf_driver_smoother(tmp_path, oracle, dev):
    from fbs_amd import ops, samplers
    from fbs_amd.metrics import tabulate
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        spec = importlib.util.spec_from_file_location("toy_kf_driver_s", os.path.join(ROOT, "examples", "toy_kf.py"))
        tk = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tk)
        from _gp_toy import gp_setting
    finally:
        sys.path.remove(os.path.join(ROOT, "examples"))
    samples, gp_mean, gp_cov = tk.main(["--d", "4", "--nsamples", "40", "--batch", "16", "--quiet", "--smoother",
                                        "--outdir", str(tmp_path)])
    assert samples.shape == (40, 4) and np.isfinite(samples).all()
    path = os.path.join(str(tmp_path), "kfs-const-666.npz")
    saved = np.load(path)
    assert set(saved.files) == {"samples", "gp_mean", "gp_cov", "path_mean", "path_var"}
    _eq(saved["samples"], samples, "saved samples")
    stats = tabulate([path])
    assert stats and all(np.isfinite(m) for m, s in stats.values())
    g = gp_setting(tk.argparse.Namespace(id=666, d=4, sde="const"), dev)
    key, subkeys = g["key"], []
    for _ in range(40):
        key, subkey = ops.split(key)
        subkeys.append(subkey)
    direct = _np(samplers.kalman_path_sampler(np.stack(subkeys), g["y0_t"], g["bridge"]))
    T = g["bridge"].T
    assert saved["path_mean"].shape == saved["path_var"].shape == (T + 1, 4)
    _eq(samples, direct[:, T], "driver samples")
    _eq(saved["path_mean"], direct.mean(axis=0), "path_mean")
    _eq(saved["path_var"], direct.var(axis=0, ddof=1), "path_var")
    # paths[:, T] is the Kalman conditional sampler's draw: the default driver's samples on the same schedule
    _eq(samples, _np(samplers.kalman_conditional_sampler(np.stack(subkeys), g["y0_t"], g["bridge"])), "against the default run")
