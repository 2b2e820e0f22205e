"""GPU parity of the fused CSGM (fbsmi_csgm_*, GaussianCSGM, sdes.simulators.euler_maruyama) against the numpy
restatement of its numeric specification (tests/csgm_restate.py) on the same keys, bit for bit."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from csgm_restate import Restate
from helpers import WIDTHS
from test_csgm_tables import float64_recursion
from test_gpu_tw_fused import _eq, _np, _sde

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS_VAR = 0.7


@functools.lru_cache(maxsize=None)
def _model(d, T, sde_name):
    """The Gaussian-process toy of gp_csgm.py:30-58 at width d with a non-zero prior mean, on T steps of [0, 1]."""
    import fbs_amd
    zs = np.linspace(0., 5., d)
    cov = np.exp(-np.abs(zs[None, :] - zs[:, None]))
    rng = np.random.default_rng(100 + d)
    mean, y = 0.3 * rng.normal(size=d), rng.normal(size=d).astype(f32)
    return fbs_amd.GaussianCSGM(mean, cov, _sde(sde_name), np.linspace(0., 1., T + 1), OBS_VAR, y, device="cuda:0")


def _keys(B, seed0=11):
    import oracle as O
    return np.stack([O.PRNGKey(seed0 + b) for b in range(B)])


@functools.lru_cache(maxsize=None)
def _want(d, T, sde_name, seed):
    """The restated sample under PRNGKey(seed): computed once, shared by the tests that need it.  -> (u0, path)"""
    import oracle as O
    return Restate(O, _model(d, T, sde_name)).sample(O.PRNGKey(seed))


def _want_batch(d, T, sde_name, B, seed0=11):
    w = [_want(d, T, sde_name, seed0 + b) for b in range(B)]
    return np.stack([u for u, _ in w]), np.stack([p for _, p in w], axis=1)   # (B, d), (T+1, B, d)


SHAPES = [(1, 8, 1, "const"), (2, 5, 3, "const"), (3, 8, 33, "lin"), (5, 6, 70, "const"), (17, 6, 32, "const"),
          (24, 6, 65, "lin"), (33, 4, 31, "const"), (100, 3, 64, "const"), (128, 3, 33, "lin"), (100, 37, 8, "const")]


# Every width of the ladder: both sides of every 16-row tile, so every k_csgm<NQ>, NQ = 1..8, is launched below, on and
# above its last full tile (no zero padding at the multiples of 16); NQ = 5 and 6 are the widths at which only some waves
# own a second row tile.  T alternates 3 and 4 (both parities of the LDS ping-pong and of k + 1 == T), the SDE changes
# every second width (so both run at both T), B cycles through one sample, either side of a workgroup's 16, and 33.
LADDER = [(d, (3, 4)[i % 2], (1, 15, 16, 17, 33)[i % 5], ("const", "lin")[(i // 2) % 2]) for i, d in enumerate(WIDTHS)]


def _sample_mode(shape, want=_want_batch):
    d, T, B, sde_name = shape
    m = _model(d, T, sde_name)
    u0_w, path_w = want(d, T, sde_name, B)
    assert np.isfinite(u0_w).all() and np.isfinite(path_w).all()
    h = m.handle(B, store_path=True)
    out = h.sample(_keys(B))
    v = h.views()
    assert out.shape == (B, d) and v["u0"].shape == (B, d) and v["path"].shape == (T + 1, B, d)
    _eq(_np(v["u0"]), u0_w, "u0")
    _eq(_np(v["path"]), path_w, "path")
    _eq(_np(out), path_w[-1], "samples")


@pytest.mark.parametrize("shape", SHAPES, ids=["d{}-T{}-B{}-{}".format(*s) for s in SHAPES])
def test_sample_mode(shape, oracle, dev):
    _sample_mode(shape)


@pytest.mark.parametrize("shape", LADDER, ids=["d{}-T{}-B{}-{}".format(*s) for s in LADDER])
def test_sample_mode_across_the_width_ladder(shape, oracle, dev):
    d, T, B, sde_name = shape
    u0_1, path_1 = _want(d, T, sde_name, 11)                       # the first key through the per-key restatement
    u0_w, path_w = _want_batched(d, T, sde_name, B)
    _eq(u0_w[0], u0_1, "batched restatement: u0")
    _eq(path_w[:, 0], path_1, "batched restatement: path")
    _sample_mode(shape, _want_batched)


@functools.lru_cache(maxsize=None)
def _want_batched(d, T, sde_name, B, seed0=11):
    """_want_batch through the restatement's batched form (tests/test_csgm_tables.py holds it to the per-key one bit for
    bit): the wide cases in a fraction of a second.  -> (u0 (B, d), path (T+1, B, d))"""
    import oracle as O
    return Restate(O, _model(d, T, sde_name)).sample_batch(_keys(B, seed0))


def test_large_batch(oracle, dev):
    """B = 4113: 257 workgroups and one sample over, more workgroups than the device has compute units.  The restatement
    is batched over the samples (Restate.sample_batch), and held to the per-key one on the first 40 keys."""
    d, T, B = 3, 2, 4113
    m = _model(d, T, "const")
    keys = _keys(B)
    u0_w, path_w = _want_batched(d, T, "const", B)
    u0_1, path_1 = _want_batch(d, T, "const", 40)
    _eq(u0_w[:40], u0_1, "batched restatement: u0")
    _eq(path_w[:, :40], path_1, "batched restatement: path")
    assert np.isfinite(path_w).all()
    h = m.handle(B, store_path=True)
    out = h.sample(keys)
    v = h.views()
    _eq(_np(v["u0"]), u0_w, "u0")
    _eq(_np(v["path"]), path_w, "path")
    _eq(_np(out), path_w[-1], "samples")


def _integrate_mode(d, T, sde_name, store_path, oracle, dev):
    B = 19
    m = _model(d, T, sde_name)
    rs = Restate(oracle, m)
    u0 = np.random.default_rng(3).normal(size=(B, d)).astype(f32)
    keys = _keys(B, 40)
    want = np.stack([rs.integrate(keys[b], u0[b], return_path=True) for b in range(B)], axis=1)
    assert np.isfinite(want).all()
    h = m.handle(B, store_path=store_path)
    out = h.integrate(keys, torch.from_numpy(u0).to(dev))
    _eq(_np(out), want[-1], "final states")
    v = h.views()
    _eq(_np(v["u0"]), u0, "u0 view")
    if store_path:
        _eq(_np(v["path"]), want, "path")
    else:
        assert "path" not in v


@pytest.mark.parametrize("store_path", [True, False])
def test_integrate_mode(store_path, oracle, dev):
    _integrate_mode(24, 6, "const", store_path, oracle, dev)


# integrate mode (u0 from the caller: the clamped load of rows >= d, the table fetch from table 1) at an exact tile count
# (16, 48, 96), just past one (65, 113) and at NQ = 5, where wave 0 alone owns a second row tile
@pytest.mark.parametrize("store_path", [True, False])
@pytest.mark.parametrize("d,T,sde_name", [(16, 3, "const"), (48, 4, "lin"), (65, 3, "lin"), (80, 4, "const"), (96, 3, "const"),
                                          (113, 4, "lin")])
def test_integrate_mode_across_widths(d, T, sde_name, store_path, oracle, dev):
    _integrate_mode(d, T, sde_name, store_path, oracle, dev)


def test_without_store_path(oracle, dev):
    d, T, B = 17, 6, 32
    m = _model(d, T, "const")
    h = m.handle(B)
    assert h is not m.handle(B, store_path=True) and m.handle(B, store_path=False) is h    # cached per argument tuple
    out = h.sample(_keys(B))
    u0_w, path_w = _want_batch(d, T, "const", B)
    _eq(_np(out), path_w[-1], "samples")
    v = h.views()
    assert sorted(v) == ["u0"]
    _eq(_np(v["u0"]), u0_w, "u0")


def test_handle_reused_with_other_keys_and_a_short_batch(oracle, dev):
    d, T, B = 5, 6, 70
    m = _model(d, T, "const")
    h = m.handle(B, store_path=True)
    for seed0 in (200, 11, 300):
        out = h.sample(_keys(B, seed0))
        _, path_w = _want_batch(d, T, "const", B, seed0)
        _eq(_np(h.views()["path"]), path_w, f"seeds from {seed0}: path")
        _eq(_np(out), path_w[-1], f"seeds from {seed0}: samples")
    out = h.sample(_keys(13))                                      # a short last batch
    u0_w, path_w = _want_batch(d, T, "const", 13)
    assert out.shape == (13, d)
    _eq(_np(out), path_w[-1], "short batch")
    _eq(_np(h.views()["u0"]), u0_w, "short batch u0")
    _eq(_np(h.views()["path"]), path_w, "short batch path")
    one = h.sample(oracle.PRNGKey(11))                             # (2,): one sample
    _eq(_np(one), path_w[-1][:1], "one key")
    with pytest.raises(ValueError):
        h.sample(_keys(B + 1))


@pytest.mark.parametrize("return_path", [False, True])
def test_dispatch_takes_the_fused_engine(return_path, oracle, dev):
    from fbs_amd.sdes.simulators import euler_maruyama
    d, T = 24, 6
    m = _model(d, T, "lin")
    rs = Restate(oracle, m)
    key, u0 = oracle.PRNGKey(77), np.random.default_rng(4).normal(size=d).astype(f32)
    want = rs.integrate(key, u0, return_path=True)
    got = euler_maruyama(key, torch.from_numpy(u0).to(dev), m.ts_np, m.reverse_drift, m.reverse_dispersion,
                         return_path=return_path)
    if return_path:
        assert got.shape == (T + 1, d)
        _eq(_np(got), want, "path")
    else:
        assert got.shape == (d,)
        _eq(_np(got), want[-1], "final state")


@pytest.mark.parametrize("how", ["nsteps2", "lambda"])
def test_dispatch_elsewhere_runs_the_host_loop(how, oracle, dev):
    """Sub-stepping, or a drift that is not the model's closure, takes the host loop on the closure tier: against the float64
    recursion on the same draws at T = 2, 1e-5 relative to the largest magnitude, the project's float tolerance."""
    from fbs_amd import ops
    from fbs_amd.sdes.simulators import euler_maruyama
    d, T = 24, 2
    m = _model(d, T, "const")
    key, u0 = oracle.PRNGKey(31), np.random.default_rng(5).normal(size=d).astype(f32)
    x0 = torch.from_numpy(u0).to(dev)
    t64 = m.tables64
    if how == "lambda":
        got = euler_maruyama(key, x0, m.ts_np, lambda u, t: m.reverse_drift(u, t), m.reverse_dispersion)
        want = float64_recursion(oracle, m, key, u0)[-1]
    else:
        # two sub-steps per interval: the second starts off the model's grid, so the closures are tabulated by hand
        ts, sde = m.ts_np, m.sde
        drift = lambda u, t: u @ m.dev["A"][int(round(float(t) * T - 0.25))].T + m.dev["cvec"][int(round(float(t) * T - 0.25))]
        disp = lambda t: float(sde.dispersion(float(ts[-1]) - float(t)))
        got = euler_maruyama(key, x0, ts, drift, disp, integration_nsteps=2)
        with pytest.raises(ValueError):    # the model's own closures under sub-stepping: the host loop, which leaves the grid
            euler_maruyama(key, x0, ts, m.reverse_drift, m.reverse_dispersion, integration_nsteps=2)
        x, keys = u0.astype(np.float64), oracle.split(key, T)
        for k in range(T):
            xi = _np(ops.normal(keys[k], (2, d), device=dev)).astype(np.float64)
            h = abs(ts[k + 1] - ts[k]) / 2
            for j in range(2):
                x = x + (t64["A"][k] @ x + t64["cvec"][k]) * h + disp(ts[k] + j * h) * np.sqrt(h) * xi[j]
        want = x
    err = np.abs(_np(got).astype(np.float64) - want).max() / np.abs(want).max()
    print(f"host loop ({how}) against float64: {err:.3g}")
    assert got.shape == (d,) and err <= 1e-5


def test_driver_fused(oracle, dev, tmp_path):
    """examples/toy_csgm.py --fused with a ragged last batch (12 samples, 5 at a time) against the restated driver loop
    (gp_csgm.py:110-114); the .npz schema is the driver's; without --fused the file still runs."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        spec = importlib.util.spec_from_file_location("toy_csgm_example", os.path.join(ROOT, "examples", "toy_csgm.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        import _gp_toy
        import fbs_amd
        argv = ["--d", "5", "--nsamples", "12", "--outdir", str(tmp_path), "--quiet"]
        samples, gp_mean, gp_cov = mod.main(argv + ["--fused", "--batch", "5"])
        assert samples.shape == (12, 5) and samples.dtype == np.float32
        with np.load(os.path.join(str(tmp_path), "csgm-const-666.npz")) as z:
            assert sorted(z.files) == ["gp_cov", "gp_mean", "samples"]
            _eq(z["samples"], samples, "saved samples")
            assert z["gp_mean"].shape == (5,) and z["gp_cov"].shape == (5, 5)
        args = _gp_toy.add_common_args(__import__("argparse").ArgumentParser()).parse_args(argv)
        g = _gp_toy.gp_setting(args, dev)
        model = fbs_amd.GaussianCSGM(np.zeros(5), g["cov_mat"], g["sde"], g["ts"], g["obs_var"], g["y0"], device=dev)
        rs, key, want = Restate(oracle, model), g["key"], []
        for _ in range(12):
            key, subkey = oracle.split(key, 2)
            want.append(rs.sample(subkey)[1][-1])
        _eq(samples, np.stack(want), "driver samples")
        plain, _, _ = mod.main(["--d", "5", "--nsamples", "2", "--outdir", str(tmp_path), "--quiet"])
        assert plain.shape == (2, 5) and np.isfinite(plain).all()
    finally:
        sys.path.remove(os.path.join(ROOT, "examples"))
