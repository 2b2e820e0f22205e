"""GPU parity of the fused twisted SMC (fbsmi_tw_*, GaussianTwisted, samplers.smc.twisted_smc) against the numpy
restatement of its numeric specification (tests/tw_restate.py) on the same keys, bit for bit."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from tw_restate import Restate

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS_VAR = 0.7


def _np(t):
    return t.detach().cpu().numpy()


def _eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    x = a.view(np.uint32) if a.dtype == np.float32 else a
    y = b.view(np.uint32) if b.dtype == np.float32 else b
    bad = np.flatnonzero(x.ravel() != y.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first {bad[:4]}: {a.ravel()[bad[:4]]} vs {b.ravel()[bad[:4]]}"


def _sde(name):
    from fbs_amd.sdes import StationaryConstLinearSDE, StationaryLinLinearSDE
    return StationaryLinLinearSDE(beta_min=0.02, beta_max=4., t0=0., T=1.) if name == "lin" else StationaryConstLinearSDE(a=-0.5, b=1.)


@functools.lru_cache(maxsize=None)
def _model(d, T, sde_name, obs_var=OBS_VAR, device="cuda:0"):
    """The Gaussian-process toy of gp_twisted.py:30-58 at width d with a non-zero prior mean, on T steps of [0, 1]."""
    import fbs_amd
    zs = np.linspace(0., 5., d)
    cov = np.exp(-np.abs(zs[None, :] - zs[:, None]))
    rng = np.random.default_rng(100 + d)
    mean, y = 0.3 * rng.normal(size=d), rng.normal(size=d).astype(f32)
    return fbs_amd.GaussianTwisted(mean, cov, _sde(sde_name), np.linspace(0., 1., T + 1), obs_var, y, device=device)


@functools.lru_cache(maxsize=None)
def _want(d, T, N, sde_name, resampling, seed, obs_var=OBS_VAR, device="cuda:0"):
    """The restated run under PRNGKey(seed): computed once, shared by the tests that need it."""
    import oracle as O
    return Restate(O, _model(d, T, sde_name, obs_var, device)).run(O.PRNGKey(seed), N, resampling)


@functools.lru_cache(maxsize=None)
def _want_sample(d, T, N, sde_name, seed, obs_var=OBS_VAR):
    import oracle as O
    return Restate(O, _model(d, T, sde_name, obs_var)).sample(O.PRNGKey(seed), N)


SHAPES = [(1, 8, 1, "const"), (2, 5, 2, "const"), (3, 8, 16, "const"), (3, 8, 100, "lin"), (10, 6, 257, "const"),
          (10, 6, 1000, "const"), (24, 6, 48, "const"), (24, 4, 300, "lin"), (100, 3, 64, "const"), (128, 3, 33, "lin")]


def _single_run(shape, resampling, oracle, obs_var=OBS_VAR):
    d, T, N, sde_name = shape
    m = _model(d, T, sde_name, obs_var)
    xs_w, lws_w, inds_w = _want(d, T, N, sde_name, resampling, 11, obs_var)
    assert np.isfinite(xs_w).all() and np.isfinite(lws_w).all()
    h = m.handle(N, resampling, nruns=1, store_ancestors=True)
    xs, lws = h.run(oracle.PRNGKey(11))
    assert xs.shape == (1, N, d) and lws.shape == (1, N)
    _eq(_np(h.views()["ancestors"])[0], inds_w, "ancestors")
    _eq(_np(xs)[0], xs_w, "particles")
    _eq(_np(lws)[0], lws_w, "log-weights")


@pytest.mark.parametrize("resampling", ["stratified", "systematic"])
@pytest.mark.parametrize("shape", SHAPES, ids=["d{}-T{}-N{}-{}".format(*s) for s in SHAPES])
def test_single_run(shape, resampling, oracle, dev):
    _single_run(shape, resampling, oracle)


# The widths of k_tw_gemm: nq = Kp / 16 = 1..7 column groups through the two-at-a-time operand pipeline (odd and even
# counts), exact row tiles (2 d = 32, 64, ...), the first width whose columns need the second staging half (65), against
# ensemble sizes on either side of the 32-slot tile (31 / 32 / 33) and of the one-tile boundary (255 / 256 / 257: three
# launches a step up to 256, five above), and nb = 2 and 3 tiles.  obs_var = 5: with 0.7 these wide models collapse (d = 64,
# N = 255 keeps 3 distinct ancestors in step 0) and the gather would read a handful of rows; tests/test_tw_tables.py
# asserts that every step of every case here keeps at least N / 4 distinct ancestors.
WIDE_OBS_VAR = 5.0
WIDE = [(16, 4, 32, "const"), (32, 3, 31, "lin"), (32, 3, 33, "lin"), (48, 3, 256, "const"), (64, 3, 255, "const"),
        (65, 4, 64, "lin"), (80, 3, 257, "const"), (96, 4, 33, "const"), (112, 3, 100, "lin"), (17, 3, 512, "const"),
        (33, 3, 513, "const")]
# The ensemble sizes of k_tw_norm / k_tw_cdf / lse_from_partials: nb = 5, 17 (the top tree past thread 0), 256 (the last
# size with one tile pair per thread), 274 (four per thread), 512 (capacity: two waves of the top tree); (d, T, N), const
# SDE, obs_var = 0.7 but for the one model of width 16, which at 0.7 keeps 150 of 1025 ancestors in step 0.
LARGE = [(16, 2, 1025), (3, 3, 4097), (2, 3, 65536), (3, 2, 70001), (1, 2, 131072)]


def ladder_obs_var(d):
    return WIDE_OBS_VAR if d >= 16 else OBS_VAR


@pytest.mark.parametrize("resampling", ["stratified", "systematic"])
@pytest.mark.parametrize("shape", WIDE, ids=["d{}-T{}-N{}-{}".format(*s) for s in WIDE])
def test_single_run_across_the_widths(shape, resampling, oracle, dev):
    _single_run(shape, resampling, oracle, WIDE_OBS_VAR)


@pytest.mark.parametrize("shape", [(48, 3, 256, "const"), (80, 3, 257, "const")], ids=["d48-N256", "d80-N257"])
def test_sample_across_the_one_tile_boundary(shape, oracle, dev):
    """sample() (the select graph: the last normalisation, its cdf above one tile, the choice) at wide models."""
    d, T, N, sde_name = shape
    h = _model(d, T, sde_name, WIDE_OBS_VAR).handle(N, "stratified", nruns=1)
    for seed in (11, 12):
        smp = h.sample(oracle.PRNGKey(seed)[None])
        assert smp.shape == (1, d)
        _eq(_np(smp)[0], _want_sample(d, T, N, sde_name, seed, WIDE_OBS_VAR), f"seed {seed} sample")


@pytest.mark.parametrize("resampling", ["stratified", "systematic"])
@pytest.mark.parametrize("shape", LARGE, ids=["d{}-T{}-N{}".format(*s) for s in LARGE])
def test_single_run_at_large_ensembles(shape, resampling, oracle, dev):
    _single_run(shape + ("const",), resampling, oracle, ladder_obs_var(shape[0]))


def test_batched_runs_at_a_large_ensemble(oracle, dev):
    """nruns = 3 at N = 4097 (nb = 17): the per-run offsets of the tile partials with more tiles than one thread holds."""
    d, T, N = 3, 3, 4097
    seeds = [11, 12, 13]
    h = _model(d, T, "const").handle(N, "stratified", nruns=3, store_ancestors=True)
    xs, lws = h.run(np.stack([oracle.PRNGKey(s) for s in seeds]))
    anc = _np(h.views()["ancestors"])
    assert xs.shape == (3, N, d) and lws.shape == (3, N) and anc.shape == (3, T, N)
    for b, s in enumerate(seeds):
        xs_w, lws_w, inds_w = _want(d, T, N, "const", "stratified", s)
        _eq(anc[b], inds_w, f"run {b} ancestors")
        _eq(_np(xs)[b], xs_w, f"run {b} particles")
        _eq(_np(lws)[b], lws_w, f"run {b} log-weights")


@pytest.mark.parametrize("shape", [(10, 6, 257, "const"), (24, 6, 48, "const")], ids=["d10-N257", "d24-N48"])
def test_batched_runs(shape, oracle, dev):
    d, T, N, sde_name = shape
    m, B = _model(d, T, sde_name), 5
    seeds = [11, 12, 13, 14, 15]
    keys = np.stack([oracle.PRNGKey(s) for s in seeds])
    h = m.handle(N, "stratified", nruns=B, store_ancestors=True)
    xs, lws = h.run(keys)
    anc = _np(h.views()["ancestors"])
    assert xs.shape == (B, N, d) and lws.shape == (B, N) and anc.shape == (B, T, N)
    for b, s in enumerate(seeds):
        xs_w, lws_w, inds_w = _want(d, T, N, sde_name, "stratified", s)
        _eq(anc[b], inds_w, f"run {b} ancestors")
        _eq(_np(xs)[b], xs_w, f"run {b} particles")
        _eq(_np(lws)[b], lws_w, f"run {b} log-weights")
    smp = h.sample(keys)
    assert smp.shape == (B, d)
    for b, s in enumerate(seeds):
        _eq(_np(smp)[b], _want_sample(d, T, N, sde_name, s), f"run {b} sample")


def _five(m):
    return m.init_sampler, m.transition_logpdf, m.twisting_logpdf, m.twisting_prop_sampler, m.twisting_prop_logpdf


def test_dispatch_takes_the_fused_engine(oracle, dev):
    from fbs_amd.samplers import stratified
    from fbs_amd.samplers.smc import twisted_smc
    d, T, N = 24, 6, 48
    m = _model(d, T, "const")
    y = torch.from_numpy(m.host["y"]).to(dev)
    xs, lws = twisted_smc(oracle.PRNGKey(11), y, m.ts_np, *_five(m), resampling=stratified, nparticles=N)
    xs_w, lws_w, _ = _want(d, T, N, "const", "stratified", 11)
    assert xs.shape == (N, d) and lws.shape == (N,)
    _eq(_np(xs), xs_w, "particles")
    _eq(_np(lws), lws_w, "log-weights")


def test_dispatch_multinomial_runs_the_host_loop(oracle, dev):
    """One step (T = 1) of the host loop on the model's closures against the float64 evaluation of the same step from the
    same draws and ancestors: 1e-5 relative to the largest magnitude, the project's float tolerance."""
    from fbs_amd import ops
    from fbs_amd.samplers import multinomial
    from fbs_amd.samplers.smc import twisted_smc
    d, N = 24, 48
    m = _model(d, 1, "const")
    key = oracle.PRNGKey(21)
    y = torch.from_numpy(m.host["y"]).to(dev)
    xs, lws = twisted_smc(key, y, m.ts_np, *_five(m), resampling=multinomial, nparticles=N)
    assert xs.shape == (N, d) and lws.shape == (N,) and torch.isfinite(lws).all()
    # the same step by hand: float32 draws and ancestors as the loop has them, the arithmetic in float64
    key_init, key_filter = ops.split(key, 2)
    key_resampling, key_prop = ops.split(ops.split(key_filter, 1)[0], 2)
    x0 = m.init_sampler(key_init, N)
    log_ws = ops.normalise(m.twisting_logpdf(y, x0, m.ts_np[0]), log_space=True)
    inds = _np(multinomial(ops.math_map("exp", log_ws), key_resampling)).astype(np.int64)
    t64 = m.tables64
    z0 = _np(ops.normal(key_init, (N, d), device=dev)).astype(np.float64)
    x0_64 = t64["m_ref"][None, :] + z0 @ t64["Lt"]
    xp = x0_64[inds]
    z = _np(ops.normal(key_prop, (N, d), device=dev)).astype(np.float64)
    want = xp + (xp @ t64["C"][1].T + t64["c"][1]) * t64["dt"] + t64["sd"][1] * z
    err = np.abs(_np(xs).astype(np.float64) - want).max() / np.abs(want).max()
    print(f"host loop against float64, one step: {err:.3g}")
    assert err <= 1e-5


def test_closures_against_the_fused_terms(oracle, dev):
    d, T, N = 24, 6, 48
    m = _model(d, T, "const")
    h = m.handle(N, "stratified", nruns=1)
    xs, _ = h.run(oracle.PRNGKey(11))
    v = h.views()
    assert "ancestors" not in v                                    # kept only when asked for
    xs, t = xs[0], m.ts_np[-1]
    xp = v["xs_prev"][0][v["last_ancestors"][0].long()]
    y = torch.from_numpy(m.host["y"]).to(dev)
    for name, got, want in (("twisting_prop_logpdf", m.twisting_prop_logpdf(xs, xp, t, y), v["pl"][0]),
                            ("transition_logpdf", m.transition_logpdf(xs, xp, t), v["tl"][0]),
                            ("twisting_logpdf", m.twisting_logpdf(y, xs, t), v["log_ps"][0])):
        err = float((got - want).abs().max() / want.abs().max())
        print(f"{name}: {err:.3g}")
        assert got.shape == (N,) and err <= 1e-5, name


def test_handle_reused_with_other_keys(oracle, dev):
    """Graph replay and state reset: a second and a third call on one handle give the restatement's result for their keys."""
    d, T, N = 10, 6, 257
    m = _model(d, T, "const")
    h = m.handle(N, "stratified", nruns=1, store_ancestors=True)
    assert m.handle(N, "stratified", nruns=1, store_ancestors=True) is h     # cached
    for seed in (12, 11, 13):
        xs, lws = h.run(oracle.PRNGKey(seed))
        xs_w, lws_w, inds_w = _want(d, T, N, "const", "stratified", seed)
        _eq(_np(h.views()["ancestors"])[0], inds_w, f"seed {seed} ancestors")
        _eq(_np(xs)[0], xs_w, f"seed {seed} particles")
        _eq(_np(lws)[0], lws_w, f"seed {seed} log-weights")
    _eq(_np(h.sample(oracle.PRNGKey(14)[None]))[0], _want_sample(d, T, N, "const", 14), "sample after runs")


def test_driver_fused(oracle, dev, tmp_path):
    """examples/toy_twisted.py --fused with a ragged last batch (12 samples, 5 at a time) against the restated driver loop
    (gp_twisted.py:144-148); the .npz schema is the driver's; without --fused the file still runs."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        spec = importlib.util.spec_from_file_location("toy_twisted_example", os.path.join(ROOT, "examples", "toy_twisted.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        import _gp_toy
        import fbs_amd
        argv = ["--d", "5", "--nparticles", "64", "--nsamples", "12", "--outdir", str(tmp_path), "--quiet"]
        samples, gp_mean, gp_cov = mod.main(argv + ["--fused", "--batch", "5"])
        assert samples.shape == (12, 5) and samples.dtype == np.float32
        with np.load(os.path.join(str(tmp_path), "twisted-const-64-666.npz")) as z:
            assert sorted(z.files) == ["gp_cov", "gp_mean", "samples"]
            _eq(z["samples"], samples, "saved samples")
            assert z["gp_mean"].shape == (5,) and z["gp_cov"].shape == (5, 5)
        args = mod.add_common_args(__import__("argparse").ArgumentParser()).parse_args(argv)
        g = _gp_toy.gp_setting(args, dev)
        model = fbs_amd.GaussianTwisted(np.zeros(5), g["cov_mat"], g["sde"], g["ts"], g["obs_var"], g["y0"], device=dev)
        rs, key, want = Restate(oracle, model), g["key"], []
        for _ in range(12):
            key, subkey = oracle.split(key, 2)
            want.append(rs.sample(subkey, 64))
        _eq(samples, np.stack(want), "driver samples")
        plain, _, _ = mod.main(["--d", "5", "--nparticles", "64", "--nsamples", "2", "--outdir", str(tmp_path), "--quiet"])
        assert plain.shape == (2, 5) and np.isfinite(plain).all()
    finally:
        sys.path.remove(os.path.join(ROOT, "examples"))
