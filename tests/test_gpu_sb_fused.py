"""GPU: the Gaussian Schrodinger-bridge toy on the fused engine (fbs_amd.GaussianSBBridge) -- the Euler-Maruyama path
kernel bit for bit against its numpy restatement, fused sweeps / chains / filters against the oracle composed with that
restatement, dispatch from the reference's signatures, and the example drivers' --fused mode."""
import os

import numpy as np
import pytest
import torch

from helpers import oracle_model_from, toy_4d
from sb_restate import em_path, gibbs_kernel_sb, sb_problem

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _eq(got, want, what):
    got, want = np.ascontiguousarray(_np(got)), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == np.bool_ or want.dtype == np.bool_:
        np.testing.assert_array_equal(got.astype(bool), want.astype(bool), err_msg=what)
    else:
        np.testing.assert_array_equal(got.view(np.uint8), want.astype(got.dtype).view(np.uint8), err_msg=what)


def _model(d, T, nsub, dev, sig=1.0, seed=0):
    import fbs_amd
    m0, c0, m1, c1 = sb_problem(d, seed)
    return fbs_amd.GaussianSBBridge(m0, c0, m1, c1, np.linspace(0.0, 1.0, T + 1), du=d, sig=sig, nsub=nsub, device=dev)


def _em(br):
    h = br.em_host
    return h["M"], h["c"], h["ddt"], h["s"], br.nsub


@pytest.mark.parametrize("D,T,nsub", [(6, 20, 10), (20, 12, 10), (48, 6, 4), (128, 4, 3), (256, 3, 2)])
def test_em_path_bit_exact(oracle, dev, D, T, nsub):
    br = _model(D // 2, T, nsub, dev, sig=0.8)
    rng = np.random.default_rng(D)
    x0, y0 = rng.normal(size=D // 2).astype(np.float32), rng.normal(size=D // 2).astype(np.float32)
    key = oracle.PRNGKey(100 + D)
    got = br.fwd_sampler(key, x0, y0)
    torch.cuda.synchronize()
    M, c, ddt, s, _ = _em(br)
    want = em_path(oracle, key, M, c, ddt, s, np.concatenate([x0, y0]), T, nsub)
    _eq(got, want, f"EM path D={D}")


def test_em_path_matches_closure_tier(oracle, dev):
    """Against the shipped closure tier (euler_maruyama with make_gaussian_bw_sb's drift, one launch per sub-step) under the
    same key: an independent check of the key schedule and the tables."""
    from fbs_amd.sdes import euler_maruyama, make_gaussian_bw_sb
    d, T, nsub, sig = 10, 30, 10, 1.0
    br = _model(d, T, nsub, dev, sig=sig)
    m0, c0, m1, c1 = sb_problem(d, 0)
    _, _, drift = make_gaussian_bw_sb(m0, c0, m1, c1, sig=sig)
    rng = np.random.default_rng(4)
    z0 = torch.from_numpy(rng.normal(size=2 * d).astype(np.float32)).to(dev)
    key = oracle.PRNGKey(9)
    got = _np(br.fwd_sampler(key, z0[:d], z0[d:]))
    ref = _np(euler_maruyama(key, z0, br.ts_np, drift, lambda t: sig, integration_nsteps=nsub, return_path=True))
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), np.abs(got - ref).max()


_SWEEP = [(d, eb, ef, N) for d in (3, 10) for eb in (True, False) for ef in (False, True) for N in (16, 100, 1000)]


@pytest.mark.parametrize("d,eb,ef,N", _SWEEP)
def test_fused_sweep_bit_exact(oracle, dev, d, eb, ef, N):
    T, nsub = 8, 3
    br = _model(d, T, nsub, dev, seed=d)
    om = oracle_model_from(oracle, br)
    rng = np.random.default_rng(N + d)
    x0, y0 = rng.normal(size=d).astype(np.float32), rng.normal(size=d).astype(np.float32)
    bs = rng.integers(0, N, T + 1).astype(np.int32)
    key = oracle.PRNGKey(7 + N)
    sweep = br.sweep_handle(N, eb, ef)
    got = sweep.sweep(key, x0, y0, bs)
    v = sweep.views()
    want = gibbs_kernel_sb(oracle, om, _em(br), key, x0, y0, bs, N, eb, ef)
    for i, what in enumerate(("x0_next", "us_star_next", "bs_next", "acc")):
        _eq(got[i], want[i], what)
    for name in ("us_T", "lw_T", "us_star", "vs"):
        _eq(v[name], want[4][name], name)


@pytest.mark.parametrize("d,N,eb", [(3, 100, True), (10, 16, False), (24, 64, True)])
def test_fused_sweep_chain_groups_and_wide(oracle, dev, d, N, eb):
    """C = 4 chains (two chain groups of two), and the wide family (d = 24: drift on the matrix cores)."""
    T, nsub, Cn = 6, 2, 4
    br = _model(d, T, nsub, dev, seed=1)
    om = oracle_model_from(oracle, br)
    rng = np.random.default_rng(d)
    x0 = rng.normal(size=(Cn, d)).astype(np.float32)
    y0 = rng.normal(size=d).astype(np.float32)
    bs = rng.integers(0, N, (Cn, T + 1)).astype(np.int32)
    keys = oracle.split(oracle.PRNGKey(5), Cn)
    sweep = br.sweep_handle(N, eb, False, nchains=Cn)
    assert len(sweep.children) == 2
    got = sweep.sweep(keys, x0, y0, bs)
    v = sweep.views()
    for c in range(Cn):
        want = gibbs_kernel_sb(oracle, om, _em(br), keys[c], x0[c], y0, bs[c], N, eb, False)
        for i, what in enumerate(("x0_next", "us_star_next", "bs_next", "acc")):
            _eq(got[i][c], want[i], f"chain {c} {what}")
        for name in ("us_T", "lw_T", "us_star", "vs"):
            _eq(v[name][c], want[4][name], f"chain {c} {name}")


def test_chain_driver(oracle, dev):
    """sweep_handle(...).chain over 5 sweeps = 5 restated sweeps under key, subkey = split(key) (sb/gibbs.py:176-184)."""
    d, T, nsub, N, nsweeps = 3, 6, 3, 32, 5
    br = _model(d, T, nsub, dev)
    om = oracle_model_from(oracle, br)
    rng = np.random.default_rng(2)
    x0, y0 = rng.normal(size=d).astype(np.float32), rng.normal(size=d).astype(np.float32)
    bs = np.zeros(T + 1, np.int32)
    key = oracle.PRNGKey(11)
    k_out, x_out, bs_out, x0s = br.sweep_handle(N, True, False).chain(key, x0, y0, bs, nsweeps)
    wk, wx, wbs = key, x0, bs
    for i in range(nsweeps):
        wk, sub = oracle.split(wk, 2)
        wx, _, wbs, _, _ = gibbs_kernel_sb(oracle, om, _em(br), sub, wx, y0, wbs, N, True, False)
        _eq(x0s[i], wx, f"sweep {i} x0")
    _eq(x_out, wx, "x0")
    _eq(bs_out, wbs, "bs_star")
    np.testing.assert_array_equal(np.asarray(k_out, np.uint32), np.asarray(wk, np.uint32))


def test_dispatch_gibbs_kernel_and_filter(oracle, dev):
    from fbs_amd.samplers import bootstrap_filter, gibbs_kernel, stratified
    from fbs_amd import ops
    d, T, nsub, N = 3, 8, 3, 64
    br = _model(d, T, nsub, dev)
    rng = np.random.default_rng(6)
    x0, y0 = rng.normal(size=d).astype(np.float32), rng.normal(size=d).astype(np.float32)
    bs = rng.integers(0, N, T + 1).astype(np.int32)
    key = oracle.PRNGKey(13)
    want = br.gibbs_kernel(key, x0, y0, bs, N, True, False)
    br._sweeps.clear()
    got = gibbs_kernel(key, torch.from_numpy(x0).to(dev), torch.from_numpy(y0).to(dev), None, bs, br.ts_np, br.fwd_sampler,
                       None, br.unpack, N, br.transition_sampler, br.transition_logpdf, br.likelihood_logpdf, marg_y=False,
                       explicit_backward=True, explicit_final=False)
    assert len(br._sweeps) == 1, "sde=None with the model's closures must take the fused engine"
    for g_, w_, what in zip(got, want, ("x0", "us_star", "bs", "acc")):
        _eq(g_, _np(w_), what)
    # bootstrap_filter on the model's closures and stratified resampling = the oracle's filter on the same tables
    om = oracle_model_from(oracle, br)
    vs = torch.from_numpy(rng.normal(size=(T + 1, d)).astype(np.float32)).to(dev)
    fkey = oracle.PRNGKey(17)
    uT, nell = bootstrap_filter(br.transition_sampler, br.likelihood_logpdf, vs, br.ts_np, br.ref_sampler, fkey, N,
                                stratified, log=True, return_last=True)
    init = _np(br.ref_sampler(ops.split(fkey, 2)[0], vs[0], N))
    w_uT, w_nell = oracle.bootstrap_filter_lg(om, fkey, _np(vs), init, "stratified")
    _eq(uT, w_uT, "filter particles")
    _eq(_np(nell).reshape(()), np.float32(w_nell).reshape(()), "filter -log likelihood")


def test_ref_sampler_lower_factor(oracle, dev):
    """ref_sampler = posterior of N(mean1, cov1) given the y part, m + z @ cholesky_lower (sb/gibbs.py:131-134)."""
    from fbs_amd import ops
    d = 3
    br = _model(d, 4, 2, dev)
    yT = np.array([0.3, -0.2, 1.0])
    key = oracle.PRNGKey(3)
    got = _np(br.ref_sampler(key, yT, 5))
    m1, c1 = br.mean1, br.cov1
    gain = c1[:d, d:] @ np.linalg.inv(c1[d:, d:])
    m = m1[:d] + gain @ (yT - m1[d:])
    L = np.linalg.cholesky(c1[:d, :d] - gain @ c1[d:, :d])
    z = _np(ops.normal(key, (5, d), device=dev)).astype(np.float64)
    np.testing.assert_allclose(got, m + z @ L, rtol=1e-5, atol=1e-5)


def test_lg_handle_after_sb_handle(oracle, dev):
    """An LG sweep created after an SB one in the same process runs the exact-transition forward paths as before."""
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    sb = _model(3, 6, 2, dev)
    sb.sweep_handle(16, True, False).sweep(oracle.PRNGKey(1), np.zeros(3, np.float32), np.zeros(3, np.float32),
                                           np.zeros(7, np.int32))
    toy = toy_4d()
    T, N = 10, 64
    br = fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(a=-0.5, b=1.0),
                                      np.linspace(0, 1, T + 1), du=toy["du"], device=dev)
    om = oracle_model_from(oracle, br)
    x0 = np.array([0.2, -0.1], np.float32)
    bs = np.arange(T + 1, dtype=np.int32) % N
    key = oracle.PRNGKey(21)
    for eb in (True, False):
        got = br.sweep_handle(N, eb, False).sweep(key, x0, toy["y0"], bs)
        want = oracle.gibbs_kernel_lg(om, key, x0, toy["y0"], bs, N, eb, False)
        for i in range(4):
            _eq(got[i], want[i], f"LG eb={eb} output {i}")


def _load_example(name):
    import importlib.util
    import sys
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    spec = importlib.util.spec_from_file_location(name + "_sbfused", os.path.join(ex, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_toy_sb_gibbs_driver_fused(tmp_path, dev):
    mod = _load_example("toy_sb_gibbs")
    samples, gp_mean, gp_cov = mod.main(["--d", "3", "--nparticles", "16", "--nsamples", "60", "--explicit_backward",
                                         "--fused", "--outdir", str(tmp_path), "--quiet"])
    assert samples.shape == (60, 3) and np.isfinite(samples).all()
    z = (samples[20:].mean(0) - gp_mean) / np.sqrt(np.diag(gp_cov))
    assert np.abs(z).max() < 1.5
    assert set(np.load(os.path.join(str(tmp_path), "gibbs-eb-16-666.npz")).files) == {"samples", "gp_mean", "gp_cov"}


def test_toy_sb_filter_driver_fused(tmp_path, dev):
    mod = _load_example("toy_sb_filter")
    for x0 in ("proper", "heuristic"):
        samples, gp_mean, gp_cov = mod.main(["--d", "3", "--nparticles", "32", "--nsamples", "40", "--x0", x0, "--fused",
                                             "--outdir", str(tmp_path), "--quiet"])
        assert samples.shape == (40, 3) and np.isfinite(samples).all()
        z = (samples.mean(0) - gp_mean) / np.sqrt(np.diag(gp_cov))
        assert np.abs(z).max() < 1.5, (x0, z)
        assert set(np.load(os.path.join(str(tmp_path), f"filter-{x0}-32-666.npz")).files) == {"samples", "gp_mean", "gp_cov"}
