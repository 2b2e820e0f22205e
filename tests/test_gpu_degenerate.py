"""GPU parity of the fused engines on COLLAPSED ensembles: effective sample size ~ 1, long runs of exactly-zero weights
(plateaus in the cdf, zero subtrees in the summation tree), kill fractions up to a whole tile but one slot.  The inputs are
those of tests/degenerate.py; tests/test_degenerate_inputs.py proves on the CPU that each of them reaches that regime and
that the oracle stays finite on it.  Everything here is bit equality with the oracle, as in tests/test_gpu_lg.py."""
import numpy as np
import pytest
import torch

import degenerate as D
import fsamp_restate as R
from helpers import oracle_model_from
from tw_restate import Restate

pytestmark = pytest.mark.gpu

f32 = np.float32
OUTPUTS = ("x0_next", "us_star_next", "bs_star_next", "acc")


def _np(t):
    return t.detach().cpu().numpy()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    x = a.view(np.uint32) if a.dtype == np.float32 else a
    y = b.view(np.uint32) if b.dtype == np.float32 else b
    bad = np.flatnonzero(x.ravel() != y.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {bad[:5]}: {a.ravel()[bad[:5]]} vs {b.ravel()[bad[:5]]}"


def _bridge(toy, T, Tend, dev):
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    return fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(a=-0.5, b=1.),
                                        np.linspace(0, Tend, T + 1), toy["du"], device=dev)


# ---- the sweep's step kernels --------------------------------------------------------------------------------------------
def _sweep_case(case, oracle, dev, monkeypatch):
    """The body of test_gpu_lg.test_fused_sweep_matches_oracle on a collapsed model: two sweeps chained, without and with
    the graph."""
    _, name, N, T, Tend, eb, ef, env, _ = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    toy = D.named_toy(name)
    br = _bridge(toy, T, Tend, dev)
    om = oracle_model_from(oracle, br)
    x0, bs = D.sweep_inputs(toy, N, T)
    sweep = br.sweep_handle(N, eb, ef)
    for trial, use_graph in enumerate((False, True)):
        key = D.sweep_key(oracle, trial)
        want = oracle.gibbs_kernel_lg(om, key, x0, toy["y0"], bs, N, eb, ef, debug=True)
        got = sweep.sweep(key, x0, toy["y0"], bs, use_graph=use_graph)
        v = sweep.views()
        _eq(_np(v["us_T"]), want[4], "final particles")
        _eq(_np(v["lw_T"]), want[5], "final log-weights")
        for i, what in enumerate(OUTPUTS):
            _eq(_np(got[i]), want[i], what)
        x0, bs = want[0], want[2]
    del sweep
    br._sweeps.clear()


@pytest.mark.parametrize("case", D.NARROW, ids=[c[0] for c in D.NARROW])
def test_narrow_sweep_on_a_collapsed_model(case, oracle, dev, monkeypatch):
    """One case per branch of sweep_one_tile_* / sweep_steps_narrow with one slot per thread (the table in
    tests/degenerate.py names the kernel each reaches), at the smallest N that reaches it."""
    _sweep_case(case, oracle, dev, monkeypatch)


def test_propq4_with_whole_tiles_killed(oracle, dev, monkeypatch):
    """k_lg_heaps + k_lg_propQ<4>, N = 200 000: at the collapsed step all but a handful of the 1024 slots of every tile are
    killed, so phase 1 fills the queue to the tile and phase 2 takes two passes; the searches meet a cdf that is one step."""
    _sweep_case(D.PROPQ4, oracle, dev, monkeypatch)


def test_propq16_with_whole_tiles_killed(oracle, dev, monkeypatch):
    """k_lg_propQ<16>, N = 1 100 000: tiles of 4096 slots, eight passes over a full queue, a ragged last tile."""
    _sweep_case(D.PROPQ16, oracle, dev, monkeypatch)


def test_batched_chains_on_a_collapsed_model(oracle, dev):
    """Three chains of one launch sequence with different x0 (so different steps collapse in each), checked per chain."""
    _, name, N, T, Tend, x0s = D.CHAINS
    toy = D.named_toy(name)
    br = _bridge(toy, T, Tend, dev)
    om = oracle_model_from(oracle, br)
    C = len(x0s)
    x0 = np.array(x0s, f32).reshape(C, 1)
    bs = np.tile(D.sweep_inputs(toy, N, T)[1], (C, 1))
    keys = oracle.split(oracle.PRNGKey(5), C)
    sweep = br.sweep_handle(N, True, False, nchains=C)
    got = sweep.sweep(keys, x0, toy["y0"], bs)
    v = sweep.views()
    for c in range(C):
        want = oracle.gibbs_kernel_lg(om, keys[c], x0[c], toy["y0"], bs[c], N, True, False, debug=True)
        for i, what in enumerate(OUTPUTS):
            _eq(_np(got[i][c]), want[i], f"{what} chain {c}")
        _eq(_np(v["us_T"][c]), want[4], f"particles chain {c}")
        _eq(_np(v["lw_T"][c]), want[5], f"log-weights chain {c}")


@pytest.mark.parametrize("case", D.WIDE, ids=[c[0] for c in D.WIDE])
def test_wide_sweep_on_a_collapsed_model(case, oracle, dev):
    """The matrix-core family: one tile, tiled, odd sizes, and three chains just past the switch to k_lgw_gemm_fat."""
    _, du, dv, N, C, T, Tend, _ = case
    toy = D.collapse_gp(du, dv, **D.GP)
    br = _bridge(toy, T, Tend, dev)
    om = oracle_model_from(oracle, br)
    rng = np.random.default_rng(du + N)
    x0 = rng.normal(size=(C, du)).astype(f32)
    bs = rng.integers(0, N, (C, T + 1)).astype(np.int32)
    sweep = br.sweep_handle(N, True, False, nchains=C)
    sq = (lambda a: a[0]) if C == 1 else (lambda a: a)
    un = (lambda a: _np(a)[None]) if C == 1 else _np
    for trial, use_graph in enumerate((False, True)):
        keys = oracle.split(oracle.PRNGKey(7 + trial), max(C, 2))[:C]
        got = sweep.sweep(sq(keys), sq(x0), toy["y0"], sq(bs), use_graph=use_graph)
        v = sweep.views()
        nx0, nbs = x0.copy(), bs.copy()
        for c in range(C):
            want = oracle.gibbs_kernel_lg(om, keys[c], x0[c], toy["y0"], bs[c], N, True, False, debug=True)
            _eq(un(v["us_T"])[c], want[4], f"final particles chain {c}")
            _eq(un(v["lw_T"])[c], want[5], f"final log-weights chain {c}")
            for i, what in enumerate(OUTPUTS):
                _eq(un(got[i])[c], want[i], f"{what} chain {c}")
            nx0[c], nbs[c] = want[0], want[2]
        x0, bs = nx0, nbs
    del sweep
    br._sweeps.clear()


# ---- fused filters -------------------------------------------------------------------------------------------------------
_FILTER_WANT = {}


def _filter_setup(oracle, name, n, dev):
    """Bridge, inputs and the oracle's results of a filter case (computed once, shared by the parametrised tests)."""
    toy = D.named_toy(name)
    br = _bridge(toy, D.FILTER_T, 1.0, dev)
    if (name, n) not in _FILTER_WANT:
        om = oracle_model_from(oracle, br)
        _FILTER_WANT[(name, n)] = (om, D.filter_inputs(oracle, om, toy["y0"], n, 2), {})
    return (br,) + _FILTER_WANT[(name, n)]


@pytest.mark.parametrize("resampling", ["stratified", "systematic"])
@pytest.mark.parametrize("flow", ["bootstrap", "pmcmc"])
@pytest.mark.parametrize("case", D.FILTERS, ids=[f"{m}-{n}" for m, n in D.FILTERS])
def test_fused_filter_on_adversarial_inputs(case, flow, resampling, oracle, dev):
    """filter_handle(n, flow, resampling, nchains=2) on the reversed forward path of a collapsed model and initial
    particles five standard deviations wide: the stratified / systematic searches cross cdfs that are a single step."""
    name, n = case
    br, om, (keys, vs, init), cache = _filter_setup(oracle, name, n, dev)
    fn = oracle.bootstrap_filter_lg if flow == "bootstrap" else oracle.pmcmc_filter_step_lg
    if (flow, resampling) not in cache:
        cache[(flow, resampling)] = [fn(om, keys[c], vs[c], init[c], resampling) for c in range(2)]
    want = cache[(flow, resampling)]
    uT, ell = br.filter_handle(n, flow, resampling, nchains=2).run(keys, _t(vs, dev), _t(init, dev))
    assert uT.shape == (2, n, br.du) and ell.shape == (2,)
    for c in range(2):
        _eq(_np(uT[c]), np.asarray(want[c][0]).reshape(n, br.du), f"chain {c} particles")
        _eq(_np(ell[c]).reshape(1), np.array([want[c][1]], f32), f"chain {c} log-likelihood")
    br._sweeps.clear()


# ---- pMCMC ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [None, 0.1])
@pytest.mark.parametrize("name,n", D.PMCMC)
def test_pmcmc_step_on_a_collapsed_model(name, n, delta, oracle, dev):
    """One fused iteration, two chains.  The proposal's log-likelihood estimate is hugely negative: chain 0 starts from
    log_ell = -3e38 (the oracle accepts), chain 1 from log_ell = 0 (it rejects).  Every MCMCState field bit-equal."""
    toy = D.named_toy(name)
    br = _bridge(toy, D.PMCMC_T, 1.0, dev)
    om = oracle_model_from(oracle, br)
    ref = D.ref_sampler_of(oracle, toy, br)
    keys, uT, ell, ys, mean_path = D.pmcmc_inputs(oracle, om, toy, br)
    h = br.pmcmc_handle(n, "stratified", nchains=2, delta=delta)
    got = h.step(keys, _t(uT, dev), _t(ell, dev), _t(ys, dev), _t(toy["y0"], dev))
    g_uT, g_ell, g_ys = _np(got[0]), _np(got[1]), _np(got[2])
    g_prob, g_acc, g_prop, g_old = (_np(x) for x in got[3])
    outcomes = []
    for c in range(2):
        w = D.pmcmc_oracle_iteration(oracle, om, keys[c], uT[c], ell[c], ys[c], toy["y0"], n, ref, mean_path, delta)
        tag = f"{name} chain {c}"
        _eq(g_uT[c], np.asarray(w[0], f32).reshape(-1), f"uT {tag}")
        _eq(g_ell[c:c + 1], np.array([w[1]], f32), f"log_ell {tag}")
        _eq(g_ys[c], w[2], f"ys {tag}")
        assert bool(g_acc[c]) == w[3], f"is_accepted {tag}"
        _eq(g_prob[c:c + 1], np.array([w[4]], f32), f"acceptance_prob {tag}")
        _eq(g_prop[c:c + 1], np.array([w[5]], f32), f"prop_log_ell {tag}")
        _eq(g_old[c:c + 1], ell[c:c + 1], f"state log_ell {tag}")
        outcomes.append(bool(w[3]))
    assert outcomes == [True, False], "the oracle must accept from -3e38 and reject from 0"
    br._sweeps.clear()


# ---- filter sampler --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("2d", 64), ("2d", 4096), ("gp20", 200)])
def test_filter_sampler_on_a_collapsed_model(name, n, oracle, dev):
    """filter_conditional_sampler at B = 3 through the bridge's own closures (the fused engine) against
    tests/fsamp_restate.py."""
    from fbs_amd import samplers
    toy = D.named_toy(name)
    T = 8
    ts = np.linspace(0, 1.0, T + 1)
    br = _bridge(toy, T, 1.0, dev)
    om = oracle_model_from(oracle, br)
    keys = oracle.split(oracle.PRNGKey(41), 3)
    assert br.fused_filter_sampler_supported(n, 3)
    samples, nell = samplers.filter_conditional_sampler(keys, toy["y0"], ts, br.fwd_ys_sampler, br.ref_sampler,
                                                        br.transition_sampler, br.likelihood_logpdf, n,
                                                        samplers.stratified, return_nell=True)
    assert ("fsamp", n, "stratified", 3) in br._sweeps, "the bridge's closures must take the fused engine"
    assert samples.shape == (3, br.du) and nell.shape == (3,)
    tab = br.pmcmc_tables_host(None)
    for b in range(3):
        w_vs, w_u0s, w_sample, w_nell = R.want(oracle, om, tab, keys[b], toy["y0"], n, "stratified")
        assert np.isfinite(w_sample).all() and np.isfinite(w_nell)
        _eq(_np(samples[b]), w_sample, f"sample {b}")
        _eq(_np(nell[b]).reshape(1), np.array([w_nell], f32), f"nell {b}")
    br._sweeps.clear()


# ---- twisted SMC -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resampling", ["stratified", "systematic"])
@pytest.mark.parametrize("shape", D.TW_SHAPES, ids=["d{}-T{}-N{}".format(*s) for s in D.TW_SHAPES])
def test_twisted_smc_on_a_collapsed_model(shape, resampling, oracle, dev):
    """obs_var = 0.01 and y scaled by 20: the restated run reaches ESS 1 (test_degenerate_inputs.py); ancestors, particles
    and log-weights bit-equal (k_tw_cdf and the search inside k_tw_gemm<0> on single-step cdfs)."""
    d, T, N = shape
    m = D.collapse_tw(d, T, dev)
    xs_w, lws_w, inds_w = Restate(oracle, m).run(oracle.PRNGKey(11), N, resampling)
    h = m.handle(N, resampling, nruns=1, store_ancestors=True)
    xs, lws = h.run(oracle.PRNGKey(11))
    assert xs.shape == (1, N, d) and lws.shape == (1, N)
    _eq(_np(h.views()["ancestors"])[0], inds_w, "ancestors")
    _eq(_np(xs)[0], xs_w, "particles")
    _eq(_np(lws)[0], lws_w, "log-weights")


def test_twisted_sample_on_a_collapsed_model(oracle, dev):
    d, T, N = 10, 6, 257
    m = D.collapse_tw(d, T, dev)
    keys = np.stack([oracle.PRNGKey(s) for s in (11, 12)])
    smp = m.handle(N, "stratified", nruns=2, store_ancestors=True).sample(keys)
    assert smp.shape == (2, d)
    rs = Restate(oracle, m)
    for b in range(2):
        _eq(_np(smp)[b], rs.sample(keys[b], N), f"run {b} sample")
