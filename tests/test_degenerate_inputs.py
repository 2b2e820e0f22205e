"""The inputs of tests/test_gpu_degenerate.py really are degenerate, and the oracle stays finite on them.  CPU only.

For every collapsed model at the (N, T) the GPU tests use, on the oracle's own stored log-weights:
  * every oracle output is finite, no NaN anywhere;
  * at least one step has ESS < 2 and zero_frac >= 0.9 -- here demanded of a step the killing resampler is handed
    (rows 0 .. T - 1 of log_wss), which is stricter than "any step";
  * at least one such step has kill_frac >= 0.95.
zero_frac and kill_frac = 1 - mean(w) / max(w) cannot exceed 1 - 1/n for n slots, so for the one-launch case of n = 10
slots both bounds are that maximum (0.9: nine of ten weights exactly zero), for every other case the figures above."""
import numpy as np
import pytest

import degenerate as D
from helpers import oracle_model_from
from tw_restate import Restate

f32 = np.float32


def _finite(*arrays):
    return all(np.isfinite(np.asarray(a, np.float64)).all() for a in arrays)


def _assert_collapsed(ess, zero, kill, n, what):
    print(f"{what}: min ESS {ess.min():.3g}, max zero_frac {zero.max():.4g}, max kill_frac {kill.max():.6g}")
    cap = 1.0 - 1.0 / n
    assert np.any((ess < 2) & (zero >= min(0.9, cap))), (what, ess, zero)
    assert np.any(kill >= min(0.95, cap)), (what, kill)


SWEEPS = D.NARROW + [D.PROPQ4, D.PROPQ16]


@pytest.mark.parametrize("case", SWEEPS, ids=[c[0] for c in SWEEPS])
def test_narrow_sweep_inputs_collapse(case, oracle):
    _, name, N, T, Tend, eb, ef, _, _ = case
    toy = D.named_toy(name)
    om = oracle_model_from(oracle, D.cpu_bridge(toy, T, Tend))
    x0, bs = D.sweep_inputs(toy, N, T)
    key = D.sweep_key(oracle)
    lws = D.forward_log_wss(oracle, om, key, x0, toy["y0"], bs, N, eb, ef)
    out = oracle.gibbs_kernel_lg(om, key, x0, toy["y0"], bs, N, eb, ef, debug=True)
    assert _finite(lws, *out)
    # the stored pass is the sweep's own: its last row is the sweep's final log-weights
    assert np.array_equal(lws[-1].view(np.uint32), out[5].view(np.uint32))
    ess, zero, kill = D.profile_of(oracle, lws[:T])
    _assert_collapsed(ess, zero, kill, N + int(ef), case[0])


def test_batched_chains_inputs_collapse(oracle):
    _, name, N, T, Tend, x0s = D.CHAINS
    toy = D.named_toy(name)
    om = oracle_model_from(oracle, D.cpu_bridge(toy, T, Tend))
    _, bs = D.sweep_inputs(toy, N, T)
    keys = oracle.split(oracle.PRNGKey(5), len(x0s))
    profiles = []
    for c, x0 in enumerate(x0s):
        lws = D.forward_log_wss(oracle, om, keys[c], np.array([x0], f32), toy["y0"], bs, N)
        assert _finite(lws, *oracle.gibbs_kernel_lg(om, keys[c], np.array([x0], f32), toy["y0"], bs, N, debug=True))
        profiles.append(D.profile_of(oracle, lws[:T]))
    # y0 is shared and it is y0 that collapses this model: no x0 gives a benign chain (x0 = E[x0 | y0] = 1996.998 still
    # collapses at every other step), so chains 0 and 1 are held to the conditions; chain 2 (x0 = 7) is the mildest the model
    # gives, ESS between 1.7 and 127 on its collapsed steps
    for c in (0, 1):
        _assert_collapsed(*profiles[c], N, f"chain {c}")
    ess, zero, kill = profiles[2]
    print(f"chain 2: min ESS {ess.min():.3g}, max zero_frac {zero.max():.4g}, max kill_frac {kill.max():.6g}")
    assert ess[2:].min() < 2 and ess[2:].max() > 100


@pytest.mark.parametrize("case", D.WIDE, ids=[c[0] for c in D.WIDE])
def test_wide_sweep_inputs_collapse(case, oracle):
    _, du, dv, N, C, T, Tend, _ = case
    toy = D.collapse_gp(du, dv, **D.GP)
    om = oracle_model_from(oracle, D.cpu_bridge(toy, T, Tend))
    rng = np.random.default_rng(du + N)
    x0 = rng.normal(size=(C, du)).astype(f32)
    bs = rng.integers(0, N, (C, T + 1)).astype(np.int32)
    keys = oracle.split(oracle.PRNGKey(7), max(C, 2))
    for c in range(C):
        lws = D.forward_log_wss(oracle, om, keys[c], x0[c], toy["y0"], bs[c], N)
        assert _finite(lws, *oracle.gibbs_kernel_lg(om, keys[c], x0[c], toy["y0"], bs[c], N, debug=True))
        _assert_collapsed(*D.profile_of(oracle, lws[:T]), N, f"{case[0]} chain {c}")


@pytest.mark.parametrize("resampling", ["stratified", "systematic"])
@pytest.mark.parametrize("case", D.FILTERS, ids=[f"{m}-{n}" for m, n in D.FILTERS])
def test_filter_inputs_collapse(case, resampling, oracle):
    name, n = case
    toy = D.named_toy(name)
    om = oracle_model_from(oracle, D.cpu_bridge(toy, D.FILTER_T, 1.0))
    keys, vs, init = D.filter_inputs(oracle, om, toy["y0"], n)
    for c in range(3):
        uT, nell = oracle.bootstrap_filter_lg(om, keys[c], vs[c], init[c], resampling)
        uT2, ell = oracle.pmcmc_filter_step_lg(om, keys[c], vs[c], init[c], resampling)
        assert _finite(uT, nell, uT2, ell, vs[c])
    _assert_collapsed(*D.filter_weight_profile(oracle, om, keys[0], vs[0], init[0], resampling), n, f"{name}-{n}")


@pytest.mark.parametrize("resampling", ["stratified", "systematic"])
@pytest.mark.parametrize("shape", D.TW_SHAPES, ids=["d{}-T{}-N{}".format(*s) for s in D.TW_SHAPES])
def test_twisted_inputs_collapse(shape, resampling, oracle):
    d, T, N = shape
    rs = Restate(oracle, D.collapse_tw(d, T, "cpu"))
    (xs, lws, inds), seen = D.tw_run_recording(oracle, rs, oracle.PRNGKey(11), N, resampling)
    assert xs.shape == (N, d) and inds.shape == (T, N) and _finite(xs, lws, *seen)
    ess, zero, kill = D.profile_of_weights(seen)
    print(f"d{d}-T{T}-N{N} {resampling}: min ESS {ess.min():.3g}, max zero_frac {zero.max():.4g}, max kill_frac {kill.max():.6g}")
    assert ess.min() < 2


@pytest.mark.parametrize("delta", [None, 0.1])
@pytest.mark.parametrize("name,n", D.PMCMC)
def test_pmcmc_inputs_accept_and_reject(name, n, delta, oracle):
    toy = D.named_toy(name)
    br = D.cpu_bridge(toy, D.PMCMC_T, 1.0)
    om = oracle_model_from(oracle, br)
    ref = D.ref_sampler_of(oracle, toy, br)
    keys, uT, ell, ys, mean_path = D.pmcmc_inputs(oracle, om, toy, br)
    outcomes = []
    for c in range(2):
        w = D.pmcmc_oracle_iteration(oracle, om, keys[c], uT[c], ell[c], ys[c], toy["y0"], n, ref, mean_path, delta)
        print(f"{name} delta={delta} chain {c}: prop_log_ell {w[5]:.6g}, accepted {w[3]}")
        assert _finite(w[0], w[2], w[4], w[5]) and w[5] < -1000     # hugely negative, yet finite
        outcomes.append(bool(w[3]))
    assert outcomes == [True, False]


@pytest.mark.parametrize("name,n", [("2d", 64), ("2d", 4096), ("gp20", 200)])
def test_filter_sampler_inputs_stay_finite(name, n, oracle):
    import fsamp_restate
    toy = D.named_toy(name)
    br = D.cpu_bridge(toy, 8, 1.0)
    om = oracle_model_from(oracle, br)
    for key in oracle.split(oracle.PRNGKey(41), 3):
        assert _finite(*fsamp_restate.want(oracle, om, br.pmcmc_tables_host(None), key, toy["y0"], n, "stratified"))
