"""CPU: tests/diag_restate.py rebuilds the right vectors.  The (lse, ess) rows tests/test_gpu_diag.py holds the device to are
oracle.logsumexp / oracle.ess of log-weight vectors re-derived from the oracle's stored passes; here every such vector is tied
back, bit for bit, to what the oracle itself computed from it."""
import numpy as np
import pytest

import degenerate as D
import diag_restate as R
from helpers import bits, oracle_model_from, toy_2d, toy_4d, toy_gp

f32 = np.float32
MODELS = {"2d": toy_2d, "4d": toy_4d, "gp24": lambda: toy_gp(24)}


def _om(oracle, toy, T, Tend=1.0):
    return oracle_model_from(oracle, D.cpu_bridge(toy, T, Tend))


@pytest.mark.parametrize("eb,ef", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("N", [10, 300])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_sweep_vectors_normalise_to_the_stored_log_weights(model, N, eb, ef, oracle):
    """lw_k - lse_k is the oracle's stored log_wss[k], for every k; and the pass is the sweep's own."""
    toy, T = MODELS[model](), 6
    om = _om(oracle, toy, T)
    x0, bs = D.sweep_inputs(toy, N, T)
    key = D.sweep_key(oracle)
    lws, stored = R.sweep_lws(oracle, om, key, x0, toy["y0"], bs, N, eb, ef)
    lse, ess = R.rows_of(oracle, lws)
    assert len(lws) == T + 1 and stored.shape == (T + 1, N + int(ef))
    for k in range(T + 1):
        assert np.array_equal(bits((lws[k] - lse[k]).astype(f32)), bits(stored[k])), k
    want = oracle.gibbs_kernel_lg(om, key, x0, toy["y0"], bs, N, eb, ef, debug=True)
    assert np.array_equal(bits(stored[-1]), bits(want[5]))
    assert np.all(ess >= 1.0 - 1e-6) and np.all(ess <= (N + int(ef)) * (1.0 + 1e-6))
    if not ef:   # N equal weights -log N: lse = 0 up to the rounding of N * exp(-log N), ess = N likewise
        assert abs(float(lse[0])) < 1e-5 and abs(float(ess[0]) - N) < 1e-3 * N


@pytest.mark.parametrize("resampling", ["stratified", "systematic"])
@pytest.mark.parametrize("model,n", [("2d", 10), ("4d", 300), ("gp24", 100)])
def test_filter_vectors_reproduce_the_oracles_likelihoods(model, n, resampling, oracle):
    toy, T = MODELS[model](), 6
    om = _om(oracle, toy, T)
    keys, vs, init = D.filter_inputs(oracle, om, toy["y0"], n, nchains=1)
    # flow 1: the restatement is the oracle's pmcmc_filter_step
    lws1, uT, ell = R.pmcmc_restated(oracle, om, keys[0], vs[0], init[0], resampling)
    want_uT, want_ell = oracle.pmcmc_filter_step_lg(om, keys[0], vs[0], init[0], resampling)
    assert np.array_equal(bits(uT), bits(want_uT)) and bits(np.array([ell], f32))[0] == bits(np.array([want_ell], f32))[0]
    assert len(lws1) == T
    # flow 0: the negative log-likelihood, re-accumulated from the lse column in the oracle's order
    lws0, nell = R.bootstrap_lws(oracle, om, keys[0], vs[0], init[0], resampling)
    lse, _ = R.rows_of(oracle, lws0)
    assert bits(np.array([R.nell_from_lse(lse, n)], f32))[0] == bits(np.array([nell], f32))[0]


def _ess64(O, log_ws):
    """1 / sum w^2 in float64 of the float32 weights exp(log_ws[k]) (normalised log-weights)."""
    return np.array([1.0 / (O.exp(np.asarray(lw, f32)).astype(np.float64) ** 2).sum() for lw in log_ws])


def test_collapsed_sweep_rows_show_the_collapse(oracle):
    """On collapsed inputs of tests/degenerate.py the restated ESS rows give what tests/test_degenerate_inputs.py asserts of
    the same passes: a step the killing resampler is handed with ESS < 2 (and zero_frac >= 0.9 there).  They are 1 / sum w^2
    of the stored float32 weights (_ess64: the same terms summed in float64; the tree sum of n <= 2048 float32 terms and one
    division stay within 1e-5 of it).  That is NOT degenerate.profile_of's (sum w)^2 / sum w^2 where log-weights of
    magnitude 1e6 leave the float32 weights summing to 1 only within a few per cent."""
    for case in (D.NARROW[0], D.NARROW[3]):
        _, name, N, T, Tend, eb, ef, _, _ = case
        toy = D.named_toy(name)
        om = _om(oracle, toy, T, Tend)
        x0, bs = D.sweep_inputs(toy, N, T)
        lws, stored = R.sweep_lws(oracle, om, D.sweep_key(oracle), x0, toy["y0"], bs, N, eb, ef)
        _, ess = R.rows_of(oracle, lws)
        _, zero, _ = D.profile_of(oracle, stored)
        np.testing.assert_allclose(ess, _ess64(oracle, stored), rtol=1e-5)
        assert np.any((ess[:T] < 2) & (zero[:T] >= min(0.9, 1.0 - 1.0 / N))), (case[0], ess, zero)


def test_collapsed_filter_rows_show_the_collapse(oracle):
    name, n = D.FILTERS[0]
    toy = D.named_toy(name)
    om = _om(oracle, toy, D.FILTER_T)
    keys, vs, init = D.filter_inputs(oracle, om, toy["y0"], n)
    lws, _ = R.bootstrap_lws(oracle, om, keys[0], vs[0], init[0], "stratified")
    _, ess = R.rows_of(oracle, lws)
    _, zero, _ = D.filter_weight_profile(oracle, om, keys[0], vs[0], init[0], "stratified")
    np.testing.assert_allclose(ess, _ess64(oracle, [oracle.normalise(lw, True) for lw in lws]), rtol=1e-5)
    assert np.any((ess < 2) & (zero >= 0.9))
