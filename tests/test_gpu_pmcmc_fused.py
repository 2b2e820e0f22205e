"""GPU parity of the fused pMCMC engine (fbsmi_lg_pmcmc_*, LGPmcmc, samplers.pmcmc_chain) and of the batched fused
filters it stands on, against the oracle on the same keys, bit for bit."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import toy_gp, toy_2d, toy_4d, toy_31, oracle_model_from

pytestmark = pytest.mark.gpu

f32 = np.float32
# start uT, start log_ell, seed of the iteration keys; chain c's ys = lg_fwd_sampler(PRNGKey(1 + c), y0)
STARTS = [(0.3, -40.0, 21), (-0.7, -38.0, 22), (1.1, -36.5, 23), (0.0, -37.0, 24)]


def _np(t):
    return t.detach().cpu().numpy()


def _eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    x = a.view(np.uint32) if a.dtype == np.float32 else a
    y = b.view(np.uint32) if b.dtype == np.float32 else b
    bad = np.flatnonzero(x.ravel() != y.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first {bad[:4]}: {a.ravel()[bad[:4]]} vs {b.ravel()[bad[:4]]}"


def _setup(toy, T, Tend, dev):
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    toy = toy() if callable(toy) else toy
    ts = np.linspace(0, Tend, T + 1)
    br = fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(-0.5, 1.0), ts, toy["du"],
                                      device=dev)
    return toy, ts, br


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- 3. batched fused filters ---------------------------------------------------------------------------------------
FILTER_CASES = [("2d", 64), ("2d", 256), ("2d", 4096), ("2d", 65536), ("2d", 70000), ("gp20", 200), ("gp20", 1000)]


@pytest.mark.parametrize("resampling", ["stratified", "systematic"])
@pytest.mark.parametrize("flow", ["bootstrap", "pmcmc"])
@pytest.mark.parametrize("case", FILTER_CASES, ids=[f"{m}-{n}" for m, n in FILTER_CASES])
def test_batched_fused_filter(case, flow, resampling, oracle, dev):
    """filter_handle(..., nchains=C), C in {2, 3}: chain c is the oracle's filter on chain c's key, vs and particles.
    The sizes cross every branch of the launch sequence: one launch, tree step, three launches per step, wide one-tile,
    wide multi-tile."""
    which, n = case
    toy, ts, br = _setup(toy_2d if which == "2d" else toy_gp(20), 30, 2.0, dev)
    om = oracle_model_from(oracle, br)
    keys, vs, init, want = [], [], [], []
    for c, kc in enumerate(oracle.split(oracle.PRNGKey(3), 3)):
        k1, k2, k3 = oracle.split(kc, 3)
        vs.append(oracle.lg_fwd_sampler(om, k1, toy["y0"])[::-1].copy())
        init.append(oracle.normal(k2, (n, br.du)))
        keys.append(k3)
        if flow == "bootstrap":
            want.append(oracle.bootstrap_filter_lg(om, k3, vs[c], init[c], resampling, return_last=True))
        else:
            want.append(oracle.pmcmc_filter_step_lg(om, k3, vs[c], init[c], resampling))
    keys, vs, init = np.stack(keys), np.stack(vs), np.stack(init)
    for C in (2, 3):
        h = br.filter_handle(n, flow, resampling, nchains=C)
        uT, ell = h.run(keys[:C], _t(vs[:C], dev), _t(init[:C], dev))
        assert uT.shape == (C, n, br.du) and ell.shape == (C,)
        for c in range(C):
            _eq(_np(uT[c]), np.asarray(want[c][0]).reshape(n, br.du), f"C={C} chain {c} particles")
            _eq(_np(ell[c]).reshape(1), np.array([want[c][1]], f32), f"C={C} chain {c} log-likelihood")


# ---- 4./5. one iteration with explicit keys -------------------------------------------------------------------------
def _ref_restated(O, tab, key, yT, n):
    """ref_sampler in the order include/fbsmi.h specifies (elementwise numpy operations round separately)."""
    du = tab["chol"].shape[0]
    y = np.asarray(yT, f32).astype(np.float64).reshape(-1)
    m = np.empty(du, f32)
    for j in range(du):
        s = np.float64(0.0)
        for c in range(y.size):
            s = s + tab["gain"][j, c] * (y[c] - tab["m_v"][c])
        m[j] = f32(tab["m_u"][j] + s)
    z = O.normal(key, (n, du))
    L = tab["chol"]
    acc = z[:, 0:1] * L[0:1, :]
    for c in range(1, du):
        acc = acc + z[:, c:c + 1] * L[c:c + 1, :]
    return (m[None, :] + acc).astype(f32)


def _ref_sampler(O, toy, br, ts):
    """oracle.lg_ref_sampler at du = dv = 1 (where it fixes an order), its restatement otherwise."""
    from fbs_amd.sdes.linear import discretise_linear_sde_np
    if br.du == 1 and br.dv == 1:
        FQ_T = discretise_linear_sde_np(br.sde, ts[-1], ts[0])
        return lambda k, yT, n: O.lg_ref_sampler(toy["m0"], toy["cov0"], FQ_T, 1, k, yT, n)
    tab = br.pmcmc_tables_host(None)
    return lambda k, yT, n: _ref_restated(O, tab, k, yT, n)


def _mean_path(br, ts, y0):
    return (np.asarray(br.sde.mean(ts, ts[0], 1.0), f32).reshape(-1, 1) * y0.reshape(1, -1)).astype(f32)


def _oracle_iteration(O, om, key, uT, log_ell, ys, y0, n, ref, mean_path, delta, resampling="stratified"):
    """oracle.pmcmc_kernel_lg plus the two MCMCState fields it does not return, from the same primitives:
    -> (uT, log_ell, ys, is_accepted, acceptance_prob, prop_log_ell)."""
    want = O.pmcmc_kernel_lg(om, key, uT, log_ell, ys, y0, n, ref, mean_path, delta, resampling=resampling)
    k_prop, k_u0, k_f, _ = O.split(key, 4)
    fwd = lambda k: O.lg_fwd_sampler(om, k, y0)
    prop_ys = fwd(k_prop) if delta is None else O.pcn_proposal(k_prop, delta, np.asarray(ys, f32), mean_path, fwd)
    vs = prop_ys[::-1].copy()
    _, prop_ell = O.pmcmc_filter_step_lg(om, k_f, vs, ref(k_u0, vs[0], n), resampling)
    log_acc = np.minimum(f32(0.0), f32(prop_ell) - f32(log_ell))
    prob = O.exp(np.array([log_acc], f32))[0]
    if want[3]:
        _eq(np.array([want[1]], f32), np.array([prop_ell], f32), "restated prop_log_ell")
    return want + (prob, f32(prop_ell))


def _start(O, om, toy, br, c, ell_shift=0.0):
    u, ell, seed = STARTS[c]
    return (np.full(br.du, u, f32), f32(ell + ell_shift), O.lg_fwd_sampler(om, O.PRNGKey(1 + c), toy["y0"]), O.PRNGKey(seed))


# (name, model, particles, T, iterations, shift of the start log_ell).  The 20-dimensional model's log-likelihood estimates
# lie between -57 and -113 in the oracle's run, so its chains start 45 lower: then they too accept and reject.
STEP_CASES = [("2d", toy_2d, 64, 40, 6, 0.0), ("4d", toy_4d, 64, 40, 6, 0.0), ("31", toy_31, 64, 40, 6, 0.0),
              ("gp20", None, 200, 40, 3, -45.0)]


@pytest.mark.parametrize("delta", [None, 0.1])
@pytest.mark.parametrize("chains", [(1,), (0, 1, 2)], ids=["C1", "C3"])
@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_step_against_oracle(case, chains, delta, oracle, dev):
    """LGPmcmc.step, chained iterations with explicit keys: every output of every chain and iteration equals
    oracle.pmcmc_kernel_lg (du = dv = 1: with oracle.lg_ref_sampler; otherwise with the restated ref_sampler).  For the
    2-D toy, and for every model with three chains, both outcomes of the accept step occur (asserted on the oracle's run)."""
    name, toy, n, T, iters, shift = case
    toy, ts, br = _setup(toy if toy is not None else toy_gp(20), T, 3.0, dev)
    om = oracle_model_from(oracle, br)
    ref, mean_path = _ref_sampler(oracle, toy, br, ts), _mean_path(br, ts, toy["y0"])
    C = len(chains)
    st = [_start(oracle, om, toy, br, c, shift) for c in chains]
    keys = [oracle.split(s[3], iters) for s in st]
    uT, ell, ys = np.stack([s[0] for s in st]), np.array([s[1] for s in st], f32), np.stack([s[2] for s in st])
    h = br.pmcmc_handle(n, "stratified", nchains=C, delta=delta)
    outcomes = []
    for it in range(iters):
        k = np.stack([keys[c][it] for c in range(C)])
        sq = (lambda a: a[0]) if C == 1 else (lambda a: a)
        got = h.step(sq(k), _t(sq(uT), dev), _t(sq(ell), dev), _t(sq(ys), dev), _t(toy["y0"], dev))
        un = (lambda a: _np(a)[None]) if C == 1 else _np
        g_uT, g_ell, g_ys = un(got[0]), un(got[1]), un(got[2])
        g_prob, g_acc, g_prop, g_old = (un(x) for x in got[3])
        for c in range(C):
            w = _oracle_iteration(oracle, om, k[c], uT[c], ell[c], ys[c], toy["y0"], n, ref, mean_path, delta)
            tag = f"{name} chain {chains[c]} it {it}"
            _eq(g_uT[c], np.asarray(w[0], f32).reshape(-1), f"uT {tag}")
            _eq(g_ell[c:c + 1], np.array([w[1]], f32), f"log_ell {tag}")
            _eq(g_ys[c], w[2], f"ys {tag}")
            assert bool(g_acc[c]) == w[3], f"is_accepted {tag}"
            _eq(g_prob[c:c + 1], np.array([w[4]], f32), f"acceptance_prob {tag}")
            _eq(g_prop[c:c + 1], np.array([w[5]], f32), f"prop_log_ell {tag}")
            _eq(g_old[c:c + 1], ell[c:c + 1], f"state log_ell {tag}")
            outcomes.append(w[3])
            uT[c], ell[c], ys[c] = np.asarray(w[0], f32).reshape(-1), w[1], w[2]
    if name == "2d" or C == 3:
        assert any(outcomes) and not all(outcomes), "the oracle's run must both accept and reject"


# ---- 6. the chained entry point -------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [None, 0.1])
@pytest.mark.parametrize("C", [1, 4])
def test_chain_equals_steps_with_the_driver_schedule(C, delta, oracle, dev):
    """chain(key, ..., nsamples=8) == eight step calls with key, subkey = split(key); split(subkey, C) on the host --
    C = 1 included -- and returns the advanced key; with and without the captured graph, and a second call on the same
    handle continues from the first's state."""
    toy, ts, br = _setup(toy_2d, 40, 3.0, dev)
    om = oracle_model_from(oracle, br)
    st = [_start(oracle, om, toy, br, c) for c in range(C)]
    y0 = _t(toy["y0"], dev)
    sq = (lambda a: a[0]) if C == 1 else (lambda a: a)
    state0 = (_t(sq(np.stack([s[0] for s in st])), dev), _t(sq(np.array([s[1] for s in st], f32)), dev),
              _t(sq(np.stack([s[2] for s in st])), dev))
    h = br.pmcmc_handle(64, "stratified", nchains=C, delta=delta)
    # host-side schedule, 16 iterations
    key = oracle.PRNGKey(77)
    state, want = state0, []
    for i in range(16):
        key, subkey = oracle.split(key, 2)
        kc = oracle.split(subkey, C)
        out = h.step(sq(kc), *state, y0)
        state = out[:3]
        want.append((_np(out[0]),) + tuple(_np(x) for x in out[3]))
    key16 = key
    for use_graph in (True, False):
        k8, uT, ell, ys, samples, ms = h.chain(oracle.PRNGKey(77), *state0, y0, 8, use_graph=use_graph)
        k16, uT2, ell2, ys2, samples2, ms2 = h.chain(k8, uT, ell, ys, y0, 8, use_graph=use_graph)
        _eq(np.asarray(k16, np.uint32), np.asarray(key16, np.uint32), "advanced key")
        assert samples.shape == ((8, 1) if C == 1 else (8, C, 1))
        got_s = np.concatenate([_np(samples), _np(samples2)])
        for i in range(16):
            _eq(got_s[i], want[i][0], f"sample {i} graph={use_graph}")
            for f, name in enumerate(("acceptance_prob", "is_accepted", "prop_log_ell", "log_ell")):
                g = np.concatenate([_np(ms[f]), _np(ms2[f])])[i]
                _eq(np.asarray(g), np.asarray(want[i][1 + f]), f"{name} {i} graph={use_graph}")
        _eq(_np(uT2), _np(state[0]), "final uT")
        _eq(_np(ell2), _np(state[1]), "final log_ell")
        _eq(_np(ys2), _np(state[2]), "final ys")


# ---- 7. the two tiers of samplers.pmcmc_chain -----------------------------------------------------------------------
@pytest.mark.parametrize("delta", [None, 0.1])
def test_pmcmc_chain_tiers_agree(delta, oracle, dev, monkeypatch):
    from fbs_amd import samplers
    from fbs_amd import linear_gaussian as LG
    toy, ts, br = _setup(toy_2d, 40, 3.0, dev)
    om = oracle_model_from(oracle, br)
    C, n, ns = 3, 64, 6
    st = [_start(oracle, om, toy, br, c) for c in range(C)]
    args = (_t(np.stack([s[0] for s in st]), dev), _t(np.array([s[1] for s in st], f32), dev),
            _t(np.stack([s[2] for s in st]), dev), _t(toy["y0"], dev), ts)
    fused_calls = []
    real_chain = LG.LGPmcmc.chain
    monkeypatch.setattr(LG.LGPmcmc, "chain", lambda self, *a, **k: (fused_calls.append(1), real_chain(self, *a, **k))[1])
    closures = (br.fwd_ys_sampler, br.sde, br.ref_sampler, br.transition_sampler, br.likelihood_logpdf)
    fused = samplers.pmcmc_chain(oracle.PRNGKey(5), *args, *closures, samplers.stratified, n, ns, delta=delta)
    assert fused_calls == [1], "the bridge's own closures must take the fused engine"
    hide = lambda fn: (lambda *a, **k: fn(*a, **k))      # a plain lambda hides the bridge: the loop tier runs
    plain = (hide(br.fwd_ys_sampler), br.sde, hide(br.ref_sampler), hide(br.transition_sampler), hide(br.likelihood_logpdf))
    loop = samplers.pmcmc_chain(oracle.PRNGKey(5), *args, *plain, samplers.stratified, n, ns, delta=delta)
    assert fused_calls == [1]
    _eq(np.asarray(fused[0], np.uint32), np.asarray(loop[0], np.uint32), "key")
    for i, name in ((1, "uTs"), (2, "log_ells"), (3, "yss"), (4, "samples")):
        assert fused[i].shape == loop[i].shape, name
        _eq(_np(fused[i]), _np(loop[i]), name)
    assert fused[4].shape == (ns, C, 1)
    for name in ("is_accepted", "prop_log_ell", "log_ell"):
        _eq(_np(getattr(fused[5], name)), _np(getattr(loop[5], name)), name)
    acc = _np(fused[5].is_accepted)
    assert acc.any() and not acc.all()
    # acceptance_prob: the fused tier evaluates fbsmi_expf (pinned to the oracle in the tests above), pmcmc_kernel's host
    # path torch.exp.  Two float32 exponentials, each within 2 ulp of the true value, differ by at most 4 ulp = 4 * 2^-23
    # relative; where the proposal is accepted both are exp(0) = 1 exactly.
    a, b = _np(fused[5].acceptance_prob).astype(np.float64), _np(loop[5].acceptance_prob).astype(np.float64)
    assert np.all(np.abs(a - b) <= 4 * 2.0 ** -23 * np.abs(b))
    # a resampler the fused filter does not have: the loop tier, without error
    out = samplers.pmcmc_chain(oracle.PRNGKey(5), *args, *closures, samplers.multinomial, n, 2, delta=delta)
    assert fused_calls == [1] and out[4].shape == (2, C, 1) and torch.isfinite(out[4]).all()


# ---- 8. the driver --------------------------------------------------------------------------------------------------
def test_toy_pmcmc_driver_fused(tmp_path, dev):
    """examples/toy_pmcmc.py --fused at the arguments of test_gpu_lg.py::test_toy_filter_and_pmcmc_drivers: the same
    assertions as the unfused driver meets there."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import sys
    sys.path.insert(0, os.path.join(root, "examples"))
    try:
        spec = importlib.util.spec_from_file_location("toy_pmcmc_fused", os.path.join(root, "examples", "toy_pmcmc.py"))
        pm = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(pm)
    finally:
        sys.path.remove(os.path.join(root, "examples"))
    samples, gp_mean, gp_cov = pm.main(["--d", "20", "--nparticles", "200", "--nsamples", "150", "--nchains", "2",
                                        "--delta", "0.005", "--outdir", str(tmp_path), "--quiet", "--fused"])
    assert samples.shape == (2, 150, 20) and np.isfinite(samples).all()
    z = (samples[:, 50:].reshape(-1, 20).mean(0) - gp_mean) / np.sqrt(np.diag(gp_cov))
    assert np.abs(z).max() < 2.5
    assert set(np.load(os.path.join(str(tmp_path), "pmcmc-0.005-const-200-666.npz")).files) == {"samples", "gp_mean", "gp_cov"}


# ---- 9. a long chain, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.1, None])
def test_long_chain_against_oracle_loop(delta, oracle, dev):
    """200 iterations of four chains in one chain() call: every sample and every MCMCState field equals the oracle loop
    (hundreds of accept / reject decisions, both outcomes)."""
    toy, ts, br = _setup(toy_2d, 40, 3.0, dev)
    om = oracle_model_from(oracle, br)
    C, n, ns = 4, 64, 200
    ref, mean_path = _ref_sampler(oracle, toy, br, ts), _mean_path(br, ts, toy["y0"])
    st = [_start(oracle, om, toy, br, c) for c in range(C)]
    uT, ell, ys = np.stack([s[0] for s in st]), np.array([s[1] for s in st], f32), np.stack([s[2] for s in st])
    h = br.pmcmc_handle(n, "stratified", nchains=C, delta=delta)
    k_out, g_uT, g_ell, g_ys, samples, ms = h.chain(oracle.PRNGKey(9), _t(uT, dev), _t(ell, dev), _t(ys, dev),
                                                    _t(toy["y0"], dev), ns)
    samples, ms = _np(samples), [_np(x) for x in ms]
    key = oracle.PRNGKey(9)
    naccept = 0
    for i in range(ns):
        key, subkey = oracle.split(key, 2)
        for c, kc in enumerate(oracle.split(subkey, C)):
            old = ell[c]
            w = _oracle_iteration(oracle, om, kc, uT[c], ell[c], ys[c], toy["y0"], n, ref, mean_path, delta)
            uT[c], ell[c], ys[c] = np.asarray(w[0], f32).reshape(-1), w[1], w[2]
            tag = f"iteration {i} chain {c}"
            _eq(samples[i, c], uT[c], f"sample {tag}")
            _eq(ms[0][i, c:c + 1], np.array([w[4]], f32), f"acceptance_prob {tag}")
            assert bool(ms[1][i, c]) == w[3], f"is_accepted {tag}"
            _eq(ms[2][i, c:c + 1], np.array([w[5]], f32), f"prop_log_ell {tag}")
            _eq(ms[3][i, c:c + 1], np.array([old], f32), f"log_ell {tag}")
            naccept += int(w[3])
    assert 0 < naccept < ns * C
    _eq(np.asarray(k_out, np.uint32), np.asarray(key, np.uint32), "advanced key")
    _eq(_np(g_uT), uT, "final uT")
    _eq(_np(g_ell), ell, "final log_ell")
    _eq(_np(g_ys), ys, "final ys")


def test_sb_model_is_left_to_the_loop(dev):
    """A model with an Euler-Maruyama forward process has no exact proposal path: no fused handle, at either layer."""
    import ctypes as C
    import fbs_amd
    from fbs_amd import _lib
    rng = np.random.default_rng(0)
    A = rng.normal(size=(2, 2))
    cov = A @ A.T + np.eye(2)
    sb = fbs_amd.GaussianSBBridge(np.zeros(2), np.eye(2), np.array([0.5, -0.5]), cov, np.linspace(0, 1, 11), du=1,
                                  device=dev)
    assert not sb.fused_pmcmc_supported(64)
    with pytest.raises(NotImplementedError):
        sb.pmcmc_handle(64)
    lg = _setup(toy_2d, 10, 1.0, dev)[2]
    h = C.c_void_p()
    with pytest.raises(NotImplementedError):       # FBSMI_ERR_UNSUPPORTED: F and sqQ are all-zero placeholders
        _lib.call("fbsmi_lg_pmcmc_create", C.byref(sb.struct), C.byref(lg.pmcmc_tables(None)), 64, 0, 1, C.byref(h))
