"""GPU parity of the fused backward simulation (fbsmi_lg_backsim, LGBacksim): bootstrap_backward_smoother (mode
'smoother') against oracle.backward_smoother_lg and backward_sampling_pass (mode 'sampling') against
oracle.backward_sampling_pass_lg, bit for bit on the same keys, chain c of a batch against the oracle on chain c's inputs.

The shapes are the smallest at which each code path can go wrong: one tile (n <= 256, the whole pass in one launch per chunk
of means) and several tiles (a launch per stage) on both sides of 256 and of the tile multiples, ensembles that are no
multiple of the 64-slot tiles of the mean pre-pass, models with du != dv, and wide models that are ragged against its row
blocks; T = 20 crosses the 16-step chunk of the mean workspace."""
import numpy as np
import pytest
import torch

from helpers import oracle_model_from, toy_2d, toy_31, toy_4d, toy_gp
from sb_restate import sb_problem

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    x = a.view(np.uint32) if a.dtype == np.float32 else a
    y = b.view(np.uint32) if b.dtype == np.float32 else b
    bad = np.flatnonzero(x.ravel() != y.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first {bad[:4]}: {a.ravel()[bad[:4]]} vs {b.ravel()[bad[:4]]}"


def toy_gp20():
    return toy_gp(20)


def toy_gp33_7():
    return toy_gp(33, dv=7)


def toy_gp100():
    return toy_gp(100)


def _setup(toy, T, dev, Tend=1.0):
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    toy = toy()
    ts = np.linspace(0, Tend, T + 1)
    br = fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(-0.5, 1.0), ts, toy["du"], device=dev)
    return toy, ts, br


# (model, n, T, chains): every n of {1, 2, 10, 255, 256, 257, 513, 777, 1024, 4097} and T of {1, 7, 20}; one case per kernel
# family for the larger n
CASES = [
    (toy_2d, 1, 1, 1), (toy_2d, 1, 7, 3), (toy_2d, 2, 7, 1), (toy_2d, 10, 20, 3), (toy_2d, 255, 7, 1), (toy_2d, 256, 20, 1),
    (toy_2d, 257, 7, 3), (toy_2d, 513, 20, 1), (toy_2d, 4097, 7, 1),
    (toy_4d, 10, 1, 1), (toy_4d, 256, 7, 3), (toy_4d, 777, 7, 1), (toy_4d, 1024, 1, 3),
    (toy_31, 2, 20, 1), (toy_31, 255, 7, 3), (toy_31, 257, 1, 1), (toy_31, 1024, 7, 1),
    (toy_gp20, 10, 7, 1), (toy_gp20, 256, 7, 1), (toy_gp20, 513, 20, 3),
    (toy_gp33_7, 1, 7, 1), (toy_gp33_7, 255, 7, 3), (toy_gp33_7, 257, 20, 1), (toy_gp33_7, 777, 1, 1),
    (toy_gp100, 100, 5, 1),
]
_IDS = [f"{c[0].__name__}-n{c[1]}-T{c[2]}-C{c[3]}" for c in CASES]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _smoother_inputs(oracle, om, toy, n, c):
    """A bootstrap-filter path (with the duplicate particles resampling creates) and its observation path."""
    k1, k2, k3, k4 = oracle.split(oracle.PRNGKey(100 + 7 * c + n), 4)
    vs = oracle.lg_fwd_sampler(om, k1, toy["y0"])[::-1].copy()
    init = oracle.normal(k2, (n, om.du))
    filt, _ = oracle.bootstrap_filter_lg(om, k3, vs, init, "stratified", return_last=False)
    return k4, vs, filt


def _sampling_inputs(oracle, om, n, c):
    """uss / log_wss of a CSMC forward pass with n slots."""
    rng = np.random.default_rng(1000 + 13 * c + n)
    T = om.T
    us_star = (0.5 * rng.normal(size=(T + 1, om.du))).astype(np.float32)
    vs = (0.5 * rng.normal(size=(T + 1, om.dv))).astype(np.float32)
    bs = rng.integers(0, n, T + 1).astype(np.int32)
    us0 = rng.normal(size=(n, om.du)).astype(np.float32)
    lw0 = rng.normal(size=n).astype(np.float32)
    k_fwd, k_bwd = oracle.split(oracle.PRNGKey(200 + 5 * c + n), 2)
    fp = oracle.csmc_forward_pass_lg(om, k_fwd, us_star, bs, vs, us0, lw0)
    assert np.isfinite(fp["log_wss"].max(axis=1)).all()
    return k_bwd, vs, fp["uss"], fp["log_wss"]


@pytest.mark.parametrize("toy,n,T,C", CASES, ids=_IDS)
def test_smoother_matches_oracle(toy, n, T, C, oracle, dev):
    toy, ts, br = _setup(toy, T, dev)
    om = oracle_model_from(oracle, br)
    ins = [_smoother_inputs(oracle, om, toy, n, c) for c in range(C)]
    h = br.backsim_handle(n, "smoother", C)
    stack = lambda j: _t(np.stack([i[j] for i in ins]) if C > 1 else ins[0][j], dev)
    got = _np(h.run(stack(0), stack(1), stack(2)))
    got = got if C > 1 else got[None]
    for c, (key, vs, filt) in enumerate(ins):
        _eq(got[c], oracle.backward_smoother_lg(om, key, filt, vs), f"smoother trajectory, chain {c}")


@pytest.mark.parametrize("toy,n,T,C", CASES, ids=_IDS)
def test_backward_sampling_matches_oracle(toy, n, T, C, oracle, dev):
    toy, ts, br = _setup(toy, T, dev)
    om = oracle_model_from(oracle, br)
    ins = [_sampling_inputs(oracle, om, n, c) for c in range(C)]
    h = br.backsim_handle(n, "sampling", C)
    stack = lambda j: _t(np.stack([i[j] for i in ins]) if C > 1 else ins[0][j], dev)
    xs, Bs = h.run(stack(0), stack(1), stack(2), stack(3))
    xs, Bs = (_np(xs), _np(Bs)) if C > 1 else (_np(xs)[None], _np(Bs)[None])
    for c, (key, vs, uss, lws) in enumerate(ins):
        wxs, wBs = oracle.backward_sampling_pass_lg(om, key, vs, uss, lws)
        _eq(Bs[c], wBs, f"Bs, chain {c}")
        _eq(xs[c], wxs, f"xs, chain {c}")


@pytest.mark.parametrize("toy,n", [(toy_4d, 40), (toy_gp20, 300)])
def test_csmc_kernel_backward_sampling_end_to_end(toy, n, oracle, dev):
    from fbs_amd.samplers.csmc.csmc import csmc_kernel
    from fbs_amd.samplers.csmc.resamplings import killing
    T = 7
    toy, ts, br = _setup(toy, T, dev)
    om = oracle_model_from(oracle, br)
    rng = np.random.default_rng(n)
    us_star = (0.5 * rng.normal(size=(T + 1, br.du))).astype(np.float32)
    vs = (0.5 * rng.normal(size=(T + 1, br.dv))).astype(np.float32)
    bs = rng.integers(0, n + 1, T + 1).astype(np.int32)
    us0 = rng.normal(size=(n + 1, br.du)).astype(np.float32)
    lw0 = rng.normal(size=n + 1).astype(np.float32)
    key = oracle.PRNGKey(12)
    h = br.backsim_handle(n + 1, "sampling")
    r0 = h.runs
    xs, Bs = csmc_kernel(key, _t(us_star, dev), bs, _t(vs, dev), ts, lambda k_, m_: _t(us0, dev), lambda v0, u0s, v1: _t(lw0, dev),
                         br.transition_sampler, br.transition_logpdf, br.likelihood_logpdf, killing, n, backward=True)
    assert h.runs == r0 + 1
    wxs, wBs = oracle.csmc_kernel_lg(om, key, us_star, bs, vs, us0, lw0, backward=True)
    _eq(_np(Bs), wBs, "Bs")
    _eq(_np(xs), wxs, "xs")


@pytest.mark.parametrize("n", [100, 600])
def test_backward_sampling_with_minus_infinity_weights(n, oracle, dev):
    """A fixed-seed input with -inf among the stored log-weights (at least one finite entry per time step): the oracle
    alone returns in-range indices of finite weight, and the engine returns the same."""
    T = 7
    toy, ts, br = _setup(toy_4d, T, dev)
    om = oracle_model_from(oracle, br)
    rng = np.random.default_rng(77 + n)
    uss = rng.normal(size=(T + 1, n, br.du)).astype(np.float32)
    vs = rng.normal(size=(T + 1, br.dv)).astype(np.float32)
    lws = rng.normal(size=(T + 1, n)).astype(np.float32)
    lws[rng.random(size=lws.shape) < 0.3] = -np.inf
    lws[:, 3] = rng.normal(size=T + 1).astype(np.float32)
    lws[2, :] = -np.inf
    lws[2, n - 1] = 0.0                                         # one finite entry, the last slot
    lws = np.stack([oracle.normalise(r, log_space=True) for r in lws]).astype(np.float32)
    key = oracle.PRNGKey(5)
    wxs, wBs = oracle.backward_sampling_pass_lg(om, key, vs, uss, lws)
    assert ((wBs >= 0) & (wBs < n)).all() and wBs[2] == n - 1
    assert np.isfinite(lws[np.arange(T + 1), wBs]).all()
    xs, Bs = br.backsim_handle(n, "sampling").run(key, _t(vs, dev), _t(uss, dev), _t(lws, dev))
    _eq(_np(Bs), wBs, "Bs")
    _eq(_np(xs), wxs, "xs")


def test_samplers_dispatch_to_the_handle(oracle, dev):
    from fbs_amd.samplers import smc
    from fbs_amd.samplers.csmc.csmc import backward_sampling_pass
    T, n = 20, 300
    toy, ts, br = _setup(toy_2d, T, dev)
    om = oracle_model_from(oracle, br)
    key, vs, filt = _smoother_inputs(oracle, om, toy, n, 0)
    wrapped = lambda *a: br.transition_logpdf(*a)
    h = br.backsim_handle(n, "smoother")
    r0 = h.runs
    a = smc.bootstrap_backward_smoother(key, _t(filt, dev), _t(vs, dev), ts, br.transition_logpdf)
    assert h.runs == r0 + 1
    b = smc.bootstrap_backward_smoother(key, _t(filt, dev), _t(vs, dev), ts, wrapped)
    assert h.runs == r0 + 1
    _eq(_np(a), _np(b), "smoother: fused against host loop")
    _eq(_np(a), oracle.backward_smoother_lg(om, key, filt, vs), "smoother against oracle")

    key, vs, uss, lws = _sampling_inputs(oracle, om, n, 0)
    h = br.backsim_handle(n, "sampling")
    r0 = h.runs
    xa, Ba = backward_sampling_pass(key, br.transition_logpdf, _t(vs, dev), ts, _t(uss, dev), _t(lws, dev))
    assert h.runs == r0 + 1
    xb, Bb = backward_sampling_pass(key, wrapped, _t(vs, dev), ts, _t(uss, dev), _t(lws, dev))
    assert h.runs == r0 + 1
    _eq(_np(xa), _np(xb), "sampling xs: fused against host loop")
    _eq(_np(Ba), _np(Bb), "sampling Bs: fused against host loop")
    assert Ba.dtype == Bb.dtype and xa.shape == xb.shape


def test_schrodinger_bridge_closure_dispatches(oracle, dev):
    import fbs_amd
    from fbs_amd.samplers import smc
    d, T, n = 2, 7, 300
    m0, c0, m1, c1 = sb_problem(d, 0)
    ts = np.linspace(0.0, 1.0, T + 1)
    br = fbs_amd.GaussianSBBridge(m0, c0, m1, c1, ts, du=d, sig=1.0, nsub=4, device=dev)
    om = oracle_model_from(oracle, br)
    rng = np.random.default_rng(3)
    vs = rng.normal(size=(T + 1, d)).astype(np.float32)
    init = rng.normal(size=(n, d)).astype(np.float32)
    filt, _ = oracle.bootstrap_filter_lg(om, oracle.PRNGKey(8), vs, init, "stratified", return_last=False)
    key = oracle.PRNGKey(9)
    h = br.backsim_handle(n, "smoother")
    r0 = h.runs
    traj = smc.bootstrap_backward_smoother(key, _t(filt, dev), _t(vs, dev), ts, br.transition_logpdf)
    assert h.runs == r0 + 1
    _eq(_np(traj), oracle.backward_smoother_lg(om, key, filt, vs), "SB smoother trajectory")


def test_gibbs_init_smoother_equals_oracle_composition(oracle, dev):
    from fbs_amd.samplers import gibbs_init
    T, n = 25, 300
    toy, ts, br = _setup(toy_2d, T, dev, Tend=2.0)
    om = oracle_model_from(oracle, br)
    key = oracle.PRNGKey(31)
    y0 = torch.from_numpy(toy["y0"]).to(dev)
    h = br.backsim_handle(n, "smoother")
    r0 = h.runs
    x0s, us_s = gibbs_init(key, y0, (1,), ts, br.fwd_sampler, br.sde, br.unpack, br.transition_sampler,
                           br.transition_logpdf, br.likelihood_logpdf, n, method='smoother', marg_y=False)
    assert h.runs == r0 + 1
    k_fwd, k_bridge, k_u0, k_bf, k_fwd2, k_bwd = oracle.split(key, 6)
    path = oracle.lg_fwd_sampler(om, k_fwd, np.array([0.0, toy["y0"][0]], np.float32))
    vs = path[::-1, 1:].copy()
    init = oracle.normal(k_u0, (n, 1))
    filt, _ = oracle.bootstrap_filter_lg(om, k_bf, vs, init, "stratified", return_last=False)
    _eq(_np(x0s), filt[-1, 0], "smoother x0")
    _eq(_np(us_s), oracle.backward_smoother_lg(om, k_bwd, filt, vs), "smoother us_star")


@pytest.mark.parametrize("n", [100, 513])
@pytest.mark.parametrize("mode", ["smoother", "sampling"])
def test_graph_replay_equals_fresh_handles(mode, n, oracle, dev):
    from fbs_amd.linear_gaussian import LGBacksim
    T = 20
    toy, ts, br = _setup(toy_4d, T, dev)
    om = oracle_model_from(oracle, br)
    if mode == "smoother":
        ins = [_smoother_inputs(oracle, om, toy, n, c) for c in range(2)]
    else:
        ins = [_sampling_inputs(oracle, om, n, c) for c in range(2)]
    run = lambda h, i: h.run(i[0], _t(i[1], dev), *(_t(a, dev) for a in i[2:]))
    flat = lambda o: [_np(x) for x in (o if isinstance(o, tuple) else (o,))]
    h = LGBacksim(br, n, mode)
    replayed = [flat(run(h, i)) for i in ins]                       # the second run replays the captured graph
    fresh = [flat(run(LGBacksim(br, n, mode), i)) for i in ins]
    for r, f in zip(replayed, fresh):
        for a, b in zip(r, f):
            _eq(a, b, "graph replay against a fresh handle")
    assert h.runs == 2
