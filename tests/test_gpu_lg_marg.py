"""GPU: gibbs_kernel(marg_y=True) on the fused sweep engine (fbsmi_lg_sweep_set_bridge) -- the dispatch from the
reference's signature, the Doob-bridge kernels alone through the handle's views, whole sweeps and chains against the numpy
restatement (tests/marg_restate.py), and the example driver's --marg.  Every comparison is of bit patterns."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import oracle_model_from, toy_2d, toy_4d, toy_gp
from marg_restate import bridge_tables_by_hand, bridge_vs, gibbs_chain_marg, gibbs_kernel_marg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _eq(got, want, what):
    got, want = np.ascontiguousarray(_np(got)), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == np.bool_ or want.dtype == np.bool_:
        np.testing.assert_array_equal(got.astype(bool), want.astype(bool), err_msg=what)
    else:
        np.testing.assert_array_equal(got.view(np.uint8), want.astype(got.dtype).view(np.uint8), err_msg=what)


def _sde(which):
    from fbs_amd.sdes import StationaryConstLinearSDE, StationaryLinLinearSDE
    return StationaryConstLinearSDE(-0.5, 1.0) if which == "const" else StationaryLinLinearSDE(0.02, 4.0, 0.0, 1.0)


def _bridge(toy, T, dev, sde="const"):
    import fbs_amd
    ts = np.linspace(0.0, 1.0, T + 1)
    return fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], _sde(sde), ts, toy["du"], device=dev), ts


def _toy(du, dv, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(du + dv, du + dv))
    return dict(m0=rng.normal(size=du + dv), cov0=A @ A.T / (du + dv) + 0.5 * np.eye(du + dv),
                y0=rng.normal(size=dv).astype(np.float32), du=du)


def _check_sweep(oracle, br, om, tab, sweep, key, x0, y0, bs, N, eb, ef, use_graph=True, what=""):
    got = sweep.sweep(key, x0, y0, bs, use_graph=use_graph)
    v = sweep.views()
    want = gibbs_kernel_marg(oracle, om, tab, key, x0, y0, bs, N, eb, ef)
    for name in ("vs", "us_star", "us_T", "lw_T"):
        _eq(v[name], want[4][name], what + name)
    for i, name in enumerate(("x0_next", "us_star_next", "bs_next", "acc")):
        _eq(got[i], want[i], what + name)


# ---- 1. dispatch ----------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def test_dispatch_takes_the_fused_engine(oracle, dev, monkeypatch):
    """With a LinearGaussianBridge's own closures, grid and SDE, gibbs_kernel(marg_y=True) never reaches the closure tier's
    bridge_sampler and equals the oracle; a foreign SDE or a wrapped closure still takes the closure tier."""
    import fbs_amd.samplers.gibbs as G
    from fbs_amd.sdes import StationaryConstLinearSDE

    def raiser(*a, **k):
        raise _Reached()

    monkeypatch.setattr(G, "bridge_sampler", raiser)
    toy, n, T = toy_4d(), 64, 9
    br, ts = _bridge(toy, T, dev)
    om = oracle_model_from(oracle, br)
    t64 = bridge_tables_by_hand(br.sde, ts, 100)
    bridge = lambda key_, y_first, y_last: oracle.doob_bridge_np(key_, t64["A"], t64["B"], t64["S"], t64["ddt"], y_first,
                                                                 y_last, T, 100, True)
    rng = np.random.default_rng(8)
    x0 = rng.normal(size=br.du).astype(np.float32)
    bs = rng.integers(0, n, T + 1).astype(np.int32)
    key = oracle.PRNGKey(2)
    x0t, y0t = torch.from_numpy(x0).to(dev), torch.from_numpy(toy["y0"]).to(dev)
    call = lambda fwd, sde: G.gibbs_kernel(key, x0t, y0t, None, bs, ts, fwd, sde, br.unpack, n, br.transition_sampler,
                                           br.transition_logpdf, br.likelihood_logpdf, marg_y=True)
    got = call(br.fwd_sampler, br.sde)
    want = oracle.gibbs_kernel_lg_marg_y(om, key, x0, toy["y0"], bs, n, bridge)
    for a, b, w in zip(got, want, ("x0", "us_star", "bs_star", "acc")):
        _eq(a, b, w)
    _eq(call(br.fwd_sampler, StationaryConstLinearSDE(-0.5, 1.0))[0], want[0], "an equal SDE object")
    with pytest.raises(_Reached):
        call(br.fwd_sampler, StationaryConstLinearSDE(-0.4, 1.0))
    with pytest.raises(_Reached):
        call(br.fwd_sampler, None)
    with pytest.raises(_Reached):
        call(lambda *a, **k: br.fwd_sampler(*a, **k), br.sde)


def test_set_bridge_refuses_an_em_forward_handle(dev):
    import fbs_amd
    from fbs_amd import _lib
    from sb_restate import sb_problem
    m0, c0, m1, c1 = sb_problem(3, 0)
    T = 4
    sb = fbs_amd.GaussianSBBridge(m0, c0, m1, c1, np.linspace(0.0, 1.0, T + 1), du=3, sig=1.0, nsub=2, device=dev)
    h = sb.sweep_handle(16, True, False)
    z = torch.zeros(T * 2, device=dev)
    st = _lib.DoobBridgeStruct(2, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr())
    with pytest.raises(NotImplementedError):
        _lib.call("fbsmi_lg_sweep_set_bridge", h.h, ctypes.byref(st))
    with pytest.raises(NotImplementedError):
        sb.sweep_handle(16, True, False, marg_y=True)


# ---- 2. the bridge kernels alone --------------------------------------------------------------------
@pytest.mark.parametrize("sde", ["const", "lin"])
@pytest.mark.parametrize("du,dv,nsub,T", [(1, 1, 1, 1), (2, 3, 3, 5), (1, 1, 7, 17), (2, 5, 100, 17), (1, 128, 100, 3)])
def test_bridge_path_equals_oracle(oracle, dev, du, dv, nsub, T, sde):
    """views()["vs"] against reverse(doob_bridge_np) from the forward path's end points, us_star untouched; the tables
    are set directly, so nsub * dv is odd in three of the cases; C = 1 and C = 3 chains in one handle."""
    from fbs_amd import _lib
    from fbs_amd.linear_gaussian import LGSweep
    toy = _toy(du, dv, 10 * dv + nsub)
    br, ts = _bridge(toy, T, dev, sde)
    om = oracle_model_from(oracle, br)
    st = br.bridge_tables(nsub)
    N = 8
    for Cn in (1, 3):
        h = LGSweep(br, N, True, False, False, Cn)
        assert not h.children
        _lib.call("fbsmi_lg_sweep_set_bridge", h.h, ctypes.byref(st))
        rng = np.random.default_rng(Cn)
        x0 = rng.normal(size=(Cn, du)).astype(np.float32)
        bs = rng.integers(0, N, (Cn, T + 1)).astype(np.int32)
        keys = oracle.split(oracle.PRNGKey(40 + T), Cn)
        h.sweep(keys if Cn > 1 else keys[0], x0 if Cn > 1 else x0[0], toy["y0"], bs if Cn > 1 else bs[0])
        v = h.views()
        for c in range(Cn):
            key_fwd, _, key_bridge = oracle.split(keys[c], 3)
            path = oracle.lg_fwd_sampler(om, key_fwd, np.concatenate([x0[c], toy["y0"]]))
            want = bridge_vs(oracle, st._host, key_bridge, path[0, du:], path[-1, du:])
            _eq(v["vs"][c] if Cn > 1 else v["vs"], want, f"C={Cn} chain {c} vs")
            _eq(v["us_star"][c] if Cn > 1 else v["us_star"], path[::-1, :du], f"C={Cn} chain {c} us_star")
        with pytest.raises(RuntimeError):      # once per handle, before its first sweep
            _lib.call("fbsmi_lg_sweep_set_bridge", h.h, ctypes.byref(st))


# ---- 3. whole sweeps ---------------------------------------------------------------------------------
_SWEEPS = [(toy_2d, 20, 12, True, False), (toy_2d, 513, 5, True, False), (toy_2d, 1024, 5, True, False)] + \
          [(toy_4d, 64, 9, eb, ef) for eb in (True, False) for ef in (False, True)] + \
          [(lambda: toy_gp(24), 100, 6, True, False), (lambda: toy_gp(24), 300, 6, True, False)]


@pytest.mark.parametrize("toy,N,T,eb,ef", _SWEEPS)
def test_fused_marg_sweep_bit_exact(oracle, dev, toy, N, T, eb, ef):
    toy = toy()
    br, ts = _bridge(toy, T, dev)
    om = oracle_model_from(oracle, br)
    rng = np.random.default_rng(N + T)
    x0 = rng.normal(size=br.du).astype(np.float32)
    bs = rng.integers(0, N, T + 1).astype(np.int32)
    sweep = br.sweep_handle(N, eb, ef, marg_y=True)
    assert sweep is not br.sweep_handle(N, eb, ef)          # marg_y is part of the cache key
    _check_sweep(oracle, br, om, br.bridge_tables(100)._host, sweep, oracle.PRNGKey(7 + N), x0, toy["y0"], bs, N, eb, ef)


def test_graph_replay_with_new_inputs(oracle, dev):
    toy, N, T = toy_4d(), 64, 9
    br, ts = _bridge(toy, T, dev, "lin")
    om = oracle_model_from(oracle, br)
    tab = br.bridge_tables(100)._host
    sweep = br.sweep_handle(N, True, False, marg_y=True)
    rng = np.random.default_rng(3)
    for i, use_graph in enumerate((False, True, True)):
        x0 = rng.normal(size=br.du).astype(np.float32)
        y0 = rng.normal(size=br.dv).astype(np.float32)
        bs = rng.integers(0, N, T + 1).astype(np.int32)
        _check_sweep(oracle, br, om, tab, sweep, oracle.PRNGKey(20 + i), x0, y0, bs, N, True, False, use_graph,
                     f"sweep {i} (use_graph={use_graph}) ")


# ---- 4. chains -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 4])
def test_chain_key_schedule(oracle, dev, Cn):
    toy, N, T, nsweeps = toy_4d(), 32, 6, 3
    br, ts = _bridge(toy, T, dev)
    om = oracle_model_from(oracle, br)
    rng = np.random.default_rng(Cn)
    x0 = rng.normal(size=(Cn, br.du)).astype(np.float32)
    bs = rng.integers(0, N, (Cn, T + 1)).astype(np.int32)
    key = oracle.PRNGKey(11)
    sweep = br.sweep_handle(N, True, False, nchains=Cn, marg_y=True)
    assert len(sweep.children) == (2 if Cn == 4 else 0)
    assert all(ch.marg_y for ch in sweep.children)
    k_out, x_out, bs_out, x0s = sweep.chain(key, x0 if Cn > 1 else x0[0], toy["y0"], bs if Cn > 1 else bs[0], nsweeps)
    wk, wx, wbs, wout = gibbs_chain_marg(oracle, om, br.bridge_tables(100)._host, key, x0, toy["y0"], bs, N, nsweeps)
    _eq(x0s, wout if Cn > 1 else wout[:, 0], "x0s")
    _eq(x_out, wx if Cn > 1 else wx[0], "x0")
    _eq(bs_out, wbs if Cn > 1 else wbs[0], "bs_star")
    np.testing.assert_array_equal(np.asarray(k_out, np.uint32), np.asarray(wk, np.uint32))


# ---- 6. the example driver -----------------------------------------------------------------------------
def test_example_driver_marg(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "toy_gibbs.py"), "--marg", "--d", "2",
                          "--nparticles", "16", "--nsamples", "3", "--nchains", "2", "--outdir", str(tmp_path)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    f = np.load(os.path.join(str(tmp_path), "gibbs-marg-const-16-666.npz"))
    assert f["samples"].shape == (2, 3, 2) and np.isfinite(f["samples"]).all()
