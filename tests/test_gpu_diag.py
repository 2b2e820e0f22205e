"""GPU: the opt-in per-step diagnostics of the fused engines (fbsmi_lg_sweep_set_diagnostics, fbsmi_lg_filter_set_diagnostics)
against tests/diag_restate.py, which rebuilds every (lse, ess) row from oracle pieces (proven on the CPU by
tests/test_diag_restate.py).  Every comparison is of uint32 views: the device computes the same two-level logsumexp and the
same summation tree as the oracle.  Each case also runs the same arguments on a handle without diagnostics and demands
bit-identical outputs (switching them on changes nothing but the extra launches).

One case per branch of the launch lists: the regime each case reaches is named beside it (the sizes follow enqueue_sweep /
enqueue_filter in fbs_amd/csrc/fbsmi_lg.hip)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import degenerate as D
import diag_restate as R
from helpers import oracle_model_from, toy_2d, toy_31, toy_4d, toy_gp

pytestmark = pytest.mark.gpu
f32 = np.float32
TOYS = {"2d": toy_2d, "4d": toy_4d, "31": toy_31, "gp24": lambda: toy_gp(24), "gp100": lambda: toy_gp(100),
        "gp99": lambda: toy_gp(99)}


def _np(t):
    return t.detach().cpu().numpy()


def _eq(got, want, what):
    got, want = np.ascontiguousarray(_np(got) if isinstance(got, torch.Tensor) else got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    bad = np.flatnonzero(g.ravel() != w.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: {got.ravel()[bad[:5]]} vs {want.ravel()[bad[:5]]}"


def _bridge(toy, T, dev, Tend=1.0):
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    return fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(a=-0.5, b=1.),
                                        np.linspace(0, Tend, T + 1), toy["du"], device=dev)


def _sweep_pair(br, N, eb, ef, C, marg=False):
    return (br.sweep_handle(N, eb, ef, nchains=C, marg_y=marg, diagnostics=True),
            br.sweep_handle(N, eb, ef, nchains=C, marg_y=marg))


def _sweep_case(O, dev, toy, N, T, C=1, eb=True, ef=False, Tend=1.0, rows=None, marg=False, br=None, y0=None):
    """One sweep of C chains with diagnostics on and off: outputs bit-identical, rows = the restatement's.
    rows(c, key, x0, bs) -> (lse, ess) replaces R.sweep_rows for the sweeps whose paths the oracle does not draw."""
    toy = TOYS[toy]() if isinstance(toy, str) else toy
    br = _bridge(toy, T, dev, Tend) if br is None else br
    y0 = toy["y0"] if y0 is None else y0
    om = oracle_model_from(O, br)
    rng = np.random.default_rng(N + T + C)
    x0 = rng.normal(size=(C, br.du)).astype(f32)
    bs = rng.integers(0, N, (C, T + 1)).astype(np.int32)
    keys = O.split(O.PRNGKey(13), max(C, 2))[:C]
    on, off = _sweep_pair(br, N, eb, ef, C, marg)
    sq = (lambda a: a) if C > 1 else (lambda a: a[0])
    got = on.sweep(sq(keys), sq(x0), y0, sq(bs))
    dg, views = on.diagnostics(), on.views()
    base = off.sweep(sq(keys), sq(x0), y0, sq(bs))
    torch.cuda.synchronize()
    for a, b, what in zip(got, base, ("x0_next", "us_star_next", "bs_next", "acc")):
        _eq(a, _np(b), f"{what}: diagnostics on against off")
    assert "diag" not in off.views()
    _eq(views["diag"][..., 0], _np(dg["lse"]), "views()['diag'] lse column")
    _eq(views["diag"][..., 1], _np(dg["ess"]), "views()['diag'] ess column")
    n = N + int(ef)
    for c in range(C):
        lse, ess = rows(c, keys[c], x0[c], bs[c]) if rows else R.sweep_rows(O, om, keys[c], x0[c], y0, bs[c], N, eb, ef)
        glse, gess = (_np(dg[k])[c] if C > 1 else _np(dg[k]) for k in ("lse", "ess"))
        print(f"N={N} C={C} chain {c}: ess min {ess.min():.6g} max {ess.max():.6g} of {n}; sum lse {lse.sum():.6g}")
        _eq(glse, lse, f"lse rows, chain {c}")
        _eq(gess, ess, f"ess rows, chain {c}")
    br._sweeps.clear()
    return dg


# (id, toy, N, T, C, eb, ef, environment, the step kernels the launch list reaches)
SWEEPS = [
    ("one-tile-1", "2d", 1, 5, 1, True, False, {}, "k_lg_step1 (the step-wise route of one narrow tile)"),
    ("one-tile-10", "4d", 10, 8, 1, True, False, {}, "k_lg_step1"),
    ("one-tile-10-stored", "2d", 10, 6, 1, False, False, {}, "k_lg_step1, stored path + backward scanning"),
    ("one-tile-256", "31", 256, 4, 3, True, False, {}, "k_lg_step1, full tile, three chains"),
    ("one-tile-255-ef", "4d", 255, 4, 1, True, True, {}, "k_lg_step1, 256 slots, init likelihood in row 0"),
    ("general-257", "2d", 257, 4, 1, True, False, {}, "k_lg_prop1, two tiles, one slot in the second"),
    ("general-256-ef", "4d", 256, 4, 1, True, True, {}, "k_lg_prop1, 2^8 + 1 slots (too few tiles for the tree step)"),
    ("plus1-512-ef", "2d", 512, 4, 1, True, True, {}, "k_lg_prop1t, 2^9 + 1 slots: the tree of 512 + a one-slot tile"),
    ("tree-512", "4d", 512, 5, 1, True, False, {}, "k_lg_norm<1,0,true> + k_lg_prop1t (pinned)"),
    ("tree-512-stored", "2d", 512, 4, 1, False, False, {}, "k_lg_prop1t, stored path"),
    ("tree-512-c4-groups", "2d", 512, 3, 4, True, False, {}, "k_lg_prop1t, four chains as two handles"),
    ("tree-512-c4-halfwave", "2d", 512, 3, 4, True, False, {"FBSMI_CHAIN_GROUPS": "1", "FBSMI_TREE_HALVES": "2"},
     "k_lg_prop1th<., 2>, four chains in one handle"),
    ("tree-512-c4-pairs", "2d", 512, 3, 2, True, False, {"FBSMI_TREE_HALVES": "2", "FBSMI_PROP_HALFWAVE": "0"},
     "k_lg_prop1tp<., 2>"),
    ("tree-1024-c2", "31", 1024, 3, 2, True, False, {}, "k_lg_prop1t, four tiles"),
    ("general-777", "31", 777, 4, 1, True, False, {}, "k_lg_norm + k_lg_cdf + k_lg_prop1, ragged last tile"),
    ("prop2t-65536-c5", "2d", 65536, 2, 5, True, False, {"FBSMI_CHAIN_GROUPS": "1"},
     "k_lg_prop2t: 256 tiles x 5 chains = 1280 workgroups of the one-slot kernels"),
    ("prop2-81920-c4", "2d", 81920, 2, 4, True, False, {"FBSMI_CHAIN_GROUPS": "1"},
     "k_lg_prop2: 320 tiles x 4 chains = 1280, not a power of two"),
    ("propQ4-200000", "2d", 200000, 2, 1, True, False, {}, "k_lg_heaps + k_lg_propQ<4>, tiles of 1024, k_lg_diag<4>"),
    ("wide-one-tile-100", "gp24", 100, 4, 1, True, False, {}, "k_lgw_gemm<1>: rows from the per-row terms"),
    ("wide-one-tile-100-ef", "gp24", 100, 3, 1, True, True, {}, "k_lgw_gemm<1>, row 0 from the init product's terms"),
    ("wide-one-tile-100-stored-c2", "gp24", 100, 3, 2, False, False, {}, "k_lgw_gemm<1> unpinned, stored path"),
    ("wide-tiled-300", "gp24", 300, 4, 1, True, False, {}, "k_lgw_anc + k_lgw_gemm<0> + k_lgw_lse"),
    ("wide-tiled-300-ef", "gp24", 300, 3, 1, True, True, {}, "the same, row 0 by k_lgw_gemm<3> + k_lgw_lse"),
    ("wide-fat-3201-rowsum", "gp100", 3201, 2, 1, True, False, {}, "k_lgw_gemm_fat<true> + k_lg_lwpart: 101 x 7 = 707 > 700"),
    ("wide-fat-3201-odd", "gp99", 3201, 2, 1, True, False, {}, "k_lgw_gemm_fat<false> + k_lgw_lse (D = 198)"),
]


@pytest.mark.parametrize("case", SWEEPS, ids=[c[0] for c in SWEEPS])
def test_sweep_rows_match_the_restatement(case, oracle, dev, monkeypatch):
    _, toy, N, T, C, eb, ef, env, _ = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _sweep_case(oracle, dev, toy, N, T, C, eb, ef)


def test_sweep_rows_three_launch_step_on_a_power_of_two():
    """N = 512 with FBSMI_TREE_STEP=0 (k_lg_norm + k_lg_cdf + k_lg_prop1 where the tree step is the rule), the switch set in a
    fresh child process."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import torch, oracle as O, test_gpu_diag as t\n"
            "O.lib(); t._sweep_case(O, torch.device('cuda:0'), '2d', 512, 4); print('child-ok')\n") % (here, os.path.dirname(here))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FBSMI_TREE_STEP="0"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "child-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_marg_y_sweep_rows(oracle, dev):
    """marg_y=True: vs is the Doob bridge's path (fbsmi_lg_sweep_set_bridge); the rows are of the pass on that path."""
    from marg_restate import gibbs_kernel_marg
    toy, N, T = toy_4d(), 300, 4
    br = _bridge(toy, T, dev)
    om = oracle_model_from(oracle, br)
    tab = br.bridge_tables(100)._host

    def rows(c, key, x0, bs):
        v = gibbs_kernel_marg(oracle, om, tab, key, x0, toy["y0"], bs, N)[4]
        return R.sweep_rows_on(oracle, om, oracle.split(oracle.split(key, 3)[1], 4)[0], v["us_star"], v["vs"], bs, N)

    _sweep_case(oracle, dev, toy, N, T, rows=rows, marg=True, br=br)


def test_schrodinger_bridge_sweep_rows(oracle, dev):
    """GaussianSBBridge: the paths come from the Euler-Maruyama forward process (fbsmi_lg_sweep_set_em_forward)."""
    import fbs_amd
    from sb_restate import gibbs_kernel_sb, sb_problem
    d, N, T, nsub = 3, 100, 5, 3
    m0, c0, m1, c1 = sb_problem(d, d)
    br = fbs_amd.GaussianSBBridge(m0, c0, m1, c1, np.linspace(0.0, 1.0, T + 1), du=d, sig=1.0, nsub=nsub, device=dev)
    om = oracle_model_from(oracle, br)
    h = br.em_host
    em = (h["M"], h["c"], h["ddt"], h["s"], br.nsub)
    y0 = np.random.default_rng(3).normal(size=d).astype(f32)

    def rows(c, key, x0, bs):
        v = gibbs_kernel_sb(oracle, om, em, key, x0, y0, bs, N, True, False)[4]
        return R.sweep_rows_on(oracle, om, oracle.split(oracle.split(key, 3)[1], 4)[0], v["us_star"], v["vs"], bs, N)

    _sweep_case(oracle, dev, dict(du=d), N, T, rows=rows, br=br, y0=y0)


def test_chain_leaves_the_last_sweeps_rows(oracle, dev):
    """fbsmi_lg_gibbs_chain with diagnostics: after three sweeps the buffer holds the third sweep's rows; the chain's own
    outputs are those of a handle without diagnostics."""
    toy, N, T = toy_2d(), 300, 5
    br = _bridge(toy, T, dev)
    om = oracle_model_from(oracle, br)
    x0, bs = D.sweep_inputs(toy, N, T)
    key = oracle.PRNGKey(77)
    on, off = _sweep_pair(br, N, True, False, 1)
    got = on.chain(key, x0, toy["y0"], bs, 3)
    dg = on.diagnostics()
    base = off.chain(key, x0, toy["y0"], bs, 3)
    for a, b, what in zip(got, base, ("key", "x0", "bs_star", "x0s")):
        _eq(a, _np(b) if isinstance(b, torch.Tensor) else b, what)
    k2, x2, b2, _ = oracle.gibbs_chain_lg(om, key, x0, toy["y0"], bs, N, 2)
    lse, ess = R.sweep_rows(oracle, om, oracle.split(k2, 2)[1], x2, toy["y0"], b2, N)
    _eq(dg["lse"], lse, "lse rows of the third sweep")
    _eq(dg["ess"], ess, "ess rows of the third sweep")


@pytest.mark.parametrize("case", [D.NARROW[0], D.NARROW[3]], ids=lambda c: c[0])
def test_collapsed_narrow_sweep_rows(case, oracle, dev):
    """Collapsed ensembles of tests/degenerate.py (ESS exactly 1.0 on some steps, weights exactly zero): rows bit-equal."""
    _, name, N, T, Tend, eb, ef, _, _ = case
    dg = _sweep_case(oracle, dev, D.named_toy(name), N, T, 1, eb, ef, Tend)
    ess = _np(dg["ess"])
    assert np.any(ess == 1.0) and np.any(ess < 2), ess


@pytest.mark.parametrize("case", [D.WIDE[0], D.WIDE[1]], ids=lambda c: c[0])
def test_collapsed_wide_sweep_rows(case, oracle, dev):
    _, du, dv, N, C, T, Tend, _ = case
    dg = _sweep_case(oracle, dev, D.collapse_gp(du, dv, **D.GP), N, T, C, True, False, Tend)
    assert np.any(_np(dg["ess"]) < 2)


# ---- filters ---------------------------------------------------------------------------------------------------------------
# (toy, n, chains, the launch list of enqueue_filter)
FILTERS = [
    ("2d", 10, 3, "filter_narrow_one_launch (k_filt_sweep1<., DiagDev>)"),
    ("4d", 256, 1, "filter_narrow_one_launch, full tile"),
    ("2d", 512, 3, "filter_narrow_tree (k_filt_norm<1, true> + k_filt_prop1t)"),
    ("31", 777, 1, "filter_narrow_general"),
    ("gp24", 100, 3, "filter_wide_one_tile"),
    ("gp24", 300, 1, "filter_wide_tiles"),
]
FILTER_T = 5


@pytest.mark.parametrize("resampling", ["stratified", "systematic"])
@pytest.mark.parametrize("flow", ["bootstrap", "pmcmc"])
@pytest.mark.parametrize("case", FILTERS, ids=[f"{c[0]}-{c[1]}-c{c[2]}" for c in FILTERS])
def test_filter_rows_match_the_restatement(case, flow, resampling, oracle, dev):
    name, n, C, _ = case
    _filter_case(oracle, dev, TOYS[name](), n, C, flow, resampling, FILTER_T)


def _filter_case(O, dev, toy, n, C, flow, resampling, T):
    br = _bridge(toy, T, dev)
    om = oracle_model_from(O, br)
    keys, vs, init = (a[:C] for a in D.filter_inputs(O, om, toy["y0"], n, nchains=max(C, 2)))
    sq = (lambda a: a) if C > 1 else (lambda a: a[0])
    on = br.filter_handle(n, flow, resampling, nchains=C, diagnostics=True)
    off = br.filter_handle(n, flow, resampling, nchains=C)
    uT, ell = on.run(sq(keys), sq(vs), sq(init))
    dg = on.diagnostics()
    uT0, ell0 = off.run(sq(keys), sq(vs), sq(init))
    torch.cuda.synchronize()
    _eq(uT, _np(uT0), "uT: diagnostics on against off")
    _eq(ell, _np(ell0), "loglik: diagnostics on against off")
    with pytest.raises(RuntimeError, match="no diagnostics"):
        off.diagnostics()
    glse, gess, gell = (_np(t).reshape(C, -1) for t in (dg["lse"], dg["ess"], ell.reshape(C)))
    worst = np.inf
    for c in range(C):
        if flow == "bootstrap":
            lws, nell = R.bootstrap_lws(O, om, keys[c], vs[c], init[c], resampling)
            _eq(gell[c], np.array([nell], f32), f"negative log-likelihood, chain {c}")
            # the returned estimate, re-derived from the device's own lse column in the oracle's order
            _eq(gell[c], np.array([R.nell_from_lse(glse[c], n)], f32), f"loglik from the lse column, chain {c}")
        else:
            lws, wuT, wl = R.pmcmc_restated(O, om, keys[c], vs[c], init[c], resampling)
            _eq(_np(uT).reshape(C, n, -1)[c], wuT, f"uT, chain {c}")
            _eq(gell[c], np.array([wl], f32), f"log_ell, chain {c}")
        lse, ess = R.rows_of(O, lws)
        worst = min(worst, float(ess.min()))
        _eq(glse[c], lse, f"lse rows, chain {c}")
        _eq(gess[c], ess, f"ess rows, chain {c}")
    print(f"{flow} {resampling} n={n} C={C}: min ESS {worst:.6g} of {n}")
    br._sweeps.clear()
    return gess


@pytest.mark.parametrize("name,n", [("2d", 64), ("gp20", 200)])
def test_collapsed_filter_rows(name, n, oracle, dev):
    """Collapsed filter inputs of tests/degenerate.py, one narrow and one wide, both flows."""
    for flow in ("bootstrap", "pmcmc"):
        ess = _filter_case(oracle, dev, D.named_toy(name), n, 3, flow, "stratified", D.FILTER_T)
        assert np.any(ess < 2), ess


# ---- the switch ------------------------------------------------------------------------------------------------------------
def test_handles_without_diagnostics_refuse_and_late_switches_are_refused(oracle, dev):
    from fbs_amd import _lib
    toy, N, T = toy_2d(), 300, 3
    br = _bridge(toy, T, dev)
    x0, bs = D.sweep_inputs(toy, N, T)
    off = br.sweep_handle(N, True, False)
    with pytest.raises(RuntimeError, match="no diagnostics"):     # before any sweep: nothing to launch, nothing to copy
        off._diag_rows()
    off.sweep(oracle.PRNGKey(1), x0, toy["y0"], bs)
    with pytest.raises(RuntimeError, match="no diagnostics"):
        off._diag_rows()
    with pytest.raises(RuntimeError, match="before the handle's first run"):
        _lib.call("fbsmi_lg_sweep_set_diagnostics", off.h, 1)
    assert "diag" not in off.views()
    on = br.sweep_handle(N, True, False, diagnostics=True)
    assert on is not off and on is br.sweep_handle(N, True, False, diagnostics=True)   # the flag is part of the cache key
    filt = br.filter_handle(N, "bootstrap")
    assert filt is not br.filter_handle(N, "bootstrap", diagnostics=True)
    with pytest.raises(RuntimeError, match="no diagnostics"):
        filt.diagnostics()
