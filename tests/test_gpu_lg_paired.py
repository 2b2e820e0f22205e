"""k_lg_prop1t<., 2 | 4>: workgroups that own tiles N/2 apart (one Threefry call per pair of slots and draw, the killed
slots' redraw searches dealt out from an LDS queue).  Every case is compared bit for bit with the CPU oracle
(``gibbs_kernel_lg(..., debug=True)``: the four outputs, the final particles and log-weights) and with a handle of
one-tile workgroups (FBSMI_TREE_HALVES=1) on the same inputs.
"""
import numpy as np
import pytest

from helpers import toy_2d, toy_4d, toy_31, toy_gp, oracle_model_from

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _bridge(toy, ts, dev):
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    return fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(a=-0.5, b=1.), ts, toy["du"], device=dev)


def _eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    if a.dtype == np.float32:
        bad = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
    else:
        bad = np.flatnonzero(a.ravel() != b.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {bad[:5]}: {a.ravel()[bad[:5]]} vs {b.ravel()[bad[:5]]}"


OUTPUTS = ("x0_next", "us_star_next", "bs_star_next", "acc")


def _sweep(toy, ts, dev, monkeypatch, halves, N, eb, C, keys, x0, y0, bs):
    """One sweep of a fresh handle created under FBSMI_TREE_HALVES=halves -> (outputs, views) as numpy arrays with a
    leading chain axis."""
    monkeypatch.setenv("FBSMI_TREE_HALVES", halves)
    br = _bridge(toy, ts, dev)     # a bridge of its own: handles are cached per bridge, the switch is read at creation
    h = br.sweep_handle(N, eb, False, nchains=C)
    sq = lambda a: a if C > 1 else a[0]
    got = h.sweep(sq(keys), sq(x0), y0, sq(bs), use_graph=False)
    views = h.views()
    lead = lambda t: _np(t).reshape((C,) + tuple(t.shape[(1 if C > 1 else 0):]))
    return br, [lead(g) for g in got], {k: lead(v) for k, v in views.items() if v is not None}


def _check(toy_, N, T, C, halves, oracle, dev, monkeypatch, bs=None, y0=None, eb=True, seed=0):
    ts = np.linspace(0, 1.0, T + 1)
    rng = np.random.default_rng(N + C + seed)
    du = toy_["du"]
    x0 = rng.normal(size=(C, du)).astype(np.float32)
    if bs is None:
        bs = rng.integers(0, N, (C, T + 1)).astype(np.int32)
    bs = np.asarray(bs, np.int32).reshape(C, T + 1)
    y0 = toy_["y0"] if y0 is None else np.asarray(y0, np.float32)
    keys = oracle.split(oracle.PRNGKey(31), max(C, 2))[:C]
    br, got, v = _sweep(toy_, ts, dev, monkeypatch, halves, N, eb, C, keys, x0, y0, bs)
    _, got1, v1 = _sweep(toy_, ts, dev, monkeypatch, "1", N, eb, C, keys, x0, y0, bs)
    om = oracle_model_from(oracle, br)
    for c in range(C):
        want = oracle.gibbs_kernel_lg(om, keys[c], x0[c], y0, bs[c], N, eb, False, debug=True)
        assert np.isfinite(want[5]).all()
        for i, what in enumerate(OUTPUTS):
            _eq(got[i][c], want[i], f"{what} chain {c}")
        _eq(v["us_T"][c], want[4], f"particles chain {c}")
        _eq(v["lw_T"][c], want[5], f"log-weights chain {c}")
    for i, what in enumerate(OUTPUTS):
        _eq(got[i], got1[i], f"{what} against one-tile workgroups")
    assert set(v) == set(v1)
    for name in v:
        _eq(v[name], v1[name], f"{name} against one-tile workgroups")
    return v


@pytest.mark.parametrize("first", [0, 1, 2, 3])
def test_one_workgroup_holds_the_ensemble_reference_on_tile_edges(first, oracle, dev, monkeypatch):
    """N = 512, one 512-thread workgroup holds both tiles (N/2 apart = adjacent here).  The reference indices run through
    0, 255, 256, 511 in turn (starting at each of them), so the pin and J_prob[i*] land on the tile edges either side of
    N/2 and the rotation j* - J wraps."""
    edge = [0, 255, 256, 511]
    T = 8
    bs = [edge[(first + k) % 4] for k in range(T + 1)]
    _check(toy_2d(), 512, T, 1, "2", oracle, dev, monkeypatch, bs=bs, seed=first)


def test_one_workgroup_per_chain_holds_two_pairs_of_tiles(oracle, dev, monkeypatch):
    """N = 1024, three chains, du = 2, 1024-thread workgroups: tiles (0, 1) and (2, 3), a chain index in every address."""
    _check(toy_4d(), 1024, 6, 3, "4", oracle, dev, monkeypatch)


@pytest.mark.parametrize("toy", [toy_31, lambda: toy_gp(16)], ids=["du3", "du16"])
def test_several_workgroups_per_chain_wider_states(toy, oracle, dev, monkeypatch):
    """N = 2048, two chains, four 512-thread workgroups per chain.  du = 3 (DMAX = 4) hands the partner's noise through LDS;
    du = 16 (DMAX = 16, the widest narrow model) is past that rule: every slot draws its own noise, and the ancestor's row
    is fetched after the search."""
    _check(toy(), 2048, 6, 2, "2", oracle, dev, monkeypatch)


@pytest.mark.parametrize("N", [512, 2048])
def test_queue_empty_and_nearly_full(N, oracle, dev, monkeypatch):
    """Both extremes of the queue of killed slots.  Step 0 of every sweep starts from uniform weights, where the kill test
    u * w_max >= w never holds: an empty queue.  For the other extreme the observation is y0 = 20 (the toy's marginal
    standard deviation of y is 0.7), chosen with the oracle: every log-weight stays finite (final log-weights within
    [-11.8, -3.5] at N = 512 and [-16.0, -4.1] at N = 2048), and the expected killed fraction mean(1 - w / w_max) of the
    oracle's final weights is 0.93 at N = 512 and 0.97 at N = 2048 (0.16 / 0.08 at the toy's own y0 = 0)."""
    _check(toy_2d(), N, 6, 1, "2", oracle, dev, monkeypatch, y0=[20.0])


def test_stored_path_ancestors_and_particles(oracle, dev, monkeypatch):
    """explicit_backward=False at N = 1024: the ancestor matrix As, the stored particles uss and log-weights of every step
    are compared with those of the one-tile workgroups, next to the oracle's outputs of the backward scan over them."""
    v = _check(toy_31(), 1024, 6, 2, "2", oracle, dev, monkeypatch, eb=False)
    assert {"As", "uss", "log_wss"} <= set(v)
