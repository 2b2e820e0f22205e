"""k_lg_prop1th with tree_build_roles (the default): J found by wave 0 alone out of its registers, four tree leaves per lane and
the nodes of the walk read by lane, the w side on the waves that used to wait, one workgroup barrier.  One sweep per case,
compared bit for bit -- the four outputs, the final particles and log-weights and every view -- with the CPU oracle
(``gibbs_kernel_lg(..., debug=True)``), with a handle created under FBSMI_J_WAVE=0 (tree_build_shared: J by four waves through
LDS heaps, the text this one replaces) and with one created under FBSMI_PROP_HALFWAVE=0 (k_lg_prop1tp).
The cases are the smallest shapes at which each part of the one-wave search can go wrong; tests/test_jwave_restate.py checks
the same algorithm on the CPU."""
import numpy as np
import pytest

import degenerate as D
from helpers import toy_2d, toy_4d, toy_31, toy_gp, oracle_model_from
from jwave_restate import K_BLOCK, oracle_forward, oracle_steps

pytestmark = pytest.mark.gpu

OUTPUTS = ("x0_next", "us_star_next", "bs_star_next", "acc")
# the handle under test, and the two it is compared with: (FBSMI_J_WAVE, FBSMI_PROP_HALFWAVE)
DEFAULT, OTHERS = (None, "1"), {"FBSMI_J_WAVE=0": ("0", "1"), "FBSMI_PROP_HALFWAVE=0": (None, "0")}


def _np(t):
    return t.detach().cpu().numpy()


def _bridge(toy, ts, dev):
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    return fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(a=-0.5, b=1.), ts, toy["du"], device=dev)


def _eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    x = a.view(np.uint32) if a.dtype == np.float32 else a
    y = b.view(np.uint32) if b.dtype == np.float32 else b
    bad = np.flatnonzero(x.ravel() != y.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {bad[:5]}: {a.ravel()[bad[:5]]} vs {b.ravel()[bad[:5]]}"


def _sweep(toy, ts, dev, monkeypatch, halves, switches, N, eb, C, keys, x0, y0, bs):
    """One sweep (no graph) of a fresh handle created under FBSMI_TREE_HALVES=halves and the two switches -> (bridge, outputs,
    views) as numpy arrays with a leading chain axis."""
    j_wave, halfwave = switches
    monkeypatch.setenv("FBSMI_TREE_HALVES", halves)
    monkeypatch.setenv("FBSMI_PROP_HALFWAVE", halfwave)
    if j_wave is None:
        monkeypatch.delenv("FBSMI_J_WAVE", raising=False)
    else:
        monkeypatch.setenv("FBSMI_J_WAVE", j_wave)
    br = _bridge(toy, ts, dev)     # a bridge of its own: handles are cached per bridge, the switches are read at creation
    h = br.sweep_handle(N, eb, False, nchains=C)
    sq = lambda a: a if C > 1 else a[0]
    got = h.sweep(sq(keys), sq(x0), y0, sq(bs), use_graph=False)
    views = h.views()
    lead = lambda t: _np(t).reshape((C,) + tuple(t.shape[(1 if C > 1 else 0):]))
    return br, [lead(g) for g in got], {k: lead(v) for k, v in views.items() if v is not None}


def _inputs(toy_, N, T, C, oracle, seed=0):
    rng = np.random.default_rng(N + C + seed)
    x0 = rng.normal(size=(C, toy_["du"])).astype(np.float32)
    bs = rng.integers(0, N, (C, T + 1)).astype(np.int32)
    keys = oracle.split(oracle.PRNGKey(31 + seed), max(C, 2))[:C]
    return x0, bs, keys


def _check(toy_, N, T, C, halves, oracle, dev, monkeypatch, bs=None, y0=None, eb=True, seed=0, Tend=1.0, x0=None, keys=None,
           finite=True):
    ts = np.linspace(0, Tend, T + 1)
    x0_rand, bs_rand, keys_rand = _inputs(toy_, N, T, C, oracle, seed)
    x0 = x0_rand if x0 is None else np.asarray(x0, np.float32).reshape(C, -1)
    keys = keys_rand if keys is None else np.asarray(keys, np.uint32).reshape(C, 2)
    bs = np.asarray(bs_rand if bs is None else bs, np.int32).reshape(C, T + 1)
    y0 = toy_["y0"] if y0 is None else np.asarray(y0, np.float32)
    br, got, v = _sweep(toy_, ts, dev, monkeypatch, halves, DEFAULT, N, eb, C, keys, x0, y0, bs)
    om = oracle_model_from(oracle, br)
    for c in range(C):
        want = oracle.gibbs_kernel_lg(om, keys[c], x0[c], y0, bs[c], N, eb, False, debug=True)
        assert not finite or np.isfinite(want[5]).all()
        for i, what in enumerate(OUTPUTS):
            _eq(got[i][c], want[i], f"{what} chain {c}")
        _eq(v["us_T"][c], want[4], f"particles chain {c}")
        _eq(v["lw_T"][c], want[5], f"log-weights chain {c}")
    for name, switches in OTHERS.items():
        _, got1, v1 = _sweep(toy_, ts, dev, monkeypatch, halves, switches, N, eb, C, keys, x0, y0, bs)
        for i, what in enumerate(OUTPUTS):
            _eq(got[i], got1[i], f"{what} against {name}")
        assert set(v) == set(v1)
        for view in v:
            _eq(v[view], v1[view], f"{view} against {name}")
    return v


@pytest.mark.parametrize("nb", [2, 4, 8, 32, 64, 128, 256])
def test_tile_leaves_in_one_lane_up_to_all_lanes(nb, oracle, dev, monkeypatch):
    """nb tiles, N = 256 nb: the leaves of the tree over the tiles sit in one lane (2, 4), two lanes, a quad-permute row of
    eight lanes (32), across the row mirrors and the 16- and 32-lane swaps, and in all 64 lanes (256); lanes behind the last
    tile hold zeros.  Two chains, so every per-chain buffer is read at an offset (of 8 bytes only for two tiles)."""
    _check(toy_2d(), nb * K_BLOCK, 3 if nb >= 128 else 4, 2, "2", oracle, dev, monkeypatch)


def test_four_tiles_per_workgroup(oracle, dev, monkeypatch):
    """k_lg_prop1th<., 4>: sixteen waves, the roles on waves 0-3, the noise on waves 8-15, waves 4-7 with nothing before the
    barrier.  N = 1024, three chains, du = 2."""
    _check(toy_4d(), 1024, 4, 3, "4", oracle, dev, monkeypatch)


# (N, seed): chosen on the CPU so that the oracle alone gives every landing below (see the test)
LANDINGS = [(512, 3), (2048, 3)]


def _edge_indices(N, T):
    edge = [0, 255, 256, N - 1, N // 2 + 77]
    return [edge[k % 5] for k in range(T + 1)]


def landings(steps, nb):
    """Where J of each step lands, as a set of names."""
    seen = set()
    for st in steps:
        J, i = st["J"], st["i_ref"]
        seen.add("J == i*" if J == i else ("tile of i*, not i*" if J // K_BLOCK == i // K_BLOCK else "another tile"))
        if J // K_BLOCK == 0:
            seen.add("tile 0")
        if J // K_BLOCK == nb - 1:
            seen.add("last tile")
    return seen


ALL_LANDINGS = {"J == i*", "tile of i*, not i*", "another tile", "tile 0", "last tile"}


@pytest.mark.parametrize("N,seed", LANDINGS)
def test_reference_index_on_edges_and_every_landing_of_J(N, seed, oracle, dev, monkeypatch):
    """The reference indices run over 0, 255, 256, N - 1 and an interior index: the tile of i* is the first and the last one,
    the patched leaf is in the first and the last lane and at the first and last of a lane's four leaves.  The J of every step
    is first derived from the oracle alone, and the steps of the two chains must between them have J == i*, J in the tile of
    i* but not i*, J in another tile, J in tile 0 and J in the last tile -- a condition on the inputs, met by the seed."""
    T, C, toy_ = 8, 2, toy_2d()
    bs = np.tile(np.asarray(_edge_indices(N, T), np.int32), (C, 1))
    x0, _, keys = _inputs(toy_, N, T, C, oracle, seed)
    om = oracle_model_from(oracle, D.cpu_bridge(toy_, T))
    steps = [st for c in range(C) for st in oracle_steps(oracle, om, keys[c], x0[c], toy_["y0"], bs[c], N)]
    assert landings(steps, N // K_BLOCK) == ALL_LANDINGS
    _check(toy_, N, T, C, "2", oracle, dev, monkeypatch, bs=bs, seed=seed)


def test_nearly_every_slot_killed(oracle, dev, monkeypatch):
    """y0 = 20 at N = 512 (test_gpu_lg_paired.py::test_queue_empty_and_nearly_full justifies the choice with the oracle: the
    log-weights stay finite, 0.93 of the final weights are killed): J_prob is nearly 1 / N everywhere and J_prob[i*] small."""
    _check(toy_2d(), 512, 6, 1, "2", oracle, dev, monkeypatch, y0=[20.0])


def test_collapsed_weights(oracle, dev, monkeypatch):
    """The prop1th-2048 input of tests/degenerate.py: w_max = 1 and every other subtree zero, so J_prob[i*] is clamped by
    fmaxf(., 0) and the walks go all one way."""
    case = [c for c in D.NARROW if c[0] == "prop1th-2048"][0]
    _, name, N, T, Tend, eb, _, _, _ = case
    toy_ = D.named_toy(name)
    x0, bs = D.sweep_inputs(toy_, N, T)
    _check(toy_, N, T, 1, "2", oracle, dev, monkeypatch, bs=bs, x0=x0, keys=D.sweep_key(oracle, 0), Tend=Tend, eb=eb, finite=False)


@pytest.mark.parametrize("toy", [toy_31, lambda: toy_gp(16)], ids=["du3", "du16"])
def test_wider_states(toy, oracle, dev, monkeypatch):
    """N = 2048, two chains: DMAX = 4 (the noise waves park both normals of a pair in LDS) and DMAX = 16 (every slot draws its
    own noise, so the role waves draw theirs before they take up their roles)."""
    _check(toy(), 2048, 4, 2, "2", oracle, dev, monkeypatch)


def test_stored_path_ancestors_and_particles(oracle, dev, monkeypatch):
    """explicit_backward=False at N = 1024: As, uss and log_wss of every step against the other two kernels and against the
    oracle's own forward pass under the sweep's keys."""
    toy_, N, T, C = toy_31(), 1024, 4, 2
    v = _check(toy_, N, T, C, "2", oracle, dev, monkeypatch, eb=False)
    assert {"As", "uss", "log_wss"} <= set(v)
    x0, bs, keys = _inputs(toy_, N, T, C, oracle)
    om = oracle_model_from(oracle, _bridge(toy_, np.linspace(0, 1.0, T + 1), dev))
    for c in range(C):
        want, _ = oracle_forward(oracle, om, keys[c], x0[c], toy_["y0"], bs[c], N, eb=False)
        for name in ("As", "uss", "log_wss"):
            _eq(v[name][c].reshape(want[name].shape), want[name], f"{name} chain {c} against the oracle")
