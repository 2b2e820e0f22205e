"""The entry loads of the Gibbs step kernels: a step's tables (G, g, sd, lognorm) and its vectors (v_prev, v, ustar) held by
value from the kernel's entry on at DMAX = 1 (gibbs_step_entry / StepValues), the reference row pinned there, and the J
wave's tile sums loaded as two 8-byte pieces at clamped addresses (tile_values4_issue).  None of it
moves any arithmetic, so every result is bit for bit what it was: one sweep per case, without a graph, and the four outputs,
the final particles and the final log-weights compared with the CPU oracle (``gibbs_kernel_lg(..., debug=True)``); the
stored path (ancestors, particles and log-weights of every step) with the oracle's own forward pass.

The shapes are the smallest at which each part can go wrong: two tiles (the clamped loads of a lane hit the same two
values), four tiles (the first shape where a lane's four values are all real) and eight; one step (the tables of both ends
of the path, s and s + 1) and three; one to three chains (every per-chain buffer at an offset); and a random non-zero y0, so
that v and v_prev matter in every drift and every log-likelihood."""
import functools

import numpy as np
import pytest

from helpers import toy_2d, toy_4d, toy_31, toy_gp, oracle_model_from
from jwave_restate import oracle_forward
from test_gpu_lg import _bridge, _eq, _np

pytestmark = pytest.mark.gpu

MODELS = {"dmax1": toy_2d, "dmax2": toy_4d, "dmax4": toy_31, "dmax16": functools.partial(toy_gp, 16, dv=1)}
OUTPUTS = ("x0_next", "us_star_next", "bs_star_next", "acc")


def _y0(toy, seed):
    """A non-zero observation start of the model's width (the toys' own y0 of toy_2d is 0)."""
    y0 = np.random.default_rng(100 + seed).normal(size=np.shape(toy["y0"])).astype(np.float32)
    assert np.all(y0 != 0)
    return y0


@functools.lru_cache(maxsize=None)
def _reference(model, n, ef, eb, nchains, steps, bs_key):
    """(x0, y0, bs, keys, oracle outputs per chain): computed once per ensemble, shared by the kernels run on it, read-only."""
    import torch
    import oracle as O
    toy = MODELS[model]()
    br = _bridge(toy, np.linspace(0, 1.0, steps + 1), torch.device("cpu"))   # host tables only
    om = oracle_model_from(O, br)
    rows = n + int(ef)
    rng = np.random.default_rng(rows + 7 * nchains + steps)
    x0 = rng.normal(size=(nchains, toy["du"])).astype(np.float32)
    bs = rng.integers(0, rows, (nchains, steps + 1)).astype(np.int32) if bs_key is None else \
        np.tile(np.asarray(bs_key, np.int32), (nchains, 1))
    y0 = _y0(toy, rows)
    keys = O.split(O.PRNGKey(47), max(nchains, 2))[:nchains]
    want = [O.gibbs_kernel_lg(om, keys[c], x0[c], y0, bs[c], n, eb, ef, debug=True) for c in range(nchains)]
    for ws in want:
        for w in ws:
            w.setflags(write=False)
    return x0, y0, bs, keys, om, want


def _check(model, n, steps, nchains, switches, dev, monkeypatch, ef=False, eb=True, bs=None):
    for name in ("FBSMI_TREE_HALVES", "FBSMI_PROP_HALFWAVE", "FBSMI_TWO_SLOT_PROP", "FBSMI_TREE_STEP", "FBSMI_J_WAVE"):
        monkeypatch.delenv(name, raising=False)
    for name, value in switches.items():
        monkeypatch.setenv(name, value)
    toy = MODELS[model]()
    x0, y0, bs, keys, om, want = _reference(model, n, ef, eb, nchains, steps, None if bs is None else tuple(bs))
    br = _bridge(toy, np.linspace(0, 1.0, steps + 1), dev)   # a bridge of its own: the switches are read when a handle is made
    sweep = br.sweep_handle(n, eb, ef, nchains=nchains)
    one = nchains == 1
    got = sweep.sweep(keys[0] if one else keys, x0[0] if one else x0, y0, bs[0] if one else bs, use_graph=False)
    v = sweep.views()
    pick = lambda t, c: _np(t) if one else _np(t[c])
    for c in range(nchains):
        assert np.isfinite(want[c][5]).all()
        for i, what in enumerate(OUTPUTS):
            _eq(pick(got[i], c), want[c][i], f"{what} chain {c}")
        _eq(pick(v["us_T"], c), want[c][4], f"final particles chain {c}")
        _eq(pick(v["lw_T"], c), want[c][5], f"final log-weights chain {c}")
    return v, (x0, y0, bs, keys, om)


# ---- the headline kernel: k_lg_prop1th<DMAX, 2, true> behind k_lg_norm<1, 0, true>
@pytest.mark.parametrize("nchains", [1, 2, 3])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("n", [512, 1024, 2048])
@pytest.mark.parametrize("model", list(MODELS))
def test_prop1th_tables_by_value_and_entry_rounds(model, n, steps, nchains, dev, monkeypatch):
    _check(model, n, steps, nchains, {"FBSMI_TREE_HALVES": "2"}, dev, monkeypatch)


@pytest.mark.parametrize("i_ref", ["first tile", "last tile"])
@pytest.mark.parametrize("j_ref", ["0", "N/2-1", "N/2", "N-1"])
@pytest.mark.parametrize("model", ["dmax1", "dmax2"])
def test_preloaded_ustar_and_uref_at_the_edges(model, j_ref, i_ref, dev, monkeypatch):
    """The pinned slot j* = bs[s + 1] takes the preloaded us_star[s + 1] and the preloaded reference row up[:, bs[s]]: j* is the
    first and the last slot of either side of a pair (lanes l and l + 32 of one wave hold slots N/2 apart), i* lies in the first
    and in the last tile (the tile the J wave loads at entry).  Three steps, so that every step has both."""
    n = 1024
    j = {"0": 0, "N/2-1": n // 2 - 1, "N/2": n // 2, "N-1": n - 1}[j_ref]
    i = 5 if i_ref == "first tile" else n - 3
    _check(model, n, 3, 2, {"FBSMI_TREE_HALVES": "2"}, dev, monkeypatch, bs=[i, j, i, j])


def test_prop1th_four_tiles_per_workgroup(dev, monkeypatch):
    """k_lg_prop1th<1, 4, true>: sixteen waves, the same entry."""
    _check("dmax1", 1024, 3, 2, {"FBSMI_TREE_HALVES": "4"}, dev, monkeypatch)


def test_prop1th_stored_path(dev, monkeypatch):
    """explicit_backward=False at DMAX = 1: the slot tail stores As and uss from the preloaded values; with log_wss (k_lg_norm)
    against the oracle's own forward pass under the sweep's keys."""
    import oracle as O
    n, steps, nchains = 1024, 3, 2
    v, (x0, y0, bs, keys, om) = _check("dmax1", n, steps, nchains, {"FBSMI_TREE_HALVES": "2"}, dev, monkeypatch, eb=False)
    assert {"As", "uss", "log_wss"} <= {k for k, t in v.items() if t is not None}
    for c in range(nchains):
        want, _ = oracle_forward(O, om, keys[c], x0[c], y0, bs[c], n, eb=False)
        for name in ("As", "uss", "log_wss"):
            _eq(_np(v[name][c]).reshape(want[name].shape), want[name], f"{name} chain {c}")


# ---- every other kernel that shares the slot body: (nparticles, explicit_final, switches), as sweep_steps_narrow dispatches
OTHERS = {
    "k_lg_prop1t": (512, False, {"FBSMI_TREE_HALVES": "1"}),
    "k_lg_prop1tp": (1024, False, {"FBSMI_TREE_HALVES": "2", "FBSMI_PROP_HALFWAVE": "0"}),
    "k_lg_prop1th-shared-trees": (1024, False, {"FBSMI_TREE_HALVES": "2", "FBSMI_J_WAVE": "0"}),
    "k_lg_prop2t": (1024, False, {"FBSMI_TWO_SLOT_PROP": "1"}),
    "k_lg_prop2": (1024, False, {"FBSMI_TWO_SLOT_PROP": "1", "FBSMI_TREE_STEP": "0"}),
    "k_lg_prop1-cdf": (600, False, {}),                # no power of two: the cdf path
    "lg_step1_body": (100, False, {}),                 # one tile: the whole pass is one launch, loads behind stores
    "k_lg_prop1t-plus1": (512, True, {}),              # 513 slots with explicit_final
}


@pytest.mark.parametrize("model", ["dmax1", "dmax2"])
@pytest.mark.parametrize("kernel", list(OTHERS))
def test_kernels_that_share_the_slot_body(kernel, model, dev, monkeypatch):
    n, ef, switches = OTHERS[kernel]
    _check(model, n, 3, 2, switches, dev, monkeypatch, ef=ef)
