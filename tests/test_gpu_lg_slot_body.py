"""The per-slot step that the narrow Gibbs propagation kernels share (gibbs_step_entry / gibbs_slot_gather /
gibbs_slot_finish of fbs_amd/csrc/fbsmi_lg.hip): every kernel that uses it, at every DMAX it is instantiated for, against the
CPU oracle, bit for bit.  DMAX is 1, 2, 4 or 16 with max(du, dv): toy_2d, toy_4d, toy_31 and the 16-dimensional
Gaussian-process toy observed in one coordinate (still a narrow model).

Two chains, T = 4; the reference path visits slot 0, the last slot and both sides of a tile edge (a wave edge where the
ensemble is one tile).  The forcing switches are those of NARROW in tests/degenerate.py."""
import functools

import numpy as np
import pytest

from helpers import toy_2d, toy_4d, toy_31, toy_gp, oracle_model_from
from test_gpu_lg import _bridge, _eq, _np

pytestmark = pytest.mark.gpu

T, C = 4, 2
MODELS = {"dmax1": toy_2d, "dmax2": toy_4d, "dmax4": toy_31, "dmax16": functools.partial(toy_gp, 16, dv=1)}

# id -> (nparticles, explicit_final, forcing switches): the step kernel the dispatch code reaches (sweep_steps_narrow in
# fbsmi_lg.hip; nb = tiles of 256 slots, C = 2 chains per launch).  What each row relies on:
KERNELS = {
    "k_lg_prop1": (777, False, {}),                        # N neither a power of two nor 2^k + 1: no tree, one slot per thread
    "k_lg_prop1t": (512, False, {}),                       # power of two, nb * C = 4 < 512: no paired workgroups by default
    "k_lg_prop1t-plus1": (512, True, {}),                  # 513 slots = 2^k + 1 (FBSMI_TREE_PLUS1 unset): always one tile each
    "k_lg_prop1th-2": (1024, False, {"FBSMI_TREE_HALVES": "2"}),                       # forced; nb = 4 is even
    "k_lg_prop1tp-2": (1024, False, {"FBSMI_TREE_HALVES": "2", "FBSMI_PROP_HALFWAVE": "0"}),
    "k_lg_prop1th-4": (1024, False, {"FBSMI_TREE_HALVES": "4"}),                       # forced; nb % 4 == 0
    "k_lg_prop2t": (1024, False, {"FBSMI_TWO_SLOT_PROP": "1"}),                        # forced; N % 512 == 0, tree step
    "k_lg_prop2": (1024, False, {"FBSMI_TWO_SLOT_PROP": "1", "FBSMI_TREE_STEP": "0"}),  # ... without the tree step
    "lg_step1_body": (200, False, {}),                     # N <= 256: one tile, the whole pass is one launch (k_lg_sweep1)
}


def _inputs(toy, rows, nchains, steps, edge):
    """x0 and reference indices: every chain's path holds 0, rows - 1 and both sides of `edge`."""
    rng = np.random.default_rng(rows + toy["du"])
    x0 = rng.normal(size=(nchains, toy["du"])).astype(np.float32)
    visit = np.array([0, rows - 1, edge, edge - 1, rows // 2], np.int32)
    bs = np.stack([np.roll(visit, c)[:steps + 1] for c in range(nchains)])
    return x0, bs


@functools.lru_cache(maxsize=None)
def _reference(model, n, ef, eb, nchains, steps, edge):
    """(x0, bs, keys, oracle outputs per chain) -- the same for every kernel run on this ensemble; read-only."""
    import torch
    import oracle as O
    toy = MODELS[model]()
    br = _bridge(toy, np.linspace(0, 1.0, steps + 1), torch.device("cpu"))   # host tables only
    om = oracle_model_from(O, br)
    x0, bs = _inputs(toy, n + int(ef), nchains, steps, edge)
    keys = O.split(O.PRNGKey(31), max(nchains, 2))[:nchains]
    want = [O.gibbs_kernel_lg(om, keys[c], x0[c], toy["y0"], bs[c], n, eb, ef, debug=True) for c in range(nchains)]
    for ws in want:
        for w in ws[:6]:
            w.setflags(write=False)
    return x0, bs, keys, want


def _check(model, n, ef, eb, switches, dev, monkeypatch, nchains=C, steps=T, edge=256):
    for name, value in switches.items():
        monkeypatch.setenv(name, value)
    toy = MODELS[model]()
    x0, bs, keys, want = _reference(model, n, ef, eb, nchains, steps, edge)
    br = _bridge(toy, np.linspace(0, 1.0, steps + 1), dev)
    sweep = br.sweep_handle(n, eb, ef, nchains=nchains)
    got = sweep.sweep(keys if nchains > 1 else keys[0], x0 if nchains > 1 else x0[0], toy["y0"], bs if nchains > 1 else bs[0])
    v = sweep.views()
    for c in range(nchains):
        pick = (lambda t: _np(t[c])) if nchains > 1 else _np
        for i, what in enumerate(("x0_next", "us_star_next", "bs_star_next", "acc")):
            _eq(pick(got[i]), want[c][i], f"{what} chain {c}")
        _eq(pick(v["us_T"]), want[c][4], f"final particles chain {c}")
        _eq(pick(v["lw_T"]), want[c][5], f"final log-weights chain {c}")


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_shared_slot_body_matches_oracle(kernel, model, dev, monkeypatch):
    n, ef, switches = KERNELS[kernel]
    _check(model, n, ef, True, switches, dev, monkeypatch, edge=256 if n > 256 else 64)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_shared_slot_body_stored_path(kernel, dev, monkeypatch):
    """explicit_backward=False: the ancestors and particles of every step are stored by the shared tail (gibbs_slot_gather's
    As, gibbs_slot_finish's uss) and the backward scan reads them.  Once per kernel, at DMAX = 2."""
    n, ef, switches = KERNELS[kernel]
    _check("dmax2", n, ef, False, switches, dev, monkeypatch, edge=256 if n > 256 else 64)


@pytest.mark.parametrize("model,eb", [("dmax1", True), ("dmax16", True), ("dmax2", False)])
def test_shared_slot_body_several_slots_per_thread(model, eb, dev, monkeypatch):
    """k_lg_heaps + k_lg_propQ<4, .>: N > 131072 (four slots per thread, tiles of 1024 slots); one chain, T = 2.  The third
    case is the kernel's stored path (explicit_backward=False) at DMAX = 2."""
    _check(model, 200000, False, eb, {}, dev, monkeypatch, nchains=1, steps=2, edge=1024)
