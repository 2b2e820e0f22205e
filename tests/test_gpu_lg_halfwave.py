"""k_lg_prop1th<., 2 | 4>: the workgroups of tiles N/2 apart with both slots of a pair in one wave (lanes l and l + 32), so the
kill-test and redraw uniforms take one Threefry call per pair, the words changing hands by a cross-lane swap.  Every case is
compared bit for bit with the CPU oracle (``gibbs_kernel_lg(..., debug=True)``: the four outputs, the final particles and
log-weights) and with a handle running the paired kernel it replaces (k_lg_prop1tp, FBSMI_PROP_HALFWAVE=0) on the same inputs.
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


def _sweep(toy, ts, dev, monkeypatch, halves, halfwave, N, eb, C, keys, x0, y0, bs):
    """One sweep of a fresh handle created under FBSMI_TREE_HALVES=halves, FBSMI_PROP_HALFWAVE=halfwave -> (outputs, views)
    as numpy arrays with a leading chain axis."""
    monkeypatch.setenv("FBSMI_TREE_HALVES", halves)
    monkeypatch.setenv("FBSMI_PROP_HALFWAVE", halfwave)
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
    keys = oracle.split(oracle.PRNGKey(31), max(C, 2))[:C]
    return x0, bs, keys


def _check(toy_, N, T, C, halves, oracle, dev, monkeypatch, bs=None, y0=None, eb=True, seed=0):
    ts = np.linspace(0, 1.0, T + 1)
    x0, bs_rand, keys = _inputs(toy_, N, T, C, oracle, seed)
    bs = np.asarray(bs_rand if bs is None else bs, np.int32).reshape(C, T + 1)
    y0 = toy_["y0"] if y0 is None else np.asarray(y0, np.float32)
    br, got, v = _sweep(toy_, ts, dev, monkeypatch, halves, "1", N, eb, C, keys, x0, y0, bs)
    _, got1, v1 = _sweep(toy_, ts, dev, monkeypatch, halves, "0", N, eb, C, keys, x0, y0, bs)
    om = oracle_model_from(oracle, br)
    for c in range(C):
        want = oracle.gibbs_kernel_lg(om, keys[c], x0[c], y0, bs[c], N, eb, False, debug=True)
        assert np.isfinite(want[5]).all()
        for i, what in enumerate(OUTPUTS):
            _eq(got[i][c], want[i], f"{what} chain {c}")
        _eq(v["us_T"][c], want[4], f"particles chain {c}")
        _eq(v["lw_T"][c], want[5], f"log-weights chain {c}")
    for i, what in enumerate(OUTPUTS):
        _eq(got[i], got1[i], f"{what} against the paired kernel")
    assert set(v) == set(v1)
    for name in v:
        _eq(v[name], v1[name], f"{name} against the paired kernel")
    return v


def _oracle_forward(oracle, om, key, x0, y0, bs, N, eb=True):
    """The stored forward pass (As, log_wss, uss) of the sweep gibbs_kernel_lg(om, key, x0, y0, bs, N, eb, False) makes: the
    oracle's own csmc_forward_pass_lg with the keys and inputs of gibbs.py:126-148 (explicit_backward: the first of four
    sub-keys of key_csmc, else the first of two, csmc.py:65)."""
    du = om.du
    k3 = oracle.split(key, 3)
    path = oracle.lg_fwd_sampler(om, k3[0], np.concatenate([x0, y0]).astype(np.float32))[::-1]
    us, vs = np.ascontiguousarray(path[:, :du]), np.ascontiguousarray(path[:, du:])
    kf = oracle.split(k3[1], 4 if eb else 2)[0]
    us0 = np.repeat(us[:1], N, axis=0)
    lw0 = np.full(N, np.float32(-np.log(float(N))), np.float32)
    return oracle.csmc_forward_pass_lg(om, kf, us, bs, vs, us0, lw0)


def _oracle_shifts(oracle, om, key, x0, y0, bs, N):
    """The roll j* - J (mod N) of every step of the sweep gibbs_kernel_lg(om, key, x0, y0, bs, N, True, False) makes, read off
    the ancestors of the oracle's own forward pass (same keys, gibbs.py:126-148): a slot that is neither killed nor pinned
    has the ancestor m - shift, and those are the majority at the toy's own observation."""
    T = om.T
    As = _oracle_forward(oracle, om, key, x0, y0, bs, N)["As"]
    shifts = []
    for s in range(T):
        votes = np.bincount((np.arange(N) - As[s]) % N, minlength=N)
        assert votes.max() > N // 2
        shifts.append(int(votes.argmax()))
    return shifts


@pytest.mark.parametrize("first", [0, 1, 2, 3])
def test_one_workgroup_holds_the_ensemble_reference_on_tile_edges(first, oracle, dev, monkeypatch):
    """N = 512, one 512-thread workgroup holds both tiles: every wave has a block of 32 slots of either tile.  The reference
    indices run through 0, 255, 256, 511 in turn (starting at each of them), so the pin and J_prob[i*] land on the tile
    edges either side of N/2 -- the first lane of a lower half-wave, the last of an upper one -- and the rotation wraps."""
    edge = [0, 255, 256, 511]
    T = 8
    bs = [edge[(first + k) % 4] for k in range(T + 1)]
    _check(toy_2d(), 512, T, 1, "2", oracle, dev, monkeypatch, bs=bs, seed=first)


def test_word_select_for_rolls_below_at_and_above_half(oracle, dev, monkeypatch):
    """N = 512: the reference indices are chosen, step by step with the oracle, so that the roll j* - J takes the values
    0, 1, 255, 256, 257, 511, 100, 400.  With a roll of 0 every lower slot's source is in the lower half (word 0 of the
    pair's call is its own); from N/2 on it is in the upper half for every pair (word 1); in between the select differs
    from lane to lane inside a half-wave.  J of step s depends on the indices up to s only, so index s + 1 = J + roll."""
    N, T = 512, 8
    want_shift = [0, 1, 255, 256, 257, 511, 100, 400]
    toy_ = toy_2d()
    ts = np.linspace(0, 1.0, T + 1)
    x0, bs, keys = _inputs(toy_, N, T, 1, oracle)
    om = oracle_model_from(oracle, _bridge(toy_, ts, dev))
    bs = bs[0].copy()
    for s in range(T):
        J = (int(bs[s + 1]) - _oracle_shifts(oracle, om, keys[0], x0[0], toy_["y0"], bs, N)[s]) % N
        bs[s + 1] = (J + want_shift[s]) % N
    assert _oracle_shifts(oracle, om, keys[0], x0[0], toy_["y0"], bs, N) == want_shift
    _check(toy_, N, T, 1, "2", oracle, dev, monkeypatch, bs=bs)


@pytest.mark.parametrize("toy", [toy_31, lambda: toy_gp(16)], ids=["du3", "du16"])
def test_several_workgroups_per_chain_wider_states(toy, oracle, dev, monkeypatch):
    """N = 2048, two chains, four 512-thread workgroups per chain.  du = 3 (DMAX = 4) parks both normals of a pair in LDS for
    the threads that own the slots; du = 16 (DMAX = 16, the widest narrow model) is past that rule: every slot draws its
    own noise, and the ancestor's row is fetched after the search."""
    _check(toy(), 2048, 6, 2, "2", oracle, dev, monkeypatch)


def test_one_workgroup_per_chain_holds_two_pairs_of_tiles(oracle, dev, monkeypatch):
    """N = 1024, three chains, du = 2, 1024-thread workgroups: sixteen waves, waves 0-7 on tiles (0, 2), waves 8-15 on tiles
    (1, 3), a chain index in every address."""
    _check(toy_4d(), 1024, 6, 3, "4", oracle, dev, monkeypatch)


def test_nearly_every_slot_killed(oracle, dev, monkeypatch):
    """The observation is y0 = 20 at N = 512 (the toy's marginal standard deviation of y is 0.7), as in
    test_gpu_lg_paired.py::test_queue_empty_and_nearly_full, where the choice is justified with the oracle: every log-weight
    stays finite and the expected killed fraction of the final weights is 0.93.  Nearly every lane takes the two probe
    rounds behind the redraw word that came from its partner (step 0, from uniform weights, kills no slot)."""
    _check(toy_2d(), 512, 6, 1, "2", oracle, dev, monkeypatch, y0=[20.0])


def test_stored_path_ancestors_and_particles(oracle, dev, monkeypatch):
    """explicit_backward=False at N = 1024: the ancestor matrix As, the stored particles uss and log-weights of every step
    are compared with those of the paired kernel and of the oracle's own forward pass (csmc_forward_pass_lg under the sweep's
    keys), next to the oracle's outputs of the backward scan over them."""
    toy_, N, T, C = toy_31(), 1024, 6, 2
    v = _check(toy_, N, T, C, "2", oracle, dev, monkeypatch, eb=False)
    assert {"As", "uss", "log_wss"} <= set(v)
    # ... and with the oracle's own stored forward pass on the same inputs
    x0, bs, keys = _inputs(toy_, N, T, C, oracle)
    om = oracle_model_from(oracle, _bridge(toy_, np.linspace(0, 1.0, T + 1), dev))
    for c in range(C):
        want = _oracle_forward(oracle, om, keys[c], x0[c], toy_["y0"], bs[c], N, eb=False)
        _eq(v["As"][c].reshape(want["As"].shape), want["As"], f"As chain {c} against the oracle")
        _eq(v["uss"][c].reshape(want["uss"].shape), want["uss"], f"uss chain {c} against the oracle")
        _eq(v["log_wss"][c].reshape(want["log_wss"].shape), want["log_wss"], f"log_wss chain {c} against the oracle")
