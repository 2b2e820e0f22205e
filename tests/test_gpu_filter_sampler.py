"""GPU parity of the fused bootstrap-filter conditional sampler (fbsmi_lg_fsamp_*, LGFilterSampler,
samplers.filter_conditional_sampler, examples/toy_filter.py --fused) against the oracle composition of
tests/fsamp_restate.py on the same keys, bit for bit."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from helpers import toy_gp, toy_2d, toy_4d, toy_31, oracle_model_from
import fsamp_restate as R

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(t):
    return t.detach().cpu().numpy()


def _eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    x = a.view(np.uint32) if a.dtype == np.float32 else a
    y = b.view(np.uint32) if b.dtype == np.float32 else b
    bad = np.flatnonzero(x.ravel() != y.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first {bad[:4]}: {a.ravel()[bad[:4]]} vs {b.ravel()[bad[:4]]}"


_BRIDGES = {}


def _setup(name, T, dev):
    """The bridge of a named toy on ts = linspace(0, 2, T + 1) (shared by the tests: handles are cached on it)."""
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    if (name, T) not in _BRIDGES:
        toy = {"2d": toy_2d, "31": toy_31, "4d": toy_4d, "gp20": lambda: toy_gp(20), "gp12v5": lambda: toy_gp(12, dv=5),
               "gp128": lambda: toy_gp(128)}[name]()
        ts = np.linspace(0, 2, T + 1)
        br = fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(-0.5, 1.0), ts, toy["du"], device=dev)
        _BRIDGES[(name, T)] = (toy, ts, br)
    return _BRIDGES[(name, T)]


_WANT = {}


def _want(O, name, T, br, toy, key, n, resampling):
    """The oracle's sample of one key (computed once per case and shared)."""
    k = (name, T, int(key[0]), int(key[1]), n, resampling)
    if k not in _WANT:
        _WANT[k] = R.want(O, oracle_model_from(O, br), br.pmcmc_tables_host(None), key, toy["y0"], n, resampling)
    return _WANT[k]


def _keys(O, seed, B):
    return O.split(O.PRNGKey(seed), B)


def _check(O, name, T, br, toy, h, keys, n, resampling, use_graph=True):
    samples, nell = h.sample(keys, toy["y0"], return_nell=True, use_graph=use_graph)
    v = h.views()
    B = len(keys)
    assert samples.shape == (B, br.du) and nell.shape == (B,)
    assert v["vs"].shape == (B, br.T + 1, br.dv) and v["u0s"].shape == v["uT"].shape == (B, n, br.du)
    for b in range(B):
        w_vs, w_u0s, w_sample, w_nell = _want(O, name, T, br, toy, keys[b], n, resampling)
        tag = f"{name} N={n} B={B} {resampling} sample {b}"
        _eq(_np(v["vs"][b]), w_vs, f"vs {tag}")
        _eq(_np(v["u0s"][b]), w_u0s, f"u0s {tag}")
        _eq(_np(samples[b]), w_sample, f"sample {tag}")
        _eq(_np(nell[b]).reshape(1), np.array([w_nell], f32), f"nell {tag}")
        _eq(_np(v["uT"][b, 0]), w_sample, f"uT row 0 {tag}")
    return samples, nell


# ---- 1. parity --------------------------------------------------------------------------------------------------------
# (model, T, particles, batch sizes, resamplings).  The particle counts cross the filter's launch sequences: one launch
# (<= 256), normalise / cdf / propagate (300), tree step (4096), wide one tile (gp: <= 256); the models cross the front
# kernel's: dv = 1 .. 128 (one and two waves), du != dv both ways, du > 64 >= dv.
BOTH = ("stratified", "systematic")
PARITY = [("2d", 30, 64, (1, 3), BOTH), ("2d", 30, 300, (1, 3), BOTH[:1]), ("2d", 30, 4096, (1, 3), BOTH[:1]),
          ("31", 30, 64, (3,), BOTH[:1]), ("4d", 30, 300, (2,), BOTH[:1]), ("gp20", 30, 200, (1, 3), BOTH),
          ("gp12v5", 30, 64, (2,), BOTH[:1]), ("gp128", 4, 32, (2,), BOTH[:1])]
PARITY = [(m, T, n, B, r) for m, T, n, Bs, rs in PARITY for B in Bs for r in rs]


@pytest.mark.parametrize("case", PARITY, ids=[f"{m}-{n}-B{B}-{r}" for m, T, n, B, r in PARITY])
def test_parity_with_the_oracle(case, oracle, dev):
    name, T, n, B, resampling = case
    toy, ts, br = _setup(name, T, dev)
    assert br.fused_filter_sampler_supported(n, B)
    _check(oracle, name, T, br, toy, br.filter_sampler_handle(n, resampling, B), _keys(oracle, 41, 3)[:B], n, resampling)


# ---- 2. ragged batch ----------------------------------------------------------------------------------------------------
def test_ragged_batch(oracle, dev):
    toy, ts, br = _setup("2d", 30, dev)
    keys = _keys(oracle, 43, 5)
    h = br.filter_sampler_handle(64, "stratified", 5)
    full, full_nell = h.sample(keys, toy["y0"], return_nell=True)
    part, part_nell = h.sample(keys[:3], toy["y0"], return_nell=True)
    assert part.shape == (3, 1) and h.views()["vs"].shape[0] == 3
    _eq(_np(part), _np(full[:3]), "ragged samples")
    _eq(_np(part_nell), _np(full_nell[:3]), "ragged nell")
    one = h.sample(keys[4], toy["y0"])                                    # a single key of shape (2,)
    _eq(_np(one), _np(full[4:5]), "one key")
    with pytest.raises(ValueError):
        h.sample(_keys(oracle, 43, 6), toy["y0"])


# ---- 3. chunking --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("2d", 64), ("gp20", 200)])
def test_chunking_does_not_change_results(name, n, oracle, dev):
    from fbs_amd import samplers
    toy, ts, br = _setup(name, 30, dev)
    keys = _keys(oracle, 44, 5)
    args = (keys, toy["y0"], ts, br.fwd_ys_sampler, br.ref_sampler, br.transition_sampler, br.likelihood_logpdf, n,
            samplers.stratified)
    one, one_nell = samplers.filter_conditional_sampler(*args, return_nell=True)
    two, two_nell = samplers.filter_conditional_sampler(*args, return_nell=True, _bound=2 * n * br.du)   # chunks of 2, 2, 1
    assert one.shape == (5, br.du) and one_nell.shape == (5,)
    _eq(_np(two), _np(one), "chunked samples")
    _eq(_np(two_nell), _np(one_nell), "chunked nell")
    for b in range(5):
        w = _want(oracle, name, 30, br, toy, keys[b], n, "stratified")
        _eq(_np(one[b]), w[2], f"sample {b}")
        _eq(_np(one_nell[b]).reshape(1), np.array([w[3]], f32), f"nell {b}")
    assert samplers.filter_conditional_sampler(*args).shape == (5, br.du)


# ---- 4. graph / no graph, no state between calls ------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("2d", 4096), ("gp20", 200)])
def test_use_graph_and_consecutive_calls(name, n, oracle, dev):
    toy, ts, br = _setup(name, 30, dev)
    h = br.filter_sampler_handle(n, "stratified", 2)
    ka, kb = _keys(oracle, 41, 3)[:2], _keys(oracle, 45, 2)
    for use_graph in (True, False, True):
        _check(oracle, name, 30, br, toy, h, ka, n, "stratified", use_graph)
        _check(oracle, name, 30, br, toy, h, kb, n, "stratified", use_graph)


# ---- 5. tier agreement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("2d", 64), ("gp20", 200), ("gp12v5", 64)])
def test_tiers_agree_where_that_is_well_defined(name, n, oracle, dev):
    from fbs_amd import ops
    toy, ts, br = _setup(name, 30, dev)
    keys = _keys(oracle, 46, 2)
    h = br.filter_sampler_handle(n, "stratified", 2)
    h.sample(keys, toy["y0"])
    v = h.views()
    tab = br.pmcmc_tables_host(None)
    for b in range(2):
        key_fwd, _, key_bf = ops.split(keys[b], 3)
        vs = torch.flip(br.fwd_ys_sampler(key_fwd, torch.from_numpy(toy["y0"]).to(dev)), [0])
        _eq(_np(v["vs"][b]), _np(vs), f"vs {b}")
        key_init = ops.split(key_bf, 2)[0]
        u0 = _np(br.ref_sampler(key_init, vs[0], n)).astype(np.float64)
        # |m_j| + sum_c |z_ic| |chol_cj|: the two tiers accumulate the same terms in different orders
        yT = _np(vs[0]).astype(np.float64)
        m = tab["m_u"] + tab["gain"] @ (yT - tab["m_v"])
        z = np.abs(oracle.normal(key_init, (n, br.du)).astype(np.float64))
        bound = 1e-5 * (np.abs(m)[None, :] + z @ np.abs(tab["chol"].astype(np.float64)))
        err = np.abs(_np(v["u0s"][b]).astype(np.float64) - u0)
        assert np.all(err <= bound), f"u0s {b}: max err / bound = {(err / bound).max():.3g}"


# ---- 6. create-time refusals --------------------------------------------------------------------------------------------
def test_create_time_refusals(oracle, dev):
    import fbs_amd
    from fbs_amd import _lib, samplers
    rng = np.random.default_rng(0)
    A = rng.normal(size=(2, 2))
    ts = np.linspace(0, 1, 11)
    sb = fbs_amd.GaussianSBBridge(np.zeros(2), np.eye(2), np.array([0.5, -0.5]), A @ A.T + np.eye(2), ts, du=1, device=dev)
    assert not sb.fused_filter_sampler_supported(64, 1)
    with pytest.raises(NotImplementedError):
        sb.filter_sampler_handle(64)
    from fbs_amd.sdes import StationaryConstLinearSDE
    lg = fbs_amd.LinearGaussianBridge(toy_2d()["m0"], toy_2d()["cov0"], StationaryConstLinearSDE(-0.5, 1.0), ts, 1, device=dev)
    h = C.c_void_p()
    with pytest.raises(NotImplementedError, match="no exact forward transition"):   # F and sqQ are all-zero placeholders
        _lib.call("fbsmi_lg_fsamp_create", C.byref(sb.struct), C.byref(lg.pmcmc_tables(None)), 64, 0, 1, C.byref(h))
    with pytest.raises(RuntimeError, match="null"):
        _lib.call("fbsmi_lg_fsamp_create", C.byref(lg.struct), None, 64, 0, 1, C.byref(h))
    assert not h.value
    # the public function falls back to the loop for such a model (its observation path is the y part of a joint
    # Euler-Maruyama path, as examples/toy_sb_filter.py draws it: the bridge's own fwd_ys_sampler refuses)
    from fbs_amd.samplers.smc import _fused_filter_sampler
    assert _fused_filter_sampler(ts, sb.fwd_ys_sampler, sb.ref_sampler, sb.transition_sampler, sb.likelihood_logpdf, 64,
                                 samplers.stratified) is None
    keys = _keys(oracle, 47, 3)
    fwd_ys = lambda key, y0: sb.unpack(sb.fwd_sampler(key, np.zeros(1, f32), y0))[1]
    out = samplers.filter_conditional_sampler(keys, np.zeros(1, f32), ts, fwd_ys, sb.ref_sampler,
                                              sb.transition_sampler, sb.likelihood_logpdf, 64, samplers.stratified)
    assert out.shape == (3, 1) and torch.isfinite(out).all()
    # beyond the wide filter's bound: an argument check of the library before any allocation or launch
    toy, _, wide = _setup("gp20", 30, dev)
    assert not wide.fused_filter_sampler_supported(131073, 1)
    with pytest.raises(NotImplementedError, match="131072"):
        wide.filter_sampler_handle(131073)


# ---- 7. the driver ------------------------------------------------------------------------------------------------------
def test_toy_filter_driver_fused(tmp_path, oracle, dev):
    O_ = oracle
    from fbs_amd import ops, samplers
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        spec = importlib.util.spec_from_file_location("toy_filter_fused", os.path.join(ROOT, "examples", "toy_filter.py"))
        tf = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tf)
        from _gp_toy import gp_setting
    finally:
        sys.path.remove(os.path.join(ROOT, "examples"))
    argv = ["--d", "10", "--nsamples", "6", "--nparticles", "50", "--outdir", str(tmp_path), "--quiet"]
    samples, gp_mean, gp_cov = tf.main(argv + ["--fused", "--batch", "4"])
    assert samples.shape == (6, 10) and np.isfinite(samples).all()
    saved = np.load(os.path.join(str(tmp_path), "filter-const-50-666.npz"))
    assert set(saved.files) == {"samples", "gp_mean", "gp_cov"}
    _eq(saved["samples"], samples, "saved samples")
    g = gp_setting(tf.argparse.Namespace(id=666, d=10, sde="const"), dev)
    key, subkeys = g["key"], []
    for _ in range(6):
        key, subkey = ops.split(key)
        subkeys.append(subkey)
    br = g["bridge"]
    direct = samplers.filter_conditional_sampler(np.stack(subkeys), g["y0_t"], g["ts"], br.fwd_ys_sampler, br.ref_sampler,
                                                 br.transition_sampler, br.likelihood_logpdf, 50, samplers.stratified)
    _eq(samples, _np(direct), "driver samples")
    # both went through the fused engine, not the loop: the direct call's bridge holds the six-sample handle, and the
    # samples are the oracle composition's (the loop tier's differ from it: one flipped ancestor, see the tier test)
    assert ("fsamp", 50, "stratified", 6) in br._sweeps
    want = np.stack([R.want(O_, oracle_model_from(O_, br), br.pmcmc_tables_host(None), k, g["y0"], 50, "stratified")[2]
                     for k in subkeys])
    _eq(samples, want, "driver samples against the oracle composition")
