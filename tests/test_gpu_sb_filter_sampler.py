"""GPU parity of the fused SB bootstrap-filter conditional sampler (fbsmi_lg_fsamp_create_em, SBFilterSampler,
samplers.sb_filter_conditional_sampler, examples/toy_sb_filter.py --fused --batch) against the oracle composition of
tests/sb_fsamp_restate.py on the same keys, bit for bit."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from helpers import oracle_model_from, toy_2d
from sb_restate import gibbs_kernel_sb, sb_problem
import fsamp_restate
import sb_fsamp_restate as R

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


_MODELS = {}


def _setup(du, dv, T, nsub, dev):
    """The SB bridge of sb_problem cut to D = du + dv coordinates on ts = linspace(0, 1, T + 1), y0 and a proper prior
    (a random SPD covariance's lower factor), shared by the tests: handles are cached on the bridge."""
    import fbs_amd
    k = (du, dv, T, nsub)
    if k not in _MODELS:
        D = du + dv
        m0, c0, m1, c1 = sb_problem((D + 1) // 2, 0)
        ts = np.linspace(0.0, 1.0, T + 1)
        br = fbs_amd.GaussianSBBridge(m0[:D], c0[:D, :D], m1[:D], c1[:D, :D], ts, du=du, sig=1.0, nsub=nsub, device=dev)
        rng = np.random.default_rng(1000 * du + dv)
        y0 = rng.normal(size=dv).astype(f32)
        A = rng.normal(size=(du, du))
        prior = (rng.normal(size=du).astype(f32), np.linalg.cholesky(A @ A.T / du + 0.5 * np.eye(du)).astype(f32))
        _MODELS[k] = (br, ts, y0, prior)
    return _MODELS[k]


def _em(br):
    h = br.em_host
    return h["M"], h["c"], h["ddt"], h["s"], br.nsub


_WANT = {}


def _want(O, case, br, y0, key, n, resampling, prior):
    """The oracle's sample of one key (computed once per case and shared)."""
    k = (case, int(key[0]), int(key[1]), n, resampling, prior is not None)
    if k not in _WANT:
        _WANT[k] = R.want(O, oracle_model_from(O, br), _em(br), br.pmcmc_tables_host(None), key, y0, n, resampling, prior)
    return _WANT[k]


def _keys(O, seed, B):
    return O.split(O.PRNGKey(seed), B)


def _check(O, case, br, y0, h, keys, n, resampling, prior=None, use_graph=True):
    samples, nell = h.sample(keys, y0, return_nell=True, use_graph=use_graph)
    v = h.views()
    B = len(keys)
    assert samples.shape == (B, br.du) and nell.shape == (B,)
    assert v["vs"].shape == (B, br.T + 1, br.dv) and v["u0s"].shape == v["uT"].shape == (B, n, br.du)
    for b in range(B):
        w_vs, w_u0s, w_sample, w_nell = _want(O, case, br, y0, keys[b], n, resampling, prior)
        tag = f"{case} N={n} B={B} {resampling} {'proper' if prior else 'heuristic'} sample {b}"
        _eq(_np(v["vs"][b]), w_vs, f"vs {tag}")
        _eq(_np(v["u0s"][b]), w_u0s, f"u0s {tag}")
        _eq(_np(v["uT"][b, 0]), w_sample, f"uT row 0 {tag}")
        _eq(_np(samples[b]), w_sample, f"sample {tag}")
        _eq(_np(nell[b]).reshape(1), np.array([w_nell], f32), f"nell {tag}")
    return samples, nell


# ---- 1. parity --------------------------------------------------------------------------------------------------------
# (du, dv, T, nsub, particles, batch sizes, resamplings, priors).  The particle counts cross the filter's launch sequences
# (one launch, three launches at 300, the tree step at 4096, the wide family at d = 20); the models cross the front's:
# D = 2 .. 256 (one to four waves, one to eight M chunks), du != dv both ways, T = 1 and nsub = 1, and T = 1025, one past
# the intervals whose keys the front keeps in LDS (the handle's slab takes them).
BOTH = ("stratified", "systematic")
PARITY = [(1, 1, 6, 3, 64, (1, 3), BOTH[:1], (False,)),
          (3, 3, 20, 10, 300, (3,), BOTH[:1], (False, True)),
          (3, 3, 12, 10, 4096, (2,), BOTH[:1], (False,)),
          (20, 20, 12, 10, 200, (1, 3), BOTH, (False,)),
          (20, 20, 12, 10, 200, (3,), BOTH[:1], (True,)),
          (5, 7, 8, 4, 64, (2,), BOTH[:1], (False,)),
          (7, 5, 8, 4, 64, (2,), BOTH[:1], (False,)),
          (33, 32, 4, 3, 32, (2,), BOTH[:1], (False,)),
          (128, 128, 3, 2, 32, (2,), BOTH[:1], (False,)),
          (3, 3, 1, 1, 64, (2,), BOTH[:1], (False,)),
          (1, 1, 1025, 1, 32, (2,), BOTH[:1], (False,))]
PARITY = [(du, dv, T, nsub, n, B, r, p) for du, dv, T, nsub, n, Bs, rs, ps in PARITY for B in Bs for r in rs for p in ps]


@pytest.mark.parametrize("case", PARITY, ids=["-".join(str(x) for x in c[:6]) + f"-{c[6]}-{'proper' if c[7] else 'heuristic'}"
                                             for c in PARITY])
def test_parity_with_the_oracle(case, oracle, dev):
    du, dv, T, nsub, n, B, resampling, proper = case
    br, ts, y0, prior = _setup(du, dv, T, nsub, dev)
    prior = prior if proper else None
    assert br.fused_sb_filter_sampler_supported(n, B)
    h = br.sb_filter_sampler_handle(n, resampling, B, prior)
    assert h is br.sb_filter_sampler_handle(n, resampling, B, prior), "handles are cached by the sizes and the prior's bytes"
    _check(oracle, case[:4], br, y0, h, _keys(oracle, 41, 3)[:B], n, resampling, prior)


def test_the_prior_is_part_of_the_cache_key(dev):
    br, ts, y0, prior = _setup(3, 3, 20, 10, dev)
    a, b = br.sb_filter_sampler_handle(64, "stratified", 2), br.sb_filter_sampler_handle(64, "stratified", 2, prior)
    other = (prior[0] + f32(1), prior[1])
    assert a is not b and br.sb_filter_sampler_handle(64, "stratified", 2, other) is not b
    assert br.sb_filter_sampler_handle(64, "stratified", 2, (prior[0].astype(np.float64), prior[1].copy())) is b


# ---- 2. ragged batch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proper", [False, True])
def test_ragged_batch(proper, oracle, dev):
    br, ts, y0, prior = _setup(3, 3, 20, 10, dev)
    prior = prior if proper else None
    keys = _keys(oracle, 43, 5)
    h = br.sb_filter_sampler_handle(64, "stratified", 5, prior)
    full, full_nell = h.sample(keys, y0, return_nell=True)
    part, part_nell = h.sample(keys[:3], y0, return_nell=True)
    assert part.shape == (3, 3) and h.views()["vs"].shape[0] == 3
    assert h._last is br.sb_filter_sampler_handle(64, "stratified", 3, prior), "the cached handle of that size and prior"
    _eq(_np(part), _np(full[:3]), "ragged samples")
    _eq(_np(part_nell), _np(full_nell[:3]), "ragged nell")
    one = h.sample(keys[4], y0)                                           # a single key of shape (2,)
    _eq(_np(one), _np(full[4:5]), "one key")
    with pytest.raises(ValueError):
        h.sample(_keys(oracle, 43, 6), y0)
    for b in (0, 4):
        _eq(_np(full[b]), _want(oracle, (3, 3, 20, 10), br, y0, keys[b], 64, "stratified", prior)[2], f"sample {b}")


# ---- 3. chunking --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("du,T,n", [(3, 20, 64), (20, 12, 200)])
def test_chunking_does_not_change_results(du, T, n, oracle, dev):
    from fbs_amd import samplers
    br, ts, y0, prior = _setup(du, du, T, 10, dev)
    keys = _keys(oracle, 44, 5)
    args = (keys, y0, ts, br.fwd_sampler, br.unpack, br.ref_sampler, br.transition_sampler, br.likelihood_logpdf, n,
            samplers.stratified)
    one, one_nell = samplers.sb_filter_conditional_sampler(*args, return_nell=True)
    two, two_nell = samplers.sb_filter_conditional_sampler(*args, return_nell=True, _bound=2 * n * br.du)   # chunks of 2, 2, 1
    assert one.shape == (5, br.du) and one_nell.shape == (5,)
    assert ("sb_fsamp", n, "stratified", 5, None) in br._sweeps and ("sb_fsamp", n, "stratified", 2, None) in br._sweeps
    _eq(_np(two), _np(one), "chunked samples")
    _eq(_np(two_nell), _np(one_nell), "chunked nell")
    for b in range(5):
        w = _want(oracle, (du, du, T, 10), br, y0, keys[b], n, "stratified", None)
        _eq(_np(one[b]), w[2], f"sample {b}")
        _eq(_np(one_nell[b]).reshape(1), np.array([w[3]], f32), f"nell {b}")
    assert samplers.sb_filter_conditional_sampler(*args).shape == (5, br.du)


# ---- 4. graph / no graph, no state between calls ------------------------------------------------------------------------
@pytest.mark.parametrize("du,T,n", [(3, 12, 4096), (20, 12, 200)])
def test_use_graph_and_consecutive_calls(du, T, n, oracle, dev):
    br, ts, y0, prior = _setup(du, du, T, 10, dev)
    h = br.sb_filter_sampler_handle(n, "stratified", 2)
    ka, kb = _keys(oracle, 41, 3)[:2], _keys(oracle, 45, 2)
    for use_graph in (True, False, True):
        _check(oracle, (du, du, T, 10), br, y0, h, ka, n, "stratified", None, use_graph)
        _check(oracle, (du, du, T, 10), br, y0, h, kb, n, "stratified", None, use_graph)


# ---- 5. tier agreement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("du,dv,T,nsub,n", [(3, 3, 20, 10, 64), (20, 20, 12, 10, 200), (5, 7, 8, 4, 64)])
def test_tiers_agree_where_that_is_well_defined(du, dv, T, nsub, n, oracle, dev):
    from fbs_amd import ops
    br, ts, y0, prior = _setup(du, dv, T, nsub, dev)
    keys = _keys(oracle, 46, 2)
    h = br.sb_filter_sampler_handle(n, "stratified", 2)
    h.sample(keys, y0)
    v = h.views()
    tab = br.pmcmc_tables_host(None)
    for b in range(2):
        key_x0, key_em, key_bf, key_init = R.keys_of(ops, keys[b])
        x0 = ops.normal(key_x0, (du,), device=dev)
        vs = torch.flip(br.fwd_sampler(key_em, x0, torch.from_numpy(y0).to(dev))[:, du:], [0])   # the same em_path_run
        _eq(_np(v["vs"][b]), _np(vs), f"vs {b}")
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
    from fbs_amd import _lib
    from fbs_amd.sdes import StationaryConstLinearSDE
    sb, ts, y0, prior = _setup(3, 3, 8, 3, dev)
    toy = toy_2d()
    lg = fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(-0.5, 1.0), np.linspace(0, 2, 31), 1,
                                      device=dev)
    assert not hasattr(lg, "sb_filter_sampler_handle")
    tab = sb.pmcmc_tables(None)
    mean, chol = (torch.from_numpy(a).to(dev) for a in prior)
    h = C.c_void_p()
    create = lambda fwd, tables, m, c, B: _lib.call("fbsmi_lg_fsamp_create_em", C.byref(sb.struct), fwd, tables, m, c, 64, 0,
                                                    B, C.byref(h))
    with pytest.raises(RuntimeError, match="null"):
        create(None, C.byref(tab), None, None, 1)
    with pytest.raises(RuntimeError, match="null"):
        create(C.byref(sb.em_struct), None, None, None, 1)
    with pytest.raises(RuntimeError, match="both"):
        create(C.byref(sb.em_struct), C.byref(tab), mean.data_ptr(), None, 1)
    with pytest.raises(RuntimeError, match="both"):
        create(C.byref(sb.em_struct), C.byref(tab), None, chol.data_ptr(), 1)
    bad = _lib.EMForwardStruct(0, *(sb.em_dev[k].data_ptr() for k in ("M", "c", "ddt", "s")))
    with pytest.raises(RuntimeError, match="forward tables"):
        create(C.byref(bad), C.byref(tab), None, None, 1)
    with pytest.raises(NotImplementedError, match="65535"):
        create(C.byref(sb.em_struct), C.byref(tab), None, None, 65536)
    assert not h.value
    assert not sb.fused_sb_filter_sampler_supported(64, 65536)
    with pytest.raises(NotImplementedError):                                  # the separable engine keeps refusing the model
        sb.filter_sampler_handle(64)
    # afterwards the separable engine and the SB sweep in the same process still match their oracles
    keys = _keys(oracle, 47, 2)
    hl = lg.filter_sampler_handle(64, "stratified", 2)
    got = hl.sample(keys, toy["y0"])
    for b in range(2):
        w = fsamp_restate.want(oracle, oracle_model_from(oracle, lg), lg.pmcmc_tables_host(None), keys[b], toy["y0"], 64,
                               "stratified")
        _eq(_np(got[b]), w[2], f"LG sample {b}")
    rng = np.random.default_rng(3)
    x0 = rng.normal(size=3).astype(f32)
    bs = rng.integers(0, 16, sb.T + 1).astype(np.int32)
    got = sb.sweep_handle(16, True, False).sweep(keys[0], x0, y0, bs)
    want = gibbs_kernel_sb(oracle, oracle_model_from(oracle, sb), _em(sb), keys[0], x0, y0, bs, 16, True, False)
    for i, what in enumerate(("x0_next", "us_star_next", "bs_next")):
        _eq(_np(got[i]), np.asarray(want[i], _np(got[i]).dtype), f"SB sweep {what}")
    # and the SB engine itself still runs
    _check(oracle, (3, 3, 8, 3), sb, y0, sb.sb_filter_sampler_handle(64, "stratified", 2), keys, 64, "stratified")


# ---- 7. the driver ------------------------------------------------------------------------------------------------------
def test_toy_sb_filter_driver_batched(tmp_path, dev):
    ex = os.path.join(ROOT, "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    spec = importlib.util.spec_from_file_location("toy_sb_filter_batched", os.path.join(ex, "toy_sb_filter.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for x0 in ("proper", "heuristic"):
        argv = ["--d", "3", "--nparticles", "32", "--nsamples", "40", "--x0", x0, "--fused", "--outdir", str(tmp_path), "--quiet"]
        samples, gp_mean, gp_cov = mod.main(argv + ["--batch", "16"])
        assert samples.shape == (40, 3) and np.isfinite(samples).all()
        z = (samples.mean(0) - gp_mean) / np.sqrt(np.diag(gp_cov))
        assert np.abs(z).max() < 1.5, (x0, z)
        saved = np.load(os.path.join(str(tmp_path), f"filter-{x0}-32-666.npz"))
        assert set(saved.files) == {"samples", "gp_mean", "gp_cov"}
        _eq(saved["samples"], samples, "saved samples")
        whole = mod.main(argv + ["--batch", "40"])[0]
        _eq(samples, whole, f"--batch 16 against --batch 40 ({x0})")
