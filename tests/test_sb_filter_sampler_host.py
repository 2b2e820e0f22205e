"""CPU: the host side of the fused SB bootstrap-filter conditional sampler -- the dispatch predicate of
fbs_amd.samplers.sb_filter_conditional_sampler, its reuse of the chunk planner, the restated proper-x0 chain and the public
signature.  No device is touched."""
import inspect

import numpy as np
import pytest

import sb_fsamp_restate as R

ROLES = ("fwd_sampler", "fwd_ys_sampler", "unpack", "ref_sampler", "transition_sampler", "likelihood_logpdf",
         "transition_logpdf")


def _bare_bridge(cls, ts, du=1, dv=1, sde=None, em=False):
    """A bridge with what the dispatch predicate reads and no device behind it (the constructor needs a GPU)."""
    from fbs_amd.linear_gaussian import _Closure
    br = object.__new__(cls)
    br.du, br.dv, br.sde = du, dv, sde
    br.ts_np = np.asarray(ts, np.float64)
    br.T = br.ts_np.size - 1
    if em:
        br.em_struct = object()
    for role in ROLES:
        setattr(br, role, _Closure(br, lambda *a, **k: pytest.fail("the predicate must not call a closure"), role))
    return br


def _own(b):
    return b.fwd_sampler, b.unpack, b.ref_sampler, b.transition_sampler, b.likelihood_logpdf


def test_dispatch_predicate_refuses_without_touching_a_device():
    from fbs_amd import samplers
    from fbs_amd.gaussian_sb import GaussianSBBridge
    from fbs_amd.linear_gaussian import LinearGaussianBridge
    from fbs_amd.samplers.smc import _fused_sb_filter_sampler as pred
    from fbs_amd.sdes import StationaryConstLinearSDE
    ts = np.linspace(0, 1, 31)
    br, other = _bare_bridge(GaussianSBBridge, ts, em=True), _bare_bridge(GaussianSBBridge, ts, em=True)
    assert br.fused_sb_filter_sampler_supported(64) and br.fused_sb_filter_sampler_supported(64, 65535)
    assert not br.fused_sb_filter_sampler_supported(64, 65536) and not br.fused_sb_filter_sampler_supported(64, 0)
    assert pred(ts, *_own(br), 64, samplers.stratified) == (br, "stratified")
    assert pred(ts, *_own(br), 64, samplers.systematic) == (br, "systematic")
    plain = lambda *a, **k: None
    assert pred(ts, plain, plain, plain, plain, plain, 64, samplers.stratified) is None                       # foreign closures
    assert pred(ts, plain, br.unpack, br.ref_sampler, br.transition_sampler, br.likelihood_logpdf, 64,
                samplers.stratified) is None
    assert pred(ts, br.fwd_sampler, plain, br.ref_sampler, br.transition_sampler, br.likelihood_logpdf, 64,
                samplers.stratified) is None
    assert pred(ts, other.fwd_sampler, br.unpack, br.ref_sampler, br.transition_sampler, br.likelihood_logpdf, 64,
                samplers.stratified) is None                                                                 # two bridges
    assert pred(ts, br.fwd_sampler, br.unpack, other.ref_sampler, br.transition_sampler, br.likelihood_logpdf, 64,
                samplers.stratified) is None
    assert pred(ts, br.fwd_ys_sampler, br.unpack, br.ref_sampler, br.transition_sampler, br.likelihood_logpdf, 64,
                samplers.stratified) is None                                                                 # wrong roles
    assert pred(ts, br.unpack, br.fwd_sampler, br.ref_sampler, br.transition_sampler, br.likelihood_logpdf, 64,
                samplers.stratified) is None
    assert pred(ts, br.fwd_sampler, br.unpack, br.ref_sampler, br.transition_sampler, br.transition_logpdf, 64,
                samplers.stratified) is None                                                                 # wrong weight
    assert pred(np.linspace(0, 1, 41), *_own(br), 64, samplers.stratified) is None                           # another grid
    assert pred(ts * 1.01, *_own(br), 64, samplers.stratified) is None
    assert pred(ts, *_own(br), 64, samplers.multinomial) is None
    lg = _bare_bridge(LinearGaussianBridge, ts, sde=StationaryConstLinearSDE(-0.5, 1.0))   # an LG bridge: no em_struct
    assert not hasattr(lg, "sb_filter_sampler_handle") and not hasattr(lg, "fused_sb_filter_sampler_supported")
    assert pred(ts, *_own(lg), 64, samplers.stratified) is None
    noem = _bare_bridge(GaussianSBBridge, ts)                                              # (and an SB bridge without one)
    assert pred(ts, *_own(noem), 64, samplers.stratified) is None
    wide = _bare_bridge(GaussianSBBridge, ts, du=128, dv=128, em=True)                     # D = 256, the engine's bound
    assert pred(ts, *_own(wide), 131072, samplers.stratified) == (wide, "stratified")
    assert pred(ts, *_own(wide), 131073, samplers.stratified) is None                      # the filter's bound
    assert pred(ts, *_own(_bare_bridge(GaussianSBBridge, ts, du=129, dv=128, em=True)), 64, samplers.stratified) is None


def test_the_chunk_planner_is_reused_unchanged(monkeypatch):
    """sb_filter_conditional_sampler plans its calls with samplers.smc.plan_filter_chunks, on (keys, N, du, _bound)."""
    from fbs_amd import samplers
    from fbs_amd.gaussian_sb import GaussianSBBridge
    from fbs_amd.samplers import smc
    assert smc.plan_filter_chunks(5, 64, 3, bound=2 * 64 * 3) == [(0, 2), (2, 4), (4, 5)]
    assert smc.plan_filter_chunks(5, 64, 3) == [(0, 5)] and smc.plan_filter_chunks(5, 64, 3, bound=64 * 3 - 1) is None
    seen = []

    class Planned(Exception):
        pass

    def spy(*a, **k):
        seen.append((a, k))
        raise Planned

    monkeypatch.setattr(smc, "plan_filter_chunks", spy)
    ts = np.linspace(0, 1, 31)
    br = _bare_bridge(GaussianSBBridge, ts, du=3, dv=3, em=True)
    keys = np.arange(10, dtype=np.uint32).reshape(5, 2)
    with pytest.raises(Planned):
        samplers.sb_filter_conditional_sampler(keys, np.zeros(3, np.float32), ts, *_own(br), 64, samplers.stratified,
                                               _bound=2 * 64 * 3)
    assert seen == [((5, 64, 3, 2 * 64 * 3), {})]


def test_restated_proper_x0_equals_mean_plus_z_chol():
    """The header's float32 chain (ascending c, separately rounded) against mean + z @ chol in float64, du = 5."""
    rng = np.random.default_rng(5)
    du = 5
    A = rng.normal(size=(du, du))
    chol = np.linalg.cholesky(A @ A.T / du + 0.5 * np.eye(du)).astype(np.float32)
    mean = rng.normal(size=du).astype(np.float32)
    for _ in range(4):
        z = rng.normal(size=du).astype(np.float32)
        got = R.x0_restated(z, mean, chol)
        ref = mean.astype(np.float64) + z.astype(np.float64) @ chol.astype(np.float64)
        assert got.dtype == np.float32 and got.shape == (du,)
        rel = np.abs(got.astype(np.float64) - ref) / np.abs(ref)
        print("relative error of the restated x0:", rel)
        assert np.all(rel <= 1e-6), rel


def test_sb_filter_conditional_sampler_signature():
    from fbs_amd import samplers
    from fbs_amd.samplers.smc import FSAMP_STATE_ELEMS
    sig = inspect.signature(samplers.sb_filter_conditional_sampler)
    assert list(sig.parameters) == ["keys", "y0", "ts", "fwd_sampler", "unpack", "ref_sampler", "transition_sampler",
                                    "likelihood_logpdf", "nparticles", "resampling", "x0_prior", "return_nell", "_bound"]
    assert sig.parameters["x0_prior"].default is None and sig.parameters["return_nell"].default is False
    assert sig.parameters["_bound"].default == FSAMP_STATE_ELEMS
    assert all(p.default is inspect.Parameter.empty for n, p in list(sig.parameters.items())[:10])


def test_the_loop_refuses_an_x0_of_unknown_size():
    """Foreign closures carry no du: without a prior the size of x0 is unknown, and nothing is drawn or launched."""
    from fbs_amd import samplers
    plain = lambda *a, **k: pytest.fail("nothing may be called")
    with pytest.raises(ValueError, match="x0_prior"):
        samplers.sb_filter_conditional_sampler(np.zeros((2, 2), np.uint32), np.zeros(3, np.float32), np.linspace(0, 1, 5),
                                               plain, plain, plain, plain, plain, 16, samplers.stratified)
