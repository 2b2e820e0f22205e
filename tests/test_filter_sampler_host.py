"""CPU: the host side of the fused bootstrap-filter conditional sampler -- the restated ref_sampler against the oracle, the
dispatch predicate of fbs_amd.samplers.filter_conditional_sampler and its chunk planner.  No device is touched."""
import numpy as np
import pytest

from helpers import toy_2d
import fsamp_restate as R


def _bare_bridge(cls, ts, du=1, dv=1, sde=None, em=False):
    """A bridge with what the dispatch predicate reads and no device behind it (the constructor needs a GPU)."""
    from fbs_amd.linear_gaussian import _Closure
    br = object.__new__(cls)
    br.du, br.dv, br.sde = du, dv, sde
    br.ts_np = np.asarray(ts, np.float64)
    br.T = br.ts_np.size - 1
    if em:
        br.em_struct = object()
    for role in ("fwd_ys_sampler", "ref_sampler", "transition_sampler", "likelihood_logpdf", "transition_logpdf"):
        setattr(br, role, _Closure(br, lambda *a, **k: pytest.fail("the predicate must not call a closure"), role))
    return br


def test_restated_ref_sampler_equals_the_oracle_at_du_dv_1(oracle):
    from fbs_amd.linear_gaussian import lg_pmcmc_tables
    from fbs_amd.sdes import StationaryConstLinearSDE
    from fbs_amd.sdes.linear import discretise_linear_sde_np
    toy, ts = toy_2d(), np.linspace(0, 2, 31)
    Ft, Qt = discretise_linear_sde_np(StationaryConstLinearSDE(-0.5, 1.0), ts[-1], ts[0])
    tab = lg_pmcmc_tables(Ft * toy["m0"], Ft ** 2 * toy["cov0"] + Qt * np.eye(2), 1)
    for i, key in enumerate(oracle.split(oracle.PRNGKey(12), 3)):
        yT = np.array([0.3 * i - 0.2], np.float32)
        for n in (1, 7, 64):
            got = R.ref_restated(oracle, tab, key, yT, n)
            ref = oracle.lg_ref_sampler(toy["m0"], toy["cov0"], (Ft, Qt), 1, key, yT, n)
            assert got.shape == ref.shape == (n, 1)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (i, n)


def test_filter_conditional_sampler_is_exported():
    from fbs_amd import samplers
    assert callable(samplers.filter_conditional_sampler)
    import inspect
    names = list(inspect.signature(samplers.filter_conditional_sampler).parameters)
    assert names[:10] == ["keys", "y0", "ts", "fwd_ys_sampler", "ref_sampler", "transition_sampler", "likelihood_logpdf",
                          "nparticles", "resampling", "return_nell"]


def test_dispatch_predicate_refuses_without_touching_a_device():
    from fbs_amd import samplers
    from fbs_amd.gaussian_sb import GaussianSBBridge
    from fbs_amd.linear_gaussian import LinearGaussianBridge
    from fbs_amd.samplers.smc import _fused_filter_sampler
    from fbs_amd.sdes import StationaryConstLinearSDE
    ts = np.linspace(0, 2, 31)
    sde = StationaryConstLinearSDE(-0.5, 1.0)
    br, other = _bare_bridge(LinearGaussianBridge, ts, sde=sde), _bare_bridge(LinearGaussianBridge, ts, sde=sde)
    own = lambda b: (b.fwd_ys_sampler, b.ref_sampler, b.transition_sampler, b.likelihood_logpdf)
    assert _fused_filter_sampler(ts, *own(br), 64, samplers.stratified) == (br, "stratified")
    assert _fused_filter_sampler(ts, *own(br), 64, samplers.systematic) == (br, "systematic")
    plain = lambda *a, **k: None
    assert _fused_filter_sampler(ts, plain, plain, plain, plain, 64, samplers.stratified) is None              # foreign closures
    assert _fused_filter_sampler(ts, plain, br.ref_sampler, br.transition_sampler, br.likelihood_logpdf, 64,
                                 samplers.stratified) is None
    assert _fused_filter_sampler(ts, other.fwd_ys_sampler, br.ref_sampler, br.transition_sampler, br.likelihood_logpdf, 64,
                                 samplers.stratified) is None                                                # two bridges
    assert _fused_filter_sampler(ts, br.ref_sampler, br.fwd_ys_sampler, br.transition_sampler, br.likelihood_logpdf, 64,
                                 samplers.stratified) is None                                                # wrong roles
    assert _fused_filter_sampler(ts, br.fwd_ys_sampler, br.ref_sampler, br.transition_sampler, br.transition_logpdf, 64,
                                 samplers.stratified) is None                                                # wrong weight
    assert _fused_filter_sampler(np.linspace(0, 2, 41), *own(br), 64, samplers.stratified) is None            # another grid
    assert _fused_filter_sampler(ts * 1.01, *own(br), 64, samplers.stratified) is None
    assert _fused_filter_sampler(ts, *own(br), 64, samplers.multinomial) is None
    sb = _bare_bridge(GaussianSBBridge, ts, em=True)                                   # Euler-Maruyama forward process
    assert _fused_filter_sampler(ts, *own(sb), 64, samplers.stratified) is None
    wide = _bare_bridge(LinearGaussianBridge, ts, du=20, dv=20, sde=sde)
    assert _fused_filter_sampler(ts, *own(wide), 131072, samplers.stratified) == (wide, "stratified")
    assert _fused_filter_sampler(ts, *own(wide), 131073, samplers.stratified) is None                         # the filter's bound


@pytest.mark.parametrize("B,N,du", [(1, 64, 1), (5000, 100, 100), (7, 131072, 128)])
def test_chunk_planner_covers_every_key_once_within_the_bound(B, N, du):
    from fbs_amd.samplers.smc import FSAMP_STATE_ELEMS, plan_filter_chunks
    assert FSAMP_STATE_ELEMS * 4 == 256 * 2 ** 20                                      # float32 elements of 256 MB
    chunks = plan_filter_chunks(B, N, du)
    assert [i for a, b in chunks for i in range(a, b)] == list(range(B))
    for a, b in chunks:
        assert 1 <= b - a <= 65535 and (b - a) * N * du * 4 <= 256 * 2 ** 20
    if B * N * du <= FSAMP_STATE_ELEMS:
        assert chunks == [(0, B)]
    assert plan_filter_chunks(B, N, du, bound=2 * N * du) == [(a, min(a + 2, B)) for a in range(0, B, 2)]
    assert plan_filter_chunks(B, N, du, bound=N * du - 1) is None                      # one sample alone does not fit
