"""GPU: bootstrap_filter_batched, pmcmc_filter_step_batched, pmcmc_kernel_batched and gibbs_init_batched equal the loops of
their single-ensemble namesakes over the ensembles, bit for bit, with a score whose output row depends on its own input row
only; the lockstep paths call the network once per step for all ensembles; everything the lockstep paths do not take falls
back to the loop; the driver's --batch writes the sequential run's files for --method filter and pmcmc."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 4
N = 5
PMCMC_SEED = 0          # a seed at which one batch of three ensembles holds accepted and rejected proposals (asserted)
PMCMC_ITERS = 3


def _model(dev, chunk=7):
    from fbs_amd.images import ImageRestore
    from fbs_amd.score import ScoreBridge
    from fbs_amd.sdes import StationaryLinLinearSDE
    ts = np.linspace(0, 2.0, T + 1)
    sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=2.0)
    ds = ImageRestore("inpaint-3", (8, 8, 1), device=dev)
    calls = []

    def score_fn(x, t):                                  # row-wise: a row's output does not depend on its neighbours
        calls.append(int(x.shape[0]))
        return (0.25 * x.roll(1, 2) - 0.5 * x) * float(t)

    return ds, ScoreBridge(score_fn, ds, sde, ts, chunk=chunk), sde, ts, calls


def _inputs(oracle, dev, ds, sb, B, shared, seed=0):
    """keys, masks, y0s, observation paths in reverse time (B, T + 1, q, c); `shared`: one mask and one y0 for all."""
    from fbs_amd import ops
    keys = oracle.split(oracle.PRNGKey(1000 * seed + 41 + B), B)
    masks = [ds.gen_mask(oracle.PRNGKey(200 + (0 if shared else b))) for b in range(B)]
    if shared:
        masks = [masks[0]] * B
    y0s = [ds.unpack(ops.uniform(oracle.PRNGKey(300 + (0 if shared else b)), (8, 8, 1), device=dev), masks[b])[1]
           for b in range(B)]
    yss = torch.stack([sb.fwd_ys_sampler(oracle.PRNGKey(1000 * seed + 400 + b), y0s[b]) for b in range(B)], 0)
    return keys, masks, y0s, yss


def _bits_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), what


def _per_step(B, n=N, chunk=7):
    return -(-(B * n) // chunk)


def _resampler(name):
    from fbs_amd import samplers
    return getattr(samplers, name)


# ---------------------------------------------------------------------------------------------------
# bootstrap_filter_batched
# ---------------------------------------------------------------------------------------------------
def _filter_both(oracle, dev, B, shared, resampling, return_last, nparticles=N, chunk=7, closures=None):
    from fbs_amd.samplers import bootstrap_filter, bootstrap_filter_batched
    ds, sb, sde, ts, calls = _model(dev, chunk)
    keys, masks, y0s, yss = _inputs(oracle, dev, ds, sb, B, shared)
    vss = torch.flip(yss, [1])
    cl = closures(sb) if closures else (sb.transition_sampler, sb.likelihood_logpdf)
    loop = [bootstrap_filter(*cl, vss[b], ts, sb.ref_sampler, keys[b], nparticles, resampling, log=True,
                             return_last=return_last, mask_=masks[b]) for b in range(B)]
    del calls[:]
    got = bootstrap_filter_batched(*cl, vss, ts, sb.ref_sampler, keys, nparticles, resampling, log=True,
                                   return_last=return_last, mask_=masks[0] if shared else masks)
    torch.cuda.synchronize()
    want = (torch.stack([o[0] for o in loop], 0), torch.stack([o[1] for o in loop], 0))
    return got, want, list(calls)


@pytest.mark.parametrize("return_last", (True, False))
@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("rname", ("stratified", "systematic"))
@pytest.mark.parametrize("B", (3, 1))
def test_bootstrap_filter_lockstep_equals_the_loop(oracle, dev, B, rname, shared, return_last):
    got, want, calls = _filter_both(oracle, dev, B, shared, _resampler(rname), return_last)
    assert tuple(got[0].shape) == ((B, N, 9, 1) if return_last else (B, T + 1, N, 9, 1)) and tuple(got[1].shape) == (B,)
    _bits_equal(got[0], want[0], "samples")
    _bits_equal(got[1], want[1], "nell")
    assert torch.isfinite(got[1]).all()
    per_step = _per_step(B)
    assert len(calls) == T * per_step and sum(calls) == T * B * N, calls              # chunks straddle ensembles
    if B == 3:
        assert calls[:per_step] == [7, 7, 1]


# ---------------------------------------------------------------------------------------------------
# pmcmc_filter_step_batched, pmcmc_kernel_batched
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("rname", ("stratified", "systematic"))
@pytest.mark.parametrize("B", (3, 1))
def test_pmcmc_filter_step_lockstep_equals_the_loop(oracle, dev, B, rname, shared):
    from fbs_amd.samplers import pmcmc_filter_step_batched
    from fbs_amd.samplers.smc import pmcmc_filter_step
    ds, sb, sde, ts, calls = _model(dev)
    keys, masks, y0s, yss = _inputs(oracle, dev, ds, sb, B, shared)
    vss = torch.flip(yss, [1])
    u0s = torch.stack([sb.ref_sampler(oracle.PRNGKey(500 + b), None, N) for b in range(B)], 0)
    cl = (sb.transition_sampler, sb.likelihood_logpdf, _resampler(rname), N)
    loop = [pmcmc_filter_step(keys[b], vss[b], u0s[b], ts, *cl, mask_=masks[b]) for b in range(B)]
    del calls[:]
    us, log_ell = pmcmc_filter_step_batched(keys, vss, u0s, ts, *cl, mask_=masks[0] if shared else masks)
    torch.cuda.synchronize()
    assert tuple(us.shape) == (B, N, 9, 1) and tuple(log_ell.shape) == (B,)
    _bits_equal(us, torch.stack([o[0] for o in loop], 0), "us")
    _bits_equal(log_ell, torch.stack([o[1] for o in loop], 0), "log_ell")
    assert len(calls) == T * _per_step(B) and sum(calls) == T * B * N, calls          # one evaluation per step, not two


def _pmcmc_chains(oracle, dev, B, shared, rname, delta, seed, iters=PMCMC_ITERS, nparticles=N, chunk=7):
    """`iters` iterations of the driver's pMCMC loop, by the loop of pmcmc_kernel and by
    pmcmc_kernel_batched, compared after every iteration.  -> (is_accepted of the loop (iters, B), network calls)."""
    from fbs_amd.samplers import pmcmc_kernel, pmcmc_kernel_batched
    from fbs_amd.samplers.smc import pmcmc_filter_step
    ds, sb, sde, ts, calls = _model(dev, chunk)
    _, masks, y0s, yss = _inputs(oracle, dev, ds, sb, B, shared, seed)
    args = (ts, sb.fwd_ys_sampler, sde, sb.ref_sampler, sb.transition_sampler, sb.likelihood_logpdf, _resampler(rname),
            nparticles)
    # the chains start at the likelihood estimates of their initial observation paths (from the driver's log_ell = 0 no
    # proposal of this model is ever accepted)
    start = [pmcmc_filter_step(oracle.PRNGKey(1000 * seed + 600 + b), torch.flip(yss[b], [0]),
                               sb.ref_sampler(oracle.PRNGKey(1000 * seed + 700 + b), None, nparticles), *args[:1], *args[4:],
                               mask_=masks[b]) for b in range(B)]
    single = [(start[b][0][0], start[b][1], yss[b]) for b in range(B)]
    state = (torch.stack([s[0][0] for s in start], 0), torch.stack([s[1] for s in start], 0), yss)
    accepted, counts = [], []
    for i in range(iters):
        keys = oracle.split(oracle.PRNGKey(1000 * seed + 50 + i), B)
        loop = [pmcmc_kernel(keys[b], *single[b], y0s[b], *args, delta=delta, mask_=masks[b]) for b in range(B)]
        single = [o[:3] for o in loop]
        del calls[:]
        got = pmcmc_kernel_batched(keys, *state, y0s[0] if shared else y0s, *args, delta=delta,
                                   mask_=masks[0] if shared else masks)
        torch.cuda.synchronize()
        counts.append(list(calls))
        state = got[:3]
        for j, what in enumerate(("uT", "log_ell", "ys")):
            _bits_equal(got[j], torch.stack([torch.as_tensor(o[j], device=dev) for o in loop], 0), (what, i))
        for f in got[3]._fields:
            _bits_equal(getattr(got[3], f), torch.stack([getattr(o[3], f) for o in loop], 0), (f, i))
        assert got[3].is_accepted.dtype == torch.bool and tuple(got[3].is_accepted.shape) == (B,)
        accepted.append([bool(o[3].is_accepted) for o in loop])
    return np.array(accepted), counts


@pytest.mark.parametrize("delta", (None, 0.005))
@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("rname", ("stratified", "systematic"))
@pytest.mark.parametrize("B", (3, 1))
def test_pmcmc_kernel_lockstep_equals_the_loop(oracle, dev, B, rname, shared, delta):
    accepted, counts = _pmcmc_chains(oracle, dev, B, shared, rname, delta, PMCMC_SEED)
    print("is_accepted (iteration, ensemble):", accepted.astype(int).tolist())
    for calls in counts:
        assert len(calls) == T * _per_step(B) and sum(calls) == T * B * N, calls
    if B == 3:
        # accepted and rejected ensembles in ONE batch: the device-side select takes both branches in one call
        assert any(row.any() and not row.all() for row in accepted), accepted.tolist()


# ---------------------------------------------------------------------------------------------------
# gibbs_init_batched
# ---------------------------------------------------------------------------------------------------
def _init_both(oracle, dev, B, shared, method, marg_y=True, nparticles=N, chunk=7):
    from fbs_amd.samplers import gibbs_init, gibbs_init_batched
    ds, sb, sde, ts, calls = _model(dev, chunk)
    keys, masks, y0s, _ = _inputs(oracle, dev, ds, sb, B, shared)
    args = (ts, sb.fwd_sampler, sde, sb.unpack, sb.transition_sampler, sb.transition_logpdf, sb.likelihood_logpdf, nparticles)
    loop = [gibbs_init(keys[b], y0s[b], (9, 1), *args, method=method, marg_y=marg_y, mask_=masks[b]) for b in range(B)]
    del calls[:]
    got = gibbs_init_batched(keys, y0s[0] if shared else y0s, (9, 1), *args, method=method, marg_y=marg_y,
                             mask_=masks[0] if shared else masks)
    torch.cuda.synchronize()
    return got, loop, list(calls)


@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("method", ("filter", "smoother"))
@pytest.mark.parametrize("B", (3, 1))
def test_gibbs_init_lockstep_equals_the_loop(oracle, dev, B, method, shared):
    got, loop, calls = _init_both(oracle, dev, B, shared, method, marg_y=(method == "smoother"))
    assert tuple(got[0].shape) == (B, 9, 1) and tuple(got[1].shape) == (B, T + 1, 9, 1)
    _bits_equal(got[0], torch.stack([o[0] for o in loop], 0), "approx_x0")
    _bits_equal(got[1], torch.stack([o[1] for o in loop], 0), "approx_us_star")
    filter_calls = T * _per_step(B)
    assert calls[:filter_calls] == ([7, 7, 1] * T if B == 3 else [5] * T), calls      # the filter, in lockstep
    if method == "filter":
        assert len(calls) == filter_calls
    else:
        assert calls[filter_calls:] == [N] * (B * T)                                  # the backward smoother, per ensemble


def test_gibbs_init_debug_runs_the_loop(oracle, dev):
    got, loop, calls = _init_both(oracle, dev, 2, False, "debug")
    _bits_equal(got[0], torch.stack([o[0] for o in loop], 0), "approx_x0")
    assert got[1] is None and calls == [N] * (2 * T)


# ---------------------------------------------------------------------------------------------------
# fallbacks: the loop of the single function, one network call per ensemble and step
# ---------------------------------------------------------------------------------------------------
def test_fallback_multinomial(oracle, dev):
    from fbs_amd.samplers import multinomial
    got, want, calls = _filter_both(oracle, dev, 2, False, multinomial, True)
    _bits_equal(got[0], want[0], "samples")
    _bits_equal(got[1], want[1], "nell")
    assert calls == [N] * (2 * T)
    accepted, counts = _pmcmc_chains(oracle, dev, 2, False, "multinomial", None, 1, iters=1)
    assert counts == [[N] * (2 * T)]


def test_fallback_more_than_1024_particles(oracle, dev):
    from fbs_amd.samplers import stratified
    got, want, calls = _filter_both(oracle, dev, 2, False, stratified, True, nparticles=1025, chunk=2048)
    _bits_equal(got[0], want[0], "samples")
    _bits_equal(got[1], want[1], "nell")
    assert calls == [1025] * (2 * T)


def test_fallback_foreign_closure(oracle, dev):
    """A weight closure that is not the bridge's own method: the generic two-closure loop, per ensemble."""
    from fbs_amd.samplers import stratified

    def closures(sb):
        return sb.transition_sampler, (lambda v, us, v_prev, t_prev, **kw: sb.likelihood_logpdf(v, us, v_prev, t_prev, **kw))

    got, want, calls = _filter_both(oracle, dev, 2, False, stratified, True, closures=closures)
    _bits_equal(got[0], want[0], "samples")
    _bits_equal(got[1], want[1], "nell")
    assert calls == [N] * (2 * T)                        # the bridge shares one evaluation between the two closures


# ---------------------------------------------------------------------------------------------------
# a real network, the driver
# ---------------------------------------------------------------------------------------------------
def test_mnist_shaped_unet_run(oracle, dev):
    """Shapes and finiteness only: bit equality with the loop is not promised for library convolutions."""
    from fbs_amd import ops
    from fbs_amd.images import ImageRestore
    from fbs_amd.samplers import bootstrap_filter_batched, pmcmc_kernel_batched, stratified
    from fbs_amd.score import ScoreBridge
    from fbs_amd.sdes import StationaryLinLinearSDE
    from fbs_amd.unet import UNet
    torch.manual_seed(0)
    B, n, Tn = 2, 6, 3
    ts = np.linspace(0, 2.0, Tn + 1)
    sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=2.0)
    ds = ImageRestore("inpaint-15", (28, 28, 1), device=dev)
    net = UNet(dt=2.0 / 200, dim=8, in_channels=1, upsampling="pixel_shuffle").to(dev).eval()

    def score_fn(x, t):
        with torch.no_grad():
            return net(x, t).reshape(x.shape)

    sb = ScoreBridge(score_fn, ds, sde, ts, chunk=64)
    masks = [ds.gen_mask(oracle.PRNGKey(5 + b)) for b in range(B)]
    y0s = [ds.unpack(ops.uniform(oracle.PRNGKey(8 + b), (28, 28, 1), device=dev), masks[b])[1] for b in range(B)]
    yss = torch.stack([sb.fwd_ys_sampler(oracle.PRNGKey(11 + b), y0s[b]) for b in range(B)], 0)
    keys = oracle.split(oracle.PRNGKey(1), B)
    us, nell = bootstrap_filter_batched(sb.transition_sampler, sb.likelihood_logpdf, torch.flip(yss, [1]), ts, sb.ref_sampler,
                                        keys, n, stratified, mask_=masks)
    assert us.shape == (B, n, 225, 1) and nell.shape == (B,)
    assert torch.isfinite(us).all() and torch.isfinite(nell).all()
    uT, log_ell, ys, st = pmcmc_kernel_batched(keys, torch.zeros((B, 225, 1), device=dev), torch.zeros(B, device=dev), yss,
                                               y0s, ts, sb.fwd_ys_sampler, sde, sb.ref_sampler, sb.transition_sampler,
                                               sb.likelihood_logpdf, stratified, n, delta=0.005, mask_=masks)
    assert uT.shape == (B, 225, 1) and log_ell.shape == (B,) and ys.shape == yss.shape
    assert st.is_accepted.shape == (B,) and st.is_accepted.dtype == torch.bool
    assert torch.isfinite(uT).all() and torch.isfinite(log_ell).all() and torch.isfinite(ys).all()
    assert ((st.acceptance_prob >= 0) & (st.acceptance_prob <= 1)).all()


COMMON = ["--ny0s", "3", "--nsamples", "2", "--nparticles", "4", "--test_nsteps", "3", "--dim", "8", "--fp32", "--quiet"]


def _driver():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import imgs_restore
    return imgs_restore


@pytest.mark.parametrize("method", ("filter", "pmcmc-0.005"))
def test_driver_batch_writes_the_sequential_files(tmp_path, dev, method):
    imgs_restore = _driver()
    seq, bat = tmp_path / "seq", tmp_path / "bat"
    imgs_restore.main(COMMON + ["--method", method, "--outdir", str(seq)])
    out = imgs_restore.main(COMMON + ["--method", method, "--batch", "2", "--outdir", str(bat)])     # groups of 2 and 1
    assert out.shape == (2, 28, 28, 1) and np.isfinite(out).all()
    names = sorted(os.listdir(seq))
    assert sorted(os.listdir(bat)) == names
    assert [f for f in names if f.endswith(f"-{method}.npy")] == [f"mnist-inpaint-15-lin-4-{k}-{method}.npy" for k in range(3)]
    assert len(names) == 6
    for f in names:
        a, b = np.load(seq / f), np.load(bat / f)
        if f.endswith(".npz"):
            assert np.array_equal(a["test_img"], b["test_img"])                      # the same test images
        else:
            assert a.shape == b.shape == (2, 28, 28, 1) and np.isfinite(b).all(), f


def test_driver_batch_init_writes_the_same_file_set(tmp_path, dev):
    imgs_restore = _driver()
    seq, bat = tmp_path / "seq", tmp_path / "bat"
    args = COMMON + ["--method", "gibbs-eb-ef"]
    imgs_restore.main(args + ["--batch", "2", "--outdir", str(seq)])
    out = imgs_restore.main(args + ["--batch", "2", "--batch_init", "--outdir", str(bat)])
    assert out.shape == (2, 28, 28, 1) and np.isfinite(out).all()
    names = sorted(os.listdir(seq))
    assert sorted(os.listdir(bat)) == names and len(names) == 9
    for f in names:
        a, b = np.load(seq / f), np.load(bat / f)
        if f.endswith(".npz"):
            assert np.array_equal(a["test_img"], b["test_img"])
        else:
            assert a.shape == b.shape and np.isfinite(b).all(), f
