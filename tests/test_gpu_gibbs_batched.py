"""GPU: gibbs_kernel_batched equals the loop of gibbs_kernel over the ensembles, bit for bit, with a score whose output
row depends on its own input row only; the lockstep path calls the network once per step for all ensembles; everything the
lockstep path does not take falls back to the loop; the driver's --batch writes the sequential run's files."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 4


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


def _inputs(oracle, dev, ds, B, nparticles):
    from fbs_amd import ops
    keys = oracle.split(oracle.PRNGKey(31 + B), B)
    masks = [ds.gen_mask(oracle.PRNGKey(200 + b)) for b in range(B)]
    y0s = [ds.unpack(ops.uniform(oracle.PRNGKey(300 + b), (8, 8, 1), device=dev), masks[b])[1] for b in range(B)]
    rng = np.random.default_rng(B)
    x0s = torch.from_numpy(rng.normal(size=(B, 9, 1)).astype(np.float32)).to(dev)
    us_stars = torch.from_numpy(rng.normal(size=(B, T + 1, 9, 1)).astype(np.float32)).to(dev)
    bs_stars = rng.integers(0, nparticles, (B, T + 1)).astype(np.int32)
    return keys, x0s, y0s, us_stars, bs_stars, masks


def _both(oracle, dev, B, nparticles, chunk=7, **flags):
    from fbs_amd.samplers import gibbs_kernel, gibbs_kernel_batched
    ds, sb, sde, ts, calls = _model(dev, chunk)
    keys, x0s, y0s, us_stars, bs_stars, masks = _inputs(oracle, dev, ds, B, nparticles)
    cl = (sb.transition_sampler, sb.transition_logpdf, sb.likelihood_logpdf)
    loop = [gibbs_kernel(keys[b], x0s[b], y0s[b], us_stars[b], bs_stars[b], ts, sb.fwd_sampler, sde, sb.unpack, nparticles,
                         *cl, mask_=masks[b], **flags) for b in range(B)]
    del calls[:]
    got = gibbs_kernel_batched(keys, x0s, y0s, us_stars, bs_stars, ts, sb.fwd_sampler, sde, sb.unpack, nparticles, *cl,
                               mask_=masks, **flags)
    torch.cuda.synchronize()
    return got, loop, list(calls)


def _assert_equal(got, loop, B):
    shapes = ((B, 9, 1), (B, T + 1, 9, 1), (B, T + 1), (B, T + 1))
    for g, shape, i, what in zip(got, shapes, range(4), ("x0", "us_star", "bs_star", "acc")):
        assert tuple(g.shape) == shape, what
        want = torch.stack([o[i] for o in loop], 0)
        assert g.dtype == want.dtype, what
        assert torch.equal(g.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), what


@pytest.mark.parametrize("explicit_final", (False, True))
@pytest.mark.parametrize("B", (3, 1))
def test_lockstep_equals_the_loop(oracle, dev, B, explicit_final):
    nparticles = 5
    got, loop, calls = _both(oracle, dev, B, nparticles, explicit_final=explicit_final)
    _assert_equal(got, loop, B)
    rows = nparticles + (1 if explicit_final else 0)
    per_step = -(-(B * rows) // 7)
    assert len(calls) == (T + (1 if explicit_final else 0)) * per_step, calls        # chunks straddle ensembles
    assert sum(calls) == (T + (1 if explicit_final else 0)) * B * rows
    if B == 3:
        assert calls[:per_step] == [7] * (per_step - 1) + [B * rows - 7 * (per_step - 1)]   # and leave a tail


def test_marg_y_and_one_shared_observation(oracle, dev):
    from fbs_amd.samplers import gibbs_kernel, gibbs_kernel_batched
    ds, sb, sde, ts, _ = _model(dev)
    B, nparticles = 2, 5
    keys, x0s, y0s, us_stars, bs_stars, masks = _inputs(oracle, dev, ds, B, nparticles)
    cl = (sb.transition_sampler, sb.transition_logpdf, sb.likelihood_logpdf)
    args = (ts, sb.fwd_sampler, sde, sb.unpack, nparticles) + cl
    loop = [gibbs_kernel(keys[b], x0s[b], y0s[0], None, bs_stars[b], *args, marg_y=True, mask_=masks[0]) for b in range(B)]
    got = gibbs_kernel_batched(keys, x0s, y0s[0], None, bs_stars, *args, marg_y=True, mask_=masks[0])   # one y0, one mask
    _assert_equal(got, loop, B)


def test_fallbacks_equal_the_loop(oracle, dev):
    """explicit_backward=False and more than 1024 rows per ensemble run the loop: same results, nothing refused."""
    got, loop, calls = _both(oracle, dev, 2, 5, explicit_backward=False)
    _assert_equal(got, loop, 2)
    got, loop, calls = _both(oracle, dev, 2, 1025, chunk=2048)
    _assert_equal(got, loop, 2)
    assert calls == [1025] * (2 * T)                                                 # one call per ensemble and step


def test_mnist_shaped_unet_run(oracle, dev):
    from fbs_amd import ops
    from fbs_amd.images import ImageRestore
    from fbs_amd.samplers import gibbs_kernel_batched
    from fbs_amd.score import ScoreBridge
    from fbs_amd.sdes import StationaryLinLinearSDE
    from fbs_amd.unet import UNet
    torch.manual_seed(0)
    B, N, Tn = 2, 6, 3
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
    x0s = torch.zeros((B, 225, 1), device=dev)
    out = gibbs_kernel_batched(oracle.split(oracle.PRNGKey(1), B), x0s, y0s, None, np.zeros((B, Tn + 1), np.int32), ts,
                               sb.fwd_sampler, sde, sb.unpack, N, sb.transition_sampler, sb.transition_logpdf,
                               sb.likelihood_logpdf, explicit_final=True, mask_=masks)
    x0n, usn, bsn, acc = out
    assert x0n.shape == (B, 225, 1) and usn.shape == (B, Tn + 1, 225, 1) and bsn.shape == (B, Tn + 1)
    assert acc.shape == (B, Tn + 1) and acc.dtype == torch.bool
    assert torch.isfinite(usn).all() and torch.isfinite(x0n).all()
    assert int(bsn.min()) >= 0 and int(bsn.max()) < N


def test_driver_batch_writes_the_sequential_files(tmp_path, dev):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import imgs_restore
    common = ["--ny0s", "3", "--nsamples", "2", "--nparticles", "4", "--test_nsteps", "3", "--dim", "8", "--fp32", "--quiet"]
    seq, bat = tmp_path / "seq", tmp_path / "bat"
    imgs_restore.main(common + ["--outdir", str(seq)])
    out = imgs_restore.main(common + ["--batch", "2", "--outdir", str(bat)])          # groups of 2 and 1
    assert out.shape == (2, 28, 28, 1) and np.isfinite(out).all()
    names = sorted(os.listdir(seq))
    assert sorted(os.listdir(bat)) == names
    results = [f for f in names if f.endswith("-gibbs-eb-ef.npy")]
    assert results == [f"mnist-inpaint-15-lin-4-{k}-gibbs-eb-ef.npy" for k in range(3)]
    inits_equal = True
    for f in names:
        a, b = np.load(seq / f), np.load(bat / f)
        if f.endswith(".npz"):
            assert np.array_equal(a["test_img"], b["test_img"])                      # the same test images
        else:
            assert a.shape == b.shape and np.isfinite(b).all(), f
        if f.endswith("-gibbs-init.npy"):
            inits_equal = inits_equal and np.array_equal(a, b)                        # per image, the sequential run's keys
    if not inits_equal:
        # gibbs_init runs per image with the sequential run's keys, so its draws are the sequential run's -- unless the
        # network's own convolutions are not reproducible run to run on this machine (tests/test_gpu_images_e2e.py)
        again = tmp_path / "again"
        imgs_restore.main(common + ["--outdir", str(again)])
        assert not all(np.array_equal(np.load(seq / f), np.load(again / f)) for f in names if f.endswith("-gibbs-init.npy")), \
            "--batch changed an image's gibbs_init although the network is reproducible"
