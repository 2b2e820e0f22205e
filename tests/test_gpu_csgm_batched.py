"""GPU: the image CSGM sampler batched over trajectories (fbsmi_em_csgm_step_batched, fbsmi_normal_batched,
fbs_amd.csgm.make_image_csgm_batched, examples/imgs_restore.py --method csgm --batch B).

Kernel level: each half of the step kernel against the composition the single sampler runs (ops.normal per trajectory,
F * y0 + sqrt(Q) * z, ds.concat; -sde.drift + dispersion^2 * unpack(net), fbsmi_em_update), bit for bit.  Shapes: (9, 9, 1)
inpaint-4 with 5 steps has an observed part of 65 elements (an odd draw: the padded last Threefry pair) and du = 16;
(9, 9, 1) inpaint-5 has du = 25, so the scan draw of 5 * 25 elements is odd too; (20, 20, 1) inpaint-5 has D = 400 > 256 (a
second, ragged round of the workgroup, dv = 375 > 256); (20, 20, 1) supr-2 has du = 300 > 256 (the update itself takes the
ragged round); (12, 12, 2) supr-2 is a scattered mask with two channels.  (ImageRestore's inpainting masks hide the
rectangle, so du = s^2 and dv is the rest: the two extra shapes put the odd scan draw and du > 256 where the kernel's
update half meets them.)

Sampler: conditional_sampler_batched against the stacked loop of make_image_csgm with a row-wise stand-in score, bit for
bit, and against a float64 replay of the recursion, per trajectory, with a score that couples the pixels of an image.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TEND = 2.0
SHAPES = {                      # name -> (task, image shape, steps)
    "odd-dv": ("inpaint-4", (9, 9, 1), 5),
    "odd-scan": ("inpaint-5", (9, 9, 1), 5),
    "two-rounds": ("inpaint-5", (20, 20, 1), 4),
    "du-over-256": ("supr-2", (20, 20, 1), 3),
    "scattered-2ch": ("supr-2", (12, 12, 2), 4),
}
BATCHES = [(1, 1), (3, 1), (3, 3)]                                  # (B, nmasks)


def _sde():
    from fbs_amd.sdes import StationaryLinLinearSDE
    return StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=TEND)


def _problem(oracle, dev, name, B, nmasks, seed=0):
    """The dataset, B masks (one object repeated when nmasks == 1), B observations and B keys."""
    from fbs_amd.images import ImageRestore
    task, shape, T = SHAPES[name]
    ds = ImageRestore(task, shape, device=dev)
    made = [ds.gen_mask(oracle.PRNGKey(60 + seed + b)) for b in range(nmasks)]
    if nmasks > 1:
        assert any(not torch.equal(made[0].unobs_inds_ravelled, m.unobs_inds_ravelled) for m in made[1:])
    masks = [made[b if nmasks > 1 else 0] for b in range(B)]
    rng = np.random.default_rng(11 + seed)
    imgs = torch.from_numpy(rng.uniform(size=(B,) + shape).astype(np.float32)).to(dev)
    y0s = [ds.unpack(imgs[b], masks[b])[1].contiguous() for b in range(B)]
    keys = np.asarray(oracle.split(oracle.PRNGKey(500 + seed), B), np.uint32).reshape(B, 2)
    return ds, masks, y0s, keys, np.linspace(0, TEND, T + 1)


def _bits(t):
    t = t.contiguous()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)).cpu().numpy()


def _launch(mb, u, net, coef, scan, ntot, noff, y, F, sq, est, img, u_new, B):
    from fbs_amd import _lib, ops
    from fbs_amd.score import _NET_DT
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    _lib.call("fbsmi_em_csgm_step_batched", mb.ref, u.data_ptr(), ptr(net), 0 if net is None else _NET_DT[net.dtype],
              coef["cx"], coef["cs"], coef["dt"], coef["c"], scan.data_ptr(), ntot, noff, ptr(y), F, sq, est.data_ptr(),
              0 if img is None else _NET_DT[img.dtype], ptr(img), B, ptr(u_new), ops._stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,nmasks", BATCHES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_step_kernel_against_the_single_sampler_composition(oracle, dev, name, B, nmasks):
    from fbs_amd import _lib, ops
    from fbs_amd.score import EMMask, EMMaskBatch
    from fbs_amd.sdes import make_linear_sde
    ds, masks, y0s, keys, ts = _problem(oracle, dev, name, B, nmasks)
    sde, T = _sde(), ts.size - 1
    shape = ds.image_shape
    mb = EMMaskBatch([EMMask(m, shape[2], dev) for m in (masks if nmasks > 1 else masks[:1])])
    assert mb.nmasks == nmasks
    du, dv, D = mb.du, mb.dv, mb.D
    x_shape = tuple(ds.unobs_shape)
    k, dt = T - 2, TEND / T                                        # a step in the middle: a non-zero noise offset
    s_ = TEND - float(ts[k])
    Fq, Q = (float(x) for x in make_linear_sde(sde)[0](s_, float(ts[0])))
    F32, sq32 = float(np.float32(Fq)), float(np.float32(math.sqrt(Q)))
    coef = dict(cx=-float(sde.drift(1.0, s_)), cs=float(sde.dispersion(s_)) ** 2, dt=float(np.float32(dt)),
                c=float(np.float32(float(sde.dispersion(s_)) * math.sqrt(dt))))
    scan_keys = np.asarray(oracle.split(oracle.PRNGKey(71), B), np.uint32).reshape(B, 2)
    est_keys = np.asarray(oracle.split(oracle.PRNGKey(72), B), np.uint32).reshape(B, 2)
    scan, est = ops.keys_to_device(scan_keys, dev), ops.keys_to_device(est_keys, dev)
    rng = np.random.default_rng(5)
    u = torch.from_numpy(rng.normal(size=(B, du)).astype(np.float32)).to(dev)
    y = torch.stack([v.reshape(-1) for v in y0s], 0).contiguous()
    net32 = torch.from_numpy(rng.normal(size=(B, D)).astype(np.float32)).to(dev)
    ntot, noff = T * du, k * du

    # references, computed once: the single sampler's own composition, trajectory by trajectory
    def v_hat(b):
        return Fq * y0s[b] + math.sqrt(Q) * ops.normal(est_keys[b], tuple(y0s[b].shape), device=dev)

    def updated(b, net):
        ub = u[b].reshape(x_shape)
        score_u = ds.unpack(net[b].reshape(shape).float(), masks[b])[0]
        f = (-sde.drift(ub, s_) + float(sde.dispersion(s_)) ** 2 * score_u).to(torch.float32).contiguous()
        out = torch.empty_like(ub)
        _lib.call("fbsmi_em_update", ub.data_ptr(), f.data_ptr(), coef["dt"], coef["c"], int(scan_keys[b][0]),
                  int(scan_keys[b][1]), ntot, noff, du, out.data_ptr(), ops._stream())
        return out

    vh = [v_hat(b) for b in range(B)]
    want_cat = torch.stack([ds.concat(u[b].reshape(x_shape), vh[b], masks[b]) for b in range(B)], 0).reshape(B, D)

    # the concat half alone: float32 and bfloat16 (round to nearest even: torch's conversion)
    for dtype in (torch.float32, torch.bfloat16):
        img = torch.full((B, D), float("nan"), dtype=dtype, device=dev)
        _launch(mb, u, None, coef, scan, ntot, noff, y, F32, sq32, est, img, None, B)
        assert np.array_equal(_bits(img), _bits(want_cat.to(dtype))), f"concat half, {dtype}"

    for net in (net32, net32.to(torch.bfloat16)):
        want_u = torch.stack([updated(b, net) for b in range(B)], 0).reshape(B, du)
        want_both = torch.stack([ds.concat(want_u[b].reshape(x_shape), vh[b], masks[b]) for b in range(B)], 0).reshape(B, D)
        tag = f"net {net.dtype}"
        # the update half alone
        u_new = torch.full((B, du), float("nan"), device=dev)
        _launch(mb, u, net, coef, scan, ntot, noff, y, F32, sq32, est, None, u_new, B)
        assert np.array_equal(_bits(u_new), _bits(want_u)), f"update half, {tag}"
        # both halves in one launch, out of place and in place
        for dtype in (torch.float32, torch.bfloat16):
            img = torch.full((B, D), float("nan"), dtype=dtype, device=dev)
            u_new = torch.full((B, du), float("nan"), device=dev)
            _launch(mb, u, net, coef, scan, ntot, noff, y, F32, sq32, est, img, u_new, B)
            assert np.array_equal(_bits(u_new), _bits(want_u)), f"both halves, u_new, {tag}"
            assert np.array_equal(_bits(img), _bits(want_both.to(dtype))), f"both halves, img {dtype}, {tag}"
            u_io = u.clone()
            img.fill_(float("nan"))
            _launch(mb, u_io, net, coef, scan, ntot, noff, y, F32, sq32, est, img, u_io, B)
            assert np.array_equal(_bits(u_io), _bits(want_u)), f"in place, u, {tag}"
            assert np.array_equal(_bits(img), _bits(want_both.to(dtype))), f"in place, img {dtype}, {tag}"


@pytest.mark.parametrize("n", [1, 2, 65, 375, 1031])
def test_normal_batched_rows_are_single_draws(oracle, dev, n):
    """Odd and even n, one element, more than one workgroup per row (1031: 516 pairs over three workgroups)."""
    from fbs_amd import _lib, ops
    B = 3
    keys = np.asarray(oracle.split(oracle.PRNGKey(90 + n), B), np.uint32).reshape(B, 2)
    out = torch.full((B, n), float("nan"), device=dev)
    _lib.call("fbsmi_normal_batched", ops.keys_to_device(keys, dev).data_ptr(), B, n, out.data_ptr(), ops._stream())
    want = torch.stack([ops.normal(keys[b], (n,), device=dev) for b in range(B)], 0)
    assert np.array_equal(_bits(out), _bits(want))


def _rowwise_score(calls):
    def score(x, t):
        calls.append(int(x.shape[0]))
        return (0.25 * x.roll(1, 2) - 0.5 * x) * float(t)
    return score


@pytest.mark.parametrize("B,nmasks", BATCHES)
@pytest.mark.parametrize("name", ["odd-dv", "scattered-2ch"])
def test_batched_sampler_equals_the_stacked_loop(oracle, dev, name, B, nmasks):
    """chunk = 2: B = 3 is a two-row call and a one-row tail per step, B = 1 one one-row call."""
    from fbs_amd.csgm import make_image_csgm, make_image_csgm_batched
    ds, masks, y0s, keys, ts = _problem(oracle, dev, name, B, nmasks, seed=1)
    sde, T = _sde(), ts.size - 1
    calls, loop_calls = [], []
    batched = make_image_csgm_batched(_rowwise_score(calls), ds, sde, ts, chunk=2)
    single = make_image_csgm(_rowwise_score(loop_calls), ds, sde, ts)
    want = torch.stack([single(keys[b], y0s[b], masks[b]) for b in range(B)], 0)
    got = batched(keys, y0s, masks if nmasks > 1 else masks[0])
    assert got.shape == (B,) + tuple(ds.unobs_shape) and torch.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(want))
    assert calls == ([2, 1] if B == 3 else [1]) * T                # nsteps * ceil(B / chunk) calls, the right rows
    assert loop_calls == [1] * (B * T)
    # the observations stacked, and a list of B masks that are one object: the same trajectories
    again = batched(keys, torch.stack(y0s, 0), masks)
    assert np.array_equal(_bits(again), _bits(want))
    if B > 1:                                                      # distinct keys, distinct trajectories
        assert not torch.equal(got[0], got[1])


def test_batched_sampler_float64_replay(oracle, dev):
    """The replay of test_image_csgm_sampler_closed_form (tests/test_gpu_images_e2e.py), per trajectory and independent of
    the single sampler: s(x, t) = -c x + g mean over the image's own pixels, so a row's score needs its whole image but
    no other row; B = 3, a mask and an observation per trajectory, (12, 12, 2) inpaint-5, 9 steps."""
    from fbs_amd.csgm import make_image_csgm_batched
    from fbs_amd.images import ImageRestore
    from fbs_amd.sdes import make_linear_sde
    T, c, g, B = 9, 0.6, 0.8, 3
    ts = np.linspace(0, TEND, T + 1)
    dt = TEND / T
    sde = _sde()
    ds = ImageRestore("inpaint-5", (12, 12, 2), device=dev)
    masks = [ds.gen_mask(oracle.PRNGKey(4 + b)) for b in range(B)]
    imgs = torch.from_numpy(np.random.default_rng(1).uniform(size=(B, 12, 12, 2)).astype(np.float32)).to(dev)
    y0s = [ds.unpack(imgs[b], masks[b])[1] for b in range(B)]
    keys = np.asarray(oracle.split(oracle.PRNGKey(21), B), np.uint32).reshape(B, 2)
    sampler = make_image_csgm_batched(lambda x, t: -c * x + g * x.mean(dim=(1, 2, 3), keepdim=True), ds, sde, ts)
    got = sampler(keys, y0s, masks)
    assert got.shape == (B,) + tuple(ds.unobs_shape)
    discretise = make_linear_sde(sde)[0]
    for b in range(B):
        y = y0s[b].cpu().numpy().astype(np.float64)
        key_init, key_sde = oracle.split(keys[b], 2)
        u = oracle.normal(key_init, tuple(ds.unobs_shape)).astype(np.float64)
        key_scan, key_est = oracle.split(key_sde, 2)
        key_ests = oracle.split(key_est, T)
        rnds = oracle.normal(key_scan, (T,) + tuple(ds.unobs_shape)).astype(np.float64)
        for k in range(T):
            s_ = TEND - ts[k]
            beta = sde.beta(s_)
            F, Q = (float(x) for x in discretise(s_, 0.0))
            v_hat = F * y + math.sqrt(Q) * oracle.normal(key_ests[k], y.shape).astype(np.float64)
            mean = (u.sum() + v_hat.sum()) / (u.size + v_hat.size)
            u = u + (0.5 * beta * u + beta * (-c * u + g * mean)) * dt + math.sqrt(beta) * math.sqrt(dt) * rnds[k]
        np.testing.assert_allclose(got[b].cpu().numpy(), u, rtol=5e-5, atol=5e-5, err_msg=f"trajectory {b}")


def test_driver_batch_writes_the_sequential_files(tmp_path, dev):
    """examples/imgs_restore.py --method csgm --batch 3: four trajectories (two images, two samples) in groups of 3 and 1;
    the file names and array shapes of --batch 1, all finite.  (No bit equality with a real UNet: its library kernels may
    be chosen by batch size.)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import imgs_restore
    shapes = {}
    for batch in (1, 3):
        out_dir = tmp_path / f"batch{batch}"
        out = imgs_restore.main(["--method", "csgm", "--batch", str(batch), "--nsamples", "2", "--ny0s", "2", "--test_nsteps", "5",
                                 "--dim", "8", "--fp32", "--quiet", "--outdir", str(out_dir)])
        assert out.shape == (2, 28, 28, 1) and np.isfinite(out).all()
        shapes[batch] = {}
        for f in sorted(os.listdir(out_dir)):
            a = np.load(os.path.join(out_dir, f))
            a = a["test_img"] if f.endswith(".npz") else a
            assert np.isfinite(a).all(), f
            shapes[batch][f] = a.shape
    assert shapes[3] == shapes[1]
    assert sum(f.endswith("-csgm.npy") for f in shapes[3]) == 2 and sum(f.endswith("-true.npz") for f in shapes[3]) == 2
    assert all(s == (2, 28, 28, 1) for f, s in shapes[3].items() if f.endswith("-csgm.npy"))
