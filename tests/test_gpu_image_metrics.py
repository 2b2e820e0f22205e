"""GPU: fbs_amd.image_metrics (fbsmi_img_psnr_ssim_batched, fbsmi_chain_autocorr_batched) against the float64 restatements
of tests/imgmetrics_restate.py, and examples/imgs_restore.py --metrics.

Bounds (absolute).  SSIM 1e-10: the float64 cancellation in E[xx] - ux^2 is at most about 49 * 1.1e-16 * 0.25 ~ 1e-15, which
against C2 = 9e-4 is about 1e-12; the bound is 100 times that and five orders below the smallest formula mistake
(tests/test_image_metrics_host.py).  PSNR 1e-9 dB: a sum of at most 262 144 terms (256 x 256 x 4) has a relative error of at most 2.9e-11,
times 10 / ln 10 = 4.3: about 1.2e-10 dB.  Autocorrelation 1e-9: the inputs are random walks, far from the cancellation of a nearly constant
variable.  The restatements are pinned to the specification's formulas, not to skimage or numpyro.
"""
import os
import sys

import numpy as np
import pytest
import torch

import imgmetrics_restate as R

pytestmark = pytest.mark.gpu

SSIM_TOL, PSNR_TOL, AC_TOL = 1e-10, 1e-9, 1e-9


def _check_scores(got_p, got_s, want_p, want_s, what):
    inf = np.isposinf(want_p)
    assert np.array_equal(np.isposinf(got_p), inf), f"{what}: PSNR is +inf in other places than the restatement's"
    dp = np.max(np.abs(got_p[~inf] - want_p[~inf])) if (~inf).any() else 0.0
    ds = np.max(np.abs(got_s - want_s))
    print(f"{what}: max |PSNR difference| = {dp:.3g} dB, max |SSIM difference| = {ds:.3g}")
    assert np.isfinite(got_s).all()
    assert dp <= PSNR_TOL, f"{what}: PSNR off by {dp}"
    assert ds <= SSIM_TOL, f"{what}: SSIM off by {ds}"


@pytest.mark.parametrize("kind", R.IMAGE_KINDS)
@pytest.mark.parametrize("shape", R.IMAGE_SHAPES)
def test_psnr_ssim_against_the_restatement(shape, kind, dev):
    from fbs_amd.image_metrics import psnr_ssim
    for G, S in ((1, 1), (3, 5)):
        t, r = R.make_images(kind, G, S, shape)
        want_p, want_s = R.psnr_ssim(t, r, clip=True)
        psnr, ssim = psnr_ssim(torch.from_numpy(t).to(dev), torch.from_numpy(r).to(dev))
        assert psnr.shape == ssim.shape == (G, S) and psnr.dtype == ssim.dtype == torch.float64 and psnr.is_cuda
        psnr, ssim = psnr.cpu().numpy(), ssim.cpu().numpy()
        _check_scores(psnr, ssim, want_p, want_s, f"{kind} {shape} G = {G} S = {S}")
        if kind == "equal":
            assert np.all(ssim == 1.0) and np.all(np.isposinf(psnr))             # exactly
        if kind == "outside":
            assert ((r < 0) | (r > 1)).any()                                     # the clip had work to do
    # image (g, s) of the (3, 5) call has the bits of the same image scored alone
    for g in range(G):
        for s in range(S):
            p1, s1 = psnr_ssim(torch.from_numpy(t[g:g + 1]).to(dev), torch.from_numpy(r[g:g + 1, s:s + 1]).to(dev))
            assert p1.cpu().numpy().tobytes() == psnr[g, s].tobytes() and s1.cpu().numpy().tobytes() == ssim[g, s].tobytes()


def test_psnr_ssim_257_images_numpy_and_unclipped(dev):
    """G * S = 257 (more images than a workgroup has threads), numpy in and out, the one-image form, and clip = False."""
    from fbs_amd.image_metrics import psnr_ssim
    shape = (28, 28, 1)
    t, r = R.make_images("noisy", 257, 1, shape)
    want_p, want_s = R.psnr_ssim(t, r)
    psnr, ssim = psnr_ssim(t, r)
    assert isinstance(psnr, np.ndarray) and psnr.shape == (257, 1) and psnr.dtype == np.float64
    _check_scores(psnr, ssim, want_p, want_s, "noisy 257 x 1")
    p1, s1 = psnr_ssim(t[256], r[256])                                           # (H, W, C) and (S, H, W, C)
    assert p1.shape == (1,) and p1[0] == psnr[256, 0] and s1[0] == ssim[256, 0]
    t, r = R.make_images("outside", 2, 3, (8, 13, 3))
    want_p, want_s = R.psnr_ssim(t, r, clip=False)
    psnr, ssim = psnr_ssim(t, r, clip=False)
    _check_scores(psnr, ssim, want_p, want_s, "outside, not clipped")
    assert np.max(np.abs(want_s - R.psnr_ssim(t, r, clip=True)[1])) > 1e-3       # and the flag matters


@pytest.mark.parametrize("shape", R.CHAIN_SHAPES)
def test_chain_autocorrelation_against_the_restatement(shape, dev):
    from fbs_amd.image_metrics import chain_autocorrelation
    M, S, D, L = shape
    x = R.make_chains(M, S, D)
    want = np.stack([R.autocorr_direct(x[m], L) for m in range(M)], 0)
    want_best = np.stack([R.best_curve(want[m]) for m in range(M)], 0)
    ac, best = chain_autocorrelation(torch.from_numpy(x).to(dev), L)
    assert ac.shape == (M, L, D) and best.shape == (M, L) and ac.dtype == best.dtype == torch.float64
    ac, best = ac.cpu().numpy(), best.cpu().numpy()
    assert np.array_equal(np.isnan(ac), np.isnan(want)), "NaN in other places than the restatement's"
    assert np.array_equal(np.isnan(best), np.isnan(want_best))
    ok = ~np.isnan(want)
    da = np.max(np.abs(ac[ok] - want[ok])) if ok.any() else 0.0
    okb = ~np.isnan(want_best)
    db = np.max(np.abs(best[okb] - want_best[okb])) if okb.any() else 0.0
    print(f"autocorrelation {shape}: max |ac difference| = {da:.3g}, max |best difference| = {db:.3g}")
    assert da <= AC_TOL and db <= AC_TOL
    if D > 1:
        assert np.isnan(ac[:, :, 0]).all() and np.isnan(ac[:, :, D - 1]).all()   # the constant columns
    if M > 1:
        assert np.isnan(ac[-1]).all() and np.isnan(best[-1]).all()               # the all-constant chain
        assert not np.isnan(best[:-1]).any()
    for m in range(M):                                                           # chain m alone: the same bits
        a1, b1 = chain_autocorrelation(x[m], L)
        assert isinstance(a1, np.ndarray) and a1.shape == (L, D) and b1.shape == (L,)
        assert a1.tobytes() == ac[m].tobytes() and b1.tobytes() == best[m].tobytes()


def test_all_constant_single_chain(dev):
    from fbs_amd.image_metrics import chain_autocorrelation
    ac, best = chain_autocorrelation(np.full((1, 6, 70), 0.1, np.float32), 3)
    assert np.isnan(ac).all() and np.isnan(best).all()


DRIVER = ["--dim", "8", "--nparticles", "12", "--nsamples", "2", "--ny0s", "3", "--test_nsteps", "5", "--chunk", "8", "--fp32",
          "--quiet"]


@pytest.mark.parametrize("batch", (2, 1))
@pytest.mark.parametrize("method", ("gibbs-eb-ef", "csgm"))
def test_driver_metrics(method, batch, tmp_path, dev):
    """examples/imgs_restore.py --metrics at the sizes of tests/test_gpu_images_e2e.py: every <result>-metrics.npz equals
    the metrics of the saved .npy against the saved -true.npz; without the flag the same argv writes the same result files
    byte for byte and no metrics file."""
    from fbs_amd.image_metrics import chain_autocorrelation, psnr_ssim
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import imgs_restore
    argv = ["--task", "inpaint", "--rect_size", "15", "--method", method, "--batch", str(batch)] + DRIVER
    with_m, plain = tmp_path / "metrics", tmp_path / "plain"
    imgs_restore.main(argv + ["--metrics", "--outdir", str(with_m)])
    imgs_restore.main(argv + ["--outdir", str(plain)])
    names = sorted(os.listdir(plain))
    assert not any("metrics" in f for f in names)
    scored = [f[:-len(".npy")] for f in names if f.endswith(f"-{method}.npy")]
    assert len(scored) == 3
    assert sorted(os.listdir(with_m)) == sorted(names + [f + "-metrics.npz" for f in scored])
    for f in scored:
        head = f[:-len(method) - 1]
        block = np.load(with_m / (f + ".npy"))
        true = np.load(with_m / (head + "-true.npz"))["test_img"]
        z = np.load(with_m / (f + "-metrics.npz"))
        psnr, ssim = psnr_ssim(true, block)
        assert z["psnr"].shape == (2,) and z["psnr"].tobytes() == psnr.tobytes() and z["ssim"].tobytes() == ssim.tobytes()
        assert np.isfinite(z["psnr"]).all() and np.isfinite(z["ssim"]).all()
        if method == "csgm":
            assert sorted(z.files) == ["psnr", "ssim"]
        else:
            best = chain_autocorrelation(block.reshape(2, -1), 2)[1]
            assert sorted(z.files) == ["autocorr_best", "psnr", "ssim"]
            assert z["autocorr_best"].tobytes() == best.tobytes()
    # examples/tabulate_imgs.py on the same directory: the table and the curve are the means of what the driver wrote
    import tabulate_imgs
    table, curves = tabulate_imgs.main(["--outdir", str(with_m), "--task", "inpaint-15", "--nparticles", "12", "--ny0s", "3",
                                        "--methods", method, "--autocorr", "--max_lags", "2"])
    zs = [np.load(with_m / (f + "-metrics.npz")) for f in scored]
    for name in ("psnr", "ssim"):
        every = np.stack([z[name] for z in zs], 0)
        assert table[method]["n"] == 6
        assert np.allclose(table[method][name], (np.mean(every), np.std(every)), rtol=1e-13, atol=0)
    if method == "csgm":
        assert curves == {}
    else:
        want = np.mean(np.stack([z["autocorr_best"] for z in zs], 0), axis=0)
        assert curves[method].shape == (2,) and np.allclose(curves[method], want, rtol=1e-13, atol=0, equal_nan=True)
    arrays = [f for f in names if f.endswith(".npy")]
    same = all(open(with_m / f, "rb").read() == open(plain / f, "rb").read() for f in arrays)
    if not same:
        # the flag draws no key and touches no state of the samplers; two runs of one argv can still differ where the
        # network's own float32 convolutions are not reproducible run to run (tests/test_gpu_images_e2e.py).  Then a third,
        # plain run differs from the second as well; if it does not, the flag changed the results.
        again = tmp_path / "again"
        imgs_restore.main(argv + ["--outdir", str(again)])
        assert not all(open(again / f, "rb").read() == open(plain / f, "rb").read() for f in arrays), \
            "--metrics changed the result files although the network is reproducible"
    for f in names:                                                              # the keys: test images, masks, file set
        if f.endswith("-true.npz"):
            assert np.load(with_m / f)["test_img"].tobytes() == np.load(plain / f)["test_img"].tobytes()
