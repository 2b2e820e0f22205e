"""CPU: the float64 restatements of the image metrics (tests/imgmetrics_restate.py) agree with each other and tell the
formula mistakes that matter apart; fbs_amd.image_metrics refuses unsupported shapes before it touches a device and finds
the result files of every method; the entry points are declared, bound and exported."""
import ctypes
import os
import re

import numpy as np
import pytest

import imgmetrics_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fbsmi_img_psnr_ssim_workspace_bytes", "fbsmi_img_psnr_ssim_batched", "fbsmi_chain_autocorr_batched")


@pytest.mark.parametrize("shape", R.IMAGE_SHAPES)
def test_ssim_forms_agree(shape):
    """uniform_filter plus crop against the explicit loop over windows: 1e-12 (measured: at most 1.2e-13)."""
    worst = 0.0
    for kind in R.IMAGE_KINDS:
        t, r = R.make_images(kind, 1, 1, shape)
        x, y = R.clip01(t[0]), R.clip01(r[0, 0])
        a, b = R.ssim_filter(x, y), R.ssim_windows(x, y)
        worst = max(worst, abs(a - b))
        if kind == "equal":
            assert a == 1.0 and np.isposinf(R.psnr(x, y))
    print(f"ssim forms {shape}: max |difference| = {worst:.3g}")
    assert worst <= 1e-12


@pytest.mark.parametrize("shape", R.CHAIN_SHAPES)
def test_autocorr_forms_agree(shape):
    """The FFT route against the direct sum: 1e-12 (measured: at most 2.7e-15), NaN in the same places."""
    M, S, D, L = shape
    x = R.make_chains(M, S, D)
    worst = 0.0
    for m in range(M):
        a, b = R.autocorr_fft(x[m], L), R.autocorr_direct(x[m], L)
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.array_equal(np.isnan(b).all(axis=0), R.constant_columns(x[m]))
        if (~np.isnan(b)).any():
            worst = max(worst, np.nanmax(np.abs(a - b)))
            assert np.allclose(b[0][~np.isnan(b[0])], 1.0, rtol=0, atol=1e-15)
        np.testing.assert_allclose(R.best_curve(a), R.best_curve(b), rtol=0, atol=1e-12, equal_nan=True)
    print(f"autocorrelation forms {shape}: max |difference| = {worst:.3g}")
    assert worst <= 1e-12
    if M > 1:
        assert np.isnan(R.best_curve(R.autocorr_direct(x[-1], L))).all()         # the all-constant chain


def test_restatement_discriminates_the_formula_mistakes():
    """On the 28 x 28 'noisy' input of the GPU test: population covariances move SSIM by more than 1e-4, a 5 x 5 window or
    no crop by more than 1e-3 -- orders above the GPU test's 1e-10."""
    t, r = R.make_images("noisy", 1, 1, (28, 28, 1))
    x, y = R.clip01(t[0]), R.clip01(r[0, 0])
    good = R.ssim_filter(x, y)
    pop, win5, nocrop = R.ssim_filter(x, y, sample_cov=False), R.ssim_filter(x, y, win=5), R.ssim_filter(x, y, crop=False)
    print(f"ssim {good:.6f}; population covariance {abs(pop - good):.3g}, 5x5 window {abs(win5 - good):.3g}, "
          f"no crop {abs(nocrop - good):.3g}")
    assert abs(pop - good) > 1e-4
    assert abs(win5 - good) > 1e-3
    assert abs(nocrop - good) > 1e-3


def test_unsupported_shapes_raise_before_any_launch():
    from fbs_amd.image_metrics import chain_autocorrelation, psnr_ssim
    z = lambda *s: np.zeros(s, np.float32)
    for t, r in ((z(1, 6, 8, 1), z(1, 2, 6, 8, 1)),                              # H < 7
                 (z(1, 8, 257, 1), z(1, 2, 8, 257, 1)),                          # W > 256
                 (z(1, 8, 8, 5), z(1, 2, 8, 8, 5)),                              # C = 5
                 (z(2, 8, 8, 1), z(3, 2, 8, 8, 1)),                              # G differs
                 (z(1, 8, 8, 1), z(1, 2, 8, 9, 1)),                              # W differs
                 (z(1, 8, 8, 1), z(1, 2, 8, 8, 3)),                              # C differs
                 (z(1, 8, 8, 1), z(2, 8, 8, 1)),                                 # restored without its sample axis
                 (z(8, 8), z(2, 8, 8))):
        with pytest.raises(ValueError):
            psnr_ssim(t, r)
    for x, L in ((z(1, 5, 3), 6), (z(1, 5, 3), 0), (z(5,), 2), (z(1, 1, 5, 3), 2)):   # L > S, L < 1, wrong rank
        with pytest.raises(ValueError):
            chain_autocorrelation(x, L)


def test_tabulate_images_finds_every_method_suffix(tmp_path, monkeypatch):
    """The file names are the driver's (examples/imgs_restore.py): every method's suffix, csgm and twisted included, with
    the scoring stubbed (no device)."""
    from fbs_amd import image_metrics as IM
    methods = {"filter": "-filter", "filter-marg": "-filter-marg", "gibbs": "-gibbs", "gibbs-eb": "-gibbs-eb",
               "gibbs-eb-ef": "-gibbs-eb-ef", "gibbs-eb-ef-marg": "-gibbs-eb-ef-marg", "pmcmc-0.005": "-pmcmc-0.005",
               "pmcmc-1": "-pmcmc-1.0", "pmcmc": "-pmcmc-None", "twisted": "-twisted", "csgm": "-csgm"}
    for m, suffix in methods.items():
        assert IM.method_suffix(m) == suffix
    with pytest.raises(ValueError):
        IM.method_suffix("lpips")
    ny0s, S, shape = 3, 2, (8, 8, 1)
    rng = np.random.default_rng(0)
    for k in range(ny0s):
        head = os.path.join(tmp_path, f"mnist-supr-4-lin-12-{k}")
        np.savez(head + "-true", test_img=rng.uniform(size=shape).astype(np.float32))
        for j, suffix in enumerate(methods.values()):
            np.save(head + suffix, np.full((S,) + shape, float(j), np.float32))
    calls = []

    def stub(true_imgs, restored, clip=True):
        calls.append((true_imgs.shape, restored.shape, clip))
        level = restored.reshape(restored.shape[0], restored.shape[1], -1)[:, :, 0].astype(np.float64)
        return level + np.arange(S), -level

    monkeypatch.setattr(IM, "psnr_ssim", stub)
    table = IM.tabulate_images(str(tmp_path), "mnist", "supr-4", "lin", 12, list(methods), ny0s)
    assert list(table) == list(methods)
    assert calls == [((ny0s,) + shape, (ny0s, S) + shape, True)] * len(methods)  # one call per method, all its images
    for j, m in enumerate(methods):
        assert table[m]["n"] == ny0s * S
        assert table[m]["psnr"] == (j + 0.5, 0.5) and table[m]["ssim"] == (-float(j), 0.0)
    with pytest.raises(FileNotFoundError):
        IM.tabulate_images(str(tmp_path), "mnist", "supr-4", "lin", 12, ["filter"], ny0s + 1)


def test_metric_symbols_declared_bound_and_exported():
    from fbs_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fbsmi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fbsmi_[a-z0-9_]+)\s*\(", text))
    L = ctypes.CDLL(_lib.build())
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/fbsmi.h"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(L, n), f"{n} is not exported"
    assert os.path.join(os.path.dirname(_lib.__file__), "csrc", "fbsmi_metrics.hip") in _lib._SRC
    lib = _lib.lib()
    assert lib.fbsmi_abi_version() == 1
    # argument checks come before any device call: they answer without a GPU
    assert lib.fbsmi_img_psnr_ssim_workspace_bytes(15, 28, 28, 1) == 15 * 2 * 8              # one band
    assert lib.fbsmi_img_psnr_ssim_workspace_bytes(1, 25, 256, 3) == 3 * 2 * 2 * 8           # two bands
    assert lib.fbsmi_img_psnr_ssim_workspace_bytes(1, 6, 28, 1) == 0
    assert lib.fbsmi_img_psnr_ssim_batched(None, None, 1, 1, 28, 28, 1, 1, None, None, None, None) == -1
    assert lib.fbsmi_chain_autocorr_batched(None, 1, 5, 3, 2, None, None, None) == -1
