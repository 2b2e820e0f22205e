"""Float64 numpy restatements of the image metrics (include/fbsmi.h, "image metrics"), each in two independent forms, and
the inputs the host and GPU tests share.  A helper, not a test file.

The restatements are pinned to the formulas of the specification -- the ones skimage.metrics.structural_similarity /
peak_signal_noise_ratio and numpyro.diagnostics.autocorrelation document -- not to those packages, which are not
dependencies.
"""
import numpy as np
from scipy import ndimage
from scipy.fft import irfft, next_fast_len, rfft

C1, C2 = 0.01 ** 2, 0.03 ** 2


def clip01(a):
    return np.clip(np.asarray(a, np.float64), 0.0, 1.0)


def psnr(x, y):
    """x, y (H, W, C) float64; data range 1."""
    mse = np.mean((x - y) ** 2, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(1.0 / mse)


def ssim_filter(x, y, win=7, sample_cov=True, crop=True):
    """Form 1: window means by scipy.ndimage.uniform_filter per channel, then the crop by win // 2.  sample_cov = False
    (population covariances), win = 5 and crop = False are the mistakes the host test tells apart from the specification."""
    n = win * win
    norm = n / (n - 1.0) if sample_cov else 1.0
    pad = win // 2
    out = []
    for c in range(x.shape[-1]):
        a, b = x[..., c], y[..., c]
        f = lambda z: ndimage.uniform_filter(z, size=win)
        ux, uy = f(a), f(b)
        vx, vy, vxy = norm * (f(a * a) - ux * ux), norm * (f(b * b) - uy * uy), norm * (f(a * b) - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        out.append(np.mean(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad] if crop else S, dtype=np.float64))
    return float(np.mean(out))


def ssim_windows(x, y, win=7):
    """Form 2: an explicit loop over the windows that lie inside the image, np.mean / np.var(ddof=1) of each."""
    H, W, C = x.shape
    out = []
    for c in range(C):
        tot = 0.0
        for i in range(H - win + 1):
            for j in range(W - win + 1):
                a, b = x[i:i + win, j:j + win, c].ravel(), y[i:i + win, j:j + win, c].ravel()
                ux, uy = a.mean(), b.mean()
                vx, vy = a.var(ddof=1), b.var(ddof=1)
                vxy = np.sum((a - ux) * (b - uy)) / (a.size - 1)
                tot += ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        out.append(tot / ((H - win + 1) * (W - win + 1)))
    return float(np.mean(out))


def psnr_ssim(true_imgs, restored, clip=True, ssim=ssim_filter):
    """true_imgs (G, H, W, C), restored (G, S, H, W, C) -> psnr, ssim (G, S) float64."""
    prep = clip01 if clip else (lambda a: np.asarray(a, np.float64))
    t, r = prep(true_imgs), prep(restored)
    G, S = r.shape[:2]
    p, s = np.zeros((G, S)), np.zeros((G, S))
    for g in range(G):
        for k in range(S):
            p[g, k], s[g, k] = psnr(t[g], r[g, k]), ssim(t[g], r[g, k])
    return p, s


def constant_columns(x):
    """x (S, D) float32: the variables whose samples all have the same bits."""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.all(bits == bits[0], axis=0)


def autocorr_fft(x, L):
    """Form 1: the FFT route (zero-padded to twice a fast length, the power spectrum back-transformed, divided by the number
    of terms of every lag and by lag 0), then the constant rule, which replaces the route's rounding-noise 0 / 0."""
    x = np.asarray(x, np.float32)
    S = x.shape[0]
    c = x.astype(np.float64) - x.astype(np.float64).mean(axis=0)
    n2 = 2 * next_fast_len(S)
    f = rfft(c, n=n2, axis=0)
    ac = irfft(f * np.conj(f), n=n2, axis=0)[:S]
    with np.errstate(divide="ignore", invalid="ignore"):
        ac = ac / np.arange(S, 0, -1.0)[:, None]
        ac = ac / ac[:1]
    ac = ac[:L]
    ac[:, constant_columns(x)] = np.nan
    return ac


def autocorr_direct(x, L):
    """Form 2: the direct sum of the specification, a variable at a time."""
    x = np.asarray(x, np.float32)
    S, D = x.shape
    const = constant_columns(x)
    ac = np.full((L, D), np.nan)
    for d in range(D):
        if const[d]:
            continue
        c = x[:, d].astype(np.float64)
        c = c - c.sum() / S
        var = np.sum(c * c) / S
        for k in range(L):
            ac[k, d] = (np.sum(c[:S - k] * c[k:]) / (S - k)) / var
    return ac


def best_curve(ac):
    """ac (L, D) -> (L,): min over the non-NaN variables of max(ac, 0); NaN where there is none."""
    pos = np.where(np.isnan(ac), np.nan, np.maximum(ac, 0.0))
    out = np.full(ac.shape[0], np.nan)
    some = ~np.all(np.isnan(pos), axis=1)
    out[some] = np.nanmin(pos[some], axis=1)
    return out


# ---- shared inputs ----

IMAGE_KINDS = ("noisy", "flat", "outside", "equal")
# (H, W, C): one window; a row of windows; odd with three channels; MNIST; past a wave and no multiple of it; the extreme
# aspect ratios; then both sides of the band edge, which depends on the width (a staged plane holds 6144 // W rows): at
# W = 256 one band up to H = 24, at W = 96 up to H = 64; then the largest plane (14 bands, the LDS maximum of 58 KiB); one
# band of 250 window rows with exactly 6144 staged floats, 10 segments of 25 rows (the longest running-sum drift); four
# channels, one segment and 127 idle threads; the 64 x 64 x 3 configuration
IMAGE_SHAPES = ((7, 7, 1), (7, 9, 1), (8, 13, 3), (28, 28, 1), (33, 65, 3), (256, 7, 1), (7, 256, 2),
                (24, 256, 1), (25, 256, 1), (64, 96, 1), (65, 96, 1),
                (256, 256, 1), (256, 24, 1), (40, 129, 4), (64, 64, 3))


def make_images(kind, G, S, shape, seed=0):
    """true_imgs (G, H, W, C) and restored (G, S, H, W, C), float32."""
    H, W, C = shape
    rng = np.random.default_rng([seed, G, S, H, W, C, IMAGE_KINDS.index(kind)])
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    phase = rng.uniform(0, 2 * np.pi, (G, 1, 1, C))
    smooth = 0.5 + 0.35 * np.sin(0.2 * i[None, :, :, None] + phase) * np.cos(0.13 * j[None, :, :, None] + 0.5 * phase)
    if kind == "noisy":                                              # smooth plus noise of about the window's contrast:
        t = smooth                                                   # there the covariance normalisation shows in SSIM
        r = t[:, None] + 0.05 * rng.normal(size=(G, S, H, W, C))
    elif kind == "flat":                                             # 0.5 +- 1e-3 against exactly 0.5: the cancellation case
        t = np.full((G, H, W, C), 0.5)
        r = 0.5 + rng.uniform(-1e-3, 1e-3, (G, S, H, W, C))
    elif kind == "outside":                                          # values outside [0, 1] before the clip
        t = 2.0 * smooth - 0.5
        r = t[:, None] + 0.3 * rng.normal(size=(G, S, H, W, C))
    else:                                                            # equal images
        t = smooth + 0.1 * rng.normal(size=(G, H, W, C))
        r = np.repeat(t[:, None], S, axis=1)
    return np.ascontiguousarray(t, np.float32), np.ascontiguousarray(r, np.float32)


# (M, S, D, L)
CHAIN_SHAPES = ((1, 2, 1, 2), (1, 5, 4, 5), (3, 100, 37, 20), (2, 21, 130, 20), (1, 100, 784, 20))


def make_chains(M, S, D, seed=0):
    """chains (M, S, D) float32: cumulative sums of normals (every non-constant variable moves by far more than 1e-3 of its
    level); constant columns at d = 0, d = D - 1 and on both sides of every wave and workgroup boundary there is (D > 1);
    with M > 1 the last chain has every column constant."""
    rng = np.random.default_rng([seed, M, S, D])
    x = np.cumsum(rng.normal(size=(M, S, D)), axis=1).astype(np.float32)
    if D > 1:
        for d in (0, D - 1, 63, 64, 255, 256):
            if d < D:
                x[:, :, d] = x[:, :1, d]
    if M > 1:
        x[-1] = x[-1, :1]
    return x
