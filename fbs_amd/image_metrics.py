"""Image-quality metrics on the device: the evaluation side of the image tier (the paper's Tables 2 and 3, Figure 8).

``psnr_ssim`` scores a whole block of restored images against their true images in one launch pair and
``chain_autocorrelation`` gives the per-pixel autocorrelation of Gibbs / pMCMC image chains with the "best variable" curve
(include/fbsmi.h, "image metrics": the arithmetic is specified there, in float64).  ``tabulate_images`` reads the files
examples/imgs_restore.py writes and prints what the reference's experiments/tabulators/tabulate_imgs.py prints, without
LPIPS.  The toy tier's host statistics are fbs_amd/metrics.py.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib

MIN_SIDE, MAX_SIDE, MAX_CHANNELS = 7, 256, 4
CHAIN_METHODS = ("gibbs", "pmcmc")


def _device_f32(x, dev=None) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if not x.is_cuda:
        x = x.to(dev if dev is not None else torch.device("cuda:0"))
    return x.to(torch.float32).contiguous()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def psnr_ssim(true_imgs, restored, clip: bool = True):
    """PSNR (dB) and SSIM of restored (G, S, H, W, C) against true_imgs (G, H, W, C), both (G, S) float64, with data range 1:
    what skimage's peak_signal_noise_ratio and structural_similarity (7x7 uniform window, sample covariances, crop by 3)
    are asked for in the reference's tabulator.  clip first maps both images into [0, 1] (``normalise(method='clip')``).
    One true image (H, W, C) with restored (S, H, W, C) gives (S,).  7 <= H, W <= 256 and 1 <= C <= 4, else ValueError.
    Torch tensors give device tensors; numpy arrays are moved to the device and give numpy arrays."""
    ts, rs = tuple(true_imgs.shape), tuple(restored.shape)
    single = len(ts) == 3
    if single:
        ts, rs = (1,) + ts, (1,) + rs
    if len(ts) != 4 or len(rs) != 5:
        raise ValueError(f"psnr_ssim wants true_imgs (G, H, W, C) and restored (G, S, H, W, C), got {ts} and {rs}")
    G, H, W, Cn = ts
    S = rs[1]
    if rs[0] != G or rs[2:] != (H, W, Cn):
        raise ValueError(f"psnr_ssim: restored {rs} does not match true_imgs {ts}")
    if not (MIN_SIDE <= H <= MAX_SIDE and MIN_SIDE <= W <= MAX_SIDE and 1 <= Cn <= MAX_CHANNELS):
        raise ValueError(f"psnr_ssim supports 7 <= H, W <= 256 and 1 <= C <= 4, got H = {H}, W = {W}, C = {Cn}")
    if G < 1 or S < 1:
        raise ValueError("psnr_ssim needs at least one image")
    as_numpy = isinstance(restored, np.ndarray)
    r = _device_f32(restored, true_imgs.device if isinstance(true_imgs, torch.Tensor) and true_imgs.is_cuda else None)
    t = _device_f32(true_imgs, r.device)
    with torch.cuda.device(r.device):
        psnr = torch.empty((G, S), dtype=torch.float64, device=r.device)
        ssim = torch.empty((G, S), dtype=torch.float64, device=r.device)
        nbytes = _lib.lib().fbsmi_img_psnr_ssim_workspace_bytes(G * S, H, W, Cn)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=r.device)
        _lib.call("fbsmi_img_psnr_ssim_batched", t.data_ptr(), r.data_ptr(), G, S, H, W, Cn, 1 if clip else 0,
                  psnr.data_ptr(), ssim.data_ptr(), ws.data_ptr(), _stream())
    if single:
        psnr, ssim = psnr[0], ssim[0]
    if as_numpy:
        return psnr.cpu().numpy(), ssim.cpu().numpy()
    return psnr, ssim


def chain_autocorrelation(chains, max_lags: int):
    """Autocorrelation of every variable of chains (M, S, D) at lags 0 .. max_lags - 1: ac (M, max_lags, D) and the best
    variable's curve best (M, max_lags) = min over the variables of max(ac, 0), both float64.  The estimator is the
    unbiased one of numpyro.diagnostics.autocorrelation, as a direct sum.  A variable whose samples are all equal (an
    observed pixel) has NaN at every lag and is left out of best.  One chain (S, D) gives (max_lags, D) and (max_lags,).
    1 <= max_lags <= S, else ValueError."""
    cs = tuple(chains.shape)
    single = len(cs) == 2
    if single:
        cs = (1,) + cs
    if len(cs) != 3:
        raise ValueError(f"chain_autocorrelation wants chains (M, S, D), got {tuple(chains.shape)}")
    M, S, D = cs
    L = int(max_lags)
    if M < 1 or S < 1 or D < 1:
        raise ValueError(f"chain_autocorrelation: empty chains {cs}")
    if not 1 <= L <= S:
        raise ValueError(f"chain_autocorrelation needs 1 <= max_lags <= S = {S}, got {max_lags}")
    if M > 65535:
        raise ValueError("chain_autocorrelation takes at most 65535 chains a call")
    as_numpy = isinstance(chains, np.ndarray)
    x = _device_f32(chains)
    with torch.cuda.device(x.device):
        ac = torch.empty((M, L, D), dtype=torch.float64, device=x.device)
        best = torch.empty((M, L), dtype=torch.float64, device=x.device)
        _lib.call("fbsmi_chain_autocorr_batched", x.data_ptr(), M, S, D, L, ac.data_ptr(), best.data_ptr(), _stream())
    if single:
        ac, best = ac[0], best[0]
    if as_numpy:
        return ac.cpu().numpy(), best.cpu().numpy()
    return ac, best


def method_suffix(method: str) -> str:
    """The suffix examples/imgs_restore.py gives the result file of a method, as named on its command line plus '-marg'
    where --marg was set: 'filter[-marg]', 'gibbs[-eb][-ef][-marg]', 'pmcmc[-<delta>]' (written with the float's repr:
    'pmcmc-1' is saved as '-pmcmc-1.0', plain 'pmcmc' as '-pmcmc-None'), 'twisted', 'csgm'."""
    parts = method.split("-")
    if parts[0] == "pmcmc":
        return f"-pmcmc-{float(parts[-1]) if len(parts) > 1 else None}"
    if parts[0] == "gibbs":
        return "-gibbs" + "".join(f"-{flag}" for flag in ("eb", "ef", "marg") if flag in parts[1:])
    if parts[0] in ("filter", "twisted", "csgm"):
        return "-" + method
    raise ValueError(f"Unknown method {method}")


def result_head(outdir, dataset, task, sde, nparticles, k) -> str:
    return os.path.join(outdir, f"{dataset}-{task}-{sde}-{nparticles}-{k}")


def _load_method(outdir, dataset, task, sde, nparticles, method, ny0s):
    trues, blocks = [], []
    for k in range(ny0s):
        head = result_head(outdir, dataset, task, sde, nparticles, k)
        trues.append(np.load(head + "-true.npz")["test_img"])
        blocks.append(np.load(head + method_suffix(method) + ".npy"))
    return np.stack(trues, 0).astype(np.float32), np.stack(blocks, 0).astype(np.float32)


def _host(x) -> np.ndarray:
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def tabulate_images(outdir, dataset, task, sde, nparticles, methods, ny0s, q=0.95):
    """Mean and standard deviation of PSNR and SSIM over the (ny0s, nsamples) restored images of every method, from the
    files examples/imgs_restore.py wrote into outdir: f'{dataset}-{task}-{sde}-{nparticles}-{k}' + '-true.npz' and
    + method_suffix(method) + '.npy' for k < ny0s.  All images of a method are scored in one psnr_ssim call.  Returns
    {method: {'psnr': (mean, std), 'ssim': (mean, std), 'n': ny0s * nsamples}}.  q is the reference's unused setting, kept
    for its place in the argument list."""
    table = {}
    for method in methods:
        trues, blocks = _load_method(outdir, dataset, task, sde, nparticles, method, ny0s)
        psnr, ssim = psnr_ssim(trues, blocks, clip=True)
        psnr, ssim = _host(psnr), _host(ssim)
        table[method] = {"psnr": (float(np.mean(psnr)), float(np.std(psnr))),
                         "ssim": (float(np.mean(ssim)), float(np.std(ssim))), "n": int(psnr.size)}
    return table


def tabulate_autocorr(outdir, dataset, task, sde, nparticles, methods, ny0s, max_lags=20):
    """The best-variable autocorrelation curve (max_lags,) of every chain method (gibbs*, pmcmc*), averaged over the ny0s
    image chains: one curve of Figure 8.  Other methods draw independent samples and are skipped."""
    curves = {}
    for method in methods:
        if method.split("-")[0] not in CHAIN_METHODS:
            continue
        _, blocks = _load_method(outdir, dataset, task, sde, nparticles, method, ny0s)
        _, best = chain_autocorrelation(blocks.reshape(blocks.shape[0], blocks.shape[1], -1), max_lags)
        curves[method] = np.mean(_host(best), axis=0)
    return curves
