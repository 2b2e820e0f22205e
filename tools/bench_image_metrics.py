"""Time fbs_amd.image_metrics against the host float64 restatement (tests/imgmetrics_restate.py) at the sizes of a run:
100 x 100 MNIST-shaped images, 10 x 100 images of 64 x 64 x 3, and the autocorrelation of 100 chains of 100 samples of 784
pixels at 20 lags.

Device: data already on the GPU (where the samplers leave it), HIP events around one call after a warm-up, the median of 10
runs.  Host: the restatement's uniform_filter / FFT forms in a process pool over the CPUs this process may use (at most
OMP_NUM_THREADS of them), wall clock, one run; the pool does its work before the GPU is opened.  Prints one JSON line.

    python tools/bench_image_metrics.py [--host_images N]   (N: score only the first N images a case on the host and scale)
"""
import argparse
import json
import os
import statistics
import sys
import time
from multiprocessing import get_context

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imgmetrics_restate as R  # noqa: E402

IMAGE_CASES = (("mnist 100x100 of 28x28x1", 100, 100, (28, 28, 1)), ("celeba 10x100 of 64x64x3", 10, 100, (64, 64, 3)))
CHAIN_CASE = ("autocorr (100, 100, 784) L=20", 100, 100, 784, 20)


def _score(args):
    t, r = args
    return R.psnr_ssim(t[None], r[None])


def _autocorr(args):
    x, L = args
    ac = R.autocorr_fft(x, L)
    return ac, R.best_curve(ac)


def _cpus() -> int:
    n = len(os.sched_getaffinity(0))
    env = os.environ.get("OMP_NUM_THREADS")
    return max(1, min(n, int(env)) if env else min(n, 16))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--host_images", type=int, default=0, help="host: score this many images a case and scale (0: all)")
    p.add_argument("--runs", type=int, default=10)
    args = p.parse_args(argv)
    rng = np.random.default_rng(0)
    images, host = {}, {}
    ncpu = _cpus()
    with get_context("fork").Pool(ncpu) as pool:                              # before the GPU is opened
        for name, G, S, shape in IMAGE_CASES:
            t = rng.uniform(size=(G,) + shape).astype(np.float32)
            r = np.clip(t[:, None] + 0.1 * rng.normal(size=(G, S) + shape), -0.2, 1.2).astype(np.float32)
            images[name] = (t, r)
            jobs = [(t[g], r[g]) for g in range(G)]
            if args.host_images:
                jobs = [(t[0], r[0][:max(1, args.host_images)])]
            n = sum(j[1].shape[0] for j in jobs)
            t0 = time.perf_counter()
            pool.map(_score, jobs)
            host[name] = (time.perf_counter() - t0) * (G * S) / n
        name, M, S, D, L = CHAIN_CASE
        chains = np.cumsum(rng.normal(size=(M, S, D)), axis=1).astype(np.float32)
        t0 = time.perf_counter()
        pool.map(_autocorr, [(chains[m], L) for m in range(M)])
        host[name] = time.perf_counter() - t0

    import torch
    from fbs_amd.image_metrics import chain_autocorrelation, psnr_ssim
    if not torch.cuda.is_available():
        raise RuntimeError("bench_image_metrics needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    rows = []
    for name, G, S, shape in IMAGE_CASES:
        t, r = (torch.from_numpy(a).to(dev) for a in images[name])
        med, lo, hi = timed(lambda: psnr_ssim(t, r))
        rows.append(dict(case=name, device_ms_median=med, device_ms_min=lo, device_ms_max=hi, host_ms=host[name] * 1e3,
                         input_mbytes=(t.numel() + r.numel()) * 4 / 1e6))
    name, M, S, D, L = CHAIN_CASE
    x = torch.from_numpy(chains).to(dev)
    med, lo, hi = timed(lambda: chain_autocorrelation(x, L))
    rows.append(dict(case=name, device_ms_median=med, device_ms_min=lo, device_ms_max=hi, host_ms=host[name] * 1e3,
                     input_mbytes=x.numel() * 4 / 1e6))
    for row in rows:
        print(f"{row['case']:34s} device {row['device_ms_median']:9.3f} ms (min {row['device_ms_min']:.3f}, max "
              f"{row['device_ms_max']:.3f})   host {row['host_ms']:10.1f} ms on {ncpu} CPUs", file=sys.stderr)
    print(json.dumps(dict(tool="bench_image_metrics", gpu=torch.cuda.get_device_name(0), host_cpus=ncpu, runs=args.runs,
                          host_images=args.host_images, rows=rows)))


if __name__ == "__main__":
    main()
