"""Time per Gibbs sweep of the Gaussian Schrodinger-bridge toy (experiments/sb/gibbs.py's setting: d = 10, T = 100,
10 Euler-Maruyama sub-steps per interval) on the closure tier (examples/toy_sb_gibbs.py without --fused: host loops, one
launch per sub-step and per sampler operation) and on the fused engine (fbs_amd.GaussianSBBridge: one hipGraph replay per
sweep, the chain driven on the device), for 10 and 100 particles and 1 and 4 chains.  Warm-up first, device-synchronised
wall clock around the timed sweeps; one JSON line per configuration.  Not the headline benchmark (bench.py).

--fused-only N: only the fused chain of N sweeps at 100 particles, one chain (the run to put under a kernel-trace profiler:
the path kernel's share of the sweep)."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from fbs_amd import ops  # noqa: E402
from fbs_amd.samplers import gibbs_kernel  # noqa: E402
from toy_sb_gibbs import sb_setting  # noqa: E402


def setting(d, fused, dev):
    return sb_setting(SimpleNamespace(id=666, d=d, fused=fused), dev)


def time_closure(g, nparticles, nchains, eb, sweeps, warmup):
    """Per sweep: every chain one gibbs_kernel call on the closure tier (the reference's vmap over chains is a loop here)."""
    d, T = g.d, g.nsteps
    dev = g.y0.device
    x0 = [torch.zeros(d, device=dev) for _ in range(nchains)]
    bs = [np.zeros(T + 1, np.int32) for _ in range(nchains)]
    key = g.key

    def sweep():
        nonlocal key
        key, sub = ops.split(key)
        keys = ops.split(sub, nchains) if nchains > 1 else [sub]
        for c in range(nchains):
            x0[c], _, bs[c], _ = gibbs_kernel(keys[c], x0[c], g.y0, None, bs[c], g.ts, g.fwd_sampler, None, g.unpack,
                                              nparticles, g.transition_sampler, g.transition_logpdf, g.likelihood_logpdf,
                                              marg_y=False, explicit_backward=eb, explicit_final=False)
    for _ in range(warmup):
        sweep()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(sweeps):
        sweep()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / sweeps


def time_fused(g, nparticles, nchains, eb, sweeps, warmup):
    d, T = g.d, g.nsteps
    h = g.bridge.sweep_handle(nparticles, eb, False, nchains=nchains)
    shape = (nchains, d) if nchains > 1 else (d,)
    x0 = np.zeros(shape, np.float32)
    bs = np.zeros((nchains, T + 1) if nchains > 1 else (T + 1,), np.int32)
    key, x0, bs, _ = h.chain(g.key, x0, g.y0, bs, warmup, keep=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h.chain(key, x0, g.y0, bs, sweeps, keep=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--closure-sweeps", type=int, default=3)
    ap.add_argument("--fused-sweeps", type=int, default=200)
    ap.add_argument("--explicit_backward", type=int, default=1)
    ap.add_argument("--fused-only", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eb = bool(args.explicit_backward)
    gf = setting(args.d, True, dev)
    if args.fused_only:
        s = time_fused(gf, 100, 1, eb, args.fused_only, 5)
        print(json.dumps(dict(tier="fused", d=args.d, nparticles=100, nchains=1, sweeps=args.fused_only, ms_per_sweep=s * 1e3)))
        return
    gc = setting(args.d, False, dev)
    for n in (10, 100):
        for nc in (1, 4):
            tc = time_closure(gc, n, nc, eb, args.closure_sweeps, 1)
            tf = time_fused(gf, n, nc, eb, args.fused_sweeps, 10)
            print(json.dumps(dict(d=args.d, T=gf.nsteps, nsub=10, nparticles=n, nchains=nc, explicit_backward=eb,
                                  closure_ms_per_sweep=round(tc * 1e3, 3), fused_ms_per_sweep=round(tf * 1e3, 4),
                                  speedup=round(tc / tf, 1))), flush=True)


if __name__ == "__main__":
    main()
