"""Time per conditional sample of the twisted-SMC toy (experiments/toy/gp_twisted.py: d = 100, T = 200), closure tier
against fused engine, for nparticles in {100, 10 000} and B in {1, 64} samples per fused call.

(a) closure tier: examples/toy_twisted.py's conditional_sampler -- twisted_smc's host loop, the twisting gradient by
    torch.autograd (what the example runs without --fused);
(b) fused: TwistedHandle.sample, one hipGraph replay for B samples.
Both are warmed up, timed with a host clock round work that ends in a device synchronise, and alternate over `--repeats`
windows; the median and the min .. max spread of the windows are printed, then one JSON line.
python tools/bench_twisted.py [--sde const] [--repeats 5] [--closure-samples 1] [--fused-calls 3]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import fbs_amd
from fbs_amd import ops
from _gp_toy import gp_setting
from toy_twisted import closure_sampler

ap = argparse.ArgumentParser()
ap.add_argument("--sde", type=str, default="const")
ap.add_argument("--d", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--closure-samples", type=int, default=1)
ap.add_argument("--fused-calls", type=int, default=3)
ap.add_argument("--nparticles", type=int, nargs="+", default=[100, 10000])
ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
args = ap.parse_args()
dev = torch.device("cuda:0")
g = gp_setting(argparse.Namespace(id=666, d=args.d, sde=args.sde), dev)
model = fbs_amd.GaussianTwisted(np.zeros(args.d), g["cov_mat"], g["sde"], g["ts"], g["obs_var"], g["y0"], device=dev)


def window(fn, nsamples):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / nsamples * 1e3


results = {}
for n in args.nparticles:
    sampler = closure_sampler(g, n, dev)

    def closure():
        for k in ops.split(ops.PRNGKey(3), args.closure_samples):
            sampler(k)

    for B in args.batches:
        h = model.handle(n, "stratified", nruns=B)
        keys = ops.split(ops.PRNGKey(4), B)

        def fused():
            for _ in range(args.fused_calls):
                h.sample(keys)

        closure(), fused()                                   # warm-up of every shape the windows use
        a, b = [], []
        for _ in range(args.repeats):                        # alternate the two tiers
            a.append(window(closure, args.closure_samples))
            b.append(window(fused, args.fused_calls * B))
        ma, mb = float(np.median(a)), float(np.median(b))
        name = f"d = {args.d}, T = {model.T}, {n} particles, B = {B}"
        print(f"{name} ({args.sde}): closure tier {ma:.2f} ms per sample (min {min(a):.2f} .. max {max(a):.2f}), "
              f"fused {mb:.4f} ms (min {min(b):.4f} .. max {max(b):.4f}), ratio {ma / mb:.0f}x over {args.repeats} windows")
        results[name] = dict(closure_ms=ma, closure_min=min(a), closure_max=max(a), fused_ms=mb, fused_min=min(b),
                             fused_max=max(b), fused_below_closure_in_every_window=bool(max(b) < min(a)))
print(json.dumps(dict(bench="twisted_sample", sde=args.sde, results=results)))
