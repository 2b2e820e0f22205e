"""Time per conditional sample of the CSGM toy (experiments/toy/gp_csgm.py: d = 100, T = 200), closure tier against fused
engine at B in {1, 16, 64, 1000} samples per fused call.

(a) closure tier: examples/toy_csgm.py's conditional_sampler -- euler_maruyama's host loop, per step one torch matrix
    product, the elementwise launches round it and one fbsmi_em_update (what the example runs without --fused);
(b) fused: CsgmHandle.sample, one kernel launch for B samples.
Both are warmed up, timed with a host clock round work that ends in a device synchronise, and alternate over `--repeats`
windows; the median and the min .. max spread of the windows are printed, then one JSON line.
python tools/bench_csgm.py [--sde const] [--repeats 5] [--closure-samples 1] [--fused-calls 5]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import fbs_amd
from fbs_amd import ops
from _gp_toy import gp_setting
from toy_csgm import closure_sampler

ap = argparse.ArgumentParser()
ap.add_argument("--sde", type=str, default="const")
ap.add_argument("--d", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--closure-samples", type=int, default=1)
ap.add_argument("--fused-calls", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64, 1000])
args = ap.parse_args()
dev = torch.device("cuda:0")
g = gp_setting(argparse.Namespace(id=666, d=args.d, sde=args.sde), dev)
model = fbs_amd.GaussianCSGM(np.zeros(args.d), g["cov_mat"], g["sde"], g["ts"], g["obs_var"], g["y0"], device=dev)
sampler = closure_sampler(g, dev)


def window(fn, nsamples):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / nsamples * 1e3


def closure():
    for k in ops.split(ops.PRNGKey(3), args.closure_samples):
        sampler(k)


results = {}
for B in args.batches:
    h = model.handle(B)
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
    name = f"d = {args.d}, T = {model.T}, B = {B}"
    print(f"{name} ({args.sde}): closure tier {ma:.2f} ms per sample (min {min(a):.2f} .. max {max(a):.2f}), "
          f"fused {mb:.5f} ms per sample (min {min(b):.5f} .. max {max(b):.5f}), {mb * B:.3f} ms per call, "
          f"ratio {ma / mb:.0f}x over {args.repeats} windows")
    results[name] = dict(closure_ms=ma, closure_min=min(a), closure_max=max(a), fused_ms=mb, fused_min=min(b),
                         fused_max=max(b), fused_call_ms=mb * B, fused_below_closure_in_every_window=bool(max(b) < min(a)))
print(json.dumps(dict(bench="csgm_sample", sde=args.sde, results=results)))
