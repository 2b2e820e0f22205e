"""Time per conditional sample of the bootstrap-filter sampler (experiments/toy/gp_filter.py, T = 200) on the d = 100 toy
at 100 particles and on the narrow 2-D toy at 4096 particles: the per-sample loop against the fused engine at B in
{1, 64, 1024} samples per call.

(a) loop: the body of examples/toy_filter.py's conditional_sampler, once per sample -- fwd_ys_sampler, the host-side
    ref_sampler and one replay of the flow-0 filter graph (what the example runs without --fused);
(b) fused: fbs_amd.samplers.filter_conditional_sampler on B keys (LGFilterSampler: one graph replay per chunk).
Both are warmed up, timed with a host clock round work that ends in a device synchronise, and alternate over `--repeats`
windows; the median and the min .. max spread of the windows are printed, then one JSON line and the verdict on the
feature's acceptance condition (at B = 64 the fused per-sample time is below the loop's on both toys) and on the separate
B = 1 finding (fused at most 8 %, the box-to-box spread, above the loop's on both).  The exit status is 1 when either fails.
python tools/bench_filter_sampler.py [--repeats 5] [--loop-samples 8] [--fused-ms 300] [--batches 1 64 1024]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import fbs_amd
from fbs_amd import ops
from fbs_amd.samplers import bootstrap_filter, filter_conditional_sampler, stratified
from fbs_amd.sdes import StationaryConstLinearSDE
from _gp_toy import gp_setting

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--loop-samples", type=int, default=8)
ap.add_argument("--fused-ms", type=float, default=300.0, help="least work of a fused window (sets its number of calls)")
ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
args = ap.parse_args()
dev = torch.device("cuda:0")

g = gp_setting(argparse.Namespace(id=666, d=100, sde="const"), dev)
narrow = fbs_amd.LinearGaussianBridge(np.array([-1.0, 1.0]), np.array([[2.0, 0.4], [0.4, 0.5]]),
                                      StationaryConstLinearSDE(a=-0.5, b=1.0), g["ts"], du=1, device=dev)
TOYS = [("d = 100, N = 100", g["bridge"], g["y0_t"], 100), ("2-D, N = 4096", narrow, torch.zeros(1, device=dev), 4096)]
ts = g["ts"]


def window(fn, nsamples):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / nsamples * 1e3


results = {}
loop_keys = ops.split(ops.PRNGKey(3), args.loop_samples)     # derived outside the timed windows, like the fused tier's
verdict = {}
for name, br, y0, n in TOYS:
    def loop():
        for key_ in loop_keys:                                               # examples/toy_filter.py:conditional_sampler
            key_fwd, key_bwd, key_bf = ops.split(key_, 3)
            vs = torch.flip(br.fwd_ys_sampler(key_fwd, y0), [0])
            bootstrap_filter(br.transition_sampler, br.likelihood_logpdf, vs, ts, br.ref_sampler, key_bf, n, stratified,
                             log=True, return_last=True)[0][0]

    for B in args.batches:
        keys = ops.split(ops.PRNGKey(4), B)
        calls = 1

        def fused():
            for _ in range(calls):
                filter_conditional_sampler(keys, y0, ts, br.fwd_ys_sampler, br.ref_sampler, br.transition_sampler,
                                           br.likelihood_logpdf, n, stratified)

        loop(), fused()                                      # warm-up of every shape the windows use
        calls = max(1, int(args.fused_ms / max(window(fused, 1), 1e-3)))
        a, b = [], []
        for _ in range(args.repeats):                        # alternate the two tiers
            a.append(window(loop, args.loop_samples))
            b.append(window(fused, calls * B))
        ma, mb = float(np.median(a)), float(np.median(b))
        tag = f"{name}, T = {br.T}, B = {B}"
        print(f"{tag}: loop {ma:.3f} ms per sample (min {min(a):.3f} .. max {max(a):.3f}), fused {mb:.4f} ms per sample "
              f"(min {min(b):.4f} .. max {max(b):.4f}), {mb * B:.3f} ms per call, ratio {ma / mb:.1f}x over {args.repeats} "
              f"windows of {args.loop_samples} / {calls * B} samples", flush=True)
        results[tag] = dict(loop_ms=ma, loop_min=min(a), loop_max=max(a), fused_ms=mb, fused_min=min(b), fused_max=max(b),
                            fused_call_ms=mb * B, fused_below_loop=bool(mb < ma), fused_within_8pct_of_loop=bool(mb <= 1.08 * ma))
        verdict[(name, B)] = (mb < ma, mb <= 1.08 * ma)
toys = [t[0] for t in TOYS]
at64 = all(verdict[(t, 64)][0] for t in toys) if 64 in args.batches else None
at1 = all(verdict[(t, 1)][1] for t in toys) if 1 in args.batches else None
print(json.dumps(dict(bench="filter_sampler", results=results, fused_below_loop_at_B64_on_both_toys=at64,
                      fused_within_8pct_of_loop_at_B1_on_both_toys=at1)))
say = lambda v: "not evaluated" if v is None else ("met" if v else "NOT met")
print(f"acceptance condition (B = 64: fused per-sample time below the loop's on both toys): {say(at64)}")
print(f"finding (B = 1: fused at most 8 % above the loop's on both toys): {say(at1)}")
sys.exit(1 if at64 is False or at1 is False else 0)
