"""Time per conditional sample of the bootstrap-filter sampler on the Gaussian Schrodinger bridge (experiments/sb/filter.py:
d = 10, T = 100, nsub = 10) at 10 and 100 particles: the per-sample loop against the fused engine at B in {1, 64, 1024}
samples per call.

(a) loop: the body of examples/toy_sb_filter.py --fused without --batch, once per sample -- key splits, the x0 draw, one
    fbsmi_lg_em_path launch, the host-side ref_sampler and one replay of the flow-0 filter graph;
(b) fused: fbs_amd.samplers.sb_filter_conditional_sampler on B keys (SBFilterSampler: one graph replay per chunk).
Both are warmed up, timed with a host clock round work that ends in a device synchronise, and alternate over `--repeats`
windows; the median and the min .. max spread of the windows are printed, then one JSON line and the verdict on the
feature's two conditions: at B = 64 the fused per-sample time is below the loop's in EVERY window on both particle counts,
and at B = 1 the fused call's median is at most 8 % (the box-to-box spread) above the loop's.  The exit status is 1 when
either fails.
python tools/bench_sb_filter_sampler.py [--x0 heuristic|proper] [--repeats 5] [--loop-samples 8] [--fused-ms 300]
                                        [--batches 1 64 1024] [--nparticles 10 100]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from fbs_amd import ops
from fbs_amd.samplers import bootstrap_filter, sb_filter_conditional_sampler, stratified
from toy_sb_gibbs import sb_setting

ap = argparse.ArgumentParser()
ap.add_argument("--x0", default="heuristic", choices=("heuristic", "proper"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--loop-samples", type=int, default=8)
ap.add_argument("--fused-ms", type=float, default=300.0, help="least work of a fused window (sets its number of calls)")
ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
ap.add_argument("--nparticles", type=int, nargs="+", default=[10, 100])
args = ap.parse_args()
dev = torch.device("cuda:0")

g = sb_setting(argparse.Namespace(id=666, d=10, fused=True), dev)
br, d, y0, ts = g.bridge, g.d, g.y0, g.ts
prior = (g.gp_mean, np.linalg.cholesky(g.gp_cov)) if args.x0 == "proper" else None


def window(fn, nsamples):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / nsamples * 1e3


results = {}
loop_keys = ops.split(ops.PRNGKey(3), args.loop_samples)     # derived outside the timed windows, like the fused tier's
verdict = {}
for n in args.nparticles:
    def loop():
        for key_ in loop_keys:                                               # examples/toy_sb_filter.py:conditional_sampler
            key_fwd, key_bwd, key_bf = ops.split(key_, 3)
            key_x0, key_em = ops.split(key_fwd)
            x0_ = g.gp_posterior_sampler(key_x0) if args.x0 == "proper" else ops.normal(key_x0, (d,), device=dev)
            vs = torch.flip(g.em_path(key_em, x0_, y0)[:, d:], [0])
            bootstrap_filter(g.transition_sampler, g.likelihood_logpdf, vs, ts, g.ref_sampler, key_bf, n, stratified,
                             log=True, return_last=True)[0][0]

    for B in args.batches:
        keys = ops.split(ops.PRNGKey(4), B)
        calls = 1

        def fused():
            for _ in range(calls):
                sb_filter_conditional_sampler(keys, y0, ts, br.fwd_sampler, br.unpack, br.ref_sampler, br.transition_sampler,
                                              br.likelihood_logpdf, n, stratified, x0_prior=prior)

        loop(), fused()                                      # warm-up of every shape the windows use
        calls = max(1, int(args.fused_ms / max(window(fused, 1), 1e-3)))
        a, b = [], []
        for _ in range(args.repeats):                        # alternate the two tiers
            a.append(window(loop, args.loop_samples))
            b.append(window(fused, calls * B))
        ma, mb = float(np.median(a)), float(np.median(b))
        tag = f"d = {d}, T = {br.T}, nsub = {br.nsub}, N = {n}, B = {B}"
        print(f"{tag}: loop {ma:.3f} ms per sample (min {min(a):.3f} .. max {max(a):.3f}), fused {mb:.4f} ms per sample "
              f"(min {min(b):.4f} .. max {max(b):.4f}), {mb * B:.3f} ms per call, ratio {ma / mb:.1f}x over {args.repeats} "
              f"windows of {args.loop_samples} / {calls * B} samples", flush=True)
        below = all(y < x for x, y in zip(a, b))             # every window against the loop window beside it
        results[tag] = dict(loop_ms=ma, loop_min=min(a), loop_max=max(a), fused_ms=mb, fused_min=min(b), fused_max=max(b),
                            fused_call_ms=mb * B, fused_below_loop_in_every_window=below,
                            fused_within_8pct_of_loop=bool(mb <= 1.08 * ma))
        verdict[(n, B)] = (below, mb <= 1.08 * ma)
at64 = all(verdict[(n, 64)][0] for n in args.nparticles) if 64 in args.batches else None
at1 = all(verdict[(n, 1)][1] for n in args.nparticles) if 1 in args.batches else None
print(json.dumps(dict(bench="sb_filter_sampler", x0=args.x0, results=results,
                      fused_below_loop_at_B64_in_every_window=at64, fused_within_8pct_of_loop_at_B1=at1)))
say = lambda v: "not evaluated" if v is None else ("met" if v else "NOT met")
print(f"condition (B = 64: fused per-sample time below the loop's in every window, both particle counts): {say(at64)}")
print(f"condition (B = 1: fused call at most 8 % above the loop's, both particle counts): {say(at1)}")
sys.exit(1 if at64 is False or at1 is False else 0)
