"""Time per sample of the Kalman sampler and smoother of the Gaussian SB toy (examples/toy_sb_kf.py: d = 10, T = 100,
nsub = 10) at B in {1, 64, 1024} samples per call, next to the SB filter sampler at 10 and 100 particles and to the
Euler-Maruyama path kernel alone, on the same keys in the same run.

(a) kf:      SBKalman.sample on B keys (the Euler-Maruyama front, then fbsmi_kf's recursion and draw: two launches);
(b) kfs:     SBKalmanSmoother.sample on B keys (the same front, the storing recursion, the backward pass: three launches);
(c) filter:  SBFilterSampler.sample on B keys at each --nparticles (sb_filter_conditional_sampler's engine: the same front,
             then the batched bootstrap filter, one hipGraph replay);
(d) em_path: one fbsmi_lg_em_path call (one path, one workgroup: the T * nsub dependent sub-steps every front runs).
All are warmed up, timed with a host clock round work that ends in a device synchronise, and alternate over `--repeats`
windows; the median and the min .. max spread of the windows are printed, then the float32 error of (a) against the
float64 recursion on the same observation paths, then one JSON line.  No target is set: the figures are what is written
down.
python tools/bench_sb_kf.py [--repeats 5] [--window-ms 300] [--batches 1 64 1024] [--nparticles 10 100]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from fbs_amd import ops
from fbs_amd.gaussian_sb import sb_kalman_model
from fbs_amd.lg_kalman import kalman_filter_np
from toy_sb_gibbs import sb_setting

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window-ms", type=float, default=300.0, help="least work of a window (sets its number of calls)")
ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
ap.add_argument("--nparticles", type=int, nargs="+", default=[10, 100])
ap.add_argument("--d", type=int, default=10)
args = ap.parse_args()
dev = torch.device("cuda:0")

g = sb_setting(argparse.Namespace(id=666, d=args.d, fused=True), dev)
br, y0 = g.bridge, g.y0


def window(fn, nsamples):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / nsamples * 1e3


results = {}
x0 = ops.normal(ops.PRNGKey(5), (br.du,), device=dev)
for B in args.batches:
    keys = ops.split(ops.PRNGKey(4), B)
    hk, hs = br.sb_kalman_handle(B), br.sb_kalman_smoother_handle(B)
    fns = {"kf": lambda: hk.sample(keys, y0), "kfs": lambda: hs.sample(keys, y0)}
    for n in args.nparticles:
        hf = br.sb_filter_sampler_handle(n, "stratified", B)
        fns[f"filter{n}"] = lambda hf=hf: hf.sample(keys, y0)
    fns["em_path"] = lambda: br.fwd_sampler(keys[0], x0, y0)
    per = {k: 1 if k == "em_path" else B for k in fns}
    calls = {}
    for k, fn in fns.items():
        fn()                                             # warm-up of every shape the windows use
        calls[k] = max(1, int(args.window_ms / max(window(fn, 1), 1e-3)))
    times = {k: [] for k in fns}
    for _ in range(args.repeats):                        # alternate them
        for k, fn in fns.items():
            times[k].append(window(lambda: [fn() for _ in range(calls[k])], calls[k] * per[k]))
    med = {k: float(np.median(v)) for k, v in times.items()}
    tag = f"d = {br.du}, T = {br.T}, nsub = {br.nsub}, B = {B}"
    print(f"{tag}: " + "; ".join(f"{k} {med[k]:.4f} ms per sample (min {min(times[k]):.4f} .. max {max(times[k]):.4f}), "
                                 f"{med[k] * per[k]:.3f} ms per call of {per[k]}" for k in fns)
          + f" over {args.repeats} windows", flush=True)
    results[tag] = dict({f"{k}_ms": med[k] for k in fns}, **{f"{k}_min": min(times[k]) for k in fns},
                        **{f"{k}_max": max(times[k]) for k in fns})

# the float32 engine against the float64 recursion on its own observation paths
B = min(64, max(args.batches))
keys = ops.split(ops.PRNGKey(4), B)
hk = br.sb_kalman_handle(B)
_, means, ll = hk.sample(keys, y0, return_moments=True)
vs = hk.views()["vs"].cpu().numpy().astype(np.float64)
kt = sb_kalman_model(br).tables64
em = el = 0.0
for b in range(B):
    m64, ll64 = kalman_filter_np(kt, vs[b])
    em = max(em, float(np.abs(means[b].cpu().numpy() - m64).max() / np.abs(m64).max()))
    el = max(el, abs(float(ll[b]) - ll64) / abs(ll64))
print(f"float32 against float64 over {B} samples: means {em:.2e} of max |m|, loglik {el:.2e} relative")
print(json.dumps(dict(bench="sb_kf", results=results, f32_means=em, f32_loglik=el)))
