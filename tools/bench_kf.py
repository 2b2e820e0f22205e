"""Time per conditional sample of the Kalman-filter sampler (examples/toy_kf.py, T = 200) on the d = 100 toy and on the
narrow 2-D toy at B in {1, 64, 1024} samples per call, next to the fused bootstrap-filter sampler at 100 particles on the
same keys in the same run.

(a) kf: fbs_amd.samplers.kalman_conditional_sampler on B keys (LGKalman: two launches per call);
(b) filter: fbs_amd.samplers.filter_conditional_sampler on B keys at 100 particles (LGFilterSampler: one graph replay).
Both are warmed up, timed with a host clock round work that ends in a device synchronise, and alternate over `--repeats`
windows; the median and the min .. max spread of the windows are printed, then one JSON line.  No target is set: the
figures are what is written down.
python tools/bench_kf.py [--repeats 5] [--window-ms 300] [--batches 1 64 1024] [--nparticles 100]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import fbs_amd
from fbs_amd import ops
from fbs_amd.samplers import filter_conditional_sampler, kalman_conditional_sampler, stratified
from fbs_amd.sdes import StationaryConstLinearSDE
from _gp_toy import gp_setting

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window-ms", type=float, default=300.0, help="least work of a window (sets its number of calls)")
ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
ap.add_argument("--nparticles", type=int, default=100)
args = ap.parse_args()
dev = torch.device("cuda:0")

g = gp_setting(argparse.Namespace(id=666, d=100, sde="const"), dev)
narrow = fbs_amd.LinearGaussianBridge(np.array([-1.0, 1.0]), np.array([[2.0, 0.4], [0.4, 0.5]]),
                                      StationaryConstLinearSDE(a=-0.5, b=1.0), g["ts"], du=1, device=dev)
TOYS = [("d = 100", g["bridge"], g["y0_t"]), ("2-D", narrow, torch.zeros(1, device=dev))]
ts, n = g["ts"], args.nparticles


def window(fn, nsamples):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / nsamples * 1e3


results = {}
for name, br, y0 in TOYS:
    for B in args.batches:
        keys = ops.split(ops.PRNGKey(4), B)
        calls = {"kf": 1, "filter": 1}

        def kf():
            for _ in range(calls["kf"]):
                kalman_conditional_sampler(keys, y0, br)

        def filt():
            for _ in range(calls["filter"]):
                filter_conditional_sampler(keys, y0, ts, br.fwd_ys_sampler, br.ref_sampler, br.transition_sampler,
                                           br.likelihood_logpdf, n, stratified)

        kf(), filt()                                         # warm-up of every shape the windows use
        calls["kf"] = max(1, int(args.window_ms / max(window(kf, 1), 1e-3)))
        calls["filter"] = max(1, int(args.window_ms / max(window(filt, 1), 1e-3)))
        a, b = [], []
        for _ in range(args.repeats):                        # alternate the two samplers
            a.append(window(kf, calls["kf"] * B))
            b.append(window(filt, calls["filter"] * B))
        ma, mb = float(np.median(a)), float(np.median(b))
        tag = f"{name}, T = {br.T}, B = {B}"
        print(f"{tag}: kf {ma:.4f} ms per sample (min {min(a):.4f} .. max {max(a):.4f}), {ma * B:.3f} ms per call; filter "
              f"N = {n} {mb:.4f} ms per sample (min {min(b):.4f} .. max {max(b):.4f}), {mb * B:.3f} ms per call; "
              f"filter / kf {mb / ma:.2f}x over {args.repeats} windows of {calls['kf'] * B} / {calls['filter'] * B} samples",
              flush=True)
        results[tag] = dict(kf_ms=ma, kf_min=min(a), kf_max=max(a), kf_call_ms=ma * B, filter_ms=mb, filter_min=min(b),
                            filter_max=max(b), filter_call_ms=mb * B, nparticles=n)
print(json.dumps(dict(bench="kf", results=results)))
