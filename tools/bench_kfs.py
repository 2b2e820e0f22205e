"""Time per path of the Kalman smoother and path sampler (examples/toy_kf.py --smoother, T = 200) on the d = 100 toy and on
the narrow 2-D toy at B in {1, 64, 1024} samples per call, next to the Kalman conditional sampler of the same build and to
the particle route at 100 particles, on the same keys in the same run.

(a) sample:   LGKalmanSmoother.sample on B keys (three launches per call);
(b) smooth:   LGKalmanSmoother.smooth on the observation paths of (a) (three launches, nothing drawn);
(c) kf:       LGKalman.sample on B keys (fbsmi_kf_sample: two launches per call);
(d) particle: filter_handle(store_path=True, nchains=B).run + backsim_handle(n, 'smoother', B).run at n particles on the
              observation paths of (a) (bootstrap_filter keeping its path, then bootstrap_backward_smoother).
All are warmed up, timed with a host clock round work that ends in a device synchronise, and alternate over `--repeats`
windows; the median and the min .. max spread of the windows are printed, then one JSON line.  No target is set: the
figures are what is written down.
python tools/bench_kfs.py [--repeats 5] [--window-ms 300] [--batches 1 64 1024] [--nparticles 100]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import fbs_amd
from fbs_amd import ops
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
n = args.nparticles


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
        hs, hk = br.kalman_smoother_handle(B), br.kalman_handle(B)
        # the particle route keeps (chains, T+1, n, du) floats: at most 2^29 of them, so fewer chains per call where B
        # of them do not fit (its time per path is then that of the smaller call)
        Bp = B if B * (br.T + 1) * n * br.du <= 1 << 29 else 64
        hf, hb = br.filter_handle(n, "bootstrap", "stratified", store_path=True, nchains=Bp), br.backsim_handle(n, "smoother", Bp)
        hs.sample(keys, y0)
        vs = hs.views()["vs"]
        u0s = torch.stack([br.ref_sampler(keys[b], vs[b, 0], n) for b in range(min(Bp, 8))])
        u0s = u0s.repeat((Bp + u0s.shape[0] - 1) // u0s.shape[0], 1, 1)[:Bp].contiguous()   # timing inputs only
        kq, vq, uq = (keys[:Bp], vs[:Bp].contiguous(), u0s) if Bp > 1 else (keys[0], vs[0], u0s[0])

        def particle():
            hb.run(kq, vq, hf.run(kq, vq, uq)[2])

        fns = {"sample": lambda: hs.sample(keys, y0), "smooth": lambda: hs.smooth(vs), "kf": lambda: hk.sample(keys, y0),
               "particle": particle}
        calls = {}
        for k, fn in fns.items():
            fn()                                             # warm-up of every shape the windows use
            calls[k] = max(1, int(args.window_ms / max(window(fn, 1), 1e-3)))
        times = {k: [] for k in fns}
        per = {k: Bp if k == "particle" else B for k in fns}
        for _ in range(args.repeats):                        # alternate the four
            for k, fn in fns.items():
                times[k].append(window(lambda: [fn() for _ in range(calls[k])], calls[k] * per[k]))
        med = {k: float(np.median(v)) for k, v in times.items()}
        tag = f"{name}, T = {br.T}, B = {B}"
        print(f"{tag}: " + "; ".join(f"{k} {med[k]:.4f} ms per path (min {min(times[k]):.4f} .. max {max(times[k]):.4f}), "
                                     f"{med[k] * per[k]:.3f} ms per call of {per[k]}" for k in fns)
              + f"; sample / kf {med['sample'] / med['kf']:.2f}x, particle N = {n} / sample {med['particle'] / med['sample']:.2f}x "
              f"over {args.repeats} windows", flush=True)
        results[tag] = dict({f"{k}_ms": med[k] for k in fns}, **{f"{k}_min": min(times[k]) for k in fns},
                            **{f"{k}_max": max(times[k]) for k in fns}, nparticles=n, particle_chains=Bp)
print(json.dumps(dict(bench="kfs", results=results)))
