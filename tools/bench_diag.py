"""What the opt-in per-step diagnostics (sweep_handle / filter_handle(..., diagnostics=True)) cost: time per Gibbs sweep and
per bootstrap_filter run of one handle pair, diagnostics off / on, same process, same arguments.

Sweeps (4 chains, explicit_backward): BASELINE config 1 (2-D toy, N = 1024, T = 200), BASELINE config 2 (N = 65 536,
T = 500), the reference's d = 100 toy at 100 particles (T = 200).  Filters (one run, flow 0, stratified): the 2-D toy at
N = 4096 (T = 200) and the d = 100 toy at 100 particles.
Both handles start from the same state, are timed with a host clock round work that ends in a device synchronise, and alternate
over `--repeats` windows; the median and the min .. max spread of the windows are printed, then one JSON line.
python tools/bench_diag.py [--repeats 5] [--sweeps 20] [--runs 50]"""
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
ap.add_argument("--sweeps", type=int, default=20)
ap.add_argument("--runs", type=int, default=50)
ap.add_argument("--nchains", type=int, default=4)
args = ap.parse_args()
dev = torch.device("cuda:0")
C = args.nchains


def toy2d(T, Tend):
    return fbs_amd.LinearGaussianBridge(np.array([-1.0, 1.0]), np.array([[2.0, 0.4], [0.4, 0.5]]),
                                        StationaryConstLinearSDE(a=-0.5, b=1.0), np.linspace(0.0, Tend, T + 1), du=1, device=dev)


def gp100():
    g = gp_setting(argparse.Namespace(id=666, d=100, sde="const"), dev)
    return g["bridge"], g["y0_t"]


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def compare(name, off_fn, on_fn, n, unit, steps):
    off_fn(2), on_fn(2)                                       # warm-up: both graphs captured
    a, b = [], []
    for _ in range(args.repeats):                             # alternate the two
        a.append(window(off_fn, n))
        b.append(window(on_fn, n))
    ma, mb = float(np.median(a)), float(np.median(b))
    print(f"{name}: diagnostics off {ma:.3f} ms per {unit} (min {min(a):.3f} .. max {max(a):.3f}), on {mb:.3f} ms "
          f"(min {min(b):.3f} .. max {max(b):.3f}): +{mb - ma:.3f} ms = {(mb - ma) / steps * 1e3:.2f} us per step, "
          f"{100 * (mb / ma - 1):.1f} %; {args.repeats} windows of {n}")
    return dict(off_ms=ma, off_min=min(a), off_max=max(a), on_ms=mb, on_min=min(b), on_max=max(b),
                adds_us_per_step=(mb - ma) / steps * 1e3, steps=steps)


y2 = torch.zeros(1, device=dev)
gp, ygp = gp100()
results = {}
for name, br, y0, n in (("sweep, config 1 (2-D toy, N = 1024, T = 200)", toy2d(200, 2.0), y2, 1024),
                        ("sweep, config 2 (2-D toy, N = 65536, T = 500)", toy2d(500, 2.0), y2, 65536),
                        ("sweep, d = 100 toy, 100 particles, T = 200", gp, ygp, 100)):
    off = br.sweep_handle(n, True, False, nchains=C)
    on = br.sweep_handle(n, True, False, nchains=C, diagnostics=True)
    x0 = torch.zeros((C, br.du), device=dev)
    bs = np.zeros((C, br.T + 1), np.int32)
    _, x0, bs, _ = off.chain(ops.PRNGKey(2), x0, y0, bs, 5, keep=False)      # a settled state
    results[name] = compare(f"{name}, {C} chains", lambda k: off.chain(ops.PRNGKey(3), x0, y0, bs, k, keep=False),
                            lambda k: on.chain(ops.PRNGKey(3), x0, y0, bs, k, keep=False), args.sweeps, "sweep", br.T)

for name, br, y0, n in (("bootstrap_filter, 2-D toy, N = 4096, T = 200", toy2d(200, 2.0), y2, 4096),
                        ("bootstrap_filter, d = 100 toy, 100 particles, T = 200", gp, ygp, 100)):
    off = br.filter_handle(n, "bootstrap", "stratified")
    on = br.filter_handle(n, "bootstrap", "stratified", diagnostics=True)
    key = ops.PRNGKey(5)
    vs = torch.flip(br.fwd_ys_sampler(ops.PRNGKey(6), y0), [0]).contiguous()
    u0s = br.ref_sampler(ops.PRNGKey(7), vs[0], n).contiguous()

    def runs(h):
        def go(k):
            for _ in range(k):
                h.run(key, vs, u0s)
        return go

    results[name] = compare(name, runs(off), runs(on), args.runs, "run", br.T)
print(json.dumps(dict(bench="diagnostics_on_off", nchains=C, results=results)))
