"""Time per gibbs_kernel(marg_y=True) sweep (all chains): closure tier against fused engine, and fused marg_y=True
against fused marg_y=False (what the Doob bridge adds), for config 1 (2-D toy, N = 1024, T = 200, ts = linspace(0, 2))
and the reference's d = 100 toy at 100 particles (T = 200); 4 chains.

(a) closure tier: samplers.gibbs_kernel per chain with a lambda-wrapped fwd_sampler, which keeps it off the fused engine --
    the host loop over T steps plus fbsmi_affine_em_path for the bridge, what marg_y=True ran before the fused path;
(b) fused: LGSweep.chain, one hipGraph replay per sweep for all chains, marg_y=True and marg_y=False.
All start from the same state, are timed with a host clock round work that ends in a device synchronise, and alternate
over `--repeats` windows; the median and the min .. max spread of the windows are printed, then one JSON line.
--profile: only a few fused marg_y=True sweeps per shape, for `rocprofv3 --kernel-trace --stats -- python tools/bench_marg.py --profile`
(k_lg_bridge_noise / k_lg_bridge durations).
python tools/bench_marg.py [--repeats 5] [--closure-sweeps 2] [--fused-sweeps 100]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import fbs_amd
from fbs_amd import ops
from fbs_amd.samplers import gibbs_kernel
from fbs_amd.sdes import StationaryConstLinearSDE
from _gp_toy import gp_setting

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--closure-sweeps", type=int, default=2)
ap.add_argument("--fused-sweeps", type=int, default=100)
ap.add_argument("--nchains", type=int, default=4)
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
C = args.nchains


def config1():
    ts = np.linspace(0.0, 2.0, 201)
    sde = StationaryConstLinearSDE(a=-0.5, b=1.0)
    br = fbs_amd.LinearGaussianBridge(np.array([-1.0, 1.0]), np.array([[2.0, 0.4], [0.4, 0.5]]), sde, ts, du=1, device=dev)
    return "config 1 (2-D toy, N = 1024, T = 200)", br, sde, ts, torch.zeros(1, device=dev), 1024


def gp100():
    g = gp_setting(argparse.Namespace(id=666, d=100, sde="const"), dev)
    return "d = 100 toy, 100 particles, T = 200", g["bridge"], g["sde"], g["ts"], g["y0_t"], 100


results = {}
for name, br, sde, ts, y0, n in (config1(), gp100()):
    marg = br.sweep_handle(n, True, False, nchains=C, marg_y=True)
    plain = br.sweep_handle(n, True, False, nchains=C)
    x0 = torch.zeros((C, br.du), device=dev)
    bs = np.zeros((C, br.T + 1), np.int32)
    _, x0, bs, _ = marg.chain(ops.PRNGKey(2), x0, y0, bs, 20, keep=False)     # a settled state
    if args.profile:
        marg.chain(ops.PRNGKey(3), x0, y0, bs, 10, keep=False)
        torch.cuda.synchronize()
        continue
    wrapped = lambda *a, **k: br.fwd_sampler(*a, **k)       # a foreign closure: the closure tier

    def closure(sweeps):
        k, state = ops.PRNGKey(3), [(x0[c], bs[c]) for c in range(C)]
        for _ in range(sweeps):
            k, sub = ops.split(k)
            for c, kc in enumerate(ops.split(sub, C)):
                o = gibbs_kernel(kc, state[c][0], y0, None, state[c][1], ts, wrapped, sde, br.unpack, n, br.transition_sampler,
                                 br.transition_logpdf, br.likelihood_logpdf, marg_y=True)
                state[c] = (o[0], o[2])

    def fused(sweeps):
        marg.chain(ops.PRNGKey(3), x0, y0, bs, sweeps, keep=False)

    def fused_plain(sweeps):
        plain.chain(ops.PRNGKey(3), x0, y0, bs, sweeps, keep=False)

    def window(fn, sweeps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(sweeps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / sweeps * 1e3

    closure(1), fused(10), fused_plain(10)                   # warm-up of every shape the windows use
    a, b, p = [], [], []
    for _ in range(args.repeats):                            # alternate the three
        a.append(window(closure, args.closure_sweeps))
        b.append(window(fused, args.fused_sweeps))
        p.append(window(fused_plain, args.fused_sweeps))
    ma, mb, mp = float(np.median(a)), float(np.median(b)), float(np.median(p))
    print(f"{name}, {C} chains: closure tier {ma:.2f} ms per sweep (min {min(a):.2f} .. max {max(a):.2f}), fused marg_y=True "
          f"{mb:.3f} ms (min {min(b):.3f} .. max {max(b):.3f}), ratio {ma / mb:.1f}x; fused marg_y=False {mp:.3f} ms "
          f"(min {min(p):.3f} .. max {max(p):.3f}): the bridge adds {mb - mp:.3f} ms; {args.repeats} windows")
    results[name] = dict(closure_ms=ma, closure_min=min(a), closure_max=max(a), fused_ms=mb, fused_min=min(b), fused_max=max(b),
                         fused_plain_ms=mp, fused_plain_min=min(p), fused_plain_max=max(p), bridge_adds_ms=mb - mp,
                         faster_beyond_spread=bool(max(b) < min(a)))
if not args.profile:
    print(json.dumps(dict(bench="gibbs_marg_y_sweep", nchains=C, results=results)))
