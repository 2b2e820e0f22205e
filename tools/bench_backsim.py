"""Time per backward simulation pass of the analytic model (T = 200), closure tier against the fused engine, for both
recursions: bootstrap_backward_smoother ('smoother') and backward_sampling_pass ('sampling').

(a) closure tier: the host loop of fbs_amd.samplers on the same commit, reached through a wrapped closure (a lambda round
    the bridge's transition_logpdf is not recognised by the dispatch), one call per chain;
(b) fused: LGBacksim.run, one hipGraph replay for the C chains.
Cases: the narrow GP toy (d = 2) at n = 4096 and 65 536, the d = 100 toy at n = 100 and 10 000, C = 1 and 4 chains.  The
stored path is the fused bootstrap filter's (LGFilter, store_path); the sampling mode reads it with fixed-seed normalised
log-weights.  Both tiers are warmed up, timed with a host clock round work that ends in a device synchronise, and alternate
over `--repeats` windows; the median and the min .. max spread of the windows are printed, then one JSON line.  The
acceptance condition is qualitative: fused below closure tier in every window of every case.
python tools/bench_backsim.py [--repeats 3] [--fused-calls 3] [--steps 200]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fbs_amd
from fbs_amd import ops
from fbs_amd.samplers import smc
from fbs_amd.samplers.csmc.csmc import backward_sampling_pass
from fbs_amd.sdes import StationaryConstLinearSDE

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--fused-calls", type=int, default=3)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--cases", type=str, nargs="+", default=["2:4096", "2:65536", "100:100", "100:10000"], help="d:n")
ap.add_argument("--chains", type=int, nargs="+", default=[1, 4])
args = ap.parse_args()
dev = torch.device("cuda:0")
T = args.steps
ts = np.linspace(0.0, 1.0, T + 1)


def gp_bridge(d):
    zs = np.linspace(0.0, 5.0, d)
    cov = np.exp(-np.abs(zs[None, :] - zs[:, None]))
    joint = np.block([[cov, cov], [cov, cov + np.eye(d)]])
    return fbs_amd.LinearGaussianBridge(np.zeros(2 * d), joint, StationaryConstLinearSDE(a=-0.5, b=1.0), ts, du=d, device=dev)


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


results, ok = {}, True
for case in args.cases:
    d, n = (int(x) for x in case.split(":"))
    br = gp_bridge(d)
    wrapped = lambda *a: br.transition_logpdf(*a)
    for Cn in args.chains:
        keys = ops.split(ops.PRNGKey(7), Cn)
        y0 = torch.from_numpy(np.random.default_rng(5).normal(size=d).astype(np.float32)).to(dev)
        vs = torch.stack([torch.flip(br.fwd_ys_sampler(k, y0), [0]) for k in ops.split(ops.PRNGKey(8), Cn)], 0)
        u0s = torch.stack([br.ref_sampler(k, vs[c, 0], n) for c, k in enumerate(ops.split(ops.PRNGKey(9), Cn))], 0)
        path = br.filter_handle(n, "bootstrap", "stratified", store_path=True, nchains=Cn).run(keys, vs, u0s)[2]
        path = path.reshape(Cn, T + 1, n, d)
        gen = torch.Generator(device="cpu").manual_seed(11)
        lws = torch.log_softmax(torch.randn((Cn, T + 1, n), generator=gen), dim=-1).to(dev)
        for mode in ("smoother", "sampling"):
            h = br.backsim_handle(n, mode, Cn)
            extra = (lws,) if mode == "sampling" else ()

            def fused():
                for _ in range(args.fused_calls):
                    h.run(keys, vs, path, *extra)

            def closure():
                for c in range(Cn):
                    if mode == "smoother":
                        smc.bootstrap_backward_smoother(keys[c], path[c], vs[c], ts, wrapped)
                    else:
                        backward_sampling_pass(keys[c], wrapped, vs[c], ts, path[c], lws[c])

            runs0 = h.runs
            closure(), fused()                                   # warm-up of every shape the windows use
            assert h.runs == runs0 + args.fused_calls           # (the wrapped closure did not reach the handle)
            a, b = [], []
            for _ in range(args.repeats):                        # alternate the two tiers
                a.append(window(closure, 1))
                b.append(window(fused, args.fused_calls))
            ma, mb = float(np.median(a)), float(np.median(b))
            name = f"{mode}, d = {d}, n = {n}, T = {T}, C = {Cn}"
            below = bool(max(b) < min(a))
            ok = ok and below
            print(f"{name}: closure tier {ma:.2f} ms per pass of {Cn} chain(s) (min {min(a):.2f} .. max {max(a):.2f}), "
                  f"fused {mb:.3f} ms (min {min(b):.3f} .. max {max(b):.3f}), ratio {ma / mb:.0f}x over {args.repeats} windows")
            results[name] = dict(closure_ms=ma, closure_min=min(a), closure_max=max(a), fused_ms=mb, fused_min=min(b),
                                 fused_max=max(b), fused_below_closure_in_every_window=below)
        del path, lws, u0s
print(json.dumps(dict(bench="backsim_pass", steps=T, fused_below_closure_everywhere=ok, results=results)))
sys.exit(0 if ok else 1)
