"""Time per pMCMC iteration (all chains), loop tier against fused engine, for the narrow toy (du = dv = 1, N = 4096,
T = 200) and the reference's d = 100 toy (100 particles, T = 200); 4 chains, pCN with delta = 0.005.

(a) loop tier: samplers.pmcmc_kernel per chain and iteration on the host (what examples/toy_pmcmc.py runs without --fused);
(b) fused: LGPmcmc.chain, one hipGraph replay per iteration for all chains.
Both start from the same warmed-up state, are timed with a host clock round work that ends in a device synchronise, and
alternate over `--repeats` windows; the median and the min .. max spread of the windows are printed, then one JSON line.
python tools/bench_pmcmc.py [--repeats 7] [--loop-iters 10] [--fused-iters 100]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import fbs_amd
from fbs_amd import ops
from fbs_amd.samplers import pmcmc_kernel, stratified
from fbs_amd.sdes import StationaryConstLinearSDE
from _gp_toy import gp_setting

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--loop-iters", type=int, default=10)
ap.add_argument("--fused-iters", type=int, default=100)
ap.add_argument("--nchains", type=int, default=4)
ap.add_argument("--delta", type=float, default=0.005)
args = ap.parse_args()
dev = torch.device("cuda:0")
C, delta = args.nchains, args.delta


def narrow():
    ts = np.linspace(0.0, 2.0, 201)
    sde = StationaryConstLinearSDE(a=-0.5, b=1.0)
    br = fbs_amd.LinearGaussianBridge(np.array([-1.0, 1.0]), np.array([[2.0, 0.4], [0.4, 0.5]]), sde, ts, du=1, device=dev)
    return "narrow toy, N = 4096, T = 200", br, sde, ts, torch.zeros(1, device=dev), 4096


def gp100():
    g = gp_setting(argparse.Namespace(id=666, d=100, sde="const"), dev)
    return "d = 100 toy, 100 particles, T = 200", g["bridge"], g["sde"], g["ts"], g["y0_t"], 100


results = {}
for name, br, sde, ts, y0, n in (narrow(), gp100()):
    h = br.pmcmc_handle(n, "stratified", nchains=C, delta=delta)
    key = ops.PRNGKey(1)
    ys0 = torch.stack([br.fwd_ys_sampler(k, y0) for k in ops.split(key, C)])
    # a first proposal is always accepted against log_ell = -1e30; twenty more iterations settle the state
    _, uT, ell, ys, _, _ = h.chain(ops.PRNGKey(2), torch.zeros((C, br.du), device=dev), torch.full((C,), -1e30, device=dev),
                                   ys0, y0, 21)

    def loop(iters):
        k, state = ops.PRNGKey(3), [(uT[c], ell[c], ys[c]) for c in range(C)]
        for _ in range(iters):
            k, sub = ops.split(k)
            for c, kc in enumerate(ops.split(sub, C)):
                state[c] = pmcmc_kernel(kc, *state[c], y0, ts, br.fwd_ys_sampler, sde, br.ref_sampler, br.transition_sampler,
                                        br.likelihood_logpdf, stratified, n, delta=delta)[:3]

    def fused(iters):
        h.chain(ops.PRNGKey(3), uT, ell, ys, y0, iters)

    def window(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(iters)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    loop(2), fused(10)                                    # warm-up of every shape the windows use
    a, b = [], []
    for _ in range(args.repeats):                         # alternate the two tiers
        a.append(window(loop, args.loop_iters))
        b.append(window(fused, args.fused_iters))
    ma, mb = float(np.median(a)), float(np.median(b))
    print(f"{name}, {C} chains, delta = {delta}: loop tier {ma:.3f} ms per iteration (min {min(a):.3f} .. max {max(a):.3f}), "
          f"fused {mb:.3f} ms (min {min(b):.3f} .. max {max(b):.3f}), ratio {ma / mb:.1f}x over {args.repeats} windows")
    results[name] = dict(loop_ms=ma, loop_min=min(a), loop_max=max(a), fused_ms=mb, fused_min=min(b), fused_max=max(b),
                         faster_beyond_spread=bool(max(b) < min(a)))
print(json.dumps(dict(bench="pmcmc_iteration", nchains=C, delta=delta, results=results)))
