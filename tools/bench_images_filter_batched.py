"""Image bootstrap filters and pMCMC steps batched over ensembles: bootstrap_filter_batched and pmcmc_kernel_batched against
the loops of the unchanged bootstrap_filter and pmcmc_kernel over the same B ensembles, in one process on one card.  MNIST
inpaint-15, UNet dim 64 (random init), bf16 autocast, a short grid -- the method of tools/bench_images_batched.py.  Per case:
warm-up, then the median over `--reps` runs of either path; time per run and per ensemble-step; and the number of network
calls either path made in one run.  One JSON line per case.  Not the headline benchmark."""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbs_amd import ops
from fbs_amd.images import ImageRestore
from fbs_amd.samplers import bootstrap_filter, bootstrap_filter_batched, pmcmc_kernel, pmcmc_kernel_batched, stratified
from fbs_amd.score import ScoreBridge
from fbs_amd.sdes import StationaryLinLinearSDE
from fbs_amd.unet import UNet

ap = argparse.ArgumentParser()
ap.add_argument("--nparticles", default="10,100")
ap.add_argument("--batches", default="1,4,16,64")
ap.add_argument("--methods", default="filter,pmcmc")
ap.add_argument("--nsteps", type=int, default=20)
ap.add_argument("--reps", type=int, default=10, help="timed runs per path (the median is reported)")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--chunk", type=int, default=8192, help="rows per network call: at least B * nparticles = one call per step")
ap.add_argument("--out", default="", help="also append the JSON lines to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
Tend, T = 2.0, args.nsteps
ts = np.linspace(0, Tend, T + 1)
sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=Tend)
ds = ImageRestore("inpaint-15", (28, 28, 1), device=dev)
torch.manual_seed(0)
net = UNet(dt=Tend / 200, dim=64, in_channels=1, upsampling="pixel_shuffle").to(dev).eval()
ncalls = [0]


def score_fn(x, t):
    ncalls[0] += 1
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        return net(x, t)


sb = ScoreBridge(score_fn, ds, sde, ts, chunk=args.chunk, net_input_dtype=torch.bfloat16)


def timed(fn, reps, warmup):
    """-> (median ms, network calls of one run)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        ncalls[0] = 0
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        print(f"# {fn.__name__} {out[-1]:.1f} ms", file=sys.stderr, flush=True)
    return statistics.median(out), ncalls[0]


for method in args.methods.split(","):
    for N in (int(s) for s in args.nparticles.split(",")):
        for B in (int(s) for s in args.batches.split(",")):
            masks = [ds.gen_mask(ops.PRNGKey(100 + b)) for b in range(B)]
            y0s = [ds.unpack(ops.uniform(ops.PRNGKey(200 + b), (28, 28, 1), device=dev), masks[b])[1] for b in range(B)]
            yss = torch.stack([sb.fwd_ys_sampler(ops.PRNGKey(300 + b), y0s[b]) for b in range(B)], 0)
            vss = torch.flip(yss, [1])
            uTs, ells = torch.zeros((B, 225, 1), device=dev), torch.zeros(B, device=dev)
            count = [0]

            def keys():
                count[0] += 1
                return ops.split(ops.PRNGKey(count[0]), B)

            if method == "filter":
                def batched():
                    bootstrap_filter_batched(sb.transition_sampler, sb.likelihood_logpdf, vss, ts, sb.ref_sampler, keys(), N,
                                             stratified, mask_=masks)

                def loop():
                    k = keys()
                    for b in range(B):
                        bootstrap_filter(sb.transition_sampler, sb.likelihood_logpdf, vss[b], ts, sb.ref_sampler, k[b], N,
                                         stratified, mask_=masks[b])
            else:
                pm = (ts, sb.fwd_ys_sampler, sde, sb.ref_sampler, sb.transition_sampler, sb.likelihood_logpdf, stratified, N)

                def batched():
                    pmcmc_kernel_batched(keys(), uTs, ells, yss, y0s, *pm, delta=0.005, mask_=masks)

                def loop():
                    k = keys()
                    for b in range(B):
                        pmcmc_kernel(k[b], uTs[b], ells[b], yss[b], y0s[b], *pm, delta=0.005, mask_=masks[b])

            ms_b, calls_b = timed(batched, args.reps, args.warmup)
            ms_l, calls_l = timed(loop, args.reps, args.warmup)
            line = json.dumps({
                "workload": f"MNIST inpaint-15, UNet dim 64 (random init) bf16, {method}, {N} particles, {T} steps",
                "method": method, "B": B, "nparticles": N, "nsteps": T, "reps": args.reps,
                "batched_ms": ms_b, "loop_ms": ms_l,
                "batched_ms_per_ensemble_step": ms_b / (B * T), "loop_ms_per_ensemble_step": ms_l / (B * T),
                "speedup": ms_l / ms_b, "batched_network_calls": calls_b, "loop_network_calls": calls_l,
                "chunk": args.chunk})
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
