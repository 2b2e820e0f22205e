"""Image Gibbs sweeps batched under the reference drivers' default flags: gibbs_kernel_batched(explicit_backward=False)
against the loop of the unchanged gibbs_kernel over the same B ensembles, plain and with marg_y, in one process on one
card.  MNIST inpaint-15, UNet dim 64 (random init), bf16 autocast, a short grid.  Per case: warm-up, then the median over
`--sweeps` sweeps of either path, with the smallest and largest sweep of each (the run-to-run spread the B = 1 rows are
read against); time per sweep and per ensemble-step.  One JSON line per case.  Not the headline benchmark."""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbs_amd import ops
from fbs_amd.images import ImageRestore
from fbs_amd.samplers import gibbs_kernel, gibbs_kernel_batched
from fbs_amd.score import ScoreBridge
from fbs_amd.sdes import StationaryLinLinearSDE
from fbs_amd.unet import UNet

ap = argparse.ArgumentParser()
ap.add_argument("--nparticles", default="10,100")
ap.add_argument("--batches", default="1,4,16,64")
ap.add_argument("--nsteps", type=int, default=20)
ap.add_argument("--sweeps", type=int, default=10, help="timed sweeps per path (the median is reported)")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--process-warmup", type=int, default=12, help="untimed sweeps before the first case of the process")
ap.add_argument("--chunk", type=int, default=8192, help="rows per network call: at least B * rows = one call per step")
ap.add_argument("--marg_y", default="0,1", help="which of the plain (0) and marg_y (1) sweeps to time")
ap.add_argument("--out", default="", help="also append the JSON lines to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
Tend, T = 2.0, args.nsteps
ts = np.linspace(0, Tend, T + 1)
sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=Tend)
ds = ImageRestore("inpaint-15", (28, 28, 1), device=dev)
torch.manual_seed(0)
net = UNet(dt=Tend / 200, dim=64, in_channels=1, upsampling="pixel_shuffle").to(dev).eval()


def score_fn(x, t):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        return net(x, t)


sb = ScoreBridge(score_fn, ds, sde, ts, chunk=args.chunk, net_input_dtype=torch.bfloat16)
cl = (sb.transition_sampler, sb.transition_logpdf, sb.likelihood_logpdf)
first_case = True


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        print(f"# {fn.__name__} {out[-1]:.1f} ms", file=sys.stderr, flush=True)
    return (statistics.median(out), min(out), max(out)) if out else None


for marg in (bool(int(s)) for s in args.marg_y.split(",")):
    for N in (int(s) for s in args.nparticles.split(",")):
        for B in (int(s) for s in args.batches.split(",")):
            masks = [ds.gen_mask(ops.PRNGKey(100 + b)) for b in range(B)]
            y0s = [ds.unpack(ops.uniform(ops.PRNGKey(200 + b), (28, 28, 1), device=dev), masks[b])[1] for b in range(B)]
            x0s = torch.zeros((B, 225, 1), device=dev)
            bs = np.zeros((B, T + 1), np.int32)
            count = [0]

            def keys():
                count[0] += 1
                return ops.split(ops.PRNGKey(count[0]), B)

            def batched():
                gibbs_kernel_batched(keys(), x0s, y0s, None, bs, ts, sb.fwd_sampler, sde, sb.unpack, N, *cl, marg_y=marg,
                                     explicit_backward=False, mask_=masks)

            def loop():
                k = keys()
                for b in range(B):
                    gibbs_kernel(k[b], x0s[b], y0s[b], None, bs[b], ts, sb.fwd_sampler, sde, sb.unpack, N, *cl, marg_y=marg,
                                 explicit_backward=False, mask_=masks[b])

            if first_case:                                    # a fresh process runs its first dozen sweeps ~10 % slow
                timed(batched, 0, args.process_warmup)
                first_case = False
            ms_b, lo_b, hi_b = timed(batched, args.sweeps, args.warmup)
            ms_l, lo_l, hi_l = timed(loop, args.sweeps, args.warmup)
            line = json.dumps({
                "workload": f"MNIST inpaint-15, UNet dim 64 (random init) bf16, gibbs{'-marg_y' if marg else ''}, "
                            f"{N} particles, {T} steps",
                "marg_y": marg, "B": B, "nparticles": N, "nsteps": T, "sweeps": args.sweeps,
                "batched_ms_per_sweep": ms_b, "batched_ms_min": lo_b, "batched_ms_max": hi_b,
                "loop_ms_per_sweep": ms_l, "loop_ms_min": lo_l, "loop_ms_max": hi_l,
                "batched_ms_per_ensemble_step": ms_b / (B * T), "loop_ms_per_ensemble_step": ms_l / (B * T),
                "speedup": ms_l / ms_b, "chunk": args.chunk})
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
