"""Image backward smoother batched over ensembles: gibbs_init_batched(method='smoother') with smoother='loop' (the backward
smoother per ensemble), 'lockstep' (one network call per step for all ensembles) and 'reuse' (the filter's network outputs
kept: no network call in the backward pass), in one process on one card.  MNIST inpaint-15, UNet dim 64 (random init), bf16
autocast, a short grid -- the method of tools/bench_images_filter_batched.py.  Per case: warm-up of all three, then the
median over `--reps` runs of each; the whole init and, timed on its own on the stored particles of one filter, the backward
pass; time per run and per ensemble-step; and the number of network calls either made in one run.  One JSON line per case.
Not the headline benchmark."""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbs_amd import ops
from fbs_amd.images import ImageRestore
from fbs_amd.samplers import (bootstrap_backward_smoother_batched, bootstrap_filter_batched, gibbs_init_batched,
                              stratified)
from fbs_amd.samplers.smc import bootstrap_backward_smoother
from fbs_amd.score import ScoreBridge
from fbs_amd.sdes import StationaryLinLinearSDE
from fbs_amd.unet import UNet

ap = argparse.ArgumentParser()
ap.add_argument("--nparticles", default="10,100")
ap.add_argument("--batches", default="1,4,16,64")
ap.add_argument("--nsteps", type=int, default=20)
ap.add_argument("--reps", type=int, default=10, help="timed runs per mode (the median is reported)")
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
MODES = ("loop", "lockstep", "reuse")


def timed(fns, reps, warmup):
    """fns: name -> callable.  All warmed up first, then timed in turn -> name -> (median ms, min ms, max ms, network calls)."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    res = {}
    for name, fn in fns.items():
        out = []
        for _ in range(reps):
            ncalls[0] = 0
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        print(f"# {name} " + " ".join(f"{x:.1f}" for x in out) + " ms", file=sys.stderr, flush=True)
        res[name] = (statistics.median(out), min(out), max(out), ncalls[0])
    return res


for N in (int(s) for s in args.nparticles.split(",")):
    for B in (int(s) for s in args.batches.split(",")):
        masks = [ds.gen_mask(ops.PRNGKey(100 + b)) for b in range(B)]
        y0s = [ds.unpack(ops.uniform(ops.PRNGKey(200 + b), (28, 28, 1), device=dev), masks[b])[1] for b in range(B)]
        count = [0]

        def keys():
            count[0] += 1
            return ops.split(ops.PRNGKey(count[0]), B)

        def init(mode):
            return lambda: gibbs_init_batched(keys(), y0s, (225, 1), ts, sb.fwd_sampler, sde, sb.unpack, sb.transition_sampler,
                                              sb.transition_logpdf, sb.likelihood_logpdf, N, method="smoother", marg_y=True,
                                              smoother=mode, mask_=masks)

        # the backward pass alone, on the stored particles and network outputs of one filter
        yss = torch.stack([sb.fwd_ys_sampler(ops.PRNGKey(300 + b), y0s[b]) for b in range(B)], 0)
        vss = torch.flip(yss, [1])
        uss, _ = bootstrap_filter_batched(sb.transition_sampler, sb.likelihood_logpdf, vss, ts, sb.ref_sampler,
                                          ops.split(ops.PRNGKey(7), B), N, stratified, return_last=False, mask_=masks)
        mb = sb.em_mask_batch(masks, B)
        kept = torch.stack([sb._network_batched(uss[:, t].contiguous().reshape(B, N, -1), None,
                                                vss[:, t].contiguous().reshape(B, -1), ts[t], mb).clone() for t in range(T)], 0)

        def back_loop():
            k = keys()
            for b in range(B):
                bootstrap_backward_smoother(k[b], uss[b], vss[b], ts, sb.transition_logpdf, mask_=masks[b])

        back = {"loop": back_loop,
                "lockstep": lambda: bootstrap_backward_smoother_batched(keys(), uss, vss, ts, sb.transition_logpdf, mask_=masks),
                "reuse": lambda: bootstrap_backward_smoother_batched(keys(), uss, vss, ts, sb.transition_logpdf,
                                                                     network_outputs=kept, mask_=masks)}
        r_back = timed({"backward " + m: back[m] for m in MODES}, args.reps, args.warmup)
        r_init = timed({"init " + m: init(m) for m in MODES}, args.reps, args.warmup)
        row = {"workload": f"MNIST inpaint-15, UNet dim 64 (random init) bf16, gibbs_init smoother, {N} particles, {T} steps",
               "B": B, "nparticles": N, "nsteps": T, "reps": args.reps, "chunk": args.chunk,
               "store_bytes": int(kept.numel() * kept.element_size())}
        for m in MODES:
            for part, res in (("backward", r_back), ("init", r_init)):
                med, lo, hi, calls = res[f"{part} {m}"]
                row[f"{part}_{m}_ms"] = med
                row[f"{part}_{m}_ms_min_max"] = [lo, hi]
                row[f"{part}_{m}_ms_per_ensemble_step"] = med / (B * T)
                row[f"{part}_{m}_network_calls"] = calls
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
