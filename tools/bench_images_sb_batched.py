"""Image forward paths batched over ensembles: gibbs_kernel_batched with the bridge's own fwd_sampler (the forward noising
paths of all B ensembles drawn in lockstep, ScoreBridge.fwd_sampler_batched) against the same call with fwd_sampler wrapped in
a plain lambda (the paths drawn one ensemble at a time around the same lockstep SMC loop), in one process on one card.
MNIST supr-4, UNet dim 64 (random init), bf16 autocast, explicit_backward and explicit_final on, a short grid.  First the
Schrodinger-bridge model (mode 'drift': a path is T calls of the forward network), then the score model (a path is a handful
of launches).  Per case: warm-up, then the median over `--sweeps` sweeps of either path, the forward-network calls of a
sweep, and for B = 1 the spread of the per-ensemble path's own sweeps.  One JSON line per case.  Not the headline
benchmark."""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbs_amd import ops
from fbs_amd.images import ImageRestore
from fbs_amd.samplers import gibbs_kernel_batched
from fbs_amd.score import ScoreBridge
from fbs_amd.sdes import StationaryLinLinearSDE
from fbs_amd.unet import UNet

ap = argparse.ArgumentParser()
ap.add_argument("--nparticles", type=int, default=10)
ap.add_argument("--batches", default="1,4,16,64")
ap.add_argument("--modes", default="drift,score")
ap.add_argument("--nsteps", type=int, default=20)
ap.add_argument("--sweeps", type=int, default=10, help="timed sweeps per path (the median is reported)")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--process-warmup", type=int, default=12, help="untimed sweeps before the first case of the process")
ap.add_argument("--chunk", type=int, default=8192, help="rows per network call: at least B * rows = one call per step")
ap.add_argument("--out", default="", help="also append the JSON lines to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
T, N = args.nsteps, args.nparticles
torch.manual_seed(0)
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
    return out


for mode in args.modes.split(","):
    Tend = 0.5 if mode == "drift" else 2.0
    ts = np.linspace(0, Tend, T + 1)
    sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=Tend)
    ds = ImageRestore("supr-4", (28, 28, 1), sr_random=mode != "drift", device=dev)
    mk = lambda: UNet(dt=Tend / 200, dim=64, in_channels=1, upsampling="pixel_shuffle").to(dev).eval()
    net, net_fwd = mk(), (mk() if mode == "drift" else None)
    fwd_calls = [0]

    def run(module, x, t):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return module(x, t)

    def fwd_rows(x, t):
        fwd_calls[0] += 1
        return run(net_fwd, x, t)

    def fwd_one(x, t):
        fwd_calls[0] += 1
        return run(net_fwd, x.unsqueeze(0), t).float().reshape(x.shape)

    kw = dict(mode="drift", fwd_drift_fn=fwd_one, fwd_drift_rows_fn=fwd_rows) if mode == "drift" else {}
    sb = ScoreBridge(lambda x, t: run(net, x, t), ds, sde, ts, chunk=args.chunk, net_input_dtype=torch.bfloat16, **kw)
    cl = (sb.transition_sampler, sb.transition_logpdf, sb.likelihood_logpdf)
    wrapped = lambda *a, **k: sb.fwd_sampler(*a, **k)        # not the bridge's own method: the per-ensemble paths
    for B in (int(s) for s in args.batches.split(",")):
        masks = [ds.gen_mask(ops.PRNGKey(100 + b)) for b in range(B)]
        y0s = [ds.unpack(ops.uniform(ops.PRNGKey(200 + b), (28, 28, 1), device=dev), masks[b])[1] for b in range(B)]
        x0s = torch.zeros((B,) + tuple(ds.unobs_shape), device=dev)
        bs = np.zeros((B, T + 1), np.int32)
        count = [0]

        def sweep(fwd):
            count[0] += 1
            gibbs_kernel_batched(ops.split(ops.PRNGKey(count[0]), B), x0s, y0s, None, bs, ts, fwd, sde, sb.unpack, N, *cl,
                                 explicit_backward=True, explicit_final=True, mask_=masks)

        def lockstep_paths():
            sweep(sb.fwd_sampler)

        def per_ensemble_paths():
            sweep(wrapped)

        if first_case:                                        # a fresh process runs its first dozen sweeps ~10 % slow
            timed(lockstep_paths, 0, args.process_warmup)
            first_case = False
        ms_b = timed(lockstep_paths, args.sweeps, args.warmup)
        ms_l = timed(per_ensemble_paths, args.sweeps, args.warmup)
        fwd_calls[0] = 0
        lockstep_paths()
        calls_b, fwd_calls[0] = fwd_calls[0], 0
        per_ensemble_paths()
        calls_l = fwd_calls[0]
        mb, ml = statistics.median(ms_b), statistics.median(ms_l)
        line = json.dumps({
            "workload": f"MNIST supr-4, {'SB (drift)' if mode == 'drift' else 'score'} model, UNet dim 64 (random init) bf16, "
                        f"gibbs-eb-ef, {N} particles, {T} steps",
            "mode": mode, "B": B, "nparticles": N, "nsteps": T, "sweeps": args.sweeps,
            "lockstep_paths_ms_per_sweep": mb, "per_ensemble_paths_ms_per_sweep": ml, "speedup": ml / mb,
            "lockstep_paths_ms_per_ensemble": mb / B, "per_ensemble_paths_ms_per_ensemble": ml / B,
            "per_ensemble_paths_min_max_ms": [min(ms_l), max(ms_l)], "lockstep_paths_min_max_ms": [min(ms_b), max(ms_b)],
            "fwd_network_calls_per_sweep": {"lockstep": calls_b, "per_ensemble": calls_l}, "chunk": args.chunk})
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
