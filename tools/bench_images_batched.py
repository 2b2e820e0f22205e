"""Image Gibbs sweeps batched over ensembles: gibbs_kernel_batched against the loop of the unchanged gibbs_kernel over the
same B ensembles, in one process on one card.  MNIST inpaint-15, UNet dim 64 (random init), bf16 autocast,
explicit_backward and explicit_final on, a short grid.  Per case: warm-up, then the median over `--sweeps` sweeps of either
path; time per sweep and per ensemble-step; and the time of ONE network call at `rows` and at B * rows rows -- the premise
that a call of a hundred rows leaves most of the card idle.  One JSON line per case.  Not the headline benchmark."""
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
ap.add_argument("--chunk", type=int, default=8192, help="rows per network call: at least B * rows = one call per step")
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
    return statistics.median(out)


def network_ms(rows):
    x = torch.randn((rows, 28, 28, 1), device=dev).to(torch.bfloat16)

    def network_call():
        score_fn(x, 1.0)

    return timed(network_call, 20, 3)


for N in (int(s) for s in args.nparticles.split(",")):
    rows = N + 1
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
            gibbs_kernel_batched(keys(), x0s, y0s, None, bs, ts, sb.fwd_sampler, sde, sb.unpack, N, *cl,
                                 explicit_backward=True, explicit_final=True, mask_=masks)

        def loop():
            k = keys()
            for b in range(B):
                gibbs_kernel(k[b], x0s[b], y0s[b], None, bs[b], ts, sb.fwd_sampler, sde, sb.unpack, N, *cl,
                             explicit_backward=True, explicit_final=True, mask_=masks[b])

        ms_b = timed(batched, args.sweeps, args.warmup)
        ms_l = timed(loop, args.sweeps, args.warmup)
        line = json.dumps({
            "workload": f"MNIST inpaint-15, UNet dim 64 (random init) bf16, gibbs-eb-ef, {N} particles ({rows} rows), {T} steps",
            "B": B, "nparticles": N, "rows": rows, "nsteps": T, "sweeps": args.sweeps,
            "batched_ms_per_sweep": ms_b, "loop_ms_per_sweep": ms_l,
            "batched_ms_per_ensemble_step": ms_b / (B * T), "loop_ms_per_ensemble_step": ms_l / (B * T),
            "speedup": ms_l / ms_b,
            "network_ms_rows": network_ms(rows), "network_ms_B_rows": network_ms(B * rows), "chunk": args.chunk})
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
