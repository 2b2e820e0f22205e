"""The image twisted SMC batched over ensembles: make_image_twisted_batched against the loop of the unchanged
make_image_twisted(...).conditional_sampler over the same B ensembles, both in one process on one card.  MNIST inpaint-15,
UNet dim 64 (random init), bf16 autocast, a short grid, stratified resampling -- the method of
tools/bench_images_csgm_batched.py.  Per (B, particles): warm-up, then the median over `--reps` runs of either path; time
per run and per ensemble-step; the loop's own run-to-run spread (its fastest and slowest run); and the number of network
passes either path made in one run (a pass = one call of the score function: the loop makes three per step and ensemble,
two forward and one forward + backward; lockstep two per step for all ensembles, one of them forward + backward).  One
JSON line per case.  Every case runs in a child process of its own under its own time limit, and the first child that
fails or runs out of time ends the tool: nothing more is started on the card.  Not the headline benchmark."""
import argparse, json, os, statistics, subprocess, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,4,16,64")
ap.add_argument("--particles", default="10,100")
ap.add_argument("--nsteps", type=int, default=20)
ap.add_argument("--reps", type=int, default=10, help="timed runs per path (the median is reported)")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--chunk", type=int, default=4096, help="rows per network call: at least B * particles = one call per pass")
ap.add_argument("--fp32_input", action="store_true",
                help="the no-grad pass reads the float32 particles, as the loop does (default: a bfloat16 copy)")
ap.add_argument("--limit", type=float, default=0.0,
                help="seconds a child may run (0: 120 + 0.012 * max(particles, 10) * B * nsteps * (reps + warmup), twice "
                     "the expected time of both paths)")
ap.add_argument("--out", default="", help="also append the JSON lines to this file")
ap.add_argument("--case", default="", help="(internal) 'B,particles': run this case in this process")
args = ap.parse_args()

if not args.case:
    for n in (int(s) for s in args.particles.split(",")):
        for B in (int(s) for s in args.batches.split(",")):
            limit = args.limit or 120 + 0.012 * max(n, 10) * B * args.nsteps * (args.reps + args.warmup)
            cmd = [sys.executable, os.path.abspath(__file__), "--case", f"{B},{n}", "--nsteps", str(args.nsteps), "--reps",
                   str(args.reps), "--warmup", str(args.warmup), "--chunk", str(args.chunk), "--out", args.out]
            if args.fp32_input:
                cmd.append("--fp32_input")
            try:
                rc = subprocess.run(cmd, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                sys.exit(f"B = {B}, {n} particles: no result within {limit:.0f} s; stopping")
            if rc != 0:
                sys.exit(f"B = {B}, {n} particles: exit status {rc}; stopping")
    sys.exit(0)

import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbs_amd import ops
from fbs_amd.images import ImageRestore
from fbs_amd.samplers import stratified
from fbs_amd.sdes import StationaryLinLinearSDE
from fbs_amd.twisted import make_image_twisted, make_image_twisted_batched
from fbs_amd.unet import UNet

dev = torch.device("cuda:0")
B, n = (int(s) for s in args.case.split(","))
Tend, T = 2.0, args.nsteps
ts = np.linspace(0, Tend, T + 1)
sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=Tend)
ds = ImageRestore("inpaint-15", (28, 28, 1), device=dev)
torch.manual_seed(0)
net = UNet(dt=Tend / 200, dim=64, in_channels=1, upsampling="pixel_shuffle").to(dev).eval()
ncalls = [0]


def score_fn(x, t):                                                  # differentiable: the callers decide about no_grad
    ncalls[0] += 1
    with torch.autocast("cuda", dtype=torch.bfloat16):
        return net(x, t).float().reshape(x.shape)


single = make_image_twisted(score_fn, ds, sde, ts, n)
lockstep = make_image_twisted_batched(score_fn, ds, sde, ts, n, chunk=args.chunk,
                                      net_input_dtype=torch.float32 if args.fp32_input else torch.bfloat16)
masks = [ds.gen_mask(ops.PRNGKey(100 + b)) for b in range(B)]
y0s = [ds.unpack(ops.uniform(ops.PRNGKey(200 + b), (28, 28, 1), device=dev), masks[b])[1] for b in range(B)]
count = [0]


def keys():
    count[0] += 1
    return ops.split(ops.PRNGKey(count[0]), B)


def batched():
    lockstep.conditional_sampler_batched(keys(), y0s, masks, stratified)


def loop():
    k = keys()
    for b in range(B):
        single.conditional_sampler(k[b], y0s[b], stratified, mask_=masks[b])


def timed(fn, reps, warmup):
    """-> (median ms, fastest, slowest, network passes of one run)"""
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
        print(f"# B={B} n={n} {fn.__name__} {out[-1]:.1f} ms", file=sys.stderr, flush=True)
    return statistics.median(out), min(out), max(out), ncalls[0]


ms_b, lo_b, hi_b, calls_b = timed(batched, args.reps, args.warmup)
ms_l, lo_l, hi_l, calls_l = timed(loop, args.reps, args.warmup)
line = json.dumps({
    "workload": f"MNIST inpaint-15, UNet dim 64 (random init) bf16, twisted, {T} steps, stratified",
    "method": "twisted", "B": B, "particles": n, "nsteps": T, "reps": args.reps, "batched_ms": ms_b, "loop_ms": ms_l,
    "batched_ms_min_max": [lo_b, hi_b], "loop_ms_min_max": [lo_l, hi_l],
    "batched_ms_per_ensemble_step": ms_b / (B * T), "loop_ms_per_ensemble_step": ms_l / (B * T),
    "speedup": ms_l / ms_b, "batched_network_passes": calls_b, "loop_network_passes": calls_l, "chunk": args.chunk,
    "batched_input": "float32" if args.fp32_input else "bfloat16"})
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
