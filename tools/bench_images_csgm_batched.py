"""The image CSGM sampler batched over trajectories: make_image_csgm_batched against the loop of the unchanged
make_image_csgm over the same B trajectories, both in one process on one card.  MNIST inpaint-15, UNet dim 64 (random
init), bf16 autocast, a short grid -- the method of tools/bench_images_batched.py.  Per B: warm-up, then the median over
`--reps` runs of either path; time per run and per trajectory-step; and the number of network calls either path made in
one run.  One JSON line per B.  Every B runs in a child process of its own under its own time limit, and the first child
that fails or runs out of time ends the tool: nothing more is started on the card.  Not the headline benchmark."""
import argparse, json, os, statistics, subprocess, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,4,16,64,256")
ap.add_argument("--nsteps", type=int, default=20)
ap.add_argument("--reps", type=int, default=10, help="timed runs per path (the median is reported)")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--chunk", type=int, default=4096, help="rows per network call: at least B = one call per step")
ap.add_argument("--fp32_input", action="store_true",
                help="write the batched path's network input in float32, as the loop does (default: bfloat16)")
ap.add_argument("--limit", type=float, default=0.0,
                help="seconds a child may run (0: 60 + 0.012 * B * nsteps * (reps + warmup), twice the loop's expected time)")
ap.add_argument("--out", default="", help="also append the JSON lines to this file")
ap.add_argument("--case", type=int, default=0, help="(internal) run this B in this process")
args = ap.parse_args()

if not args.case:
    for B in (int(s) for s in args.batches.split(",")):
        limit = args.limit or 60 + 0.012 * B * args.nsteps * (args.reps + args.warmup)
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(B), "--nsteps", str(args.nsteps), "--reps", str(args.reps),
               "--warmup", str(args.warmup), "--chunk", str(args.chunk), "--out", args.out]
        if args.fp32_input:
            cmd.append("--fp32_input")
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"B = {B}: no result within {limit:.0f} s; stopping")
        if rc != 0:
            sys.exit(f"B = {B}: exit status {rc}; stopping")
    sys.exit(0)

import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbs_amd import ops
from fbs_amd.csgm import make_image_csgm, make_image_csgm_batched
from fbs_amd.images import ImageRestore
from fbs_amd.sdes import StationaryLinLinearSDE
from fbs_amd.unet import UNet

dev = torch.device("cuda:0")
B, Tend, T = args.case, 2.0, args.nsteps
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


single = make_image_csgm(score_fn, ds, sde, ts)
lockstep = make_image_csgm_batched(score_fn, ds, sde, ts, chunk=args.chunk,
                                   net_input_dtype=torch.float32 if args.fp32_input else torch.bfloat16)
masks = [ds.gen_mask(ops.PRNGKey(100 + b)) for b in range(B)]
y0s = [ds.unpack(ops.uniform(ops.PRNGKey(200 + b), (28, 28, 1), device=dev), masks[b])[1] for b in range(B)]
count = [0]


def keys():
    count[0] += 1
    return ops.split(ops.PRNGKey(count[0]), B)


def batched():
    lockstep(keys(), y0s, masks)


def loop():
    k = keys()
    for b in range(B):
        single(k[b], y0s[b], masks[b])


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
        print(f"# B={B} {fn.__name__} {out[-1]:.1f} ms", file=sys.stderr, flush=True)
    return statistics.median(out), ncalls[0]


ms_b, calls_b = timed(batched, args.reps, args.warmup)
ms_l, calls_l = timed(loop, args.reps, args.warmup)
line = json.dumps({
    "workload": f"MNIST inpaint-15, UNet dim 64 (random init) bf16, csgm, {T} steps",
    "method": "csgm", "B": B, "nsteps": T, "reps": args.reps, "batched_ms": ms_b, "loop_ms": ms_l,
    "batched_ms_per_trajectory_step": ms_b / (B * T), "loop_ms_per_trajectory_step": ms_l / (B * T),
    "speedup": ms_l / ms_b, "batched_network_calls": calls_b, "loop_network_calls": calls_l, "chunk": args.chunk,
    "batched_input": "float32" if args.fp32_input else "bfloat16"})
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
