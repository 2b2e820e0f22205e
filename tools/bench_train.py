"""Time one training step of the score network (fbs_amd.train.make_adam_kernel on fbs_amd.sdes.make_linear_sde_law_loss,
save_mem) against a torch-only restatement in the same process, and the trainer's own kernels alone.

Shape: MNIST, 28 x 28 x 1, UNet dim 64, batch 64, float32 and bfloat16 autocast.  The restatement draws its noise with
torch.randn, forms the loss with torch operations, steps torch.optim.Adam and blends the EMA with torch._foreach_*; it gets
a copy of the same initial weights, and like the trainer it keeps the library convolutions out of its differentiable pass
(fbs_amd.train.torch_own_convolutions).  The two alternate step by step; the medians of --runs steps after a warm-up of both are
reported, timed by device events round a whole step (the host work of a step is inside, the queue is drained before).  Then
the noise, loss and update kernels alone, and the update kernel's bytes -- nine vector passes of 4 P bytes: p, m, v, ema read
and written, g read -- over its time as a share of the 8 TB/s HBM peak.  Reported, not gated.  Prints one JSON line.

    python tools/bench_train.py [--runs 10] [--dim 64] [--batch 64]
"""
import argparse
import copy
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--batch", type=int, default=64)
    args = p.parse_args(argv)
    import torch
    from fbs_amd import ops
    from fbs_amd.sdes import StationaryLinLinearSDE, make_linear_sde_law_loss
    from fbs_amd.sdes.linear import discretise_linear_sde_np
    from fbs_amd.sdes.losses import dsm_loss_batched, dsm_noise_batched, dsm_tables, upload
    from fbs_amd.train import adam_ema_step, make_adam_kernel, sqnorm, torch_own_convolutions
    from fbs_amd.unet import UNet
    if not torch.cuda.is_available():
        raise RuntimeError("bench_train needs a GPU: the trainer has no CPU path")
    dev = torch.device("cuda:0")
    B, shape, T = args.batch, (28, 28, 1), 2.0
    D = int(np.prod(shape))
    rng = np.random.default_rng(0)
    data = torch.from_numpy(rng.uniform(size=(256,) + shape).astype(np.float32)).to(dev)
    sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5., t0=0., T=T)
    keys = ops.split(ops.PRNGKey(7), 4096)

    def event_ms(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    rows = []
    for bf16 in (False, True):
        torch.manual_seed(0)
        net = UNet(dt=T / 200, dim=args.dim, in_channels=1, upsampling='pixel_shuffle').to(dev)
        ref = copy.deepcopy(net)

        def run(module, x, t):
            if bf16:
                with torch.autocast('cuda', dtype=torch.bfloat16):
                    return module(x, t)
            return module(x, t)

        loss_fn = make_linear_sde_law_loss(sde, lambda x, t, prm: run(net, x, t), t0=0., T=T, random_times=True, save_mem=True)
        step, ema_kernel = make_adam_kernel(net, loss_fn, 2e-4, grad_clip=1.0)
        idx = torch.arange(B, dtype=torch.int32, device=dev)
        count = {"k": 0}

        def ours():
            ema_kernel(400 + count["k"], 300, 2, 0.99)
            step(keys[count["k"]], data, idx)
            count["k"] += 1

        # the torch-only restatement: the same step with library operations only
        opt = torch.optim.Adam(ref.parameters(), lr=2e-4)
        ref_params = [q for q in ref.parameters()]
        ref_ema = [q.detach().clone() for q in ref_params]
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        rcount = {"k": 0}

        def theirs():
            ts = np.sort(np.random.default_rng(rcount["k"]).uniform(1e-5, T, B)).astype(np.float32)
            F, Q = discretise_linear_sde_np(sde, ts.astype(np.float64), 0.0)
            Ft, Qt, tt = (torch.from_numpy(np.asarray(a, np.float32)).to(dev, non_blocking=True) for a in (F, Q, ts))
            x0 = data[idx.long()]
            xi = torch.randn(x0.shape, device=dev, generator=gen)
            sh = (-1, 1, 1, 1)
            xt = Ft.reshape(sh) * x0 + torch.sqrt(Qt).reshape(sh) * xi
            opt.zero_grad(set_to_none=True)
            with torch_own_convolutions():                               # as the trainer's differentiable pass
                out = run(ref, xt, tt).float()
                cs = -(xt - Ft.reshape(sh) * x0) / Qt.reshape(sh)
                loss = torch.mean(torch.mean((out - cs) ** 2, dim=(1, 2, 3)) * Qt)
                loss.backward()
            torch.nn.utils.clip_grad_norm_(ref_params, 1.0)
            opt.step()
            if (400 + rcount["k"]) % 2 == 0:
                with torch.no_grad():
                    torch._foreach_mul_(ref_ema, 0.99)
                    torch._foreach_add_(ref_ema, ref_params, alpha=0.01)
            rcount["k"] += 1

        for _ in range(args.warmup):
            ours()
            theirs()
        t_ours, t_theirs = [], []
        for _ in range(args.runs):
            t_ours.append(event_ms(ours))
            t_theirs.append(event_ms(theirs))

        # the trainer's kernels alone
        fp, st = step.params, step.state
        P = fp.numel
        ts = np.linspace(0.1, T, B).astype(np.float32)
        F, sq, gc = dsm_tables(sde, ts, 0.0, B * D)
        keys_d, F_d, sq_d, gc_d = upload(dev, keys[:B].view(np.int32), F, sq, gc)
        flat = data.reshape(data.shape[0], -1)
        netout = torch.randn((B, D), device=dev).to(torch.bfloat16 if bf16 else torch.float32)
        g = torch.randn(P, device=dev) * 1e-3
        pv, mv, vv, ev = (torch.randn(P, device=dev) for _ in range(4))
        vv = vv.abs()

        def med(fn):
            for _ in range(3):
                fn()
            return statistics.median(event_ms(fn) for _ in range(args.runs))

        k_noise = med(lambda: dsm_noise_batched(flat, idx, keys_d, F_d, sq_d, torch.float32))
        k_loss = med(lambda: dsm_loss_batched(netout, 0, keys_d, None, None, None, None, sq_d, gc_d))
        k_sqn = med(lambda: sqnorm(g, st["gnorm2"]))
        k_upd = med(lambda: adam_ema_step(pv, g, mv, vv, ev, 2e-4, 0.9, 0.999, 1e-8, 5, st["gnorm2"], 1.0, 2, 0.99))
        torch_adam = torch.optim.Adam([torch.nn.Parameter(pv.clone())], lr=2e-4)
        torch_adam.param_groups[0]["params"][0].grad = g.clone()
        k_torch_upd = med(lambda: torch_adam.step())
        rows.append(dict(net="bf16" if bf16 else "f32", params=P, step_ms_median=statistics.median(t_ours),
                         step_ms_min=min(t_ours), step_ms_max=max(t_ours), torch_step_ms_median=statistics.median(t_theirs),
                         torch_step_ms_min=min(t_theirs), torch_step_ms_max=max(t_theirs), noise_kernel_ms=k_noise,
                         loss_kernels_ms=k_loss, sqnorm_kernels_ms=k_sqn, update_kernel_ms=k_upd,
                         torch_adam_step_ms=k_torch_upd, update_bytes=9 * 4 * P,
                         update_share_of_hbm_peak=9 * 4 * P / (k_upd * 1e-3) / HBM_PEAK))
        r = rows[-1]
        print(f"{r['net']:5s} P={P}: step {r['step_ms_median']:.2f} ms (min {r['step_ms_min']:.2f}, max {r['step_ms_max']:.2f}); "
              f"torch-only {r['torch_step_ms_median']:.2f} ms (min {r['torch_step_ms_min']:.2f}, max {r['torch_step_ms_max']:.2f}); "
              f"noise {k_noise * 1e3:.1f} us, loss {k_loss * 1e3:.1f} us, sqnorm {k_sqn * 1e3:.1f} us, update {k_upd * 1e3:.1f} us "
              f"= {r['update_share_of_hbm_peak']:.3f} of the HBM peak (torch.optim.Adam.step alone {k_torch_upd * 1e3:.1f} us)",
              file=sys.stderr)
    print(json.dumps(dict(tool="bench_train", gpu=torch.cuda.get_device_name(0), runs=args.runs, batch=B, shape=list(shape),
                          dim=args.dim, rows=rows)))


if __name__ == "__main__":
    main()
