"""Image inpainting / super-resolution with the forward-backward samplers on MI355X.

Counterpart of the reference drivers experiments/imgs/inpainting.py and experiments/imgs/supr.py (they differ by the
mask only; here `--task inpaint` / `--task supr`) and, with `--sb`, of experiments/sb_imgs/supr.py: same command-line
flags, same key schedule, same result arrays (`*-gibbs-eb-ef.npy`, `*-filter.npy`, `*-pmcmc-<delta>.npy` of shape
(nsamples, H, W, C)), written against fbs_amd.  `--method twisted` is experiments/imgs/inpainting_twisted.py (the twisted-SMC
baseline: whole-image particles, the twisting function's gradient through the score network by torch.autograd; result
`*-twisted.npy`), `--method csgm` experiments/imgs/inpainting_csgm.py / supr_csgm.py (conditional score-based sampling: one
reverse-SDE trajectory with the observed pixels re-noised every step; `*-csgm.npy`).  The closures are the bound methods of one fbs_amd.score.ScoreBridge, so
every SMC step is two HIP kernels around one network evaluation (PyTorch-ROCm).  With `--batch B` the test images of the
gibbs*, filter and pmcmc* methods advance in groups of B, one network evaluation per step for the group (fbs_amd.samplers
gibbs_kernel_batched, gibbs_init_batched, pmcmc_kernel_batched); every image keeps the keys of the sequential run.  With
`--batch_init --init_method smoother` the initialiser's backward smoother advances in lockstep too, on the network outputs
its filter kept (`--init_smoother` chooses otherwise).  With
`--method csgm --batch B` the (image, sample) trajectories of the run advance in groups of B (fbs_amd.csgm
make_image_csgm_batched), each with the key of the sequential run; with `--method twisted --batch B` the (image, sample)
twisted-SMC runs do (fbs_amd.twisted make_image_twisted_batched: the same keys and draws, its own specified arithmetic).

The reference loads a trained checkpoint (`./checkpoints/<dataset>_<sde>_<epoch>.npz`, a flat `param` / `ema_param`
vector in ravel_pytree order) and a dataset (`../datasets/mnist.npz`, `datasets/celeba_hq<res>.npy`); neither exists in
this environment.  If the files are there they are used (fbs_amd.unet.UNet.load_flat_params); otherwise the network is
randomly initialised and the test image is uniform noise -- the sampler runs the same either way (PNG output is left
out: matplotlib is not a dependency).

With `--metrics` every group's restored block is scored on the device against its test image before it is saved
(fbs_amd.image_metrics): `<result file>-metrics.npz` holds `psnr` and `ssim` per sample and, for the gibbs* and pmcmc* chains,
`autocorr_best`, the best variable's autocorrelation curve.  examples/tabulate_imgs.py tabulates the result files.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbs_amd import ops  # noqa: E402
from fbs_amd.images import ImageRestore  # noqa: E402
from fbs_amd.samplers import (gibbs_init, gibbs_init_batched, gibbs_kernel, gibbs_kernel_batched, pmcmc_kernel,  # noqa: E402
                              pmcmc_kernel_batched, stratified)
from fbs_amd.score import ScoreBridge  # noqa: E402
from fbs_amd.sdes import StationaryConstLinearSDE, StationaryLinLinearSDE  # noqa: E402
from fbs_amd.unet import UNet  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser(description='Inpainting / super-resolution.')
    p.add_argument('--task', type=str, default='inpaint', help='inpaint (inpainting.py) or supr (supr.py).')
    p.add_argument('--sb', action='store_true', help='Schrodinger-bridge model (experiments/sb_imgs/supr.py).')
    p.add_argument('--dataset', type=str, default='mnist', help="'mnist' or 'celeba-64' / 'celeba-128'.")
    p.add_argument('--rect_size', type=int, default=15, help='The w/h of the inpainting rectangle.')
    p.add_argument('--rate', type=int, default=4, help='The rate of super-resolution.')
    p.add_argument('--sde', type=str, default='lin')
    p.add_argument('--test_nsteps', type=int, default=200)
    p.add_argument('--test_epoch', type=int, default=2999)
    p.add_argument('--sb_step', type=int, default=9)
    p.add_argument('--test_ema', action='store_true', default=False)
    p.add_argument('--test_seed', type=int, default=666)
    p.add_argument('--ny0s', type=int, default=10)
    p.add_argument('--start_from', type=int, default=0)
    p.add_argument('--nparticles', type=int, default=100)
    p.add_argument('--nsamples', type=int, default=100)
    p.add_argument('--method', type=str, default='gibbs-eb-ef', help="'filter', 'gibbs[-eb][-ef]', 'pmcmc[-delta]', 'twisted', 'csgm'.")
    p.add_argument('--init_method', type=str, default='filter')
    p.add_argument('--marg', action='store_true', default=False, help='Whether marginalise out the Y path.')
    p.add_argument('--dim', type=int, default=64, help='UNet width (64 in the reference).')
    p.add_argument('--fp32', action='store_true', help='float32 network instead of bf16 autocast.')
    p.add_argument('--chunk', type=int, default=4096, help='Particles per network call (a power of two: MIOpen ships kernels for those batch sizes; bigger calls are faster per particle).')
    p.add_argument('--batch', type=int, default=1, help="'filter', 'gibbs*' and 'pmcmc*' methods: test images that advance together, one network call per step for all of them; 'csgm': (image, sample) trajectories that advance together, one launch and one network call per step; 'twisted': (image, sample) twisted-SMC runs that advance together, six launches and two network passes per step (1: one at a time).")
    p.add_argument('--batch_init', action='store_true', help="With --batch and a gibbs* method: the images' gibbs_init filters advance together too (gibbs_init_batched); by default gibbs_init runs per image.")
    p.add_argument('--init_smoother', type=str, default=None, choices=('loop', 'lockstep', 'reuse'), help="With --batch_init and --init_method smoother: how the backward smoother runs behind the batched filter (gibbs_init_batched's `smoother`). Default 'reuse': no network call in the backward pass.")
    p.add_argument('--outdir', type=str, default='./imgs/results')
    p.add_argument('--metrics', action='store_true', help="Score every restored image on the device against its test image (fbs_amd.image_metrics) and write <result file>-metrics.npz next to it: psnr and ssim (nsamples,), and for the gibbs* and pmcmc* chains autocorr_best (lags,).")
    p.add_argument('--metrics_max_lags', type=int, default=20, help='With --metrics: lags of autocorr_best (at most nsamples).')
    p.add_argument('--quiet', action='store_true')
    args = p.parse_args(argv)

    dev = torch.device('cuda:0')
    resolution = 28 if args.dataset == 'mnist' else int(args.dataset.split('-')[-1])
    nchannels = 1 if args.dataset == 'mnist' else 3
    task = f'inpaint-{args.rect_size}' if args.task == 'inpaint' else f'supr-{args.rate}'
    key = ops.PRNGKey(args.test_seed)                                              # inpainting.py:54-55
    key, data_key = ops.split(key)
    T = 0.5 if args.sb else 2.0                                                    # sb_imgs/supr.py:46 / inpainting.py:57
    nsteps = args.test_nsteps
    ts = np.linspace(0, T, nsteps + 1)
    key, subkey = ops.split(key)                                                   # the dataset's key (unused without data)
    ds = ImageRestore(task, (resolution, resolution, nchannels), sr_random=not args.sb, device=dev)
    sde = StationaryConstLinearSDE(a=-0.5, b=1.) if args.sde == 'const' else \
        StationaryLinLinearSDE(beta_min=0.02, beta_max=5., t0=0., T=T)
    key, subkey = ops.split(key)                                                   # the network's init key

    # the trained model(s): flat parameter vectors in ravel_pytree order, if present
    torch.manual_seed(args.test_seed)
    mk = lambda: UNet(dt=T / 200, dim=args.dim, in_channels=nchannels, upsampling='pixel_shuffle').to(dev).eval()
    net, net_fwd = mk(), (mk() if args.sb else None)
    ck = f'./checkpoints/sb_{args.dataset}_{args.sde}_{args.sb_step}.npz' if args.sb else \
        f'./checkpoints/{args.dataset}_{args.sde}_{args.test_epoch}.npz'
    if os.path.exists(ck):
        z = np.load(ck)
        if args.sb:
            net_fwd.load_flat_params(z['param_fwd'])
            net.load_flat_params(z['param_bwd'])
        else:
            net.load_flat_params(z['ema_param' if args.test_ema else 'param'])
    elif not args.quiet:
        print(f'no checkpoint at {ck}: randomly initialised network')

    def run(module, x, t):
        with torch.no_grad():
            if args.fp32:
                return module(x, t)
            with torch.autocast('cuda', dtype=torch.bfloat16):
                return module(x, t)

    sb = ScoreBridge(lambda x, t: run(net, x, t), ds, sde, ts, chunk=args.chunk, mode='drift' if args.sb else 'score',
                     net_input_dtype=torch.float32 if args.fp32 else torch.bfloat16,
                     fwd_drift_fn=(lambda x, t: run(net_fwd, x.unsqueeze(0), t).float().reshape(x.shape)) if args.sb else None,
                     fwd_drift_rows_fn=(lambda x, t: run(net_fwd, x, t)) if args.sb else None)
    x_shape = tuple(ds.unobs_shape)
    delta = float(args.method.split('-')[-1]) if ('pmcmc' in args.method and len(args.method.split('-')) > 1) else None
    eb, ef = ('eb' in args.method, 'ef' in args.method) if 'gibbs' in args.method else (True, True)
    if args.sb:
        eb = ef = True                                                             # sb_imgs/supr.py:169-172
    cl = dict(transition_sampler=sb.transition_sampler, transition_logpdf=sb.transition_logpdf,
              likelihood_logpdf=sb.likelihood_logpdf)
    os.makedirs(args.outdir, exist_ok=True)

    def save_metrics(paths, test_imgs, blocks):
        # --metrics: the restored blocks (len(paths), nsamples, H, W, C) against their test images, one call for all of them
        from fbs_amd.image_metrics import chain_autocorrelation, psnr_ssim
        blocks = torch.from_numpy(np.ascontiguousarray(blocks)).to(dev)
        psnr, ssim = psnr_ssim(torch.stack(list(test_imgs), 0), blocks)
        extra = [{} for _ in paths]
        if 'gibbs' in args.method or 'pmcmc' in args.method:                         # a chain: Figure 8's best variable
            lags = max(1, min(args.metrics_max_lags, args.nsamples))
            best = chain_autocorrelation(blocks.reshape(len(paths), args.nsamples, -1), lags)[1].cpu().numpy()
            extra = [dict(autocorr_best=best[b]) for b in range(len(paths))]
        psnr, ssim = psnr.cpu().numpy(), ssim.cpu().numpy()
        for b, path in enumerate(paths):
            np.savez(path + '-metrics', psnr=psnr[b], ssim=ssim[b], **extra[b])

    out = None
    if args.batch > 1 and ('gibbs' in args.method or args.method == 'filter' or 'pmcmc' in args.method):
        # Groups of --batch test images advance together (gibbs_kernel_batched, gibbs_init_batched, pmcmc_kernel_batched):
        # one network call per step for the group.  Every image keeps the keys of the sequential run: an image consumes
        # nsamples splits of the `key` chain for 'filter' (one per sample) and 1 + nsamples for gibbs (gibbs_init, then one
        # per sweep) and pMCMC (the initial observation path, then one per iteration), so its keys follow from its
        # position alone.
        is_gibbs, is_filter = 'gibbs' in args.method, args.method == 'filter'
        jobs = []
        for k in range(args.ny0s):
            data_key, subkey = ops.split(data_key)
            if k < args.start_from:
                continue
            k_img, k_mask = ops.split(subkey)
            k_first = None
            if not is_filter:
                key, k_first = ops.split(key)
            k_iters = np.zeros((args.nsamples, 2), np.uint32)
            for i in range(args.nsamples):
                key, k_iters[i] = ops.split(key)
            jobs.append((k, k_img, k_mask, k_first, k_iters))
        marg = "-marg" if args.marg else ""
        suffix = f'-gibbs{"-eb" if eb else ""}{"-ef" if ef else ""}{marg}' if is_gibbs else (
            f'-filter{marg}' if is_filter else f'-pmcmc-{delta}')
        for g0 in range(0, len(jobs), args.batch):
            group = jobs[g0:g0 + args.batch]                                       # the last group may be smaller
            nb = len(group)
            masks, y0s, heads, test_imgs = [], [], [], []
            for k, k_img, k_mask, _, _ in group:
                test_img = ops.uniform(k_img, (resolution, resolution, nchannels), device=dev)
                mask = ds.gen_mask(k_mask)
                _, test_y0 = ds.unpack(test_img, mask)
                head = os.path.join(args.outdir, f'{args.dataset}-{task}-{args.sde}-{args.nparticles}-{k}')
                np.savez(head + '-true', test_img=test_img.cpu().numpy())
                masks.append(mask), y0s.append(test_y0), heads.append(head), test_imgs.append(test_img)
            to_img = lambda b, x0: ds.concat(x0.unsqueeze(0), y0s[b], masks[b])[0].cpu().numpy()
            keys_of = lambda i: np.stack([job[4][i] for job in group], 0)
            # the smoother behind a batched init reuses the filter's network outputs unless --init_smoother says otherwise
            init = lambda keys_, method: gibbs_init_batched(keys_, y0s, x_shape, ts, sb.fwd_sampler, sde, sb.unpack,
                                                            nparticles=args.nparticles, method=method, marg_y=args.marg,
                                                            smoother=args.init_smoother or 'reuse', mask_=masks, **cl)[0]
            restored = np.zeros((nb, args.nsamples, resolution, resolution, nchannels), np.float32)
            if is_filter:
                for i in range(args.nsamples):
                    x0s = init(keys_of(i), 'filter')
                    for b in range(nb):
                        restored[b, i] = to_img(b, x0s[b])
                    if not args.quiet:
                        print(f'{task} | filter x{nb} | iter: {i}')
            elif is_gibbs:
                if args.batch_init:
                    x0s = init(np.stack([job[3] for job in group], 0), args.init_method)
                else:
                    x0s = torch.stack([gibbs_init(group[b][3], y0s[b], x_shape, ts, sb.fwd_sampler, sde, sb.unpack,   # per image
                                                  nparticles=args.nparticles, method=args.init_method, marg_y=args.marg,
                                                  mask_=masks[b], **cl)[0] for b in range(nb)], 0)
                for b in range(nb):
                    np.save(heads[b] + '-gibbs-init', to_img(b, x0s[b]))
                bs_stars = np.zeros((nb, nsteps + 1), np.int32)
                for i in range(args.nsamples):
                    x0s, _, bs_stars, acc = gibbs_kernel_batched(keys_of(i), x0s, y0s, None, bs_stars, ts, sb.fwd_sampler, sde,
                                                                 sb.unpack, args.nparticles, marg_y=args.marg,
                                                                 explicit_backward=eb, explicit_final=ef, mask_=masks, **cl)
                    for b in range(nb):
                        restored[b, i] = to_img(b, x0s[b])
                    if not args.quiet:
                        print(f'{task} | Gibbs x{nb} | iter: {i}, acc: {float(acc.float().mean()):.3f}')
            else:
                x0s = torch.zeros((nb,) + x_shape, device=dev)
                log_ells = torch.zeros(nb, device=dev)
                yss = torch.stack([sb.fwd_ys_sampler(group[b][3], y0s[b]) for b in range(nb)], 0)
                for i in range(args.nsamples):
                    x0s, log_ells, yss, st = pmcmc_kernel_batched(keys_of(i), x0s, log_ells, yss, y0s, ts, sb.fwd_ys_sampler,
                                                                  sde, sb.ref_sampler, sb.transition_sampler,
                                                                  sb.likelihood_logpdf, stratified, args.nparticles,
                                                                  delta=delta, mask_=masks)
                    for b in range(nb):
                        restored[b, i] = to_img(b, x0s[b])
                    if not args.quiet:
                        print(f'{task} | pMCMC {delta} x{nb} | iter: {i}, acc_prob: {float(st.acceptance_prob.mean()):.3f}')
            if args.metrics:
                save_metrics([head + suffix for head in heads], test_imgs, restored)
            for b in range(nb):
                np.save(heads[b] + suffix, restored[b])
            out = restored[-1]
        return out
    if args.batch > 1 and args.method == 'csgm':
        # The (image, sample) pairs of the run are one flat list of independent trajectories, taken --batch at a time
        # (make_image_csgm_batched): one launch and one network call per step for the group.  A sequential image consumes
        # nsamples splits of the `key` chain, so every trajectory's key follows from its position alone.
        from fbs_amd.csgm import make_image_csgm_batched
        sampler = make_image_csgm_batched(lambda x, t: run(net, x, t), ds, sde, ts, chunk=args.chunk,
                                          net_input_dtype=torch.float32 if args.fp32 else torch.bfloat16)
        images, jobs = [], []
        for k in range(args.ny0s):
            data_key, subkey = ops.split(data_key)
            if k < args.start_from:
                continue
            k_img, k_mask = ops.split(subkey)
            test_img = ops.uniform(k_img, (resolution, resolution, nchannels), device=dev)
            mask = ds.gen_mask(k_mask)
            _, test_y0 = ds.unpack(test_img, mask)
            head = os.path.join(args.outdir, f'{args.dataset}-{task}-{args.sde}-{args.nparticles}-{k}')
            np.savez(head + '-true', test_img=test_img.cpu().numpy())
            images.append((head, mask, test_y0, np.zeros((args.nsamples, resolution, resolution, nchannels), np.float32),
                           test_img))
            for i in range(args.nsamples):
                key, subkey = ops.split(key)
                jobs.append((len(images) - 1, i, subkey))
        for g0 in range(0, len(jobs), args.batch):
            group = jobs[g0:g0 + args.batch]                                       # the last group may be smaller
            x0s = sampler(np.stack([j[2] for j in group], 0), [images[j[0]][2] for j in group],
                          [images[j[0]][1] for j in group])
            for b, (m, i, _) in enumerate(group):
                _, mask, test_y0, restored, _ = images[m]
                restored[i] = ds.concat(x0s[b].unsqueeze(0), test_y0, mask)[0].cpu().numpy()
            if not args.quiet:
                print(f'{task} | cSGM x{len(group)} | trajectories: {g0 + len(group)} / {len(jobs)}')
        if args.metrics:
            save_metrics([im[0] + '-csgm' for im in images], [im[4] for im in images], np.stack([im[3] for im in images], 0))
        for head, _, _, restored, _ in images:
            np.save(head + '-csgm', restored)
            out = restored
        return out
    if args.batch > 1 and args.method == 'twisted':
        # The (image, sample) pairs are independent twisted-SMC runs, grouped exactly as the csgm trajectories above
        # (make_image_twisted_batched): two network passes and six launches per step for the group; every run's key
        # follows from its position alone.
        from fbs_amd.twisted import make_image_twisted_batched

        def score(uv, t):                                                            # differentiable: no no_grad here
            if args.fp32:
                return net(uv, t).reshape(uv.shape)
            with torch.autocast('cuda', dtype=torch.bfloat16):
                return net(uv, t).float().reshape(uv.shape)

        tw = make_image_twisted_batched(score, ds, sde, ts, args.nparticles, chunk=args.chunk,
                                        net_input_dtype=torch.float32 if args.fp32 else torch.bfloat16)
        images, jobs = [], []
        for k in range(args.ny0s):
            data_key, subkey = ops.split(data_key)
            if k < args.start_from:
                continue
            k_img, k_mask = ops.split(subkey)
            test_img = ops.uniform(k_img, (resolution, resolution, nchannels), device=dev)
            mask = ds.gen_mask(k_mask)
            _, test_y0 = ds.unpack(test_img, mask)
            head = os.path.join(args.outdir, f'{args.dataset}-{task}-{args.sde}-{args.nparticles}-{k}')
            np.savez(head + '-true', test_img=test_img.cpu().numpy())
            images.append((head, mask, test_y0, np.zeros((args.nsamples, resolution, resolution, nchannels), np.float32),
                           test_img))
            for i in range(args.nsamples):
                key, subkey = ops.split(key)
                jobs.append((len(images) - 1, i, subkey))
        for g0 in range(0, len(jobs), args.batch):
            group = jobs[g0:g0 + args.batch]                                       # the last group may be smaller
            samples = tw.conditional_sampler_batched(np.stack([j[2] for j in group], 0), [images[j[0]][2] for j in group],
                                                     [images[j[0]][1] for j in group], stratified)
            for b, (m, i, _) in enumerate(group):
                images[m][3][i] = samples[b].cpu().numpy()
            if not args.quiet:
                print(f'{task} | twisted x{len(group)} | runs: {g0 + len(group)} / {len(jobs)}')
        if args.metrics:
            save_metrics([im[0] + '-twisted' for im in images], [im[4] for im in images], np.stack([im[3] for im in images], 0))
        for head, _, _, restored, _ in images:
            np.save(head + '-twisted', restored)
            out = restored
        return out
    for k in range(args.ny0s):
        data_key, subkey = ops.split(data_key)
        if k < args.start_from:
            continue
        k_img, k_mask = ops.split(subkey)                                          # dataset.sampler: an image and a mask
        test_img = ops.uniform(k_img, (resolution, resolution, nchannels), device=dev)
        mask = ds.gen_mask(k_mask)
        _, test_y0 = ds.unpack(test_img, mask)
        head = os.path.join(args.outdir, f'{args.dataset}-{task}-{args.sde}-{args.nparticles}-{k}')
        np.savez(head + '-true', test_img=test_img.cpu().numpy())
        restored = np.zeros((args.nsamples, resolution, resolution, nchannels), np.float32)
        to_img = lambda x0: ds.concat(x0.unsqueeze(0), test_y0, mask)[0].cpu().numpy()
        if args.method == 'filter':
            for i in range(args.nsamples):
                key, subkey = ops.split(key)
                x0, _ = gibbs_init(subkey, test_y0, x_shape, ts, sb.fwd_sampler, sde, sb.unpack, nparticles=args.nparticles,
                                   method='filter', marg_y=args.marg, mask_=mask, **cl)
                restored[i] = to_img(x0)
            suffix = f'-filter{"-marg" if args.marg else ""}'
        elif 'gibbs' in args.method:
            key, subkey = ops.split(key)
            x0, us_star = gibbs_init(subkey, test_y0, x_shape, ts, sb.fwd_sampler, sde, sb.unpack,
                                     nparticles=args.nparticles, method=args.init_method, marg_y=args.marg, mask_=mask, **cl)
            bs_star = np.zeros(nsteps + 1, np.int32)
            np.save(head + '-gibbs-init', to_img(x0))
            for i in range(args.nsamples):
                key, subkey = ops.split(key)
                x0, us_star, bs_star, acc = gibbs_kernel(subkey, x0, test_y0, us_star, bs_star, ts, sb.fwd_sampler, sde,
                                                         sb.unpack, args.nparticles, marg_y=args.marg,
                                                         explicit_backward=eb, explicit_final=ef, mask_=mask, **cl)
                restored[i] = to_img(x0)
                if not args.quiet:
                    print(f'{task} | Gibbs | iter: {i}, acc: {float(acc.float().mean()):.3f}')
            suffix = f'-gibbs{"-eb" if eb else ""}{"-ef" if ef else ""}{"-marg" if args.marg else ""}'
        elif args.method == 'twisted':                                               # inpainting_twisted.py:148-191
            from fbs_amd.twisted import make_image_twisted

            def score(uv, t):                                                        # differentiable: no no_grad here
                if args.fp32:
                    return net(uv, t).reshape(uv.shape)
                with torch.autocast('cuda', dtype=torch.bfloat16):
                    return net(uv, t).float().reshape(uv.shape)

            tw = make_image_twisted(score, ds, sde, ts, args.nparticles)
            for i in range(args.nsamples):
                key, subkey = ops.split(key)
                sample = tw.conditional_sampler(subkey, test_y0, stratified, mask_=mask)
                restored[i] = sample.cpu().numpy()
                if not args.quiet:
                    print(f'{task} | twisted | iter: {i}')
            suffix = '-twisted'
        elif args.method == 'csgm':                                                  # inpainting_csgm.py:147-158
            from fbs_amd.csgm import make_image_csgm
            sampler = make_image_csgm(lambda x, t: run(net, x, t), ds, sde, ts)
            for i in range(args.nsamples):
                key, subkey = ops.split(key)
                restored[i] = to_img(sampler(subkey, test_y0, mask))
                if not args.quiet:
                    print(f'{task} | cSGM | iter: {i}')
            suffix = '-csgm'
        elif 'pmcmc' in args.method:
            key, subkey = ops.split(key)
            x0, log_ell, ys = torch.zeros(x_shape, device=dev), 0., sb.fwd_ys_sampler(subkey, test_y0)
            for i in range(args.nsamples):
                key, subkey = ops.split(key)
                x0, log_ell, ys, st = pmcmc_kernel(subkey, x0, log_ell, ys, test_y0, ts, sb.fwd_ys_sampler, sde,
                                                   sb.ref_sampler, sb.transition_sampler, sb.likelihood_logpdf, stratified,
                                                   args.nparticles, delta=delta, mask_=mask)
                restored[i] = to_img(x0)
                if not args.quiet:
                    print(f'{task} | pMCMC {delta} | iter: {i}, acc_prob: {float(st.acceptance_prob):.3f}')
            suffix = f'-pmcmc-{delta}'
        else:
            raise ValueError(f'Unknown method {args.method}')
        if args.metrics:
            save_metrics([head + suffix], [test_img], restored[None])
        np.save(head + suffix, restored)
        out = restored
    return out


if __name__ == '__main__':
    main()
