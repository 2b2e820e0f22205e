"""Train the score network of the image experiments on MI355X: the counterpart of experiments/imgs/train.py.

Same flags, same key schedule (PRNGKey(666); the data, network and epoch keys split off in the reference's order), the same
loss (fbs_amd.sdes.make_linear_sde_law_loss), optimiser (optax.adam behind an optional clip_by_global_norm(1.), the
reference's three schedules) and EMA regime (ema_kernel(j, 300, 2, 0.99)); the checkpoint is the reference's
`./checkpoints/<dataset>_<sde>_<epoch>.npz` with `param` / `ema_param` in ravel_pytree order, which
examples/imgs_restore.py loads unchanged.  Per step the host splits keys and sorts a few random times; the noising, the loss
and its derivative, the clip norm and the update are HIP kernels, the network's forward and backward PyTorch autograd, and
nothing is read back except the loss every --log_every steps.

Differences from the reference, all forced by what a machine without its data sets and without jax has:
  * the data: `--data FILE` (.npy, or .npz with an array `X` or its first array, (N, H, W, C) in [0, 1], kept on the
    device), or `--synthetic N` (N seeded images of smooth random blobs).  The reference's MNIST / CelebA-HQ loaders are not
    reproduced.
  * the epoch permutation is the argsort of uniform(key, (N,)) on the host, NOT jax.random.choice's permutation: the same
    key gives a different order than the reference (and the reference's enumerate_subset flips, which its training data
    sets do not use, are absent).
  * the final check saves its seven images -- the test sample, its noised terminal value, five reverse_simulator draws from
    the EMA weights -- as `<outdir>/<dataset>_<sde>_backward_test.npy` instead of drawing a figure.
  * the network is initialised by PyTorch's initialisers from a seed derived from the network key, not by flax's.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbs_amd import ops  # noqa: E402
from fbs_amd.sdes import (StationaryConstLinearSDE, StationaryExpLinearSDE, StationaryLinLinearSDE, make_linear_sde,  # noqa: E402
                          make_linear_sde_law_loss, reverse_simulator)
from fbs_amd.sdes.losses import uniform_host  # noqa: E402
from fbs_amd.train import (constant_schedule, cosine_decay_schedule, exponential_decay, make_adam_kernel,  # noqa: E402
                           save_checkpoint)
from fbs_amd.unet import UNet  # noqa: E402


def synthetic_blobs(n: int, shape, seed: int = 0) -> np.ndarray:
    """n images (H, W, C) in [0, 1]: a few Gaussian bumps of random place, width and colour each."""
    H, W, C = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing='ij')
    out = np.zeros((n, H, W, C), np.float64)
    for i in range(n):
        for _ in range(int(rng.integers(2, 5))):
            cy, cx, s = rng.uniform(0.15, 0.85), rng.uniform(0.15, 0.85), rng.uniform(0.08, 0.25)
            bump = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            out[i] += bump[:, :, None] * rng.uniform(0.3, 1.0, C)[None, None, :]
    return np.clip(out, 0.0, 1.0).astype(np.float32)


def load_data(path: str) -> np.ndarray:
    z = np.load(path)
    if isinstance(z, np.lib.npyio.NpzFile):
        z = z['X'] if 'X' in z.files else z[z.files[0]]
    z = np.asarray(z, np.float32)
    if z.ndim == 3:
        z = z[..., None]
    if z.ndim != 4:
        raise ValueError(f'{path}: expected (N, H, W, C) images, got shape {z.shape}')
    return z


def main(argv=None):
    p = argparse.ArgumentParser(description='Training forward noising model.')
    p.add_argument('--dataset', type=str, default='mnist', help='mnist, celeba-64 or celeba-128: names the checkpoint and sets the default shape.')
    p.add_argument('--sde', type=str, default='lin')
    p.add_argument('--upsampling', type=str, default='pixel_shuffle')
    p.add_argument('--loss_type', type=str, default='score')
    p.add_argument('--lr', type=float, default=2e-4)
    p.add_argument('--batch_size', type=int, default=2)
    p.add_argument('--nsteps', type=int, default=2)
    p.add_argument('--schedule', type=str, default='cos')
    p.add_argument('--nepochs', type=int, default=40)
    p.add_argument('--save_mem', action='store_true', default=False, help='Save memory by sharing the batch of x and t')
    p.add_argument('--grad_clip', action='store_true', default=False)
    p.add_argument('--data', type=str, default=None, help='.npy / .npz of (N, H, W, C) images in [0, 1]; kept on the device.')
    p.add_argument('--synthetic', type=int, default=0, help='Train on this many seeded images of smooth random blobs.')
    p.add_argument('--resolution', type=int, default=None, help='With --synthetic: image size (default: the data set\'s).')
    p.add_argument('--dim', type=int, default=64, help='UNet width (64 in the reference).')
    p.add_argument('--dim_mults', type=str, default='1,2,4', help='UNet stage multipliers (1,2,4 in the reference).')
    p.add_argument('--bf16', action='store_true', help='bfloat16 autocast for the network only (default float32, the reference\'s precision).')
    p.add_argument('--save_every', type=int, default=100, help='Epochs between checkpoints (the last epoch is always saved).')
    p.add_argument('--log_every', type=int, default=50, help='Steps between loss prints (a print reads the loss back).')
    p.add_argument('--check_nsteps', type=int, default=500, help='Steps of the final reverse-SDE check (0: skip it).')
    p.add_argument('--ckpt_dir', type=str, default='./checkpoints')
    p.add_argument('--outdir', type=str, default='./tmp_figs')
    p.add_argument('--quiet', action='store_true')
    args = p.parse_args(argv)

    dev = torch.device('cuda:0')
    say = (lambda *a: None) if args.quiet else print
    resolution = 28 if args.dataset == 'mnist' else int(args.dataset.split('-')[-1])
    nchannels = 1 if args.dataset == 'mnist' else 3
    key = ops.PRNGKey(666)                                                         # train.py:44-45
    key, data_key = ops.split(key)
    T = 2
    key, subkey = ops.split(key)                                                   # the data set's key (train.py:53)
    if args.data is not None:
        images = load_data(args.data)
    elif args.synthetic > 0:
        r = resolution if args.resolution is None else args.resolution
        images = synthetic_blobs(args.synthetic, (r, r, nchannels), seed=int(subkey[1]))
    else:
        raise SystemExit('imgs_train.py: give --data FILE or --synthetic N (the reference data sets are not shipped)')
    data = torch.from_numpy(np.ascontiguousarray(images)).to(dev)
    data_size, d = int(data.shape[0]), tuple(data.shape[1:])
    say(f'Train on {args.dataset}: {data_size} images of shape {d}')

    if args.sde == 'const':                                                        # train.py:64-72
        sde = StationaryConstLinearSDE(a=-0.5, b=1.)
    elif args.sde == 'lin':
        sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5., t0=0., T=T)
    elif args.sde == 'exp':
        sde = StationaryExpLinearSDE(a=-0.5, b=1., c=1., z=1.)
    else:
        raise NotImplementedError('...')

    train_nsamples, nepochs = args.batch_size, args.nepochs
    if train_nsamples > data_size:
        raise SystemExit(f'imgs_train.py: batch size {train_nsamples} exceeds the {data_size} images')
    key, subkey = ops.split(key)                                                   # the network's key (train.py:82)
    torch.manual_seed(int(subkey[0]) ^ int(subkey[1]))
    module = UNet(dt=T / 200, dim=args.dim, in_channels=d[-1], upsampling=args.upsampling,
                  dim_mults=tuple(int(s) for s in args.dim_mults.split(','))).to(dev)

    def nn_score(x, t, param=None):
        if args.bf16:
            with torch.autocast('cuda', dtype=torch.bfloat16):
                return module(x, t)
        return module(x, t)

    loss_fn = make_linear_sde_law_loss(sde, nn_score, t0=0., T=T, nsteps=args.nsteps, random_times=True,
                                       loss_type=args.loss_type, save_mem=args.save_mem)
    nsteps_per_epoch = data_size // train_nsamples
    if args.schedule == 'cos':                                                     # train.py:92-98
        until_steps = max(int(0.95 * nepochs) * nsteps_per_epoch, 1)
        schedule = cosine_decay_schedule(init_value=args.lr, decay_steps=until_steps, alpha=1e-2)
    elif args.schedule == 'exp':
        schedule = exponential_decay(args.lr, data_size // train_nsamples, .96)
    else:
        schedule = constant_schedule(args.lr)
    step, ema_kernel = make_adam_kernel(module, loss_fn, schedule, grad_clip=1. if args.grad_clip else None)
    fp, state = step.params, step.state

    ckpt = None
    for i in range(nepochs):
        data_key, subkey = ops.split(data_key)
        perm = torch.from_numpy(np.argsort(uniform_host(subkey, data_size), kind='stable').astype(np.int32)).to(dev)
        for j in range(nsteps_per_epoch):
            subkey, subkey2 = ops.split(subkey)
            ema_kernel(j, 300, 2, 0.99)                                            # what this step does with the EMA
            loss = step(subkey2, data, perm[j * train_nsamples:(j + 1) * train_nsamples])
            if not args.quiet and (j % args.log_every == 0 or j == nsteps_per_epoch - 1):
                print(f'{args.dataset} | {args.upsampling} | {args.sde} | {args.loss_type} | {args.schedule} | '
                      f'Epoch: {i} / {nepochs}, iter: {j} / {nsteps_per_epoch}, loss: {float(loss):.4f}')
        if (i + 1) % args.save_every == 0 or i == nepochs - 1:
            ckpt = os.path.join(args.ckpt_dir, f'{args.dataset}_{args.sde}_{i}.npz')
            save_checkpoint(ckpt, fp, state['ema'])
            say(f'checkpoint: {ckpt}')
    say('Training done.')

    if args.check_nsteps > 0:                                                      # train.py:129-153
        ts = np.linspace(0, T, args.check_nsteps + 1)
        fp.load_vector(state['ema'])                                               # the EMA weights, visible to the caches
        module.eval()

        def learnt_score(x, t):
            with torch.no_grad():
                return nn_score(x, t).float().reshape(x.shape)

        _, _, simulate_cond_forward = make_linear_sde(sde)
        key = ops.PRNGKey(666)
        key, subkey = ops.split(key)
        test_sample0 = data[int(uniform_host(subkey, 1)[0] * data_size) % data_size]
        key, subkey = ops.split(key)
        terminal_val = simulate_cond_forward(subkey, test_sample0, ts)[-1]
        key, subkey = ops.split(key)
        draws = [reverse_simulator(k, terminal_val, ts, learnt_score, sde.drift, sde.dispersion,
                                   integrator='euler-maruyama') for k in ops.split(subkey, 5)]
        out = torch.stack([test_sample0, terminal_val] + draws).cpu().numpy()
        say(float(out[2:].min()), float(out[2:].max()))
        os.makedirs(args.outdir, exist_ok=True)
        path = os.path.join(args.outdir, f'{args.dataset}_{args.sde}_backward_test.npy')
        np.save(path, out)
        say(f'reverse-SDE check: {path}')
    return ckpt


if __name__ == '__main__':
    main()
