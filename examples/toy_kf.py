"""Gaussian-process regression with the Kalman-filter conditional sampler on MI355X.

Counterpart of the reference driver experiments/toy/gp_kf.py (its flags and key schedule; the reference only plots, the
result here is a .npz in toy_filter.py's schema -- samples (nsamples, d), gp_mean, gp_cov -- that tabulate_toy.py reads).
The sampler is the EXACT filter of the discretised model the other toy drivers run (T = 200 steps, not gp_kf.py's ad hoc
recursion: DESIGN.md section 4.6), so what is left in its error statistics is the discretisation bias and the Monte-Carlo
error of `nsamples` draws.

The samples are drawn `--batch` at a time on the device (fbs_amd.samplers.kalman_conditional_sampler): the subkeys of the
driver's schedule are derived on the host first, each sample depends on its own subkey only.

``--smoother`` draws whole trajectories u_0..u_T from the exact smoothing law instead (the forward filter, then the
backward sampler: fbs_amd.samplers.kalman_path_sampler).  Its file, kfs-<sde>-<id>.npz, holds the
default schema with samples = paths[:, T] -- the same draws as the default run -- plus path_mean and path_var (T+1, d)."""
import argparse
import os

import numpy as np
import torch

from _gp_toy import add_common_args, gp_setting
from fbs_amd import ops
from fbs_amd.samplers import kalman_conditional_sampler, kalman_path_sampler


def smoother_main(args, g, subkeys, dev):
    """--smoother: whole paths from p(u_0..u_T | v_0..v_T), `--batch` at a time; the default schema with
    samples = paths[:, T] (the default run's draws on the same schedule) plus the pathwise mean and variance over the
    draws, (T+1, d) each, in kfs-<sde>-<id>.npz."""
    br, y0 = g['bridge'], g['y0_t']
    paths = torch.empty((args.nsamples, br.T + 1, g['d']), device=dev)
    step = max(1, args.batch)
    for a in range(0, args.nsamples, step):
        b = min(a + step, args.nsamples)
        paths[a:b] = kalman_path_sampler(subkeys[a:b], y0, br)
    paths = paths.cpu().numpy()
    samples = np.ascontiguousarray(paths[:, br.T])
    path_mean, path_var = paths.mean(axis=0), paths.var(axis=0, ddof=1)
    if not args.quiet:
        err = np.abs(samples.mean(axis=0) - g['gp_mean']).max()
        print(f'ID: {args.id} | kf smoother | {args.nsamples} paths | max |mean - gp_mean| = {err:.3f} | '
              f'mean path variance at k = 0: {float(path_var[0].mean()):.3f}, at k = T: {float(path_var[-1].mean()):.3f}')
    os.makedirs(args.outdir, exist_ok=True)
    np.savez(os.path.join(args.outdir, f'kfs-{args.sde}-{args.id}'),
             samples=samples, gp_mean=g['gp_mean'], gp_cov=g['gp_cov'], path_mean=path_mean, path_var=path_var)
    return samples, g['gp_mean'], g['gp_cov']


def main(argv=None):
    parser = add_common_args(argparse.ArgumentParser())
    parser.add_argument('--batch', type=int, default=1024, help='Samples per fused call.')
    parser.add_argument('--smoother', action='store_true',
                        help='Draw whole paths from the exact smoothing law (kalman_path_sampler) and save their moments.')
    args = parser.parse_args(argv)
    dev = torch.device('cuda:0')
    g = gp_setting(args, dev)
    key, br, y0 = g['key'], g['bridge'], g['y0_t']

    subkeys = np.empty((args.nsamples, 2), np.uint32)
    for i in range(args.nsamples):                                                  # gp_kf.py:160-161, on the host
        key, subkeys[i] = ops.split(key)
    if args.smoother:
        return smoother_main(args, g, subkeys, dev)
    samples = torch.empty((args.nsamples, g['d']), device=dev)
    logliks = torch.empty(args.nsamples, device=dev)
    step = max(1, args.batch)
    for a in range(0, args.nsamples, step):
        b = min(a + step, args.nsamples)
        samples[a:b], _, logliks[a:b] = kalman_conditional_sampler(subkeys[a:b], y0, br, return_moments=True)
    samples = samples.cpu().numpy()
    if not args.quiet:
        err = np.abs(samples.mean(axis=0) - g['gp_mean']).max()
        print(f'ID: {args.id} | kf | {args.nsamples} samples | max |mean - gp_mean| = {err:.3f} | '
              f'mean log-likelihood {float(logliks.mean()):.3f}')
    os.makedirs(args.outdir, exist_ok=True)
    np.savez(os.path.join(args.outdir, f'kf-{args.sde}-{args.id}'),
             samples=samples, gp_mean=g['gp_mean'], gp_cov=g['gp_cov'])
    return samples, g['gp_mean'], g['gp_cov']


if __name__ == '__main__':
    main()
