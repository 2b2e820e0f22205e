"""Gaussian-process regression with the Kalman-filter conditional sampler on the NON-separable Gaussian Schrodinger bridge.

The exact counterpart of toy_sb_filter.py (its setting, flags incl. `--x0 proper|heuristic` and `--batch`, key schedule and
.npz schema -- samples (nsamples, d), gp_mean, gp_cov -- that tabulate_toy.py reads): every sample's observation path is
the one toy_sb_filter.py --fused --batch draws from the same subkey (the y half of an Euler-Maruyama path of the bridge's
drift from (x0, y0)), and the sample is a draw from the exact filtering law of the discretised reverse model instead of a
bootstrap filter's particle (fbs_amd.samplers.sb_kalman_conditional_sampler).  What is left in its
error statistics is the discretisation bias and the Monte-Carlo error of `nsamples` draws.  The file is
kf-<x0>-<id>.npz; --nparticles is accepted and unused.

``--smoother`` draws whole trajectories u_0..u_T from the exact smoothing law instead
(fbs_amd.samplers.sb_kalman_path_sampler).  Its file, kfs-<x0>-<id>.npz, holds the default schema with samples =
paths[:, T] -- the same draws as the default run -- plus path_mean and path_var (T+1, d)."""
import argparse
import os

import numpy as np
import torch

from toy_sb_gibbs import common_args, sb_setting
from fbs_amd import ops
from fbs_amd.samplers import sb_kalman_conditional_sampler, sb_kalman_path_sampler


def main(argv=None):
    parser = common_args(argparse.ArgumentParser())
    parser.add_argument('--x0', type=str, default='heuristic', help="How the forward path's x0 is drawn: 'proper' or 'heuristic'.")
    parser.add_argument('--batch', type=int, default=1024, help='Samples per fused call.')
    parser.add_argument('--smoother', action='store_true',
                        help='Draw whole paths from the exact smoothing law (sb_kalman_path_sampler) and save their moments.')
    args = parser.parse_args(argv)
    if args.x0 not in ('proper', 'heuristic'):
        raise ValueError(f'Invalid "{args.x0}" method')
    args.fused = True                                                                # the sampler has the fused engine only
    dev = torch.device('cuda:0')
    g = sb_setting(args, dev)
    key, d, br = g.key, g.d, g.bridge
    prior = (g.gp_mean, np.linalg.cholesky(g.gp_cov)) if args.x0 == 'proper' else None

    subkeys = np.empty((args.nsamples, 2), np.uint32)
    for i in range(args.nsamples):                                                   # sb/filter.py:167-168, on the host
        key, subkeys[i] = ops.split(key)
    step = max(1, args.batch)
    os.makedirs(args.outdir, exist_ok=True)
    if args.smoother:
        paths = torch.empty((args.nsamples, br.T + 1, d), device=dev)
        for a in range(0, args.nsamples, step):
            b = min(a + step, args.nsamples)
            paths[a:b] = sb_kalman_path_sampler(subkeys[a:b], g.y0, br, x0_prior=prior)
        paths = paths.cpu().numpy()
        samples = np.ascontiguousarray(paths[:, br.T])
        path_mean, path_var = paths.mean(axis=0), paths.var(axis=0, ddof=1)
        if not args.quiet:
            err = np.abs(samples.mean(axis=0) - g.gp_mean).max()
            print(f'ID: {args.id} | SB kf smoother ({args.x0}) | {args.nsamples} paths | max |mean - gp_mean| = {err:.3f} | '
                  f'mean path variance at k = 0: {float(path_var[0].mean()):.3f}, at k = T: {float(path_var[-1].mean()):.3f}')
        np.savez(os.path.join(args.outdir, f'kfs-{args.x0}-{args.id}'),
                 samples=samples, gp_mean=g.gp_mean, gp_cov=g.gp_cov, path_mean=path_mean, path_var=path_var)
        return samples, g.gp_mean, g.gp_cov
    samples = torch.empty((args.nsamples, d), device=dev)
    logliks = torch.empty(args.nsamples, device=dev)
    for a in range(0, args.nsamples, step):
        b = min(a + step, args.nsamples)
        samples[a:b], _, logliks[a:b] = sb_kalman_conditional_sampler(subkeys[a:b], g.y0, br, x0_prior=prior,
                                                                      return_moments=True)
    samples = samples.cpu().numpy()
    if not args.quiet:
        err = np.abs(samples.mean(axis=0) - g.gp_mean).max()
        print(f'ID: {args.id} | SB kf ({args.x0}) | {args.nsamples} samples | max |mean - gp_mean| = {err:.3f} | '
              f'mean log-likelihood {float(logliks.mean()):.3f}')
    np.savez(os.path.join(args.outdir, f'kf-{args.x0}-{args.id}'), samples=samples, gp_mean=g.gp_mean, gp_cov=g.gp_cov)
    return samples, g.gp_mean, g.gp_cov


if __name__ == '__main__':
    main()
