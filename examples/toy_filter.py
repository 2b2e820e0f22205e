"""Gaussian-process regression with the bootstrap-filter conditional sampler on MI355X.

Counterpart of the reference driver experiments/toy/gp_filter.py (same flags, key schedule and .npz schema:
samples (nsamples, d), gp_mean, gp_cov).  Every sample is one bootstrap_filter run (T = 200 steps); with the
analytic score the whole run is one hipGraph replay (for d > 16: drift on the f32 matrix cores).

--fused draws the samples `--batch` at a time on the device (fbs_amd.samplers.filter_conditional_sampler): the subkeys of
the driver's schedule are derived on the host first, each sample depends on its own subkey only."""
import argparse
import os

import numpy as np
import torch

from _gp_toy import add_common_args, gp_setting
from fbs_amd import ops
from fbs_amd.samplers import bootstrap_filter, filter_conditional_sampler, stratified


def main(argv=None):
    parser = add_common_args(argparse.ArgumentParser())
    parser.add_argument('--fused', action='store_true', help='Batches of samples on the fused engine.')
    parser.add_argument('--batch', type=int, default=64, help='Samples per fused call.')
    parser.add_argument('--diag', action='store_true',
                        help='With --fused: per-step ESS and log-normaliser of every run (saved as ess, lse).')
    args = parser.parse_args(argv)
    if args.diag and not args.fused:
        parser.error('--diag reads the fused engine: it needs --fused')
    dev = torch.device('cuda:0')
    g = gp_setting(args, dev)
    key, br, ts, y0 = g['key'], g['bridge'], g['ts'], g['y0_t']

    def conditional_sampler(key_):                                                  # gp_filter.py:134-142
        key_fwd, key_bwd, key_bf = ops.split(key_, 3)
        vs = torch.flip(br.fwd_ys_sampler(key_fwd, y0), [0])
        return bootstrap_filter(br.transition_sampler, br.likelihood_logpdf, vs, ts, br.ref_sampler, key_bf,
                                args.nparticles, stratified, log=True, return_last=True)[0][0]

    def diag_batch(subkeys_):
        """conditional_sampler for a batch of subkeys on the batched filter handle with diagnostics on (the sampler handle
        keeps none): observation paths and initial particles by the closures, then one fused bootstrap_filter call.
        The initial particles are the closure's ref_sampler's; the fused sampler's own rounds them differently, so about a
        fifth of its samples differ from these in the last bit or two (measured: at most 4.8e-7).
        -> samples (B, d), {"lse", "ess"} (B, T)."""
        k3 = [ops.split(k, 3) for k in subkeys_]                                    # key_fwd, key_bwd, key_bf
        vs = torch.stack([torch.flip(br.fwd_ys_sampler(k[0], y0), [0]) for k in k3], 0)
        u0s = torch.stack([br.ref_sampler(ops.split(k[2], 2)[0], vs[c, 0], args.nparticles) for c, k in enumerate(k3)], 0)
        filt = br.filter_handle(args.nparticles, "bootstrap", "stratified", nchains=len(k3), diagnostics=True)
        uT = filt.run(np.stack([k[2] for k in k3]), vs, u0s)[0].reshape(len(k3), args.nparticles, g['d'])
        dg = filt.diagnostics()
        return uT[:, 0], {n: t.reshape(len(k3), -1) for n, t in dg.items()}

    samples = torch.empty((args.nsamples, g['d']), device=dev)
    diag = {}
    if args.fused and args.diag:
        subkeys = np.empty((args.nsamples, 2), np.uint32)
        for i in range(args.nsamples):                                              # gp_filter.py:145-146, on the host
            key, subkeys[i] = ops.split(key)
        ess, lse = [], []
        for a in range(0, args.nsamples, max(1, args.batch)):
            b = min(a + max(1, args.batch), args.nsamples)
            samples[a:b], dg = diag_batch(subkeys[a:b])
            ess.append(dg["ess"])
            lse.append(dg["lse"])
        diag = dict(ess=torch.cat(ess).cpu().numpy(), lse=torch.cat(lse).cpu().numpy())   # (nsamples, T)
    elif args.fused:
        subkeys = np.empty((args.nsamples, 2), np.uint32)
        for i in range(args.nsamples):                                              # gp_filter.py:145-146, on the host
            key, subkeys[i] = ops.split(key)
        for a in range(0, args.nsamples, max(1, args.batch)):
            b = min(a + max(1, args.batch), args.nsamples)
            samples[a:b] = filter_conditional_sampler(subkeys[a:b], y0, ts, br.fwd_ys_sampler, br.ref_sampler,
                                                      br.transition_sampler, br.likelihood_logpdf, args.nparticles,
                                                      stratified)
    else:
        for i in range(args.nsamples):                                              # gp_filter.py:145-149
            key, subkey = ops.split(key)
            samples[i] = conditional_sampler(subkey)
    samples = samples.cpu().numpy()
    if not args.quiet:
        err = np.abs(samples.mean(axis=0) - g['gp_mean']).max()
        print(f'ID: {args.id} | filter | {args.nsamples} samples | max |mean - gp_mean| = {err:.3f}')
    if args.diag:
        from _gp_toy import print_diag
        print_diag('run', diag['ess'], diag['lse'], args.nparticles)
    os.makedirs(args.outdir, exist_ok=True)
    np.savez(os.path.join(args.outdir, f'filter-{args.sde}-{args.nparticles}-{args.id}'),
             samples=samples, gp_mean=g['gp_mean'], gp_cov=g['gp_cov'], **diag)     # gp_filter.py:152-153
    return samples, g['gp_mean'], g['gp_cov']


if __name__ == '__main__':
    main()
