"""Gibbs sweeps of B independent ensembles in lockstep: the test images of one run, or several chains of one image.

The ensembles share the time grid, the SDE and the network, so every SMC step of all of them is one network call on
B * rows rows between single launches of the batched sampler kernels (fbs_amd/csrc/fbsmi_batch.hip), instead of B calls
on `rows` rows each among a dozen launches per ensemble.  ``gibbs_kernel_batched`` is the loop of ``gibbs_kernel`` over
the ensembles, with the same keys, run that way.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import ops
from ..score import bridge_of, is_own_method
from .gibbs import bridge_sampler, force_move, gibbs_kernel

MAX_LOCKSTEP_ROWS = 1024                                   # rows of one ensemble in the batched kernels


def sweep_key_schedule(keys, nsteps: int) -> dict:
    """Every key a sweep of ``gibbs_kernel`` (explicit_backward) derives from its own, for B sweeps, on the host:
    gibbs.py:126 (fwd, csmc, bridge), :147 (k_fwd, x0, us, bs), csmc.py:150 (init, scan), :157 (one per step) and :136
    (resampling, transition).  -> (B, 2) arrays 'fwd', 'bridge', 'x0', 'us', 'bs', 'init' and (nsteps, B, 2) arrays
    'resampling', 'transition', all uint32."""
    keys = np.asarray(keys, np.uint32).reshape(-1, 2)
    B, T = keys.shape[0], int(nsteps)
    out = {name: np.zeros((B, 2), np.uint32) for name in ("fwd", "bridge", "x0", "us", "bs", "init")}
    out["resampling"] = np.zeros((T, B, 2), np.uint32)
    out["transition"] = np.zeros((T, B, 2), np.uint32)
    for b in range(B):
        out["fwd"][b], key_csmc, out["bridge"][b] = ops.split(keys[b], 3)
        k_fwd, out["x0"][b], out["us"][b], out["bs"][b] = ops.split(key_csmc, 4)
        out["init"][b], key_scan = ops.split(k_fwd, 2)
        step_keys = ops.split(key_scan, T)
        for k in range(T):
            out["resampling"][k, b], out["transition"][k, b] = ops.split(step_keys[k], 2)
    return out


def _is_mask(m) -> bool:
    return hasattr(m, "unobs_inds_ravelled")


def _host_int(x) -> np.ndarray:
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)


def gibbs_kernel_batched(keys, x0s, y0s, us_stars, bs_stars, ts, fwd_sampler, sde, unpack, nparticles, transition_sampler,
                         transition_logpdf, likelihood_logpdf, marg_y: bool = False, explicit_backward: bool = True,
                         explicit_final: bool = False, **kwargs):
    """``gibbs_kernel`` for B ensembles: keys (B, 2), x0s (B, p, c), y0s one observation (q, c) or B of them, us_stars and
    bs_stars with a leading axis B, ``mask_`` one mask or a list of B masks.  Returns the four results of
    ``gibbs_kernel``, each with a leading axis B, equal to the stacked results of

        [gibbs_kernel(keys[b], x0s[b], y0s[b], us_stars[b], bs_stars[b], ..., mask_=masks[b]) for b in range(B)]

    bit for bit whenever the score function's output row does not depend on which other rows share its call.  That is
    not promised for a real UNet: library convolution and matrix kernels may be chosen by batch size and differ in the
    last bits, after which a resampling decision can flip and the two runs part ways as two valid draws.

    The ensembles advance in lockstep -- one network call per step, one launch per sampler operation, no host
    synchronisation inside the time loop -- when the closures are one ScoreBridge's own, ``mask_`` is the only keyword,
    explicit_backward is set, the masks have one shape and an ensemble has at most 1024 rows.  Anything else runs the loop
    above: the same result without the speed-up.  The forward paths before and after the loop are drawn for all ensembles
    at once (``ScoreBridge.fwd_sampler_batched``) when ``fwd_sampler`` and ``unpack`` are that bridge's own methods too,
    and by a call per ensemble for any other closure."""
    keys = np.asarray(keys.detach().cpu() if isinstance(keys, torch.Tensor) else keys, np.uint32).reshape(-1, 2)
    B = keys.shape[0]
    masks = kwargs.get("mask_")
    per_mask = masks is not None and not _is_mask(masks)
    if per_mask and len(masks) != B:
        raise ValueError(f"{len(masks)} masks for {B} ensembles")
    y_batched = isinstance(y0s, (list, tuple)) or (isinstance(y0s, torch.Tensor) and y0s.dim() == x0s[0].dim() + 1)
    kw = lambda b: {**kwargs, "mask_": masks[b]} if per_mask else kwargs
    y0 = lambda b: y0s[b] if y_batched else y0s
    rows = int(nparticles) + (1 if explicit_final else 0)

    sb = bridge_of(transition_sampler, likelihood_logpdf) if set(kwargs) == {"mask_"} else None
    lockstep = sb is not None and explicit_backward and rows <= MAX_LOCKSTEP_ROWS
    if lockstep:
        ems = [sb._em_mask(kw(b)["mask_"]) for b in range(B)]
        lockstep = all((e.du, e.dv) == (ems[0].du, ems[0].dv) for e in ems)
    if not lockstep:
        outs = [gibbs_kernel(keys[b], x0s[b], y0(b), None if us_stars is None else us_stars[b], bs_stars[b], ts,
                             fwd_sampler, sde, unpack, nparticles, transition_sampler, transition_logpdf,
                             likelihood_logpdf, marg_y=marg_y, explicit_backward=explicit_backward,
                             explicit_final=explicit_final, **kw(b)) for b in range(B)]
        return tuple(torch.stack([o[i] for o in outs], 0) for i in range(4))

    T = len(ts) - 1
    sk = sweep_key_schedule(keys, T)
    mb = sb.em_mask_batch(masks if per_mask else [masks], B)
    # the bridge's own forward sampler draws the paths of all ensembles at once (ScoreBridge.fwd_sampler_batched)
    own_fwd = is_own_method(sb, fwd_sampler, "fwd_sampler") and is_own_method(sb, unpack, "unpack")
    if own_fwd:                                                                     # preamble (gibbs.py:127-130)
        us_star, vs = sb.fwd_sampler_batched(sk["fwd"], x0s, y0s, mb)               # (T + 1, B, p, c), (T + 1, B, q, c)
        if marg_y:
            vs = torch.stack([torch.flip(bridge_sampler(sk["bridge"][b], vs[T, b], vs[0, b], ts, sde), [0])
                              for b in range(B)], 1).contiguous()
    else:                                                                           # the same, per ensemble
        uss, vss = [], []
        for b in range(B):
            path_x, path_y = unpack(fwd_sampler(sk["fwd"][b], x0s[b], y0(b), **kw(b)), **kw(b))
            uss.append(torch.flip(path_x, [0]))
            vss.append(torch.flip(bridge_sampler(sk["bridge"][b], path_y[0], path_y[-1], ts, sde), [0]) if marg_y
                       else torch.flip(path_y, [0]))
        us_star = torch.stack(uss, 1).contiguous()                                  # (T + 1, B, p, c)
        vs = torch.stack(vss, 1).contiguous()                                       # (T + 1, B, q, c)
    dev = us_star.device
    bs_np = np.stack([_host_int(bs_stars[b]).reshape(-1) for b in range(B)], 0).astype(np.int32)   # (B, T + 1)
    bs_dev = torch.from_numpy(np.ascontiguousarray(bs_np.T)).to(dev)                # (T + 1, B)
    k_res = ops.keys_to_device(sk["resampling"], dev)                               # the whole sweep's keys, uploaded once
    k_tr = ops.keys_to_device(sk["transition"], dev)
    unobs = tuple(us_star.shape[2:])

    # initial particles and weights (gibbs.py:132-144, csmc.py:151-155)
    if explicit_final:
        us = torch.stack([ops.normal(sk["init"][b], (rows,) + unobs, device=dev) for b in range(B)], 0)
    else:
        us = us_star[0].unsqueeze(1).expand((B, rows) + unobs).clone()
    us[torch.arange(B, device=dev), bs_dev[0].long()] = us_star[0]
    if explicit_final:
        _, lw = sb.fused_step_batched(us, None, vs[0], vs[1], ts[0], None, mb, want_us=False)
    else:
        lw = torch.full((B, rows), -math.log(nparticles), dtype=torch.float32, device=dev)
    w = ops.normalise_batched(lw)                                                   # exp(normalise(., log_space=True))

    for k in range(T):                                                              # csmc.py:132-148 for all ensembles
        A = ops.cond_killing_batched(k_res[k], w, bs_dev[k], bs_dev[k + 1])
        us, lw = sb.fused_step_batched(us, A, vs[k + 1], vs[k], ts[k], k_tr[k], mb, pins=(bs_dev[k + 1], us_star[k + 1]))
        w = ops.normalise_batched(lw)

    # postamble: forced move per ensemble, fresh reference paths and indices (gibbs.py:152-156, 167-168)
    x0n, usn, bsn, acc = [], [], [], []
    for b in range(B):
        idx, _ = force_move(sk["x0"][b], w[b], int(bs_np[b, -1]))
        x0 = us[b][idx.long()]
        if own_fwd:
            x0n.append(x0)                                                          # the paths follow, all at once
        else:
            us_next = torch.flip(unpack(fwd_sampler(sk["us"][b], x0, y0(b), **kw(b)), **kw(b))[0], [0])
            x0n.append(us_next[-1])
            usn.append(us_next)
        bs_next = ops.randint(sk["bs"][b], (T + 1,), 0, nparticles, device=dev)
        bsn.append(bs_next)
        acc.append(bs_next != bs_dev[:, b])
    if own_fwd:
        us_next = sb.fwd_sampler_batched(sk["us"], torch.stack(x0n, 0), y0s, mb, want_vs=False, batch_major=True)[0]
        return us_next[:, -1].contiguous(), us_next, torch.stack(bsn, 0), torch.stack(acc, 0)
    return torch.stack(x0n, 0), torch.stack(usn, 0), torch.stack(bsn, 0), torch.stack(acc, 0)
