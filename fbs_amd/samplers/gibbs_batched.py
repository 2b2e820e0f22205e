"""Gibbs sweeps of B independent ensembles in lockstep: the test images of one run, or several chains of one image.

The ensembles share the time grid, the SDE and the network, so every SMC step of all of them is one network call on
B * rows rows between single launches of the batched sampler kernels (fbs_amd/csrc/fbsmi_batch.hip), instead of B calls
on `rows` rows each among a dozen launches per ensemble.  ``gibbs_kernel_batched`` is the loop of ``gibbs_kernel`` over
the ensembles, with the same keys, run that way, under every flag: with ``explicit_backward`` the forced move, the row
pick and the fresh reference indices of all ensembles are one launch each, without it the ancestors and particles of
every step go straight into one stored array and one launch scans all ensembles backwards, and with ``marg_y`` the Doob
bridges of all observation paths are one launch.  Nothing in the lockstep path runs once per ensemble except a forward
sampler that is not the bridge's own.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib, ops
from ..score import bridge_of, is_own_method
from ..sdes.simulators import doob_bridge_simulator_batched
from .gibbs import gibbs_kernel

MAX_LOCKSTEP_ROWS = 1024                                   # rows of one ensemble in the batched kernels
# explicit_backward=False keeps the particles of every step of every ensemble, (T + 1) * B * rows * du floats, until the
# backward scan.  This bounds that array: a batch above it advances in consecutive groups of the largest size that fits,
# one ensemble alone above it runs the loop.  It is a cap on memory, not a tuned number.
LOCKSTEP_STORE_BYTES = 1 << 31


def sweep_key_schedule(keys, nsteps: int, explicit_backward: bool = True) -> dict:
    """Every key a sweep of ``gibbs_kernel`` derives from its own, for B sweeps, on the host.  With explicit_backward:
    gibbs.py:126 (fwd, csmc, bridge), :147 (k_fwd, x0, us, bs), csmc.py:150 (init, scan), :157 (one per step) and :136
    (resampling, transition).  -> (B, 2) arrays 'fwd', 'bridge', 'x0', 'us', 'bs', 'init' and (nsteps, B, 2) arrays
    'resampling', 'transition', all uint32.  Without it the schedule is ``csmc_kernel``'s: csmc.py:29 (key_fwd, bwd)
    instead of gibbs.py:147, then ``_forward``'s as above.  -> 'fwd', 'bridge', 'bwd', 'init', 'resampling', 'transition'."""
    keys = np.asarray(keys, np.uint32).reshape(-1, 2)
    B, T = keys.shape[0], int(nsteps)
    names = ("fwd", "bridge", "x0", "us", "bs", "init") if explicit_backward else ("fwd", "bridge", "bwd", "init")
    out = {name: np.zeros((B, 2), np.uint32) for name in names}
    out["resampling"] = np.zeros((T, B, 2), np.uint32)
    out["transition"] = np.zeros((T, B, 2), np.uint32)
    for b in range(B):
        out["fwd"][b], key_csmc, out["bridge"][b] = ops.split(keys[b], 3)
        if explicit_backward:
            k_fwd, out["x0"][b], out["us"][b], out["bs"][b] = ops.split(key_csmc, 4)
        else:
            k_fwd, out["bwd"][b] = ops.split(key_csmc, 2)
        out["init"][b], key_scan = ops.split(k_fwd, 2)
        step_keys = ops.split(key_scan, T)
        for k in range(T):
            out["resampling"][k, b], out["transition"][k, b] = ops.split(step_keys[k], 2)
    return out


def lockstep_groups(B: int, bytes_per_ensemble: int, cap: int):
    """How B ensembles that each store `bytes_per_ensemble` advance under the cap: "loop" when one ensemble alone exceeds
    it, else the consecutive (start, stop) groups of the largest size that fits, covering range(B) in order (one group
    when the whole batch fits)."""
    B, per, cap = int(B), int(bytes_per_ensemble), int(cap)
    if per > cap:
        return "loop"
    g = B if per <= 0 else max(1, min(B, cap // per))
    return [(s, min(s + g, B)) for s in range(0, B, g)]


def _is_mask(m) -> bool:
    return hasattr(m, "unobs_inds_ravelled")


def _host_int(x) -> np.ndarray:
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)


def _take(us, inds):
    """us[b][inds[b]] for every ensemble."""
    return us[torch.arange(us.shape[0], device=us.device)[:, None], inds.long()]


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
    the masks have one shape and an ensemble has at most 1024 rows, whatever marg_y, explicit_backward and
    explicit_final are.  Anything else runs the loop above: the same result without the speed-up.  After the time loop
    the forced move, the row pick, the fresh indices and their comparison are four launches for all ensembles
    (explicit_backward), or one launch scans all ensembles backwards through the stored ancestors and particles
    (otherwise); with marg_y the Doob bridges of all ensembles are one launch.  The forward paths before and after the
    loop are drawn for all ensembles at once (``ScoreBridge.fwd_sampler_batched``) when ``fwd_sampler`` and ``unpack`` are
    that bridge's own methods too, and by a call per ensemble for any other closure.

    Without explicit_backward the particles of every step are kept until the backward scan, (T + 1) * B * rows * du
    floats.  ``LOCKSTEP_STORE_BYTES`` (2 GiB) caps that array: a larger batch advances in consecutive groups of the
    largest size that fits, each in lockstep, and one ensemble alone above the cap runs the loop.  The constant is a
    cap on memory, not a tuned number."""
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
    T = len(ts) - 1

    sb = bridge_of(transition_sampler, likelihood_logpdf) if set(kwargs) == {"mask_"} else None
    lockstep = sb is not None and rows <= MAX_LOCKSTEP_ROWS
    if lockstep:
        ems = [sb._em_mask(kw(b)["mask_"]) for b in range(B)]
        lockstep = all((e.du, e.dv) == (ems[0].du, ems[0].dv) for e in ems)
    groups = None
    if lockstep and not explicit_backward:
        groups = lockstep_groups(B, 4 * (T + 1) * rows * ems[0].du, LOCKSTEP_STORE_BYTES)
        lockstep = groups != "loop"
    if not lockstep:
        outs = [gibbs_kernel(keys[b], x0s[b], y0(b), None if us_stars is None else us_stars[b], bs_stars[b], ts,
                             fwd_sampler, sde, unpack, nparticles, transition_sampler, transition_logpdf,
                             likelihood_logpdf, marg_y=marg_y, explicit_backward=explicit_backward,
                             explicit_final=explicit_final, **kw(b)) for b in range(B)]
        return tuple(torch.stack([o[i] for o in outs], 0) for i in range(4))
    if groups is not None and len(groups) > 1:                                      # each group in lockstep, in order
        outs = [gibbs_kernel_batched(keys[s:e], x0s[s:e], y0s[s:e] if y_batched else y0s,
                                     None if us_stars is None else us_stars[s:e], bs_stars[s:e], ts, fwd_sampler, sde,
                                     unpack, nparticles, transition_sampler, transition_logpdf, likelihood_logpdf,
                                     marg_y=marg_y, explicit_backward=False, explicit_final=explicit_final,
                                     **({**kwargs, "mask_": list(masks[s:e])} if per_mask else kwargs))
                for s, e in groups]
        return tuple(torch.cat([o[i] for o in outs], 0) for i in range(4))

    sk = sweep_key_schedule(keys, T, explicit_backward=explicit_backward)
    mb = sb.em_mask_batch(masks if per_mask else [masks], B)
    # the bridge's own forward sampler draws the paths of all ensembles at once (ScoreBridge.fwd_sampler_batched)
    own_fwd = is_own_method(sb, fwd_sampler, "fwd_sampler") and is_own_method(sb, unpack, "unpack")
    if own_fwd:                                                                     # preamble (gibbs.py:127-130)
        us_star, vs = sb.fwd_sampler_batched(sk["fwd"], x0s, y0s, mb)               # (T + 1, B, p, c), (T + 1, B, q, c)
        if marg_y:                                                                  # all bridges in one launch, flipped
            vs = doob_bridge_simulator_batched(sk["bridge"], sde, vs[T], vs[0], ts, integration_nsteps=100, replace=True,
                                               reverse=True, time_major=True)
    else:                                                                           # the same, per ensemble
        uss, path_ys = [], []
        for b in range(B):
            path_x, path_y = unpack(fwd_sampler(sk["fwd"][b], x0s[b], y0(b), **kw(b)), **kw(b))
            uss.append(torch.flip(path_x, [0]))
            path_ys.append(path_y)
        us_star = torch.stack(uss, 1).contiguous()                                  # (T + 1, B, p, c)
        if marg_y:
            vs = doob_bridge_simulator_batched(sk["bridge"], sde, torch.stack([p[0] for p in path_ys], 0),
                                               torch.stack([p[-1] for p in path_ys], 0), ts, integration_nsteps=100,
                                               replace=True, reverse=True, time_major=True)
        else:
            vs = torch.stack([torch.flip(p, [0]) for p in path_ys], 1).contiguous()  # (T + 1, B, q, c)
    dev = us_star.device
    bs_np = np.stack([_host_int(bs_stars[b]).reshape(-1) for b in range(B)], 0).astype(np.int32)   # (B, T + 1)
    bs_old = torch.from_numpy(bs_np).to(dev)                                        # (B, T + 1)
    bs_dev = bs_old.T.contiguous()                                                  # (T + 1, B)
    k_res = ops.keys_to_device(sk["resampling"], dev)                               # the whole sweep's keys, uploaded once
    k_tr = ops.keys_to_device(sk["transition"], dev)
    unobs = tuple(us_star.shape[2:])
    du = mb.du
    store = not explicit_backward
    if store:                                                                       # what forward_pass stacks (csmc.py:46)
        uss_all = torch.empty((T + 1, B, rows) + unobs, dtype=torch.float32, device=dev)
        As_all = torch.empty((T, B, rows), dtype=torch.int32, device=dev)

    # initial particles and weights (gibbs.py:132-144, csmc.py:151-155)
    if explicit_final:
        us = uss_all[0] if store else torch.empty((B, rows) + unobs, dtype=torch.float32, device=dev)
        _lib.call("fbsmi_normal_batched", ops.keys_to_device(sk["init"], dev).data_ptr(), B, rows * du, us.data_ptr(),
                  ops._stream())
    else:
        us = us_star[0].unsqueeze(1).expand((B, rows) + unobs)
        if store:
            uss_all[0].copy_(us)
            us = uss_all[0]
        else:
            us = us.clone()
    us[torch.arange(B, device=dev), bs_dev[0].long()] = us_star[0]
    if explicit_final:
        _, lw = sb.fused_step_batched(us, None, vs[0], vs[1], ts[0], None, mb, want_us=False)
    else:
        lw = torch.full((B, rows), -math.log(nparticles), dtype=torch.float32, device=dev)

    for k in range(T):                                                              # csmc.py:132-148 for all ensembles
        w = ops.normalise_batched(lw)                                               # exp(normalise(., log_space=True))
        A = ops.cond_killing_batched(k_res[k], w, bs_dev[k], bs_dev[k + 1], out=As_all[k] if store else None)
        us, lw = sb.fused_step_batched(us, A, vs[k + 1], vs[k], ts[k], k_tr[k], mb, pins=(bs_dev[k + 1], us_star[k + 1]),
                                       out_us=uss_all[k + 1] if store else None)

    if store:                                                                       # csmc.py:34: one backward scan for all
        us_next, bs_next = ops.backscan_batched(sk["bwd"], ops.normalise_batched(lw, log_space=True), As_all, uss_all)
        return us_next[:, -1].contiguous(), us_next, bs_next, bs_next != bs_old     # gibbs.py:157-159

    # postamble: forced move, row pick, fresh indices, comparison -- one launch each (gibbs.py:152-156, 167-168)
    idx = ops.force_move_batched(sk["x0"], ops.normalise_batched(lw), bs_dev[T])
    x0 = _take(us, idx[:, None])[:, 0]
    bs_next = ops.randint_batched(sk["bs"], T + 1, 0, nparticles, device=dev)
    acc = bs_next != bs_old
    if own_fwd:                                                                     # the fresh paths, all at once
        us_next = sb.fwd_sampler_batched(sk["us"], x0, y0s, mb, want_vs=False, batch_major=True)[0]
        return us_next[:, -1].contiguous(), us_next, bs_next, acc
    usn = [torch.flip(unpack(fwd_sampler(sk["us"][b], x0[b], y0(b), **kw(b)), **kw(b))[0], [0]) for b in range(B)]
    us_next = torch.stack(usn, 0)
    return us_next[:, -1].contiguous(), us_next, bs_next, acc
