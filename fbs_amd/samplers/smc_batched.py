"""Bootstrap filters and particle-marginal MH steps of B independent ensembles in lockstep: the test images of one run,
the samples of one image, or both.

The ensembles share the time grid, the SDE and the network, so every SMC step of all of them is one network call on
B * nparticles rows between single launches of the batched sampler kernels (fbs_amd/csrc/fbsmi_batch.hip), instead of B
calls on `nparticles` rows each among a dozen launches per ensemble.  Every function here is the loop of its
single-ensemble namesake in ``smc.py`` / ``gibbs.py`` over the ensembles, with the same keys, run that way, and falls back
to that loop when the lockstep conditions do not hold.  ``gibbs_init_batched`` also draws the Doob bridges of ``marg_y``
(its default) for all ensembles in one launch.  ``bootstrap_backward_smoother_batched`` is the backward smoother of all
ensembles, two launches per step round one network call -- or round none, on the network outputs the filter kept.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib, ops
from ..score import bridge_of, is_own_method
from ..sdes.simulators import doob_bridge_simulator_batched
from . import gibbs_batched as _gibbs_batched
from . import resampling as _resampling
from .common import MCMCState
from .gibbs import gibbs_init
from .gibbs_batched import MAX_LOCKSTEP_ROWS, _is_mask, _take
from .smc import (bootstrap_backward_smoother, bootstrap_filter, pcn_proposal, pmcmc_filter_step, pmcmc_kernel)


def _host_keys(keys) -> np.ndarray:
    return np.asarray(keys.detach().cpu() if isinstance(keys, torch.Tensor) else keys, np.uint32).reshape(-1, 2)


def _step_keys(keys, nsteps: int):
    """split(key, T), then split(., 2) per step, for B keys -> two (T, B, 2) uint32 arrays (first, second)."""
    B, T = keys.shape[0], int(nsteps)
    first, second = np.zeros((T, B, 2), np.uint32), np.zeros((T, B, 2), np.uint32)
    for b in range(B):
        step_keys = ops.split(keys[b], T)
        for k in range(T):
            first[k, b], second[k, b] = ops.split(step_keys[k], 2)
    return first, second


def filter_key_schedule(keys, nsteps: int) -> dict:
    """Every key ``bootstrap_filter`` derives from its own, for B filters, on the host: smc.py:45 (init, steps), :47 (one
    per step) and :56 (proposal, resampling).  -> (B, 2) array 'init' and (nsteps, B, 2) arrays 'proposal', 'resampling',
    all uint32."""
    keys = _host_keys(keys)
    init, steps = np.zeros_like(keys), np.zeros_like(keys)
    for b in range(keys.shape[0]):
        init[b], steps[b] = ops.split(keys[b], 2)
    proposal, resampling = _step_keys(steps, nsteps)
    return {"init": init, "proposal": proposal, "resampling": resampling}


def pmcmc_key_schedule(keys, nsteps: int) -> dict:
    """Every key ``pmcmc_kernel`` derives from its own, for B kernels, on the host: smc.py:296 (prop, u0, filter, mh) and,
    inside ``pmcmc_filter_step``, :255 (one per step) and :261 (proposal, resampling).  -> (B, 2) arrays 'prop', 'u0',
    'filter', 'mh' and (nsteps, B, 2) arrays 'proposal', 'resampling', all uint32."""
    keys = _host_keys(keys)
    out = {name: np.zeros_like(keys) for name in ("prop", "u0", "filter", "mh")}
    for b in range(keys.shape[0]):
        out["prop"][b], out["u0"][b], out["filter"][b], out["mh"][b] = ops.split(keys[b], 4)
    out["proposal"], out["resampling"] = _step_keys(out["filter"], nsteps)
    return out


def _masks_of(kwargs, B: int):
    """(masks, per_mask, kw) of the ``mask_`` keyword: one mask, or a list of B."""
    masks = kwargs.get("mask_")
    per_mask = masks is not None and not _is_mask(masks)
    if per_mask and len(masks) != B:
        raise ValueError(f"{len(masks)} masks for {B} ensembles")
    kw = lambda b: {**kwargs, "mask_": masks[b]} if per_mask else kwargs
    return masks, per_mask, kw


def _lockstep(transition_sampler, weight_closure, resampling, nparticles, kwargs, B: int, log: bool = True):
    """(bridge, resampler name, mask batch) when B ensembles can advance in lockstep, else None: the closures are one
    ScoreBridge's own, ``mask_`` is the only keyword, log weights, the package's stratified or systematic resampler,
    masks of one shape, at most 1024 particles.  Draws nothing."""
    if not log or set(kwargs) != {"mask_"} or int(nparticles) > MAX_LOCKSTEP_ROWS:
        return None
    sb = bridge_of(transition_sampler, weight_closure)
    rname = "stratified" if resampling is _resampling.stratified else (
        "systematic" if resampling is _resampling.systematic else None)
    if sb is None or rname is None:
        return None
    masks, per_mask, kw = _masks_of(kwargs, B)
    ems = [sb._em_mask(kw(b)["mask_"]) for b in range(B)]
    if any((e.du, e.dv) != (ems[0].du, ems[0].dv) for e in ems):
        return None
    return sb, rname, sb.em_mask_batch(masks if per_mask else [masks], B)


def _host_ts(ts):
    """The grid as host floats, read once: the time loop then never waits for the device."""
    return [float(t) for t in (ts.detach().cpu().numpy() if isinstance(ts, torch.Tensor) else np.asarray(ts)).reshape(-1)]


def net_store_fits(nsteps: int, B: int, n: int, D: int, itemsize: int, cap: int = None) -> bool:
    """Whether the network outputs of a whole filter, nsteps * B * n * D elements of `itemsize` bytes, may be kept for the
    backward smoother (``gibbs_init_batched(smoother='reuse')``): at most ``LOCKSTEP_STORE_BYTES`` (or `cap`) bytes.  A
    store above it is not made, and the smoother evaluates the network again."""
    cap = _gibbs_batched.LOCKSTEP_STORE_BYTES if cap is None else cap
    return int(nsteps) * int(B) * int(n) * int(D) * int(itemsize) <= int(cap)


def _filter_lockstep(sb, rname, mb, us, vss, ts, key_proposal, key_resampling, nparticles, return_last, net_store=None):
    """The time loop of ``bootstrap_filter`` (smc.py:55-71) for all ensembles.  us (B, n, p, c) the initial particles.
    net_store: a dict that receives, under 'net', the network output of every step, (T, B * n, D) in the network's dtype
    (step k ran on concat(filtering[k], vs[k]) at ts[k]; with return_last=False only, where no step gathers ancestors),
    or None when ``net_store_fits`` refuses its size."""
    dev = us.device
    nsteps = vss.shape[1] - 1
    kept = None
    vs = vss.transpose(0, 1).contiguous()                                          # (T + 1, B, q, c)
    ts_h = _host_ts(ts)
    k_prop = ops.keys_to_device(key_proposal, dev)                                  # the whole run's keys, uploaded once
    k_res = ops.keys_to_device(key_resampling, dev)
    nell = torch.zeros(us.shape[0], dtype=torch.float32, device=dev)
    logn = np.float32(math.log(nparticles))
    filtering = [us]
    pending = None                                                                  # ancestors not gathered yet
    for k in range(nsteps):
        us_new, lw = sb.fused_step_batched(us, pending, vs[k + 1], vs[k], ts_h[k], k_prop[k], mb)
        if net_store is not None and not return_last:
            net = sb._buf["net"]                                                    # (B * n, D), written by the call above
            if k == 0 and net_store_fits(nsteps, 1, net.shape[0], net.shape[1], net.element_size()):
                kept = torch.empty((nsteps,) + tuple(net.shape), dtype=net.dtype, device=dev)
            if kept is not None:
                kept[k].copy_(net)
        w, c = ops.normalise_batched(lw, return_lse=True)
        nell = nell - (c - logn)
        inds = ops.resample_batched(w, k_res[k], rname)
        if return_last and k < nsteps - 1:
            us, pending = us_new, inds
            continue
        us, pending = _take(us_new, inds), None
        if not return_last:
            filtering.append(us)
    if net_store is not None:
        net_store["net"] = kept
    return (us if return_last else torch.stack(filtering, 1)), nell


def smoother_key_schedule(keys, nsteps: int) -> dict:
    """Every key ``bootstrap_backward_smoother`` uses, for B smoothers, on the host: smc.py:109 draws the index of u_T
    with the PARENT key, and :108, :110 split its second half into one key per step.  -> (B, 2) array 'last' (the parent
    keys) and (nsteps, B, 2) array 'steps', both uint32; steps[s] is the key of the s-th backward step, the one that
    picks time nsteps - 1 - s."""
    keys = _host_keys(keys)
    B, T = keys.shape[0], int(nsteps)
    steps = np.zeros((T, B, 2), np.uint32)
    for b in range(B):
        steps[:, b] = ops.split(ops.split(keys[b], 2)[1], T)
    return {"last": keys.copy(), "steps": steps}


def _backsim_lockstep(transition_logpdf, nrows: int, kwargs, B: int):
    """(bridge, mask batch) when the backward pass of B ensembles can advance in lockstep, else None: the closure is one
    ScoreBridge's own ``transition_logpdf``, ``mask_`` is the only keyword, masks of one shape, at most 1024 rows."""
    sb = getattr(transition_logpdf, "__self__", None)
    if set(kwargs) != {"mask_"} or int(nrows) > MAX_LOCKSTEP_ROWS or not is_own_method(sb, transition_logpdf,
                                                                                      "transition_logpdf"):
        return None
    masks, per_mask, kw = _masks_of(kwargs, B)
    ems = [sb._em_mask(kw(b)["mask_"]) for b in range(B)]
    if any((e.du, e.dv) != (ems[0].du, ems[0].dv) for e in ems):
        return None
    return sb, sb.em_mask_batch(masks if per_mask else [masks], B)


def bootstrap_backward_smoother_batched(keys, filter_uss, vss, ts, transition_logpdf, network_outputs=None, **kwargs):
    """``bootstrap_backward_smoother`` for B ensembles: keys (B, 2), filter_uss (B, T + 1, n, p, c) as
    ``bootstrap_filter_batched(return_last=False)`` returns them, vss (B, T + 1, q, c), ``mask_`` one mask or a list of B.
    Returns the trajectories (B, T + 1, p, c), equal to

        torch.stack([bootstrap_backward_smoother(keys[b], filter_uss[b], vss[b], ts, transition_logpdf, mask_=masks[b])])

    bit for bit whenever the score function's output row does not depend on which other rows share its call.

    The ensembles advance in lockstep when the closure is one ScoreBridge's own ``transition_logpdf``, ``mask_`` is the
    only keyword, the masks have one shape and n <= 1024: per step one network call on B * n rows
    (``ScoreBridge.transition_logpdf_batched``) and two launches -- fbsmi_em_translp_batched, then
    fbsmi_backsim_pick_batched, which writes the picked row straight into the preallocated trajectory where the next step
    reads it as its target -- with every key uploaded once and nothing read back inside the loop.  Anything else runs the
    loop above.

    network_outputs (T, B * n, D): the network's output on concat(filter_uss[:, t], vss[:, t]) at ts[t] for every t, in
    its own dtype -- what the filter that produced filter_uss computed at its step t.  With it the lockstep pass makes
    no network call at all; the loop ignores it."""
    keys = _host_keys(keys)
    B = keys.shape[0]
    n = int(filter_uss.shape[2])
    lock = _backsim_lockstep(transition_logpdf, n, kwargs, B)
    if lock is None:
        _, _, kw = _masks_of(kwargs, B)
        return torch.stack([bootstrap_backward_smoother(keys[b], filter_uss[b], vss[b], ts, transition_logpdf, **kw(b))
                            for b in range(B)], 0)
    sb, mb = lock
    dev = filter_uss.device
    T = int(filter_uss.shape[1]) - 1
    if network_outputs is not None and (network_outputs.dim() != 3 or int(network_outputs.shape[0]) != T):
        raise ValueError("network_outputs must be (T, B * n, D)")
    filter_uss = ops._f32c(filter_uss, "filter_uss")
    vss = ops._f32c(vss, "vss")
    ts_h = _host_ts(ts)
    sk = smoother_key_schedule(keys, T)
    k_steps = ops.keys_to_device(sk["steps"], dev)                                  # the whole pass's keys, uploaded once
    traj = torch.empty((B, T + 1) + tuple(filter_uss.shape[3:]), dtype=torch.float32, device=dev)
    last = ops.randint_batched(sk["last"], 1, 0, n, device=dev)                     # :109, (B, 1)
    traj[:, T] = _take(filter_uss[:, T], last)[:, 0]
    for s in range(T):                                                              # filter_us[-2::-1], vs[-2::-1], ts[-2::-1]
        t = T - 1 - s
        lw = sb.transition_logpdf_batched(traj[:, t + 1], filter_uss[:, t], vss[:, t], ts_h[t], mb,
                                          net=None if network_outputs is None else network_outputs[t])     # :101
        ops.backsim_pick_batched(k_steps[s], lw, filter_uss[:, t], out=traj[:, t])  # :103-104 and the row gather
    return traj


def bootstrap_filter_batched(transition_sampler, measurement_cond_pdf, vss, ts, init_sampler, keys, nparticles, resampling,
                             log: bool = True, return_last: bool = True, **kwargs):
    """``bootstrap_filter`` for B ensembles: vss (B, T + 1, q, c), keys (B, 2), ``mask_`` one mask or a list of B masks.
    Returns (samples (B, n, p, c) [return_last] or (B, T + 1, n, p, c), nell (B,)), equal to the stacked results of

        [bootstrap_filter(..., vss[b], ts, init_sampler, keys[b], ..., mask_=masks[b]) for b in range(B)]

    bit for bit whenever the score function's output row does not depend on which other rows share its call.  That is
    not promised for a real UNet: library convolution and matrix kernels may be chosen by batch size and differ in the
    last bits, after which a resampling decision can flip and the two runs part ways as two valid draws.

    The ensembles advance in lockstep -- one network call per step, one launch per sampler operation, no host
    synchronisation inside the time loop -- when the closures are one ScoreBridge's own, ``mask_`` is the only keyword,
    log is set, resampling is this package's stratified or systematic, the masks have one shape and nparticles <= 1024.
    Anything else runs the loop above: the same result without the speed-up."""
    keys = _host_keys(keys)
    B = keys.shape[0]
    lock = _lockstep(transition_sampler, measurement_cond_pdf, resampling, nparticles, kwargs, B, log)
    if lock is None:
        _, _, kw = _masks_of(kwargs, B)
        outs = [bootstrap_filter(transition_sampler, measurement_cond_pdf, vss[b], ts, init_sampler, keys[b], nparticles,
                                 resampling, log=log, return_last=return_last, **kw(b)) for b in range(B)]
        return torch.stack([o[0] for o in outs], 0), torch.stack([o[1].reshape(()) for o in outs], 0)
    sb, rname, mb = lock
    sk = filter_key_schedule(keys, vss.shape[1] - 1)
    us = torch.stack([init_sampler(sk["init"][b], vss[b, 0], nparticles) for b in range(B)], 0)
    return _filter_lockstep(sb, rname, mb, us, vss, ts, sk["proposal"], sk["resampling"], nparticles, return_last)


def pmcmc_filter_step_batched(keys, vss, u0s, ts, transition_sampler, likelihood_logpdf, resampling, nparticles, **kwargs):
    """``pmcmc_filter_step`` for B ensembles: keys (B, 2), vss (B, T + 1, q, c), u0s (B, n, p, c) -> (us (B, n, p, c),
    log_ell (B,)), the stacked results of the loop over the ensembles under the contract and the lockstep conditions of
    ``bootstrap_filter_batched``."""
    keys = _host_keys(keys)
    B = keys.shape[0]
    lock = _lockstep(transition_sampler, likelihood_logpdf, resampling, nparticles, kwargs, B)
    if lock is None:
        _, _, kw = _masks_of(kwargs, B)
        outs = [pmcmc_filter_step(keys[b], vss[b], u0s[b], ts, transition_sampler, likelihood_logpdf, resampling,
                                  nparticles, **kw(b)) for b in range(B)]
        return torch.stack([o[0] for o in outs], 0), torch.stack([o[1].reshape(()) for o in outs], 0)
    sb, rname, mb = lock
    nsteps = (ts.shape[0] if hasattr(ts, "shape") else len(ts)) - 1
    key_proposal, key_resampling = _step_keys(keys, nsteps)
    return _pmcmc_lockstep(sb, rname, mb, u0s, vss, ts, key_proposal, key_resampling, nparticles)


def _pmcmc_lockstep(sb, rname, mb, us, vss, ts, key_proposal, key_resampling, nparticles):
    """The time loop of ``pmcmc_filter_step`` (smc.py:260-272) for all ensembles."""
    dev = us.device
    nsteps = len(key_proposal)
    vs = vss.transpose(0, 1).contiguous()
    ts_h = _host_ts(ts)
    k_prop = ops.keys_to_device(key_proposal, dev)
    k_res = ops.keys_to_device(key_resampling, dev)
    log_ell = torch.zeros(us.shape[0], dtype=torch.float32, device=dev)
    logn = np.float32(math.log(nparticles))
    for k in range(nsteps):
        cell = {}

        def resample(lw):
            w, cell["c"] = ops.normalise_batched(lw, return_lse=True)
            return ops.resample_batched(w, k_res[k], rname)

        us, _, _ = sb.fused_weight_then_propose_batched(us, vs[k + 1], vs[k], ts_h[k], k_prop[k], mb, resample)
        log_ell = (log_ell - logn) + cell["c"]
    return us, log_ell


def _per_ensemble(x, B: int, inner_dim: int):
    """b -> x[b] when x is a list of B or a tensor with a leading axis B over `inner_dim`-dimensional items, else b -> x."""
    batched = isinstance(x, (list, tuple)) or (isinstance(x, torch.Tensor) and x.dim() == inner_dim + 1)
    if batched and len(x) != B:
        raise ValueError(f"{len(x)} observations for {B} ensembles")
    return (lambda b: x[b]) if batched else (lambda b: x)


def pmcmc_kernel_batched(keys, uTs, log_ells, yss, y0s, ts, fwd_ys_sampler, sde, ref_sampler, transition_sampler,
                         likelihood_logpdf, resampling, nparticles, delta: float = None, which_u: int = 0, **kwargs):
    """``pmcmc_kernel`` for B ensembles: keys (B, 2), uTs (B, p, c), log_ells (B,), yss (B, T + 1, q, c), y0s one
    observation (q, c) or B of them.  Returns (uTs, log_ells, yss, MCMCState of (B,) tensors), the stacked results of the
    loop over the ensembles under the contract and the lockstep conditions of ``bootstrap_filter_batched``.
    ``ref_sampler`` runs per ensemble, and so does the proposal unless ``fwd_ys_sampler`` is the bridge's own method: then
    the observation paths of all ensembles (both draws of a pCN proposal: 2 B paths) are one launch
    (``ScoreBridge.fwd_ys_sampler_batched``).  The filter advances in lockstep and the accept step is taken on the device
    for all ensembles at once, without reading anything back."""
    keys = _host_keys(keys)
    B = keys.shape[0]
    y0 = _per_ensemble(y0s, B, yss.dim() - 2)
    lock = _lockstep(transition_sampler, likelihood_logpdf, resampling, nparticles, kwargs, B)
    if lock is None:
        _, _, kw = _masks_of(kwargs, B)
        outs = [pmcmc_kernel(keys[b], uTs[b], log_ells[b], yss[b], y0(b), ts, fwd_ys_sampler, sde, ref_sampler,
                             transition_sampler, likelihood_logpdf, resampling, nparticles, delta=delta, which_u=which_u,
                             **kw(b)) for b in range(B)]
        state = MCMCState(*(torch.stack([o[3][i].reshape(()) for o in outs], 0) for i in range(len(MCMCState._fields))))
        return (torch.stack([o[0] for o in outs], 0), torch.stack([o[1].reshape(()) for o in outs], 0),
                torch.stack([o[2] for o in outs], 0), state)
    sb, rname, mb = lock
    dev = yss.device
    nsteps = yss.shape[1] - 1
    sk = pmcmc_key_schedule(keys, nsteps)
    if delta is not None:                                                           # smc.py:300-304
        ts_np = np.asarray(ts.detach().cpu() if isinstance(ts, torch.Tensor) else ts, np.float64).reshape(-1)
        coef = torch.as_tensor(np.asarray(sde.mean(ts_np, ts_np[0], 1.0), np.float32), device=dev)
    props, u0s, zs = [], [], []
    own_fwd = is_own_method(sb, fwd_ys_sampler, "fwd_ys_sampler")
    if own_fwd and delta is None:                                                   # all proposals in one launch (:297-298)
        prop_yss = sb.fwd_ys_sampler_batched(sk["prop"], y0s)
    elif own_fwd:                                                                   # pcn_proposal (:282-288), stacked: both
        key_rnds = np.stack([ops.split(sk["prop"][b], 2) for b in range(B)], 1)     # draws of all ensembles in one launch
        y0_t = sb._rows(y0s, B, int(np.prod(yss.shape[2:])), "y0s").reshape((B,) + tuple(yss.shape[2:]))
        rnds = sb.fwd_ys_sampler_batched(key_rnds.reshape(2 * B, 2), torch.cat([y0_t, y0_t], 0))
        rnds0, rnds1 = rnds[:B], rnds[B:]
        mean = (coef.reshape((1, -1) + (1,) * (y0_t.dim() - 1)) * y0_t.unsqueeze(1)).reshape(yss.shape)
        beta = 2 / (2 + delta)
        p = yss + math.sqrt(delta / 2) * (rnds0 - mean)
        prop_yss = beta * p + (1 - beta) * mean + math.sqrt(1 - beta) * (rnds1 - mean)
    for b in range(B):                                                              # preamble, per ensemble (:297-307, :314)
        y0_b = y0(b)
        if own_fwd:
            prop_ys = prop_yss[b]
        elif delta is None:
            prop_ys = fwd_ys_sampler(sk["prop"][b], y0_b)
        else:
            y0_t = y0_b if isinstance(y0_b, torch.Tensor) else torch.as_tensor(np.asarray(y0_b, np.float32), device=dev)
            mean = (coef.reshape((-1,) + (1,) * y0_t.dim()) * y0_t).reshape(yss[b].shape)
            prop_ys = pcn_proposal(sk["prop"][b], delta, yss[b], mean, lambda key_: fwd_ys_sampler(key_, y0_b))
        props.append(prop_ys)
        u0s.append(ref_sampler(sk["u0"][b], torch.flip(prop_ys, [0])[0], nparticles))
        zs.append(ops.uniform(sk["mh"][b], (), device=dev))
    if not own_fwd:
        prop_yss = torch.stack(props, 0)
    prop_uTs, prop_log_ell = _pmcmc_lockstep(sb, rname, mb, torch.stack(u0s, 0), torch.flip(prop_yss, [1]), ts,
                                             sk["proposal"], sk["resampling"], nparticles)
    prop_uT = prop_uTs[:, which_u]
    log_ell_t = (log_ells if isinstance(log_ells, torch.Tensor) else
                 torch.as_tensor(np.asarray(log_ells, np.float32), device=dev)).to(torch.float32).reshape(B)
    log_acc_prob = torch.minimum(torch.zeros_like(prop_log_ell), prop_log_ell - log_ell_t)       # :313
    acc = ops.math_map("log", torch.stack(zs, 0)) < log_acc_prob                    # :315
    state = MCMCState(acceptance_prob=torch.exp(log_acc_prob), is_accepted=acc, prop_log_ell=prop_log_ell,
                      log_ell=log_ell_t)
    pick = lambda new, old: torch.where(acc.reshape((B,) + (1,) * (new.dim() - 1)), new, old)
    return pick(prop_uT, uTs), pick(prop_log_ell, log_ell_t), pick(prop_yss, yss), state


def gibbs_init_batched(keys, y0s, x0_shape, ts, fwd_sampler, sde, unpack, transition_sampler, transition_logpdf,
                       likelihood_logpdf, nparticles, method: str = 'smoother', marg_y: bool = True, x0s=None,
                       smoother: str = 'loop', **kwargs):
    """``gibbs_init`` for B ensembles: keys (B, 2), y0s one observation or B of them, x0s None or (B, p, c), ``mask_`` one
    mask or a list of B.  Returns (approx_x0 (B, ...), approx_us_star (B, T + 1, p, c) or None for 'debug'), the stacked
    results of the loop over the ensembles under the contract and the lockstep conditions of
    ``bootstrap_filter_batched``.  With 'filter' and 'smoother' the bootstrap filters advance in lockstep, and so do the
    forward paths when ``fwd_sampler`` and ``unpack`` are the bridge's own methods (``ScoreBridge.fwd_sampler_batched``;
    any other closure is called per ensemble); with marg_y the Doob bridges of all ensembles are one launch
    (``doob_bridge_simulator_batched``) and the initial particles of all ensembles are one draw.  'debug' and 'kalman'
    run the loop.

    ``smoother`` says how the backward smoother of method 'smoother' runs behind the lockstep filter:
    'loop' (the default), per ensemble: B * T network calls of `nparticles` rows; 'lockstep',
    ``bootstrap_backward_smoother_batched``: T network calls for all ensembles; 'reuse', the same with the network
    outputs the filter computed -- step t of the smoother evaluates the network on concat(filter_us[t], vs[t]) at ts[t],
    the input of the filter's step t -- kept in a (T, B * nparticles, D) array of the network's dtype, so the backward
    pass makes no network call.  A store above ``LOCKSTEP_STORE_BYTES`` is not made and 'reuse' runs 'lockstep'.  The
    three give the same bits under the contract above."""
    if smoother not in ("loop", "lockstep", "reuse"):
        raise ValueError(f"Unknown smoother {smoother}")
    keys = _host_keys(keys)
    B = keys.shape[0]
    y0 = _per_ensemble(y0s, B, len(tuple(x0_shape)))
    _, _, kw = _masks_of(kwargs, B)
    lock = _lockstep(transition_sampler, likelihood_logpdf, _resampling.stratified, nparticles, kwargs, B) \
        if method in ("filter", "smoother") else None
    if lock is None:
        outs = [gibbs_init(keys[b], y0(b), x0_shape, ts, fwd_sampler, sde, unpack, transition_sampler, transition_logpdf,
                           likelihood_logpdf, nparticles, method=method, marg_y=marg_y,
                           x0=None if x0s is None else x0s[b], **kw(b)) for b in range(B)]
        return (torch.stack([o[0] for o in outs], 0),
                None if outs[0][1] is None else torch.stack([o[1] for o in outs], 0))
    sb, rname, mb = lock
    y00 = y0(0)
    dev = y00.device if isinstance(y00, torch.Tensor) else ops._default_device()
    ks = [ops.split(keys[b], 6) for b in range(B)]                                  # gibbs.py:40: fwd, bridge, u0, bf, fwd2, bwd
    key_of = lambda i: np.stack([ks[b][i] for b in range(B)], 0)
    # the bridge's own forward sampler draws the paths of all ensembles at once (ScoreBridge.fwd_sampler_batched)
    own_fwd = is_own_method(sb, fwd_sampler, "fwd_sampler") and is_own_method(sb, unpack, "unpack")
    if own_fwd:                                                                     # preamble (gibbs.py:38-47)
        x0_all = torch.zeros((B,) + tuple(x0_shape), dtype=torch.float32, device=dev) if x0s is None else x0s
        _, vss = sb.fwd_sampler_batched(key_of(0), x0_all, y0s, mb, batch_major=True)
        ends = (vss[:, -1], vss[:, 0])                                              # the paths' two ends, in forward order
    else:                                                                           # the same, per ensemble
        path_ys = []
        for b in range(B):
            x0 = torch.zeros(tuple(x0_shape), dtype=torch.float32, device=dev) if x0s is None else x0s[b]
            path_ys.append(unpack(fwd_sampler(ks[b][0], x0, y0(b), **kw(b)), **kw(b))[1])
        if marg_y:
            ends = (torch.stack([p[0] for p in path_ys], 0), torch.stack([p[-1] for p in path_ys], 0))
        else:
            vss = torch.stack([torch.flip(p, [0]) for p in path_ys], 0)
    if marg_y:                                                                      # the bridges of all ensembles: one launch
        vss = doob_bridge_simulator_batched(key_of(1), sde, ends[0], ends[1], ts, integration_nsteps=100, replace=True,
                                            reverse=True)
    u0s = torch.empty((B, nparticles) + tuple(x0_shape), dtype=torch.float32, device=dev)
    _lib.call("fbsmi_normal_batched", ops.keys_to_device(key_of(2), dev).data_ptr(), B, u0s[0].numel(), u0s.data_ptr(),
              ops._stream())
    sk = filter_key_schedule(key_of(3), vss.shape[1] - 1)
    # the filter's network outputs serve the smoother only when it evaluates the same bridge
    store = {} if (method == "smoother" and smoother == "reuse"
                   and is_own_method(sb, transition_logpdf, "transition_logpdf")) else None
    uss, _ = _filter_lockstep(sb, rname, mb, u0s, vss, ts, sk["proposal"], sk["resampling"], nparticles,
                              method == "filter", net_store=store)
    if method == "smoother" and smoother != "loop":                                 # postamble (gibbs.py:56-57), at once
        return uss[:, -1, 0].contiguous(), bootstrap_backward_smoother_batched(
            key_of(5), uss, vss, ts, transition_logpdf, network_outputs=None if store is None else store["net"], **kwargs)
    if own_fwd and method == "filter":                                              # postamble (gibbs.py:49-52), at once
        approx_x0 = uss[:, 0].contiguous()
        return approx_x0, sb.fwd_sampler_batched(np.stack([ks[b][4] for b in range(B)], 0), approx_x0, y0s, mb,
                                                 want_vs=False, batch_major=True)[0]
    x0n, usn = [], []
    for b in range(B):                                                              # postamble, per ensemble (gibbs.py:49-57)
        if method == "filter":
            approx_x0 = uss[b, 0]
            us_star = torch.flip(unpack(fwd_sampler(ks[b][4], approx_x0, y0(b), **kw(b)), **kw(b))[0], [0])
        else:
            approx_x0 = uss[b, -1, 0]
            us_star = bootstrap_backward_smoother(ks[b][5], uss[b], vss[b], ts, transition_logpdf, **kw(b))
        x0n.append(approx_x0)
        usn.append(us_star)
    return torch.stack(x0n, 0), torch.stack(usn, 0)
