"""Bootstrap particle filter, backward smoother, particle-marginal MH (fbs/samplers/smc.py).

Closures are Python callables on GPU tensors as in the reference; resampling, gathers, logsumexp
and categorical draws are libfbsmi kernels.  Each function reproduces the reference's step order
(the three loops differ: see SURVEY.md section 3.3).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import ops
from ..lg_twisted import fused_twisted
from ..score import bridge_of
from . import resampling as _resampling
from .common import MCMCState


def _fused_filter(transition_sampler, weight_closure, resampling, kwargs, nparticles):
    """(model, resampling name) when the fused analytic-model filter applies, else None."""
    model = getattr(transition_sampler, "_fbsmi_lg", None)
    if model is None or getattr(weight_closure, "_fbsmi_lg", None) is not model or kwargs:
        return None
    if getattr(weight_closure, "_role", "") != "likelihood_logpdf" or not model.fused_filter_supported(nparticles):
        return None
    name = "stratified" if resampling is _resampling.stratified else (
        "systematic" if resampling is _resampling.systematic else None)
    return (model, name) if name else None


def bootstrap_filter(transition_sampler, measurement_cond_pdf, vs, ts, init_sampler, key, nparticles, resampling,
                     log: bool = True, return_last: bool = True, **kwargs):
    """Bootstrap particle filter (smc.py:9-88) -> (samples, negative log-likelihood)."""
    nsteps = vs.shape[0] - 1
    fused = _fused_filter(transition_sampler, measurement_cond_pdf, resampling, kwargs, nparticles) if log else None
    if fused is not None and fused[0].T == nsteps:
        model, rname = fused
        key_init, _ = ops.split(key, 2)                                             # :77
        init_samples = init_sampler(key_init, vs[0], nparticles)                    # :78
        out = model.filter_handle(nparticles, "bootstrap", rname, store_path=not return_last).run(key, vs, init_samples)
        return (out[0].reshape(init_samples.shape), out[1]) if return_last else (
            out[2].reshape((nsteps + 1,) + tuple(init_samples.shape)), out[1])
    key_init, key_steps = ops.split(key, 2)                                         # :77
    us_prev = init_sampler(key_init, vs[0], nparticles)                             # :78
    keys = ops.split(key_steps, nsteps)                                             # :79
    log_nell = torch.zeros((), dtype=torch.float32, device=us_prev.device)
    logn = np.float32(math.log(nparticles))
    filtering = [us_prev]
    # closures of one ScoreBridge (log weights): one network evaluation per step, and with return_last the
    # resampling gather of step k is folded into the network-input kernel of step k + 1
    sb = bridge_of(transition_sampler, measurement_cond_pdf) if (log and set(kwargs) == {"mask_"}) else None
    pending = None                                                                  # ancestors not gathered yet
    for k in range(nsteps):                                                         # scan_body :58-74
        key_proposal, key_resampling = ops.split(keys[k], 2)
        v, v_prev, t_prev = vs[k + 1], vs[k], ts[k]
        if sb is not None:
            us, log_weights = sb.fused_step(us_prev, pending, v, v_prev, t_prev, key_proposal, kwargs["mask_"])
        else:
            us = transition_sampler(us_prev, v_prev, t_prev, key_proposal, **kwargs)    # :63
            log_weights = measurement_cond_pdf(v, us_prev, v_prev, t_prev, **kwargs)    # :65
        weights, c = ops.normalise(log_weights, log_space=False, return_lse=True)   # :66,68,69
        log_nell = log_nell - (c - logn)                                            # :67
        inds = resampling(weights, key_resampling)
        if sb is not None and return_last and k < nsteps - 1:
            us_prev, pending = us, inds
            continue
        us_prev, pending = ops.take_rows(us, inds), None                            # :72
        if not return_last:
            filtering.append(us_prev)
    if return_last:
        return us_prev, log_nell
    return torch.stack(filtering, 0), log_nell


FSAMP_STATE_ELEMS = 1 << 26   # B * N * du float32 elements of ONE particle buffer of a fused call: 256 MB
FSAMP_MAX_SAMPLES = 16384     # samples per fused call (the engine itself takes 65535, the grid's y extent)


def plan_filter_chunks(nkeys: int, nparticles: int, du: int, bound: int = FSAMP_STATE_ELEMS,
                       max_samples: int = FSAMP_MAX_SAMPLES):
    """[(start, stop), ..] covering range(nkeys) in order, each with (stop - start) * nparticles * du <= bound elements and at
    most max_samples samples; None when one sample alone exceeds the bound.

    The bound is on one particle buffer (B, N, du), not on the handle: a flow-0 filter of B chains holds four such buffers
    (two generations, the final particles, the staging of the initial ones) plus five (B, N) weight / cdf rows, and a wide
    model (du or dv > 16) two more (B, N, du) noise buffers and dv + 1 rows -- 4 + 5 / du times the bound for a narrow model
    (9 x at du = 1: 2.3 GB at the full bound), about 7 to 8 times for a wide one -- and per-step tables of B * T * (8 + 2 D)
    words, which max_samples keeps to 0.1 GB at T = 200, D = 2.  Every distinct chunk size is a handle of its own, cached
    on the bridge for its lifetime."""
    per = int(nparticles) * int(du)
    if per > bound:
        return None
    step = max(1, min(int(max_samples), bound // per))
    return [(s, min(s + step, int(nkeys))) for s in range(0, int(nkeys), step)]


def _fused_filter_sampler(ts, fwd_ys_sampler, ref_sampler, transition_sampler, likelihood_logpdf, nparticles, resampling):
    """(model, resampling name) when the fused filter sampler (LGFilterSampler) applies: the four closures belong to one
    LinearGaussianBridge in their own roles, ts is its grid, its forward transition is exact, the resampler is one the
    fused filter has and the engine takes the size; else None.  Touches no device."""
    fused = _fused_filter(transition_sampler, likelihood_logpdf, resampling, {}, nparticles)
    if fused is None:
        return None
    model = fused[0]
    for closure, role in ((fwd_ys_sampler, "fwd_ys_sampler"), (ref_sampler, "ref_sampler"),
                          (transition_sampler, "transition_sampler")):
        if getattr(closure, "_fbsmi_lg", None) is not model or getattr(closure, "_role", "") != role:
            return None
    if not model.fused_filter_sampler_supported(nparticles, 1) or not model.same_grid(ts):
        return None
    return fused


def filter_conditional_sampler(keys, y0, ts, fwd_ys_sampler, ref_sampler, transition_sampler, likelihood_logpdf,
                               nparticles, resampling, return_nell=False, _bound=FSAMP_STATE_ELEMS):
    """The bootstrap-filter conditional sampler of experiments/toy/gp_filter.py:134-142 for every key of `keys` (B, 2)
    [or (2,)]: -> samples (B, du) [, negative log-likelihood estimates (B)].  Each sample depends on its own key only.

    With the closures of one LinearGaussianBridge on its own grid and stratified / systematic resampling the batch runs on
    the device (LGFilterSampler), in chunks of samples that keep B * N * du within `_bound` elements per call; otherwise
    the driver's body runs once per key."""
    k = np.asarray(keys.detach().cpu() if isinstance(keys, torch.Tensor) else keys).astype(np.uint32).reshape(-1, 2)
    fused = _fused_filter_sampler(ts, fwd_ys_sampler, ref_sampler, transition_sampler, likelihood_logpdf, nparticles,
                                  resampling)
    chunks = plan_filter_chunks(k.shape[0], nparticles, fused[0].du, _bound) if fused is not None else None
    if chunks:
        model, rname = fused
        outs = [model.filter_sampler_handle(nparticles, rname, b - a).sample(k[a:b], y0, return_nell=True) for a, b in chunks]
        samples, nell = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
        return (samples, nell) if return_nell else samples
    samples, nells = [], []
    for key_ in k:                                                                  # gp_filter.py:134-142
        key_fwd, key_bwd, key_bf = ops.split(key_, 3)
        vs = torch.flip(fwd_ys_sampler(key_fwd, y0), [0])
        us, nell = bootstrap_filter(transition_sampler, likelihood_logpdf, vs, ts, ref_sampler, key_bf, nparticles,
                                    resampling, log=True, return_last=True)
        samples.append(us[0])
        nells.append(nell.reshape(()))
    samples, nells = torch.stack(samples), torch.stack(nells)
    return (samples, nells) if return_nell else samples


def _fused_sb_filter_sampler(ts, fwd_sampler, unpack, ref_sampler, transition_sampler, likelihood_logpdf, nparticles,
                             resampling):
    """(model, resampling name) when the fused SB filter sampler (SBFilterSampler) applies: the five closures belong to
    one GaussianSBBridge in their own roles, ts is its grid, the resampler is one the fused filter has and the engine takes
    the size; else None.  Touches no device."""
    fused = _fused_filter(transition_sampler, likelihood_logpdf, resampling, {}, nparticles)
    if fused is None:
        return None
    model = fused[0]
    for closure, role in ((fwd_sampler, "fwd_sampler"), (unpack, "unpack"), (ref_sampler, "ref_sampler"),
                          (transition_sampler, "transition_sampler")):
        if getattr(closure, "_fbsmi_lg", None) is not model or getattr(closure, "_role", "") != role:
            return None
    supported = getattr(model, "fused_sb_filter_sampler_supported", None)   # (a LinearGaussianBridge has none)
    if supported is None or not supported(nparticles, 1) or not model.same_grid(ts):
        return None
    return fused


def sb_filter_conditional_sampler(keys, y0, ts, fwd_sampler, unpack, ref_sampler, transition_sampler, likelihood_logpdf,
                                  nparticles, resampling, x0_prior=None, return_nell=False, _bound=FSAMP_STATE_ELEMS):
    """The bootstrap-filter conditional sampler of experiments/sb/filter.py:137-161 for every key of `keys` (B, 2)
    [or (2,)]: -> samples (B, du) [, negative log-likelihood estimates (B)].  The observation path is the y half of
    fwd_sampler's joint path from (x0, y0), x0 = mean + normal @ chol_lower with x0_prior = (mean, chol_lower) ('proper')
    or x0 = normal with None ('heuristic').  Each sample depends on its own key only.

    With the closures of one GaussianSBBridge on its own grid and stratified / systematic resampling the batch runs on the
    device (SBFilterSampler), in chunks of samples that keep B * N * du within `_bound` elements per call; otherwise the
    driver's body runs once per key (x0 then has the prior mean's size, or the du of the bridge that fwd_sampler belongs to;
    with neither the size is unknown and a ValueError is raised)."""
    k = np.asarray(keys.detach().cpu() if isinstance(keys, torch.Tensor) else keys).astype(np.uint32).reshape(-1, 2)
    fused = _fused_sb_filter_sampler(ts, fwd_sampler, unpack, ref_sampler, transition_sampler, likelihood_logpdf,
                                     nparticles, resampling)
    chunks = plan_filter_chunks(k.shape[0], nparticles, fused[0].du, _bound) if fused is not None else None
    if chunks:
        model, rname = fused
        outs = [model.sb_filter_sampler_handle(nparticles, rname, b - a, x0_prior).sample(k[a:b], y0, return_nell=True)
                for a, b in chunks]
        samples, nell = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
        return (samples, nell) if return_nell else samples
    model = getattr(fwd_sampler, "_fbsmi_lg", None)
    if x0_prior is None and model is None:
        raise ValueError("sb_filter_conditional_sampler: the size of x0 is unknown -- closures that are not a bridge's own "
                         "need x0_prior = (mean, chol_lower)")
    dev = y0.device if isinstance(y0, torch.Tensor) else (model.device if model is not None else ops._default_device())
    y0 = y0 if isinstance(y0, torch.Tensor) else torch.as_tensor(np.asarray(y0, np.float32), device=dev)
    if x0_prior is not None:
        mean, chol = (torch.as_tensor(np.asarray(a, np.float32), device=dev) for a in x0_prior)
    du = int(mean.numel()) if x0_prior is not None else model.du
    samples, nells = [], []
    for key_ in k:                                                                  # sb/filter.py:137-161
        key_fwd, key_bwd, key_bf = ops.split(key_, 3)
        key_x0, key_em = ops.split(key_fwd)
        x0 = ops.normal(key_x0, (du,), device=dev)
        if x0_prior is not None:
            x0 = mean + x0 @ chol
        vs = torch.flip(unpack(fwd_sampler(key_em, x0, y0))[1], [0])
        us, nell = bootstrap_filter(transition_sampler, likelihood_logpdf, vs, ts, ref_sampler, key_bf, nparticles,
                                    resampling, log=True, return_last=True)
        samples.append(us[0])
        nells.append(nell.reshape(()))
    samples, nells = torch.stack(samples), torch.stack(nells)
    return (samples, nells) if return_nell else samples


def fused_backsim(transition_logpdf, args, kwargs, ts, path):
    """The model whose fused backward simulation (LGBacksim) applies to a stored float32 path (T+1, n, du): the closure is
    one LinearGaussianBridge's own transition_logpdf, called without extra arguments on the bridge's own grid, and the
    engine takes the size; else None."""
    model = getattr(transition_logpdf, "_fbsmi_lg", None)
    if model is None or getattr(transition_logpdf, "_role", "") != "transition_logpdf" or args or kwargs:
        return None
    if not isinstance(path, torch.Tensor) or path.dtype != torch.float32 or path.dim() != 3:
        return None
    if path.shape[0] != model.T + 1 or path.shape[2] != model.du or not model.fused_backsim_supported(path.shape[1]):
        return None
    return model if model.same_grid(ts) else None


def bootstrap_backward_smoother(key, filter_us, vs, ts, transition_logpdf, *args, **kwargs):
    """Backward particle smoother on bootstrap-filter output (smc.py:91-112).  With the transition_logpdf of one
    LinearGaussianBridge on its own grid the whole pass runs fused on the device (LGBacksim); otherwise the host loop."""
    model = fused_backsim(transition_logpdf, args, kwargs, ts, filter_us)
    if model is not None:
        return model.backsim_handle(filter_us.shape[1], "smoother").run(key, vs, filter_us)
    nsteps = filter_us.shape[0] - 1
    key_last, key_smoother = ops.split(key, 2)                                      # :108
    uT = ops.choice(key, filter_us[-1], axis=0)   # :109 -- the reference draws with the PARENT key
    keys = ops.split(key_smoother, nsteps)
    traj = [uT]
    u_kp1 = uT
    for s in range(nsteps):                       # filter_us[-2::-1], vs[-2::-1], ts[-2::-1]
        t = nsteps - 1 - s
        log_ws = transition_logpdf(u_kp1, filter_us[t], vs[t], ts[t], *args, **kwargs)  # :101
        w = ops.normalise(log_ws, log_space=False)                                  # :103
        i = ops.categorical(keys[s], w)                                             # :104
        u_kp1 = filter_us[t][i.long()]
        traj.append(u_kp1)
    return torch.stack(traj[::-1], 0)


def pmcmc_filter_step(key, vs_bridge, u0s, ts, transition_sampler, likelihood_logpdf, resampling, nparticles,
                      **kwargs):
    """Particle filter inside pMCMC (smc.py:115-158): weight -> resample old -> propagate."""
    nsteps = (ts.shape[0] if hasattr(ts, "shape") else len(ts)) - 1
    fused = _fused_filter(transition_sampler, likelihood_logpdf, resampling, kwargs, nparticles)
    if fused is not None and fused[0].T == nsteps:
        model, rname = fused
        uT, ell = model.filter_handle(nparticles, "pmcmc", rname).run(key, vs_bridge, u0s)
        return uT.reshape(u0s.shape), ell
    keys = ops.split(key, nsteps)                                                   # :154
    us = u0s
    log_ell = torch.zeros((), dtype=torch.float32, device=u0s.device)
    logn = np.float32(math.log(nparticles))
    sb = bridge_of(transition_sampler, likelihood_logpdf) if set(kwargs) == {"mask_"} else None
    for k in range(nsteps):                                                         # scan_body :138-152
        key_proposal, key_resampling = ops.split(keys[k], 2)
        v, v_prev, t_prev = vs_bridge[k + 1], vs_bridge[k], ts[k]
        if sb is not None:                                                          # :144-150, one network evaluation
            cell = {}

            def resample(lw):
                w, cell["c"] = ops.normalise(lw, log_space=False, return_lse=True)
                return resampling(w, key_resampling)

            us, _, _ = sb.fused_weight_then_propose(us, v, v_prev, t_prev, key_proposal, kwargs["mask_"], resample)
            log_ell = (log_ell - logn) + cell["c"]
            continue
        log_ws = likelihood_logpdf(v, us, v_prev, t_prev, **kwargs)                 # :144
        w, c = ops.normalise(log_ws, log_space=False, return_lse=True)              # :145,147,148
        log_ell = (log_ell - logn) + c                                              # :146
        inds = resampling(w, key_resampling)
        us_prev = ops.take_rows(us, inds)                                           # :149
        us = transition_sampler(us_prev, v_prev, t_prev, key_proposal, **kwargs)    # :150
    return us, log_ell


def pcn_proposal(key, delta: float, x, mean, sampler):
    """The pCN proposal (smc.py:161-168)."""
    beta = 2 / (2 + delta)
    key_rnds = ops.split(key, 2)
    rnds0, rnds1 = sampler(key_rnds[0]), sampler(key_rnds[1])
    p = x + math.sqrt(delta / 2) * (rnds0 - mean)
    return beta * p + (1 - beta) * mean + math.sqrt(1 - beta) * (rnds1 - mean)


def pmcmc_kernel(key, uT, log_ell, ys, y0, ts, fwd_ys_sampler, sde, ref_sampler, transition_sampler,
                 likelihood_logpdf, resampling, nparticles, delta: float = None, which_u: int = 0, **kwargs):
    """Particle-marginal MH kernel targeting p(uT | vT = y0) (smc.py:171-258).

    Returns (uT, log_ell, ys, MCMCState)."""
    key_prop, key_u0, key_filter, key_mh = ops.split(key, 4)                        # :231
    if delta is None:
        prop_ys = fwd_ys_sampler(key_prop, y0)                                      # :234
    else:
        ts_np = np.asarray(ts.detach().cpu() if isinstance(ts, torch.Tensor) else ts, np.float64).reshape(-1)
        y0_t = y0 if isinstance(y0, torch.Tensor) else torch.as_tensor(np.asarray(y0, np.float32), device=ys.device)
        coef = np.asarray(sde.mean(ts_np, ts_np[0], 1.0), np.float32)              # mean is linear in y0
        mean = torch.as_tensor(coef, device=ys.device).reshape((-1,) + (1,) * y0_t.dim()) * y0_t  # :236
        mean = mean.reshape(ys.shape)
        prop_ys = pcn_proposal(key_prop, delta, ys, mean, lambda key_: fwd_ys_sampler(key_, y0))  # :237
    vs = torch.flip(prop_ys, [0])                                                   # :239
    u0s = ref_sampler(key_u0, vs[0], nparticles)                                    # :241
    prop_uTs, prop_log_ell = pmcmc_filter_step(key_filter, vs, u0s, ts, transition_sampler, likelihood_logpdf,
                                               resampling, nparticles, **kwargs)    # :242
    prop_uT = prop_uTs[which_u]
    log_ell_t = log_ell if isinstance(log_ell, torch.Tensor) else torch.as_tensor(np.float32(log_ell),
                                                                                  device=prop_log_ell.device)
    log_acc_prob = torch.minimum(torch.zeros_like(prop_log_ell), prop_log_ell - log_ell_t)  # :246
    z = ops.uniform(key_mh, (), device=prop_log_ell.device)                         # :248
    acc_flag = ops.math_map("log", z.reshape(1)).reshape(()) < log_acc_prob        # :249
    state = MCMCState(acceptance_prob=torch.exp(log_acc_prob), is_accepted=acc_flag, prop_log_ell=prop_log_ell,
                      log_ell=log_ell_t)
    if bool(acc_flag.item()):                                                       # :255-258
        return prop_uT, prop_log_ell, prop_ys, state
    return uT, log_ell_t, ys, state


def _fused_pmcmc(fwd_ys_sampler, sde, ref_sampler, transition_sampler, likelihood_logpdf, resampling, ts, nparticles, delta):
    """(model, resampling name) when the fused pMCMC engine applies: all four closures belong to one
    LinearGaussianBridge on its own grid, its forward transition is exact, and the resampler is one the fused filter has."""
    fused = _fused_filter(transition_sampler, likelihood_logpdf, resampling, {}, nparticles)
    if fused is None:
        return None
    model = fused[0]
    for closure, role in ((fwd_ys_sampler, "fwd_ys_sampler"), (ref_sampler, "ref_sampler"),
                          (transition_sampler, "transition_sampler")):
        if getattr(closure, "_fbsmi_lg", None) is not model or getattr(closure, "_role", "") != role:
            return None
    if not model.fused_pmcmc_supported(nparticles) or not model.same_grid(ts):
        return None
    if delta is not None and sde is not model.sde:       # the pCN mean path is tabulated from the bridge's own SDE
        return None
    return fused


def pmcmc_chain(key, uTs, log_ells, yss, y0, ts, fwd_ys_sampler, sde, ref_sampler, transition_sampler, likelihood_logpdf,
                resampling, nparticles, nsamples, delta: float = None):
    """The pMCMC loop of experiments/toy/gp_pmcmc.py:170-179 for C = uTs.shape[0] chains: per iteration
    ``key, subkey = split(key)`` and chain c runs pmcmc_kernel with split(subkey, C)[c].

    uTs (C, du), log_ells (C,), yss (C, T+1, dv), y0 (dv,).  Returns (key, uTs, log_ells, yss, samples, states) with
    samples (nsamples, C, du) and states an MCMCState of (nsamples, C) tensors.  With the closures of one
    LinearGaussianBridge and stratified / systematic resampling the whole loop runs on the device (LGPmcmc.chain);
    otherwise pmcmc_kernel is called per chain and iteration with the same keys."""
    nchains, nsamples = int(uTs.shape[0]), int(nsamples)
    fused = _fused_pmcmc(fwd_ys_sampler, sde, ref_sampler, transition_sampler, likelihood_logpdf, resampling, ts,
                         nparticles, delta)
    if fused is not None:
        model, rname = fused
        h = model.pmcmc_handle(nparticles, rname, nchains, delta)
        out = h.chain(key, uTs, log_ells, yss, y0, nsamples)
        if nchains > 1:
            return out
        key, uT, ell, ys, samples, st = out                # (the handle squeezes a single chain's axis)
        return (key, uT[None], ell[None], ys[None], samples[:, None], MCMCState(*(f[:, None] for f in st)))
    dev = uTs.device
    state = [(uTs[c], log_ells[c], yss[c]) for c in range(nchains)]
    samples = torch.empty((nsamples, nchains) + tuple(uTs.shape[1:]), dtype=torch.float32, device=dev)
    fields = [[] for _ in MCMCState._fields]
    for i in range(nsamples):
        key, subkey = ops.split(key)
        row = [[] for _ in MCMCState._fields]
        for c, kc in enumerate(ops.split(subkey, nchains)):
            uT, log_ell, ys, st = pmcmc_kernel(kc, *state[c], y0, ts, fwd_ys_sampler, sde, ref_sampler, transition_sampler,
                                               likelihood_logpdf, resampling, nparticles, delta=delta)
            state[c] = (uT, log_ell, ys)
            samples[i, c] = uT
            for r, f in zip(row, st):
                r.append(f.reshape(()))
        for fl, r in zip(fields, row):
            fl.append(torch.stack(r))
    states = MCMCState(*(torch.stack(fl) if fl else torch.empty((0, nchains), device=dev) for fl in fields))
    return (key, torch.stack([s[0] for s in state]), torch.stack([torch.as_tensor(s[1], device=dev).reshape(()) for s in state]),
            torch.stack([s[2] for s in state]), samples, states)


def twisted_smc(key, y, ts, init_sampler, transition_logpdf, twisting_logpdf, twisting_prop_sampler,
                twisting_prop_logpdf, resampling, nparticles, **kwargs):
    """Twisted SMC baseline (smc.py:261-309; Algorithm 1 of arXiv 2306.17775).  With the five closures of one
    GaussianTwisted on its own grid and y, and stratified / systematic resampling, the whole run is one fused launch
    sequence on the device (TwistedHandle.run); otherwise the host loop below."""
    fused = fused_twisted(y, ts, init_sampler, transition_logpdf, twisting_logpdf, twisting_prop_sampler,
                          twisting_prop_logpdf, resampling, nparticles, kwargs)
    if fused is not None:
        xs, log_ws = fused[0].handle(nparticles, fused[1]).run(key)
        return xs[0], log_ws[0]
    nsteps = (ts.shape[0] if hasattr(ts, "shape") else len(ts)) - 1
    key_init, key_filter = ops.split(key, 2)
    keys = ops.split(key_filter, nsteps)
    xs = init_sampler(key_init, nparticles)
    log_ps = twisting_logpdf(y, xs, ts[0], **kwargs)
    log_ws = ops.normalise(log_ps, log_space=True)
    for k in range(nsteps):
        key_resampling, key_prop = ops.split(keys[k], 2)
        t_prev = ts[k + 1]  # the reference scans over ts[1:] (:306-307)
        inds = resampling(ops.math_map("exp", log_ws), key_resampling)
        xs_prev = ops.take_rows(xs, inds)
        log_ps_prev = log_ps[inds.long()]
        xs = twisting_prop_sampler(key_prop, xs_prev, t_prev, y, **kwargs)
        log_ps = twisting_logpdf(y, xs, t_prev, **kwargs)
        log_ws = (transition_logpdf(xs, xs_prev, t_prev) + log_ps
                  - twisting_prop_logpdf(xs, xs_prev, t_prev, y, **kwargs) - log_ps_prev)
        log_ws = ops.normalise(log_ws, log_space=True)
    return xs, log_ws
