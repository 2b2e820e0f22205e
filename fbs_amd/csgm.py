"""Conditional score-based generative sampling for image restoration (Song et al., 2021): the `csgm` baseline of the
reference's image tables.

Counterpart of experiments/imgs/inpainting_csgm.py:88-124 and supr_csgm.py (they differ by the mask only): ONE trajectory of
the reverse SDE of the unobserved pixels, the observed pixels replaced at every step by a fresh noising of y0 to the current
time.  No particles, no resampling: per step one draw of the observed part, one network evaluation and one Euler-Maruyama
update whose noise is the step's slice of normal(key_scan, (nsteps, *x_shape)), drawn inside the kernel (fbsmi_em_update).

``make_image_csgm_batched`` runs B such trajectories in lockstep: per step one fbsmi_em_csgm_step_batched launch (the update
and the next network input of every trajectory, both draws inside the kernel) and one network call on B rows.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, ops
from .sdes import make_linear_sde


def make_image_csgm(score_fn, ds, sde, ts):
    """score_fn(uv (1, w, h, c), t) -> score of the same shape.  -> conditional_sampler(key, y0, mask_) -> x0 (p, c)."""
    ts = np.asarray(ts, np.float64)
    T = float(ts[-1])
    nsteps = ts.size - 1
    dt = T / nsteps                                                                   # inpainting_csgm.py:49
    discretise = make_linear_sde(sde)[0]
    x_shape = tuple(ds.unobs_shape)

    def reverse_drift(u, t, mask_, key_, y0):                                         # :88-92
        s_ = T - float(t)
        F, Q = (float(x) for x in discretise(s_, float(ts[0])))
        v_hat = F * y0 + math.sqrt(Q) * ops.normal(key_, tuple(y0.shape), device=y0.device)
        uv = ds.concat(u, v_hat, mask_)
        score_u = ds.unpack(score_fn(uv.unsqueeze(0), s_).reshape(uv.shape).float(), mask_)[0]
        return -sde.drift(u, s_) + float(sde.dispersion(s_)) ** 2 * score_u

    def euler_maruyama(key_, u0, mask_, y0):                                          # :103-113
        key_scan, key_est = ops.split(key_)
        key_ests = ops.split(key_est, nsteps)
        k0, k1 = (int(x) for x in key_scan)
        numel = int(u0.numel())
        u = u0.contiguous()
        for k in range(nsteps):
            t = float(ts[k])
            f = reverse_drift(u, t, mask_, key_ests[k], y0).to(torch.float32).contiguous()
            c = float(np.float32(float(sde.dispersion(T - t)) * math.sqrt(dt)))
            out = torch.empty_like(u)
            _lib.call("fbsmi_em_update", u.data_ptr(), f.data_ptr(), float(np.float32(dt)), c, k0, k1, nsteps * numel,
                      k * numel, numel, out.data_ptr(), ops._stream())
            u = out
        return u

    def conditional_sampler(key_, y0, mask_):                                         # :116-121
        key_init, key_sde = ops.split(key_, 2)
        u0 = ops.normal(key_init, x_shape, device=y0.device)                          # cond_ref_sampler :99-100
        return euler_maruyama(key_sde, u0, mask_, y0)

    return conditional_sampler


def csgm_key_schedule(keys, nsteps: int) -> dict:
    """Every key ``conditional_sampler`` derives from its own, for B trajectories, on the host: (init, sde) = split(key),
    (scan, est) = split(sde), split(est, nsteps).  -> (B, 2) arrays 'init', 'scan' and the (nsteps, B, 2) array 'est',
    all uint32."""
    keys = np.asarray(keys, np.uint32).reshape(-1, 2)
    B, T = keys.shape[0], int(nsteps)
    out = {"init": np.zeros((B, 2), np.uint32), "scan": np.zeros((B, 2), np.uint32), "est": np.zeros((T, B, 2), np.uint32)}
    for b in range(B):
        out["init"][b], key_sde = ops.split(keys[b], 2)
        out["scan"][b], key_est = ops.split(key_sde)
        out["est"][:, b] = ops.split(key_est, T)
    return out


def make_image_csgm_batched(score_fn, ds, sde, ts, chunk: int = 4096, net_input_dtype=torch.float32):
    """score_fn(uv (rows, w, h, c), t) -> score of the same shape, float32 or bfloat16.
    -> conditional_sampler_batched(keys (B, 2), y0s, masks) -> x0 (B, p, c): B trajectories of ``make_image_csgm`` in
    lockstep.  y0s: a list of B observations (q, c) or their stack (one (q, c) tensor: shared); masks: one mask or a list
    of B masks.  Per step ONE fbsmi_em_csgm_step_batched launch (the update of step k and the network input of step k + 1
    for every trajectory) and ceil(B / chunk) network calls on the flat (B, w, h, c) buffer; nothing per trajectory and no
    host synchronisation inside the time loop.

    The result equals the stacked results of

        [make_image_csgm(score_fn, ds, sde, ts)(keys[b], y0s[b], masks[b]) for b in range(B)]

    bit for bit whenever the score function's output row does not depend on which other rows share its call and
    net_input_dtype is float32.  That is not promised for a real UNet: library convolution and matrix kernels may be
    chosen by batch size and differ in the last bits; the two runs are then two valid draws.  Masks of different (du, dv)
    run that loop: the same result without the speed-up."""
    from .score import _NET_DT, ScoreBridge
    ts = np.asarray(ts, np.float64)
    T = float(ts[-1])
    nsteps = ts.size - 1
    dt = T / nsteps
    discretise = make_linear_sde(sde)[0]
    x_shape = tuple(ds.unobs_shape)
    single = make_image_csgm(score_fn, ds, sde, ts)
    sb = ScoreBridge(score_fn, ds, sde, ts, chunk=chunk, net_input_dtype=net_input_dtype)   # mask tables and buffers, cached
    chunk = int(chunk)
    # per-step float32 tables from float64: the forward time of step k, the re-noising of y0 to it, the reverse drift's
    # coefficients (ScoreBridge._coef) and the noise scale of fbsmi_em_update
    s_fwd = [T - float(ts[k]) for k in range(nsteps)]
    FQ = [tuple(float(x) for x in discretise(s_, float(ts[0]))) for s_ in s_fwd]
    tab = {"F": np.array([F for F, _ in FQ], np.float32), "sq": np.array([math.sqrt(Q) for _, Q in FQ], np.float32),
           "cx": np.array([-float(sde.drift(1.0, s_)) for s_ in s_fwd], np.float32),
           "cs": np.array([float(sde.dispersion(s_)) ** 2 for s_ in s_fwd], np.float32),
           "c": np.array([float(sde.dispersion(s_)) * math.sqrt(dt) for s_ in s_fwd], np.float32)}
    dt32 = float(np.float32(dt))

    @torch.no_grad()
    def conditional_sampler_batched(keys, y0s, masks):
        keys = np.asarray(keys.detach().cpu() if isinstance(keys, torch.Tensor) else keys, np.uint32).reshape(-1, 2)
        B = keys.shape[0]
        per_mask = not hasattr(masks, "unobs_inds_ravelled")
        if per_mask and len(masks) != B:
            raise ValueError(f"{len(masks)} masks for {B} trajectories")
        shared_y = isinstance(y0s, torch.Tensor) and y0s.dim() == len(x_shape)
        if not shared_y and len(y0s) != B:
            raise ValueError(f"{len(y0s)} observations for {B} trajectories")
        y0 = lambda b: y0s if shared_y else y0s[b]
        mask = lambda b: masks[b] if per_mask else masks
        ems = [sb._em_mask(mask(b)) for b in range(B if per_mask else 1)]
        if any((e.du, e.dv) != (ems[0].du, ems[0].dv) for e in ems):
            return torch.stack([single(keys[b], y0(b), mask(b)) for b in range(B)], 0)
        mb = sb.em_mask_batch(list(masks) if per_mask else [masks], B)
        du, dv, D = mb.du, mb.dv, mb.D
        dev = ds.device
        ks = csgm_key_schedule(keys, nsteps)                                          # uploaded once
        k_init, k_scan, k_est = (ops.keys_to_device(ks[n], dev) for n in ("init", "scan", "est"))
        y = torch.stack([ops._f32c(y0(b), "y0").reshape(-1) for b in range(B)], 0).contiguous()
        if y.shape[1] != dv:
            raise ValueError(f"y0 holds {y.shape[1]} floats, the masks' observed part {dv}")
        w, h, c = ds.image_shape
        img = sb._buffer("img", (B, w, h, c), net_input_dtype, dev)
        u = torch.empty((B, du), dtype=torch.float32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None

        def step(net, k_upd, k_cat):
            """The update of step k_upd (net given) and the network input of step k_cat (None: the last step)."""
            i, j = (0 if k_upd is None else k_upd), (nsteps - 1 if k_cat is None else k_cat)
            _lib.call("fbsmi_em_csgm_step_batched", mb.ref, u.data_ptr(), ptr(net), 0 if net is None else _NET_DT[net.dtype],
                      float(tab["cx"][i]), float(tab["cs"][i]), dt32, float(tab["c"][i]), k_scan.data_ptr(), nsteps * du,
                      i * du, ptr(y), float(tab["F"][j]), float(tab["sq"][j]), k_est[j].data_ptr(),
                      _NET_DT[net_input_dtype], None if k_cat is None else img.data_ptr(), B, u.data_ptr(), ops._stream())

        _lib.call("fbsmi_normal_batched", k_init.data_ptr(), B, du, u.data_ptr(), ops._stream())   # cond_ref_sampler
        if nsteps:
            step(None, None, 0)
        for k in range(nsteps):
            net = None
            for s in range(0, B, chunk):
                out = score_fn(img[s:s + chunk], s_fwd[k])
                if net is None:
                    if out.dtype not in _NET_DT:
                        out = out.float()
                    net = sb._buffer("net", (B, D), out.dtype, dev)
                net[s:s + chunk] = out.reshape(-1, D)
            step(net, k, k + 1 if k + 1 < nsteps else None)
        return u.reshape((B,) + x_shape)

    return conditional_sampler_batched
