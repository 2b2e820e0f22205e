"""Model closures around a score / drift network for the image tasks (experiments/imgs/inpainting.py:98-161,
supr.py identical up to the mask; experiments/sb_imgs/supr.py:80-141 for the Schrodinger-bridge model).

Per SMC step the reference evaluates the network twice on the same input (inside ``transition_sampler``
and inside ``likelihood_logpdf``: csmc.py:142,145) and spreads concat / unpack / drift / Euler-Maruyama /
norm.logpdf / sum over a dozen array passes.  Here a step is

    fbsmi_em_concat  (ancestor gather + concat -> the network input, written once)
    the network      (PyTorch-ROCm, in chunks of `chunk` particles)
    fbsmi_em_finish  (unpack + drift + proposal with in-kernel normal draw + pin + row-summed log-density)

``ScoreBridge.fused_step`` is that sequence; ``fbs_amd.samplers`` calls it when it is handed this bridge's
closures.  The three closures themselves keep the reference's signatures and run on the same kernels
(the network output of a given (us_prev, v_prev, t_prev, mask) is computed once and shared).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib, ops

_NET_DT = {torch.float32: 0, torch.bfloat16: 1}


class EMMask:
    """Device tables of a mask for the fused kernels (include/fbsmi.h, fbsmi_em_mask)."""

    def __init__(self, mask, channels: int, device):
        c = int(channels)
        unobs = mask.unobs_inds_ravelled.detach().cpu().numpy().astype(np.int64)
        obs = mask.obs_inds_ravelled.detach().cpu().numpy().astype(np.int64)
        u_off = (unobs[:, None] * c + np.arange(c)[None, :]).reshape(-1)
        v_off = (obs[:, None] * c + np.arange(c)[None, :]).reshape(-1)
        D = u_off.size + v_off.size
        role = np.full(D, np.iinfo(np.int64).min, np.int64)
        role[u_off] = np.arange(u_off.size)
        role[v_off] = ~np.arange(v_off.size)
        if (role == np.iinfo(np.int64).min).any():
            raise ValueError("the mask does not cover every pixel exactly once")
        self.mask = mask                                   # keeps the key object alive
        self.du, self.dv, self.D = int(u_off.size), int(v_off.size), int(D)
        dev = lambda a: torch.from_numpy(a.astype(np.int32)).to(device)
        self.u_off, self.v_off, self.role = dev(u_off), dev(v_off), dev(role)
        self.struct = _lib.EMMaskStruct(self.du, self.dv, self.u_off.data_ptr(), self.v_off.data_ptr(),
                                        self.role.data_ptr())

    @property
    def ref(self):
        return C.byref(self.struct)


class EMMaskBatch:
    """The masks of B ensembles that advance in lockstep (include/fbsmi.h, fbsmi_em_mask_batch): the tables of one mask
    shared by all, or of B masks of one shape (same du and dv) stacked."""

    def __init__(self, ems):
        ems = list(ems)
        if not ems or any((m.du, m.dv) != (ems[0].du, ems[0].dv) for m in ems):
            raise ValueError("the masks of one batch must have the same du and dv")
        self.ems = ems                                     # keeps the tables' owners (and their key objects) alive
        self.nmasks, self.du, self.dv, self.D = len(ems), ems[0].du, ems[0].dv, ems[0].D
        stack = lambda name: torch.stack([getattr(m, name) for m in ems], 0).contiguous()
        self.u_off, self.v_off, self.role = stack("u_off"), stack("v_off"), stack("role")
        self.struct = _lib.EMMaskBatchStruct(self.du, self.dv, self.nmasks, self.u_off.data_ptr(), self.v_off.data_ptr(),
                                             self.role.data_ptr())

    @property
    def ref(self):
        return C.byref(self.struct)


class ScoreBridge:
    def __init__(self, score_fn, dataset, sde, ts, chunk: int = 1024, mode: str = "score",
                 net_input_dtype=torch.float32, fwd_drift_fn=None, fwd_drift_rows_fn=None):
        """score_fn(x (B, w, h, c), t float) -> (B, w, h, c), float32 or bfloat16.

        mode 'score': score_fn is the trained score at forward time t and the reverse drift is
        -sde.drift + dispersion^2 * score (inpainting.py:102-103); mode 'drift': score_fn is the learned
        backward drift itself (sb_imgs/supr.py:84-85) and ``fwd_drift_fn(x, t)`` the learned forward drift
        that ``fwd_sampler`` integrates (supr.py:132-137).  net_input_dtype: dtype the network input is
        written in (torch.bfloat16 saves the cast pass of an autocast network).
        ``fwd_drift_rows_fn(x (rows, w, h, c) float32, t) -> (rows, w, h, c)``, float32 or bfloat16: the same forward drift
        on a batch of images, one per row; with it ``fwd_sampler_batched`` integrates the paths of B ensembles in
        lockstep."""
        if mode not in ("score", "drift"):
            raise ValueError(f"unknown mode {mode}")
        self.score_fn, self.dataset, self.sde = score_fn, dataset, sde
        self.mode, self.fwd_drift_fn, self.fwd_drift_rows_fn = mode, fwd_drift_fn, fwd_drift_rows_fn
        self.ts = np.asarray(ts, np.float64)
        self.T = float(self.ts[-1])
        self.nsteps = self.ts.size - 1
        self.dt = self.T / self.nsteps                       # inpainting.py:58-59
        self.chunk = int(chunk)
        self.net_input_dtype = net_input_dtype
        self._cache = None
        self._masks = {}
        self._mask_batches = {}
        self._buf = {}
        self.profile = None                                  # set to a dict to collect torch events per phase
        self.capture = None                                  # set to a dict: operands and results of the LAST fused step

    # -- plumbing -----------------------------------------------------------------------------------
    def _em_mask(self, mask_) -> EMMask:
        m = self._masks.get(id(mask_))
        if m is None or m.mask is not mask_:
            m = EMMask(mask_, self.dataset.image_shape[2], self.dataset.device)
            self._masks[id(mask_)] = m
        return m

    def _buffer(self, name, shape, dtype, device):
        b = self._buf.get(name)
        if b is None or b.shape != tuple(shape) or b.dtype != dtype or b.device != device:
            b = torch.empty(tuple(shape), dtype=dtype, device=device)
            self._buf[name] = b
        return b

    def _coef(self, t_prev):
        """(mode, cx, cs, sd) of the step that leaves reverse time t_prev."""
        tf = self.T - float(t_prev)
        sd = math.sqrt(self.dt) * float(self.sde.dispersion(tf))
        if self.mode == "drift":
            return 1, 0.0, 1.0, sd
        return 0, -float(self.sde.drift(1.0, tf)), float(self.sde.dispersion(tf)) ** 2, sd

    def _mark(self, name):
        if self.profile is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.profile.setdefault(name, []).append(e)
        return e

    @torch.no_grad()
    def _network(self, us, A, v_prev, t_prev, em: EMMask) -> torch.Tensor:
        """nn(concat(us[A], v_prev), T - t) for every row -> (n, D), the network's own output dtype."""
        us = ops._f32c(us, "us")
        n = int(A.numel()) if A is not None else int(us.shape[0])
        w, h, c = self.dataset.image_shape
        img = self._buffer("img", (n, w, h, c), self.net_input_dtype, us.device)
        vp = ops._f32c(v_prev, "v_prev")
        self._mark("concat0")
        _lib.call("fbsmi_em_concat", em.ref, us.data_ptr(), A.data_ptr() if A is not None else None, vp.data_ptr(), n,
                  _NET_DT[self.net_input_dtype], img.data_ptr(), ops._stream())
        self._mark("concat1")
        tf = self.T - float(t_prev)
        out = None
        # Fixed chunks of `chunk` rows plus a tail (explicit_final's row N + 1 is a call of its own when chunk divides N):
        # one call of N + 1 rows is 8 % faster per step once MIOpen has built kernels for that batch size, but on a fresh
        # machine every unusual batch size costs tens of seconds of kernel builds (measured: +50 s / +120 s for a sweep of
        # configs 3 / 5) -- callers that run many sweeps pass chunk >= N + 1.
        per = self.chunk
        for s in range(0, n, per):
            y = self.score_fn(img[s:s + per], tf)
            if out is None:
                if y.dtype not in _NET_DT:
                    y = y.float()
                out = self._buffer("net", (n, em.D), y.dtype, us.device)
            out[s:s + per] = y.reshape(-1, em.D)
        self._mark("net1")
        return out

    def _finish(self, em, us, A, net, t_prev, v, v_prev, key_, row_slice, pin, want_us, want_lw, net_A=None):
        mode, cx, cs, sd = self._coef(t_prev)
        n = int(net_A.numel() if net_A is not None else net.shape[0])
        row0, cnt, tot = (0, n, n) if row_slice is None else (int(row_slice[0]), int(row_slice[1]), int(row_slice[2]))
        if cnt != n:
            raise ValueError(f"row_slice says {cnt} local rows, the ensemble shard has {n}")
        us_new = torch.empty((n, em.du), dtype=torch.float32, device=net.device) if want_us else None
        lw = torch.empty(n, dtype=torch.float32, device=net.device) if want_lw else None
        k0, k1 = ops._k(key_) if want_us else (0, 0)
        pin_row, pin_val = (-1, None) if pin is None else (int(pin[0]), ops._f32c(pin[1], "pin value"))
        vv = ops._f32c(v, "v") if want_lw else None
        vp = ops._f32c(v_prev, "v_prev") if want_lw else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        self._mark("finish0")
        _lib.call("fbsmi_em_finish", em.ref, ptr(us), ptr(A), net.data_ptr(), ptr(net_A), _NET_DT[net.dtype], mode, cx, cs,
                  self.dt, sd, ptr(vv), ptr(vp), k0, k1, tot, row0, n, pin_row, ptr(pin_val), ptr(us_new), ptr(lw),
                  ops._stream())
        self._mark("finish1")
        return us_new, lw

    # -- the fused step -------------------------------------------------------------------------------
    def fused_step(self, us, A, v, v_prev, t_prev, key_, mask_, pin=None, row_slice=None, want_lw=True):
        """One SMC step of csmc.forward_pass (csmc.py:140-145) / smc.py:63-65 around one network evaluation:
        us_prev = us[A] (A None: identity), proposal, pin = (local row, value) or None, log-weights of
        the gathered particles.  -> (us_new (n, p, c), lw (n,))."""
        em = self._em_mask(mask_)
        self._cache = None                                   # the shared network buffer is about to be rewritten
        us2 = ops._f32c(us, "us").reshape(us.shape[0], -1)
        A32 = A.to(torch.int32).contiguous() if A is not None else None
        net = self._network(us2, A32, v_prev, t_prev, em)
        us_new, lw = self._finish(em, us2, A32, net, t_prev, v, v_prev, key_, row_slice, pin, True, want_lw)
        if self.capture is not None:                         # parity tests replay this step through the oracle
            self.capture.update(us=us2, A=A32, net=net, img=self._buf["img"], v=v, v_prev=v_prev, t_prev=float(t_prev),
                                key=np.asarray(key_, np.uint32).copy(), pin=pin, row_slice=row_slice, us_new=us_new,
                                lw=lw, coef=self._coef(t_prev), em=em)
        return us_new.reshape((us_new.shape[0],) + tuple(self.dataset.unobs_shape)), lw

    # -- the fused step for B ensembles in lockstep ---------------------------------------------------
    def em_mask_batch(self, masks, B: int) -> EMMaskBatch:
        """The stacked tables of one mask (shared) or a list of B masks of one shape; built once per set of masks."""
        if isinstance(masks, EMMaskBatch):
            mb = masks
        else:
            lst = [masks] if hasattr(masks, "unobs_inds_ravelled") else list(masks)
            if len(lst) > 1 and all(m is lst[0] for m in lst):
                lst = lst[:1]
            key = tuple(id(m) for m in lst)
            mb = self._mask_batches.get(key)
            if mb is None or any(e.mask is not m for e, m in zip(mb.ems, lst)):
                mb = EMMaskBatch([self._em_mask(m) for m in lst])
                self._mask_batches[key] = mb
        if mb.nmasks not in (1, int(B)):
            raise ValueError(f"{mb.nmasks} masks for {B} ensembles: pass one mask or one per ensemble")
        return mb

    @torch.no_grad()
    def _network_batched(self, us3, A32, vp, t_prev, mb: EMMaskBatch) -> torch.Tensor:
        """nn(concat(us[b][A[b]], v_prev[b]), T - t) for every row of every ensemble -> (B * n, D) in the network's own
        output dtype: one fbsmi_em_concat_batched launch, then the network in `chunk`-row pieces over the flat B * n rows
        (a chunk may straddle ensembles).  us3 (B, n, du) float32 contiguous, A32 (B, n) int32 or None, vp (B, dv).  The
        result is the bridge's shared 'net' buffer: the next network evaluation overwrites it."""
        B, n = int(us3.shape[0]), int(us3.shape[1])
        self._cache = None                                   # the shared network buffer is about to be rewritten
        dev = us3.device
        w, h, c = self.dataset.image_shape
        img = self._buffer("img", (B * n, w, h, c), self.net_input_dtype, dev)
        _lib.call("fbsmi_em_concat_batched", mb.ref, us3.data_ptr(), A32.data_ptr() if A32 is not None else None,
                  vp.data_ptr(), B, n, _NET_DT[self.net_input_dtype], img.data_ptr(), ops._stream())
        tf = self.T - float(t_prev)
        net = None
        for s in range(0, B * n, self.chunk):
            y = self.score_fn(img[s:s + self.chunk], tf)
            if net is None:
                if y.dtype not in _NET_DT:
                    y = y.float()
                net = self._buffer("net", (B * n, mb.D), y.dtype, dev)
            net[s:s + self.chunk] = y.reshape(-1, mb.D)
        return net

    @staticmethod
    def _ensemble_blocks(x, B: int, name: str):
        """x (B, ...) float32 on the device -> (tensor, stride in floats between its ensembles): read in place when every
        x[b] is contiguous and the ensembles are a fixed non-negative stride apart, copied otherwise."""
        ops._require_cuda(x, name)
        if x.dtype != torch.float32 or not x[0].is_contiguous() or (B > 1 and x.stride(0) < x[0].numel()):
            x = ops._f32c(x, name)
        return x, (int(x.stride(0)) if B > 1 else int(x[0].numel()))

    @torch.no_grad()
    def transition_logpdf_batched(self, u, us, v_prev, t_prev, masks, net=None):
        """``transition_logpdf`` for B ensembles at the same time step: u (B, p, c) the targets, us (B, n, p, c) the
        particles, v_prev (B, q, c); masks one mask, a list of B masks of one shape, or an EMMaskBatch.  -> lw (B, n) with
        lw[b] = transition_logpdf(u[b], us[b], v_prev[b], t_prev, masks[b]) bit for bit whenever the network's output row
        does not depend on which rows share its call.  One fbsmi_em_translp_batched launch; u and us may be time slices
        of stored (B, T + 1, ...) arrays and are then read in place.  Without ``net`` the network runs on
        concat(us, v_prev) as in ``fused_step_batched``; with ``net`` (B * n, D), its output on that input kept from an
        earlier call, there is no network call and v_prev is not read."""
        B, n = int(us.shape[0]), int(us.shape[1])
        mb = self.em_mask_batch(masks, B)
        us_b, us_stride = self._ensemble_blocks(us, B, "us")
        u_b, u_stride = self._ensemble_blocks(u, B, "u")
        if us_b[0].numel() != n * mb.du or u_b[0].numel() != mb.du:
            raise ValueError(f"us rows and u must hold the masks' unobserved part, {mb.du} floats")
        if net is None:
            net = self._network_batched(ops._f32c(us_b, "us").reshape(B, n, -1), None,
                                        ops._f32c(v_prev, "v_prev").reshape(B, -1), t_prev, mb)
        elif net.dtype not in _NET_DT or not net.is_contiguous() or net.numel() != B * n * mb.D or net.device != us_b.device:
            raise ValueError("net must be a contiguous float32 or bfloat16 (B * n, D) tensor on the particles' device")
        mode, cx, cs, sd = self._coef(t_prev)
        lw = torch.empty((B, n), dtype=torch.float32, device=us_b.device)
        _lib.call("fbsmi_em_translp_batched", mb.ref, us_b.data_ptr(), us_stride, net.data_ptr(), _NET_DT[net.dtype], mode,
                  cx, cs, self.dt, sd, u_b.data_ptr(), u_stride, B, n, lw.data_ptr(), ops._stream())
        return lw

    @torch.no_grad()
    def fused_step_batched(self, us, A, v, v_prev, t_prev, keys, masks, pins=None, want_us=True, out_us=None):
        """``fused_step`` for B ensembles at the same time step: one fbsmi_em_concat_batched launch, the network in
        `chunk`-row pieces over the flat B * n rows (a chunk may straddle ensembles), one fbsmi_em_finish_batched launch.
        us (B, n, p, c); A (B, n) ancestors local to each ensemble, or None; v, v_prev (B, q, c); keys (B, 2) (host uint32,
        or their bits on the device: ensemble b draws normal(keys[b], (n, p, c)) as a call of its own would); masks one
        mask, a list of B masks of one shape, or an EMMaskBatch; pins = (rows (B,) int32 with -1 for none, values
        (B, p, c)) or None.  want_us=False: weights only (keys and pins are not read).  out_us: a contiguous float32
        device tensor of B * n * p * c elements that receives us_new (a slot of a stored particle array; not `us` itself).
        -> (us_new (B, n, p, c) or None, lw (B, n)); ensemble b has the bits of its own ``fused_step`` whenever the
        network's output row does not depend on which rows share its call."""
        us3 = ops._f32c(us, "us")
        B, n = int(us3.shape[0]), int(us3.shape[1])
        us3 = us3.reshape(B, n, -1)
        mb = self.em_mask_batch(masks, B)
        if us3.shape[2] != mb.du:
            raise ValueError(f"us rows hold {us3.shape[2]} floats, the masks' unobserved part {mb.du}")
        dev = us3.device
        A32 = A.to(torch.int32).contiguous() if A is not None else None
        vv, vp = ops._f32c(v, "v").reshape(B, -1), ops._f32c(v_prev, "v_prev").reshape(B, -1)
        ptr = lambda t: t.data_ptr() if t is not None else None
        net = self._network_batched(us3, A32, vp, t_prev, mb)
        mode, cx, cs, sd = self._coef(t_prev)
        us_new = None
        if want_us and out_us is not None:
            if out_us.dtype != torch.float32 or out_us.device != dev or not out_us.is_contiguous() or \
                    out_us.numel() != B * n * mb.du:
                raise ValueError("out_us must be a contiguous float32 tensor of B * n * du elements on the particles' device")
            us_new = out_us.view(B, n, mb.du)
        elif want_us:
            us_new = torch.empty((B, n, mb.du), dtype=torch.float32, device=dev)
        lw = torch.empty((B, n), dtype=torch.float32, device=dev)
        kd = ops.keys_to_device(keys, dev) if want_us else None
        pin_row = pin_val = None
        if want_us and pins is not None:
            pin_row = torch.as_tensor(pins[0], device=dev).to(torch.int32).contiguous()
            pin_val = ops._f32c(pins[1], "pin values").reshape(B, -1)
            if pin_row.numel() != B or pin_val.shape[1] != mb.du:
                raise ValueError("pins must be (rows (B,), values (B, p, c))")
        if want_us and kd.numel() != 2 * B:
            raise ValueError("keys must be (B, 2)")
        _lib.call("fbsmi_em_finish_batched", mb.ref, us3.data_ptr(), ptr(A32), net.data_ptr(), _NET_DT[net.dtype], mode,
                  cx, cs, self.dt, sd, vv.data_ptr(), vp.data_ptr(), ptr(kd), B, n, ptr(pin_row), ptr(pin_val),
                  ptr(us_new), lw.data_ptr(), ops._stream())
        if us_new is not None:
            us_new = us_new.reshape((B, n) + tuple(self.dataset.unobs_shape))
        return us_new, lw

    def fused_weight_then_propose(self, us, v, v_prev, t_prev, key_, mask_, resample):
        """One step of pmcmc_filter_step (fbs/samplers/smc.py:144-150): weight the particles, resample,
        propose from the resampled ones.  The reference evaluates the network on `us` for the weights and
        again on `us[inds]` for the proposal; the second input is a row gather of the first, so the network
        runs once and the proposal reads its output rows through `inds`.
        resample(log_ws (n,)) -> inds (n,) int32.  -> (us_new, log_ws (unnormalised), inds)."""
        em = self._em_mask(mask_)
        self._cache = None
        us2 = ops._f32c(us, "us").reshape(us.shape[0], -1)
        net = self._network(us2, None, v_prev, t_prev, em)
        _, lw = self._finish(em, None, None, net, t_prev, v, v_prev, None, None, None, False, True)
        inds = resample(lw).to(torch.int32).contiguous()
        us_new, _ = self._finish(em, us2, inds, net, t_prev, None, None, key_, None, None, True, False, net_A=inds)
        return us_new.reshape((us_new.shape[0],) + tuple(self.dataset.unobs_shape)), lw, inds

    @torch.no_grad()
    def fused_weight_then_propose_batched(self, us, v, v_prev, t_prev, keys, masks, resample):
        """``fused_weight_then_propose`` for B ensembles at the same time step: one weights-only ``fused_step_batched``
        (the step's only network evaluation), ``resample(lw (B, n)) -> inds (B, n)`` local to each ensemble, then one
        fbsmi_em_propose_batched launch that reads the same network buffer through ``inds``.  us (B, n, p, c);
        v, v_prev (B, q, c); keys (B, 2) as in ``fused_step_batched``.  -> (us_new (B, n, p, c), lw (B, n), inds)."""
        us3 = ops._f32c(us, "us")
        B, n = int(us3.shape[0]), int(us3.shape[1])
        us3 = us3.reshape(B, n, -1)
        mb = self.em_mask_batch(masks, B)
        _, lw = self.fused_step_batched(us3, None, v, v_prev, t_prev, None, mb, want_us=False)
        net = self._buf["net"]                               # (B * n, D), written by the call above
        inds = resample(lw).to(torch.int32).contiguous()
        kd = ops.keys_to_device(keys, us3.device)
        if tuple(inds.shape) != (B, n) or kd.numel() != 2 * B:
            raise ValueError("resample must return (B, n) ancestors and keys must be (B, 2)")
        mode, cx, cs, sd = self._coef(t_prev)
        us_new = torch.empty((B, n, mb.du), dtype=torch.float32, device=us3.device)
        _lib.call("fbsmi_em_propose_batched", mb.ref, us3.data_ptr(), inds.data_ptr(), net.data_ptr(), _NET_DT[net.dtype],
                  mode, cx, cs, self.dt, sd, kd.data_ptr(), B, n, us_new.data_ptr(), ops._stream())
        return us_new.reshape((B, n) + tuple(self.dataset.unobs_shape)), lw, inds

    # -- network output shared by the closures of one step --------------------------------------------
    def _net_of(self, us_prev, v_prev, t_prev, mask_):
        c = self._cache
        hit = (c is not None and c["us"] is us_prev and c["usv"] == us_prev._version and c["v"] is v_prev
               and c["vv"] == v_prev._version and c["t"] == float(t_prev) and c["mask"] is mask_)
        if not hit:
            em = self._em_mask(mask_)
            net = self._network(us_prev.reshape(us_prev.shape[0], -1), None, v_prev, t_prev, em)
            # the entry owns references to its key tensors, so their storage cannot be recycled under it
            self._cache = c = {"us": us_prev, "usv": us_prev._version, "v": v_prev, "vv": v_prev._version,
                               "t": float(t_prev), "mask": mask_, "net": net, "em": em}
        return c["em"], c["net"]

    def reverse_drift(self, uv: torch.Tensor, t: float) -> torch.Tensor:      # inpainting.py:102-103
        """Reverse drift of joint images uv (B, w, h, c) at reverse time t (diagnostics; the samplers use
        the fused kernels)."""
        tf = self.T - float(t)
        out = torch.empty(uv.shape, dtype=torch.float32, device=uv.device)
        with torch.no_grad():
            for s in range(0, uv.shape[0], self.chunk):
                x = uv[s:s + self.chunk]
                y = self.score_fn(x.to(self.net_input_dtype), tf).float().reshape(x.shape)
                out[s:s + self.chunk] = y if self.mode == "drift" else \
                    -float(self.sde.drift(1.0, tf)) * x + float(self.sde.dispersion(tf)) ** 2 * y
        return out

    def reverse_dispersion(self, t):                                           # :118-119
        return float(self.sde.dispersion(self.T - float(t)))

    # -- closures (signatures of the reference, mask threaded through **kwargs as `mask_`) ----------
    def unpack(self, xy, mask_):
        return self.dataset.unpack(xy, mask_)

    def transition_sampler(self, us_prev, v_prev, t_prev, key_, mask_, row_slice=None):   # :122-128
        em, net = self._net_of(us_prev, v_prev, t_prev, mask_)
        us2 = ops._f32c(us_prev, "us_prev").reshape(us_prev.shape[0], -1)
        us_new, _ = self._finish(em, us2, None, net, t_prev, None, None, key_, row_slice, None, True, False)
        return us_new.reshape(us_prev.shape)

    def transition_logpdf(self, u, u_prev, v_prev, t_prev, mask_):                        # :131-138
        em, net = self._net_of(u_prev, v_prev, t_prev, mask_)
        mode, cx, cs, sd = self._coef(t_prev)
        us2 = ops._f32c(u_prev, "u_prev").reshape(u_prev.shape[0], -1)
        uu = ops._f32c(u, "u")
        lw = torch.empty(us2.shape[0], dtype=torch.float32, device=us2.device)
        _lib.call("fbsmi_em_transition_logpdf", em.ref, us2.data_ptr(), net.data_ptr(), _NET_DT[net.dtype], mode, cx,
                  cs, self.dt, sd, uu.data_ptr(), us2.shape[0], lw.data_ptr(), ops._stream())
        return lw

    def likelihood_logpdf(self, v, u_prev, v_prev, t_prev, mask_):                        # :141-147
        em, net = self._net_of(u_prev, v_prev, t_prev, mask_)
        _, lw = self._finish(em, None, None, net, t_prev, v, v_prev, None, None, None, False, True)
        return lw

    def fwd_sampler(self, key_, x0_, y0_, mask_):                                         # :150-152
        xy0 = self.dataset.concat(x0_.unsqueeze(0), y0_, mask_)[0]
        if self.mode == "drift":                                                          # sb_imgs/supr.py:132-137
            from .sdes.simulators import euler_maruyama
            return euler_maruyama(key_, xy0, self.ts, self.fwd_drift_fn, self.sde.dispersion, integration_nsteps=1,
                                  return_path=True)
        from .sdes import make_linear_sde
        return make_linear_sde(self.sde)[2](key_, xy0, self.ts)

    def fwd_ys_sampler(self, key_, y0_):                                                  # :155-157
        from .sdes import make_linear_sde
        return make_linear_sde(self.sde)[2](key_, y0_, self.ts)

    # -- the forward paths of B ensembles in lockstep --------------------------------------------------
    def _fwd_tables(self, device):
        """(F, S) of ``simulate_cond_forward(keep_path=True)`` on this bridge's grid (sdes/linear.py:176-178) as float32
        device tables, uploaded once per device."""
        tab = self._buf.get(("fwd_tables", device))
        if tab is None:
            from .sdes.linear import discretise_linear_sde_np
            F, Q = discretise_linear_sde_np(self.sde, self.ts[1:], self.ts[:-1])
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
            tab = self._buf[("fwd_tables", device)] = (up(F), up(np.sqrt(Q)))
        return tab

    @staticmethod
    def _path_out(B: int, slots: int, d: int, tail, batch_major: bool, device):
        """An empty path tensor, (slots, B, *tail) or (B, slots, *tail), with its (slot, ensemble) strides in floats."""
        if batch_major:
            return torch.empty((B, slots) + tuple(tail), dtype=torch.float32, device=device), d, slots * d
        return torch.empty((slots, B) + tuple(tail), dtype=torch.float32, device=device), B * d, d

    def _rows(self, x, B: int, d: int, name: str):
        """One item or B of them (a tensor or a list) -> (B, d) float32, contiguous, on the device."""
        if isinstance(x, (list, tuple)):
            x = torch.stack([torch.as_tensor(v, device=self.dataset.device) for v in x], 0)
        elif not isinstance(x, torch.Tensor):
            x = torch.as_tensor(np.asarray(x, np.float32), device=self.dataset.device)
        x = ops._f32c(x, name)
        if x.numel() == d:
            x = x.reshape(1, d).expand(B, d).contiguous()
        if x.numel() != B * d:
            raise ValueError(f"{name} holds {x.numel()} floats, neither one item of {d} nor {B} of them")
        return x.reshape(B, d)

    @torch.no_grad()
    def fwd_sampler_batched(self, keys, x0s, y0s, masks, want_vs: bool = True, batch_major: bool = False):
        """``fwd_sampler`` for B ensembles, unpacked and reversed in time: keys (B, 2), x0s (B, p, c), y0s one observation
        (q, c) or B of them, masks one mask or a list of B masks of one shape (or an EMMaskBatch).  Returns (us, vs) with

            us[:, b], vs[:, b] = (flip(part, [0]) for part in unpack(fwd_sampler(keys[b], x0s[b], y0s[b], masks[b]), masks[b]))

        bit for bit -- us (T + 1, B, p, c), vs (T + 1, B, q, c), or (B, T + 1, ...) with batch_major; vs is None without
        want_vs.  Score mode: one fbsmi_linear_path_batched launch.  Drift mode with ``fwd_drift_rows_fn``: per step,
        ceil(B / chunk) calls of it on the (B, w, h, c) state and one fbsmi_em_fwd_step_batched launch, nothing read back
        inside the loop; bit-equal whenever the drift's output row does not depend on which rows share its call.  Drift
        mode without it: the loop of ``fwd_sampler``."""
        keys_h = None if isinstance(keys, torch.Tensor) else np.asarray(keys, np.uint32).reshape(-1, 2)
        B = int(keys.numel() // 2) if keys_h is None else keys_h.shape[0]
        mb = self.em_mask_batch(masks, B)
        dev = self.dataset.device
        c = self.dataset.image_shape[2]
        T = self.nsteps
        if self.mode == "drift" and self.fwd_drift_rows_fn is None:
            if keys_h is None:
                keys_h = keys.detach().cpu().numpy().view(np.uint32).reshape(-1, 2)
            y0 = (lambda b: y0s[b]) if (isinstance(y0s, (list, tuple)) or y0s.dim() == 3) else (lambda b: y0s)
            parts = [self.unpack(self.fwd_sampler(keys_h[b], x0s[b], y0(b), mb.ems[b if mb.nmasks > 1 else 0].mask),
                                 mb.ems[b if mb.nmasks > 1 else 0].mask) for b in range(B)]
            us, vs = (torch.flip(torch.stack([p[i] for p in parts], 0), [1]) for i in range(2))
            if not batch_major:
                us, vs = us.transpose(0, 1).contiguous(), vs.transpose(0, 1).contiguous()
            return us, (vs if want_vs else None)
        x0 = self._rows(x0s, B, mb.du, "x0s")
        y0 = self._rows(y0s, B, mb.dv, "y0s") if mb.dv else None
        us, us_slot, us_b = self._path_out(B, T + 1, mb.du, (mb.du // c, c), batch_major, dev)
        vs, vs_slot, vs_b = self._path_out(B, T + 1, mb.dv, (mb.dv // c, c), batch_major, dev) if want_vs else (None, 0, 0)
        ptr = lambda t: t.data_ptr() if t is not None else None
        if self.mode == "score":
            F, S = self._fwd_tables(dev)
            kd = ops.keys_to_device(keys, dev)
            _lib.call("fbsmi_linear_path_batched", mb.ref, mb.D, F.data_ptr(), S.data_ptr(), x0.data_ptr(), ptr(y0),
                      kd.data_ptr(), B, T, 1, us.data_ptr(), us_slot, us_b, ptr(vs), vs_slot, vs_b, ops._stream())
            return us, vs
        if keys_h is None:
            keys_h = keys.detach().cpu().numpy().view(np.uint32).reshape(-1, 2)
        kd = ops.keys_to_device(np.stack([ops.split(keys_h[b], T) for b in range(B)], 1), dev)     # (T, B, 2), uploaded once
        w, h, _ = self.dataset.image_shape
        state = torch.empty((B, w, h, c), dtype=torch.float32, device=dev)
        outs = (us.data_ptr(), us_slot, us_b, ptr(vs), vs_slot, vs_b, ops._stream())
        _lib.call("fbsmi_em_fwd_step_batched", mb.ref, mb.D, x0.data_ptr(), ptr(y0), None, None, 0, 0.0, 0.0, None, 0, 0, B,
                  state.data_ptr(), T, *outs)
        net = None
        for k in range(T):                                   # euler_maruyama(integration_nsteps=1), sdes/simulators.py:55-74
            t, t_next = float(self.ts[k]), float(self.ts[k + 1])
            ddt = abs(t_next - t)
            for s in range(0, B, self.chunk):
                f = self.fwd_drift_rows_fn(state[s:s + self.chunk], t)
                if net is None:
                    if f.dtype not in _NET_DT:
                        f = f.float()
                    net = self._buffer("fwd_net", (B, mb.D), f.dtype, dev)
                net[s:s + self.chunk] = f.reshape(-1, mb.D)
            cc = float(np.float32(float(self.sde.dispersion(t)) * float(np.sqrt(ddt))))
            _lib.call("fbsmi_em_fwd_step_batched", mb.ref, mb.D, None, None, state.data_ptr(), net.data_ptr(),
                      _NET_DT[net.dtype], float(np.float32(ddt)), cc, kd[k].data_ptr(), mb.D, 0, B, state.data_ptr(),
                      T - 1 - k, *outs)
        return us, vs

    @torch.no_grad()
    def fwd_ys_sampler_batched(self, keys, y0s):
        """``fwd_ys_sampler`` for B paths in one fbsmi_linear_path_batched launch: keys (B, 2), y0s one observation (q, c) or
        B of them -> (B, T + 1, q, c) in forward order, row b = fwd_ys_sampler(keys[b], y0s[b]) bit for bit."""
        kd = ops.keys_to_device(keys, self.dataset.device)
        B = int(kd.numel() // 2)
        one = y0s[0] if isinstance(y0s, (list, tuple)) else y0s
        tail = tuple(one.shape[-2:])
        d = int(tail[0] * tail[1])
        y0 = self._rows(y0s, B, d, "y0s")
        F, S = self._fwd_tables(y0.device)
        T = self.nsteps
        out, slot, b_stride = self._path_out(B, T + 1, d, tail, True, y0.device)
        _lib.call("fbsmi_linear_path_batched", None, d, F.data_ptr(), S.data_ptr(), y0.data_ptr(), None, kd.data_ptr(), B, T,
                  0, out.data_ptr(), slot, b_stride, None, 0, 0, ops._stream())
        return out

    def ref_sampler(self, key_, _, n, row_slice=None):                                    # :160-161
        shape = (n,) + tuple(self.dataset.unobs_shape)
        return ops.normal(key_, shape, device=self.dataset.device, rows=None if row_slice is None else row_slice[:2])


def is_own_method(sb, closure, name: str) -> bool:
    """Whether `closure` is bridge `sb`'s OWN method `name` (not a subclass override, a wrapper or another bridge's): the
    test ``bridge_of`` makes, for the closures a caller replaces by the bridge's batched form."""
    return (isinstance(sb, ScoreBridge) and getattr(closure, "__self__", None) is sb
            and getattr(closure, "__func__", None) is getattr(ScoreBridge, name))


def bridge_of(*closures):
    """The ScoreBridge whose OWN transition_sampler / likelihood_logpdf (in that order; a third closure, if given, its
    transition_logpdf) the given closures are, or None.  Callers replace the pair by ``fused_step``, which has exactly those two
    methods' semantics -- so a subclass override, another method of the bridge (e.g. transition_logpdf passed as the weight
    function) or a swapped pair must not be taken for them."""
    owners = [getattr(c, "__self__", None) for c in closures]
    if not owners or not isinstance(owners[0], ScoreBridge) or not all(o is owners[0] for o in owners):
        return None
    want = (ScoreBridge.transition_sampler, ScoreBridge.likelihood_logpdf, ScoreBridge.transition_logpdf)
    if len(closures) > len(want):
        return None
    for c, w in zip(closures, want):
        if getattr(c, "__func__", None) is not w:
            return None
    return owners[0]
