"""SDE simulators with the reference's signatures (fbs/sdes/simulators.py).

``euler_maruyama`` / ``reverse_simulator`` / ``discrete_time_simulator`` take arbitrary drift
closures on torch tensors, so their time loop is host Python with the noise drawn by the JAX-
compatible device PRNG.  ``doob_bridge_simulator`` has a drift that is affine in x for every
scalar linear SDE, so the whole (T x integration_nsteps)-step path is ONE kernel launch
(fbsmi_affine_em_path), and so is ``euler_maruyama`` on the closures of a ``GaussianCSGM`` (fbsmi_csgm_run).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib, ops
from .linear import LinearSDE, _as_np, doob_bridge_tables


def reverse_simulator(key, u0, ts, score, drift, dispersion, integration_nsteps: int = 1,
                      integrator: str = 'euler-maruyama'):
    """Simulate the time-reversal of an SDE (fbs/sdes/simulators.py:8-50)."""
    T = float(_as_np(ts).reshape(-1)[-1])

    def reverse_drift(u, t):
        return -drift(u, T - t) + dispersion(T - t) ** 2 * score(u, T - t)

    def reverse_dispersion(t):
        return dispersion(T - t)

    if integrator == 'euler-maruyama':
        return euler_maruyama(key, u0, ts, reverse_drift, reverse_dispersion, integration_nsteps=integration_nsteps)
    raise NotImplementedError(f'Integrator {integrator} not implemented.')


def euler_maruyama(key, x0, ts, drift, dispersion, integration_nsteps: int = 1, return_path: bool = False):
    """Euler-Maruyama with sub-stepping (fbs/sdes/simulators.py:53-106)."""
    ts_np = _as_np(ts).reshape(-1)
    n = ts_np.size - 1
    if not isinstance(x0, torch.Tensor):
        x0 = torch.as_tensor(np.asarray(x0, np.float32), device=ops._default_device())
    ops._require_cuda(x0, "x0")
    from ..lg_csgm import fused_csgm
    hit = fused_csgm(x0, ts_np, drift, dispersion, integration_nsteps, key)
    if hit is not None:
        # the closures of one GaussianCSGM on its own grid: the whole path is one kernel launch (fbsmi_csgm_run)
        model, B = hit
        h = model.handle(B, store_path=bool(return_path))
        xT = h.integrate(key, x0.reshape(B, model.d))
        if return_path:
            return h.views()["path"].reshape((n + 1,) + tuple(x0.shape))
        return xT.reshape(x0.shape)
    keys = ops.split(key, n)
    x = x0.to(torch.float32).contiguous()
    path = [x]
    numel = x.numel()
    for k in range(n):
        t, t_next = float(ts_np[k]), float(ts_np[k + 1])
        ddt = abs(t_next - t) / integration_nsteps
        sub_ts = np.linspace(t, t_next - ddt, integration_nsteps)
        k0, k1 = int(keys[k][0]), int(keys[k][1])
        for j in range(integration_nsteps):
            t_ = float(sub_ts[j])
            # x + drift * ddt + dispersion * sqrt(ddt) * rnds[j] with rnds = normal(keys[k], (nsub, *shape)) (:91-99): one
            # kernel per sub-step, the noise drawn inside it (fbsmi_em_update)
            f = drift(x, t_)
            if not (isinstance(f, torch.Tensor) and f.shape == x.shape):
                f = torch.as_tensor(f, dtype=torch.float32, device=x.device).expand(x.shape)
            f = f.to(torch.float32).contiguous()
            c = float(np.float32(float(dispersion(t_)) * float(np.sqrt(ddt))))
            out = torch.empty_like(x)
            _lib.call("fbsmi_em_update", x.data_ptr(), f.data_ptr(), float(np.float32(ddt)), c, k0, k1,
                      integration_nsteps * numel, j * numel, numel, out.data_ptr(), ops._stream())
            x = out
        if return_path:
            path.append(x)
    return torch.stack(path, dim=0) if return_path else x


def discrete_time_simulator(key, x0, ts, f, q):
    """X(t_{k+1}) = f(X(t_k), t_{k+1}, t_k) + q(t_{k+1}, t_k) w  (fbs/sdes/simulators.py:109-123)."""
    ts_np = _as_np(ts).reshape(-1)
    if not isinstance(x0, torch.Tensor):
        x0 = torch.as_tensor(np.asarray(x0, np.float32), device=ops._default_device())
    rnds = ops.normal(key, (ts_np.size - 1,) + tuple(x0.shape), device=x0.device)
    x = x0
    for k in range(ts_np.size - 1):
        x = f(x, float(ts_np[k + 1]), float(ts_np[k])) + q(float(ts_np[k + 1]), float(ts_np[k])) * rnds[k]
    return x


def doob_bridge_simulator(key, sde: LinearSDE, x0, xT, ts, integration_nsteps: int = 1, replace: bool = False):
    """Doob h-transform bridge of a linear SDE from x0 to xT (fbs/sdes/simulators.py:126-160).

    bridge_drift(x, t) = A(t) x + B(t) xT is affine in x, so the path is one kernel launch: the
    host tabulates A, B and the dispersion at every sub-step time (float64 -> float32, doob_bridge_tables)."""
    ts_np = _as_np(ts).reshape(-1)
    T = ts_np.size - 1
    nsub = int(integration_nsteps)
    dev = x0.device if isinstance(x0, torch.Tensor) else ops._default_device()
    x0t = torch.as_tensor(np.asarray(x0, np.float32)) if not isinstance(x0, torch.Tensor) else x0
    xTt = torch.as_tensor(np.asarray(xT, np.float32)) if not isinstance(xT, torch.Tensor) else xT
    x0t = x0t.to(dev, torch.float32).contiguous()
    xTt = xTt.to(dev, torch.float32).contiguous()
    shape = tuple(x0t.shape)
    D = x0t.numel()
    tab = doob_bridge_tables(sde, ts_np, nsub)
    keys = ops.split(key, T)
    up = lambda a: torch.from_numpy(a).to(dev)
    keys_t = torch.from_numpy(keys.view(np.int32).copy()).to(dev)
    At, Bt, St, ht = up(tab["A"]), up(tab["B"]), up(tab["S"]), up(tab["ddt"])
    out = torch.empty((T + 1, D), dtype=torch.float32, device=dev)
    _lib.call("fbsmi_affine_em_path", keys_t.data_ptr(), At.data_ptr(), Bt.data_ptr(), St.data_ptr(), ht.data_ptr(),
              xTt.reshape(-1).data_ptr(), x0t.reshape(-1).data_ptr(), T, nsub, D, int(bool(replace)), out.data_ptr(),
              ops._stream())
    return out.reshape((T + 1,) + shape)


def doob_bridge_simulator_batched(keys, sde: LinearSDE, x0s, xTs, ts, integration_nsteps: int = 1, replace: bool = False,
                                  reverse: bool = False, time_major: bool = False):
    """``doob_bridge_simulator`` for B bridges on one grid in ONE launch (fbsmi_affine_em_path_batched): keys (B, 2), x0s
    and xTs (B, ...) device tensors.  The tables are built and uploaded once per call, the ``split(key, T)`` of every
    bridge is done on the host.  -> (B, T + 1, ...), or (T + 1, B, ...) with time_major; bridge b has the bits of
    ``doob_bridge_simulator(keys[b], sde, x0s[b], xTs[b], ts, integration_nsteps, replace)``, its points in reverse
    order with ``reverse`` (point k in slot T - k: what ``torch.flip(., [0])`` would give)."""
    ts_np = _as_np(ts).reshape(-1)
    T = ts_np.size - 1
    nsub = int(integration_nsteps)
    keys = np.asarray(keys.detach().cpu() if isinstance(keys, torch.Tensor) else keys, np.uint32).reshape(-1, 2)
    B = keys.shape[0]
    x0t = ops._f32c(x0s if isinstance(x0s, torch.Tensor) else torch.stack(list(x0s), 0), "x0s")
    xTt = ops._f32c(xTs if isinstance(xTs, torch.Tensor) else torch.stack(list(xTs), 0), "xTs")
    if x0t.shape[0] != B or xTt.shape != x0t.shape:
        raise ValueError("doob_bridge_simulator_batched: keys (B, 2), x0s (B, ...) and xTs (B, ...) must match")
    dev = x0t.device
    shape = tuple(x0t.shape[1:])
    D = x0t[0].numel()
    tab = doob_bridge_tables(sde, ts_np, nsub)
    step_keys = np.stack([ops.split(keys[b], T) for b in range(B)], 0) if T else np.zeros((B, 0, 2), np.uint32)
    up = lambda a: torch.from_numpy(a).to(dev)
    keys_t = ops.keys_to_device(step_keys, dev)
    At, Bt, St, ht = up(tab["A"]), up(tab["B"]), up(tab["S"]), up(tab["ddt"])
    out = torch.empty((T + 1, B, D) if time_major else (B, T + 1, D), dtype=torch.float32, device=dev)
    slot_stride, ens_stride = (B * D, D) if time_major else (D, (T + 1) * D)
    ptr = lambda t: t.data_ptr() if T else None
    _lib.call("fbsmi_affine_em_path_batched", ptr(keys_t), ptr(At), ptr(Bt), ptr(St), ptr(ht), xTt.data_ptr(),
              x0t.data_ptr(), T, nsub, D, int(bool(replace)), B, out.data_ptr(), slot_stride, ens_stride, int(bool(reverse)),
              ops._stream())
    return out.reshape(((T + 1, B) if time_major else (B, T + 1)) + shape)
