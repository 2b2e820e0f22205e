"""The conditional score sampler (CSGM; Song et al., 2021) for the analytic Gaussian model of experiments/toy/gp_csgm.py as
a model descriptor.

For a Gaussian prior ``x ~ N(mean, cov)`` observed as ``y = x + N(0, obs_var I)`` and noised by a scalar-coefficient linear
SDE, both the marginal score at forward time s and the score of ``p(y | u_s)`` are Gaussian, so the reverse drift
``-a u + b^2 (grad log p_s(u) + grad_u log p(y | u_s = u))`` (gp_csgm.py:80-94, the second term by jax.grad there) is
affine: ``f(u) = A[k] u + cvec[k]``.  A conditional sample is ``u0 = m_ref + S_ref z`` followed by T Euler-Maruyama steps.

``lg_csgm_tables`` builds the tables in float64 on the host; ``GaussianCSGM`` keeps float32 copies on the GPU and exposes
the closures (plain torch on the tables: the fall-back tier) and the fused, batched engine (``handle``; include/fbsmi.h,
fbsmi_csgm_*) that ``fbs_amd.sdes.simulators.euler_maruyama`` dispatches to when it is handed them.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .linear_gaussian import _Closure, _LGHandle
from .sdes.linear import LinearSDE, discretise_linear_sde_np

MAX_D, MAX_SAMPLES = 128, 131072   # fbsmi_csgm_create


def lg_csgm_tables(mean, cov, sde: LinearSDE, ts, obs_var, y) -> dict:
    """Float64 tables of the fused CSGM (include/fbsmi.h, fbsmi_csgm_model), no device needed.  One entry per step
    k = 0..T-1: euler_maruyama evaluates the drift and the dispersion at ts[k].

    The terminal reference follows gp_csgm.py:69-76: ``m_ref`` and ``S_ref`` are the mean and the covariance of
    ``u_T | y``, and the reference multiplies the initial normal by ``S_ref`` itself, not by a Cholesky factor of it.  That
    is kept: ``u0 = m_ref + S_ref z``."""
    mean = np.asarray(mean, np.float64).reshape(-1)
    cov = np.asarray(cov, np.float64)
    y = np.asarray(y, np.float64).reshape(-1)
    ts = np.asarray(ts, np.float64).reshape(-1)
    d, T = mean.size, ts.size - 1
    obs_var = float(obs_var)
    eye = np.eye(d)
    Kyy = cov + obs_var * eye
    A, cvec = np.zeros((T, d, d)), np.zeros((T, d))
    ddt, s_tab = np.zeros(T, np.float32), np.zeros(T, np.float32)
    for k in range(T):
        s = ts[-1] - ts[k]
        F, Q = (float(v) for v in discretise_linear_sde_np(sde, s, ts[0]))
        a, b = float(sde.drift(1.0, s)), float(sde.dispersion(s))
        Sx_inv = np.linalg.inv(F ** 2 * cov + Q * eye)
        M = F * cov @ Sx_inv                                   # E[x | u] = mean + M (u - F mean)
        cond_cov = Kyy - M @ (F * cov)                          # Cov[y | u]
        Gm = M.T @ np.linalg.inv(cond_cov)                      # grad_u log p(y | u) = Gm (y - mean - M (u - F mean))
        A[k] = -a * eye + b ** 2 * (-Sx_inv - Gm @ M)
        cvec[k] = b ** 2 * (Sx_inv @ (F * mean) + Gm @ (y - mean + M @ (F * mean)))
        h64 = abs(float(ts[k + 1]) - float(ts[k]))
        ddt[k] = np.float32(h64)
        s_tab[k] = np.float32(b * float(np.sqrt(h64)))          # the rounding of oracle.euler_maruyama_np
    F_T, Q_T = (float(v) for v in discretise_linear_sde_np(sde, ts[-1], ts[0]))
    m_ref = F_T * mean + F_T * cov @ np.linalg.solve(Kyy, y - mean)
    S_ref = F_T ** 2 * cov + Q_T * eye - F_T * cov @ np.linalg.solve(Kyy, F_T * cov)
    return dict(d=d, T=T, A=A, cvec=cvec, ddt=ddt, s=s_tab, m_ref=m_ref, S_ref=S_ref, y=y, obs_var=obs_var)


_ROLES = ("reverse_drift", "reverse_dispersion", "ref_sampler")
_ARRAYS = ("A", "cvec", "ddt", "s", "m_ref", "S_ref")


class GaussianCSGM:
    def __init__(self, mean, cov, sde: LinearSDE, ts, obs_var, y, device=None):
        self.sde = sde
        self.device = torch.device(device) if device is not None else ops._default_device()
        self.ts_np = np.asarray(ts.detach().cpu() if isinstance(ts, torch.Tensor) else ts, np.float64).reshape(-1)
        tab = self.tables64 = lg_csgm_tables(mean, cov, sde, self.ts_np, obs_var, y)
        self.d, self.T = tab["d"], tab["T"]
        self.host = {k: np.ascontiguousarray(np.asarray(tab[k], np.float32)) for k in _ARRAYS}
        self.dev = {k: torch.from_numpy(v).to(self.device) for k, v in self.host.items()}
        self.struct = _lib.CSGMModelStruct(self.d, self.T, *(self.dev[k].data_ptr() for k in _ARRAYS))
        self._handles = {}
        for role in _ROLES:
            setattr(self, role, _Closure(self, getattr(self, "_" + role), role))

    # -- helpers ---------------------------------------------------------------------------------
    def point_of(self, t) -> int:
        """Index of the step that starts at t; the closures are tabulated on the model's own grid."""
        t = float(t)
        k = int(np.argmin(np.abs(self.ts_np[:-1] - t)))
        if abs(self.ts_np[k] - t) > 1e-6 * max(1.0, abs(self.ts_np[-1])):
            raise ValueError(f"t = {t} is not the start of a step of this model's time grid (nearest: {self.ts_np[k]})")
        return k

    def same_grid(self, ts) -> bool:
        ts = np.asarray(ts.detach().cpu() if isinstance(ts, torch.Tensor) else ts, np.float64).reshape(-1)
        return ts.shape == self.ts_np.shape and bool(np.allclose(ts, self.ts_np, rtol=0.0, atol=1e-9 * max(1.0, abs(self.ts_np[-1]))))

    def fused_supported(self, nsamples: int) -> bool:
        """What fbsmi_csgm_create accepts."""
        return 1 <= self.d <= MAX_D and 1 <= int(nsamples) <= MAX_SAMPLES

    def _t(self, x) -> torch.Tensor:
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(np.asarray(x, np.float32))
        return x.to(self.device, torch.float32)

    # -- closures (experiments/toy/gp_csgm.py:69-108) ----------------------------------------------
    def _reverse_drift(self, u, t):                                                     # :93-94
        k = self.point_of(t)
        return self._t(u) @ self.dev["A"][k].T + self.dev["cvec"][k]

    def _reverse_dispersion(self, t):                                                   # :96-97
        k = self.point_of(t)
        return float(self.sde.dispersion(float(self.ts_np[-1] - self.ts_np[k])))

    def _ref_sampler(self, key):                                                        # :105
        return self.dev["m_ref"] + self.dev["S_ref"] @ ops.normal(key, (self.d,), device=self.device)

    # -- fused engine ----------------------------------------------------------------------------
    def handle(self, nsamples: int, store_path: bool = False):
        keyt = (int(nsamples), bool(store_path))
        h = self._handles.get(keyt)
        if h is None:
            h = self._handles[keyt] = CsgmHandle(self, *keyt)
        return h


def fused_csgm(x0, ts, drift, dispersion, integration_nsteps, key=None):
    """(model, B) when the fused CSGM engine serves an euler_maruyama call: drift and dispersion are the reverse_drift /
    reverse_dispersion closures of one GaussianCSGM, ts is its grid, one sub-step per interval, x0 of shape (d,) or
    (B, d) with one key per row, a supported size.

    A (B, d) state under ONE key is the host loop's: there the B rows share each step's draw normal(keys[k], (1, B, d)),
    which is not B independent trajectories."""
    model = getattr(drift, "_fbsmi_lg", None)
    if not isinstance(model, GaussianCSGM) or getattr(dispersion, "_fbsmi_lg", None) is not model:
        return None
    if getattr(drift, "_role", "") != "reverse_drift" or getattr(dispersion, "_role", "") != "reverse_dispersion":
        return None
    if int(integration_nsteps) != 1 or not model.same_grid(ts):
        return None
    shape = tuple(x0.shape)
    if len(shape) not in (1, 2) or shape[-1] != model.d:
        return None
    B = 1 if len(shape) == 1 else shape[0]
    if key is not None:
        nk = int(np.asarray(key.detach().cpu() if isinstance(key, torch.Tensor) else key).size)
        if nk != 2 * B:
            return None
    if not model.fused_supported(B):
        return None
    return model, B


class CsgmHandle(_LGHandle):
    """Owns one fbsmi_csgm handle: up to `nsamples` independent conditional samples per call, one kernel launch, nothing on
    the host inside a trajectory.  A call with fewer keys than `nsamples` (a ragged last batch) runs on the model's
    handle of that size."""

    _DESTROY = "fbsmi_csgm_destroy"

    def __init__(self, model: GaussianCSGM, nsamples, store_path=False):
        if not model.fused_supported(nsamples):
            raise NotImplementedError(f"the fused CSGM takes 1 <= d <= {MAX_D} and 1 <= nsamples <= {MAX_SAMPLES}")
        self.model, self.n, self.store = model, int(nsamples), bool(store_path)
        self.C = self.n
        self._last = self
        h = C.c_void_p()
        with torch.cuda.device(model.device):
            _lib.call("fbsmi_csgm_create", C.byref(model.struct), self.n, int(self.store), C.byref(h))
        self.h = h

    def _call(self, keys, u0):
        m = self.model
        k = np.asarray(keys.detach().cpu() if isinstance(keys, torch.Tensor) else keys).astype(np.uint32).reshape(-1, 2)
        B = k.shape[0]
        if not 1 <= B <= self.n:
            raise ValueError(f"{B} keys for a handle of {self.n} samples")
        if B < self.n:
            self._last = m.handle(B, self.store)
            return self._last._call(k, u0)
        self._last = self
        kt = torch.from_numpy(k.view(np.int32).copy()).to(m.device)
        u0t = self._dev(u0, torch.float32, (B, m.d)) if u0 is not None else None
        out = torch.empty((B, m.d), dtype=torch.float32, device=m.device)
        with torch.cuda.device(m.device):
            _lib.call("fbsmi_csgm_run", self.h, kt.data_ptr(), u0t.data_ptr() if u0t is not None else None, out.data_ptr(),
                      ops._stream())
        return out

    def sample(self, keys):
        """conditional_sampler (gp_csgm.py:103-108) for B keys at once: keys (B, 2), or (2,) for one sample -> (B, d)."""
        return self._call(keys, None)

    def integrate(self, keys, u0):
        """euler_maruyama(keys[b], u0[b], ts, reverse_drift, reverse_dispersion) for every row b -> (B, d)."""
        return self._call(keys, u0)

    def views(self) -> dict:
        """State of the last call: u0 (B, d) the initial states, path (T+1, B, d) every step's state (store_path)."""
        h, m = self._last, self.model
        out = {}
        for name, which, shape in (("u0", 0, (h.n, m.d)), ("path", 1, (m.T + 1, h.n, m.d))):
            if which == 1 and not h.store:
                continue
            t = torch.empty(shape, dtype=torch.float32, device=m.device)
            _lib.call("fbsmi_csgm_view", h.h, which, t.data_ptr(), None, ops._stream())
            out[name] = t
        return out
