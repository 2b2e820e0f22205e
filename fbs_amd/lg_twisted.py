"""Twisted SMC (Wu et al., 2023) for the analytic Gaussian model of experiments/toy/gp_twisted.py as a model descriptor.

For a Gaussian prior ``x ~ N(mean, cov)`` noised by a scalar-coefficient linear SDE, the score of the marginal at forward
time s is affine, so the reverse drift is ``rd(u) = R u + r`` (gp_twisted.py:83-84).  The twisting function
``N(y; u + rd(u) dt, obs_var I)`` (:113-115) is then a Gaussian density of the affine map ``B u + dt r`` with
``B = I + dt R``, and its gradient -- which the reference takes with jax.grad (:87-89) -- is
``B^T (y - B u - dt r) / obs_var``: the conditional reverse drift is affine too, ``rcd(u) = C u + c``.

``lg_twisted_tables`` builds those tables in float64 on the host; ``GaussianTwisted`` keeps float32 copies on the GPU and
exposes the reference's five closures (plain torch on the tables: the fall-back tier) and the fused, batched engine
(``handle``; include/fbsmi.h, fbsmi_tw_*) that ``fbs_amd.samplers.smc.twisted_smc`` dispatches to when it is handed them.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib, ops
from .linear_gaussian import _Closure, _LGHandle
from .sdes.linear import LinearSDE, discretise_linear_sde_np

MAX_D, MAX_PARTICLES = 128, 131072   # the wide family's limits (fbsmi_tw_create)
MAX_RUNS = 65535                     # nruns of a handle: a run is one grid row of every launch (fbsmi_tw_create)


def lg_twisted_tables(mean, cov, sde: LinearSDE, ts, obs_var, y) -> dict:
    """Float64 tables of the fused twisted SMC (include/fbsmi.h, fbsmi_tw_model), no device needed.  One entry per time
    point j = 0..T: twisted_smc evaluates the closures at ts[0] (initial twist) and at ts[k+1] (step k)."""
    mean = np.asarray(mean, np.float64).reshape(-1)
    cov = np.asarray(cov, np.float64)
    y = np.asarray(y, np.float64).reshape(-1)
    ts = np.asarray(ts, np.float64).reshape(-1)
    d, T = mean.size, ts.size - 1
    obs_var = float(obs_var)
    dt = float((ts[-1] - ts[0]) / T)
    eye = np.eye(d)
    R, r, Cm, c = np.zeros((T + 1, d, d)), np.zeros((T + 1, d)), np.zeros((T + 1, d, d)), np.zeros((T + 1, d))
    sd = np.zeros(T + 1)
    for j in range(T + 1):
        s = ts[-1] - ts[j]
        F, Q = discretise_linear_sde_np(sde, s, ts[0])
        P = np.linalg.inv(F ** 2 * cov + Q * eye)
        a, b = float(sde.drift(1.0, s)), float(sde.dispersion(s))
        R[j] = -a * eye - b ** 2 * P
        r[j] = b ** 2 * (P @ (F * mean))
        B = eye + dt * R[j]
        Cm[j] = R[j] - (b ** 2 / obs_var) * (B.T @ B)
        c[j] = r[j] + (b ** 2 / obs_var) * (B.T @ (y - dt * r[j]))
        sd[j] = math.sqrt(dt) * b
    F_T, Q_T = discretise_linear_sde_np(sde, ts[-1], ts[0])
    Lt = np.linalg.cholesky(F_T ** 2 * cov + Q_T * eye).T.copy()
    with np.errstate(divide="ignore"):
        lognorm = np.log(2 * np.pi * sd ** 2)
    return dict(d=d, T=T, dt=dt, R=R, r=r, C=Cm, c=c, sd=sd, lognorm=lognorm, m_ref=F_T * mean, Lt=Lt, y=y,
                obs_var=obs_var, lognorm_obs=math.log(2 * math.pi * obs_var))


_ROLES = ("init_sampler", "transition_logpdf", "twisting_logpdf", "twisting_prop_sampler", "twisting_prop_logpdf")
_ARRAYS = ("R", "r", "C", "c", "sd", "lognorm", "m_ref", "Lt", "y")


class GaussianTwisted:
    def __init__(self, mean, cov, sde: LinearSDE, ts, obs_var, y, device=None):
        self.sde = sde
        self.device = torch.device(device) if device is not None else ops._default_device()
        self.ts_np = np.asarray(ts.detach().cpu() if isinstance(ts, torch.Tensor) else ts, np.float64).reshape(-1)
        tab = self.tables64 = lg_twisted_tables(mean, cov, sde, self.ts_np, obs_var, y)
        self.d, self.T = tab["d"], tab["T"]
        self.dt, self.obs_var, self.lognorm_obs = np.float32(tab["dt"]), np.float32(tab["obs_var"]), np.float32(tab["lognorm_obs"])
        self.host = {k: np.ascontiguousarray(np.asarray(tab[k], np.float32)) for k in _ARRAYS}
        self.dev = {k: torch.from_numpy(v).to(self.device) for k, v in self.host.items()}
        self.struct = _lib.TWModelStruct(self.d, self.T, float(self.dt), *(self.dev[k].data_ptr() for k in _ARRAYS),
                                         float(self.obs_var), float(self.lognorm_obs))
        self._handles = {}
        for role in _ROLES:
            setattr(self, role, _Closure(self, getattr(self, "_" + role), role))

    # -- helpers ---------------------------------------------------------------------------------
    def point_of(self, t) -> int:
        """Index of the grid point t; the closures are tabulated on the model's own grid."""
        t = float(t)
        j = int(np.argmin(np.abs(self.ts_np - t)))
        if abs(self.ts_np[j] - t) > 1e-6 * max(1.0, abs(self.ts_np[-1])):
            raise ValueError(f"t = {t} is not a point of this model's time grid (nearest: {self.ts_np[j]})")
        return j

    def same_grid(self, ts) -> bool:
        ts = np.asarray(ts.detach().cpu() if isinstance(ts, torch.Tensor) else ts, np.float64).reshape(-1)
        return ts.shape == self.ts_np.shape and bool(np.allclose(ts, self.ts_np, rtol=0.0, atol=1e-9 * max(1.0, abs(self.ts_np[-1]))))

    def same_y(self, y) -> bool:
        y = np.asarray(y.detach().cpu() if isinstance(y, torch.Tensor) else y, np.float32).reshape(-1)
        return y.shape == self.host["y"].shape and bool(np.array_equal(y, self.host["y"]))

    def fused_supported(self, nparticles: int) -> bool:
        """What fbsmi_tw_create accepts."""
        return 1 <= self.d <= MAX_D and 1 <= int(nparticles) <= MAX_PARTICLES

    def _t(self, x) -> torch.Tensor:
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(np.asarray(x, np.float32))
        return x.to(self.device, torch.float32)

    def _affine(self, M, m, j, u):
        return u @ self.dev[M][j].T + self.dev[m][j]

    @staticmethod
    def _nlp_sum(x, loc, s2, ln):
        return ((ln + (x - loc) ** 2 / s2) / -2.0).sum(dim=-1)

    # -- closures (experiments/toy/gp_twisted.py:100-129) ------------------------------------------
    def _init_sampler(self, key_, nparticles_):                                         # :107-110
        return self.dev["m_ref"] + ops.normal(key_, (int(nparticles_), self.d), device=self.device) @ self.dev["Lt"]

    def _transition_logpdf(self, u, u_prev, t_prev):                                    # :100-104
        j = self.point_of(t_prev)
        u, u_prev = self._t(u), self._t(u_prev)
        sd = float(self.host["sd"][j])
        return self._nlp_sum(u, u_prev + self._affine("R", "r", j, u_prev) * float(self.dt), sd * sd, float(self.host["lognorm"][j]))

    def _twisting_logpdf(self, y, u, t):                                                # :113-115
        j = self.point_of(t)
        u = self._t(u)
        return self._nlp_sum(self._t(y), u + self._affine("R", "r", j, u) * float(self.dt), float(self.obs_var),
                             float(self.lognorm_obs))

    def _prop_mean(self, us, j, y):
        """us + rcd(us) dt; the tabulated c is the model's own y, another y moves it by (b^2 / obs_var) B^T (y - y_model)."""
        m = us + self._affine("C", "c", j, us) * float(self.dt)
        if not self.same_y(y):
            b2 = float(self.host["sd"][j]) ** 2 / float(self.dt)
            Bm = torch.eye(self.d, device=self.device) + float(self.dt) * self.dev["R"][j]
            m = m + ((self._t(y) - self.dev["y"]) @ Bm) * (b2 / float(self.obs_var) * float(self.dt))
        return m

    def _twisting_prop_sampler(self, key_, us, t, y):                                   # :121-123
        j = self.point_of(t)
        us = self._t(us)
        return self._prop_mean(us, j, y) + float(self.host["sd"][j]) * ops.normal(key_, tuple(us.shape), device=self.device)

    def _twisting_prop_logpdf(self, u, u_prev, t, y):                                   # :126-129
        j = self.point_of(t)
        sd = float(self.host["sd"][j])
        return self._nlp_sum(self._t(u), self._prop_mean(self._t(u_prev), j, y), sd * sd, float(self.host["lognorm"][j]))

    # -- fused engine ----------------------------------------------------------------------------
    def handle(self, nparticles: int, resampling: str = "stratified", nruns: int = 1, store_ancestors: bool = False):
        keyt = (int(nparticles), resampling, int(nruns), bool(store_ancestors))
        h = self._handles.get(keyt)
        if h is None:
            h = self._handles[keyt] = TwistedHandle(self, *keyt)
        return h


def fused_twisted(y, ts, init_sampler, transition_logpdf, twisting_logpdf, twisting_prop_sampler, twisting_prop_logpdf,
                  resampling, nparticles, kwargs):
    """(model, resampling name) when the fused twisted SMC applies: all five closures are one GaussianTwisted's own, on its
    grid and for its y, the resampler is this package's stratified or systematic, no kwargs, a supported size."""
    from .samplers import resampling as _resampling
    model = getattr(init_sampler, "_fbsmi_lg", None)
    if not isinstance(model, GaussianTwisted) or kwargs:
        return None
    for closure, role in zip((init_sampler, transition_logpdf, twisting_logpdf, twisting_prop_sampler, twisting_prop_logpdf),
                             _ROLES):
        if getattr(closure, "_fbsmi_lg", None) is not model or getattr(closure, "_role", "") != role:
            return None
    name = "stratified" if resampling is _resampling.stratified else (
        "systematic" if resampling is _resampling.systematic else None)
    if name is None or not model.fused_supported(nparticles) or not model.same_grid(ts) or not model.same_y(y):
        return None
    return model, name


class TwistedHandle(_LGHandle):
    """Owns one fbsmi_tw handle: `nruns` independent twisted-SMC runs per call, one hipGraph replay, nothing on the host
    inside a run."""

    _RES = {"stratified": 0, "systematic": 1}
    _DESTROY = "fbsmi_tw_destroy"

    def __init__(self, model: GaussianTwisted, nparticles, resampling, nruns=1, store_ancestors=False):
        if not model.fused_supported(nparticles):
            raise NotImplementedError(f"the fused twisted SMC takes 1 <= d <= {MAX_D} and 1 <= nparticles <= {MAX_PARTICLES}")
        if not 1 <= int(nruns) <= MAX_RUNS:
            raise NotImplementedError(f"the fused twisted SMC takes 1 <= nruns <= {MAX_RUNS}")
        self.model, self.n, self.C, self.store = model, int(nparticles), int(nruns), bool(store_ancestors)
        h = C.c_void_p()
        with torch.cuda.device(model.device):
            _lib.call("fbsmi_tw_create", C.byref(model.struct), self.n, self._RES[resampling], self.C, int(self.store),
                      C.byref(h))
        self.h = h

    def _call(self, keys, select, use_graph):
        m, B = self.model, self.C
        kt = self._key_t(keys, B)
        xs = torch.empty((B, self.n, m.d), dtype=torch.float32, device=m.device)
        lws = torch.empty((B, self.n), dtype=torch.float32, device=m.device)
        smp = torch.empty((B, m.d), dtype=torch.float32, device=m.device) if select else None
        _lib.call("fbsmi_tw_run", self.h, kt.data_ptr(), int(select), xs.data_ptr(), lws.data_ptr(),
                  smp.data_ptr() if select else None, int(bool(use_graph)), ops._stream())
        return xs, lws, smp

    def run(self, keys, use_graph=True):
        """keys (B, 2), or (2,) for a handle of one run -> particles (B, N, d), normalised log-weights (B, N)."""
        xs, lws, _ = self._call(keys, 0, use_graph)
        return xs, lws

    def sample(self, keys, use_graph=True):
        """gp_twisted.py:133-141 for B keys at once: key_filter, key_select = split(key), the run, the choice -> (B, d)."""
        return self._call(keys, 1, use_graph)[2]

    def views(self) -> dict:
        """State of the last run: ancestors (B, T, N) int32 of every step (store_ancestors); of the last step log_ps, tl,
        pl (B, N), xs_prev (B, N, d) before resampling and last_ancestors (B, N)."""
        m, B = self.model, self.C
        out = {}
        for name, which, shape, dtype in (("ancestors", 0, (B, m.T, self.n), torch.int32), ("log_ps", 1, (B, self.n), torch.float32),
                                          ("tl", 2, (B, self.n), torch.float32), ("pl", 3, (B, self.n), torch.float32),
                                          ("xs_prev", 4, (B, self.n, m.d), torch.float32),
                                          ("last_ancestors", 5, (B, self.n), torch.int32)):
            if which == 0 and not self.store:
                continue
            t = torch.empty(shape, dtype=dtype, device=m.device)
            _lib.call("fbsmi_tw_view", self.h, which, t.data_ptr(), None, ops._stream())
            out[name] = t
        return out
