"""The Kalman-filter conditional sampler of the analytic linear-Gaussian model (counterpart of experiments/toy/gp_kf.py).

The discretised model that ``bootstrap_filter`` targets on a LinearGaussianBridge is linear-Gaussian: with
``M_k = I + dt G[k] = [[A, B], [C, D]]`` (u rows first), ``(c; e) = dt g[k]`` and ``q = sd[k]^2``,

    u_0 | v_0 ~ N(m_0, Sigma_0)                              (ref_sampler)
    v_{k+1} | u_k, v_k ~ N(C u_k + D v_k + e, q I)           (likelihood_logpdf: given the PREVIOUS state)
    u_{k+1} | u_k, v_k ~ N(A u_k + B v_k + c, q I)           (transition_sampler: the state then propagated)

so the filtering law ``p(u_T | v_0..v_T)`` and the marginal likelihood ``p(v_1..v_T | v_0)`` are closed-form: the
N -> infinity limit of ``filter_conditional_sampler`` and the exact value of the ``-nell`` the fused filters estimate.
gp_kf.py itself takes the Jacobian of the observation mean with respect to v_prev and passes sqrt(dt) b where a covariance
is expected; this is the exact filter of the model, not that recursion.

``lg_kalman_tables`` does the data-independent covariance recursion once in float64 on the host; ``kalman_filter_np`` is
the float64 mean recursion on them (the yardstick of the tests); ``LGKalman`` owns the fused, batched engine
(include/fbsmi.h, fbsmi_kf_*).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .linear_gaussian import LinearGaussianBridge, _LGHandle

MAX_D, MAX_SAMPLES = 128, 65535      # fbsmi_kf_create
KF_PATH_ELEMS = 1 << 26              # B * (T + 1) * dv float32 elements of one call's observation paths: 256 MB
KF_MAX_SAMPLES = 16384               # samples per fused call (plan_filter_chunks' convention)


def initial_cov(cov_ref, du: int):
    """Sigma_0 = cov_ref[:du, :du] - gain cov_ref[du:, :du]: the float64 matrix whose Cholesky factor lg_pmcmc_tables
    rounds to ``chol`` (the same expressions, so the same bits)."""
    cov_ref = np.asarray(cov_ref, np.float64)
    d = int(du)
    gain = cov_ref[:d, d:] @ np.linalg.inv(cov_ref[d:, d:])
    return cov_ref[:d, :d] - gain @ cov_ref[d:, :d]


def lg_kalman_tables(tab: dict, pm_tab: dict, cov0=None) -> dict:
    """Float64 tables of the fused Kalman sampler (include/fbsmi.h, fbsmi_kf_model), no device needed.

    tab: lg_tables(...); pm_tab: lg_pmcmc_tables(...) of the terminal moments.  The initial covariance is
    ``pm_tab["cov_"]`` when present, else ``cov0``, else rebuilt from the float32 ``chol`` (exact to float32 only: pass
    ``cov0 = initial_cov(cov_ref, du)`` for the float64 one)."""
    du, dv, dt = int(tab["du"]), int(tab["dv"]), float(tab["dt"])
    G, g, sd = (np.asarray(tab[k], np.float64) for k in ("G", "g", "sd"))
    T, D = G.shape[0], du + dv
    if cov0 is None:
        cov0 = pm_tab.get("cov_")
    if cov0 is None:
        L0 = np.asarray(pm_tab["chol"], np.float64)
        cov0 = L0 @ L0.T
    Sig = np.array(cov0, np.float64)
    H, e = np.zeros((T, dv, D)), np.zeros((T, dv))
    Pm, c = np.zeros((T, du, D)), np.zeros((T, du))
    AK, W, lconst = np.zeros((T, du, dv)), np.zeros((T, dv, dv)), np.zeros(T)
    eye_u, eye_v = np.eye(du), np.eye(dv)
    for k in range(T):
        M = np.eye(D) + dt * G[k]
        A, Cm = M[:du, :du], M[du:, :du]
        q = sd[k] ** 2
        S = Cm @ Sig @ Cm.T + q * eye_v
        S = 0.5 * (S + S.T)
        K = np.linalg.solve(S, Cm @ Sig).T                      # Sigma C^T inv(S)
        Sp = Sig - K @ S @ K.T
        Ls = np.linalg.cholesky(S)
        H[k], e[k] = M[du:], dt * g[k, du:]
        Pm[k], c[k] = M[:du], dt * g[k, :du]
        AK[k] = A @ K
        W[k] = np.linalg.solve(Ls, eye_v)
        lconst[k] = -0.5 * (2.0 * np.log(np.diag(Ls)).sum() + dv * np.log(2.0 * np.pi))
        Sig = A @ Sp @ A.T + q * eye_u
        Sig = 0.5 * (Sig + Sig.T)
    return dict(du=du, dv=dv, T=T, H=H, e=e, Pm=Pm, c=c, AK=AK, W=W, lconst=lconst, cov_T=Sig,
                Lt=np.ascontiguousarray(np.linalg.cholesky(Sig).T), cov_0=np.array(cov0, np.float64),
                m_u=np.asarray(pm_tab["m_u"], np.float64), m_v=np.asarray(pm_tab["m_v"], np.float64),
                gain=np.asarray(pm_tab["gain"], np.float64))


def kalman_filter_np(kt: dict, vs, dtype=np.float64):
    """The mean recursion and the log-likelihood on lg_kalman_tables' output for one observation path vs (T+1, dv), in
    `dtype` with numpy's product order -> (m_T (du), loglik).  The float64 yardstick; float32 shows the innovation form's
    rounding."""
    f = lambda a: np.asarray(a, dtype)
    vs = f(vs)
    m = f(kt["m_u"] + kt["gain"] @ (np.asarray(vs[0], np.float64) - kt["m_v"]))
    H, e, Pm, c, AK, W, lc = (f(kt[k]) for k in ("H", "e", "Pm", "c", "AK", "W", "lconst"))
    ll = dtype(0.0)
    for k in range(kt["T"]):
        z = np.concatenate([m, vs[k]])
        r = vs[k + 1] - (H[k] @ z + e[k])
        m = (Pm[k] @ z + c[k]) + AK[k] @ r
        qv = W[k] @ r
        ll = ll + (dtype(-0.5) * (qv @ qv) + lc[k])
    return m, ll


def plan_kalman_chunks(nkeys: int, T: int, dv: int, bound: int = KF_PATH_ELEMS, max_samples: int = KF_MAX_SAMPLES):
    """[(start, stop), ..] covering range(nkeys) in order, each with (stop - start) * (T + 1) * dv <= bound elements (the
    observation paths of one call) and at most max_samples samples; None when one sample alone exceeds the bound."""
    per = (int(T) + 1) * int(dv)
    if per > bound:
        return None
    step = max(1, min(int(max_samples), bound // per))
    return [(s, min(s + step, int(nkeys))) for s in range(0, int(nkeys), step)]


_ARRAYS = ("H", "e", "Pm", "c", "AK", "W", "lconst", "Lt")


def kalman_model(bridge: LinearGaussianBridge):
    """The bridge's Kalman tables: host float64 (``tables64``), host float32 (``host``) and the device copies as an
    fbsmi_kf_model struct, built once and cached on the bridge."""
    if type(bridge) is not LinearGaussianBridge or getattr(bridge, "em_struct", None) is not None or bridge.sde is None:
        raise NotImplementedError("the Kalman conditional sampler is built for LinearGaussianBridge (an exact forward "
                                  "transition and terminal moments); GaussianSBBridge is out of scope")

    def make():
        pm = bridge.pmcmc_tables_host(None)
        kt = lg_kalman_tables(bridge.tables64, pm, initial_cov(bridge.terminal_moments()[1], bridge.du))
        host = {k: np.ascontiguousarray(np.asarray(kt[k], np.float32)) for k in _ARRAYS}
        dev = {k: torch.from_numpy(v).to(bridge.device) for k, v in host.items()}
        for k in ("m_u", "m_v", "gain"):
            dev[k] = torch.from_numpy(np.ascontiguousarray(kt[k])).to(bridge.device)
        st = _lib.KFModelStruct(bridge.du, bridge.dv, bridge.T, *(dev[k].data_ptr() for k in _ARRAYS),
                                bridge.dev["F"].data_ptr(), bridge.dev["sqQ"].data_ptr(),
                                dev["m_u"].data_ptr(), dev["m_v"].data_ptr(), dev["gain"].data_ptr())
        st._keep, st.host, st.tables64 = dev, host, kt
        return st

    return bridge._cached(("kalman_model",), make)


class LGKalman(_LGHandle):
    """Owns one fbsmi_kf handle: up to `nsamples` independent conditional samples per call -- observation paths, the exact
    filter's mean recursion and log-likelihood, the draw -- in two plain launches, nothing on the host inside a call.  A
    call with fewer keys or paths than `nsamples` (a ragged last batch) runs on the bridge's handle of that size."""

    _DESTROY = "fbsmi_kf_destroy"

    def __init__(self, model: LinearGaussianBridge, nsamples=1):
        self.struct = kalman_model(model)
        self.model, self.C = model, int(nsamples)
        self._last = self
        h = C.c_void_p()   # sizes the engine does not take are refused by the library, with its message
        with torch.cuda.device(model.device):
            _lib.call("fbsmi_kf_create", C.byref(self.struct), self.C, C.byref(h))
        self.h = h

    @property
    def cov_T(self):
        """The filtering covariance (du, du), float64: the same for every observation path."""
        return self.struct.tables64["cov_T"]

    def _route(self, B):
        if not 1 <= B <= self.C:
            raise ValueError(f"{B} samples for a handle of {self.C}")
        self._last = self if B == self.C else self.model.kalman_handle(B)
        return self._last

    def sample(self, keys, y0, return_moments=False):
        """keys (B', 2), or (2,) for one sample, y0 (dv,) -> samples (B', du) [, means (B', du), loglik (B')]."""
        m = self.model
        k = np.asarray(keys.detach().cpu() if isinstance(keys, torch.Tensor) else keys).astype(np.uint32).reshape(-1, 2)
        B = k.shape[0]
        h = self._route(B)
        if h is not self:
            return h.sample(k, y0, return_moments)
        kt = self._key_t(k, B)
        y0t = self._dev(y0, torch.float32, (m.dv,))
        out = torch.empty((B, m.du), dtype=torch.float32, device=m.device)
        means = torch.empty((B, m.du), dtype=torch.float32, device=m.device) if return_moments else None
        ll = torch.empty(B, dtype=torch.float32, device=m.device) if return_moments else None
        with torch.cuda.device(m.device):
            _lib.call("fbsmi_kf_sample", self.h, kt.data_ptr(), y0t.data_ptr(), out.data_ptr(),
                      means.data_ptr() if return_moments else None, ll.data_ptr() if return_moments else None, ops._stream())
        return (out, means, ll) if return_moments else out

    def filter(self, vs):
        """vs (B', T+1, dv), or (T+1, dv) for one path -> (means (B', du), loglik (B')); nothing is drawn."""
        m = self.model
        vst = self._dev(vs, torch.float32, (-1, m.T + 1, m.dv))
        B = vst.shape[0]
        h = self._route(B)
        if h is not self:
            return h.filter(vst)
        means = torch.empty((B, m.du), dtype=torch.float32, device=m.device)
        ll = torch.empty(B, dtype=torch.float32, device=m.device)
        with torch.cuda.device(m.device):
            _lib.call("fbsmi_kf_filter", self.h, vst.data_ptr(), means.data_ptr(), ll.data_ptr(), ops._stream())
        return means, ll

    def views(self) -> dict:
        """State of the last call (copies): vs (B, T+1, dv) the observation paths of the handle's last ``sample``, m_
        (B, du) the initial means of its last call."""
        h, m = self._last, self.model
        out = {}
        for name, which, shape in (("vs", 0, (h.C, m.T + 1, m.dv)), ("m_", 1, (h.C, m.du))):
            t = torch.empty(shape, dtype=torch.float32, device=m.device)
            _lib.call("fbsmi_kf_view", h.h, which, t.data_ptr(), None, ops._stream())
            out[name] = t
        return out


def kalman_conditional_sampler(keys, y0, bridge, return_moments=False, _bound=KF_PATH_ELEMS):
    """The Kalman-filter conditional sampler for every key of `keys` (B, 2) [or (2,)] on a LinearGaussianBridge:
    -> samples (B, du) [, filtering means (B, du), exact log-likelihoods log p(v_1..v_T | v_0) (B)].  Each sample depends
    on its own key only; the batch runs in chunks that keep one call's B * (T + 1) * dv within `_bound` elements."""
    if type(bridge) is not LinearGaussianBridge:
        raise NotImplementedError("kalman_conditional_sampler takes a LinearGaussianBridge; GaussianSBBridge is out of scope")
    k = np.asarray(keys.detach().cpu() if isinstance(keys, torch.Tensor) else keys).astype(np.uint32).reshape(-1, 2)
    chunks = plan_kalman_chunks(k.shape[0], bridge.T, bridge.dv, _bound)
    if chunks is None:
        raise NotImplementedError("one observation path alone exceeds the bound of a fused call")
    outs = [bridge.kalman_handle(b - a).sample(k[a:b], y0, return_moments=True) for a, b in chunks]
    samples, means, ll = (torch.cat([o[i] for o in outs]) for i in range(3))
    return (samples, means, ll) if return_moments else samples
