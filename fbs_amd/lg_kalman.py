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

The smoothing law ``p(u_0..u_T | v_0..v_T)`` of the same model is Gaussian too: ``lg_smoother_tables`` adds the backward
gains and factors, ``kalman_smoother_np`` is the float64 Rauch-Tung-Striebel recursion and backward sampler, and
``LGKalmanSmoother`` / ``kalman_path_sampler`` own the fused, batched engine (fbsmi_kfs_*): exact whole-path draws and
smoothed means, the yardstick of the particle engines that produce paths.

The Gaussian Schrodinger-bridge toy has the same engines under names of its own (fbs_amd/gaussian_sb.py: ``sb_kalman_model``,
``SBKalman``, ``SBKalmanSmoother``, ``sb_kalman_conditional_sampler``, ``sb_kalman_path_sampler``); the entry points here
keep refusing a GaussianSBBridge.
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


def lg_smoother_tables(tab: dict, kt: dict) -> dict:
    """Float64 tables of the fused Kalman smoother and path sampler (include/fbsmi.h, fbsmi_kfs_model), no device needed.

    tab: lg_tables(...); kt: lg_kalman_tables(...) of the same model (its ``cov_0`` starts the recursion, which is repeated
    here in the same expressions).  Per step k, with Sigma_k the predicted and Sigma_k+ the updated covariance:
    K[k] = Sigma_k C^T inv(S), J[k] = Sigma_k+ A^T inv(Sigma_{k+1}), Lb[k] the lower Cholesky factor of
    Sigma_k+ - J Sigma_{k+1} J^T; cov_s (T+1, du, du) the smoothed covariances and cross[k] = J[k] cov_s[k+1] the lag-one
    cross-covariances cov(u_k, u_{k+1} | v_0..v_T)."""
    du, dv, dt = int(tab["du"]), int(tab["dv"]), float(tab["dt"])
    G, sd = (np.asarray(tab[k], np.float64) for k in ("G", "sd"))
    T, D = G.shape[0], du + dv
    Sig = np.array(kt["cov_0"], np.float64)
    K, J, Lb = np.zeros((T, du, dv)), np.zeros((T, du, du)), np.zeros((T, du, du))
    Sp_all, Sn_all = np.zeros((T, du, du)), np.zeros((T, du, du))
    eye_u, eye_v = np.eye(du), np.eye(dv)
    for k in range(T):
        M = np.eye(D) + dt * G[k]
        A, Cm = M[:du, :du], M[du:, :du]
        q = sd[k] ** 2
        S = Cm @ Sig @ Cm.T + q * eye_v
        S = 0.5 * (S + S.T)
        K[k] = np.linalg.solve(S, Cm @ Sig).T
        Sp = Sig - K[k] @ S @ K[k].T
        Sig = A @ Sp @ A.T + q * eye_u
        Sig = 0.5 * (Sig + Sig.T)
        J[k] = np.linalg.solve(Sig, A @ Sp).T                   # Sigma+ A^T inv(Sigma_{k+1})
        R = Sp - J[k] @ Sig @ J[k].T
        Lb[k] = np.linalg.cholesky(0.5 * (R + R.T))
        Sp_all[k], Sn_all[k] = Sp, Sig
    cov_s, cross = np.zeros((T + 1, du, du)), np.zeros((T, du, du))
    cov_s[T] = kt["cov_T"]
    for k in range(T - 1, -1, -1):
        cov_s[k] = Sp_all[k] + J[k] @ (cov_s[k + 1] - Sn_all[k]) @ J[k].T
        cov_s[k] = 0.5 * (cov_s[k] + cov_s[k].T)
        cross[k] = J[k] @ cov_s[k + 1]
    return dict(du=du, dv=dv, T=T, K=K, J=J, Lb=Lb, cov_s=cov_s, cross=cross)


def kalman_smoother_np(kt: dict, st: dict, vs, dtype=np.float64, noise=None):
    """The forward recursion of kalman_filter_np keeping every m_k and r_k, then the backward recursion
    u_k = m_k + K_k r_k + J_k (u_{k+1} - m_{k+1}) + Lb_k xi_k on lg_smoother_tables' output, for one observation path vs
    (T+1, dv), in `dtype` with numpy's product order -> (path (T+1, du), m (T+1, du), r (T, dv), loglik).  noise None: the
    smoothed means (nothing drawn); noise (zT (du), xi (T, du)): the draw u_T = m_T + zT @ Lt and its backward pass."""
    f = lambda a: np.asarray(a, dtype)
    vs = f(vs)
    T, du = kt["T"], kt["du"]
    H, e, Pm, c, AK, W, lc = (f(kt[k]) for k in ("H", "e", "Pm", "c", "AK", "W", "lconst"))
    K, J, Lb = (f(st[k]) for k in ("K", "J", "Lb"))
    ms, rs = np.zeros((T + 1, du), dtype), np.zeros((T, kt["dv"]), dtype)
    ms[0] = f(kt["m_u"] + kt["gain"] @ (np.asarray(vs[0], np.float64) - kt["m_v"]))
    ll = dtype(0.0)
    for k in range(T):
        z = np.concatenate([ms[k], vs[k]])
        rs[k] = vs[k + 1] - (H[k] @ z + e[k])
        ms[k + 1] = (Pm[k] @ z + c[k]) + AK[k] @ rs[k]
        qv = W[k] @ rs[k]
        ll = ll + (dtype(-0.5) * (qv @ qv) + lc[k])
    path = np.zeros((T + 1, du), dtype)
    delta = np.zeros(du, dtype) if noise is None else f(noise[0]) @ f(kt["Lt"])
    path[T] = ms[T] + delta
    for k in range(T - 1, -1, -1):
        delta = K[k] @ rs[k] + J[k] @ delta
        if noise is not None:
            delta = delta + Lb[k] @ f(noise[1][k])
        path[k] = ms[k] + delta
    return path, ms, rs, ll


def plan_kalman_chunks(nkeys: int, T: int, dv: int, bound: int = KF_PATH_ELEMS, max_samples: int = KF_MAX_SAMPLES):
    """[(start, stop), ..] covering range(nkeys) in order, each with (stop - start) * (T + 1) * dv <= bound elements (the
    observation paths of one call) and at most max_samples samples; None when one sample alone exceeds the bound."""
    per = (int(T) + 1) * int(dv)
    if per > bound:
        return None
    step = max(1, min(int(max_samples), bound // per))
    return [(s, min(s + step, int(nkeys))) for s in range(0, int(nkeys), step)]


_ARRAYS = ("H", "e", "Pm", "c", "AK", "W", "lconst", "Lt")


def _kf_struct(bridge):
    """lg_kalman_tables of a bridge's per-step tables and terminal moments as an fbsmi_kf_model struct with its host
    float64 (``tables64``) and float32 (``host``) copies."""
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


def kalman_model(bridge: LinearGaussianBridge):
    """The bridge's Kalman tables: host float64 (``tables64``), host float32 (``host``) and the device copies as an
    fbsmi_kf_model struct, built once and cached on the bridge."""
    if type(bridge) is not LinearGaussianBridge or getattr(bridge, "em_struct", None) is not None or bridge.sde is None:
        raise NotImplementedError("the Kalman conditional sampler is built for LinearGaussianBridge (an exact forward "
                                  "transition and terminal moments); GaussianSBBridge is out of scope (its engines are "
                                  "fbs_amd.gaussian_sb's sb_kalman_model, SBKalman, SBKalmanSmoother)")
    return bridge._cached(("kalman_model",), lambda: _kf_struct(bridge))


class LGKalman(_LGHandle):
    """Owns one fbsmi_kf handle: up to `nsamples` independent conditional samples per call -- observation paths, the exact
    filter's mean recursion and log-likelihood, the draw -- in two plain launches, nothing on the host inside a call.  A
    call with fewer keys or paths than `nsamples` (a ragged last batch) runs on the bridge's handle of that size."""

    _DESTROY = "fbsmi_kf_destroy"

    def __init__(self, model: LinearGaussianBridge, nsamples=1):
        self.struct = self._struct_of(model)
        self.model, self.C = model, int(nsamples)
        self._last = self
        h = C.c_void_p()   # sizes the engine does not take are refused by the library, with its message
        with torch.cuda.device(model.device):
            _lib.call("fbsmi_kf_create", C.byref(self.struct), self.C, C.byref(h))
        self.h = h

    def _struct_of(self, model):
        """The model's fbsmi_kf_model struct."""
        return kalman_model(model)

    def _of_size(self, B):
        """The model's cached handle of this one's kind for B samples per call."""
        return self.model.kalman_handle(B)

    @property
    def cov_T(self):
        """The filtering covariance (du, du), float64: the same for every observation path."""
        return self.struct.tables64["cov_T"]

    def _route(self, B):
        if not 1 <= B <= self.C:
            raise ValueError(f"{B} samples for a handle of {self.C}")
        self._last = self if B == self.C else self._of_size(B)
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
        raise NotImplementedError("kalman_conditional_sampler takes a LinearGaussianBridge; GaussianSBBridge is out of scope "
                                  "(sb_kalman_conditional_sampler serves it)")
    return _conditional_chunks(keys, y0, bridge, bridge.kalman_handle, return_moments, _bound)


def _conditional_chunks(keys, y0, bridge, handle_of, return_moments, bound):
    """The chunked batch of a conditional sampler: handle_of(B) is the bridge's handle for B samples per call."""
    k = np.asarray(keys.detach().cpu() if isinstance(keys, torch.Tensor) else keys).astype(np.uint32).reshape(-1, 2)
    chunks = plan_kalman_chunks(k.shape[0], bridge.T, bridge.dv, bound)
    if chunks is None:
        raise NotImplementedError("one observation path alone exceeds the bound of a fused call")
    outs = [handle_of(b - a).sample(k[a:b], y0, return_moments=True) for a, b in chunks]
    samples, means, ll = (torch.cat([o[i] for o in outs]) for i in range(3))
    return (samples, means, ll) if return_moments else samples


# ---- the smoother and path sampler (include/fbsmi.h, fbsmi_kfs_*) --------------------------------------------------------
_S_ARRAYS = ("K", "J", "Lb")


def plan_smoother_chunks(nkeys: int, T: int, du: int, dv: int, bound: int = KF_PATH_ELEMS,
                         max_samples: int = KF_MAX_SAMPLES):
    """plan_kalman_chunks for the path engines: every per-call buffer -- vs (B, T+1, dv), m_k and paths (B, T+1, du), r_k
    (B, T, dv) -- stays within `bound` elements, a call within `max_samples` samples."""
    return plan_kalman_chunks(nkeys, T, max(int(du), int(dv)), bound, max_samples)


def kalman_smoother_model(bridge: LinearGaussianBridge):
    """The bridge's smoother tables: host float64 (``tables64``, with cov_s and cross), host float32 (``host``) and the
    device copies as an fbsmi_kfs_model struct on top of kalman_model's, built once and cached on the bridge."""
    kf = kalman_model(bridge)
    return bridge._cached(("kalman_smoother_model",), lambda: _kfs_struct(bridge, kf))


def _kfs_struct(bridge, kf):
    """lg_smoother_tables of a bridge on top of its fbsmi_kf_model struct `kf`, as an fbsmi_kfs_model struct."""
    st64 = lg_smoother_tables(bridge.tables64, kf.tables64)
    host = {k: np.ascontiguousarray(np.asarray(st64[k], np.float32)) for k in _S_ARRAYS}
    dev = {k: torch.from_numpy(v).to(bridge.device) for k, v in host.items()}
    st = _lib.KFSModelStruct(C.pointer(kf), *(dev[k].data_ptr() for k in _S_ARRAYS))
    st._keep, st.host, st.tables64, st.kf_struct = dev, host, st64, kf
    return st


class LGKalmanSmoother(_LGHandle):
    """Owns one fbsmi_kfs handle: up to `nsamples` independent whole-path draws from p(u_0..u_T | v_0..v_T), or its means,
    per call -- the front, the exact filter's recursion keeping every m_k and r_k, the backward pass -- in three plain
    launches, nothing on the host inside a call.  A call with fewer keys or paths than `nsamples` runs on the bridge's
    handle of that size."""

    _DESTROY = "fbsmi_kfs_destroy"

    def __init__(self, model: LinearGaussianBridge, nsamples=1):
        self.struct = self._struct_of(model)
        self.model, self.C = model, int(nsamples)
        self._last = self
        h = C.c_void_p()
        with torch.cuda.device(model.device):
            _lib.call("fbsmi_kfs_create", C.byref(self.struct), self.C, C.byref(h))
        self.h = h

    def _struct_of(self, model):
        """The model's fbsmi_kfs_model struct."""
        return kalman_smoother_model(model)

    def _of_size(self, B):
        """The model's cached handle of this one's kind for B paths per call."""
        return self.model.kalman_smoother_handle(B)

    @property
    def cov_s(self):
        """The smoothed covariances (T+1, du, du), float64: the same for every observation path."""
        return self.struct.tables64["cov_s"]

    def _route(self, B):
        if not 1 <= B <= self.C:
            raise ValueError(f"{B} samples for a handle of {self.C}")
        self._last = self if B == self.C else self._of_size(B)
        return self._last

    def _out(self, B, loglik):
        m = self.model
        return (torch.empty((B, m.T + 1, m.du), dtype=torch.float32, device=m.device),
                torch.empty(B, dtype=torch.float32, device=m.device) if loglik else None)

    @staticmethod
    def _keys_np(keys):
        return np.asarray(keys.detach().cpu() if isinstance(keys, torch.Tensor) else keys).astype(np.uint32).reshape(-1, 2)

    def sample(self, keys, y0, return_loglik=False):
        """keys (B', 2), or (2,) for one sample, y0 (dv,) -> paths (B', T+1, du) [, loglik (B')]; paths[:, T] is
        LGKalman.sample's draw on the same keys."""
        m = self.model
        k = self._keys_np(keys)
        B = k.shape[0]
        h = self._route(B)
        if h is not self:
            return h.sample(k, y0, return_loglik)
        kt = self._key_t(k, B)
        y0t = self._dev(y0, torch.float32, (m.dv,))
        paths, ll = self._out(B, return_loglik)
        with torch.cuda.device(m.device):
            _lib.call("fbsmi_kfs_sample", self.h, kt.data_ptr(), y0t.data_ptr(), paths.data_ptr(),
                      ll.data_ptr() if return_loglik else None, ops._stream())
        return (paths, ll) if return_loglik else paths

    def sample_on(self, keys, vs, return_loglik=False):
        """The same draw on the caller's observation paths vs (B', T+1, dv) [or (T+1, dv) with one key]."""
        m = self.model
        k = self._keys_np(keys)
        B = k.shape[0]
        vst = self._dev(vs, torch.float32, (B, m.T + 1, m.dv))
        h = self._route(B)
        if h is not self:
            return h.sample_on(k, vst, return_loglik)
        kt = self._key_t(k, B)
        paths, ll = self._out(B, return_loglik)
        with torch.cuda.device(m.device):
            _lib.call("fbsmi_kfs_sample_on", self.h, kt.data_ptr(), vst.data_ptr(), paths.data_ptr(),
                      ll.data_ptr() if return_loglik else None, ops._stream())
        return (paths, ll) if return_loglik else paths

    def smooth(self, vs, return_loglik=False):
        """vs (B', T+1, dv), or (T+1, dv) for one path -> the smoothed means (B', T+1, du) [, loglik (B')]."""
        m = self.model
        vst = self._dev(vs, torch.float32, (-1, m.T + 1, m.dv))
        B = vst.shape[0]
        h = self._route(B)
        if h is not self:
            return h.smooth(vst, return_loglik)
        sm, ll = self._out(B, return_loglik)
        with torch.cuda.device(m.device):
            _lib.call("fbsmi_kfs_smooth", self.h, vst.data_ptr(), sm.data_ptr(), ll.data_ptr() if return_loglik else None,
                      ops._stream())
        return (sm, ll) if return_loglik else sm

    def views(self) -> dict:
        """State of the last call (copies): vs (B, T+1, dv) the observation paths of the handle's last ``sample``, m
        (B, T+1, du) the filter means and r (B, T, dv) the innovations of its last call."""
        h, m = self._last, self.model
        out = {}
        for name, which, shape in (("vs", 0, (h.C, m.T + 1, m.dv)), ("m", 1, (h.C, m.T + 1, m.du)), ("r", 2, (h.C, m.T, m.dv))):
            t = torch.empty(shape, dtype=torch.float32, device=m.device)
            _lib.call("fbsmi_kfs_view", h.h, which, t.data_ptr(), None, ops._stream())
            out[name] = t
        return out


def kalman_path_sampler(keys, y0, bridge, return_moments=False, _bound=KF_PATH_ELEMS):
    """The forward-filter / backward-sampler for every key of `keys` (B, 2) [or (2,)] on a LinearGaussianBridge: exact draws
    from p(u_0..u_T | v_0..v_T) on each key's own observation path -> paths (B, T+1, du) [, smoothed means (B, T+1, du),
    exact log-likelihoods (B)].  The batch runs in chunks that keep every per-call buffer within `_bound` elements."""
    if type(bridge) is not LinearGaussianBridge:
        raise NotImplementedError("kalman_path_sampler takes a LinearGaussianBridge; GaussianSBBridge is out of scope "
                                  "(sb_kalman_path_sampler serves it)")
    return _path_chunks(keys, y0, bridge, bridge.kalman_smoother_handle, return_moments, _bound)


def _path_chunks(keys, y0, bridge, handle_of, return_moments, bound):
    """The chunked batch of a path sampler: handle_of(B) is the bridge's smoother handle for B paths per call."""
    k = np.asarray(keys.detach().cpu() if isinstance(keys, torch.Tensor) else keys).astype(np.uint32).reshape(-1, 2)
    chunks = plan_smoother_chunks(k.shape[0], bridge.T, bridge.du, bridge.dv, bound)
    if chunks is None:
        raise NotImplementedError("one path alone exceeds the bound of a fused call")
    paths, means, lls = [], [], []
    for a, b in chunks:
        h = handle_of(b - a)
        p, ll = h.sample(k[a:b], y0, return_loglik=True)
        paths.append(p)
        lls.append(ll)
        if return_moments:
            means.append(h.smooth(h.views()["vs"]))
    paths, ll = torch.cat(paths), torch.cat(lls)
    return (paths, torch.cat(means), ll) if return_moments else paths
