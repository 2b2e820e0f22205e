"""The Gaussian Schrodinger-bridge (SB) toy of experiments/sb/gibbs.py and sb/filter.py as a model descriptor.

The forward process is the closed-form SB between N(mean0, cov0) and N(mean1, cov1) with a Brownian reference of
dispersion ``sig`` (``fbs_amd.sdes.make_gaussian_bw_sb``).  Its drift ``M(t) z + c(t)`` is affine but, unlike the
separable linear SDEs of ``LinearGaussianBridge``, a full matrix and time-dependent; the reference simulates it by
Euler-Maruyama with ``nsub`` sub-steps per interval (sb/gibbs.py:137-139).  The reverse drift is affine as well,

    -drift(z, 1 - t) + sig^2 score(z, 1 - t) = (-M - sig^2 P) z + (-c + sig^2 P m)     (P = cov_s^{-1}, m = mean_s),

so the CSMC part of a sweep and the particle filters run on the fused engine's affine tables unchanged; the forward
paths take the Euler-Maruyama kernel (include/fbsmi.h, fbsmi_em_forward) on the tables of ``sb_tables``.

The discretised reverse model is linear-Gaussian like the analytic one, so its filtering and smoothing laws and its marginal
likelihood are closed-form on ``lg_kalman_tables`` of the same G, g, sd, dt: ``sb_kalman_model`` / ``SBKalman`` /
``sb_kalman_conditional_sampler`` and ``sb_kalman_smoother_model`` / ``SBKalmanSmoother`` / ``sb_kalman_path_sampler`` are the
exact yardsticks of the SB filter sampler, on the observation paths that sampler draws from the same keys
(include/fbsmi.h, fbsmi_kf_set_em_forward).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .lg_kalman import (KF_PATH_ELEMS, LGKalman, LGKalmanSmoother, _conditional_chunks, _kf_struct, _kfs_struct,
                        _path_chunks)
from .linear_gaussian import LGFilter, LGFilterSampler, LinearGaussianBridge
from .sdes.linear import make_gaussian_bw_sb


def sb_tables(mean0, cov0, mean1, cov1, ts, du: int, sig: float = 1.0, nsub: int = 10) -> dict:
    """Float64 tables of the Gaussian SB on the grid ts (T + 1 points).

    Reverse step k (t_prev = ts[k], bridge time s = ts[-1] - ts[k]): G, g, sd = sqrt(dt) sig, lognorm = log(2 pi sd^2)
    with dt = (ts[-1] - ts[0]) / T.  Forward sub-step r = k*nsub + j at tau = linspace(ts[k], ts[k+1] - h, nsub)[j],
    h = |ts[k+1] - ts[k]| / nsub: M[r], c[r] (drift = M z + c), s[r] = sig sqrt(h); ddt[k] = h.  F / sqQ are zero
    placeholders of the model struct (the Euler-Maruyama forward process never reads them)."""
    mean0 = np.asarray(mean0, np.float64).reshape(-1)
    ts = np.asarray(ts, np.float64).reshape(-1)
    nsub = int(nsub)
    if nsub < 1:
        raise ValueError("nsub must be at least 1")
    D, T = mean0.size, ts.size - 1
    marginal_mean, marginal_cov, drift = make_gaussian_bw_sb(mean0, cov0, mean1, cov1, sig=sig)
    affine = drift.affine
    Tend = ts[-1]
    dt = float((Tend - ts[0]) / T)
    sig2 = float(sig) ** 2
    G, g = np.zeros((T, D, D)), np.zeros((T, D))
    for k in range(T):
        s_ = Tend - ts[k]
        Ms, cs = affine(s_)
        P = np.linalg.inv(marginal_cov(s_))
        G[k] = -Ms - sig2 * P
        g[k] = -cs + sig2 * (P @ marginal_mean(s_))
    sd = np.full(T, np.sqrt(dt) * float(sig))
    M, c = np.zeros((T * nsub, D, D)), np.zeros((T * nsub, D))
    s, ddt = np.zeros(T * nsub), np.zeros(T)
    for k in range(T):
        t, t_next = float(ts[k]), float(ts[k + 1])
        h = abs(t_next - t) / nsub                      # simulators.py:53-58 (euler_maruyama's sub-grid)
        ddt[k] = h
        for j, tau in enumerate(np.linspace(t, t_next - h, nsub)):
            M[k * nsub + j], c[k * nsub + j] = affine(tau)
            s[k * nsub + j] = float(sig) * np.sqrt(h)
    return dict(du=int(du), dv=int(D - du), dt=dt, G=G, g=g, sd=sd, lognorm=np.log(2 * np.pi * sd ** 2), F=np.zeros(T),
                sqQ=np.zeros(T), nsub=nsub, M=M, c=c, ddt=ddt, s=s)


class GaussianSBBridge(LinearGaussianBridge):
    """The SB toy's model: the closures of experiments/sb/gibbs.py:113-139 as HIP kernels on the tables of sb_tables, and
    the fused sweep / filter engine of LinearGaussianBridge with the Euler-Maruyama forward process.

    ``fbs_amd.samplers.gibbs_kernel`` (with ``sde=None``, as sb/gibbs.py:171 passes it), ``bootstrap_filter`` and
    ``pmcmc_filter_step`` recognise these closures and take the fused engine."""

    def __init__(self, mean0, cov0, mean1, cov1, ts, du: int, sig: float = 1.0, nsub: int = 10, device=None):
        self.sde = None
        self.m0 = np.asarray(mean0, np.float64).reshape(-1)
        self.cov0 = np.asarray(cov0, np.float64)
        self.mean1 = np.asarray(mean1, np.float64).reshape(-1)
        self.cov1 = np.asarray(cov1, np.float64)
        self.sig, self.nsub = float(sig), int(nsub)
        tab = sb_tables(self.m0, self.cov0, self.mean1, self.cov1, ts, du, sig, nsub)
        self._setup(tab, ts, device)
        f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
        self.em_host = {k: f32(tab[k]) for k in ("M", "c", "ddt", "s")}
        self.em_dev = {k: torch.from_numpy(v).to(self.device) for k, v in self.em_host.items()}
        self.em_struct = _lib.EMForwardStruct(self.nsub, *(self.em_dev[k].data_ptr() for k in ("M", "c", "ddt", "s")))

    def _fwd_sampler(self, key, x0, y0):  # sb/gibbs.py:137-139: euler_maruyama(key, concat(x0, y0), ts, drift, 1, 10)
        z0 = torch.cat([self._t(x0).reshape(-1), self._t(y0).reshape(-1)]).contiguous()
        keys = ops.split(key, self.T)
        keys_t = torch.from_numpy(np.ascontiguousarray(keys, np.uint32).view(np.int32).copy()).to(self.device)
        out = torch.empty((self.T + 1, self.D), dtype=torch.float32, device=self.device)
        _lib.call("fbsmi_lg_em_path", keys_t.data_ptr(), C.byref(self.em_struct), z0.data_ptr(), self.T, self.D,
                  out.data_ptr(), ops._stream())
        return out

    def _fwd_ys_sampler(self, key, y0):
        raise NotImplementedError("the Schrodinger bridge's forward process is not separable: simulate (x0, y0) with "
                                  "fwd_sampler and unpack the y part")

    def terminal_moments(self):
        """The bridge's terminal marginal N(mean1, cov1): ref_sampler draws u0 | v0 from it (sb/gibbs.py:131-134)."""
        return self.mean1, self.cov1

    # -- fused bootstrap-filter conditional sampler (experiments/sb/filter.py) ----------------------
    def fused_sb_filter_sampler_supported(self, nparticles: int, nsamples: int = 1) -> bool:
        """What fbsmi_lg_fsamp_create_em accepts: an Euler-Maruyama forward process of du + dv <= 256 coordinates (one
        workgroup runs a joint path), at most 65535 samples per call and the fused filter's sizes.  Touches no device."""
        return (getattr(self, "em_struct", None) is not None and self.du + self.dv <= 256 and 1 <= int(nsamples) <= 65535
                and int(nparticles) >= 1 and self.fused_filter_supported(nparticles))

    def sb_filter_sampler_handle(self, nparticles: int, resampling: str = "stratified", nsamples: int = 1, x0_prior=None):
        """The fused conditional sampler of sb/filter.py:149-161 for `nsamples` samples per call.  x0_prior = (mean (du),
        chol_lower (du, du)): the forward path starts from x0 = mean + normal @ chol_lower ('proper'); None: from
        x0 ~ N(0, I) ('heuristic').  Cached on the bridge by the sizes and the prior's float32 bytes."""
        prior = None
        if x0_prior is not None:
            prior = (np.ascontiguousarray(np.asarray(x0_prior[0], np.float32).reshape(self.du)),
                     np.ascontiguousarray(np.asarray(x0_prior[1], np.float32).reshape(self.du, self.du)))
        keyt = ("sb_fsamp", int(nparticles), resampling, int(nsamples),
                None if prior is None else (prior[0].tobytes(), prior[1].tobytes()))
        return self._cached(keyt, lambda: SBFilterSampler(self, int(nparticles), resampling, int(nsamples), prior))

    # -- exact Kalman sampler and smoother (fbs_amd/lg_kalman.py on this model's tables) ----------------
    def _prior32(self, x0_prior):
        """x0_prior as contiguous float32 (mean (du), chol_lower (du, du)) and its part of a cache key."""
        if x0_prior is None:
            return None, None
        prior = (np.ascontiguousarray(np.asarray(x0_prior[0], np.float32).reshape(self.du)),
                 np.ascontiguousarray(np.asarray(x0_prior[1], np.float32).reshape(self.du, self.du)))
        return prior, (prior[0].tobytes(), prior[1].tobytes())

    def sb_kalman_handle(self, nsamples: int = 1, x0_prior=None):
        """The fused Kalman-filter conditional sampler (SBKalman) for `nsamples` samples per call; x0_prior as in
        sb_filter_sampler_handle.  Cached on the bridge by the size and the prior's float32 bytes."""
        prior, pk = self._prior32(x0_prior)
        return self._cached(("sb_kalman", int(nsamples), pk), lambda: SBKalman(self, int(nsamples), prior))

    def sb_kalman_smoother_handle(self, nsamples: int = 1, x0_prior=None):
        """The fused Kalman smoother and path sampler (SBKalmanSmoother) for `nsamples` paths per call, cached likewise."""
        prior, pk = self._prior32(x0_prior)
        return self._cached(("sb_kalman_smoother", int(nsamples), pk), lambda: SBKalmanSmoother(self, int(nsamples), prior))


class SBFilterSampler(LGFilterSampler):
    """Owns one fbsmi_lg_fsamp handle made by fbsmi_lg_fsamp_create_em: the bootstrap-filter conditional sampler of
    experiments/sb/filter.py:149-161 for up to `nsamples` independent samples per call -- x0, the joint Euler-Maruyama
    path, the reversal of its y half, initial particles, the batched flow-0 filter and the pick of the first particle in
    one hipGraph replay.  sample() and views() are LGFilterSampler's; a ragged call runs on the bridge's handle of that
    size and the same prior."""

    def __init__(self, model: GaussianSBBridge, nparticles, resampling="stratified", nsamples=1, x0_prior=None):
        if getattr(model, "em_struct", None) is None:
            raise NotImplementedError("the fused SB filter sampler needs an Euler-Maruyama forward process")
        self.prior = x0_prior
        self._prior_dev = None if x0_prior is None else tuple(torch.from_numpy(a).to(model.device) for a in x0_prior)
        self._setup(model, nparticles, resampling, nsamples)   # tables: lg_pmcmc_tables of the terminal marginal N(mean1, cov1)

    def _create(self, h):
        mean, chol = (None, None) if self._prior_dev is None else (t.data_ptr() for t in self._prior_dev)
        _lib.call("fbsmi_lg_fsamp_create_em", C.byref(self.model.struct), C.byref(self.model.em_struct),
                  C.byref(self.tables), mean, chol, self.n, LGFilter._RES[self.resampling], self.C, C.byref(h))

    def _of_size(self, B):
        return self.model.sb_filter_sampler_handle(self.n, self.resampling, B, self.prior)


# ---- the exact Kalman sampler and smoother of the SB toy (include/fbsmi.h, fbsmi_kf_set_em_forward) ---------------------
def _need_sb(bridge, what):
    if not isinstance(bridge, GaussianSBBridge):
        raise NotImplementedError(f"{what} takes a GaussianSBBridge (an Euler-Maruyama forward process); a "
                                  f"{type(bridge).__name__} such as LinearGaussianBridge has the entry point without sb_")


def sb_kalman_model(bridge: GaussianSBBridge):
    """The SB bridge's Kalman tables -- lg_kalman_tables(bridge.tables64, bridge.pmcmc_tables_host(None),
    initial_cov(bridge.cov1, du)) -- as host float64 (``tables64``), host float32 (``host``) and an fbsmi_kf_model struct
    whose F, sqQ are the model's all-zero placeholders; built once and cached on the bridge."""
    _need_sb(bridge, "sb_kalman_model")
    return bridge._cached(("sb_kalman_model",), lambda: _kf_struct(bridge))


def sb_kalman_smoother_model(bridge: GaussianSBBridge):
    """lg_smoother_tables on top of sb_kalman_model as an fbsmi_kfs_model struct, built once and cached on the bridge."""
    kf = sb_kalman_model(bridge)
    return bridge._cached(("sb_kalman_smoother_model",), lambda: _kfs_struct(bridge, kf))


class _SBFront:
    """What SBKalman and SBKalmanSmoother add to their base classes: the prior, and the Euler-Maruyama front set on the
    library's handle once it exists (``_SET`` names the entry of libfbsmi)."""

    _SET = None

    def _set_front(self, model, x0_prior):
        self.prior = x0_prior
        self._prior_dev = None if x0_prior is None else tuple(torch.from_numpy(a).to(model.device) for a in x0_prior)
        mean, chol = (None, None) if self._prior_dev is None else (t.data_ptr() for t in self._prior_dev)
        with torch.cuda.device(model.device):
            _lib.call(self._SET, self.h, C.byref(model.em_struct), mean, chol)


class SBKalman(_SBFront, LGKalman):
    """LGKalman on a GaussianSBBridge: sample() draws each observation path as SBFilterSampler does on the same key (x0,
    the joint Euler-Maruyama path, the reversal of its y half), then runs the exact filter and the draw; filter() and
    views() are LGKalman's.  A ragged call runs on the bridge's handle of that size and the same prior."""

    _SET = "fbsmi_kf_set_em_forward"

    def __init__(self, model: GaussianSBBridge, nsamples=1, x0_prior=None):
        _need_sb(model, "SBKalman")
        LGKalman.__init__(self, model, nsamples)
        self._set_front(model, x0_prior)

    def _struct_of(self, model):
        return sb_kalman_model(model)

    def _of_size(self, B):
        return self.model.sb_kalman_handle(B, self.prior)


class SBKalmanSmoother(_SBFront, LGKalmanSmoother):
    """LGKalmanSmoother on a GaussianSBBridge: sample() on the observation paths of SBKalman.sample; sample_on(), smooth()
    and views() are LGKalmanSmoother's."""

    _SET = "fbsmi_kfs_set_em_forward"

    def __init__(self, model: GaussianSBBridge, nsamples=1, x0_prior=None):
        _need_sb(model, "SBKalmanSmoother")
        LGKalmanSmoother.__init__(self, model, nsamples)
        self._set_front(model, x0_prior)

    def _struct_of(self, model):
        return sb_kalman_smoother_model(model)

    def _of_size(self, B):
        return self.model.sb_kalman_smoother_handle(B, self.prior)


def sb_kalman_conditional_sampler(keys, y0, bridge, x0_prior=None, return_moments=False, _bound=KF_PATH_ELEMS):
    """The Kalman-filter conditional sampler for every key of `keys` (B, 2) [or (2,)] on a GaussianSBBridge, each on the
    observation path sb_filter_conditional_sampler draws from that key: -> samples (B, du) [, filtering means (B, du),
    exact log-likelihoods log p(v_1..v_T | v_0) (B)].  x0_prior = (mean, chol_lower) ('proper') or None ('heuristic').
    The batch runs in chunks that keep one call's B * (T + 1) * dv within `_bound` elements."""
    _need_sb(bridge, "sb_kalman_conditional_sampler")
    return _conditional_chunks(keys, y0, bridge, lambda B: bridge.sb_kalman_handle(B, x0_prior), return_moments, _bound)


def sb_kalman_path_sampler(keys, y0, bridge, x0_prior=None, return_moments=False, _bound=KF_PATH_ELEMS):
    """The forward-filter / backward-sampler for every key of `keys` on a GaussianSBBridge: exact draws from
    p(u_0..u_T | v_0..v_T) on each key's own observation path -> paths (B, T+1, du) [, smoothed means (B, T+1, du), exact
    log-likelihoods (B)]; paths[:, T] is sb_kalman_conditional_sampler's draw on the same keys."""
    _need_sb(bridge, "sb_kalman_path_sampler")
    return _path_chunks(keys, y0, bridge, lambda B: bridge.sb_kalman_smoother_handle(B, x0_prior), return_moments, _bound)
