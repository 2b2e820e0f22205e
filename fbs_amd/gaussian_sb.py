"""The Gaussian Schrodinger-bridge (SB) toy of experiments/sb/gibbs.py and sb/filter.py as a model descriptor.

The forward process is the closed-form SB between N(mean0, cov0) and N(mean1, cov1) with a Brownian reference of
dispersion ``sig`` (``fbs_amd.sdes.make_gaussian_bw_sb``).  Its drift ``M(t) z + c(t)`` is affine but, unlike the
separable linear SDEs of ``LinearGaussianBridge``, a full matrix and time-dependent; the reference simulates it by
Euler-Maruyama with ``nsub`` sub-steps per interval (sb/gibbs.py:137-139).  The reverse drift is affine as well,

    -drift(z, 1 - t) + sig^2 score(z, 1 - t) = (-M - sig^2 P) z + (-c + sig^2 P m)     (P = cov_s^{-1}, m = mean_s),

so the CSMC part of a sweep and the particle filters run on the fused engine's affine tables unchanged; the forward
paths take the Euler-Maruyama kernel (include/fbsmi.h, fbsmi_em_forward) on the tables of ``sb_tables``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
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
