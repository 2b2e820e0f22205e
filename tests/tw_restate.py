"""Numpy restatement of the fused twisted SMC's numeric specification (include/fbsmi.h, fbsmi_tw_*): the five closures
on a GaussianTwisted's float32 tables -- fmaf chains in ascending column order, row sums in row order, one float32
rounding per operation -- run through oracle.twisted_smc_np with the oracle's resamplers and choice."""
import numpy as np

from sb_restate import fmaf

f32 = np.float32


def drift(M, m, u):
    """drift_i(M, m, u) for every row of u (N, d): acc = m_i, then acc = fmaf(M[i][c], u[c], acc), c ascending."""
    N, d = u.shape
    acc = np.broadcast_to(np.asarray(m, f32)[None, :], (N, d)).copy()
    for c in range(d):
        acc = fmaf(np.broadcast_to(M[None, :, c], (N, d)), np.broadcast_to(u[:, c:c + 1], (N, d)), acc)
    return acc


def nlp(x, loc, s2, ln):
    e = (x - loc).astype(f32)
    return ((f32(ln) + (e * e).astype(f32) / f32(s2)).astype(f32) / f32(-2)).astype(f32)


def rowsum(t):
    acc = t[:, 0].astype(f32).copy()
    for i in range(1, t.shape[1]):
        acc = (acc + t[:, i]).astype(f32)
    return acc


class Restate:
    """The closures of experiments/toy/gp_twisted.py:100-129 on model.host (float32 tables of a GaussianTwisted)."""

    def __init__(self, O, model):
        self.O, self.h, self.d = O, model.host, model.d
        self.ts = np.asarray(model.ts_np, np.float64)
        self.dt, self.obs_var, self.lognorm_obs = f32(model.dt), f32(model.obs_var), f32(model.lognorm_obs)
        self.y = model.host["y"]

    def j(self, t):
        return int(np.argmin(np.abs(self.ts - float(t))))

    def step(self, M, m, j, u):
        """u + drift(M[j], m[j], u) dt"""
        return (u + (drift(self.h[M][j], self.h[m][j], u) * self.dt).astype(f32)).astype(f32)

    def init_sampler(self, key, n):
        z, Lt = self.O.normal(key, (n, self.d)), self.h["Lt"]
        acc = (z[:, 0:1] * Lt[0][None, :]).astype(f32)
        for c in range(1, self.d):
            acc = (acc + (z[:, c:c + 1] * Lt[c][None, :]).astype(f32)).astype(f32)
        return (self.h["m_ref"][None, :] + acc).astype(f32)

    def twisting_logpdf(self, y, u, t):
        return rowsum(nlp(np.asarray(y, f32)[None, :], self.step("R", "r", self.j(t), u), self.obs_var, self.lognorm_obs))

    def twisting_prop_sampler(self, key, us, t, y):
        j = self.j(t)
        m = self.step("C", "c", j, us)
        return (m + (self.h["sd"][j] * self.O.normal(key, us.shape)).astype(f32)).astype(f32)

    def _sd2(self, j):
        return f32(self.h["sd"][j] * self.h["sd"][j])

    def twisting_prop_logpdf(self, u, u_prev, t, y):
        j = self.j(t)
        return rowsum(nlp(u, self.step("C", "c", j, u_prev), self._sd2(j), self.h["lognorm"][j]))

    def transition_logpdf(self, u, u_prev, t_prev):
        j = self.j(t_prev)
        return rowsum(nlp(u, self.step("R", "r", j, u_prev), self._sd2(j), self.h["lognorm"][j]))

    def run(self, key, nparticles, resampling="stratified"):
        """-> (particles (N, d), normalised log-weights (N,), ancestors (T, N))"""
        O = self.O
        xs, lws, inds = O.twisted_smc_np(np.asarray(key, np.uint32), self.y, self.ts, self.init_sampler, self.transition_logpdf,
                                         self.twisting_logpdf, self.twisting_prop_sampler, self.twisting_prop_logpdf,
                                         getattr(O, resampling), nparticles)
        return xs, lws, np.stack(inds).astype(np.int32)

    def sample(self, key, nparticles, resampling="stratified"):
        """conditional_sampler (gp_twisted.py:133-141)"""
        key_filter, key_select = self.O.split(np.asarray(key, np.uint32), 2)
        xs, lws, _ = self.run(key_filter, nparticles, resampling)
        return xs[int(self.O.choice(key_select, self.O.exp(lws)))]
