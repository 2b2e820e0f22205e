"""Numpy restatement of the fused CSGM's numeric specification (include/fbsmi.h, fbsmi_csgm_*) on a GaussianCSGM's float32
tables: the drift and u0 as fmaf chains in ascending column order, the trajectory through oracle.euler_maruyama_np, one
float32 rounding per operation."""
import numpy as np

from sb_restate import fmaf

f32 = np.float32


def drift(M, m, u):
    """drift_i(M, m, u) for every row of u (N, d): acc = m_i, then acc = fmaf(M[i][c], u[c], acc), c ascending
    (tests/tw_restate.py::drift)."""
    N, d = u.shape
    acc = np.broadcast_to(np.asarray(m, f32)[None, :], (N, d)).copy()
    for c in range(d):
        acc = fmaf(np.broadcast_to(M[None, :, c], (N, d)), np.broadcast_to(u[:, c:c + 1], (N, d)), acc)
    return acc


class Restate:
    """conditional_sampler of experiments/toy/gp_csgm.py:103-108 on model.host (float32 tables of a GaussianCSGM)."""

    def __init__(self, O, model):
        self.O, self.h, self.d, self.T = O, model.host, model.d, model.T
        self.ts = np.asarray(model.ts_np, np.float64)
        # a dispersion b_k that euler_maruyama_np rounds to the tabulated s[k]: float32(b_k * sqrt(ddt))
        self.b = np.array([float(model.sde.dispersion(float(self.ts[-1] - self.ts[k]))) for k in range(self.T)])
        for k in range(self.T):
            ddt = abs(float(self.ts[k + 1]) - float(self.ts[k]))
            assert f32(self.dispersion(self.ts[k]) * float(np.sqrt(ddt))) == self.h["s"][k], k
            assert f32(ddt) == self.h["ddt"][k], k

    def k(self, t):
        return int(np.argmin(np.abs(self.ts[:-1] - float(t))))

    def drift(self, x, t):
        k = self.k(t)
        x = np.asarray(x, f32)
        return drift(self.h["A"][k], self.h["cvec"][k], x.reshape(-1, self.d)).reshape(x.shape)

    def dispersion(self, t):
        return self.b[self.k(t)]

    def u0(self, key_init):
        z = self.O.normal(np.asarray(key_init, np.uint32), (self.d,))
        return drift(self.h["S_ref"], self.h["m_ref"], z[None, :])[0]

    def integrate(self, key_sde, u0, return_path=False):
        """euler_maruyama(key_sde, u0 (d,), ts, drift, dispersion): xi = normal(split(key_sde, T)[k], (1, d))[0]"""
        return self.O.euler_maruyama_np(np.asarray(key_sde, np.uint32), np.asarray(u0, f32), self.ts, self.drift, self.dispersion,
                                        integration_nsteps=1, return_path=return_path)

    def sample(self, key):
        """-> (u0 (d,), path (T+1, d)); the sample is path[-1]"""
        key_init, key_sde = self.O.split(np.asarray(key, np.uint32), 2)
        u0 = self.u0(key_init)
        return u0, self.integrate(key_sde, u0, return_path=True)

    def sample_batch(self, keys):
        """sample() for a batch of keys at once: the same chains and the same roundings in the same order (drift is per
        row already), the draws per key; what a batch of thousands can afford.  -> (u0 (B, d), path (T+1, B, d))"""
        O, h, d, T = self.O, self.h, self.d, self.T
        ks = [O.split(np.asarray(k, np.uint32), 2) for k in np.asarray(keys, np.uint32).reshape(-1, 2)]
        x = drift(h["S_ref"], h["m_ref"], np.stack([O.normal(k2[0], (d,)) for k2 in ks]))
        xi = np.stack([np.stack([O.normal(kk, (1, d))[0] for kk in O.split(k2[1], T)]) for k2 in ks], axis=1)   # (T, B, d)
        path = [x]
        for k in range(T):
            f = drift(h["A"][k], h["cvec"][k], x)
            x = ((x + (f * h["ddt"][k]).astype(f32)).astype(f32) + (h["s"][k] * xi[k]).astype(f32)).astype(f32)
            path.append(x)
        return path[0], np.stack(path)

