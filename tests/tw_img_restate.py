"""Numpy float64 restatement of the step kernels of the image twisted SMC (include/fbsmi.h, fbsmi_tw_img_*_batched) for ONE
ensemble, from the kernels' own inputs, with first-order float32 rounding bounds per output.  u = 2^-24 is the unit
roundoff; the scalars cx, cs, dt, sd, var_y are taken as the float32 values the kernels receive, and X, the network output
S, the vector-Jacobian product V, y and the draw z as the float32 arrays they read, so none of them carries an error.

Roundings counted per specified expression (the way StepRef.proposal and StepRef.logpdf of tests/lg_image_model.py do):

  den = x + (cx x + cs s) dt       t1 | t2, rd, p, den: at most four roundings on every term
                                   E_den = 4 u (|x| + |cx x dt| + |cs s dt|)
  g = (y - den) / var_y            df, the quotient:   E_g = E_den / var_y + 2 u |g|
  ct = (cs dt) g                   cs dt, the product:  E_ct = |cs dt| E_g + 2 u |ct|
  nlp(a, m, v) with E_m on m       df (u |df| + E_m), its square (u), the quotient (u), v = sd sd where it is (u), the sum
                                   with the logarithm (u); the logarithm itself: its argument 2 pi v carries the constant,
                                   v and the product (2.5 u, absolute on the logarithm) and fbsmi_logf one ulp (2 u |log|)
                                   E_term = (2 |df| E_m / v + 7 u df^2 / v + 6 u |log(2 pi v)| + 6 u) / 2
  a row sum of d terms             the pairwise tree: depth = ceil(log2 d) + 2 roundings on every term
                                   E_sum = sum E_term + depth u sum |term|
  lw = ((tl + lp) - pl) - lpg      three roundings: E_lw = E_lp + 3 u (|tl| + |lp| + |pl| + |lpg|)   (tl, pl, lpg are inputs)
  grad = (1 + cx dt) g + vjp       c1, kap (u (|cx dt| + |kap|) on kap), hg, grad:
                                   E_grad = |kap| E_g + 4 u (|kap g| + |cx dt g| + |vjp|)
  m = x + (rd + cs grad) dt        the rd path: t1 | t2, rd, cd, pm, m (five, and one on x); the grad path: cg, cd, pm, m
                                   E_m = 6 u (|x| + |cx x dt| + |cs s dt|) + cs dt (E_grad + 4 u |grad|)
  x_new = m + sd z                 nz, x_new:  E_x = E_m + u |m| + 3 u |sd z|
"""
import math

import numpy as np

U32 = 2.0 ** -24


def depth(d: int) -> int:
    return math.ceil(math.log2(max(int(d), 2))) + 2


class TwStep:
    """One step's scalars (python floats holding float32 values) and one mask's role table (D,), role[e] < 0: observed
    element ~role[e]."""

    def __init__(self, role, cx, cs, dt, sd, var_y):
        self.role = np.asarray(role, np.int64)
        self.obs = self.role < 0
        self.j = ~self.role[self.obs]                      # observed element of every observed image position
        self.D, self.dv = self.role.size, int(self.obs.sum())
        self.v_off = np.zeros(self.dv, np.int64)
        self.v_off[self.j] = np.nonzero(self.obs)[0]
        self.cx, self.cs, self.dt, self.sd, self.var_y = (float(v) for v in (cx, cs, dt, sd, var_y))
        self.kap = 1.0 + self.cx * self.dt

    @staticmethod
    def _f64(*arrays):
        return tuple(np.asarray(a, np.float64) for a in arrays)

    def den(self, X, S):
        """-> (den, rd, E_den) for X, S (n, D)."""
        X, S = self._f64(X, S)
        rd = self.cx * X + self.cs * S
        E = 4 * U32 * (np.abs(X) + np.abs(self.cx * X * self.dt) + np.abs(self.cs * S * self.dt))
        return X + rd * self.dt, rd, E

    def head_grad(self, X, S, y):
        """-> (g, E_g, rd): g = (y - den) / var_y on the observed positions, 0 elsewhere."""
        den, rd, E_den = self.den(X, S)
        y = np.asarray(y, np.float64).reshape(-1)
        g, E = np.zeros_like(den), np.zeros_like(den)
        g[:, self.obs] = (y[self.j][None, :] - den[:, self.obs]) / self.var_y
        E[:, self.obs] = E_den[:, self.obs] / self.var_y + 2 * U32 * np.abs(g[:, self.obs])
        return g, E, rd

    def _nlp_rows(self, a, m, E_m, var):
        """(row sums of nlp(a, m, var), their bound): a, m, E_m (n, d)."""
        df = a - m
        lognorm = math.log(2 * math.pi * var)
        terms = -0.5 * (lognorm + df * df / var)
        per = 0.5 * (2 * np.abs(df) * E_m / var + 7 * U32 * df * df / var + 6 * U32 * abs(lognorm) + 6 * U32)
        return terms.sum(1), per.sum(1) + depth(a.shape[1]) * U32 * np.abs(terms).sum(1)

    def twist(self, X, S, y):
        """-> (lp (n,), bound)."""
        den, _, E_den = self.den(X, S)
        y = np.asarray(y, np.float64).reshape(-1)
        if self.dv == 0:
            return np.zeros(den.shape[0]), np.zeros(den.shape[0])
        return self._nlp_rows(np.broadcast_to(y[None, :], (den.shape[0], self.dv)), den[:, self.v_off], E_den[:, self.v_off],
                              self.var_y)

    def weights(self, lp, E_lp, tl, pl, lpg):
        """-> (lw, bound) with tl, pl, lpg the float32 arrays the kernel reads."""
        lp, tl, pl, lpg = self._f64(lp, tl, pl, lpg)
        return ((tl + lp) - pl) - lpg, E_lp + 3 * U32 * (np.abs(tl) + np.abs(lp) + np.abs(pl) + np.abs(lpg))

    def cotangent(self, X, S, y):
        """-> (ct (n, D), bound)."""
        g, E_g, _ = self.head_grad(X, S, y)
        ct = self.cs * self.dt * g
        return ct, abs(self.cs * self.dt) * E_g + 2 * U32 * np.abs(ct)

    def grad(self, X, S, V, y):
        """d lp / d x = (1 + cx dt) g + vjp -> (grad, bound)."""
        g, E_g, _ = self.head_grad(X, S, y)
        V = np.asarray(V, np.float64)
        return self.kap * g + V, abs(self.kap) * E_g + 4 * U32 * (np.abs(self.kap * g) + np.abs(self.cx * self.dt * g) + np.abs(V))

    def mean(self, X, S, V, y):
        """The proposal's mean m = x + (rd + cs grad) dt -> (m, bound)."""
        X, S = self._f64(X, S)
        grad, E_grad = self.grad(X, S, V, y)
        rd = self.cx * X + self.cs * S
        m = X + (rd + self.cs * grad) * self.dt
        E = 6 * U32 * (np.abs(X) + np.abs(self.cx * X * self.dt) + np.abs(self.cs * S * self.dt)) \
            + self.cs * self.dt * (E_grad + 4 * U32 * np.abs(grad))
        return m, E

    def propose(self, X, S, V, y, Z):
        """-> (x_new, bound, m, E_m) with Z (n, D) the float32 draw."""
        m, E_m = self.mean(X, S, V, y)
        nz = self.sd * np.asarray(Z, np.float64).reshape(m.shape)
        return m + nz, E_m + U32 * np.abs(m) + 3 * U32 * np.abs(nz), m, E_m

    def logpdfs(self, X, S, V, y, x_new):
        """The two row-summed densities AT the float32 x_new the kernel produced -> (tl, E_tl, pl, E_pl)."""
        den, _, E_den = self.den(X, S)
        m, E_m = self.mean(X, S, V, y)
        xn = np.asarray(x_new, np.float64).reshape(den.shape)
        var = self.sd * self.sd
        return self._nlp_rows(xn, den, E_den, var) + self._nlp_rows(xn, m, E_m, var)


def step_scalars(sde, ts, k, data_variance=0.06):
    """(cx, cs, dt, sd, var_y) of reverse time ts[k] as the host layer computes them: float64, rounded to float32."""
    from fbs_amd.sdes import make_linear_sde
    ts = np.asarray(ts, np.float64)
    T = float(ts[-1])
    dt = T / (ts.size - 1)
    s = T - float(ts[k])
    F, Q = (float(v) for v in make_linear_sde(sde)[0](s, float(ts[0])))
    vals = (-float(sde.drift(1.0, s)), float(sde.dispersion(s)) ** 2, dt, math.sqrt(dt) * float(sde.dispersion(s)),
            F ** 2 * data_variance + Q)
    return tuple(float(np.float32(v)) for v in vals)
