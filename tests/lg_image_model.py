"""A Gaussian image model: the image tier's closures on a model whose answer is known.

With a Gaussian prior N(m0, cov0) on the ravelled image the true score at forward time t is linear,

    score(x, t) = -(F_t^2 cov0 + Q_t I)^{-1} (x - F_t m0),

so a ``ScoreBridge`` around it runs the discretised model of ``LinearGaussianBridge`` on the same prior, up to the permutation
that puts a mask's unobserved coordinates first.  ``lg_tables`` of the permuted prior (float64) is then the ground truth
of every step of the image tier, and the analytic tier's samplers are reference samplers of the image tier's.

Nothing here restates a kernel: the step references are G z + g from ``lg_tables``, never cx x + cs s.  The prior is built
so that layout mistakes change the answer: a non-constant mean, different length scales along rows and columns, a channel
matrix with distinct off-diagonal entries, and unobserved pixels correlated with observed ones.

The prior, ``perm``, the masks with a given shift, the step references, the Kalman filter and the numpy bootstrap filter
run without a GPU.
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24                                           # unit roundoff of float32


def make_sde():
    from fbs_amd.sdes import StationaryLinLinearSDE
    return StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=2.0)


def channel_matrix(c: int) -> np.ndarray:
    """c x c SPD, L L^T of a unit lower-triangular L with distinct entries (so distinct off-diagonal entries)."""
    L = np.eye(c)
    for i in range(c):
        for j in range(i):
            L[i, j] = (-1.0) ** (i + j) * 0.9 / (1.0 + i + 2.0 * j)
    return L @ L.T


def prior(shape):
    """(m0 (D,), cov0 (D, D)) in the order of ``img.reshape(-1)``: pixel-major (row, then column), channel fastest."""
    w, h, c = shape
    rows, cols = (a.reshape(-1).astype(np.float64) for a in np.meshgrid(np.arange(w), np.arange(h), indexing="ij"))
    # a product of exponential kernels (SPD), correlation length 1.5 pixels down the rows and 3.5 along the columns
    kpix = np.exp(-np.abs(rows[:, None] - rows[None, :]) / 1.5 - np.abs(cols[:, None] - cols[None, :]) / 3.5)
    cov0 = 0.6 * np.kron(kpix, channel_matrix(c)) + 0.05 * np.eye(w * h * c)
    ch = np.arange(c, dtype=np.float64)
    m0 = (0.5 * np.sin(0.7 * rows + 0.3)[:, None] + 0.3 * np.cos(1.1 * cols)[:, None] + 0.2 * ch[None, :] - 0.1).reshape(-1)
    return m0, cov0


def inpaint_mask(shape, hole: int, shift: int, device="cpu"):
    """The mask ``ImageRestore('inpaint-<hole>', shape)`` generates when its draw of the shift gives `shift`."""
    from fbs_amd.images import InpaintingMask
    w, h = shape[:2]
    hw, hh = min(hole, w), min(hole, h)
    rr, cc = (a.reshape(-1) for a in np.meshgrid(np.arange(hw), np.arange(hh), indexing="ij"))
    rect = np.ravel_multi_index([rr + shift, cc + shift], (w, h), mode="clip")
    obs = np.setdiff1d(np.arange(w * h), rect, assume_unique=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(device)
    return InpaintingMask(hw, hh, int(shift), unobs_inds_ravelled=t(rect), obs_inds_ravelled=t(obs))


def perm(mask, c: int) -> np.ndarray:
    """Image coordinates (indices into ``img.reshape(-1)``) in the order (unobserved, observed) of ``ImageRestore.unpack``:
    ``img.reshape(-1)[perm] == cat(x.reshape(-1), y.reshape(-1))`` for ``x, y = unpack(img, mask)``."""
    un = mask.unobs_inds_ravelled.detach().cpu().numpy().astype(np.int64)
    ob = mask.obs_inds_ravelled.detach().cpu().numpy().astype(np.int64)
    ch = np.arange(c, dtype=np.int64)
    return np.concatenate([(un[:, None] * c + ch[None, :]).reshape(-1), (ob[:, None] * c + ch[None, :]).reshape(-1)])


class LGImageModel:
    def __init__(self, shape, ts, sde=None):
        self.shape = tuple(shape)
        self.D = int(np.prod(shape))
        self.ts = np.asarray(ts, np.float64)
        self.sde = make_sde() if sde is None else sde
        self.m0, self.cov0 = prior(self.shape)
        self.lam, self.V = np.linalg.eigh(self.cov0)
        self._dev = {}

    def score_fn(self, dtype=torch.float32):
        """score_fn(x (B, w, h, c), t) for ``ScoreBridge``: float64 on x's own device, rounded once to float32 (and once
        more to `dtype` if that is bfloat16)."""
        from fbs_amd.sdes.linear import discretise_linear_sde_np

        def fn(x, t):
            d = self._dev.get(x.device)
            if d is None:
                d = self._dev[x.device] = tuple(torch.from_numpy(a).to(x.device) for a in (self.V, self.lam, self.m0))
            V, lam, m0 = d
            F, Q = (float(a) for a in discretise_linear_sde_np(self.sde, float(t), float(self.ts[0])))
            z = x.to(torch.float64).reshape(x.shape[0], self.D) - F * m0
            s = -(((z @ V) / (F * F * lam + Q)) @ V.T)
            s = s.to(torch.float32)
            return (s if dtype == torch.float32 else s.to(dtype)).reshape(x.shape)

        return fn

    def du_of(self, mask) -> int:
        return int(mask.unobs_inds_ravelled.numel()) * self.shape[2]

    def permuted(self, mask):
        p = perm(mask, self.shape[2])
        return self.m0[p], self.cov0[np.ix_(p, p)], self.du_of(mask)

    def tables(self, mask) -> dict:
        """``lg_tables`` of the permuted prior: G, g, sd, dt are the float64 ground truth of a step."""
        from fbs_amd.linear_gaussian import lg_tables
        m, cov, du = self.permuted(mask)
        return lg_tables(m, cov, self.sde, self.ts, du)

    def bridge(self, mask, device):
        """The ``LinearGaussianBridge`` of the permuted model (``.tables64`` are ``tables(mask)``)."""
        from fbs_amd.linear_gaussian import LinearGaussianBridge
        m, cov, du = self.permuted(mask)
        return LinearGaussianBridge(m, cov, self.sde, self.ts, du, device=device)

    def coef(self, k):
        """(cx, cs) of the reverse drift cx x + cs score of step k, float64: -a(T - ts[k]) and b(T - ts[k])^2.  Only the
        rounding bounds and the bfloat16 reference use them."""
        tf = float(self.ts[-1] - self.ts[k])
        return -float(self.sde.drift(1.0, tf)), float(self.sde.dispersion(tf)) ** 2


# ------------------------------------------------------------------------------------------------
# one step in float64, with first-order rounding bounds
# ------------------------------------------------------------------------------------------------
class StepRef:
    """Step k of the model with tables `tab` at particles U (n, du) and observation v_prev (dv,), float64.
    ``drift`` (n, D) = G[k] z + g[k] with z = (u, v_prev); ``s`` the score it implies, (drift - cx z) / cs.
    bf16: the drift is rebuilt from the score rounded to float32 and then to bfloat16, as a bfloat16 network returns it."""

    def __init__(self, tab, k, cx, cs, U, v_prev, bf16=False):
        self.du, self.dv = tab["du"], tab["dv"]
        self.dt, self.sd = float(tab["dt"]), float(tab["sd"][k])
        self.cx, self.cs = cx, cs
        U = np.asarray(U, np.float64).reshape(-1, self.du)
        self.Z = np.concatenate([U, np.broadcast_to(np.asarray(v_prev, np.float64).reshape(1, -1), (U.shape[0], self.dv))], 1)
        self.drift = self.Z @ tab["G"][k].T + tab["g"][k]
        self.s = (self.drift - cx * self.Z) / cs
        if bf16:
            from oracle.em import from_bf16_bits, to_bf16_bits
            self.s = from_bf16_bits(to_bf16_bits(self.s.astype(np.float32))).astype(np.float64)
            self.drift = cx * self.Z + cs * self.s
        # the analytic tier's own arithmetic: a float32 dot product of D terms, folded in index order, on tables rounded to
        # float32 -- (D + 2) u sum_j |G_ij z_j| + 2 u |g_i| to first order (rounded G and g, one rounding per fmaf)
        D = self.du + self.dv
        self.lg_dot = (D + 2) * U32 * (np.abs(self.Z) @ np.abs(tab["G"][k]).T + np.abs(tab["g"][k]))

    def proposal(self, zeta):
        """(u + drift_u dt + sd zeta, bound).  The kernel's path is t1 = cx x, t2 = cs s, d = t1 + t2, d dt, x + ., sd z,
        . + .: seven float32 roundings, and cx, cs, dt, sd, s are themselves rounded to float32."""
        du = self.du
        zeta = np.asarray(zeta, np.float64).reshape(-1, du)
        x, s = self.Z[:, :du], self.s[:, :du]
        ref = x + self.drift[:, :du] * self.dt + self.sd * zeta
        bound = 8 * U32 * (np.abs(x) + np.abs(self.cx * x * self.dt) + np.abs(self.cs * s * self.dt) + np.abs(self.sd * zeta))
        return ref, bound

    def logpdf(self, target, block: str, tree: bool = True):
        """(sum_j -(log(2 pi sd^2) + (target_j - mean_j)^2 / sd^2) / 2, bound) over the block 'v' (the likelihood of
        v = target) or 'u' (the transition density of u = target (n, du)), mean = prev + drift dt.
        tree: the terms are added pairwise (depth ceil(log2 d)); otherwise in index order (depth d)."""
        sl = slice(self.du, None) if block == "v" else slice(0, self.du)
        prev, s, drift = self.Z[:, sl], self.s[:, sl], self.drift[:, sl]
        tgt = np.broadcast_to(np.asarray(target, np.float64).reshape(-1, prev.shape[1]), prev.shape)
        var = self.sd ** 2
        lognorm = math.log(2 * math.pi * var)
        df = tgt - (prev + drift * self.dt)
        terms = -0.5 * (lognorm + df * df / var)
        d = prev.shape[1]
        delta = 8 * U32 * (np.abs(tgt) + np.abs(prev) + np.abs(self.cx * prev * self.dt) + np.abs(self.cs * s * self.dt))
        per = 0.5 * (2 * np.abs(df) * delta / var + 4 * U32 * df * df / var + 4 * U32 * abs(lognorm))
        # two terms the first-order count above leaves out:
        #  - sd^2 is the float32 square of the rounded sd (3 u), so with the square of df (u) and the division (u) the
        #    quadratic term carries 5 u, not 4 u;
        #  - the argument of the logarithm, 2 pi sd^2, carries 4 u (the constant, sd twice, the product), which moves the
        #    logarithm by 4 u in ABSOLUTE terms -- 4 u |log| covers that only while |log| >= 1.
        per = per + 0.5 * (U32 * df * df / var + 4 * U32)
        if not tree:      # the analytic tier: its drift carries lg_dot, which moves df by lg_dot dt
            per = per + np.abs(df) / var * self.dt * self.lg_dot[:, sl]
        depth = (math.ceil(math.log2(max(d, 2))) if tree else d) + 2
        bound = per.sum(1) + depth * U32 * np.abs(terms).sum(1)
        return terms.sum(1), bound

    def lg_proposal_extra(self):
        """What the analytic tier's float32 dot product adds to the bound of a proposal element."""
        return self.lg_dot[:, :self.du] * self.dt


# ------------------------------------------------------------------------------------------------
# the discretised reverse model as a linear-Gaussian state-space model: exact filter, and a plain particle filter
# ------------------------------------------------------------------------------------------------
def ssm_of(tab, vs):
    """Per step k: u_{k+1} = A u_k + b + sd zeta and v_{k+1} = H u_k + d + sd eta (independent given u_k), from G, g, sd,
    dt and the observation path vs (T + 1, dv) in reverse time."""
    du, dt = tab["du"], float(tab["dt"])
    vs = np.asarray(vs, np.float64).reshape(len(tab["sd"]) + 1, -1)
    out = []
    for k in range(len(tab["sd"])):
        G, g = tab["G"][k], tab["g"][k]
        A = np.eye(du) + G[:du, :du] * dt
        b = (G[:du, du:] @ vs[k] + g[:du]) * dt
        H = G[du:, :du] * dt
        d = vs[k] + (G[du:, du:] @ vs[k] + g[du:]) * dt
        out.append((A, b, H, d, float(tab["sd"][k])))
    return out


def kalman_filter(tab, vs, m=None, P=None):
    """Exact filter of ``ssm_of`` from u_0 ~ N(m, P) (default N(0, I): the image tier's initial particles).
    -> (mean and covariance of u_T given vs[1:], log p(vs[1:] | vs[0]))."""
    du = tab["du"]
    m = np.zeros(du) if m is None else np.asarray(m, np.float64)
    P = np.eye(du) if P is None else np.asarray(P, np.float64)
    vs = np.asarray(vs, np.float64).reshape(len(tab["sd"]) + 1, -1)
    ll = 0.0
    for k, (A, b, H, d, sd) in enumerate(ssm_of(tab, vs)):
        S = H @ P @ H.T + sd ** 2 * np.eye(H.shape[0])
        e = vs[k + 1] - (H @ m + d)
        ll += -0.5 * (e @ np.linalg.solve(S, e) + np.linalg.slogdet(S)[1] + e.size * math.log(2 * math.pi))
        K = np.linalg.solve(S, H @ P).T
        m, P = m + K @ e, P - K @ H @ P
        m, P = A @ m + b, A @ P @ A.T + sd ** 2 * np.eye(du)
    return m, P, ll


def _resample_np(w, rng, kind):
    """Stratified or systematic ancestors of the rows of w (M, N)."""
    M, N = w.shape
    uu = rng.random((M, N)) if kind == "stratified" else np.repeat(rng.random((M, 1)), N, 1)
    pos = (np.arange(N)[None, :] + uu) / N
    cdf = np.cumsum(w, 1)
    cdf /= cdf[:, -1:]
    return np.stack([np.minimum(np.searchsorted(cdf[i], pos[i]), N - 1) for i in range(M)], 0)


def bootstrap_filter_np(tab, vs, seed, M, N, kind="stratified"):
    """M independent bootstrap filters of N particles of ``ssm_of``, float64: -> (mean of the final particles (M, du),
    log-likelihood estimates (M,)).  The order is the image tier's: weight u_k by v_{k+1}, resample, propose u_{k+1}."""
    rng = np.random.default_rng(seed)
    du = tab["du"]
    us = rng.standard_normal((M, N, du))
    ll = np.zeros(M)
    vs = np.asarray(vs, np.float64).reshape(len(tab["sd"]) + 1, -1)
    rowsM = np.arange(M)[:, None]
    for k, (A, b, H, d, sd) in enumerate(ssm_of(tab, vs)):
        e = vs[k + 1] - (us @ H.T + d)
        lw = -0.5 * ((e * e).sum(-1) / sd ** 2 + e.shape[-1] * math.log(2 * math.pi * sd ** 2))
        c = lw.max(1, keepdims=True)
        w = np.exp(lw - c)
        ll += c[:, 0] + np.log(w.mean(1))
        us = us[rowsM, _resample_np(w, rng, kind)]
        us = us @ A.T + b + sd * rng.standard_normal(us.shape)
    return us.mean(1), ll


def log_mean_exp(x):
    x = np.asarray(x, np.float64)
    c = x.max()
    return float(c + np.log(np.mean(np.exp(x - c))))


def log_mean_exp_se(x, B):
    """Standard error of ``log_mean_exp`` of B replicates, from the spread of the replicates x (delta method)."""
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max())
    return float(e.std(ddof=1) / e.mean() / math.sqrt(B))
