"""The fused Kalman-filter conditional sampler (include/fbsmi.h, fbsmi_kf_*) restated in float32 numpy from the oracle's
primitives, every chain an explicit loop of correctly rounded fmaf in the header's order, batched over the samples (each
sample's arithmetic is its own).  Not collected: the tests import it."""
import numpy as np

from sb_restate import fmaf

f32 = np.float32


def chain(M, acc, x):
    """acc[b][i] = fmaf(M[i][c], x[b][c], acc[b][i]) for c ascending; M (R, C), acc (B, R), x (B, C)."""
    acc = np.array(acc, f32)
    M = np.asarray(M, f32)
    for c in range(M.shape[1]):
        acc = fmaf(M[None, :, c], x[:, c:c + 1], acc)
    return acc


def m0_restated(kt, yT):
    """The float64 conditional mean of ref_sampler in ascending c, rounded to float32 (tests/fsamp_restate.py).
    kt: m_u (du), m_v (dv), gain (du, dv) float64; yT (B, dv) float32."""
    y = np.asarray(yT, f32).astype(np.float64)
    B, du = y.shape[0], kt["m_u"].size
    m = np.empty((B, du), f32)
    for j in range(du):
        s = np.zeros(B, np.float64)
        for c in range(y.shape[1]):
            s = s + kt["gain"][j, c] * (y[:, c] - kt["m_v"][c])
        m[:, j] = (kt["m_u"][j] + s).astype(f32)
    return m


def filter_restated(host, kt, vs):
    """host: the float32 tables H, e, Pm, c, AK, W, lconst; kt: lg_kalman_tables' m_u, m_v, gain; vs (B, T+1, dv)
    -> (m_0 (B, du), m_T (B, du), loglik (B))."""
    vs = np.asarray(vs, f32)
    B, T1, dv = vs.shape
    du = host["c"].shape[1]
    m0 = m0_restated(kt, vs[:, 0])
    m, ll = m0.copy(), np.zeros(B, f32)
    for k in range(T1 - 1):
        z = np.concatenate([m, vs[:, k]], axis=1)
        # pred and the first part of m' run over the same operand: one stacked chain, the rows independent
        both = chain(np.concatenate([host["H"][k], host["Pm"][k]]),
                     np.broadcast_to(np.concatenate([host["e"][k], host["c"][k]])[None, :], (B, dv + du)), z)
        r = (vs[:, k + 1] - both[:, :dv]).astype(f32)
        tail = chain(np.concatenate([host["AK"][k], host["W"][k]]),
                     np.concatenate([both[:, dv:], np.zeros((B, dv), f32)], axis=1), r)
        m, qv = tail[:, :du], tail[:, du:]
        ss = np.zeros(B, f32)
        for i in range(dv):
            ss = fmaf(qv[:, i], qv[:, i], ss)
        ll = (ll + ((f32(-0.5) * ss).astype(f32) + host["lconst"][k]).astype(f32)).astype(f32)
    return m0, np.ascontiguousarray(m), ll


def draw_restated(O, host, key_kf, m_T):
    """x_j: acc = m_T[j], then fmaf(Lt[c][j], zz[c], acc), c ascending, zz = normal(key_kf, (du,)); one sample."""
    zz = O.normal(np.asarray(key_kf, np.uint32), (m_T.size,))
    return chain(np.ascontiguousarray(host["Lt"].T), m_T[None, :], zz[None, :])[0]


def want(O, om, host, kt, keys, y0):
    """The batch of conditional samples -> dict(vs (B, T+1, dv), m_ (B, du), means (B, du), loglik (B), samples (B, du))."""
    keys = np.asarray(keys, np.uint32).reshape(-1, 2)
    ks = [O.split(k, 3) for k in keys]                                     # key_fwd, key_bwd (unused), key_kf
    vs = np.stack([O.lg_fwd_sampler(om, k3[0], np.asarray(y0, f32))[::-1] for k3 in ks]).astype(f32)
    m0, mT, ll = filter_restated(host, kt, vs)
    samples = np.stack([draw_restated(O, host, k3[2], mT[b]) for b, k3 in enumerate(ks)])
    return dict(vs=vs, m_=m0, means=mT, loglik=ll, samples=samples)
