"""The fused Kalman smoother and path sampler (include/fbsmi.h, fbsmi_kfs_*) restated in float32 numpy on top of
tests/kf_restate.py: the forward step is the filter's, with every m_k and r_k kept; the backward pass carries the
deviation delta_k = u_k - m_k through explicit chains of correctly rounded fmaf in the header's order, batched over the
samples (each sample's arithmetic is its own).  Not collected: the tests import it."""
import numpy as np

from kf_restate import chain, draw_restated, m0_restated
from sb_restate import fmaf

f32 = np.float32


def forward_restated(host, kt, vs):
    """kf_restate.filter_restated keeping every step: vs (B, T+1, dv) -> (m (B, T+1, du), r (B, T, dv), loglik (B))."""
    vs = np.asarray(vs, f32)
    B, T1, dv = vs.shape
    du = host["c"].shape[1]
    ms, rs = np.empty((B, T1, du), f32), np.empty((B, T1 - 1, dv), f32)
    ms[:, 0] = m0_restated(kt, vs[:, 0])
    ll = np.zeros(B, f32)
    for k in range(T1 - 1):
        z = np.concatenate([ms[:, k], vs[:, k]], axis=1)
        both = chain(np.concatenate([host["H"][k], host["Pm"][k]]),
                     np.broadcast_to(np.concatenate([host["e"][k], host["c"][k]])[None, :], (B, dv + du)), z)
        rs[:, k] = (vs[:, k + 1] - both[:, :dv]).astype(f32)
        tail = chain(np.concatenate([host["AK"][k], host["W"][k]]),
                     np.concatenate([both[:, dv:], np.zeros((B, dv), f32)], axis=1), rs[:, k])
        ms[:, k + 1], qv = tail[:, :du], tail[:, du:]
        ss = np.zeros(B, f32)
        for i in range(dv):
            ss = fmaf(qv[:, i], qv[:, i], ss)
        ll = (ll + ((f32(-0.5) * ss).astype(f32) + host["lconst"][k]).astype(f32)).astype(f32)
    return ms, rs, ll


def backward_restated(shost, ms, rs, delta_T, xi):
    """Step k = T-1 .. 0: acc = 0, the K r_k chain, the Lb xi_k chain (xi None: left out), the J delta chain;
    paths[k] = m_k + delta_k.  paths[T] = m_T + delta_T.  ms (B, T+1, du), rs (B, T, dv), delta_T (B, du), xi (B, T, du)."""
    B, T1, du = ms.shape
    paths = np.empty_like(ms)
    delta = np.asarray(delta_T, f32)
    paths[:, T1 - 1] = (ms[:, T1 - 1] + delta).astype(f32)
    for k in range(T1 - 2, -1, -1):
        acc = chain(shost["K"][k], np.zeros((B, du), f32), rs[:, k])
        if xi is not None:
            acc = chain(shost["Lb"][k], acc, xi[:, k])
        delta = chain(shost["J"][k], acc, delta)
        paths[:, k] = (ms[:, k] + delta).astype(f32)
    return paths


def sample_on_restated(O, host, shost, kt, keys, vs):
    """fbsmi_kfs_sample_on -> dict(m (B, T+1, du), r (B, T, dv), loglik (B), paths (B, T+1, du))."""
    keys = np.asarray(keys, np.uint32).reshape(-1, 2)
    vs = np.asarray(vs, f32)
    ms, rs, ll = forward_restated(host, kt, vs)
    B, T1, du = ms.shape
    ks = [O.split(k, 3) for k in keys]                                     # key_fwd, key_bwd, key_kf
    uT = np.stack([draw_restated(O, host, k3[2], ms[b, -1]) for b, k3 in enumerate(ks)])
    xi = np.stack([O.normal(np.asarray(k3[1], np.uint32), (T1 - 1, du)) for k3 in ks]).astype(f32)
    paths = backward_restated(shost, ms, rs, (uT - ms[:, -1]).astype(f32), xi)
    paths[:, -1] = uT                                                      # stored as drawn
    return dict(m=ms, r=rs, loglik=ll, paths=paths)


def smooth_restated(host, shost, kt, vs):
    """fbsmi_kfs_smooth -> dict(m, r, loglik, smeans (B, T+1, du))."""
    ms, rs, ll = forward_restated(host, kt, np.asarray(vs, f32))
    smeans = backward_restated(shost, ms, rs, np.zeros((ms.shape[0], ms.shape[2]), f32), None)
    return dict(m=ms, r=rs, loglik=ll, smeans=smeans)


def want(O, om, host, shost, kt, keys, y0):
    """fbsmi_kfs_sample: the front of kf_restate.want, then sample_on_restated on its paths -> that dict plus vs."""
    keys = np.asarray(keys, np.uint32).reshape(-1, 2)
    vs = np.stack([O.lg_fwd_sampler(om, O.split(k, 3)[0], np.asarray(y0, f32))[::-1] for k in keys]).astype(f32)
    return dict(sample_on_restated(O, host, shost, kt, keys, vs), vs=vs)
