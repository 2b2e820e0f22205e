"""The fused Kalman sampler and smoother of the Gaussian SB toy (include/fbsmi.h, fbsmi_kf_set_em_forward) restated from
four existing pieces: the front of tests/sb_fsamp_restate.py (keys_of, x0_restated), sb_restate.em_path,
kf_restate.filter_restated / draw_restated and kfs_restate.sample_on_restated.  Not collected: the tests import it."""
import numpy as np

import kf_restate as KR
import kfs_restate as SR
from sb_fsamp_restate import keys_of, x0_restated
from sb_restate import em_path

f32 = np.float32


def front_restated(O, em, du, T, key, y0, x0_prior=None):
    """One sample's keys and observation path (sb/filter.py:137-148): -> (key_x0, key_em, key_bwd, key_kf, vs (T+1, dv)).
    em = (M, c, ddt, s, nsub) float32 host tables; x0_prior = (mean, chol_lower) float32 or None."""
    M, c, ddt, s, nsub = em
    key_x0, key_em, key_kf, _ = keys_of(O, key)                             # (keys_of's key_bf is split(key, 3)[2])
    key_bwd = O.split(key, 3)[1]
    x0 = np.asarray(O.normal(key_x0, (du,)), f32).reshape(du)
    if x0_prior is not None:
        x0 = x0_restated(x0, *x0_prior)
    path = em_path(O, key_em, M, c, ddt, s, np.concatenate([x0, np.asarray(y0, f32).reshape(-1)]), T, nsub)
    return key_x0, key_em, key_bwd, key_kf, np.ascontiguousarray(path[::-1, du:]).astype(f32)


def want(O, em, host, shost, kt, keys, y0, x0_prior=None):
    """The batch -> dict(vs (B, T+1, dv), m_ (B, du), means (B, du), loglik (B), samples (B, du)) of fbsmi_kf_sample and
    (shost not None) m (B, T+1, du), r (B, T, dv), paths (B, T+1, du) of fbsmi_kfs_sample on the same keys."""
    keys = np.asarray(keys, np.uint32).reshape(-1, 2)
    du, T = host["c"].shape[1], host["c"].shape[0]
    fronts = [front_restated(O, em, du, T, k, y0, x0_prior) for k in keys]
    vs = np.stack([f[4] for f in fronts])
    m0, mT, ll = KR.filter_restated(host, kt, vs)
    samples = np.stack([KR.draw_restated(O, host, f[3], mT[b]) for b, f in enumerate(fronts)])
    out = dict(vs=vs, m_=m0, means=mT, loglik=ll, samples=samples)
    if shost is not None:
        s = SR.sample_on_restated(O, host, shost, kt, keys, vs)
        out.update(m=s["m"], r=s["r"], paths=s["paths"], sloglik=s["loglik"])
    return out
