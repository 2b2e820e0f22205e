"""The fused SB bootstrap-filter conditional sampler (include/fbsmi.h, fbsmi_lg_fsamp_create_em) restated from the oracle's
primitives, sb_restate.em_path and fsamp_restate.ref_restated.  Not collected: the tests import it."""
import numpy as np

from fsamp_restate import ref_restated
from sb_restate import em_path

f32 = np.float32


def x0_restated(z, mean, chol):
    """mean + z @ chol in the header's order (elementwise numpy operations round separately): acc = z[0] * chol[0][j], then
    acc = acc + z[c] * chol[c][j] in ascending c, float32; x0 = mean + acc."""
    z, mean, chol = np.asarray(z, f32).reshape(-1), np.asarray(mean, f32).reshape(-1), np.asarray(chol, f32)
    acc = z[0] * chol[0, :]
    for c in range(1, z.size):
        acc = acc + z[c] * chol[c, :]
    return (mean + acc).astype(f32)


def keys_of(O, key):
    """-> key_x0, key_em, key_bf, key_init of one sample (sb/filter.py:138,153; smc.py:77)."""
    key_fwd, _key_bwd, key_bf = O.split(key, 3)
    key_x0, key_em = O.split(key_fwd, 2)
    return key_x0, key_em, key_bf, O.split(key_bf, 2)[0]


def want(O, om, em, tab, key, y0, n, resampling, x0_prior=None):
    """One conditional sample (sb/filter.py:137-161) -> (vs (T+1, dv), u0s (n, du), sample (du), nell).
    em = (M, c, ddt, s, nsub) float32 host tables; x0_prior = (mean, chol_lower) float32 or None."""
    M, c, ddt, s, nsub = em
    du = om.du
    key_x0, key_em, key_bf, key_init = keys_of(O, key)
    x0 = np.asarray(O.normal(key_x0, (du,)), f32).reshape(du)
    if x0_prior is not None:
        x0 = x0_restated(x0, *x0_prior)
    path = em_path(O, key_em, M, c, ddt, s, np.concatenate([x0, np.asarray(y0, f32).reshape(-1)]), om.T, nsub)
    vs = np.ascontiguousarray(path[::-1, du:])
    u0s = ref_restated(O, tab, key_init, vs[0], n)
    uT, nell = O.bootstrap_filter_lg(om, key_bf, vs, u0s, resampling, return_last=True)
    return vs, u0s, np.asarray(uT, f32).reshape(n, -1)[0].copy(), f32(nell)
