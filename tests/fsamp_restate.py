"""The fused bootstrap-filter conditional sampler (include/fbsmi.h, fbsmi_lg_fsamp) restated from the oracle's primitives.
Not collected: the tests import it."""
import numpy as np

f32 = np.float32


def ref_restated(O, tab, key, yT, n):
    """ref_sampler in the order include/fbsmi.h specifies (elementwise numpy operations round separately): the conditional
    mean in float64 in ascending c, the product with the lower factor in float32 in ascending c, u0 = m_ + acc.
    tab: lg_pmcmc_tables' m_u (du), m_v (dv), gain (du, dv) float64 and chol (du, du) float32."""
    chol = np.asarray(tab["chol"], f32)
    du = chol.shape[0]
    y = np.asarray(yT, f32).astype(np.float64).reshape(-1)
    m = np.empty(du, f32)
    for j in range(du):
        s = np.float64(0.0)
        for c in range(y.size):
            s = s + tab["gain"][j, c] * (y[c] - tab["m_v"][c])
        m[j] = f32(tab["m_u"][j] + s)
    z = O.normal(key, (n, du))
    acc = z[:, 0:1] * chol[0:1, :]
    for c in range(1, du):
        acc = acc + z[:, c:c + 1] * chol[c:c + 1, :]
    return (m[None, :] + acc).astype(f32)


def want(O, om, tab, key, y0, n, resampling):
    """One conditional sample (gp_filter.py:134-142, smc.py:76-79) -> (vs (T+1, dv), u0s (n, du), sample (du), nell)."""
    key_fwd, _key_bwd, key_bf = O.split(key, 3)
    vs = O.lg_fwd_sampler(om, key_fwd, np.asarray(y0, f32))[::-1].copy()
    key_init = O.split(key_bf, 2)[0]
    u0s = ref_restated(O, tab, key_init, vs[0], n)
    uT, nell = O.bootstrap_filter_lg(om, key_bf, vs, u0s, resampling, return_last=True)
    return vs, u0s, np.asarray(uT, f32).reshape(n, -1)[0].copy(), f32(nell)
