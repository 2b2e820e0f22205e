"""Numpy restatement of gibbs_kernel(marg_y=True) (fbs/samplers/gibbs.py:68-168) for the analytic model, composed from
the oracle's primitives the way tests/sb_restate.py composes the Schrodinger-bridge sweep: the forward path by
oracle.lg_fwd_sampler, the observation path re-drawn by oracle.doob_bridge_np (bridge_sampler, gibbs.py:17-20,130), the
conditional SMC by the oracle's forward pass, and the chain drivers' key schedule on top."""
import numpy as np

from sb_restate import _fwd_pass


def bridge_tables_by_hand(sde, ts, nsub):
    """The Doob bridge's coefficient tables (A, B, S [T * nsub], ddt [T]) in float64, the loop of
    tests/test_gpu_smc.py:189-195."""
    from fbs_amd.sdes.linear import _bridge_drift_coeffs
    ts = np.asarray(ts, np.float64)
    T = ts.size - 1
    A, B, S, ddt = np.zeros(T * nsub), np.zeros(T * nsub), np.zeros(T * nsub), np.zeros(T)
    for k in range(T):
        h = abs(ts[k + 1] - ts[k]) / nsub
        ddt[k] = h
        for j, t_ in enumerate(np.linspace(ts[k], ts[k + 1] - h, nsub)):
            A[k * nsub + j], B[k * nsub + j] = _bridge_drift_coeffs(sde, float(t_), float(ts[-1]))
            S[k * nsub + j] = float(sde.dispersion(float(t_)))
    return dict(nsub=nsub, A=A, B=B, S=S, ddt=ddt)


def bridge_vs(O, tab, key_bridge, y_first, y_last):
    """vs = reverse(bridge_sampler(key_bridge, y_first, y_last)) on the tables `tab` (float32 values), (T+1, dv)."""
    T = len(tab["ddt"])
    path = O.doob_bridge_np(key_bridge, tab["A"], tab["B"], tab["S"], tab["ddt"], y_first, y_last, T, tab["nsub"], True)
    return np.ascontiguousarray(path[::-1])


def gibbs_kernel_marg(O, om, tab, key, x0, y0, bs_star, nparticles, explicit_backward=True, explicit_final=False):
    """-> (x0_next, us_star_next, bs_next, acc, views) with views us_T, lw_T, us_star, vs."""
    T, du = om.T, om.du
    x0, y0 = np.asarray(x0, np.float32).reshape(du), np.asarray(y0, np.float32).reshape(om.dv)
    bs_star = np.asarray(bs_star, np.int32)
    key_fwd, key_csmc, key_bridge = O.split(key, 3)                                     # gibbs.py:126
    path = O.lg_fwd_sampler(om, key_fwd, np.concatenate([x0, y0]))                      # :127
    us = np.ascontiguousarray(path[::-1, :du])                                          # :129
    vs = bridge_vs(O, tab, key_bridge, path[0, du:], path[-1, du:])                     # :130, marg_y
    n = nparticles + 1 if explicit_final else nparticles
    if explicit_backward:
        k_fwd, k_x0, k_us, k_bs = O.split(key_csmc, 4)                                  # :147
    else:
        k_fwd, k_bwd = O.split(key_csmc, 2)                                             # csmc.py:65
    if explicit_final:                                                                  # :132-138
        us0 = O.normal(O.split(k_fwd, 2)[0], (n, du)).astype(np.float32)
        lw0 = None
    else:                                                                               # :139-144
        us0 = np.tile(us[0][None, :], (n, 1)).astype(np.float32)
        lw0 = np.full(n, -np.log(nparticles), np.float32)
    fw = _fwd_pass(O, om, k_fwd, us, bs_star, vs, us0, lw0, store=not explicit_backward)
    if explicit_backward:
        idx, _ = O.force_move(k_x0, O.exp(fw["lw_last"]), int(bs_star[-1]))             # :152
        x0n = fw["us_last"][idx]                                                        # :154
        usn = np.ascontiguousarray(O.lg_fwd_sampler(om, k_us, np.concatenate([x0n, y0]))[::-1, :du])  # :155
        bsn = O.randint(k_bs, (T + 1,), 0, nparticles)                                  # :156
    else:
        usn, bsn = O.backward_scanning_pass(k_bwd, fw["As"], fw["uss"], fw["lw_last"])  # csmc.py:75
    views = dict(us_T=fw["us_last"], lw_T=fw["lw_last"], us_star=us, vs=vs)
    return usn[-1], usn, bsn, bsn != bs_star, views


def gibbs_chain_marg(O, om, tab, key, x0s, y0, bs_stars, nparticles, nsweeps, explicit_backward=True,
                     explicit_final=False):
    """The drivers' key schedule: per sweep key, subkey = split(key); one chain sweeps with subkey
    (tests/test_gibbs.py:115-118), C > 1 chains with split(subkey, C)[c] (gp_gibbs.py:183-185).
    x0s (C, du), bs_stars (C, T+1) -> (key, x0s, bs_stars, samples (nsweeps, C, du))."""
    x0s = np.asarray(x0s, np.float32).reshape(-1, om.du).copy()
    bss = np.asarray(bs_stars, np.int32).reshape(-1, om.T + 1).copy()
    Cn = x0s.shape[0]
    out = np.zeros((nsweeps, Cn, om.du), np.float32)
    for i in range(nsweeps):
        key, subkey = O.split(key, 2)
        kc = O.split(subkey, Cn) if Cn > 1 else [subkey]
        for c in range(Cn):
            x0s[c], _, bss[c], _, _ = gibbs_kernel_marg(O, om, tab, kc[c], x0s[c], y0, bss[c], nparticles,
                                                        explicit_backward, explicit_final)
        out[i] = x0s
    return key, x0s, bss, out
