"""Numpy restatements for the Gaussian Schrodinger-bridge tests: an exact float32 fmaf, the matrix-affine Euler-Maruyama
path of include/fbsmi.h (fbsmi_em_forward) and gibbs_kernel (fbs/samplers/gibbs.py:68-168) on it, composed from the
oracle's C primitives the way oracle.gibbs_kernel_lg_marg_y is."""
import ctypes

import numpy as np


def fmaf(a, b, c):
    """Correctly rounded float32 a*b + c, elementwise.  a*b is exact in float64; the float64 sum t plus its TwoSum residual e
    is the exact result, and rounding t to float32 is then correct except where t lies exactly halfway between two float32
    values and e != 0: there e breaks the tie."""
    a64, b64, c64 = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a64 * b64
    t = p + c64
    bb = t - p
    e = (p - (t - bb)) + (c64 - bb)
    r = t.astype(np.float32)
    r64 = r.astype(np.float64)
    other = np.nextafter(r, np.where(t > r64, np.float32(np.inf), np.float32(-np.inf))).astype(np.float64)
    tie = (t != r64) & (t == (r64 + other) * 0.5) & (e != 0)
    if np.any(tie):
        nudged = np.nextafter(t, np.where(e > 0, np.inf, -np.inf)).astype(np.float32)
        r = np.where(tie, nudged, r)
    return np.asarray(r, np.float32)


def em_path(O, key, M, c, ddt, s, x0, T, nsub):
    """out (T+1, D): out[0] = x0; sub-step r = k*nsub + j: f = c[r] + sum_c M[r][:, c] x_c (fmaf chain in c order),
    x = (x + f ddt[k]) + s[r] xi_k[j], xi_k = normal(split(key, T)[k], (nsub, D))."""
    x = np.asarray(x0, np.float32).reshape(-1).copy()
    D = x.size
    out = np.zeros((T + 1, D), np.float32)
    out[0] = x
    keys = O.split(key, T)
    for k in range(T):
        z = O.normal(keys[k], (nsub, D))
        h = np.float32(ddt[k])
        for j in range(nsub):
            r = k * nsub + j
            f = np.asarray(c[r], np.float32).copy()
            for col in range(D):
                f = fmaf(M[r][:, col], np.full(D, x[col], np.float32), f)
            x = (x + f * h) + np.float32(s[r]) * z[j]
        out[k + 1] = x
    return out


_raw = {}


def _fwd_pass(O, om, key, us, bs, vs, us0, lw0, store):
    """oracle.csmc_forward_pass_lg with lw0 = None allowed (explicit_final: the initial weights come from the model)."""
    if "fp" not in _raw:
        L = ctypes.CDLL(O._SO)   # a handle of its own: argument types that let lw0 be NULL
        fn = L.orc_csmc_forward_pass_lg
        fn.argtypes = [ctypes.POINTER(O.LGStruct)] + [ctypes.c_void_p] * 6 + [ctypes.c_int32, ctypes.c_int] + \
            [ctypes.c_void_p] * 5
        _raw["fp"] = fn
    n = us0.shape[0]
    keep = lambda a: np.ascontiguousarray(a)
    key, us, bs, vs, us0 = keep(np.asarray(key, np.uint32)), keep(us), keep(np.asarray(bs, np.int32)), keep(vs), keep(us0)
    As = np.zeros((om.T, n), np.int32) if store else None
    uss = np.zeros((om.T + 1, n, om.du), np.float32) if store else None
    us_last, lw_last = np.zeros((n, om.du), np.float32), np.zeros(n, np.float32)
    p = lambda a: None if a is None else a.ctypes.data
    _raw["fp"](ctypes.byref(om.struct), p(key), p(us), p(bs), p(vs), p(us0), p(lw0), n, 0, p(As), None, p(uss),
               p(us_last), p(lw_last))
    return dict(As=As, uss=uss, us_last=us_last, lw_last=lw_last)


def gibbs_kernel_sb(O, om, em, key, x0, y0, bs_star, nparticles, explicit_backward, explicit_final):
    """-> (x0_next, us_star_next, bs_next, acc, views) with views us_T, lw_T, us_star, vs.  em = (M, c, ddt, s, nsub)."""
    M, c, ddt, s, nsub = em
    T, du = om.T, om.du
    x0, y0 = np.asarray(x0, np.float32).reshape(du), np.asarray(y0, np.float32).reshape(om.dv)
    bs_star = np.asarray(bs_star, np.int32)
    path_of = lambda k, z0: em_path(O, k, M, c, ddt, s, z0, T, nsub)
    key_fwd, key_csmc, _ = O.split(key, 3)                                              # gibbs.py:126
    path = path_of(key_fwd, np.concatenate([x0, y0]))                                   # :127
    us = np.ascontiguousarray(path[::-1, :du])                                          # :129
    vs = np.ascontiguousarray(path[::-1, du:])                                          # :130
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
        usn = np.ascontiguousarray(path_of(k_us, np.concatenate([x0n, y0]))[::-1, :du])  # :155
        bsn = O.randint(k_bs, (T + 1,), 0, nparticles)                                  # :156
    else:
        usn, bsn = O.backward_scanning_pass(k_bwd, fw["As"], fw["uss"], fw["lw_last"])  # csmc.py:75
    views = dict(us_T=fw["us_last"], lw_T=fw["lw_last"], us_star=us, vs=vs)
    return usn[-1], usn, bsn, bsn != bs_star, views


def sb_problem(d, seed=0):
    """The SB toy's marginals (experiments/sb/gibbs.py:27-67): the joint GP prior of (x, y) on linspace(0, 5, d) with
    observation noise 0.1, and a random Gaussian reference N(1, a a^T) (kept away from singular)."""
    zs = np.linspace(0., 5., d)
    cov = np.exp(-np.abs(zs[None, :] - zs[:, None]))
    joint = np.block([[cov, cov], [cov, cov + 0.1 * np.eye(d)]])
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(2 * d, 2 * d))
    return np.zeros(2 * d), joint, np.ones(2 * d), a @ a.T / (2 * d) + 0.5 * np.eye(2 * d)
