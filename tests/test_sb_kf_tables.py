"""CPU: the host side of the Kalman sampler and smoother of the Gaussian SB toy -- lg_kalman_tables / lg_smoother_tables on
sb_tables against dense joint-Gaussian conditioning of the whole discretised path, the float32 restatement
(tests/sb_kf_restate.py) against the float64 recursions, its front against the SB filter sampler's, the oracle's bootstrap
filter against the exact log-likelihood, the exports, the refusals and the argument checks of the two setters.  No device
is touched."""
import ctypes as C
import inspect

import numpy as np
import pytest

from fbs_amd.gaussian_sb import (SBKalman, SBKalmanSmoother, sb_kalman_conditional_sampler, sb_kalman_model,
                                 sb_kalman_path_sampler, sb_kalman_smoother_model)
import fsamp_restate as FR
import sb_fsamp_restate as FS
import sb_kf_restate as R
from sb_restate import sb_problem

f32 = np.float32
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
DENSE = [(1, 1, 6, 3), (3, 3, 20, 10), (5, 7, 8, 4), (7, 5, 8, 4), (20, 20, 12, 10)]
_MODELS = {}


def sb_model(du, dv, T, nsub):
    """The SB model of tests/test_gpu_sb_filter_sampler.py::_setup without a device: sb_problem cut to D = du + dv
    coordinates on ts = linspace(0, 1, T + 1), its float64 tables, y0 and a proper prior -> dict (shared by the tests)."""
    from fbs_amd.gaussian_sb import sb_tables
    from fbs_amd.lg_kalman import initial_cov, lg_kalman_tables, lg_smoother_tables
    from fbs_amd.linear_gaussian import lg_pmcmc_tables
    k = (du, dv, T, nsub)
    if k not in _MODELS:
        D = du + dv
        m0, c0, m1, c1 = sb_problem((D + 1) // 2, 0)
        ts = np.linspace(0.0, 1.0, T + 1)
        tab = sb_tables(m0[:D], c0[:D, :D], m1[:D], c1[:D, :D], ts, du, 1.0, nsub)
        pm = lg_pmcmc_tables(m1[:D], c1[:D, :D], du)
        kt = lg_kalman_tables(tab, pm, initial_cov(c1[:D, :D], du))
        st = lg_smoother_tables(tab, kt)
        rng = np.random.default_rng(1000 * du + dv)
        y0 = rng.normal(size=dv).astype(f32)
        A = rng.normal(size=(du, du))
        prior = (rng.normal(size=du).astype(f32), np.linalg.cholesky(A @ A.T / du + 0.5 * np.eye(du)).astype(f32))
        c32 = lambda a: np.ascontiguousarray(np.asarray(a, f32))
        _MODELS[k] = dict(tab=tab, pm=pm, kt=kt, st=st, y0=y0, prior=prior, T=T, du=du, dv=dv,
                          em=(c32(tab["M"]), c32(tab["c"]), c32(tab["ddt"]), c32(tab["s"]), nsub),
                          host={n: c32(kt[n]) for n in ("H", "e", "Pm", "c", "AK", "W", "lconst", "Lt")},
                          shost={n: c32(st[n]) for n in ("K", "J", "Lb")})
    return _MODELS[k]


def _oracle_model(O, tab):
    return O.LGModel(tab["du"], tab["dv"], f32(tab["dt"]), tab["G"], tab["g"], tab["sd"], tab["lognorm"], tab["F"], tab["sqQ"])


# ---- 1. the tables against dense conditioning ---------------------------------------------------------------------------
def _dense(tab, m0, Sig0, vs):
    """p(u_0..u_T | v_0..v_T) and log p(v_1..v_T | v_0) by conditioning the joint Gaussian of x = (u_0..u_T) on the stacked
    observations, no recursion over covariances (tests/test_kf_tables.py::_dense, every block kept): x is an affine map of
    independent unit normals, y_k = v_{k+1} - D v_k - e = C u_k + sd eps_k -> (means (T+1, du), covs (T+1, du, du), loglik)."""
    du, dv, dt = tab["du"], tab["dv"], tab["dt"]
    T, D = tab["G"].shape[0], du + dv
    n = (T + 1) * du
    mu, Phi = np.zeros((T + 1, du)), np.zeros((T + 1, du, n))
    mu[0], Phi[0][:, :du] = m0, np.linalg.cholesky(Sig0)
    Cbig, y, Rdiag = np.zeros((T * dv, n)), np.zeros(T * dv), np.zeros(T * dv)
    for k in range(T):
        M, gk, sd = np.eye(D) + dt * tab["G"][k], dt * tab["g"][k], tab["sd"][k]
        mu[k + 1] = M[:du, :du] @ mu[k] + M[:du, du:] @ vs[k] + gk[:du]
        Phi[k + 1] = M[:du, :du] @ Phi[k]
        Phi[k + 1][:, (k + 1) * du:(k + 2) * du] = sd * np.eye(du)
        Cbig[k * dv:(k + 1) * dv, k * du:(k + 1) * du] = M[du:, :du]
        y[k * dv:(k + 1) * dv] = vs[k + 1] - M[du:, du:] @ vs[k] - gk[du:]
        Rdiag[k * dv:(k + 1) * dv] = sd ** 2
    P = Phi.reshape(n, n)
    mean_x, cov_x = mu.reshape(n), P @ P.T
    Syy, Sxy = Cbig @ cov_x @ Cbig.T + np.diag(Rdiag), cov_x @ Cbig.T
    res = y - Cbig @ mean_x
    post_mean = mean_x + Sxy @ np.linalg.solve(Syy, res)
    post_cov = cov_x - Sxy @ np.linalg.solve(Syy, Sxy.T)
    loglik = -0.5 * (res @ np.linalg.solve(Syy, res) + np.linalg.slogdet(Syy)[1] + res.size * np.log(2 * np.pi))
    covs = np.stack([post_cov[k * du:(k + 1) * du, k * du:(k + 1) * du] for k in range(T + 1)])
    return post_mean.reshape(T + 1, du), covs, loglik


@pytest.mark.parametrize("case", DENSE, ids=["-".join(map(str, c)) for c in DENSE])
def test_tables_against_dense_conditioning(case):
    """cov_T, the filter's mean and loglik, cov_s and the smoothed means to 1e-12 relative (the bound of
    tests/test_kf_tables.py).  The smoothed law at k = T is the filtering law, so the filter's mean and cov_T are held to
    the last block of the dense posterior."""
    from fbs_amd.lg_kalman import kalman_filter_np, kalman_smoother_np
    du, dv, T, nsub = case
    m = sb_model(*case)
    tab, pm, kt, st = m["tab"], m["pm"], m["kt"], m["st"]
    assert kt["T"] == T and kt["H"].shape == (T, dv, du + dv) and st["J"].shape == (T, du, du)
    assert np.all(tab["F"] == 0) and np.all(tab["sqQ"] == 0)                            # the placeholders fbsmi_kf_create accepts
    assert np.array_equal(np.linalg.cholesky(kt["cov_0"]).astype(f32), pm["chol"])     # the matrix chol is rounded from
    rng = np.random.default_rng(3)
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())
    for trial in range(3):
        vs = rng.normal(size=(T + 1, dv))
        mT, ll = kalman_filter_np(kt, vs)
        sm, ms, rs, ll2 = kalman_smoother_np(kt, st, vs)
        m0 = kt["m_u"] + kt["gain"] @ (vs[0] - kt["m_v"])
        wm, wcov, wll = _dense(tab, m0, kt["cov_0"], vs)
        errs = dict(mean=rel(mT, wm[-1]), cov_T=rel(kt["cov_T"], wcov[-1]), loglik=abs(ll - wll) / abs(wll),
                    cov_s=rel(st["cov_s"], wcov), smeans=rel(sm, wm))
        print(f"{case} trial {trial}: relative differences " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert ll2 == ll and np.array_equal(ms[-1], mT)
        assert max(errs.values()) <= 1e-12, errs


# ---- 2. the float32 restatement against the float64 recursions -----------------------------------------------------------
NKEYS = 3
_WANT = {}


def restated(O, case, proper=False):
    """The restatement's batch of a model on its keys (computed once and shared: sample b depends on keys[b] only)."""
    k = (case, proper)
    if k not in _WANT:
        m = sb_model(*case)
        keys = O.split(O.PRNGKey(61), NKEYS)
        _WANT[k] = (keys, R.want(O, m["em"], m["host"], m["shost"], m["kt"], keys, m["y0"], m["prior"] if proper else None))
    return _WANT[k]


@pytest.mark.parametrize("case", DENSE + [(33, 32, 4, 3)], ids=["-".join(map(str, c)) for c in DENSE + [(33, 32, 4, 3)]])
def test_restatement_against_float64(case, oracle):
    """Filtering means to 1e-5 of max |m|, loglik to 1e-5 relative, the drawn paths to 1e-5 of max |path| against the float64
    recursions on the same observation paths and noise (the bound of tests/test_kf_tables.py).  Largest figures measured:
    means 6.0e-7 ((33,32,4,3)), paths 4.3e-7 ((20,20,12,10)), loglik 8.95e-6 ((3,3,20,10): a log-likelihood of -0.112, off by
    1.0e-6 absolute; at most 2.4e-7 on the other models)."""
    from fbs_amd.lg_kalman import kalman_filter_np, kalman_smoother_np
    du, dv, T, nsub = case
    m = sb_model(*case)
    keys, w = restated(oracle, case)
    assert w["vs"].shape == (NKEYS, T + 1, dv) and w["paths"].shape == (NKEYS, T + 1, du)
    assert np.array_equal(w["sloglik"].view(np.uint32), w["loglik"].view(np.uint32))
    assert np.array_equal(w["paths"][:, T].view(np.uint32), w["samples"].view(np.uint32))
    worst = dict(means=0.0, loglik=0.0, paths=0.0)
    for b in range(NKEYS):
        vs64 = w["vs"][b].astype(np.float64)
        m64, ll64 = kalman_filter_np(m["kt"], vs64)
        k3 = oracle.split(keys[b], 3)
        zz = oracle.normal(k3[2], (du,)).astype(np.float64)
        xi = oracle.normal(k3[1], (T, du)).astype(np.float64)
        p64 = kalman_smoother_np(m["kt"], m["st"], vs64, noise=(zz, xi))[0]
        worst["means"] = max(worst["means"], float(np.abs(w["means"][b] - m64).max() / np.abs(m64).max()))
        worst["loglik"] = max(worst["loglik"], abs(float(w["loglik"][b]) - ll64) / abs(ll64))
        worst["paths"] = max(worst["paths"], float(np.abs(w["paths"][b] - p64).max() / np.abs(p64).max()))
    print(f"{case}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + " of the float64 scale")
    assert np.isfinite(w["samples"]).all() and max(worst.values()) <= 1e-5, worst


# ---- 3. the front is the SB filter sampler's -------------------------------------------------------------------------------
@pytest.mark.parametrize("proper", [False, True])
def test_restated_front_is_the_filter_samplers(proper, oracle):
    """Keys and vs of the restated front equal those of tests/sb_fsamp_restate.py, bit for bit."""
    case = (3, 3, 20, 10)
    m = sb_model(*case)
    prior = m["prior"] if proper else None
    keys, w = restated(oracle, case, proper)
    om = _oracle_model(oracle, m["tab"])
    for b in range(NKEYS):
        key_x0, key_em, key_bwd, key_kf, vs = R.front_restated(oracle, m["em"], 3, 20, keys[b], m["y0"], prior)
        fx0, fem, fbf, _ = FS.keys_of(oracle, keys[b])
        k3 = oracle.split(keys[b], 3)
        assert np.array_equal(key_x0, fx0) and np.array_equal(key_em, fem)
        assert np.array_equal(key_kf, fbf) and np.array_equal(key_kf, k3[2]) and np.array_equal(key_bwd, k3[1])
        fvs = FS.want(oracle, om, m["em"], m["pm"], keys[b], m["y0"], 8, "stratified", prior)[0]
        assert np.array_equal(vs.view(np.uint32), fvs.view(np.uint32))
        assert np.array_equal(w["vs"][b].view(np.uint32), fvs.view(np.uint32))
        assert np.array_equal(w["vs"][b][20], m["y0"])
    if proper:
        assert not np.array_equal(w["vs"], restated(oracle, case, False)[1]["vs"])


# ---- 4. the oracle's bootstrap filter against the exact log-likelihood ------------------------------------------------------
@pytest.mark.parametrize("case", [(1, 1, 6, 3), (3, 3, 20, 10)], ids=["1-1-6-3", "3-3-20-10"])
def test_oracle_filter_against_the_exact_loglikelihood(case, oracle):
    from fbs_amd.lg_kalman import kalman_filter_np
    du, dv, T, nsub = case
    m = sb_model(*case)
    om = _oracle_model(oracle, m["tab"])
    vs = R.front_restated(oracle, m["em"], du, T, oracle.PRNGKey(99), m["y0"])[4]
    loglik = kalman_filter_np(m["kt"], vs.astype(np.float64))[1]
    N, keys = 4096, oracle.split(oracle.PRNGKey(17), 24)
    est = []
    for key in keys:
        u0s = FR.ref_restated(oracle, m["pm"], oracle.split(key, 2)[0], vs[0], N)
        est.append(-float(oracle.bootstrap_filter_lg(om, key, vs, u0s, "stratified", return_last=True)[1]))
    est = np.array(est)
    se = est.std(ddof=1) / np.sqrt(len(est))
    print(f"{case}: mean(-nell) - loglik = {est.mean() - loglik:+.2e}, sd {est.std(ddof=1):.4f}, standard error {se:.4f}")
    assert abs(est.mean() - loglik) <= 4 * se


# ---- 5. exports, refusals, the setters' argument checks -----------------------------------------------------------------------
def test_exports_and_refusals():
    import fbs_amd
    from fbs_amd import gaussian_sb as G, lg_kalman as K, samplers
    from fbs_amd.linear_gaussian import LinearGaussianBridge
    for name in ("sb_kalman_conditional_sampler", "sb_kalman_path_sampler"):
        assert getattr(samplers, name) is getattr(G, name) is getattr(fbs_amd, name) and name in fbs_amd.__all__
        assert list(inspect.signature(getattr(G, name)).parameters) == ["keys", "y0", "bridge", "x0_prior", "return_moments",
                                                                        "_bound"]
        assert inspect.signature(getattr(G, name)).parameters["_bound"].default == K.KF_PATH_ELEMS
    assert fbs_amd.SBKalman is G.SBKalman is SBKalman and fbs_amd.SBKalmanSmoother is G.SBKalmanSmoother is SBKalmanSmoother
    assert samplers.sb_kalman_conditional_sampler is sb_kalman_conditional_sampler
    assert samplers.sb_kalman_path_sampler is sb_kalman_path_sampler
    assert G.sb_kalman_model is sb_kalman_model and G.sb_kalman_smoother_model is sb_kalman_smoother_model
    assert list(inspect.signature(sb_kalman_model).parameters) == list(inspect.signature(sb_kalman_smoother_model).parameters) == ["bridge"]
    assert issubclass(G.SBKalman, K.LGKalman) and issubclass(G.SBKalmanSmoother, K.LGKalmanSmoother)
    assert G.SBKalman._DESTROY == "fbsmi_kf_destroy" and G.SBKalmanSmoother._DESTROY == "fbsmi_kfs_destroy"
    for name in ("sb_kalman_handle", "sb_kalman_smoother_handle"):
        assert list(inspect.signature(getattr(G.GaussianSBBridge, name)).parameters) == ["self", "nsamples", "x0_prior"]
        assert not hasattr(LinearGaussianBridge, name)
    # gaussian_sb imports lg_kalman, never the reverse
    assert "gaussian_sb" not in [ln.split()[1] for ln in inspect.getsource(K).splitlines() if ln.startswith(("from .", "import "))]
    keys, y0 = np.zeros((1, 2), np.uint32), np.zeros(1, f32)
    sb = object.__new__(G.GaussianSBBridge)                    # no device behind either: refused on the type alone
    lg = object.__new__(LinearGaussianBridge)
    for old in (lambda: K.kalman_conditional_sampler(keys, y0, sb), lambda: K.kalman_path_sampler(keys, y0, sb),
                lambda: K.kalman_model(sb), lambda: K.kalman_smoother_model(sb), lambda: K.LGKalman(sb, 1),
                lambda: K.LGKalmanSmoother(sb, 1), lambda: sb.kalman_handle(1), lambda: sb.kalman_smoother_handle(1)):
        sb._sweeps = {}
        with pytest.raises(NotImplementedError, match="GaussianSBBridge"):
            old()
    for new in (lambda: G.sb_kalman_conditional_sampler(keys, y0, lg), lambda: G.sb_kalman_path_sampler(keys, y0, lg),
                lambda: G.sb_kalman_model(lg), lambda: G.sb_kalman_smoother_model(lg), lambda: G.SBKalman(lg, 1),
                lambda: G.SBKalmanSmoother(lg, 1)):
        with pytest.raises(NotImplementedError, match="LinearGaussianBridge"):
            new()


def test_setters_refuse_null_arguments():
    """fbsmi_kf_set_em_forward / fbsmi_kfs_set_em_forward: FBSMI_ERR_ARG naming the function for a null handle or tables,
    nsub < 1 and exactly one of mean and chol, all answered before the handle is read or a device call made."""
    from fbs_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(64)                       # a non-NULL pointer; never dereferenced
    p = C.addressof(buf)
    good = _lib.EMForwardStruct(3, p, p, p, p)
    for fn, name in ((L.fbsmi_kf_set_em_forward, b"kf_set_em_forward"), (L.fbsmi_kfs_set_em_forward, b"kfs_set_em_forward")):
        bad = [(None, C.byref(good), None, None), (p, None, None, None), (p, C.byref(_lib.EMForwardStruct(0, p, p, p, p)), None, None),
               (p, C.byref(_lib.EMForwardStruct(-2, p, p, p, p)), p, p), (p, C.byref(good), p, None), (p, C.byref(good), None, p)]
        bad += [(p, C.byref(_lib.EMForwardStruct(3, *(None if i == j else p for i in range(4)))), None, None) for j in range(4)]
        for args in bad:
            assert fn(*args) == ERR_ARG and name in L.fbsmi_last_error(), (name, args, L.fbsmi_last_error())
    with pytest.raises(RuntimeError, match="kf_set_em_forward"):
        _lib.call("fbsmi_kf_set_em_forward", None, C.byref(good), None, None)
