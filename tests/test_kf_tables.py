"""CPU: the host side of the Kalman-filter conditional sampler -- lg_kalman_tables against dense joint-Gaussian conditioning,
the float32 restatement of the header's specification (tests/kf_restate.py) against the float64 recursion, the oracle's
bootstrap filter against the exact log-likelihood, fbsmi_kf_create's argument checks and the chunk planner.  No device is
touched."""
import ctypes as C

import numpy as np
import pytest

from helpers import toy_2d, toy_31, toy_4d, toy_gp, toy_rand
import fsamp_restate as FR
import kf_restate as R

f32 = np.float32
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
TOYS = {"2d": toy_2d, "4d": toy_4d, "31": toy_31}
# the width ladder of k_kf, on ts = linspace(0, 2, 7): square models on either side of the 16-row tiles and of the
# 64-column edge, and rectangular ones whose (NQu, NQv) differ, dv > du among them
SQUARE = {f"gp{d}": (lambda d=d: toy_gp(d)) for d in (16, 48, 63, 64, 65, 80, 96, 112)}
RECT = {"gp128v1": lambda: toy_gp(128, dv=1), "gp80v33": lambda: toy_gp(80, dv=33), "rand5v40": lambda: toy_rand(5, 40),
        "rand33v80": lambda: toy_rand(33, 80), "rand17v96": lambda: toy_rand(17, 96), "rand5v128": lambda: toy_rand(5, 128)}
LADDER = {**SQUARE, **RECT}
LADDER_TILES = {"gp128v1": (8, 1), "gp80v33": (5, 3), "rand5v40": (1, 3), "rand33v80": (3, 5), "rand17v96": (2, 6),
                "rand5v128": (1, 8)}
LADDER_TS = np.linspace(0, 2, 7)
DENSE = {**TOYS, **RECT, "gp48": SQUARE["gp48"]}


def ladder_keys(O, n=17):
    """The keys of the ladder's samples (those of tests/test_gpu_kf.py)."""
    return O.split(O.PRNGKey(51), 33)[:n]


def _tables(toy, ts):
    """(lg_tables, lg_pmcmc_tables, lg_kalman_tables) of a toy on the grid ts, float64, const SDE (-0.5, 1)."""
    from fbs_amd.lg_kalman import initial_cov, lg_kalman_tables
    from fbs_amd.linear_gaussian import lg_pmcmc_tables, lg_tables
    from fbs_amd.sdes import StationaryConstLinearSDE
    from fbs_amd.sdes.linear import discretise_linear_sde_np
    sde = StationaryConstLinearSDE(-0.5, 1.0)
    tab = lg_tables(toy["m0"], toy["cov0"], sde, ts, toy["du"])
    Ft, Qt = discretise_linear_sde_np(sde, ts[-1], ts[0])
    cov_ref = Ft ** 2 * np.asarray(toy["cov0"], np.float64) + Qt * np.eye(len(toy["m0"]))
    pm = lg_pmcmc_tables(Ft * np.asarray(toy["m0"], np.float64), cov_ref, toy["du"])
    return tab, pm, lg_kalman_tables(tab, pm, initial_cov(cov_ref, toy["du"]))


def _oracle_model(O, tab):
    return O.LGModel(tab["du"], tab["dv"], f32(tab["dt"]), tab["G"], tab["g"], tab["sd"], tab["lognorm"], tab["F"], tab["sqQ"])


def _host32(kt):
    return {k: np.ascontiguousarray(np.asarray(kt[k], f32)) for k in ("H", "e", "Pm", "c", "AK", "W", "lconst", "Lt")}


# ---- 1. the tables against dense conditioning ---------------------------------------------------------------------------
def _dense(tab, m0, Sig0, vs):
    """p(u_T | v_0..v_T) and log p(v_1..v_T | v_0) by conditioning the joint Gaussian of x = (u_0..u_T) on the stacked
    observations, no recursion over covariances: x is an affine map of independent unit normals (u_0 = m0 + L0 w_0,
    u_{k+1} = A u_k + B v_k + c + sd w_{k+1}), y_k = v_{k+1} - D v_k - e = C u_k + sd eps_k."""
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
    return post_mean[-du:], post_cov[-du:, -du:], loglik


@pytest.mark.parametrize("name", sorted(TOYS) + sorted(set(DENSE) - set(TOYS)))
def test_tables_against_dense_conditioning(name):
    from fbs_amd.lg_kalman import kalman_filter_np
    toy, ts = DENSE[name](), np.linspace(0, 2, 7)
    tab, pm, kt = _tables(toy, ts)
    assert kt["T"] == 6 and kt["H"].shape == (6, kt["dv"], kt["du"] + kt["dv"]) and kt["AK"].shape == (6, kt["du"], kt["dv"])
    assert np.array_equal(np.linalg.cholesky(kt["cov_0"]).astype(f32), pm["chol"])     # the matrix chol is rounded from
    assert np.allclose(kt["Lt"].T @ kt["Lt"], kt["cov_T"], rtol=0, atol=1e-14) and np.all(np.triu(kt["Lt"]) == kt["Lt"])
    rng = np.random.default_rng(3)
    for trial in range(3):
        vs = rng.normal(size=(7, kt["dv"]))
        m, ll = kalman_filter_np(kt, vs)
        m0 = kt["m_u"] + kt["gain"] @ (vs[0] - kt["m_v"])
        wm, wcov, wll = _dense(tab, m0, kt["cov_0"], vs)
        errs = (np.abs(m - wm).max() / np.abs(wm).max(), np.abs(kt["cov_T"] - wcov).max() / np.abs(wcov).max(),
                abs(ll - wll) / abs(wll))
        print(f"{name} trial {trial}: relative differences mean {errs[0]:.2e} cov {errs[1]:.2e} loglik {errs[2]:.2e}")
        assert max(errs) <= 1e-12, errs


# ---- 2. the float32 restatement against the float64 recursion -------------------------------------------------------------
def test_restatement_against_float64_at_the_drivers_shape(oracle):
    from fbs_amd.lg_kalman import kalman_filter_np
    toy, ts = toy_gp(100), np.linspace(0, 1, 201)
    tab, pm, kt = _tables(toy, ts)
    om = _oracle_model(oracle, tab)
    keys = oracle.split(oracle.PRNGKey(7), 2)
    w = R.want(oracle, om, _host32(kt), kt, keys, toy["y0"])
    assert w["vs"].shape == (2, 201, 100) and w["samples"].shape == w["means"].shape == (2, 100)
    for b in range(2):
        m64, ll64 = kalman_filter_np(kt, w["vs"][b].astype(np.float64))
        em = np.abs(w["means"][b] - m64).max()
        el = abs(float(w["loglik"][b]) - ll64) / abs(ll64)
        print(f"sample {b}: |mean - float64| = {em:.2e} (scale {np.abs(m64).max():.2f}), loglik relative {el:.2e}")
        assert em <= 1e-5 * np.abs(m64).max() and el <= 1e-5
        # the draw is the mean plus zz @ chol of the exact covariance
        zz = oracle.normal(oracle.split(keys[b], 3)[2], (100,)).astype(np.float64)
        x64 = m64 + zz @ kt["Lt"]
        assert np.abs(w["samples"][b] - x64).max() <= 1e-5 * np.abs(x64).max()


@pytest.mark.parametrize("name", list(LADDER))
def test_restatement_against_float64_across_the_width_ladder(name, oracle):
    """Means to 1e-5 of max |m|, loglik to 1e-5 relative, 17 keys, T = 6, at every model of the ladder.  (No du = 1 here:
    max |m| is then one coordinate, which can sit near zero.)  Largest figures measured: means 1.4e-6 (rand5v128), loglik 1.6e-7 (rand33v80)."""
    from fbs_amd.lg_kalman import kalman_filter_np
    toy = LADDER[name]()
    tab, pm, kt = _tables(toy, LADDER_TS)
    du, dv = kt["du"], kt["dv"]
    if name in LADDER_TILES:
        assert ((du + 15) // 16, (dv + 15) // 16) == LADDER_TILES[name]
    w = R.want(oracle, _oracle_model(oracle, tab), _host32(kt), kt, ladder_keys(oracle), toy["y0"])
    assert w["vs"].shape == (17, 7, dv) and w["samples"].shape == w["means"].shape == (17, du)
    worst_m = worst_l = 0.0
    for b in range(17):
        m64, ll64 = kalman_filter_np(kt, w["vs"][b].astype(np.float64))
        worst_m = max(worst_m, float(np.abs(w["means"][b] - m64).max() / np.abs(m64).max()))
        worst_l = max(worst_l, abs(float(w["loglik"][b]) - ll64) / abs(ll64))
    print(f"{name} (du {du}, dv {dv}): means {worst_m:.2e} of max |m|, loglik {worst_l:.2e} relative")
    assert np.isfinite(w["samples"]).all() and worst_m <= 1e-5 and worst_l <= 1e-5


def test_restatement_feels_one_ulp_in_the_last_row_and_column_of_the_u_block(oracle):
    """toy_gp(80, dv=33): one ulp on Pm[5][79][79] (row tile 4 -- the second tile of wave 0 alone -- and column group 4, in
    the last step, whose row 79 feeds mean 79 and nothing else) changes the restated means in coordinate 79 only, so a
    comparison with the restatement reaches that row and column.  Measured: 4 of the 17 samples change."""
    toy = LADDER["gp80v33"]()
    tab, pm, kt = _tables(toy, LADDER_TS)
    om, host, keys = _oracle_model(oracle, tab), _host32(kt), ladder_keys(oracle)
    w = R.want(oracle, om, host, kt, keys, toy["y0"])
    Pm = host["Pm"].copy()
    Pm[5, 79, 79] = np.nextafter(Pm[5, 79, 79], f32(np.inf))
    assert Pm[5, 79, 79] != host["Pm"][5, 79, 79]
    wb = R.want(oracle, om, dict(host, Pm=Pm), kt, keys, toy["y0"])
    assert np.array_equal(wb["vs"].view(np.uint32), w["vs"].view(np.uint32))            # the path does not read Pm
    changed = np.argwhere(wb["means"].view(np.uint32) != w["means"].view(np.uint32))
    print(f"one ulp on Pm[5][79][79]: means changed at (sample, coordinate) {changed.tolist()}")
    assert len(changed) >= 1 and np.all(changed[:, 1] == 79)


def test_restated_front_is_the_filter_samplers(oracle):
    """vs and m_0 are fbsmi_lg_fsamp's: the restatement and tests/fsamp_restate.py agree bit for bit."""
    toy, ts = toy_4d(), np.linspace(0, 2, 31)
    tab, pm, kt = _tables(toy, ts)
    om = _oracle_model(oracle, tab)
    keys = oracle.split(oracle.PRNGKey(5), 3)
    w = R.want(oracle, om, _host32(kt), kt, keys, toy["y0"])
    for b in range(3):
        vs, u0s, _, _ = FR.want(oracle, om, pm, keys[b], toy["y0"], 1, "stratified")
        assert np.array_equal(w["vs"][b].view(np.uint32), vs.view(np.uint32))
        # ref_restated's particle is m_ + z @ chol: with chol = 0 it is the conditional mean itself
        m_ = FR.ref_restated(oracle, dict(pm, chol=np.zeros_like(pm["chol"])), keys[b], vs[0], 1)[0]
        assert np.array_equal(w["m_"][b].view(np.uint32), m_.view(np.uint32))


# ---- 3. a known answer for the existing filter ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d", "4d"])
def test_oracle_filter_against_the_exact_loglikelihood(name, oracle):
    from fbs_amd.lg_kalman import kalman_filter_np
    toy, ts = TOYS[name](), np.linspace(0, 2, 31)
    tab, pm, kt = _tables(toy, ts)
    om = _oracle_model(oracle, tab)
    vs = oracle.lg_fwd_sampler(om, oracle.PRNGKey(99), toy["y0"])[::-1].copy()
    loglik = kalman_filter_np(kt, vs.astype(np.float64))[1]
    N, keys = 4096, oracle.split(oracle.PRNGKey(17), 24)
    est = []
    for key in keys:
        u0s = FR.ref_restated(oracle, pm, oracle.split(key, 2)[0], vs[0], N)
        est.append(-float(oracle.bootstrap_filter_lg(om, key, vs, u0s, "stratified", return_last=True)[1]))
    est = np.array(est)
    se = est.std(ddof=1) / np.sqrt(len(est))
    print(f"{name}: mean(-nell) - loglik = {est.mean() - loglik:+.2e}, sd {est.std(ddof=1):.4f}, standard error {se:.4f}")
    assert abs(est.mean() - loglik) <= 4 * se


# ---- 4. argument checks of fbsmi_kf_create: answered before any device call ---------------------------------------------------
def test_kf_create_validation():
    from fbs_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(64)                       # a non-NULL pointer; never dereferenced
    p = C.addressof(buf)
    names = [n for n, _ in _lib.KFModelStruct._fields_[3:]]
    assert names == ["H", "e", "Pm", "c", "AK", "W", "lconst", "Lt", "F", "sqQ", "m_u", "m_v", "gain"]

    def create(du=2, dv=2, T=4, nsamples=1, null=None, model=True):
        st = _lib.KFModelStruct(du, dv, T, *(None if n == null else p for n in names))
        h = C.c_void_p()
        rc = L.fbsmi_kf_create(C.byref(st) if model else None, nsamples, C.byref(h))
        assert not h.value
        return rc, L.fbsmi_last_error()

    for kw in [dict(model=False), dict(T=0)] + [dict(null=n) for n in names]:
        rc, msg = create(**kw)
        assert rc == ERR_ARG and b"kf_create" in msg, (kw, rc, msg)
    for kw in [dict(du=0), dict(du=129), dict(dv=0), dict(dv=129), dict(du=-1), dict(nsamples=0), dict(nsamples=65536),
               dict(nsamples=-3)]:
        rc, msg = create(**kw)
        assert rc == ERR_UNSUPPORTED and b"kf_create" in msg and b"128" in msg and b"65535" in msg, (kw, rc, msg)
    with pytest.raises(NotImplementedError, match="65535"):        # what fbs_amd._lib.call makes of it
        _lib.call("fbsmi_kf_create", C.byref(_lib.KFModelStruct(2, 2, 4, *([p] * 13))), 65536, C.byref(C.c_void_p()))
    for call, name in ((lambda: L.fbsmi_kf_sample(None, p, p, p, None, None, None), b"kf_sample"),      # a null handle
                       (lambda: L.fbsmi_kf_filter(None, p, None, None, None), b"kf_filter"),
                       (lambda: L.fbsmi_kf_view(None, 0, None, None, None), b"kf_view")):
        assert call() == ERR_ARG and name in L.fbsmi_last_error()
    L.fbsmi_kf_destroy(None)


# ---- 5. the Python layer without a device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,dv", [(1, 30, 1), (5000, 200, 100), (70000, 200, 128), (9, 1000, 128)])
def test_chunk_planner_covers_every_key_once_within_the_bound(B, T, dv):
    from fbs_amd.lg_kalman import KF_MAX_SAMPLES, KF_PATH_ELEMS, plan_kalman_chunks
    assert KF_PATH_ELEMS == 1 << 26 and KF_MAX_SAMPLES == 16384
    chunks = plan_kalman_chunks(B, T, dv)
    assert [i for a, b in chunks for i in range(a, b)] == list(range(B))
    for a, b in chunks:
        assert 1 <= b - a <= 16384 and (b - a) * (T + 1) * dv <= 1 << 26
    if B <= 16384 and B * (T + 1) * dv <= 1 << 26:
        assert chunks == [(0, B)]
    per = (T + 1) * dv
    assert plan_kalman_chunks(B, T, dv, bound=2 * per) == [(a, min(a + 2, B)) for a in range(0, B, 2)]
    assert plan_kalman_chunks(B, T, dv, bound=per - 1) is None                         # one path alone does not fit


def test_exports_and_refusals():
    import fbs_amd
    from fbs_amd import samplers
    from fbs_amd.gaussian_sb import GaussianSBBridge
    from fbs_amd.lg_kalman import LGKalman, kalman_conditional_sampler, kalman_model
    assert samplers.kalman_conditional_sampler is kalman_conditional_sampler is fbs_amd.kalman_conditional_sampler
    assert fbs_amd.LGKalman is LGKalman and callable(fbs_amd.LinearGaussianBridge.kalman_handle)
    import inspect
    assert list(inspect.signature(kalman_conditional_sampler).parameters)[:4] == ["keys", "y0", "bridge", "return_moments"]
    sb = object.__new__(GaussianSBBridge)                  # no device behind it: refused on its type alone
    with pytest.raises(NotImplementedError, match="GaussianSBBridge"):
        kalman_conditional_sampler(np.zeros((1, 2), np.uint32), np.zeros(1, f32), sb)
    with pytest.raises(NotImplementedError, match="GaussianSBBridge"):
        kalman_model(sb)
