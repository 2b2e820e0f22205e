"""CPU: the host side of the Kalman smoother and path sampler -- lg_smoother_tables and the backward recursion against dense
joint-Gaussian conditioning over the whole path, the float32 restatement of the header's specification
(tests/kfs_restate.py) against the float64 recursion, its consistency with the filter's restatement, the oracle's particle
smoother against the exact smoothing law, fbsmi_kfs_*'s argument checks and the Python layer's refusals.  No device is
touched."""
import ctypes as C

import numpy as np
import pytest

from helpers import toy_gp
import fsamp_restate as FR
import kf_restate as R
import kfs_restate as KR
from test_kf_tables import DENSE, LADDER, LADDER_TS, TOYS, _host32, _oracle_model, _tables, ladder_keys

f32 = np.float32
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
CAP = 5e-5      # max |path32 - path64| / max |path64| per sample, T <= 200


def _stables(toy, ts):
    """(lg_tables, lg_pmcmc_tables, lg_kalman_tables, lg_smoother_tables) of a toy on the grid ts, float64."""
    from fbs_amd.lg_kalman import lg_smoother_tables
    tab, pm, kt = _tables(toy, ts)
    return tab, pm, kt, lg_smoother_tables(tab, kt)


def _shost32(st):
    return {k: np.ascontiguousarray(np.asarray(st[k], f32)) for k in ("K", "J", "Lb")}


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---- 1. the tables and the recursion against dense conditioning ---------------------------------------------------------
def _dense_path(tab, m0, Sig0, vs):
    """p(u_0..u_T | v_0..v_T) by conditioning the joint Gaussian of x = (u_0..u_T) on the stacked observations
    (tests/test_kf_tables.py::_dense, the whole posterior kept) -> (mean ((T+1) du), cov ((T+1) du, (T+1) du))."""
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
    return mean_x + Sxy @ np.linalg.solve(Syy, y - Cbig @ mean_x), cov_x - Sxy @ np.linalg.solve(Syy, Sxy.T)


def _sampler_cov(kt, st):
    """The joint covariance of (u_0..u_T) that the backward sampler implies: delta_T = Lt^T zT,
    delta_k = J_k delta_{k+1} + Lb_k xi_k is a linear map of independent unit normals."""
    T, du = kt["T"], kt["du"]
    Phi = np.zeros((T + 1, du, (T + 1) * du))                # columns: xi_0 .. xi_{T-1}, zT
    Phi[T][:, T * du:] = kt["Lt"].T
    for k in range(T - 1, -1, -1):
        Phi[k] = st["J"][k] @ Phi[k + 1]
        Phi[k][:, k * du:(k + 1) * du] = st["Lb"][k]
    P = Phi.reshape((T + 1) * du, (T + 1) * du)
    return P @ P.T


@pytest.mark.parametrize("name", sorted(TOYS) + sorted(set(DENSE) - set(TOYS)))
def test_tables_and_recursion_against_dense_conditioning(name):
    from fbs_amd.lg_kalman import kalman_filter_np, kalman_smoother_np
    tab, pm, kt, st = _stables(DENSE[name](), np.linspace(0, 2, 7))
    T, du, dv = kt["T"], kt["du"], kt["dv"]
    assert T == 6 and st["K"].shape == (6, du, dv) and st["J"].shape == st["Lb"].shape == (6, du, du)
    assert st["cov_s"].shape == (7, du, du) and st["cross"].shape == (6, du, du)
    assert np.all(np.tril(st["Lb"]) == st["Lb"]) and np.array_equal(st["cov_s"][T], kt["cov_T"])
    rng = np.random.default_rng(3)
    joint = _sampler_cov(kt, st)
    for trial in range(3):
        vs = rng.normal(size=(7, dv))
        sm, ms, rs, ll = kalman_smoother_np(kt, st, vs)
        mT, wll = kalman_filter_np(kt, vs)
        assert np.array_equal(ms[T], mT) and ll == wll and np.array_equal(sm[T], mT)
        m0 = kt["m_u"] + kt["gain"] @ (vs[0] - kt["m_v"])
        wmean, wcov = _dense_path(tab, m0, kt["cov_0"], vs)
        blk = lambda a, b: wcov[a * du:(a + 1) * du, b * du:(b + 1) * du]
        errs = dict(mean=_rel(sm.reshape(-1), wmean), joint=_rel(joint, wcov),
                    cov_s=max(_rel(st["cov_s"][k], blk(k, k)) for k in range(T + 1)),
                    cross=max(float(np.abs(st["cross"][k] - blk(k, k + 1)).max() / np.abs(wcov).max()) for k in range(T)))
        print(f"{name} trial {trial}: relative differences " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) <= 1e-12, errs


# ---- 2. the float32 restatement against the float64 recursion -------------------------------------------------------------
def _restatement_figures(O, toy, ts, keys):
    """Worst max |path32 - path64| / max |path64| over the samples -> (sampled path, smoothed mean), and the batch."""
    from fbs_amd.lg_kalman import kalman_smoother_np
    tab, pm, kt, st = _stables(toy, ts)
    host, shost = _host32(kt), _shost32(st)
    w = KR.want(O, _oracle_model(O, tab), host, shost, kt, keys, toy["y0"])
    s = KR.smooth_restated(host, shost, kt, w["vs"])
    T, du = kt["T"], kt["du"]
    assert w["paths"].shape == s["smeans"].shape == (len(keys), T + 1, du) and np.isfinite(w["paths"]).all()
    worst_p = worst_s = 0.0
    for b, key in enumerate(keys):
        _, key_bwd, key_kf = O.split(key, 3)
        noise = (O.normal(key_kf, (du,)).astype(np.float64), O.normal(key_bwd, (T, du)).astype(np.float64))
        vs64 = w["vs"][b].astype(np.float64)
        p64 = kalman_smoother_np(kt, st, vs64, noise=noise)[0]
        s64 = kalman_smoother_np(kt, st, vs64)[0]
        worst_p = max(worst_p, _rel(w["paths"][b].astype(np.float64), p64))
        worst_s = max(worst_s, _rel(s["smeans"][b].astype(np.float64), s64))
    return worst_p, worst_s, w


T200 = {"gp100": lambda: toy_gp(100), "gp128v1": LADDER["gp128v1"], "gp64": LADDER["gp64"], "rand33v80": LADDER["rand33v80"]}


@pytest.mark.parametrize("name", list(T200))
def test_restatement_against_float64_at_T200(name, oracle):
    """Worst figures measured (sampled path, smoothed mean), 2 keys, ts = linspace(0, 1, 201): see DESIGN.md section 4.7."""
    worst_p, worst_s, _ = _restatement_figures(oracle, T200[name](), np.linspace(0, 1, 201),
                                               oracle.split(oracle.PRNGKey(7), 2))
    print(f"{name} T = 200: sampled path {worst_p:.2e}, smoothed mean {worst_s:.2e} of max |path|")
    assert worst_p <= CAP and worst_s <= CAP


@pytest.mark.parametrize("name", list(LADDER))
def test_restatement_against_float64_across_the_width_ladder(name, oracle):
    worst_p, worst_s, _ = _restatement_figures(oracle, LADDER[name](), LADDER_TS, ladder_keys(oracle))
    print(f"{name} T = 6: sampled path {worst_p:.2e}, smoothed mean {worst_s:.2e} of max |path|")
    assert worst_p <= CAP and worst_s <= CAP


# ---- 3. consistency with the filter's restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4d", "gp20v7", "rand33v80"])
def test_restatement_agrees_with_the_filters(name, oracle):
    make = {"4d": TOYS["4d"], "gp20v7": lambda: toy_gp(20, dv=7), "rand33v80": LADDER["rand33v80"]}[name]
    toy = make()
    tab, pm, kt, st = _stables(toy, LADDER_TS)
    om, host, keys = _oracle_model(oracle, tab), _host32(kt), ladder_keys(oracle, 5)
    w = KR.want(oracle, om, host, _shost32(st), kt, keys, toy["y0"])
    f = R.want(oracle, om, host, kt, keys, toy["y0"])
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for got, want, what in ((w["paths"][:, -1], f["samples"], "paths[:, T]"), (w["m"][:, -1], f["means"], "m_T"),
                            (w["loglik"], f["loglik"], "loglik"), (w["vs"], f["vs"], "vs"), (w["m"][:, 0], f["m_"], "m_0")):
        assert np.array_equal(bits(got), bits(want)), what
    # smooth on the same paths: the same forward pass, m_T at the end of the path
    s = KR.smooth_restated(host, _shost32(st), kt, w["vs"])
    assert np.array_equal(bits(s["m"]), bits(w["m"])) and np.array_equal(bits(s["loglik"]), bits(f["loglik"]))
    assert np.array_equal(bits(s["smeans"][:, -1]), bits((f["means"] + f32(0.0)).astype(f32)))


# ---- 4. one ulp in the last row tile and column group ---------------------------------------------------------------------------
def test_restatement_feels_one_ulp_in_the_last_row_and_column_of_J(oracle):
    """toy_gp(80, dv=33): one ulp on J[5][79][79] (row tile 4, column group 4, the first backward step) changes the
    restated paths at step 5 in coordinate 79 only and from there only downstream (steps 4..0); step 6 is untouched."""
    toy = LADDER["gp80v33"]()
    tab, pm, kt, st = _stables(toy, LADDER_TS)
    om, host, shost, keys = _oracle_model(oracle, tab), _host32(kt), _shost32(st), ladder_keys(oracle)
    w = KR.want(oracle, om, host, shost, kt, keys, toy["y0"])
    J = shost["J"].copy()
    J[5, 79, 79] = np.nextafter(J[5, 79, 79], f32(np.inf))
    assert J[5, 79, 79] != shost["J"][5, 79, 79]
    wb = KR.want(oracle, om, host, dict(shost, J=J), kt, keys, toy["y0"])
    changed = np.argwhere(wb["paths"].view(np.uint32) != w["paths"].view(np.uint32))      # (sample, step, coordinate)
    at5 = changed[changed[:, 1] == 5]
    print(f"one ulp on J[5][79][79]: {len(changed)} path entries changed, {len(at5)} of them at step 5")
    assert len(at5) >= 1 and np.all(at5[:, 2] == 79) and np.all(changed[:, 1] <= 5)
    assert np.any(changed[:, 1] < 5)


# ---- 5. the oracle's particle smoother against the exact smoothing law ------------------------------------------------------------
def particle_smoother_inputs(O, name):
    """The inputs of this test and of its fused twin (tests/test_gpu_kfs.py) -> (toy, ts, tables, om, vs, keys)."""
    toy, ts = TOYS[name](), np.linspace(0, 2, 31)
    tab, pm, kt, st = _stables(toy, ts)
    om = _oracle_model(O, tab)
    vs = O.lg_fwd_sampler(om, O.PRNGKey(99), toy["y0"])[::-1].copy()
    return toy, ts, (tab, pm, kt, st), om, vs, O.split(O.PRNGKey(17), 48)


def check_whitened_paths(paths, kt, st, vs, what):
    """paths (n, T+1, du) draws on the one observation path vs: z = (path - smoothed mean) / sqrt(diag cov_s) has mean
    within 4 / sqrt(n) of 0 and variance within 4 sqrt(2 / n) of 1 at every (step, coordinate)."""
    from fbs_amd.lg_kalman import kalman_smoother_np
    n = paths.shape[0]
    sm = kalman_smoother_np(kt, st, np.asarray(vs, np.float64))[0]
    sdev = np.sqrt(np.stack([np.diag(c) for c in st["cov_s"]]))
    z = (np.asarray(paths, np.float64) - sm[None]) / sdev[None]
    mean, var = z.mean(axis=0), z.var(axis=0, ddof=1)
    print(f"{what}: worst |mean_z| sqrt(n) = {np.abs(mean).max() * np.sqrt(n):.2f}, var_z in [{var.min():.2f}, {var.max():.2f}]")
    assert np.all(np.abs(mean) <= 4 / np.sqrt(n)) and np.all(np.abs(var - 1) <= 4 * np.sqrt(2 / n))


@pytest.mark.parametrize("name", ["2d", "4d"])
def test_oracle_particle_smoother_against_the_exact_law(name, oracle):
    toy, ts, (tab, pm, kt, st), om, vs, keys = particle_smoother_inputs(oracle, name)
    paths = []
    for key in keys:
        _, key_bwd, key_bf = oracle.split(key, 3)
        u0s = FR.ref_restated(oracle, pm, oracle.split(key_bf, 2)[0], vs[0], 1024)
        filt, _ = oracle.bootstrap_filter_lg(om, key_bf, vs, u0s, "stratified", return_last=False)
        paths.append(oracle.backward_smoother_lg(om, key_bwd, filt, vs))
    check_whitened_paths(np.stack(paths), kt, st, vs, f"{name}: oracle particle smoother, 1024 particles, 48 keys")


# ---- 6. argument checks of fbsmi_kfs_*: answered before any device call ------------------------------------------------------------
def test_kfs_create_and_entry_point_validation():
    from fbs_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(64)                       # a non-NULL pointer; never dereferenced
    p = C.addressof(buf)
    names = [n for n, _ in _lib.KFModelStruct._fields_[3:]]
    assert [n for n, _ in _lib.KFSModelStruct._fields_] == ["kf", "K", "J", "Lb"]

    def create(du=2, dv=2, T=4, nsamples=1, null=None, model=True, kf=True):
        kfst = _lib.KFModelStruct(du, dv, T, *(None if n == null else p for n in names))
        st = _lib.KFSModelStruct(C.pointer(kfst) if kf else None, *(None if n == null else p for n in ("K", "J", "Lb")))
        h = C.c_void_p()
        rc = L.fbsmi_kfs_create(C.byref(st) if model else None, nsamples, C.byref(h))
        assert not h.value
        return rc, L.fbsmi_last_error()

    for kw in [dict(model=False), dict(kf=False), dict(T=0)] + [dict(null=n) for n in names + ["K", "J", "Lb"]]:
        rc, msg = create(**kw)
        assert rc == ERR_ARG and b"kfs_create" in msg, (kw, rc, msg)
    for kw in [dict(du=0), dict(du=129), dict(dv=0), dict(dv=129), dict(du=-1), dict(nsamples=0), dict(nsamples=65536),
               dict(nsamples=-3)]:
        rc, msg = create(**kw)
        assert rc == ERR_UNSUPPORTED and b"kfs_create" in msg and b"128" in msg and b"65535" in msg, (kw, rc, msg)
    kfst = _lib.KFModelStruct(2, 2, 4, *([p] * 13))
    assert L.fbsmi_kfs_create(C.byref(_lib.KFSModelStruct(C.pointer(kfst), p, p, p)), 1, None) == ERR_ARG
    with pytest.raises(NotImplementedError, match="65535"):        # what fbs_amd._lib.call makes of it
        _lib.call("fbsmi_kfs_create", C.byref(_lib.KFSModelStruct(C.pointer(kfst), p, p, p)), 65536, C.byref(C.c_void_p()))
    for call, name in ((lambda: L.fbsmi_kfs_sample(None, p, p, p, None, None), b"kfs_sample"),       # a null handle
                       (lambda: L.fbsmi_kfs_sample_on(None, p, p, p, None, None), b"kfs_sample_on"),
                       (lambda: L.fbsmi_kfs_smooth(None, p, p, None, None), b"kfs_smooth"),
                       (lambda: L.fbsmi_kfs_view(None, 0, None, None, None), b"kfs_view")):
        assert call() == ERR_ARG and name in L.fbsmi_last_error()
    L.fbsmi_kfs_destroy(None)


@pytest.mark.parametrize("B,T,du,dv", [(1, 30, 1, 1), (5000, 200, 100, 100), (70000, 200, 128, 1), (70000, 200, 5, 128),
                                       (9, 1000, 128, 128)])
def test_chunk_planner_keeps_every_buffer_within_the_bound(B, T, du, dv):
    from fbs_amd.lg_kalman import plan_smoother_chunks
    chunks = plan_smoother_chunks(B, T, du, dv)
    assert [i for a, b in chunks for i in range(a, b)] == list(range(B))
    for a, b in chunks:
        n = b - a
        assert 1 <= n <= 16384
        assert max(n * (T + 1) * dv, n * (T + 1) * du, n * T * dv) <= 1 << 26           # vs, m_k and paths, r_k
    if B <= 16384 and B * (T + 1) * max(du, dv) <= 1 << 26:
        assert chunks == [(0, B)]
    per = (T + 1) * max(du, dv)
    assert plan_smoother_chunks(B, T, du, dv, bound=2 * per) == [(a, min(a + 2, B)) for a in range(0, B, 2)]
    assert plan_smoother_chunks(B, T, du, dv, bound=per - 1) is None                    # one path alone does not fit


def test_exports_and_refusals():
    import inspect
    import fbs_amd
    from fbs_amd import samplers
    from fbs_amd.gaussian_sb import GaussianSBBridge
    from fbs_amd.lg_kalman import LGKalmanSmoother, kalman_path_sampler, kalman_smoother_model
    assert samplers.kalman_path_sampler is kalman_path_sampler is fbs_amd.kalman_path_sampler
    assert fbs_amd.LGKalmanSmoother is LGKalmanSmoother and callable(fbs_amd.LinearGaussianBridge.kalman_smoother_handle)
    assert list(inspect.signature(kalman_path_sampler).parameters)[:4] == ["keys", "y0", "bridge", "return_moments"]
    for meth in ("sample", "sample_on", "smooth", "views", "cov_s"):
        assert hasattr(LGKalmanSmoother, meth)
    sb = object.__new__(GaussianSBBridge)                  # no device behind it: refused on its type alone
    with pytest.raises(NotImplementedError, match="GaussianSBBridge"):
        kalman_path_sampler(np.zeros((1, 2), np.uint32), np.zeros(1, f32), sb)
    with pytest.raises(NotImplementedError, match="GaussianSBBridge"):
        kalman_smoother_model(sb)
    # gibbs_init(method='kalman') takes the closures of a LinearGaussianBridge only: refused before anything is drawn
    foreign = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a foreign closure was called"))
    with pytest.raises(NotImplementedError, match="LinearGaussianBridge"):
        samplers.gibbs_init(np.zeros(2, np.uint32), np.zeros(1, f32), (1,), np.linspace(0, 1, 5), foreign, None, foreign,
                            foreign, foreign, foreign, 10, method='kalman', marg_y=False)
