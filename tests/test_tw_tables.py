"""Host side of the fused twisted SMC (fbs_amd/lg_twisted.py): the closed-form tables against float64 torch.autograd on
the reference's own formulation (gp_twisted.py:71-89,113-115), the closures' signatures, the dispatch predicate and the
four entry points in header, library and binding.  No GPU: models are built on the CPU device, which launches nothing."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("fbsmi_tw_create", "fbsmi_tw_destroy", "fbsmi_tw_run", "fbsmi_tw_view")


def _sde(name):
    from fbs_amd.sdes import StationaryConstLinearSDE, StationaryLinLinearSDE
    return StationaryLinLinearSDE(beta_min=0.02, beta_max=4., t0=0., T=1.) if name == "lin" else StationaryConstLinearSDE(a=-0.5, b=1.)


def _problem(d, seed=3):
    zs = np.linspace(0., 5., d)
    cov = np.exp(-np.abs(zs[None, :] - zs[:, None]))
    rng = np.random.default_rng(seed)
    return rng.normal(size=d), cov, rng.normal(size=d).astype(np.float32)


@pytest.mark.parametrize("sde_name", ["const", "lin"])
@pytest.mark.parametrize("d", [3, 24, 128])
def test_tables_against_float64_autograd(d, sde_name):
    from fbs_amd.lg_twisted import lg_twisted_tables
    from fbs_amd.sdes.linear import discretise_linear_sde_np
    sde, T, obs_var = _sde(sde_name), 8, 0.7
    mean, cov, y = _problem(d)
    ts = np.linspace(0., 1., T + 1)
    tab = lg_twisted_tables(mean, cov, sde, ts, obs_var, y)
    assert tab["R"].shape == (T + 1, d, d) and tab["c"].shape == (T + 1, d) and tab["sd"].shape == (T + 1,)
    dt, Tend = 1. / T, ts[-1]
    t64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    mean_t, cov_t, y_t = t64(mean), t64(cov), t64(y)

    def score(u, s):                                                                    # gp_twisted.py:71-74
        F, Q = discretise_linear_sde_np(sde, s, ts[0])
        return -torch.linalg.solve(float(F) ** 2 * cov_t + float(Q) * torch.eye(d, dtype=torch.float64), u - float(F) * mean_t)

    def reverse_drift(u, t):                                                            # :82-83
        s = Tend - t
        return -float(sde.drift(1.0, s)) * u + float(sde.dispersion(s)) ** 2 * score(u, s)

    def twisting_logpdf(y_, u, t):                                                      # :113-115
        loc = u + reverse_drift(u, t) * dt
        return torch.sum(-0.5 * np.log(2 * np.pi * obs_var) - (y_ - loc) ** 2 / (2 * obs_var))

    def reverse_cond_drift(u, t, y_):                                                   # :86-88
        uu = u.detach().requires_grad_(True)
        grad = torch.autograd.grad(twisting_logpdf(y_, uu, t), uu)[0]
        s = Tend - t
        return -float(sde.drift(1.0, s)) * u + float(sde.dispersion(s)) ** 2 * (score(u, s) + grad)

    u = t64(np.random.default_rng(9).normal(size=d) * 1.5)
    worst = 0.0
    for j in (0, T // 2, T):
        t = ts[j]
        want_m = (u + reverse_cond_drift(u, t, y_t) * dt).numpy()
        got_m = u.numpy() + (tab["C"][j] @ u.numpy() + tab["c"][j]) * dt
        want_rd = reverse_drift(u, t).numpy()
        got_rd = tab["R"][j] @ u.numpy() + tab["r"][j]
        for want, got in ((want_m, got_m), (want_rd, got_rd)):
            worst = max(worst, float(np.abs(want - got).max() / np.abs(want).max()))
        s = Tend - t
        assert tab["sd"][j] == np.sqrt(dt) * float(sde.dispersion(s))
    print(f"d = {d}, {sde_name}: largest relative difference {worst:.3g}")
    assert worst <= 1e-12
    # the reference distribution at ts[-1] and the constants
    F_T, Q_T = discretise_linear_sde_np(sde, Tend, ts[0])
    cov_ref = float(F_T) ** 2 * cov + float(Q_T) * np.eye(d)
    assert np.array_equal(tab["m_ref"], float(F_T) * mean)
    assert np.array_equal(tab["Lt"], np.triu(tab["Lt"])) and np.allclose(tab["Lt"].T @ tab["Lt"], cov_ref, rtol=1e-12, atol=1e-13)
    assert tab["dt"] == dt and tab["lognorm_obs"] == np.log(2 * np.pi * obs_var)
    assert np.array_equal(tab["lognorm"], np.log(2 * np.pi * tab["sd"] ** 2))


def _model(d=4, T=5, sde_name="const", y=None, obs_var=0.7):
    import fbs_amd
    mean, cov, y0 = _problem(d)
    return fbs_amd.GaussianTwisted(mean, cov, _sde(sde_name), np.linspace(0., 1., T + 1), obs_var, y0 if y is None else y,
                                   device="cpu")


def test_model_rounds_tables_once_and_tags_closures():
    from fbs_amd.lg_twisted import lg_twisted_tables
    m = _model()
    mean, cov, y = _problem(4)
    tab = lg_twisted_tables(mean, cov, _sde("const"), np.linspace(0., 1., 6), 0.7, y)
    for k in ("R", "r", "C", "c", "sd", "lognorm", "m_ref", "Lt", "y"):
        assert m.host[k].dtype == np.float32 and np.array_equal(m.host[k], np.asarray(tab[k], np.float32)), k
    want = dict(init_sampler=("key_", "nparticles_"), transition_logpdf=("u", "u_prev", "t_prev"),
                twisting_logpdf=("y", "u", "t"), twisting_prop_sampler=("key_", "us", "t", "y"),
                twisting_prop_logpdf=("u", "u_prev", "t", "y"))                        # gp_twisted.py:100-129
    for role, names in want.items():
        closure = getattr(m, role)
        assert closure._fbsmi_lg is m and closure._role == role and callable(closure)
        assert tuple(inspect.signature(closure._fn).parameters) == names, role


def test_dispatch_predicate():
    from fbs_amd.lg_twisted import fused_twisted
    from fbs_amd.samplers import stratified, systematic, multinomial
    m = _model()
    five = lambda mm: (mm.init_sampler, mm.transition_logpdf, mm.twisting_logpdf, mm.twisting_prop_sampler, mm.twisting_prop_logpdf)
    y, ts = m.host["y"], m.ts_np
    assert fused_twisted(y, ts, *five(m), stratified, 64, {}) == (m, "stratified")
    assert fused_twisted(torch.from_numpy(y), torch.from_numpy(ts), *five(m), systematic, 131072, {}) == (m, "systematic")
    assert fused_twisted(y + np.float32(1e-3), ts, *five(m), stratified, 64, {}) is None          # a different y
    assert fused_twisted(y, np.linspace(0., 1.1, ts.size), *five(m), stratified, 64, {}) is None   # a different grid
    assert fused_twisted(y, ts[:-1], *five(m), stratified, 64, {}) is None
    assert fused_twisted(y, ts, *five(m), multinomial, 64, {}) is None
    assert fused_twisted(y, ts, *five(m), stratified, 64, {"mask_": None}) is None                 # any kwargs
    assert fused_twisted(y, ts, *five(m), stratified, 131073, {}) is None
    assert fused_twisted(y, ts, *five(m), stratified, 0, {}) is None
    big = _model(d=129, T=2)
    assert fused_twisted(big.host["y"], big.ts_np, *five(big), stratified, 64, {}) is None         # d = 129
    assert _model(d=128, T=2).fused_supported(64) and not big.fused_supported(64)
    other = _model()
    mixed = list(five(m))
    mixed[2] = other.twisting_logpdf                                                               # another model's closure
    assert fused_twisted(y, ts, *mixed, stratified, 64, {}) is None
    swapped = list(five(m))
    swapped[1], swapped[4] = swapped[4], swapped[1]                                                # right model, wrong roles
    assert fused_twisted(y, ts, *swapped, stratified, 64, {}) is None
    assert fused_twisted(y, ts, *(lambda *a: None for _ in range(5)), stratified, 64, {}) is None


def test_tw_entry_points_declared_exported_and_bound():
    from fbs_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fbsmi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fbsmi_[a-z0-9_]+)\s*\(", text))
    L = ctypes.CDLL(_lib.build())
    for name in ENTRY_POINTS:
        assert name in declared, f"{name} is not declared in include/fbsmi.h"
        assert hasattr(L, name), f"{name} is not exported by libfbsmi"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert "fbsmi_tw_model" in text
    names = [f[0] for f in _lib.TWModelStruct._fields_]
    assert names == ["d", "T", "dt", "R", "r", "C", "c", "sd", "lognorm", "m_ref", "Lt", "y", "obs_var", "lognorm_obs"]
    assert ctypes.sizeof(_lib.TWModelStruct) == 3 * 4 + 4 + 9 * 8 + 2 * 4
    assert L.fbsmi_abi_version() == 1


def test_restatement_stays_finite_at_the_gpu_shapes(oracle):
    """The numpy restatement alone (tests/tw_restate.py), at the smallest and the widest shape of the GPU parity tests."""
    from tw_restate import Restate
    for d, T, N, sde_name in ((2, 5, 2, "const"), (128, 3, 33, "lin")):
        m = _model(d=d, T=T, sde_name=sde_name)
        xs, lws, inds = Restate(oracle, m).run(oracle.PRNGKey(5), N)
        assert xs.shape == (N, d) and inds.shape == (T, N) and np.isfinite(xs).all() and np.isfinite(lws).all()


def _gpu_cases():
    from test_gpu_tw_fused import LARGE, WIDE, ladder_obs_var
    return [(s, ladder_obs_var(s[0])) for s in WIDE] + [(s + ("const",), ladder_obs_var(s[0])) for s in LARGE]


@pytest.mark.parametrize("resampling", ["stratified", "systematic"])
@pytest.mark.parametrize("case", _gpu_cases(), ids=lambda c: "d{}-T{}-N{}-{}".format(*c[0]))
def test_restatement_keeps_a_diverse_ensemble_at_the_gpu_ladder(case, resampling, oracle):
    """The restated runs the GPU ladder is compared with (tests/test_gpu_tw_fused.py: obs_var = 5 from width 16 on, 0.7 below, the
    same models, key and resamplers) are finite, and every step keeps at least N / 4 distinct ancestors: a collapsed
    ensemble would gather a handful of rows over and over and test little of the search, the gather or the product."""
    from test_gpu_tw_fused import _want
    (d, T, N, sde_name), obs_var = case
    xs, lws, inds = _want(d, T, N, sde_name, resampling, 11, obs_var, "cpu")
    assert xs.shape == (N, d) and lws.shape == (N,) and inds.shape == (T, N)
    assert np.isfinite(xs).all() and np.isfinite(lws).all() and inds.min() >= 0 and inds.max() < N
    distinct = [int(np.unique(row).size) for row in inds]
    print(f"d = {d}, T = {T}, N = {N}, {sde_name}, {resampling}, obs_var = {obs_var}: distinct ancestors per step {distinct}")
    assert min(distinct) >= N / 4


# ---- argument checks of fbsmi_tw_create: answered before any device call ---------------------------------------------------------
def test_tw_create_validation():
    import ctypes as C
    from fbs_amd import _lib
    from fbs_amd.lg_twisted import MAX_RUNS, TwistedHandle
    OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
    L = _lib.lib()
    buf = C.create_string_buffer(64)                       # a non-NULL pointer; never dereferenced
    p = C.addressof(buf)

    def create(d=4, T=3, nparticles=8, resampling=0, nruns=1, null=None, model=True):
        tabs = [None if n == null else p for n in ("R", "r", "C", "c", "sd", "lognorm", "m_ref", "Lt", "y")]
        st = _lib.TWModelStruct(d, T, 0.25, *tabs, 0.7, 1.0)
        h = C.c_void_p()
        rc = L.fbsmi_tw_create(C.byref(st) if model else None, nparticles, resampling, nruns, 0, C.byref(h))
        assert not h.value
        return rc, L.fbsmi_last_error()

    for kw in (dict(model=False), dict(T=0), dict(nruns=0), dict(nruns=-1), dict(resampling=2), dict(null="R"), dict(null="y")):
        rc, msg = create(**kw)
        assert rc == ERR_ARG and b"tw_create" in msg, (kw, rc, msg)
    for kw in (dict(d=0), dict(d=129), dict(nparticles=0), dict(nparticles=131073)):
        rc, msg = create(**kw)
        assert rc == ERR_UNSUPPORTED and b"tw_create" in msg and b"128" in msg and b"131072" in msg, (kw, rc, msg)
    rc, msg = create(nruns=65536)
    assert rc == ERR_UNSUPPORTED and b"tw_create" in msg and b"nruns" in msg and b"65535" in msg, (rc, msg)
    rc, msg = create(nruns=1 << 30)
    assert rc == ERR_UNSUPPORTED and b"65535" in msg, (rc, msg)
    # nruns = 65535 passes the bound: with a width that is refused next, the refusal is the width's (nothing is allocated)
    rc, msg = create(nruns=65535, d=129)
    assert rc == ERR_UNSUPPORTED and b"65535" not in msg and b"128" in msg, (rc, msg)
    rc, msg = create(nruns=65536, d=129)
    assert rc == ERR_UNSUPPORTED and b"65535" in msg, (rc, msg)
    with pytest.raises(NotImplementedError, match="65535"):        # what fbs_amd._lib.call makes of it
        tabs = [p] * 9
        _lib.call("fbsmi_tw_create", C.byref(_lib.TWModelStruct(4, 3, 0.25, *tabs, 0.7, 1.0)), 8, 0, 65536, 0, C.byref(C.c_void_p()))
    # the Python layer refuses it before the library is asked
    assert MAX_RUNS == 65535
    m = _model()
    for nruns in (65536, 0):
        with pytest.raises(NotImplementedError, match="65535"):
            m.handle(8, "stratified", nruns=nruns)
        with pytest.raises(NotImplementedError, match="65535"):
            TwistedHandle(m, 8, "stratified", nruns=nruns)
    assert not m._handles or all(k[2] not in (0, 65536) for k in m._handles)

