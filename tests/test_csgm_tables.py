"""Host side of the fused CSGM (fbs_amd/lg_csgm.py): the closed-form tables against float64 torch.autograd on the
reference's own formulation (gp_csgm.py:80-91, generalised to a non-zero prior mean), the terminal reference against the
direct float64 formulas, the numpy restatement of the numeric specification (tests/csgm_restate.py) against a float64
evaluation of the same recursion, and the entry points in header, library and binding.  No GPU: models are built on the
CPU device, which launches nothing."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from helpers import WIDTHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("fbsmi_csgm_create", "fbsmi_csgm_destroy", "fbsmi_csgm_run", "fbsmi_csgm_view")
OBS_VAR = 0.7


def _sde(name):
    from fbs_amd.sdes import StationaryConstLinearSDE, StationaryLinLinearSDE
    return StationaryLinLinearSDE(beta_min=0.02, beta_max=4., t0=0., T=1.) if name == "lin" else StationaryConstLinearSDE(a=-0.5, b=1.)


def _problem(d, seed=3):
    zs = np.linspace(0., 5., d)
    cov = np.exp(-np.abs(zs[None, :] - zs[:, None]))
    rng = np.random.default_rng(seed)
    return rng.normal(size=d), cov, rng.normal(size=d).astype(np.float32)


@pytest.mark.parametrize("sde_name", ["const", "lin"])
@pytest.mark.parametrize("d", [1, 3, 24, 128])
def test_tables_against_float64_autograd(d, sde_name):
    """A[k] u + cvec[k] against the reference's reverse_drift with the gradient taken by autograd, probed with the zero
    vector (cvec) and the unit vectors (the columns of A): 1e-12 relative to the table's largest magnitude, the bound of
    tests/test_tw_tables.py.  Largest figure measured: 8.4e-14 (d = 128, lin)."""
    from fbs_amd.lg_csgm import lg_csgm_tables
    from fbs_amd.sdes.linear import discretise_linear_sde_np
    sde, T = _sde(sde_name), 200
    mean, cov, y = _problem(d)
    ts = np.linspace(0., 1., T + 1)
    tab = lg_csgm_tables(mean, cov, sde, ts, OBS_VAR, y)
    assert tab["A"].shape == (T, d, d) and tab["cvec"].shape == (T, d) and tab["ddt"].shape == (T,) and tab["s"].shape == (T,)
    t64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    mean_t, cov_t, y_t, eye = t64(mean), t64(cov), t64(y), torch.eye(d, dtype=torch.float64)
    Tend = ts[-1]

    def reverse_drift(u, t):                                                            # gp_csgm.py:80-91
        F, Q = (float(v) for v in discretise_linear_sde_np(sde, Tend - t, ts[0]))
        chol = torch.linalg.cholesky(F ** 2 * cov_t + Q * eye)
        solve = lambda b: torch.cholesky_solve(b.reshape(d, -1), chol).reshape(b.shape)
        score_x = -solve(u - F * mean_t)

        def cond_logpdf(x_):
            cond_m = mean_t + cov_t * F @ solve(x_ - F * mean_t)
            cond_cov = cov_t + OBS_VAR * eye - cov_t * F @ solve(F * cov_t)
            return torch.distributions.MultivariateNormal(cond_m, covariance_matrix=cond_cov).log_prob(y_t)

        uu = u.detach().requires_grad_(True)
        grad = torch.autograd.grad(cond_logpdf(uu), uu)[0]
        return -float(sde.drift(1.0, Tend - t)) * u + float(sde.dispersion(Tend - t)) ** 2 * (score_x + grad)

    worst = 0.0
    for k in (0, 1, 25, 50, 99, 100, 150, 198, 199):
        zero = reverse_drift(torch.zeros(d, dtype=torch.float64), ts[k]).numpy()
        cols = np.stack([reverse_drift(eye[c], ts[k]).numpy() - zero for c in range(d)], axis=1)
        for want, got in ((zero, tab["cvec"][k]), (cols, tab["A"][k])):
            scale = max(np.abs(tab["A"][k]).max(), np.abs(tab["cvec"][k]).max())
            worst = max(worst, float(np.abs(want - got).max() / scale))
        h = abs(ts[k + 1] - ts[k])
        assert tab["ddt"][k] == np.float32(h) and tab["s"][k] == np.float32(float(sde.dispersion(Tend - ts[k])) * np.sqrt(h))
    print(f"d = {d}, {sde_name}: largest difference relative to the table's largest magnitude {worst:.3g}")
    assert worst <= 1e-12


@pytest.mark.parametrize("sde_name", ["const", "lin"])
@pytest.mark.parametrize("d", [1, 3, 24, 128])
def test_terminal_reference(d, sde_name):
    """m_ref, S_ref against gp_csgm.py:69-72 written out with np.linalg.solve."""
    from fbs_amd.lg_csgm import lg_csgm_tables
    from fbs_amd.sdes.linear import discretise_linear_sde_np
    sde = _sde(sde_name)
    mean, cov, y = _problem(d)
    ts = np.linspace(0., 1., 9)
    tab = lg_csgm_tables(mean, cov, sde, ts, OBS_VAR, y)
    F, Q = (float(v) for v in discretise_linear_sde_np(sde, ts[-1], ts[0]))
    Kyy = cov + OBS_VAR * np.eye(d)
    m_want = F * mean + F * cov @ np.linalg.solve(Kyy, np.asarray(y, np.float64) - mean)
    S_want = F ** 2 * cov + Q * np.eye(d) - F * cov @ np.linalg.solve(Kyy, F * cov)
    assert tab["m_ref"].shape == (d,) and tab["S_ref"].shape == (d, d)
    assert np.abs(tab["m_ref"] - m_want).max() <= 1e-12 * np.abs(m_want).max()
    assert np.abs(tab["S_ref"] - S_want).max() <= 1e-12 * np.abs(S_want).max()
    assert np.allclose(tab["S_ref"], tab["S_ref"].T, rtol=0, atol=1e-14) and np.linalg.eigvalsh(tab["S_ref"]).min() > 0


def _model(d=4, T=5, sde_name="const"):
    import fbs_amd
    mean, cov, y = _problem(d)
    return fbs_amd.GaussianCSGM(0.3 * mean, cov, _sde(sde_name), np.linspace(0., 1., T + 1), OBS_VAR, y, device="cpu")


def float64_recursion(O, m, key, u0=None):
    """The specification's recursion in float64 on the float64 tables, from the float32 draws of the same keys:
    key = the sample's key (u0 None), or key_sde with the given u0.  -> path (T+1, d)"""
    t64 = m.tables64
    if u0 is None:
        key_init, key = O.split(np.asarray(key, np.uint32), 2)
        u0 = t64["m_ref"] + t64["S_ref"] @ O.normal(key_init, (m.d,)).astype(np.float64)
    x = np.asarray(u0, np.float64)
    path, keys = [x], O.split(np.asarray(key, np.uint32), m.T)
    for k in range(m.T):
        xi = O.normal(keys[k], (1, m.d))[0].astype(np.float64)
        x = x + (t64["A"][k] @ x + t64["cvec"][k]) * float(t64["ddt"][k]) + float(t64["s"][k]) * xi
        path.append(x)
    return np.stack(path)


def test_restatement_against_float64(oracle):
    """tests/csgm_restate.py against the float64 recursion on the same float32 draws, d = 24, T = 6: 1e-5 relative to the
    largest magnitude, the project's float tolerance."""
    from csgm_restate import Restate
    m = _model(d=24, T=6)
    rs = Restate(oracle, m)
    worst = 0.0
    for seed in (5, 6, 7):
        u0, path = rs.sample(oracle.PRNGKey(seed))
        want = float64_recursion(oracle, m, oracle.PRNGKey(seed))
        assert path.shape == (7, 24) and path.dtype == np.float32 and np.array_equal(path[0], u0)
        worst = max(worst, float(np.abs(path.astype(np.float64) - want).max() / np.abs(want).max()))
    print(f"restatement against float64: {worst:.3g}")
    assert worst <= 1e-5


@pytest.mark.parametrize("sde_name", ["const", "lin"])
@pytest.mark.parametrize("d", WIDTHS)
def test_restatement_against_float64_across_the_width_ladder(d, sde_name, oracle):
    """The same comparison at every width of helpers.WIDTHS (both sides of every 16-row tile), T = 6: bit equality of the
    kernel with the restatement says nothing about accuracy at a width where the restatement was never held to float64.
    Largest figure measured over the ladder: 4.9e-7 (d = 128, lin)."""
    from csgm_restate import Restate
    m = _model(d=d, T=6, sde_name=sde_name)
    rs = Restate(oracle, m)
    worst = 0.0
    for seed in (5, 6, 7):
        u0, path = rs.sample(oracle.PRNGKey(seed))
        want = float64_recursion(oracle, m, oracle.PRNGKey(seed))
        assert path.shape == (7, d) and path.dtype == np.float32 and np.array_equal(path[0], u0)
        worst = max(worst, float(np.abs(path.astype(np.float64) - want).max() / np.abs(want).max()))
    print(f"d = {d}, {sde_name}: restatement against float64 {worst:.3g}")
    assert worst <= 1e-5


@pytest.mark.parametrize("d,T,sde_name", [(3, 2, "const"), (17, 3, "lin"), (80, 4, "const")])
def test_batched_restatement_is_the_per_key_one(d, T, sde_name, oracle):
    """Restate.sample_batch (what the GPU tests of wide or large batches compare with) against Restate.sample, bit for bit."""
    from csgm_restate import Restate
    rs = Restate(oracle, _model(d=d, T=T, sde_name=sde_name))
    keys = np.stack([oracle.PRNGKey(11 + b) for b in range(5)])
    u0, path = rs.sample_batch(keys)
    assert u0.shape == (5, d) and path.shape == (T + 1, 5, d) and u0.dtype == path.dtype == np.float32
    for b in range(5):
        u0_1, path_1 = rs.sample(keys[b])
        assert np.array_equal(u0[b].view(np.uint32), u0_1.view(np.uint32))
        assert np.array_equal(path[:, b].view(np.uint32), path_1.view(np.uint32))


def test_restatement_feels_one_ulp_past_row_and_column_64(oracle):
    """d = 80: one ulp on A[1][79][79] (the last row and column, both past 64) changes the restated path, so a comparison
    with the restatement reaches the rows and columns the wide GPU cases exist for.  A drift that moves by one ulp is
    scaled by ddt = 1/3 before it meets x, so most single entries' ulps are rounded away there (of the diagonal entries
    tried, 79 at step 1 and 70 at step 2 survive); the entry is one that survives, and the change is where it must be."""
    from csgm_restate import Restate
    m = _model(d=80, T=3)
    u0, path = Restate(oracle, m).sample(oracle.PRNGKey(5))
    A = m.host["A"].copy()
    A[1, 79, 79] = np.nextafter(A[1, 79, 79], np.float32(np.inf))
    assert A[1, 79, 79] != m.host["A"][1, 79, 79]
    bumped = Restate(oracle, m)
    bumped.h = dict(m.host, A=A)
    u0_b, path_b = bumped.sample(oracle.PRNGKey(5))
    assert np.array_equal(u0_b.view(np.uint32), u0.view(np.uint32))                     # u0 does not read A
    changed = np.argwhere(path_b.view(np.uint32) != path.view(np.uint32))
    print(f"one ulp on A[1][79][79]: {len(changed)} of {path.size} path entries change, first {changed[:1].tolist()}")
    assert len(changed) >= 1 and changed[0].tolist() == [2, 79]                         # first in row 79, behind step 1


def test_restatement_stays_finite_at_the_gpu_shapes(oracle):
    from csgm_restate import Restate
    for d, T, sde_name in ((1, 8, "const"), (128, 3, "lin")):
        u0, path = Restate(oracle, _model(d=d, T=T, sde_name=sde_name)).sample(oracle.PRNGKey(5))
        assert u0.shape == (d,) and path.shape == (T + 1, d) and np.isfinite(path).all()


def test_model_rounds_tables_once_and_tags_closures():
    from fbs_amd.lg_csgm import lg_csgm_tables
    m = _model()
    mean, cov, y = _problem(4)
    tab = lg_csgm_tables(0.3 * mean, cov, _sde("const"), np.linspace(0., 1., 6), OBS_VAR, y)
    for k in ("A", "cvec", "ddt", "s", "m_ref", "S_ref"):
        assert m.host[k].dtype == np.float32 and np.array_equal(m.host[k], np.asarray(tab[k], np.float32)), k
    want = dict(reverse_drift=("u", "t"), reverse_dispersion=("t",), ref_sampler=("key",))   # gp_csgm.py:75,80,94
    for role, names in want.items():
        closure = getattr(m, role)
        assert closure._fbsmi_lg is m and closure._role == role and callable(closure)
        assert tuple(inspect.signature(closure._fn).parameters) == names, role
    assert m.point_of(0.2) == 1 and m.reverse_dispersion(0.2) == float(_sde("const").dispersion(0.8))
    with pytest.raises(ValueError):
        m.point_of(0.25)                                                                 # off the grid
    with pytest.raises(ValueError):
        m.point_of(1.0)                                                                  # no step starts at ts[-1]


def test_dispatch_predicate():
    from fbs_amd.lg_csgm import fused_csgm
    m = _model()
    ts, d = m.ts_np, m.d
    x1, xB = np.zeros(d, np.float32), np.zeros((7, d), np.float32)
    key, keys = np.array([1, 2], np.uint32), np.zeros((7, 2), np.uint32)
    assert fused_csgm(x1, ts, m.reverse_drift, m.reverse_dispersion, 1, key) == (m, 1)
    assert fused_csgm(torch.zeros(7, d), torch.from_numpy(ts), m.reverse_drift, m.reverse_dispersion, 1, keys) == (m, 7)
    assert fused_csgm(xB, ts, m.reverse_drift, m.reverse_dispersion, 1, key) is None             # one key for 7 rows
    assert fused_csgm(x1, ts, m.reverse_drift, m.reverse_dispersion, 2, key) is None             # sub-stepping
    assert fused_csgm(x1, np.linspace(0., 1.1, ts.size), m.reverse_drift, m.reverse_dispersion, 1, key) is None
    assert fused_csgm(x1, ts[:-1], m.reverse_drift, m.reverse_dispersion, 1, key) is None
    assert fused_csgm(np.zeros(d + 1, np.float32), ts, m.reverse_drift, m.reverse_dispersion, 1, key) is None
    assert fused_csgm(np.zeros((2, 3, d), np.float32), ts, m.reverse_drift, m.reverse_dispersion, 1, key) is None
    assert fused_csgm(x1, ts, lambda u, t: m.reverse_drift(u, t), m.reverse_dispersion, 1, key) is None
    assert fused_csgm(x1, ts, m.reverse_drift, _model().reverse_dispersion, 1, key) is None      # another model's closure
    assert fused_csgm(x1, ts, m.reverse_dispersion, m.reverse_drift, 1, key) is None             # right model, wrong roles
    big = _model(d=129, T=2)
    assert fused_csgm(np.zeros(129, np.float32), big.ts_np, big.reverse_drift, big.reverse_dispersion, 1, key) is None
    assert _model(d=128, T=2).fused_supported(131072) and not big.fused_supported(1)
    assert not m.fused_supported(0) and not m.fused_supported(131073)
    assert m.same_grid(ts) and not m.same_grid(ts + 1e-3)


def test_csgm_entry_points_declared_exported_and_bound():
    import fbs_amd
    from fbs_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fbsmi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fbsmi_[a-z0-9_]+)\s*\(", text))
    L = ctypes.CDLL(_lib.build())
    for name in ENTRY_POINTS:
        assert name in declared, f"{name} is not declared in include/fbsmi.h"
        assert hasattr(L, name), f"{name} is not exported by libfbsmi"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert "fbsmi_csgm_model" in text
    assert [f[0] for f in _lib.CSGMModelStruct._fields_] == ["d", "T", "A", "cvec", "ddt", "s", "m_ref", "S_ref"]
    assert ctypes.sizeof(_lib.CSGMModelStruct) == 2 * 4 + 6 * 8
    assert L.fbsmi_abi_version() == 1
    assert fbs_amd.GaussianCSGM is fbs_amd.lg_csgm.GaussianCSGM and "GaussianCSGM" in fbs_amd.__all__
