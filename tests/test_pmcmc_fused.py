"""Host side of the fused pMCMC engine: the four entry points in header, library and binding, and the float64 tables
handed to fbsmi_lg_pmcmc_create against the closed forms oracle.lg_ref_sampler evaluates (restated here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import toy_2d, toy_4d, toy_31

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("fbsmi_lg_pmcmc_create", "fbsmi_lg_pmcmc_destroy", "fbsmi_lg_pmcmc_step", "fbsmi_lg_pmcmc_chain")


def test_pmcmc_entry_points_declared_exported_and_bound():
    from fbs_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fbsmi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fbsmi_[a-z0-9_]+)\s*\(", text))
    L = ctypes.CDLL(_lib.build())
    for name in ENTRY_POINTS:
        assert name in declared, f"{name} is not declared in include/fbsmi.h"
        assert hasattr(L, name), f"{name} is not exported by libfbsmi"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert "fbsmi_lg_pmcmc_tables" in text
    # the struct mirrors the header: four double/float table pointers + mean_coef, four floats, two int32
    names = [f[0] for f in _lib.LGPmcmcTablesStruct._fields_]
    assert names == ["m_u", "m_v", "gain", "chol", "mean_coef", "c0", "beta", "one_minus_beta", "c1", "use_pcn", "which_u"]
    assert ctypes.sizeof(_lib.LGPmcmcTablesStruct) == 5 * 8 + 4 * 4 + 2 * 4


def _terminal_moments(toy, sde, ts):
    from fbs_amd.sdes.linear import discretise_linear_sde_np
    Ft, Qt = discretise_linear_sde_np(sde, ts[-1], ts[0])
    m0 = np.asarray(toy["m0"], np.float64)
    return Ft * m0, Ft ** 2 * np.asarray(toy["cov0"], np.float64) + Qt * np.eye(m0.size)


@pytest.mark.parametrize("toy", [toy_2d, toy_4d, toy_31])
@pytest.mark.parametrize("delta", [None, 0.1, 0.005])
def test_pmcmc_tables_closed_forms(toy, delta):
    from fbs_amd.linear_gaussian import lg_pmcmc_tables
    from fbs_amd.sdes import StationaryConstLinearSDE
    toy = toy()
    du = toy["du"]
    ts = np.linspace(0, 3.0, 41)
    m_ref, cov_ref = _terminal_moments(toy, StationaryConstLinearSDE(-0.5, 1.0), ts)
    tab = lg_pmcmc_tables(m_ref, cov_ref, du, delta)
    # the expressions of oracle.lg_ref_sampler (gp_pmcmc.py:130-133), float64
    gain = cov_ref[:du, du:] @ np.linalg.inv(cov_ref[du:, du:])
    cov_ = cov_ref[:du, :du] - gain @ cov_ref[du:, :du]
    chol = np.linalg.cholesky(cov_)
    for name, want in (("m_u", m_ref[:du]), ("m_v", m_ref[du:]), ("gain", gain)):
        assert tab[name].dtype == np.float64 and tab[name].shape == want.shape
        assert np.array_equal(tab[name].view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), name
    assert tab["chol"].dtype == np.float32 and tab["chol"].shape == (du, du)
    assert np.array_equal(tab["chol"].view(np.uint32), np.ascontiguousarray(chol.astype(np.float32)).view(np.uint32))
    assert np.array_equal(tab["chol"], np.tril(tab["chol"]))            # the LOWER factor
    assert np.allclose(tab["chol"].astype(np.float64) @ tab["chol"].astype(np.float64).T, cov_, rtol=1e-5, atol=1e-6)
    if delta is None:
        assert not tab["use_pcn"]
    else:
        beta = 2 / (2 + delta)
        assert tab["use_pcn"]
        for name, want in (("c0", np.float32(np.sqrt(delta / 2))), ("beta", np.float32(beta)),
                           ("one_minus_beta", np.float32(1 - beta)), ("c1", np.float32(np.sqrt(1 - beta)))):
            assert isinstance(tab[name], np.float32) and tab[name].view(np.uint32) == want.view(np.uint32), name


def test_pmcmc_tables_of_a_bridge_need_no_gpu():
    """The bridge's host tables (lg_pmcmc_tables on its terminal moments + the pCN mean coefficients) come from numpy
    alone; the bridge itself is built on the CPU device here, which launches nothing."""
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    toy = toy_4d()
    ts = np.linspace(0, 3.0, 41)
    sde = StationaryConstLinearSDE(-0.5, 1.0)
    br = fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], sde, ts, toy["du"], device="cpu")
    tab = br.pmcmc_tables_host(0.1)
    m_ref, cov_ref = _terminal_moments(toy, sde, ts)
    assert np.array_equal(tab["m_v"], m_ref[toy["du"]:])
    coef = np.asarray(sde.mean(ts, ts[0], 1.0), np.float32).reshape(-1)
    assert tab["mean_coef"].dtype == np.float32 and np.array_equal(tab["mean_coef"], coef)
    assert br.pmcmc_tables_host(None)["mean_coef"] is None
    assert br.fused_pmcmc_supported(64)


def test_samplers_export_pmcmc_chain():
    from fbs_amd import samplers
    assert callable(samplers.pmcmc_chain)
