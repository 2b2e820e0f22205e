"""CPU: the Gaussian Schrodinger-bridge tables (fbs_amd.gaussian_sb.sb_tables) against make_gaussian_bw_sb's own closures,
the ABI of the Euler-Maruyama forward process refusing bad arguments before any device call, and the exact fmaf of the
test restatement against libm."""
import ctypes
import ctypes.util

import numpy as np
import pytest

from sb_restate import fmaf, sb_problem


@pytest.mark.parametrize("d,sig,nsub", [(3, 1.0, 10), (5, 0.7, 3)])
def test_sb_tables_match_the_closed_form(d, sig, nsub):
    from fbs_amd.gaussian_sb import sb_tables
    from fbs_amd.sdes import make_gaussian_bw_sb
    m0, c0, m1, c1 = sb_problem(d, seed=d)
    T = 12
    ts = np.linspace(0.0, 1.0, T + 1)
    tab = sb_tables(m0, c0, m1, c1, ts, d, sig=sig, nsub=nsub)
    mean_t, cov_t, drift = make_gaussian_bw_sb(m0, c0, m1, c1, sig=sig)
    D = 2 * d
    rng = np.random.default_rng(1)
    assert tab["du"] == d and tab["dv"] == d and tab["nsub"] == nsub
    assert tab["G"].shape == (T, D, D) and tab["M"].shape == (T * nsub, D, D) and tab["s"].shape == (T * nsub,)
    dt = (ts[-1] - ts[0]) / T
    for k in range(T):
        z = rng.normal(size=(4, D))
        s_ = 1.0 - ts[k]
        score = -np.linalg.solve(cov_t(s_), (z - mean_t(s_)).T).T
        want = -drift(z, s_) + sig ** 2 * score                          # sb/gibbs.py:82-83
        got = z @ tab["G"][k].T + tab["g"][k]
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10 * np.abs(want).max())
        h = abs(ts[k + 1] - ts[k]) / nsub
        assert tab["ddt"][k] == h
        for j, tau in enumerate(np.linspace(ts[k], ts[k + 1] - h, nsub)):
            r = k * nsub + j
            want_f = drift(z, tau)
            np.testing.assert_allclose(z @ tab["M"][r].T + tab["c"][r], want_f, rtol=1e-10, atol=1e-10 * np.abs(want_f).max())
            assert tab["s"][r] == sig * np.sqrt(h)
    np.testing.assert_allclose(tab["sd"], np.sqrt(dt) * sig, rtol=1e-15)
    np.testing.assert_allclose(tab["lognorm"], np.log(2 * np.pi * tab["sd"] ** 2), rtol=1e-15)
    assert not tab["F"].any() and not tab["sqQ"].any()


def test_sb_tables_refuse_nsub_zero():
    from fbs_amd.gaussian_sb import sb_tables
    m0, c0, m1, c1 = sb_problem(2)
    with pytest.raises(ValueError):
        sb_tables(m0, c0, m1, c1, np.linspace(0, 1, 5), 2, nsub=0)


def test_em_forward_abi_refuses_bad_arguments():
    """fbsmi_lg_sweep_set_em_forward and fbsmi_lg_em_path check their arguments before anything touches the device (this
    machine has none): -1 and an error text."""
    from fbs_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    good = _lib.EMForwardStruct(10, p, p, p, p)
    fake_handle = ctypes.c_void_p(p)   # never dereferenced: the table checks come first
    assert L.fbsmi_lg_sweep_set_em_forward(None, ctypes.byref(good)) == -1
    assert L.fbsmi_lg_sweep_set_em_forward(fake_handle, None) == -1
    for bad in (_lib.EMForwardStruct(0, p, p, p, p), _lib.EMForwardStruct(-3, p, p, p, p),
                _lib.EMForwardStruct(10, None, p, p, p), _lib.EMForwardStruct(10, p, None, p, p),
                _lib.EMForwardStruct(10, p, p, None, p), _lib.EMForwardStruct(10, p, p, p, None)):
        assert L.fbsmi_lg_sweep_set_em_forward(fake_handle, ctypes.byref(bad)) == -1
        assert len(L.fbsmi_last_error()) > 0
        assert L.fbsmi_lg_em_path(p, ctypes.byref(bad), p, 4, 2, p, None) == -1
    assert L.fbsmi_lg_em_path(None, ctypes.byref(good), p, 4, 2, p, None) == -1
    assert L.fbsmi_lg_em_path(p, None, p, 4, 2, p, None) == -1
    assert L.fbsmi_lg_em_path(p, ctypes.byref(good), None, 4, 2, p, None) == -1
    assert L.fbsmi_lg_em_path(p, ctypes.byref(good), p, 4, 2, None, None) == -1
    assert L.fbsmi_lg_em_path(p, ctypes.byref(good), p, 0, 2, p, None) == -1
    assert L.fbsmi_lg_em_path(p, ctypes.byref(good), p, 4, 0, p, None) == -1
    assert L.fbsmi_lg_em_path(p, ctypes.byref(good), p, 4, 257, p, None) == -3


def test_restatement_fmaf_is_exact():
    """The vectorised fmaf of the test restatement equals libm's fmaf, including a double-rounding tie that a plain float64
    evaluation gets wrong."""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(3)
    a = rng.normal(size=3000).astype(np.float32)
    b = (rng.normal(size=3000) * np.exp(rng.uniform(-20, 20, 3000))).astype(np.float32)
    c = (rng.normal(size=3000) * np.exp(rng.uniform(-20, 20, 3000))).astype(np.float32)
    a[:2], b[:2], c[:2] = np.float32(1 + 2 ** -23), np.float32(1 - 2 ** -23), np.float32(2 ** 24 + 2)
    b[1], c[1] = np.float32(-(1 - 2 ** -23)), np.float32(-(2 ** 24 + 2))
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    got = fmaf(a, b, c)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    naive = (a.astype(np.float64) * b + c).astype(np.float32)
    assert naive[0] != want[0]   # the crafted tie: float64 then float32 rounds twice
