"""CPU: fbsmi_em_csgm_step_batched and fbsmi_normal_batched (fbs_amd/csrc/fbsmi_batch.hip) are exported and refuse bad calls on
the host, before any HIP call, each refusal with every other argument valid; the host key schedule of
make_image_csgm_batched equals the nested splits of make_image_csgm's conditional_sampler / euler_maruyama."""
import ctypes

import numpy as np
import pytest

OK, ARG, UNSUPPORTED = 0, -1, -3
P = 0x1000          # a non-null pointer value: the refusals below never dereference it
NAMES = ("fbsmi_em_csgm_step_batched", "fbsmi_normal_batched")


def test_library_has_the_two_symbols():
    from fbs_amd import _lib
    L = ctypes.CDLL(_lib.build())
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES
    assert _lib.lib().fbsmi_abi_version() == 1


def _mask(du=9, dv=55, nmasks=1, u_off=P, v_off=P, role=P):
    from fbs_amd import _lib
    return _lib.EMMaskBatchStruct(du, dv, nmasks, u_off, v_off, role)


def _step(mask="default", u=P, net=P, net_dtype=0, scan_keys=P, noise_total=5 * 9, noise_offset=2 * 9, y0=P, est_keys=P,
          out_dtype=0, img=P, B=3, u_new=P):
    """The call with every argument valid unless overridden; -> (status, last error)."""
    from fbs_amd import _lib
    L = _lib.lib()
    m = _mask() if isinstance(mask, str) else mask
    rc = L.fbsmi_em_csgm_step_batched(ctypes.byref(m) if m is not None else None, u, net, net_dtype, 0.1, 0.2, 0.01, 0.3,
                                      scan_keys, noise_total, noise_offset, y0, 0.9, 0.4, est_keys, out_dtype, img, B, u_new,
                                      None)
    return rc, L.fbsmi_last_error()


REFUSALS = {
    "null mask": dict(mask=None),
    "null u_off": dict(mask=_mask(u_off=None)),
    "null v_off with dv > 0": dict(mask=_mask(v_off=None)),
    "null role": dict(mask=_mask(role=None)),
    "du < 1": dict(mask=_mask(du=0), noise_offset=0),
    "null u": dict(u=None),
    "null y0 with dv > 0": dict(y0=None),
    "null scan keys": dict(scan_keys=None),
    "null est keys": dict(est_keys=None),
    "neither half": dict(net=None, img=None),
    "net without u_new": dict(u_new=None),
    "B = 0": dict(B=0),
    "B < 0": dict(B=-1),
    "B = 2^31": dict(B=2 ** 31, mask=_mask(nmasks=1)),
    "nmasks = 2 for B = 3": dict(mask=_mask(nmasks=2)),
    "nmasks = 0": dict(mask=_mask(nmasks=0)),
    "net_dtype 2": dict(net_dtype=2),
    "net_dtype -1": dict(net_dtype=-1),
    "out_dtype 2": dict(out_dtype=2),
    "noise_offset < 0": dict(noise_offset=-1),
    "noise_offset + du > noise_total": dict(noise_offset=5 * 9 - 8),
    "noise_total > 2^32 - 4": dict(noise_total=2 ** 32 - 3),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_step_refusals(name):
    rc, err = _step(**REFUSALS[name])
    assert rc == ARG, (name, rc)
    assert err, name                                               # a non-empty fbsmi_last_error


def test_step_refuses_nothing_as_unsupported():
    """There is no row cap: the largest B, the largest draw and a wide image are arguments like any other.  (The calls
    below are refused for another reason, a null u, so that nothing is launched; their status is ARG, never UNSUPPORTED,
    and the message names the null pointer, not a size.)"""
    for kw in (dict(B=2 ** 31 - 1), dict(noise_total=2 ** 32 - 4, noise_offset=2 ** 32 - 4 - 9),
               dict(mask=_mask(du=2 ** 20, dv=2 ** 21), noise_total=2 ** 22, noise_offset=0)):
        rc, err = _step(u=None, **kw)
        assert rc == ARG and b"null u" in err, (kw, rc, err)


def test_y0_may_be_null_without_an_observed_part():
    """dv == 0: y0 and v_off are not needed; the call then fails on the next check only (here: neither half)."""
    rc, err = _step(mask=_mask(dv=0, v_off=None), y0=None, net=None, img=None)
    assert rc == ARG and b"neither" in err


def test_normal_batched_refusals():
    from fbs_amd import _lib
    L = _lib.lib()
    nb = L.fbsmi_normal_batched
    for args in ((None, 3, 8, P), (P, 3, 8, None), (P, 0, 8, P), (P, -1, 8, P), (P, 3, -1, P), (P, 3, 2 ** 32 - 3, P),
                 (P, 2 ** 31, 8, P),                               # more workgroups than a grid holds
                 (P, 2 ** 26, 2 ** 20, P)):                        # 64 workgroups per row: 2^32 of them
        assert nb(*args, None) == ARG, args
        assert L.fbsmi_last_error(), args
    assert nb(P, 3, 0, None, None) == OK                           # nothing to draw: nothing launched, out not needed


def test_key_schedule_equals_the_nested_splits(oracle):
    """csgm.py conditional_sampler (init, sde) = split(key); euler_maruyama (scan, est) = split(sde), split(est, nsteps)."""
    from fbs_amd.csgm import csgm_key_schedule
    T = 5
    for B in (1, 3):
        keys = np.asarray(oracle.split(oracle.PRNGKey(2025), B), np.uint32).reshape(B, 2)
        ks = csgm_key_schedule(keys, T)
        assert ks["init"].shape == (B, 2) and ks["scan"].shape == (B, 2) and ks["est"].shape == (T, B, 2)
        assert all(a.dtype == np.uint32 for a in ks.values())
        for b in range(B):
            key_init, key_sde = oracle.split(keys[b], 2)
            key_scan, key_est = oracle.split(key_sde, 2)
            np.testing.assert_array_equal(ks["init"][b], key_init)
            np.testing.assert_array_equal(ks["scan"][b], key_scan)
            np.testing.assert_array_equal(ks["est"][:, b], np.asarray(oracle.split(key_est, T)).reshape(T, 2))
        assert len({tuple(r) for r in ks["est"].reshape(-1, 2)}) == B * T    # distinct trajectories and steps, distinct keys
