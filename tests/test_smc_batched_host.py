"""CPU: fbsmi_resample_batched / fbsmi_em_propose_batched (fbs_amd/csrc/fbsmi_batch.hip) are exported and refuse bad calls
on the host, before any HIP call; the host key schedules of bootstrap_filter_batched and pmcmc_kernel_batched equal the
nested splits of bootstrap_filter, pmcmc_kernel and pmcmc_filter_step."""
import ctypes

import numpy as np

OK, ARG, UNSUPPORTED = 0, -1, -3
P = 0x1000          # a non-null pointer value: the refusals below never dereference it
NAMES = ("fbsmi_resample_batched", "fbsmi_em_propose_batched")


def test_library_has_the_two_symbols():
    from fbs_amd import _lib
    L = ctypes.CDLL(_lib.build())
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES
    assert _lib.lib().fbsmi_abi_version() == 1


def test_resample_refusals():
    from fbs_amd import _lib
    L = _lib.lib()
    rs = L.fbsmi_resample_batched
    for kind in (0, 1):
        assert rs(kind, P, P, 3, 1025, P, None) == UNSUPPORTED and b"1024" in L.fbsmi_last_error()
        for hole in range(3):
            a = [P, P, P]
            a[hole] = None
            assert rs(kind, a[0], a[1], 3, 8, a[2], None) == ARG
        assert rs(kind, P, P, 0, 8, P, None) == ARG
        assert rs(kind, P, P, 3, 0, P, None) == ARG
        assert rs(kind, P, P, -1, 8, P, None) == ARG
    assert rs(2, P, P, 3, 8, P, None) == UNSUPPORTED              # multinomial
    assert rs(3, P, P, 3, 8, P, None) == UNSUPPORTED              # killing
    assert rs(-1, P, P, 3, 8, P, None) == ARG
    assert rs(4, P, P, 3, 8, P, None) == ARG


def _mask(du=9, dv=55, nmasks=1, u_off=P, v_off=P, role=P):
    from fbs_amd import _lib
    return _lib.EMMaskBatchStruct(du, dv, nmasks, u_off, v_off, role)


def test_propose_refusals():
    from fbs_amd import _lib
    L = _lib.lib()
    ref = ctypes.byref

    def propose(mask, us=P, A=P, net=P, keys=P, B=3, n=8, us_new=P + 64, net_dtype=0, mode=0):
        return L.fbsmi_em_propose_batched(ref(mask) if mask is not None else None, us, A, net, net_dtype, mode, 0.1, 0.2,
                                          0.01, 0.1, keys, B, n, us_new, None)

    assert propose(None) == ARG
    assert propose(_mask(u_off=None)) == ARG
    assert propose(_mask(role=None)) == ARG
    assert propose(_mask(v_off=None)) == ARG
    assert propose(_mask(), B=0) == ARG
    assert propose(_mask(), n=0) == ARG
    assert propose(_mask(), n=1025) == UNSUPPORTED and b"1024" in L.fbsmi_last_error()
    assert propose(_mask(nmasks=2)) == ARG                        # neither 1 nor B = 3
    assert propose(_mask(nmasks=0)) == ARG
    assert propose(_mask(du=2 ** 22 + 1), n=1024) == ARG          # n * du = 2^32 + 1024 > 2^32 - 4
    assert propose(_mask(), A=None) == ARG                        # the ancestors are required
    assert propose(_mask(), us=None) == ARG
    assert propose(_mask(), net=None) == ARG
    assert propose(_mask(), keys=None) == ARG
    assert propose(_mask(), us_new=None) == ARG
    assert propose(_mask(), us_new=P) == ARG                      # us_new aliases us
    assert propose(_mask(), net_dtype=2) == ARG
    assert propose(_mask(), mode=2) == ARG


def test_filter_key_schedule_equals_the_nested_splits():
    """smc.py bootstrap_filter: split(key, 2) -> (init, steps), split(steps, T), per step (proposal, resampling)."""
    from fbs_amd import ops
    from fbs_amd.samplers import filter_key_schedule
    B, T = 3, 4
    keys = ops.split(ops.PRNGKey(2025), B)
    sk = filter_key_schedule(keys, T)
    assert sk["init"].shape == (B, 2) and sk["proposal"].shape == (T, B, 2) and sk["resampling"].shape == (T, B, 2)
    assert all(a.dtype == np.uint32 for a in sk.values())
    for b in range(B):
        key_init, key_steps = ops.split(keys[b], 2)
        np.testing.assert_array_equal(sk["init"][b], key_init)
        step = ops.split(key_steps, T)
        for k in range(T):
            k_prop, k_res = ops.split(step[k], 2)
            np.testing.assert_array_equal(sk["proposal"][k, b], k_prop)
            np.testing.assert_array_equal(sk["resampling"][k, b], k_res)
    assert len({tuple(r) for r in sk["proposal"].reshape(-1, 2)}) == B * T


def test_pmcmc_key_schedule_equals_the_nested_splits():
    """smc.py pmcmc_kernel: split(key, 4) -> (prop, u0, filter, mh); pmcmc_filter_step: split(filter, T), per step
    (proposal, resampling)."""
    from fbs_amd import ops
    from fbs_amd.samplers import pmcmc_key_schedule
    B, T = 3, 4
    keys = ops.split(ops.PRNGKey(2026), B)
    sk = pmcmc_key_schedule(keys, T)
    assert all(a.dtype == np.uint32 for a in sk.values())
    assert sk["proposal"].shape == (T, B, 2) and sk["resampling"].shape == (T, B, 2)
    for b in range(B):
        want = ops.split(keys[b], 4)
        for name, w in zip(("prop", "u0", "filter", "mh"), want):
            np.testing.assert_array_equal(sk[name][b], w, err_msg=name)
        step = ops.split(want[2], T)
        for k in range(T):
            k_prop, k_res = ops.split(step[k], 2)
            np.testing.assert_array_equal(sk["proposal"][k, b], k_prop)
            np.testing.assert_array_equal(sk["resampling"][k, b], k_res)
    assert len({tuple(r) for r in sk["resampling"].reshape(-1, 2)}) == B * T
