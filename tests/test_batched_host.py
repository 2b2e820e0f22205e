"""CPU: the batched closure-tier entry points (fbs_amd/csrc/fbsmi_batch.hip) are exported and refuse bad calls on the host,
before any HIP call; the host key schedule of gibbs_kernel_batched equals the nested splits of gibbs_kernel / _forward."""
import ctypes

import numpy as np

ARG, UNSUPPORTED = -1, -3
P = 0x1000          # a non-null pointer value: the refusals below never dereference it
NAMES = ("fbsmi_normalise_batched", "fbsmi_cond_killing_batched", "fbsmi_em_concat_batched", "fbsmi_em_finish_batched")


def test_library_has_the_four_symbols():
    from fbs_amd import _lib
    L = ctypes.CDLL(_lib.build())
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES
    assert _lib.lib().fbsmi_abi_version() == 1


def _mask(du=9, dv=55, nmasks=1, u_off=P, v_off=P, role=P):
    from fbs_amd import _lib
    return _lib.EMMaskBatchStruct(du, dv, nmasks, u_off, v_off, role)


def test_normalise_and_killing_refusals():
    from fbs_amd import _lib
    L = _lib.lib()
    nb, ck = L.fbsmi_normalise_batched, L.fbsmi_cond_killing_batched
    assert nb(P, 3, 1025, 1, P, None, None) == UNSUPPORTED and b"1024" in L.fbsmi_last_error()
    assert nb(None, 3, 8, 1, P, None, None) == ARG
    assert nb(P, 3, 8, 1, None, None, None) == ARG
    assert nb(P, 0, 8, 1, P, None, None) == ARG
    assert nb(P, 3, 0, 1, P, None, None) == ARG
    assert nb(P, -1, 8, 0, P, P, None) == ARG
    assert ck(P, P, P, P, 3, 1025, P, None) == UNSUPPORTED
    for hole in range(4):
        a = [P, P, P, P]
        a[hole] = None
        assert ck(*a, 3, 8, P, None) == ARG
    assert ck(P, P, P, P, 3, 8, None, None) == ARG
    assert ck(P, P, P, P, 0, 8, P, None) == ARG
    assert ck(P, P, P, P, 3, 0, P, None) == ARG


def test_em_refusals():
    from fbs_amd import _lib
    L = _lib.lib()
    cat, fin = L.fbsmi_em_concat_batched, L.fbsmi_em_finish_batched
    ref = ctypes.byref

    def concat(mask, us=P, vp=P, B=3, n=8, img=P):
        return cat(ref(mask) if mask is not None else None, us, None, vp, B, n, 0, img, None)

    def finish(mask, us=P, net=P, v=P, vp=P, keys=P, B=3, n=8, us_new=P + 64, lw=P):
        return fin(ref(mask) if mask is not None else None, us, None, net, 0, 0, 0.1, 0.2, 0.01, 0.1, v, vp, keys, B, n,
                   None, None, us_new, lw, None)

    for call in (concat, finish):
        assert call(None) == ARG
        assert call(_mask(u_off=None)) == ARG
        assert call(_mask(role=None)) == ARG
        assert call(_mask(v_off=None)) == ARG
        assert call(_mask(), B=0) == ARG
        assert call(_mask(), n=0) == ARG
        assert call(_mask(), n=1025) == UNSUPPORTED
        assert call(_mask(nmasks=2)) == ARG                       # neither 1 nor B = 3
        assert call(_mask(nmasks=0)) == ARG
        assert call(_mask(du=2 ** 22 + 1), n=1024) == ARG         # n * du = 2^32 + 1024 > 2^32 - 4
        assert call(_mask(), us=None) == ARG
    assert concat(_mask(), vp=None) == ARG
    assert concat(_mask(), img=None) == ARG
    assert finish(_mask(), net=None) == ARG
    assert finish(_mask(), v=None) == ARG
    assert finish(_mask(), keys=None) == ARG
    assert finish(_mask(), us_new=None, lw=None) == ARG           # nothing asked for
    assert finish(_mask(), us_new=P) == ARG                       # us_new aliases us


def test_key_schedule_equals_the_nested_splits():
    """gibbs.py:126,147 and csmc.py:150,157,136 for B = 3 sweeps of T = 4 steps."""
    from fbs_amd import ops
    from fbs_amd.samplers.gibbs_batched import sweep_key_schedule
    B, T = 3, 4
    keys = ops.split(ops.PRNGKey(2024), B)
    sk = sweep_key_schedule(keys, T)
    assert sk["resampling"].shape == (T, B, 2) and sk["transition"].shape == (T, B, 2)
    assert all(a.dtype == np.uint32 for a in sk.values())
    for b in range(B):
        key_fwd, key_csmc, key_bridge = ops.split(keys[b], 3)                     # gibbs.py:126
        k_fwd, k_x0, k_us, k_bs = ops.split(key_csmc, 4)                          # :147
        key_init, key_scan = ops.split(k_fwd, 2)                                  # csmc.py:150
        step = ops.split(key_scan, T)                                             # :157
        for name, want in (("fwd", key_fwd), ("bridge", key_bridge), ("x0", k_x0), ("us", k_us), ("bs", k_bs),
                           ("init", key_init)):
            np.testing.assert_array_equal(sk[name][b], want, err_msg=name)
        for k in range(T):
            k_res, k_tr = ops.split(step[k], 2)                                   # :136
            np.testing.assert_array_equal(sk["resampling"][k, b], k_res)
            np.testing.assert_array_equal(sk["transition"][k, b], k_tr)
    # distinct sweeps, distinct keys
    assert len({tuple(r) for r in sk["transition"].reshape(-1, 2)}) == B * T
