"""CPU: the host side of the batched image backward passes -- the key schedule of bootstrap_backward_smoother_batched
against oracle.split, the size rule that decides whether gibbs_init_batched(smoother='reuse') keeps the filter's network
outputs, and the refusals of fbsmi_em_translp_batched / fbsmi_backsim_pick_batched, which are decided before any HIP call."""
import ctypes

import numpy as np
import pytest

ARG, UNSUPPORTED = -1, -3
P = 0x1000          # a non-null pointer value: the refusals below never dereference it


@pytest.mark.parametrize("T", (1, 4))
@pytest.mark.parametrize("B", (1, 3))
def test_smoother_key_schedule_equals_the_nested_splits(oracle, B, T):
    """smc.py:108-110: the index of u_T is drawn with the PARENT key, the steps with split(split(key, 2)[1], T)."""
    from fbs_amd.samplers import smoother_key_schedule
    keys = oracle.split(oracle.PRNGKey(77 + 10 * B + T), B)
    sk = smoother_key_schedule(keys, T)
    assert sorted(sk) == ["last", "steps"]
    assert sk["last"].shape == (B, 2) and sk["steps"].shape == (T, B, 2)
    assert sk["last"].dtype == np.uint32 and sk["steps"].dtype == np.uint32
    for b in range(B):
        np.testing.assert_array_equal(sk["last"][b], keys[b])
        _, key_smoother = oracle.split(keys[b], 2)
        want = oracle.split(key_smoother, T)
        for s in range(T):
            np.testing.assert_array_equal(sk["steps"][s, b], want[s], err_msg=f"ensemble {b}, step {s}")
    if B > 1:
        assert not np.array_equal(sk["steps"][:, 0], sk["steps"][:, 1])


def test_smoother_key_schedule_takes_device_free_inputs(oracle):
    """A (2,) key is one ensemble; a list of keys works like an array."""
    from fbs_amd.samplers import smoother_key_schedule
    key = oracle.PRNGKey(5)
    one = smoother_key_schedule(key, 3)
    assert one["last"].shape == (1, 2) and one["steps"].shape == (3, 1, 2)
    two = smoother_key_schedule([key, key], 3)
    np.testing.assert_array_equal(two["steps"][:, 0], one["steps"][:, 0])
    np.testing.assert_array_equal(two["steps"][:, 1], one["steps"][:, 0])


def test_net_store_rule(monkeypatch):
    """'reuse' keeps T * B * n * D * itemsize bytes of network output and runs 'lockstep' when that exceeds
    LOCKSTEP_STORE_BYTES -- the module attribute, read at the time of the call."""
    from fbs_amd.samplers import gibbs_batched, net_store_fits
    T, B, n, D = 4, 3, 5, 64
    size = T * B * n * D * 4
    assert net_store_fits(T, B, n, D, 4, cap=size)
    assert not net_store_fits(T, B, n, D, 4, cap=size - 1)
    assert net_store_fits(T, B, n, D, 2, cap=size // 2) and not net_store_fits(T, B, n, D, 2, cap=size // 2 - 1)
    assert net_store_fits(T, B, n, D, 4)                                             # the default cap: 2 GiB
    # MNIST, 20 steps, 64 ensembles of 1024 rows: 2 055 208 960 bytes of bfloat16 fit, twice that of float32 do not
    assert net_store_fits(20, 64, 1024, 784, 2) and not net_store_fits(20, 64, 1024, 784, 4)
    monkeypatch.setattr(gibbs_batched, "LOCKSTEP_STORE_BYTES", size - 1)
    assert not net_store_fits(T, B, n, D, 4)
    monkeypatch.setattr(gibbs_batched, "LOCKSTEP_STORE_BYTES", size)
    assert net_store_fits(T, B, n, D, 4)
    assert net_store_fits(0, B, n, D, 4, cap=0)                                      # no steps, nothing to keep


def test_gibbs_init_batched_refuses_an_unknown_smoother():
    from fbs_amd.samplers import gibbs_init_batched
    with pytest.raises(ValueError, match="smoother"):
        gibbs_init_batched(np.zeros((2, 2), np.uint32), None, (9, 1), None, None, None, None, None, None, None, 5,
                           smoother="fused")


def _mask(du=9, dv=55, nmasks=1, u_off=P, v_off=P, role=P):
    from fbs_amd import _lib
    return _lib.EMMaskBatchStruct(du, dv, nmasks, u_off, v_off, role)


def test_library_has_the_two_symbols():
    from fbs_amd import _lib
    L = ctypes.CDLL(_lib.build())
    for n in ("fbsmi_em_translp_batched", "fbsmi_backsim_pick_batched"):
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES


def test_translp_refusals():
    from fbs_amd import _lib
    L = _lib.lib()
    ref = ctypes.byref

    def call(mask, us=P, us_stride=72, net=P, net_dtype=0, mode=0, u=P, u_stride=9, B=3, n=8, lw=P):
        return L.fbsmi_em_translp_batched(ref(mask) if mask is not None else None, us, us_stride, net, net_dtype, mode, 0.1,
                                          0.2, 0.01, 0.1, u, u_stride, B, n, lw, None)

    assert call(_mask(), n=1025) == UNSUPPORTED and b"1024" in L.fbsmi_last_error()
    assert call(_mask(du=2 ** 20 + 1, dv=0)) == UNSUPPORTED
    assert call(None) == ARG
    assert call(_mask(u_off=None)) == ARG
    for hole in ("us", "net", "u", "lw"):
        assert call(_mask(), **{hole: None}) == ARG, hole
    assert call(_mask(), B=0) == ARG
    assert call(_mask(), n=0) == ARG
    assert call(_mask(du=0)) == ARG
    assert call(_mask(nmasks=2)) == ARG
    assert call(_mask(), net_dtype=2) == ARG
    assert call(_mask(), mode=-1) == ARG
    assert call(_mask(), us_stride=-1) == ARG
    assert call(_mask(), u_stride=-1) == ARG
    assert call(_mask(), B=2 ** 22, n=1024) == ARG                                   # B * n = 2^32 rows: no such grid


def test_pick_refusals():
    from fbs_amd import _lib
    L = _lib.lib()

    def call(keys=P, lw=P, log_w=None, us=P, us_stride=72, B=3, n=8, du=9, idx=P, idx_stride=1, out=P, out_stride=9):
        return L.fbsmi_backsim_pick_batched(keys, lw, log_w, us, us_stride, B, n, du, idx, idx_stride, out, out_stride, None)

    assert call(n=1025) == UNSUPPORTED and b"1024" in L.fbsmi_last_error()
    for hole in ("keys", "lw", "us", "idx", "out"):
        assert call(**{hole: None}) == ARG, hole
    assert call(B=0) == ARG
    assert call(n=0) == ARG
    assert call(du=0) == ARG
    assert call(B=2 ** 31) == ARG
    for stride in ("us_stride", "idx_stride", "out_stride"):
        assert call(**{stride: -1}) == ARG, stride
