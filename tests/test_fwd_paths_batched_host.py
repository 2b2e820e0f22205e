"""CPU: fbsmi_linear_path_batched and fbsmi_em_fwd_step_batched (fbs_amd/csrc/fbsmi_batch.hip) are exported and refuse bad
calls on the host, before any HIP call, each refusal with every other argument valid."""
import ctypes

import pytest

OK, ARG, UNSUPPORTED = 0, -1, -3
P = 0x1000          # a non-null pointer value: the refusals below never dereference it
NAMES = ("fbsmi_linear_path_batched", "fbsmi_em_fwd_step_batched")
DU, DV = 9, 55
D = DU + DV


def test_library_has_the_two_symbols():
    from fbs_amd import _lib
    L = ctypes.CDLL(_lib.build())
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES
    assert _lib.lib().fbsmi_abi_version() == 1


def _mask(du=DU, dv=DV, nmasks=1, u_off=P, v_off=P, role=P):
    from fbs_amd import _lib
    return _lib.EMMaskBatchStruct(du, dv, nmasks, u_off, v_off, role)


def _ref(m):
    return ctypes.byref(m) if m is not None else None


def _linear(mask="default", D=D, F=P, S=P, x0s=P, y0s=P, keys=P, B=3, T=5, reverse=1, out_u=P, out_v=P):
    """The call with every argument valid unless overridden; -> (status, last error)."""
    from fbs_amd import _lib
    L = _lib.lib()
    m = _mask() if isinstance(mask, str) else mask
    rc = L.fbsmi_linear_path_batched(_ref(m), D, F, S, x0s, y0s, keys, B, T, reverse, out_u, B * DU, DU, out_v, B * DV, DV, None)
    return rc, L.fbsmi_last_error()


def _step(mask="default", D=D, x0s=P, y0s=P, x=P, net=P, net_dtype=0, keys=P, noise_total=None, noise_offset=None, B=3,
          x_out=P, store_slot=2, out_u=P, out_v=P):
    from fbs_amd import _lib
    L = _lib.lib()
    m = _mask() if isinstance(mask, str) else mask
    noise_total = 2 * D if noise_total is None else noise_total   # the second of two sub-steps, unless overridden
    noise_offset = noise_total - D if noise_offset is None else noise_offset
    rc = L.fbsmi_em_fwd_step_batched(_ref(m), D, x0s, y0s, x, net, net_dtype, 0.01, 0.3, keys, noise_total, noise_offset, B,
                                     x_out, store_slot, out_u, B * DU, DU, out_v, B * DV, DV, None)
    return rc, L.fbsmi_last_error()


SHARED = {
    "null role": dict(mask=_mask(role=None)),
    "du < 1": dict(mask=_mask(du=0, dv=D)),
    "dv < 0": dict(mask=_mask(du=D + 1, dv=-1)),
    "D is not du + dv": dict(D=D + 1),
    "D = 0 without a mask": dict(mask=None, D=0),
    "D = 2^31 without a mask": dict(mask=None, D=2 ** 31),
    "B = 0": dict(B=0),
    "B < 0": dict(B=-1),
    "B = 2^31": dict(B=2 ** 31),
    "nmasks = 2 for B = 3": dict(mask=_mask(nmasks=2)),
    "nmasks = 0": dict(mask=_mask(nmasks=0)),
    "null out_u": dict(out_u=None),
    "a grid of 2^31 workgroups": dict(mask=None, D=2 ** 14, B=2 ** 25),      # 64 workgroups per ensemble
}

LINEAR = dict(SHARED, **{
    "null F": dict(F=None),
    "null S": dict(S=None),
    "null x0s": dict(x0s=None),
    "null y0s with dv > 0": dict(y0s=None),
    "null keys": dict(keys=None),
    "T < 0": dict(T=-1),
    "T * D > 2^32 - 4": dict(mask=None, D=2 ** 22, T=2 ** 10),
})

STEP = dict(SHARED, **{
    "null x_out": dict(x_out=None),
    "net without x": dict(x=None),
    "net without keys": dict(keys=None),
    "first launch without x0s": dict(net=None, x0s=None),
    "first launch without y0s, dv > 0": dict(net=None, y0s=None),
    "net_dtype 2": dict(net_dtype=2),
    "net_dtype -1": dict(net_dtype=-1),
    "noise_offset < 0": dict(noise_offset=-1),
    "noise_offset + D > noise_total": dict(noise_offset=D + 1),
    "noise_total > 2^32 - 4": dict(noise_total=2 ** 32 - 3),
})


@pytest.mark.parametrize("name", sorted(LINEAR))
def test_linear_path_refusals(name):
    rc, err = _linear(**LINEAR[name])
    assert rc == ARG, (name, rc)
    assert err, name                                               # a non-empty fbsmi_last_error


@pytest.mark.parametrize("name", sorted(STEP))
def test_step_refusals(name):
    rc, err = _step(**STEP[name])
    assert rc == ARG, (name, rc)
    assert err, name


def test_what_may_be_null():
    """The observed output, the mask (identity layout: y0s is then not read) and, without an observed part, y0s are
    optional; a store_slot < 0 needs no path output.  Each call below is refused for ANOTHER reason (null keys / null
    x_out), named in its message, so that nothing is launched."""
    for kw in (dict(out_v=None), dict(mask=None, y0s=None), dict(mask=_mask(du=D, dv=0, v_off=None), y0s=None)):
        rc, err = _linear(keys=None, **kw)
        assert rc == ARG and b"null keys" in err, (kw, rc, err)
    for kw in (dict(out_v=None), dict(mask=None, y0s=None), dict(store_slot=-1, out_u=None),
               dict(x0s=None, y0s=None),                           # an update step does not read the initial point
               dict(net=None, x=None, keys=None, noise_total=0, noise_offset=0)):   # nor the first launch the state
        rc, err = _step(x_out=None, **kw)
        assert rc == ARG and b"null x_out" in err, (kw, rc, err)


def test_nothing_is_refused_as_unsupported():
    """No row cap: the largest B, D and draw are arguments like any other."""
    for kw in (dict(B=2 ** 31 - 1, mask=None, D=64), dict(mask=None, D=2 ** 31 - 1, T=1),
               dict(mask=None, D=2 ** 20, T=2 ** 12 - 1)):
        rc, err = _linear(keys=None, **kw)
        assert rc == ARG and b"null keys" in err, (kw, rc, err)
