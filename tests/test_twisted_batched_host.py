"""CPU: the five entry points of the image twisted-SMC step (fbs_amd/csrc/fbsmi_batch.hip: fbsmi_tw_img_gather_batched,
fbsmi_tw_img_twist_batched, fbsmi_tw_img_cotangent_batched, fbsmi_tw_img_propose_batched, fbsmi_categorical_batched) are
exported and refuse bad calls on the host, before any HIP call, each refusal with every other argument valid."""
import ctypes

import pytest

OK, ARG, UNSUPPORTED = 0, -1, -3
P = 0x1000          # a non-null pointer value: the refusals below never dereference it
Q = 0x2000          # another one, where two arrays must not alias
NAMES = ("fbsmi_tw_img_gather_batched", "fbsmi_tw_img_twist_batched", "fbsmi_tw_img_cotangent_batched",
         "fbsmi_tw_img_propose_batched", "fbsmi_categorical_batched")


def test_library_has_the_five_symbols():
    from fbs_amd import _lib
    L = ctypes.CDLL(_lib.build())
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES
    assert _lib.lib().fbsmi_abi_version() == 1
    from fbs_amd.twisted import make_image_twisted_batched   # noqa: F401


def _mask(du=25, dv=56, nmasks=1, u_off=P, v_off=P, role=P):
    from fbs_amd import _lib
    return _lib.EMMaskBatchStruct(du, dv, nmasks, u_off, v_off, role)


def _ref(mask):
    m = _mask() if isinstance(mask, str) else mask
    return ctypes.byref(m) if m is not None else None


def _status(name, *args):
    from fbs_amd import _lib
    L = _lib.lib()
    return getattr(L, name)(*args, None), L.fbsmi_last_error()


def _gather(X=P, lp=P, A=P, B=3, n=5, D=81, Xp=Q, lpg=P):
    return _status("fbsmi_tw_img_gather_batched", X, lp, A, B, n, D, Xp, lpg)


def _twist(mask="default", X=P, net=P, net_dtype=0, y=P, tl=P, pl=P, lpg=P, B=3, n=5, lp=P, lw=P):
    return _status("fbsmi_tw_img_twist_batched", _ref(mask), X, net, net_dtype, 0.1, 0.2, 0.01, 0.3, y, tl, pl, lpg, B, n, lp, lw)


def _cotangent(mask="default", X=P, net=P, net_dtype=0, y=P, B=3, n=5, ct=P):
    return _status("fbsmi_tw_img_cotangent_batched", _ref(mask), X, net, net_dtype, 0.1, 0.2, 0.01, 0.3, y, B, n, ct)


def _propose(mask="default", Xp=P, net=P, net_dtype=0, vjp=P, y=P, keys=P, B=3, n=5, X_new=Q, tl=P, pl=P, out_dtype=0,
             X_new_net=None):
    return _status("fbsmi_tw_img_propose_batched", _ref(mask), Xp, net, net_dtype, vjp, 0.1, 0.2, 0.01, 0.05, 0.3, y, keys, B,
                   n, X_new, tl, pl, out_dtype, X_new_net)


def _categorical(keys=P, w=P, B=3, n=5, out=P):
    return _status("fbsmi_categorical_batched", keys, w, B, n, out)


MASK_REFUSALS = {
    "null mask": dict(mask=None),
    "null v_off with dv > 0": dict(mask=_mask(v_off=None)),
    "null role": dict(mask=_mask(role=None)),
    "B = 0": dict(B=0),
    "B < 0": dict(B=-1),
    "n = 0": dict(n=0),
    "n < 0": dict(n=-2),
    "nmasks = 2 for B = 3": dict(mask=_mask(nmasks=2)),
    "nmasks = 0": dict(mask=_mask(nmasks=0)),
    "n D > 2^32 - 4": dict(n=1024, mask=_mask(du=2 ** 21, dv=2 ** 21)),       # 2^32 elements
    "null X": None,
    "null net": dict(net=None),
    "null y with dv > 0": dict(y=None),
    "net_dtype 2": dict(net_dtype=2),
    "net_dtype -1": dict(net_dtype=-1),
}
CALLS = {"twist": (_twist, "X"), "cotangent": (_cotangent, "X"), "propose": (_propose, "Xp")}


@pytest.mark.parametrize("name", sorted(MASK_REFUSALS))
@pytest.mark.parametrize("call", sorted(CALLS))
def test_mask_kernels_refuse(call, name):
    fn, xname = CALLS[call]
    kw = MASK_REFUSALS[name] if MASK_REFUSALS[name] is not None else {xname: None}
    rc, err = fn(**kw)
    assert rc == ARG, (call, name, rc)
    assert err, (call, name)                                       # a non-empty fbsmi_last_error


@pytest.mark.parametrize("call", sorted(CALLS))
def test_mask_kernels_answer_unsupported_for_more_than_1024_rows(call):
    rc, err = CALLS[call][0](n=1025)
    assert rc == UNSUPPORTED and b"1024" in err, (call, rc, err)


def test_the_largest_draw_is_an_argument_like_any_other():
    """n D = 2^32 - 4 exactly passes the size checks: the call is then refused for another reason (a null net), never for
    its size."""
    for fn in (_twist, _cotangent, _propose):
        rc, err = fn(n=4, mask=_mask(du=2 ** 29, dv=2 ** 29 - 1), net=None)
        assert rc in (ARG, UNSUPPORTED) and b"2^32" not in err, (rc, err)


def test_further_refusals_of_each_entry_point():
    for kw in (dict(lp=None), dict(tl=None), dict(pl=None), dict(lpg=None)):                # weights without an input
        rc, err = _twist(**kw)
        assert rc == ARG and err, kw
    for kw in (dict(ct=None),):
        assert _cotangent(**kw)[0] == ARG, kw
    for kw in (dict(vjp=None), dict(keys=None), dict(X_new=None), dict(tl=None), dict(pl=None), dict(out_dtype=2),
               dict(out_dtype=-1), dict(X_new=P), dict(X_new_net=P)):                        # the last two: aliases of Xp
        rc, err = _propose(**kw)
        assert rc == ARG and err, kw
    for kw in (dict(X=None), dict(A=None), dict(Xp=None), dict(lp=None), dict(B=0), dict(n=0), dict(D=0), dict(Xp=P),
               dict(n=1024, D=2 ** 22)):
        rc, err = _gather(**kw)
        assert rc == ARG and err, kw
    assert _gather(n=1025)[0] == UNSUPPORTED
    for kw in (dict(keys=None), dict(w=None), dict(out=None), dict(B=0), dict(B=-1), dict(n=0), dict(B=2 ** 31)):
        rc, err = _categorical(**kw)
        assert rc == ARG and err, kw
    assert _categorical(n=1025)[0] == UNSUPPORTED


def test_optional_arrays_may_be_null():
    """Calls that are valid up to one null pointer checked LAST stay refused for that pointer alone: the optional arrays
    (lw with its three inputs, lp_prev_g, y without an observed part) are not what is complained about."""
    rc, err = _twist(lw=None, tl=None, pl=None, lpg=None, lp=None)
    assert rc == ARG and b"null pointer" in err
    rc, err = _twist(mask=_mask(dv=0, v_off=None), y=None, lp=None)
    assert rc == ARG and b"null pointer" in err
    rc, err = _gather(lpg=None, lp=None, Xp=None)
    assert rc == ARG and b"null pointer" in err
