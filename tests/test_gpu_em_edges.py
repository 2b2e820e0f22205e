"""GPU: the image SMC-step kernels (fbsmi_em_concat / fbsmi_em_finish / fbsmi_em_transition_logpdf, fbs_amd/csrc/fbsmi_em.hip)
on every branch of their dispatch and at the edges of their masks -- the cases of tests/em_edges.py, bit for bit against
oracle/em.py.  Every case first asserts the plan it was written for (fbsmi_em_*_plan on the pointers it is about to pass), so
a changed threshold fails here instead of quietly moving the case to another kernel.  Outputs are pre-filled with NaN and
carry guard elements, every input is compared with its snapshot after the call, and us / net carry a spare row beyond n."""
import numpy as np
import pytest
import torch

import em_edges as E
from em_edges import GUARD, NAN_BITS

pytestmark = pytest.mark.gpu

_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.uint16): torch.int16}
_FILL = {torch.float32: float("nan"), torch.int32: 0, torch.int16: 0x7FC0}
_BITS = {torch.float32: torch.int32, torch.int32: torch.int32, torch.int16: torch.int16}


class Placed:
    """A host array in a device buffer, GUARD + shift elements in (NaN around floats); .ptr is its first element."""

    def __init__(self, arr, dev, shift=0):
        a = np.ascontiguousarray(arr).reshape(-1)
        tdt = _TORCH[a.dtype]
        self.n, self.first, self.esz = a.size, GUARD + int(shift), a.dtype.itemsize
        self.buf = torch.full((a.size + 2 * GUARD + int(shift),), _FILL[tdt], dtype=tdt, device=dev)
        if a.size:
            src = a.view(np.int16) if a.dtype == np.uint16 else a
            self.buf[self.first:self.first + a.size] = torch.from_numpy(src).to(dev)
        self.ptr = self.buf.data_ptr() + self.esz * self.first
        self.snap = self.buf.view(_BITS[tdt]).clone()

    def at(self, element):
        return self.ptr + self.esz * int(element)

    def unchanged(self):
        return torch.equal(self.buf.view(_BITS[self.buf.dtype]), self.snap)


class Output:
    """n elements of NaN sentinel between guards (float32, or bfloat16 as int16 bit patterns)."""

    def __init__(self, n, dev, shift=0, bf16=False):
        self.n, self.first, self.bf16 = int(n), GUARD + int(shift), bf16
        self.esz = 2 if bf16 else 4
        if bf16:
            self.buf = torch.full((self.n + 2 * GUARD + int(shift),), 0x7FC0, dtype=torch.int16, device=dev)
        else:
            self.buf = torch.full((self.n + 2 * GUARD + int(shift),), float("nan"), dtype=torch.float32, device=dev)
        self.ptr = self.buf.data_ptr() + self.esz * self.first

    def bits(self):
        h = self.buf.detach().cpu().numpy()
        return h.view(np.uint16) if self.bf16 else h.view(np.uint32)

    def check(self, want_bits, what):
        got, sentinel = self.bits(), (0x7FC0 if self.bf16 else NAN_BITS)
        want_bits = np.ascontiguousarray(want_bits).reshape(-1)
        assert want_bits.size == self.n, (what, want_bits.size, self.n)
        for name, part in (("in front", got[:self.first]), ("behind", got[self.first + self.n:])):
            bad = np.flatnonzero(part != sentinel)
            assert bad.size == 0, f"{what}: {bad.size} guard elements {name} overwritten, first {bad[:4]}"
        body = got[self.first:self.first + self.n]
        bad = np.flatnonzero(body != want_bits)
        assert bad.size == 0, f"{what}: {bad.size} of {self.n} differ, first {bad[:4]}: {body[bad[:4]]} vs {want_bits[bad[:4]]}"

    def untouched(self, what):
        bad = np.flatnonzero(self.bits() != (0x7FC0 if self.bf16 else NAN_BITS))
        assert bad.size == 0, f"{what}: {bad.size} sentinel elements overwritten, first {bad[:4]}"


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class FinishCall:
    """Device buffers of a fbsmi_em_finish case and the pointers it passes."""

    def __init__(self, x, dtype, dev, mask_shift=None):
        c = x.case
        sh = lambda name: c.shift.get(name, 0)
        self.x, self.dtype = x, dtype
        self.mask = E.DeviceMask(x.tables, dev, mask_shift)
        self.us = Placed(x.us, dev, sh("us")) if x.us is not None else None
        self.A = Placed(x.A, dev) if x.A is not None else None
        self.net = Placed(x.net_dev, dev, sh("net"))
        self.net_A = Placed(x.net_A, dev) if x.net_A is not None else None
        self.vv = Placed(x.vv, dev)                                       # v_prev = row 0, v = row 1 of a (2, dv) path
        self.pin = Placed(x.pin_val, dev, sh("pin")) if x.pin_val is not None else None
        self.us_new = Output(c.n * c.du, dev, sh("us_new")) if c.want_us else None
        self.lw = Output(c.n, dev) if c.want_lw else None
        ptr = lambda b: b.ptr if b is not None else None
        self.p = dict(us=ptr(self.us), net=self.net.ptr, v=self.vv.at(c.dv), v_prev=self.vv.ptr, pin=ptr(self.pin),
                      us_new=ptr(self.us_new), lw=ptr(self.lw))
        for name in ("us", "net", "us_new", "pin"):                       # the misalignment is the case's, not torch's
            if self.p[name] is not None:
                esz = 2 if (name == "net" and dtype == "bf16") else 4
                assert self.p[name] % 16 == esz * sh(name), (name, self.p[name] % 16)

    def inputs(self):
        return [b for b in (self.us, self.A, self.net, self.net_A, self.vv, self.pin) if b is not None]

    def args(self, mode, **over):
        c, p = self.x.case, dict(self.p)
        a = dict(n_total=c.n_total, row0=c.row0, n=c.n, pin=-1 if c.pin is None else c.pin)
        for k, v in over.items():
            (a if k in a else p)[k] = v
        return (self.mask.ref, p["us"], self.A.ptr if self.A else None, p["net"], self.net_A.ptr if self.net_A else None,
                E.DTYPES.index(self.dtype), mode, float(E.CX), float(E.CS), float(E.DT), float(E.SD), p["v"], p["v_prev"],
                int(self.x.key[0]), int(self.x.key[1]), a["n_total"], a["row0"], a["n"], a["pin"], p["pin"], p["us_new"],
                p["lw"], 0)

    def check_inputs(self, what):
        assert self.mask.unchanged(), what + ": a mask table changed"
        assert all(b.unchanged() for b in self.inputs()), what + ": an input changed"


def _run_finish(case, dtype, mode, dev):
    from fbs_amd import _lib
    x = E.finish_inputs(case.id, dtype, mode)
    call = FinishCall(x, dtype, dev)
    what = f"{case.id} {dtype} mode {mode}"
    rc, plan = E.plan_finish(call.mask.ref, case, dtype, mode, call.p)
    assert rc == 0, _lib.lib().fbsmi_last_error()
    E.check_plan(plan, case.plan, what)
    _lib.call("fbsmi_em_finish", *call.args(mode))
    torch.cuda.synchronize()
    if case.want_us:
        call.us_new.check(_u32(x.want_us), what + ": us_new")
    if case.want_lw:
        call.lw.check(_u32(x.want_lw), what + ": lw")
    call.check_inputs(what)
    return call


def _params(cases):
    combos, ids = E.expand(cases)
    return pytest.mark.parametrize("case,dtype,mode", combos, ids=ids)


# ---- a. k_em_rows ------------------------------------------------------------------------------------------------------------
@_params(E.ROWS_CASES)
def test_rows_kernel_and_its_fallbacks(case, dtype, mode, oracle, dev):
    """A rank's row slice with proposal and weights, ancestors, net_A and a pin row inside: the one-pass rows kernel at
    every KU, every shape of the last LDS-DMA chunk, the LDS budget, the LDS tree past 64 segments, masks whose runs miss
    the wide LDS read, a slice past element 2^31 of the draw, the division branches -- and, for each condition of the
    dispatch, the nearest shape that must take the two-role kernel, with the same expected bits.
    rows-lds-13248 / -13252: the 52 KiB budget counts the row rounded up to 1 KiB PLUS the 256 bytes of segment sums, so
    the rows kernel ends at D = 13056 floats (rows-lds-fits / -over); D = 13248 is already the two-role kernel's."""
    _run_finish(case, dtype, mode, dev)


# ---- b. the role map ------------------------------------------------------------------------------------------------------------
@_params(E.ROLE_CASES)
def test_two_role_kernel_interleaved_and_rows_first(case, dtype, mode, oracle, dev):
    """Whole draws with nU + nV on both sides of 8192: interleaved roles (1:~480 and 1:2), rows first, one role absent."""
    _run_finish(case, dtype, mode, dev)


# ---- c. log-density geometry ------------------------------------------------------------------------------------------------------
@_params(E.WEIGHT_CASES)
def test_weights_at_every_part_length(case, dtype, mode, oracle, dev):
    """dv from 1 (element-wise path) over the 4 <= d < 8 clamp, ragged tails across a segment and across the four waves'
    stride, every turn of the software pipeline, to 65 segments (the LDS tree with an odd carry); v and v_prev are rows of
    a (2, dv) array (dword aligned for odd dv); dv = 0 gives +0.0."""
    call = _run_finish(case, dtype, mode, dev)
    if case.dv == 0:
        assert (call.lw.bits()[GUARD:GUARD + case.n] == 0).all()


@_params(E.TRANS_CASES)
def test_transition_logpdf_at_every_part_length(case, dtype, mode, oracle, dev):
    from fbs_amd import _lib
    x = E.trans_inputs(case.id, dtype, mode)
    what = f"{case.id} {dtype} mode {mode}"
    mask = E.DeviceMask(x.tables, dev)
    us, net, uu, lw = Placed(x.us, dev), Placed(x.net_dev, dev), Placed(x.uu, dev), Output(case.n, dev)
    rc, plan = E.plan_trans(mask.ref, case, dtype, mode, us.ptr, net.ptr, uu.at(case.du), lw.ptr)
    assert rc == 0, _lib.lib().fbsmi_last_error()
    E.check_plan(plan, case.plan, what)
    _lib.call("fbsmi_em_transition_logpdf", mask.ref, us.ptr, net.ptr, E.DTYPES.index(dtype), mode, float(E.CX), float(E.CS),
              float(E.DT), float(E.SD), uu.at(case.du), case.n, lw.ptr, 0)
    torch.cuda.synchronize()
    lw.check(_u32(x.want), what)
    assert mask.unchanged() and us.unchanged() and net.unchanged() and uu.unchanged(), what + ": an input changed"


# ---- e. proposal fallbacks, the pin, the masks on the two-role kernel ---------------------------------------------------------------
@_params(E.PROPOSAL_CASES)
def test_proposal_fallbacks_and_pin(case, dtype, mode, oracle, dev):
    """The element-wise proposal walk (half % 4 != 0, misaligned us / us_new, odd du, an odd flat total with its zero-padded
    last counter, as whole draw and as slice), n = 1, a pin in the upper half and from a dword-aligned value, a pin without
    a proposal; every mask recipe and the D - 4 clamp of the 16-byte network load on the two-role kernel."""
    _run_finish(case, dtype, mode, dev)


# ---- f. the 2^32 boundary ---------------------------------------------------------------------------------------------------------
@_params(E.BOUNDARY_CASES)
def test_last_rows_of_the_largest_draw(case, dtype, mode, oracle, dev):
    """n_total * du = 2^32 - 4 with du = 3: the element-wise walk of the last three rows tests flat indices up to 2^32 - 2
    against the draw's end without wrapping; one row more is refused before anything is launched."""
    from fbs_amd import _lib
    call = _run_finish(case, dtype, mode, dev)
    L = _lib.lib()
    fresh = FinishCall(call.x, dtype, dev)
    rc = L.fbsmi_em_finish(*fresh.args(mode, n_total=E.FIRST_REFUSED_TOTAL, row0=E.FIRST_REFUSED_TOTAL - 3))
    assert rc == -1 and b"2^32 - 4" in L.fbsmi_last_error()
    torch.cuda.synchronize()
    fresh.us_new.untouched("refused draw: us_new")
    fresh.lw.untouched("refused draw: lw")


# ---- g. k_em_concat -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.CONCAT_CASES, ids=[c.id for c in E.CONCAT_CASES])
def test_concat_variants_masks_and_rounding(case, oracle, dev):
    """One chunk, the chunk edge, a ragged second and third chunk; parts below 4 elements, a misaligned img or role table
    (the element-wise variant); every mask recipe, runs that end inside a lane's group at du - 1 / dv - 1 (the uo and vq
    clamps); bfloat16 ties, NaN payloads, infinities and denormals."""
    from fbs_amd import _lib
    from oracle import em
    x = E.concat_inputs(case.id)
    mask = E.DeviceMask(x.tables, dev, {"role": case.shift.get("role", 0)})
    us, vp, A = Placed(x.us, dev), Placed(x.vp, dev), Placed(x.A, dev)
    D = case.du + case.dv
    for out_dtype in E.DTYPES:
        for with_A in (False, True):
            what = f"{case.id} {out_dtype} {'A' if with_A else 'identity'}"
            img = Output(case.n * D, dev, case.shift.get("img", 0), bf16=out_dtype == "bf16")
            rc, plan = E.plan_concat(mask.ref, us.ptr, vp.ptr, case.n, out_dtype, img.ptr)
            assert rc == 0, _lib.lib().fbsmi_last_error()
            E.check_plan(plan, case.plan, what)
            _lib.call("fbsmi_em_concat", mask.ref, us.ptr, A.ptr if with_A else None, vp.ptr, case.n, E.DTYPES.index(out_dtype),
                      img.ptr, 0)
            torch.cuda.synchronize()
            want = x.want[with_A][:case.n]
            img.check(em.to_bf16_bits(want) if out_dtype == "bf16" else _u32(want), what)
    assert mask.unchanged() and us.unchanged() and vp.unchanged() and A.unchanged(), case.id + ": an input changed"


# ---- h. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,spoil,word", E.REFUSALS, ids=[r[0] for r in E.REFUSALS])
def test_finish_refusals_launch_nothing(rid, spoil, word, oracle, dev):
    """Real, correctly sized buffers: a check that failed to fire would launch a valid call, and the sentinels would show it."""
    from fbs_amd import _lib
    L = _lib.lib()
    x = E.finish_inputs(E.REFUSAL_CASE.id, "f32", 0)
    call = FinishCall(x, "f32", dev, spoil.get("mask_shift"))
    over = {}
    if "du" in spoil:                                                    # a 3-float image over the same buffers
        call.mask = E.DeviceMask(E.mask_tables(spoil["du"], spoil["dv"], "u_first"), dev)
    if spoil.get("alias"):
        over["us_new"] = call.p["us"]
    if "pin" in spoil:
        over["pin"] = spoil["pin"]
    if spoil.get("no_pin_value"):
        call.p["pin"] = None
    if "n_total" in spoil:
        over["n_total"] = spoil["n_total"]
    if spoil.get("no_v"):
        call.p["v"] = None
    rc = L.fbsmi_em_finish(*call.args(0, **over))
    msg = L.fbsmi_last_error()
    assert rc == -1, (rid, rc)
    assert word.encode() in msg, (rid, msg)
    torch.cuda.synchronize()
    call.us_new.untouched(rid + ": us_new")
    call.lw.untouched(rid + ": lw")
    call.check_inputs(rid)


def test_calls_of_nothing_return_ok_and_touch_nothing(oracle, dev):
    from fbs_amd import _lib
    x = E.finish_inputs(E.REFUSAL_CASE.id, "f32", 0)
    call = FinishCall(x, "f32", dev)
    _lib.call("fbsmi_em_finish", *call.args(0, n=0, n_total=0, pin=-1))
    _lib.call("fbsmi_em_finish", *call.args(0, n=0, pin=-1))
    _lib.call("fbsmi_em_finish", *call.args(0, us_new=None, lw=None))               # nothing asked for
    img = Output(6 * 16, dev)
    _lib.call("fbsmi_em_concat", call.mask.ref, call.us.ptr, None, call.vv.ptr, 0, 0, img.ptr, 0)
    _lib.call("fbsmi_em_transition_logpdf", call.mask.ref, call.us.ptr, call.net.ptr, 0, 0, float(E.CX), float(E.CS), float(E.DT),
              float(E.SD), call.pin.ptr, 0, call.lw.ptr, 0)
    torch.cuda.synchronize()
    call.us_new.untouched("n = 0: us_new")
    call.lw.untouched("n = 0: lw")
    img.untouched("n = 0: img")
    call.check_inputs("n = 0")
