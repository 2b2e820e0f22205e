"""GPU: the trainer's kernels (fbs_amd/csrc/fbsmi_train.hip) on the branches a training run takes -- the 16-byte path with
several chunks per row and with a row's workgroups looping, more than 256 rows, bases off 16-byte alignment, Adam past
one sweep of its grid, and the bfloat16 store and the clip at non-finite values.  tests/train_edges.py lists every shape
with the branch it is there for and tests/test_train_edges_host.py holds that table to the dispatch.

The assertions are those of tests/test_gpu_train_kernels.py: outputs bit for bit equal to the float32 restatements of
tests/train_restate.py (through bf16_round_full for bfloat16 outputs), the loss and the Adam step within 1e-5 relative of
the float64 restatements of the reference's formulas.  Every buffer a kernel writes lies between guards of 64 sentinel
elements, which must be unchanged afterwards: that is how a vector store beyond a row block would show."""
import functools

import numpy as np
import pytest
import torch

import train_edges as E
import train_restate as R
from helpers import bits

pytestmark = pytest.mark.gpu

REL = 1e-5
GUARD = 64
S32, S16 = 0x7fc5a5a5, 0x7fc5            # the guards' bit patterns (NaNs no kernel here produces)
f32 = np.float32


def _t(a, dev):
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)


class Buf:
    """n float32 (or bfloat16) elements on the device between two guards, the first element `off` bytes past a 16-byte
    boundary.  Filled from `init` bit for bit; otherwise the body holds the sentinel too, so that an element the kernel
    leaves out shows in the comparison."""

    def __init__(self, dev, n, bf16=False, off=0, init=None):
        item = 2 if bf16 else 4
        assert off % item == 0 and 0 <= off < 16
        self.bf16, self.n, self.first = bf16, int(n), GUARD + off // item
        self.sentinel = S16 if bf16 else S32
        self.raw = torch.full((self.first + self.n + GUARD,), self.sentinel, dtype=torch.int16 if bf16 else torch.int32,
                              device=dev)
        self.t = self.raw.view(torch.bfloat16 if bf16 else torch.float32)[self.first:self.first + self.n]
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == off
        if init is not None:
            u = np.ascontiguousarray(init, f32).reshape(-1).view(np.uint32)
            assert u.size == self.n
            if bf16:
                assert not (u & 0xffff).any()
                u = (u >> 16).astype(np.uint16).view(np.int16)
            else:
                u = u.view(np.int32)
            self.raw[self.first:self.first + self.n].copy_(torch.from_numpy(u.copy()))

    def values(self, what="buffer"):
        """the body as float32 values, after checking both guards"""
        h = self.raw.cpu().numpy()
        for name, part in (("in front of", h[:self.first]), ("behind", h[self.first + self.n:])):
            bad = np.flatnonzero(part != self.sentinel)
            assert bad.size == 0, f"{what}: {bad.size} guard elements {name} the block overwritten, first at {bad[:4]}"
        body = h[self.first:self.first + self.n]
        if self.bf16:
            return (body.view(np.uint16).astype(np.uint32) << 16).view(f32)
        return body.view(f32).copy()


def _opt(a, dev):
    return None if a is None else _t(a, dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


def loss_call(dev, net, dt16, mode, sq, gc, keys=None, xt=None, data=None, idx=None, F=None, rows=True, off=None):
    """fbsmi_dsm_loss_batched on guarded buffers -> (loss (1,), dnet (B, D) float32 values, row_sums (B,) or None)."""
    from fbs_amd import _lib, ops
    off = off or {}
    B, D = net.shape
    nb = Buf(dev, B * D, dt16, off.get("net", 0), net)
    db = Buf(dev, B * D, dt16, off.get("dnet", 0))
    xb = None if xt is None else Buf(dev, xt.size, False, off.get("xt", 0), xt)
    ab = None if data is None else Buf(dev, data.size, False, off.get("data", 0), data)
    nws = int(_lib.lib().fbsmi_dsm_loss_workspace_bytes(B, D))
    assert nws == 4 * B * E.loss_dispatch(B, D)[1]
    ws, rs, ls = Buf(dev, nws // 4), (Buf(dev, B) if rows else None), Buf(dev, 1)
    small = [_opt(a, dev) for a in (keys, idx, F, sq, gc)]
    _lib.call("fbsmi_dsm_loss_batched", nb.ptr, int(dt16), int(mode), _ptr(small[0]), xb and xb.ptr, ab and ab.ptr,
              _ptr(small[1]), _ptr(small[2]), _ptr(small[3]), _ptr(small[4]), float(f32(1.0 / (float(B) * float(D)))), B, D,
              db.ptr, rs and rs.ptr, ls.ptr, ws.ptr, ops._stream())
    torch.cuda.synchronize()
    for name, b in (("net", nb), ("xt", xb), ("data", ab), ("workspace", ws)):
        if b is not None:
            b.values(name)
    return ls.values("loss"), db.values("dnet").reshape(B, D), (rs.values("row_sums") if rows else None)


def noise_call(dev, data, idx, keys, F, sq, bf16, off=None):
    """fbsmi_dsm_noise_batched on guarded buffers -> xt (B, D) float32 values."""
    from fbs_amd import _lib, ops
    off = off or {}
    B, D = len(keys), data.shape[1]
    ab = Buf(dev, data.size, False, off.get("data", 0), data)
    xb = Buf(dev, B * D, bf16, off.get("xt", 0))
    small = [_opt(a, dev) for a in (idx, keys, F, sq)]
    _lib.call("fbsmi_dsm_noise_batched", ab.ptr, _ptr(small[0]), _ptr(small[1]), _ptr(small[2]), _ptr(small[3]), B, D,
              int(bf16), xb.ptr, ops._stream())
    torch.cuda.synchronize()
    ab.values("data")
    return xb.values("xt").reshape(B, D)


def _loss_inputs(c, mode, dt16, with_idx, rows=slice(None)):
    """the arguments of loss_call for rows `rows` of a case"""
    sel = lambda a: np.ascontiguousarray(a[rows])
    kw = dict(net=sel(c["net16"] if dt16 else c["net"]), dt16=dt16, mode=mode, sq=sel(c["sq"]), gc=sel(c["gc"]))
    if mode == 0:
        kw.update(keys=sel(c["keys"]))
        if with_idx:                                   # mode 0 reads neither: the pointer must not matter
            kw.update(idx=sel(c["idx"]))
    else:
        kw.update(xt=sel(c["xt_idx"] if with_idx else c["xt"]), data=c["data"], F=sel(c["F"]),
                  idx=sel(c["idx"]) if with_idx else None)
    return kw


@functools.lru_cache(maxsize=None)
def loss_want(D, B, mode, dt16, with_idx):
    """(S, loss, dnet) of the float32 restatement and the float64 loss of the reference's formula, once per case."""
    c = R.case(D, B)
    net = c["net16"] if dt16 else c["net"]
    F, sq = c["F"], c["sq"]
    if mode == 0:                                      # on the exact x_t = F x0 + sq xi
        e, x0 = c["xi"], c["x0_idx"]
        xt = F[:, None].astype(np.float64) * x0 + sq[:, None].astype(np.float64) * e
    else:                                              # on the stored float32 x_t
        xt = c["xt_idx"] if with_idx else c["xt"]
        x0 = c["x0_idx"] if with_idx else c["data"][:B]
        e = R.stored_noise_f32(xt, c["data"], c["idx"] if with_idx else None, F, sq)
    S, loss, dnet = R.loss_f32(net, e, sq, c["gc"], c["inv"])
    if dt16:
        dnet = R.bf16_round_full(dnet)
    return S, np.array([loss], f32), dnet, R.loss_f64(net, xt, x0, F, sq)


def _check_loss(got, want, what):
    (loss, dnet, S), (wS, wloss, wd, ref) = got, want
    if S is not None:
        assert np.array_equal(bits(S), bits(wS)), what
    assert np.array_equal(bits(loss), bits(wloss)), what
    assert np.array_equal(bits(dnet), bits(wd)), what
    rel = abs(float(loss[0]) - ref) / ref
    print(f"{what}: loss {float(loss[0]):.9g} float64 {ref:.9g} rel {rel:.2e}")
    assert rel < REL, (what, rel)


# ------------------------------------------------------------------------------------------------
# row lengths
# ------------------------------------------------------------------------------------------------
def _bs_of(D):
    return (2,) if D in E.BIG_DS else E.EDGE_BS


@pytest.mark.parametrize("D", list(E.ROW_LENGTHS))
def test_noise_at_the_row_length_edges(dev, D):
    for B in _bs_of(D):
        c = R.case(D, B)
        for tag, idx in (("xt", None), ("xt_idx", c["idx"])):
            for bf16 in (False, True):
                got = noise_call(dev, c["data"], idx, c["keys"], c["F"], c["sq"], bf16)
                want = R.bf16_round_full(c[tag]) if bf16 else c[tag]
                assert np.array_equal(bits(got), bits(want)), (B, tag, bf16)


@pytest.mark.parametrize("dt16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1], ids=["drawn", "stored"])
@pytest.mark.parametrize("D", list(E.ROW_LENGTHS))
def test_loss_at_the_row_length_edges(dev, D, mode, dt16):
    for B in _bs_of(D):
        c = R.case(D, B)
        for with_idx in (False, True):
            got = loss_call(dev, **_loss_inputs(c, mode, dt16, with_idx))
            _check_loss(got, loss_want(D, B, mode, dt16, with_idx), f"D={D} B={B} mode={mode} bf16={dt16} idx={with_idx}")


# ------------------------------------------------------------------------------------------------
# more than 256 rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["drawn", "stored"])
@pytest.mark.parametrize("B,D", list(E.ROW_COUNTS))
def test_loss_over_many_rows(dev, B, D, mode):
    """R = 1, 2 and 4 rows per thread of the finishing launch, one and several chunk roots per row: row sums and loss bit
    for bit, the loss the same without row_sums, and a row the same as when it is scored alone."""
    c = R.case(D, B)
    kw = _loss_inputs(c, mode, False, True)
    loss, dnet, S = loss_call(dev, **kw)
    _check_loss((loss, dnet, S), loss_want(D, B, mode, False, True), f"B={B} D={D} mode={mode}")
    loss_n, dnet_n, _ = loss_call(dev, rows=False, **kw)
    assert np.array_equal(bits(loss_n), bits(loss)) and np.array_equal(bits(dnet_n), bits(dnet))
    for b in sorted({0, 255, 256, B - 1}):
        if b < B:
            _, d1, S1 = loss_call(dev, **_loss_inputs(c, mode, False, True, rows=slice(b, b + 1)))
            assert np.array_equal(bits(S1), bits(S[b:b + 1])), b
            assert np.array_equal(bits(d1), bits(dnet[b:b + 1])), b


# ------------------------------------------------------------------------------------------------
# bases off 16-byte alignment
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1], ids=["drawn", "stored"])
@pytest.mark.parametrize("D", E.ALIGN_DS)
def test_loss_off_alignment_has_the_aligned_bits(dev, D, mode, dt16):
    B = E.ALIGN_B
    c = R.case(D, B)
    kw = _loss_inputs(c, mode, dt16, True)
    base = loss_call(dev, **kw)
    _check_loss(base, loss_want(D, B, mode, dt16, True), f"D={D} mode={mode} bf16={dt16} aligned")
    moves = [(name, o) for name in ("net", "dnet") for o in ((2,) if dt16 else (4, 8))]
    if mode == 1:
        moves += [(name, o) for name in ("xt", "data") for o in (4, 8)]
    for name, o in moves:
        got = loss_call(dev, off={name: o}, **kw)
        for g, w in zip(got, base):
            assert np.array_equal(bits(g), bits(w)), (name, o)


@pytest.mark.parametrize("D", E.ALIGN_DS)
def test_noise_off_alignment_has_the_aligned_bits(dev, D):
    c = R.case(D, E.ALIGN_B)
    for bf16 in (False, True):
        want = R.bf16_round_full(c["xt_idx"]) if bf16 else c["xt_idx"]
        args = (c["data"], c["idx"], c["keys"], c["F"], c["sq"], bf16)
        assert np.array_equal(bits(noise_call(dev, *args)), bits(want)), bf16
        for name, o in [("data", 4), ("data", 8)] + [("xt", o) for o in ((2,) if bf16 else (4, 8))]:
            assert np.array_equal(bits(noise_call(dev, *args, off={name: o})), bits(want)), (bf16, name, o)


# ------------------------------------------------------------------------------------------------
# special values
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 63], ids=["vec", "scalar"])
def test_bf16_store_of_the_loss_on_the_special_values(dev, D):
    """sq = gc = 1, net = 0, F = 0, data = 0 in mode 1: r is x_t, and dnet its bfloat16 rounding."""
    B = 2
    assert E.loss_dispatch(B, D)[0] == (D == 64)
    xt = E.special_f32(B * D).reshape(B, D)
    zeros, ones = np.zeros((B, D), f32), np.ones(B, f32)
    with np.errstate(all="ignore"):
        e = R.stored_noise_f32(xt, zeros, None, np.zeros(B, f32), ones)
        _, _, wd = R.loss_f32(zeros, e, ones, ones, f32(1.0 / (B * D)))
    vals = np.isfinite(xt)
    assert np.array_equal(bits(wd[vals & (xt != 0)]), bits(xt[vals & (xt != 0)]))          # r is the value itself
    want = R.bf16_round_full(wd)
    _, dnet, _ = loss_call(dev, zeros, True, 1, ones, ones, xt=xt, data=zeros, F=np.zeros(B, f32))
    assert np.isnan(want).sum() >= 6 and np.isinf(want).sum() >= 4
    assert E.same_or_both_nan(dnet, want)
    assert not E.same_or_both_nan(E.bf16_ties_away(wd), want) and not E.same_or_both_nan(E.bf16_truncate(wd), want)


@pytest.mark.parametrize("D", [64, 63], ids=["vec", "scalar"])
def test_bf16_store_of_the_noise_on_the_special_values(dev, oracle, D):
    """F = 1, sq = 0: x_t is the data value (the drawn normal is finite), stored as float32 and as bfloat16."""
    B = 2
    assert E.noise_dispatch(D)[0] == (D == 64)
    data = E.special_f32(B * D).reshape(B, D)
    keys = oracle.split(oracle.PRNGKey(5), B)
    F, sq = np.ones(B, f32), np.zeros(B, f32)
    with np.errstate(all="ignore"):
        want, xi = R.noise_f32(data, None, keys, F, sq)
    assert np.isfinite(xi).all()
    assert E.same_or_both_nan(noise_call(dev, data, None, keys, F, sq, False), want)
    assert E.same_or_both_nan(noise_call(dev, data, None, keys, F, sq, True), R.bf16_round_full(want))


@pytest.mark.parametrize("dt16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1], ids=["drawn", "stored"])
@pytest.mark.parametrize("D", [784, 2049, 3072])
def test_a_non_finite_row_stays_in_its_row(dev, D, mode, dt16):
    """One inf, then one NaN, in row 2 of net: that row's sum and the loss are not finite; the other rows' S_b and dnet
    have the bits of the clean batch."""
    c = R.case(D, 5)
    kw = _loss_inputs(c, mode, dt16, True)
    loss0, dnet0, S0 = loss_call(dev, **kw)
    assert np.isfinite(loss0).all() and np.isfinite(S0).all()
    others = [0, 1, 3, 4]
    at = D // 3
    for bad in (np.inf, -np.inf, np.nan):
        net = kw["net"].copy()
        net[2, at] = bad
        loss, dnet, S = loss_call(dev, **dict(kw, net=net))
        assert not np.isfinite(S[2]) and not np.isfinite(loss[0]), bad
        assert np.array_equal(bits(S[others]), bits(S0[others])), bad
        assert np.array_equal(bits(dnet[others]), bits(dnet0[others])), bad
        keep = np.arange(D) != at
        assert np.array_equal(bits(dnet[2, keep]), bits(dnet0[2, keep])) and not np.isfinite(dnet[2, at]), bad


@pytest.mark.parametrize("unit_sq", [False, True], ids=["sq_t0.02", "sq_1"])
@pytest.mark.parametrize("D", [72, 70], ids=["vec", "scalar"])
def test_stored_quotient_on_both_sides_of_the_short_division(dev, D, unit_sq):
    """e = (x_t - F x0) / sq must be the correctly rounded quotient inside and outside the range of the short division
    (|x_t - F x0| in [2^-60, 2^60]): zero, subnormal, 2^-61, 2^-60, 2^60, 2^61.  Read through dnet with gc = 1, net = 0."""
    xt = E.quotient_rows(D)
    B = xt.shape[0]
    sq = np.full(B, 1.0 if unit_sq else E.sq_at(0.02), f32)
    zeros, ones, F = np.zeros((B, D), f32), np.ones(B, f32), np.full(B, 0.5, f32)
    with np.errstate(all="ignore"):
        e = R.stored_noise_f32(xt, zeros, None, F, sq)
        assert np.array_equal(e.astype(np.float64), (xt.astype(np.float64) / np.float64(sq[0])).astype(f32).astype(np.float64))
        wS, wloss, wd = R.loss_f32(zeros, e, sq, ones, f32(1.0 / (B * D)))
    assert np.array_equal(bits(wd[1:]), bits(e[1:])) and np.isfinite(wd).all()
    loss, dnet, S = loss_call(dev, zeros, False, 1, sq, ones, xt=xt, data=zeros, F=F)
    for b in range(B):
        bad = np.flatnonzero(bits(dnet[b]) != bits(wd[b]))
        assert bad.size == 0, (b, bad[:4], dnet[b, bad[:4]], wd[b, bad[:4]])
    assert E.same_or_both_nan(S, wS) and E.same_or_both_nan(loss, np.array([wloss], f32))


# ------------------------------------------------------------------------------------------------
# clip + Adam + EMA
# ------------------------------------------------------------------------------------------------
LR, B1, B2, EPS, DECAY = 4.0, 0.9, 0.999, 1e-8, 0.99
NAMES = ("p", "g", "m", "v", "ema")


def _rel(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want)))


def _adam_state(n, seed):
    """p, m, v, ema of order one and kept away from zero, as test_adam_ema_step_follows_optax builds them"""
    rng = np.random.default_rng(seed)
    away = lambda a: (np.sign(a) * (0.5 + np.abs(a))).astype(f32)
    p, ema = (away(rng.normal(size=n)) for _ in range(2))
    m = (np.sign(rng.normal(size=n)) * (2.0 + rng.uniform(size=n))).astype(f32)
    v = (0.5 + rng.uniform(size=n)).astype(f32)
    return rng, dict(p=p, m=m, v=v, ema=ema)


def _adam_bufs(dev, state, g, off):
    arrays = dict(state, g=g)
    return {k: Buf(dev, arrays[k].size, False, off.get(k, 0), arrays[k]) for k in NAMES}


def _step(bufs, count, gn2, max_norm, mode):
    from fbs_amd.train import adam_ema_step
    adam_ema_step(bufs["p"].t, bufs["g"].t, bufs["m"].t, bufs["v"].t, bufs["ema"].t, LR, B1, B2, EPS, count, gn2, max_norm,
                  mode, DECAY)
    torch.cuda.synchronize()
    return {k: bufs[k].values(k) for k in NAMES}


def _adam_run(dev, n, clip, modes, off, seed):
    """Consecutive steps from the GPU's own previous state, each against the float64 restatement; the worst relative
    differences of (update, m, v, ema)."""
    from fbs_amd.train import sqnorm
    assert E.adam_dispatch(n, not off)[0] == (not off)
    rng, state = _adam_state(n, seed)
    worst = np.zeros(4)
    f = lambda x: float(f32(x))
    for count, mode in enumerate(modes):
        g = rng.normal(size=n).astype(f32)
        gnorm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        max_norm = {"off": None, "active": 0.5 * gnorm, "inactive": 2.0 * gnorm}[clip]
        bufs = _adam_bufs(dev, state, g, off)
        gn2 = None if max_norm is None else sqnorm(bufs["g"].t)
        new = _step(bufs, count, gn2, 1.0 if max_norm is None else max_norm, mode)
        assert np.array_equal(bits(new["g"]), bits(g))
        g64 = g.astype(np.float64) if max_norm is None else R.clip_by_global_norm_f64(g, f(max_norm))
        if clip == "active":
            assert np.linalg.norm(g64) < 0.51 * gnorm
        if clip == "inactive":
            assert np.array_equal(g64, g.astype(np.float64))
        wp, wm, wv = R.adam_f64(state["p"], g64, state["m"], state["v"], f(LR), f(B1), f(B2), f(EPS), count)
        we = R.ema_f64(state["ema"], wp, mode, f(DECAY))
        rels = [_rel(new["p"].astype(np.float64) - state["p"], wp - state["p"]), _rel(new["m"], wm), _rel(new["v"], wv), 0.0]
        if mode == 0:
            assert np.array_equal(bits(new["ema"]), bits(state["ema"])), count
        elif mode == 1:
            assert np.array_equal(bits(new["ema"]), bits(new["p"])), count
        else:
            rels[3] = _rel(new["ema"], we)
        assert max(rels) < REL, (count, mode, rels)
        worst = np.maximum(worst, rels)
        state = {k: new[k] for k in ("p", "m", "v", "ema")}
    return worst


@pytest.mark.parametrize("clip", ["off", "active", "inactive"])
@pytest.mark.parametrize("n,off_p", [(n, 0 if aligned else 4) for (n, aligned) in E.ADAM_LONG if n > 1025])
def test_adam_past_one_sweep_of_the_grid(dev, n, off_p, clip):
    """A full 16-byte sweep of the 4096 workgroups, a second partial sweep with a one-element tail, and the scalar path
    looping: one step per ema mode, every element against float64."""
    worst = _adam_run(dev, n, clip, [2, 0, 1], {"p": off_p} if off_p else {}, seed=n % 1000 + len(clip))
    print(f"adam n={n} p+{off_p} clip={clip}: worst relative difference update {worst[0]:.2e} m {worst[1]:.2e} "
          f"v {worst[2]:.2e} ema {worst[3]:.2e}")


@pytest.mark.parametrize("clip", ["off", "active", "inactive"])
@pytest.mark.parametrize("which", ["g", "m", "v", "ema"])
def test_adam_with_one_vector_off_alignment(dev, which, clip):
    """n = 1025 with one of g, m, v, ema alone 4 bytes off: the scalar path (for ema: only when the EMA is touched)."""
    _adam_run(dev, 1025, clip, [2, 0, 2, 0, 1], {which: 4}, seed=17 + len(clip))


@pytest.mark.parametrize("off_p", [0, 4], ids=["vec", "scalar"])
def test_adam_exact_cases(dev, off_p):
    n = 1029
    off = {"p": off_p} if off_p else {}
    assert E.adam_dispatch(n, not off_p) == ((True, 2, 1, 1) if not off_p else (False, 5, 1, 0))
    rng, state = _adam_state(n, 99)
    g = rng.normal(size=n).astype(f32)
    zero = np.zeros(n, f32)
    scalar = lambda x: torch.tensor([x], dtype=torch.float32, device=dev)
    f = lambda x: float(f32(x))

    # g = m = v = 0: the zero padding between a module's parameters stays what it is
    for gn2 in (None, scalar(0.0)):
        st = dict(p=state["p"], m=zero, v=zero, ema=state["p"])
        new = _step(_adam_bufs(dev, st, zero, off), 3, gn2, 1.0, 2)
        assert np.array_equal(bits(new["p"]), bits(state["p"]))
        assert np.array_equal(bits(new["m"]), bits(zero)) and np.array_equal(bits(new["v"]), bits(zero))
        assert _rel(new["ema"], state["p"].astype(np.float64)) < REL

    # gnorm2 = 0: s = 1, the bits of the call without a clip
    plain = _step(_adam_bufs(dev, state, g, off), 3, None, 1.0, 2)
    at0 = _step(_adam_bufs(dev, state, g, off), 3, scalar(0.0), 0.25, 2)
    for k in NAMES:
        assert np.array_equal(bits(at0[k]), bits(plain[k])), k

    # gnorm2 = inf with a finite g: g' = 0, the moments decay and everything stays finite
    new = _step(_adam_bufs(dev, state, g, off), 3, scalar(np.inf), 0.25, 2)
    g64 = R.clip_by_global_norm_f64(g, 0.25, gnorm2=np.inf)
    assert not g64.any()
    wp, wm, wv = R.adam_f64(state["p"], g64, state["m"], state["v"], f(LR), f(B1), f(B2), f(EPS), 3)
    assert all(np.isfinite(new[k]).all() for k in NAMES)
    assert _rel(new["p"].astype(np.float64) - state["p"], wp - state["p"]) < REL
    assert _rel(new["m"], wm) < REL and _rel(new["v"], wv) < REL
    assert _rel(new["ema"], R.ema_f64(state["ema"], wp, 2, f(DECAY))) < REL

    # gnorm2 = NaN: the comparison fails, the scaled branch is taken, every output is NaN (optax's where does the same)
    assert np.isnan(R.clip_by_global_norm_f64(g, 0.25, gnorm2=np.nan)).all()
    new = _step(_adam_bufs(dev, state, g, off), 3, scalar(np.nan), 0.25, 2)
    for k in ("p", "m", "v", "ema"):
        assert np.isnan(new[k]).all(), k
    assert np.array_equal(bits(new["g"]), bits(g))
