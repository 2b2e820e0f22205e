"""GPU: the stand-alone path, draw, data-movement, reduction and closure kernels at their launch and address edges --
past the capped grid of every strided launch, at misaligned base pointers (the scalar branches torch's aligned
allocations never reach), in place where include/fbsmi.h allows aliasing, and at the odd / boundary slices of the
sharded draw.  Every comparison is bit for bit against the CPU oracle; outputs are pre-filled with NaN and carry guard
elements, so an unwritten coordinate or a write out of range fails."""
import functools

import numpy as np
import pytest
import torch

from helpers import toy_2d, toy_4d, oracle_model_from

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN_BITS = 0x7FC00000            # what torch.full(..., nan) stores; the sentinel of every output and guard element
GUARD = 8                        # guard floats on either side of an output (8 floats keep a 16-byte aligned start aligned)


def _np(t):
    return t.detach().cpu().numpy()


def _eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    x = a.view(np.uint32) if a.dtype == np.float32 else a
    y = b.view(np.uint32) if b.dtype == np.float32 else b
    bad = np.flatnonzero(x.ravel() != y.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first {bad[:4]}: {a.ravel()[bad[:4]]} vs {b.ravel()[bad[:4]]}"


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan(n, dev):
    return torch.full((int(n),), float("nan"), dtype=torch.float32, device=dev)


def _untouched(t, what):
    bits = _np(t).view(np.uint32)
    bad = np.flatnonzero(bits.ravel() != NAN_BITS)
    assert bad.size == 0, f"{what}: {bad.size} sentinel elements overwritten, first {bad[:4]}"


def _fptr(t, first=0):
    """Device address of float `first` of a float32 / int32 tensor."""
    return t.data_ptr() + 4 * int(first)


def _guarded(n, dev, shift=0):
    """A NaN buffer holding n output floats behind GUARD + shift guard floats, and GUARD more after them."""
    return _nan(n + 2 * GUARD + shift, dev), GUARD + shift


def _check_guarded(buf, first, n, want, what):
    got = _np(buf)
    _eq(got[first:first + n], want, what)
    _untouched(buf[:first], what + ": guard in front")
    _untouched(buf[first + n:], what + ": guard behind")


def _stream():
    from fbs_amd import ops
    return ops._stream()


# ---- a. fbsmi_linear_path across the launch bound (4096 workgroups of 64 threads) ---------------------------------------
LIN_F = np.array([0.8125, -1.0625], f32)            # distinct per step, a sign change, exact in float32
LIN_S = np.array([0.59375, 1.71875], f32)


def _linear_ref(F, S, x0, xi):
    """out[0] = x0, out[k+1] = F[k] out[k] + S[k] xi[k]: float32 numpy, each operation rounded separately."""
    x = np.ascontiguousarray(x0, f32).reshape(-1)
    out = [x]
    for k in range(F.shape[0]):
        x = (F[k] * x).astype(f32) + (S[k] * xi[k]).astype(f32)
        out.append(x)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _linear_case(D):
    import oracle as O
    x0 = O.normal(O.PRNGKey(1000 + D), (D,))
    xi = O.normal(O.PRNGKey(2000 + D), (2, D))
    return x0, xi, _linear_ref(LIN_F, LIN_S, x0, xi)


@pytest.mark.parametrize("D", [1, 63, 64, 65, 4097, 262144, 262145, 300001])
def test_linear_path_across_the_launch_bound(D, oracle, dev):
    from fbs_amd import _lib
    x0, xi, want = _linear_case(D)
    T = 2
    out, first = _guarded((T + 1) * D, dev)
    F, S, x0t, xit = _up(LIN_F, dev), _up(LIN_S, dev), _up(x0, dev), _up(xi, dev)
    _lib.call("fbsmi_linear_path", F.data_ptr(), S.data_ptr(), x0t.data_ptr(), xit.data_ptr(), T, D, _fptr(out, first),
              _stream())
    torch.cuda.synchronize()
    _check_guarded(out, first, (T + 1) * D, want.reshape(-1), f"linear path D={D}")


def test_linear_path_wrapper_flattens_a_large_2d_state(oracle, dev):
    """fbs_amd.sdes.linear._linear_path with x0 of shape (13, 23077): 300001 coordinates in one launch."""
    from fbs_amd.sdes.linear import _linear_path
    x0, xi, want = _linear_case(300001)
    got = _linear_path(LIN_F.astype(np.float64), LIN_S.astype(np.float64), _up(x0.reshape(13, 23077), dev), _up(xi, dev))
    assert tuple(got.shape) == (3, 13, 23077)
    _eq(_np(got).reshape(3, -1), want, "_linear_path (13, 23077)")


def test_linear_path_without_steps(oracle, dev):
    """T = 0: out[0] = x0 and nothing else is touched."""
    from fbs_amd import _lib
    D = 65
    x0 = oracle.normal(oracle.PRNGKey(5), (D,))
    out, first = _guarded(D, dev)
    dummy, x0t = _nan(4, dev), _up(x0, dev)
    _lib.call("fbsmi_linear_path", dummy.data_ptr(), dummy.data_ptr(), x0t.data_ptr(), dummy.data_ptr(), 0, D,
              _fptr(out, first), _stream())
    torch.cuda.synchronize()
    _check_guarded(out, first, D, x0, "linear path T=0")


# ---- b. fbsmi_affine_em_path (Doob bridge) ------------------------------------------------------------------------------
def _bridge_tables(sde, ts, nsub):
    """The float64 tables of test_doob_bridge_and_marg_y_gibbs."""
    from fbs_amd.sdes.linear import _bridge_drift_coeffs
    T = len(ts) - 1
    A, B, S, ddt = np.zeros(T * nsub), np.zeros(T * nsub), np.zeros(T * nsub), np.zeros(T)
    for k in range(T):
        h = abs(ts[k + 1] - ts[k]) / nsub
        ddt[k] = h
        for j, t_ in enumerate(np.linspace(ts[k], ts[k + 1] - h, nsub)):
            A[k * nsub + j], B[k * nsub + j] = _bridge_drift_coeffs(sde, float(t_), float(ts[-1]))
            S[k * nsub + j] = float(sde.dispersion(float(t_)))
    return A, B, S, ddt


@functools.lru_cache(maxsize=None)
def _bridge_case(T, nsub, D):
    import oracle as O
    from fbs_amd.sdes import StationaryLinLinearSDE
    ts = np.linspace(0.0, 1.0, T + 1)
    A, B, S, ddt = (np.ascontiguousarray(a, f32) for a in _bridge_tables(StationaryLinLinearSDE(0.02, 4.0, 0.0, 1.0), ts, nsub))
    key = O.PRNGKey(300 + D)
    x0 = O.normal(O.PRNGKey(400 + D), (D,))
    xT = O.normal(O.PRNGKey(500 + D), (D,))
    want = {r: O.doob_bridge_np(key, A, B, S, ddt, x0, xT, T, nsub, bool(r)) for r in (0, 1)}
    return A, B, S, ddt, key, x0, xT, want


@pytest.mark.parametrize("replace_last", [0, 1])
@pytest.mark.parametrize("T,nsub,D", [(2, 2, 1), (2, 2, 64), (2, 2, 65), (2, 2, 262145), (3, 3, 4097)])
def test_affine_em_path_across_the_launch_bound(T, nsub, D, replace_last, oracle, dev):
    """(3, 3, 4097): nsub * D is odd, the draw of an interval ends on the zero-padded counter."""
    from fbs_amd import _lib
    A, B, S, ddt, key, x0, xT, want = _bridge_case(T, nsub, D)
    keys = _up(oracle.split(key, T).view(np.int32), dev)
    out, first = _guarded((T + 1) * D, dev)
    At, Bt, St, ht, x0t, xTt = (_up(a, dev) for a in (A, B, S, ddt, x0, xT))
    _lib.call("fbsmi_affine_em_path", keys.data_ptr(), At.data_ptr(), Bt.data_ptr(), St.data_ptr(), ht.data_ptr(),
              xTt.data_ptr(), x0t.data_ptr(), T, nsub, D, replace_last, _fptr(out, first), _stream())
    torch.cuda.synchronize()
    _check_guarded(out, first, (T + 1) * D, want[replace_last].reshape(-1),
                   f"affine em path T={T} nsub={nsub} D={D} replace_last={replace_last}")


@pytest.mark.parametrize("replace_last", [0, 1])
def test_affine_em_path_without_steps(replace_last, oracle, dev):
    """T = 0 with a dummy key buffer: out[0] is x0, or the target with replace_last."""
    from fbs_amd import _lib
    D = 65
    x0 = oracle.normal(oracle.PRNGKey(6), (D,))
    xT = oracle.normal(oracle.PRNGKey(7), (D,))
    out, first = _guarded(D, dev)
    dummy, x0t, xTt = _nan(4, dev), _up(x0, dev), _up(xT, dev)
    _lib.call("fbsmi_affine_em_path", dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(),
              dummy.data_ptr(), xTt.data_ptr(), x0t.data_ptr(), 0, 2, D, replace_last, _fptr(out, first), _stream())
    torch.cuda.synchronize()
    _check_guarded(out, first, D, xT if replace_last else x0, f"affine em path T=0 replace_last={replace_last}")


def test_doob_bridge_simulator_past_the_launch_bound(oracle, dev):
    from fbs_amd.sdes import StationaryConstLinearSDE, doob_bridge_simulator
    sde = StationaryConstLinearSDE(-0.5, 1.0)
    D, T, nsub = 262145, 2, 2
    ts = np.linspace(0.0, 1.0, T + 1)
    key = oracle.PRNGKey(4)
    x0 = oracle.normal(oracle.PRNGKey(8), (D,))
    xT = oracle.normal(oracle.PRNGKey(9), (D,))
    got = doob_bridge_simulator(key, sde, _up(x0, dev), _up(xT, dev), ts, integration_nsteps=nsub, replace=True)
    A, B, S, ddt = _bridge_tables(sde, ts, nsub)
    _eq(_np(got), oracle.doob_bridge_np(key, A, B, S, ddt, x0, xT, T, nsub, True), "doob bridge D=262145")


# ---- c. fbsmi_em_update: vector branch, scalar branch (misaligned pointers, ragged tail), in place ------------------------
EM_DDT, EM_C = f32(0.01), f32(0.3)
EM_CASES = [(1027, 1027, 0), (1027, 3081, 1027), (1026, 2053, 1027), (5, 5, 0), (3, 3, 0)]


@functools.lru_cache(maxsize=None)
def _em_case(n, n_total, offset):
    import oracle as O
    key = O.PRNGKey(77)
    x = O.normal(O.PRNGKey(78), (n,))
    drift = O.normal(O.PRNGKey(79), (n,))
    xi = O.normal(key, (n_total,))[offset:offset + n]
    want = (x + (drift * EM_DDT).astype(f32)).astype(f32) + (EM_C * xi).astype(f32)
    return key, x, drift, want.astype(f32)


def _em_update(key, x_ptr, drift_ptr, n_total, offset, n, out_ptr):
    from fbs_amd import _lib
    _lib.call("fbsmi_em_update", x_ptr, drift_ptr, float(EM_DDT), float(EM_C), int(key[0]), int(key[1]), n_total, offset, n,
              out_ptr, _stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("way", ["aligned", "misaligned", "in_place"])
@pytest.mark.parametrize("n,n_total,offset", EM_CASES)
def test_em_update_branches(n, n_total, offset, way, oracle, dev):
    key, x, drift, want = _em_case(n, n_total, offset)
    shift = 1 if way == "misaligned" else 0                # one float into a larger buffer: 4 bytes past 16-byte alignment
    xb, db = _nan(n + 1, dev), _nan(n + 1, dev)
    xb[shift:shift + n] = _up(x, dev)
    db[shift:shift + n] = _up(drift, dev)
    out, first = _guarded(n, dev, shift)
    if way == "in_place":                                  # out == x (include/fbsmi.h: "out may alias x"), on a copy of x
        out[first:first + n] = _up(x, dev)
        x_ptr = _fptr(out, first)
    else:
        x_ptr = _fptr(xb, shift)
    for p in (x_ptr, _fptr(db, shift), _fptr(out, first)):
        assert p % 16 == 4 * shift
    _em_update(key, x_ptr, _fptr(db, shift), n_total, offset, n, _fptr(out, first))
    _check_guarded(out, first, n, want, f"em_update n={n} n_total={n_total} offset={offset} {way}")
    _eq(_np(xb[shift:shift + n]), x, "em_update: x changed")
    _eq(_np(db[shift:shift + n]), drift, "em_update: drift changed")


def test_em_update_of_nothing(oracle, dev):
    """n = 0 returns OK and writes nothing."""
    buf = _nan(2 * GUARD, dev)
    _em_update(oracle.PRNGKey(77), _fptr(buf, GUARD), _fptr(buf, GUARD), 0, 0, 0, _fptr(buf, GUARD))
    _untouched(buf, "em_update n=0")
    _em_update(oracle.PRNGKey(77), None, None, 0, 0, 0, None)


# ---- d. fbsmi_random_range against the oracle ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _draw(mode, n_total):
    """The full draw of n_total elements as uint32 bit patterns: mode 0 bits, 1 uniform, 2 normal."""
    import oracle as O
    key = O.PRNGKey(4242 + n_total)
    full = (lambda: O.random_bits(key, n_total), lambda: O.uniform(key, (n_total,)), lambda: O.normal(key, (n_total,)))[mode]()
    return key, np.ascontiguousarray(full).view(np.uint32)


RANGES = [(1001, s, c) for s, c in ((0, 1001), (0, 501), (501, 500), (500, 2), (1000, 1), (499, 3), (17, 0))] + \
         [(1000, 500, 500), (1000, 499, 2), (1200001, 3, 1100000)]


@pytest.mark.parametrize("n_total,start,count", RANGES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_random_range_equals_the_slice_of_the_oracle_draw(mode, n_total, start, count, oracle, dev):
    """n_total = 1001: half = 501, the last counter of the draw is zero-padded; slices that start at, end at and straddle
    `half`, the last element, an empty slice; one slice past a grid pass of 2048 x 256 threads."""
    from fbs_amd import _lib
    key, full = _draw(mode, n_total)
    buf = torch.full((count + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=dev)
    _lib.call("fbsmi_random_range", mode, int(key[0]), int(key[1]), n_total, start, count, _fptr(buf, GUARD), _stream())
    torch.cuda.synchronize()
    got = _np(buf).view(np.uint32)
    what = f"random_range mode={mode} n_total={n_total} [{start}, {start + count})"
    _eq(got[GUARD:GUARD + count], full[start:start + count], what)
    assert (got[:GUARD] == NAN_BITS).all() and (got[GUARD + count:] == NAN_BITS).all(), what + ": guard overwritten"


def test_random_range_argument_errors(oracle, dev):
    from fbs_amd import _lib
    L = _lib.lib()
    buf = torch.full((64,), NAN_BITS, dtype=torch.int32, device=dev)
    for mode, n_total, start, count in ((2, 40, 30, 11), (1, 40, 41, 0), (2, 40, -1, 4), (3, 40, 0, 4), (0, 40, 0, -1)):
        assert L.fbsmi_random_range(mode, 1, 2, n_total, start, count, buf.data_ptr(), _stream()) == -1, (mode, n_total, start, count)
        assert b"random_range" in L.fbsmi_last_error()
    torch.cuda.synchronize()
    assert (_np(buf).view(np.uint32) == NAN_BITS).all(), "a refused call launched"


# ---- e. data movement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", ["src", "dst"])
@pytest.mark.parametrize("d", [4, 8, 784])
def test_gather_rows_misaligned_base(d, misaligned, oracle, dev):
    """d % 4 == 0 with a base pointer one float into its buffer: the scalar kernel, not the float4 one."""
    from fbs_amd import _lib
    rng = np.random.default_rng(d)
    rows, n = 500, 777
    src = rng.normal(size=(rows, d)).astype(f32)
    idx = rng.integers(0, rows, n).astype(np.int32)
    s_shift, d_shift = (1, 0) if misaligned == "src" else (0, 1)
    sb = _nan(rows * d + 1, dev)
    sb[s_shift:s_shift + rows * d] = _up(src.reshape(-1), dev)
    out, first = _guarded(n * d, dev, d_shift)
    assert _fptr(sb, s_shift) % 16 == 4 * s_shift and _fptr(out, first) % 16 == 4 * d_shift
    idxt = _up(idx, dev)
    _lib.call("fbsmi_gather_rows", _fptr(sb, s_shift), idxt.data_ptr(), n, d, _fptr(out, first), _stream())
    torch.cuda.synchronize()
    _check_guarded(out, first, n * d, src[idx].reshape(-1), f"gather_rows d={d}, {misaligned} misaligned")


@pytest.mark.parametrize("row", [0, 2])
def test_set_row_past_one_grid_pass(row, oracle, dev):
    """d = 600001 > 2048 x 256: the stride loop of k_set_row; the first and the last row, neighbours untouched."""
    from fbs_amd import _lib
    d, rows = 600001, 3
    v = oracle.normal(oracle.PRNGKey(12), (d,))
    out, first = _guarded(rows * d, dev)
    vt = _up(v, dev)
    _lib.call("fbsmi_set_row", _fptr(out, first), row, vt.data_ptr(), d, _stream())
    torch.cuda.synchronize()
    _eq(_np(out[first + row * d:first + (row + 1) * d]), v, f"set_row row {row}")
    _untouched(out[:first + row * d], f"set_row row {row}: everything in front")
    _untouched(out[first + (row + 1) * d:], f"set_row row {row}: everything behind")


# ---- f. reductions in place (include/fbsmi.h: "out may alias x", "out may alias lw") --------------------------------------
LADDER = [1, 257, 65537, 300000, 3000001]              # every ITEMS dispatch, one tile to the separate top-level scan


@functools.lru_cache(maxsize=None)
def _reduction_inputs(n):
    """The inputs of test_cumsum_sum_logsumexp_bit_exact."""
    rng = np.random.default_rng(n)
    x = rng.uniform(0, 1, n).astype(f32)
    x /= x.sum()
    lw = rng.normal(0, 3, n).astype(f32)
    return x, lw


@pytest.mark.parametrize("n", LADDER)
def test_cumsum_in_place(n, oracle, dev):
    from fbs_amd import _lib, ops
    x, _ = _reduction_inputs(n)
    buf, first = _guarded(n, dev)
    buf[first:first + n] = _up(x, dev)
    _lib.call("fbsmi_cumsum", _fptr(buf, first), n, _fptr(buf, first), ops._ws(n, dev).data_ptr(), _stream())
    torch.cuda.synchronize()
    _check_guarded(buf, first, n, oracle.cumsum(x), f"cumsum in place n={n}")


@pytest.mark.parametrize("n", LADDER)
def test_normalise_in_place(n, oracle, dev):
    from fbs_amd import _lib, ops
    _, lw = _reduction_inputs(n)
    want_lse, want_ess = f32(oracle.logsumexp(lw)), f32(oracle.ess(lw))
    ws = ops._ws(n, dev)
    for log_space in (1, 0):
        want = oracle.normalise(lw, bool(log_space))
        for with_ess in (False, True):
            buf, first = _guarded(n, dev)
            buf[first:first + n] = _up(lw, dev)
            scal = _nan(2, dev)
            p = _fptr(buf, first)
            if with_ess:
                _lib.call("fbsmi_normalise_ess", p, n, log_space, p, _fptr(scal, 0), _fptr(scal, 1), ws.data_ptr(), _stream())
            else:
                _lib.call("fbsmi_normalise", p, n, log_space, p, _fptr(scal, 0), ws.data_ptr(), _stream())
            torch.cuda.synchronize()
            what = f"normalise{'_ess' if with_ess else ''} in place n={n} log_space={log_space}"
            _check_guarded(buf, first, n, want, what)
            got = _np(scal)
            _eq(got[0], want_lse, what + ": lse")
            if with_ess:
                _eq(got[1], want_ess, what + ": ess")


# ---- g. the linear-Gaussian closures past one grid pass (4096 x 256 threads) ----------------------------------------------
def _bridge(toy, dev):
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    toy = toy()
    ts = np.linspace(0.0, 1.0, 9)
    return ts, fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(-0.5, 1.0), ts, toy["du"], device=dev)


@pytest.mark.parametrize("toy", [toy_4d, toy_2d])
def test_transition_sampler_past_one_grid_pass(toy, oracle, dev):
    """n = 600001 rows: with toy_4d (du = 2) n * du = 1200002 elements, past the 1048576 threads of one grid pass -- whole,
    and as the row slice (300000, 300001, 600001) of a sharded ensemble.  toy_2d (du = 1) is the same call below the bound."""
    ts, br = _bridge(toy, dev)
    om = oracle_model_from(oracle, br)
    n, k = 600001, 3
    key = oracle.PRNGKey(31)
    us_prev = oracle.normal(oracle.PRNGKey(32), (n, br.du))
    v_prev = oracle.normal(oracle.PRNGKey(33), (br.dv,))
    want = oracle.lg_transition_sampler(om, k, us_prev, v_prev, key)
    ut, vt = _up(us_prev, dev), _up(v_prev, dev)
    _eq(_np(br.transition_sampler(ut, vt, ts[k], key)), want, "transition_sampler n=600001")
    piece = br.transition_sampler(ut[300000:].contiguous(), vt, ts[k], key, row_slice=(300000, 300001, n))
    _eq(_np(piece), want[300000:], "row-sliced transition_sampler (300000, 300001, 600001)")


@pytest.mark.parametrize("toy", [toy_4d, toy_2d])
def test_logpdfs_past_one_grid_pass(toy, oracle, dev):
    ts, br = _bridge(toy, dev)
    om = oracle_model_from(oracle, br)
    n, k = 1100001, 5
    us_prev = oracle.normal(oracle.PRNGKey(41), (n, br.du))
    v_prev = oracle.normal(oracle.PRNGKey(42), (br.dv,))
    v = oracle.normal(oracle.PRNGKey(43), (br.dv,))
    u = oracle.normal(oracle.PRNGKey(44), (br.du,))
    ut, vt = _up(us_prev, dev), _up(v_prev, dev)
    _eq(_np(br.likelihood_logpdf(_up(v, dev), ut, vt, ts[k])), oracle.lg_likelihood_logpdf(om, k, v, us_prev, v_prev),
        "likelihood_logpdf n=1100001")
    _eq(_np(br.transition_logpdf(_up(u, dev), ut, vt, ts[k])), oracle.lg_transition_logpdf(om, k, u, us_prev, v_prev),
        "transition_logpdf n=1100001")
