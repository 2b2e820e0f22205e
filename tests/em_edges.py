"""Case tables of the image SMC-step kernels (fbs_amd/csrc/fbsmi_em.hip) at their dispatch branches and mask edges, shared by
tests/test_em_edges_host.py (CPU: every case plans the kernel and flags its table says) and tests/test_gpu_em_edges.py (GPU:
the same cases, bit for bit against oracle/em.py).  Synthetic masks from run-length recipes -- ImageRestore's masks are
rectangles and strided grids, every run s*c long and friendly aligned --, a draw by index (element i of a 2^32-element
normal draw without the draw), and the inputs and expected outputs of every case, computed once per (case, dtype, mode).
Not collected: the tests import it.  Nothing here needs a GPU; device_mask() imports torch when called."""
import ctypes as C
import functools
import zlib
from types import SimpleNamespace as NS

import numpy as np

f32 = np.float32
NAN_BITS = 0x7FC00000            # the sentinel of every output and guard element (what torch.full(..., nan) stores)
GUARD = 8                        # guard elements on either side of a buffer (8 floats keep a 16-byte aligned start aligned)
CX, CS, DT, SD = f32(0.37), f32(1.9), f32(0.002), f32(0.0721)
FULL_DRAW_MAX = 1 << 21          # flat draws up to this size come from oracle.normal, larger ones from normal_at()
MAX_DRAW = (1 << 32) - 4         # the largest n_total * du fbsmi_em_finish admits (the 2^32 finding)
DTYPES = ("f32", "bf16")
MODES = (0, 1)


# ---- synthetic masks -------------------------------------------------------------------------------------------------------
def _alternating(du, dv, next_len, lead_v=0):
    """Runs of unobserved / observed elements in turn (the first one unobserved, after `lead_v` observed elements); a run is
    next_len(pos) long, cut to what its part has left; when a part runs out the other one closes the image in one run."""
    left = [du, dv - min(lead_v, dv)]
    runs = [(1, min(lead_v, dv))] if lead_v else []
    pos, part = runs[0][1] if runs else 0, 0
    while left[0] or left[1]:
        if not left[part]:
            part ^= 1
            ln = left[part]
        elif not left[part ^ 1]:
            ln = left[part]
        else:
            ln = min(next_len(pos), left[part])
        runs.append((part, ln))
        left[part] -= ln
        pos += ln
        part ^= 1
    return runs


def _len357(pos):
    """3, 5, 7 in turn, skipping a length that would put the run's end on a multiple of 4."""
    for k in range(3):
        ln = (3, 5, 7)[(pos + k) % 3]
        if (pos + ln) % 4:
            return ln
    raise AssertionError(pos)


def _runs(du, dv, recipe):
    name, _, arg = recipe.partition("@")
    j = int(arg) if arg else 0
    if name in ("u_first", "v_tail"):
        return [(0, du), (1, dv)]
    if name in ("u_last", "u_tail"):
        return [(1, dv), (0, du)]
    if name == "singletons":
        return _alternating(du, dv, lambda pos: 1)
    if name == "runs357":
        return _alternating(du, dv, _len357)
    if name == "runs4":                       # runs of 4 that start at image offset j mod 4: consecutive, never aligned
        return _alternating(du, dv, lambda pos: 4, lead_v=j)
    if name == "runs8":                       # aligned runs: every group of four consecutive and aligned
        return _alternating(du, dv, lambda pos: 8)
    if name in ("u_end", "v_end"):            # the last j elements of a part open an aligned group of the image
        a, b = (du, dv) if name == "u_end" else (dv, du)
        gap = (-(a - j)) % 4 or 4
        assert a > j and b > gap + 2, (recipe, du, dv)
        me, other = (0, 1) if name == "u_end" else (1, 0)
        return [(me, a - j), (other, gap), (me, j), (other, b - gap)]
    raise ValueError(recipe)


@functools.lru_cache(maxsize=None)
def mask_tables(du, dv, recipe):
    """-> (u_off, v_off, role) int32: u_off and v_off partition range(D), role is the inverse map (oracle/em.py:
    element_tables).  Recipes: u_first / u_last (one long unobserved block first / last), singletons, runs357 (no run ends
    on a multiple of 4), runs4@1..3, runs8, u_end@j / v_end@j (a part ends j elements into an aligned group of the image),
    u_tail@j / v_tail@j (the part's last group of four table entries STARTS at image offset D - j: the tables of a part
    need not ascend, and a 16-byte load at that offset would leave the row)."""
    D = du + dv
    parts = [[], []]
    pos = 0
    for part, ln in _runs(du, dv, recipe):
        parts[part].extend(range(pos, pos + ln))
        pos += ln
    assert pos == D and len(parts[0]) == du and len(parts[1]) == dv, (recipe, du, dv)
    u_off, v_off = np.array(parts[0], np.int64), np.array(parts[1], np.int64)
    name, _, arg = recipe.partition("@")
    if name in ("u_tail", "v_tail"):
        t = u_off if name == "u_tail" else v_off
        assert t.size >= 4 and t.size % 4 == 0 and t[-1] == D - 1
        t[-4:] = np.roll(t[-4:], -(4 - int(arg)))
        assert t[-4] == D - int(arg)
    role = np.zeros(D, np.int64)
    role[u_off] = np.arange(du)
    role[v_off] = ~np.arange(dv)
    out = tuple(a.astype(np.int32) for a in (u_off, v_off, role))
    for a in out:
        a.setflags(write=False)
    return out


RECIPES = ("u_first", "u_last", "singletons", "runs357", "runs4@1", "runs4@2", "runs4@3", "runs8")
TAILS = tuple(f"{p}_tail@{j}" for p in "uv" for j in (1, 2, 3))
ENDS = tuple(f"{p}_end@{j}" for p in "uv" for j in (1, 2, 3))


def run_lengths(off):
    """Lengths of the runs of consecutive offsets of a table."""
    cut = np.flatnonzero(np.diff(off) != 1) + 1
    return np.diff(np.concatenate([[0], cut, [off.size]]))


class DeviceMask:
    """_lib.EMMaskStruct over device copies of (u_off, v_off, role).  shift: {table name: elements} puts that table that
    many int32 past its 16-byte aligned place (for the refusals and the element-wise variants)."""

    def __init__(self, tables, dev, shift=None):
        import torch
        from fbs_amd import _lib
        shift = shift or {}
        self.du, self.dv = int(tables[0].size), int(tables[1].size)
        self.D = self.du + self.dv
        self.bufs, ptrs = [], []
        for name, t in zip(("u_off", "v_off", "role"), tables):
            s = int(shift.get(name, 0))
            buf = torch.full((t.size + 2 * GUARD + s,), -(1 << 30), dtype=torch.int32, device=dev)
            buf[GUARD + s:GUARD + s + t.size] = torch.from_numpy(np.array(t)).to(dev)
            self.bufs.append(buf)
            ptrs.append(buf.data_ptr() + 4 * (GUARD + s) if t.size else None)
        self.snapshot = [b.clone() for b in self.bufs]
        self.struct = _lib.EMMaskStruct(self.du, self.dv, *ptrs)
        self.ref = C.byref(self.struct)

    def unchanged(self):
        import torch
        return all(torch.equal(a, b) for a, b in zip(self.bufs, self.snapshot))


def host_mask(du, dv, shift=None):
    """The same struct with made-up table addresses: enough for the plan functions, which read the values only."""
    from fbs_amd import _lib
    shift = shift or {}
    at = lambda k, name, size: (0x10000000 * (k + 1) + 4 * int(shift.get(name, 0))) if size else None
    m = _lib.EMMaskStruct(du, dv, at(0, "u_off", du), at(1, "v_off", dv), at(2, "role", du + dv))
    return m


# ---- a draw by index -------------------------------------------------------------------------------------------------------
def threefry2x32_np(key, c0, c1):
    """Threefry-2x32, 20 rounds, on arrays of counter pairs -> the two output words (checked against oracle.random_bits
    by tests/test_em_edges_host.py)."""
    u32 = np.uint32
    k0, k1 = u32(key[0]), u32(key[1])
    ks = (k0, k1, u32(k0 ^ k1 ^ u32(0x1BD11BDA)))
    x0 = (np.asarray(c0, np.uint64) + np.uint64(k0)).astype(u32)
    x1 = (np.asarray(c1, np.uint64) + np.uint64(k1)).astype(u32)
    rots = ((13, 15, 26, 6), (17, 29, 16, 24))
    for block in range(5):
        for r in rots[block % 2]:
            x0 = x0 + x1
            x1 = (x1 << u32(r)) | (x1 >> u32(32 - r))
            x1 = x1 ^ x0
        x0 = x0 + ks[(block + 1) % 3]
        x1 = x1 + ks[(block + 2) % 3] + u32(block + 1)
    return x0, x1


def bits_at(key, n_total, idx):
    """Elements idx of random_bits(key, n_total): jax pairs elements i and i + half, half = (n_total + 1) // 2, on the two
    words of one call with counters (i, i + half); the second counter is 0 where i + half >= n_total."""
    idx = np.asarray(idx, np.uint64)
    half = np.uint64((int(n_total) + 1) // 2)
    first = idx < half
    a = np.where(first, idx, idx - half)
    b = a + half
    with np.errstate(over="ignore"):
        o0, o1 = threefry2x32_np(key, a.astype(np.uint32), np.where(b < np.uint64(n_total), b, 0).astype(np.uint32))
    return np.where(first, o0, o1)


def normal_at(key, n_total, idx):
    """Elements idx of oracle.normal(key, (n_total,)), through the oracle's own bits_to_normal."""
    import oracle as O
    return O.bits_to_normal(bits_at(key, n_total, idx))


@functools.lru_cache(maxsize=8)
def _slice_draw(k0, k1, n_total, du, row0, n):
    import oracle as O
    key = np.array([k0, k1], np.uint32)
    if n_total * du <= FULL_DRAW_MAX:
        return O.normal(key, (n_total, du))[row0:row0 + n]
    return normal_at(key, n_total * du, row0 * du + np.arange(n * du, dtype=np.uint64)).reshape(n, du)


# ---- fbsmi_em_finish -------------------------------------------------------------------------------------------------------
def fcase(id, du, dv, recipe, n_total, row0, n, plan, want_us=True, want_lw=True, A=True, net_A=True, pin=None, shift=None,
          dtypes=DTYPES, modes=MODES, specials=()):
    """plan: what fbsmi_em_finish_plan must answer -- kernel, pair, vec always; ku for the rows kernel; vfirst where both
    roles are launched; tree (nseg > 64) defaults to False.  shift: {buffer: elements past 16-byte alignment}.
    specials: ((element of the observed part, kind), ...) of the division-branch layout."""
    plan = dict(plan)
    plan.setdefault("tree", False)
    return NS(id=id, du=du, dv=dv, recipe=recipe, n_total=n_total, row0=row0, n=n, plan=plan, want_us=want_us, want_lw=want_lw,
              A=A and want_us, net_A=net_A, pin=pin, shift=shift or {}, dtypes=dtypes, modes=modes, specials=tuple(specials))


ROWS = lambda ku: dict(kernel="rows", pair=0, vec=1, ku=ku)
TWO = lambda pair, vec, **kw: dict(kernel="finish", pair=pair, vec=vec, **kw)
DIV_SPECIALS = ((300, "zero"), (800, "big"), (900, "tiny"))      # segment 1: one df == 0; segment 3: |df| > 2^30, < 2^-30
DIV_SMALL = ((300, "zero"), (900, "tiny"))      # without the 2^62 / var term, whose size hides every other term of its row


def _slice(id, du, dv, plan, recipe="runs8", n=64, **kw):
    """A rank's row slice: rows [100, 100 + n) of 200, proposal and weights, ancestors, net_A, a pin row inside."""
    return fcase(id, du, dv, recipe, 200, 100, n, plan, pin=n // 2, **kw)


_UPPER_TOTAL = (MAX_DRAW - 4) // 1028
_LAST3_TOTAL = MAX_DRAW // 3

# a. k_em_rows: every condition of the dispatch with a case on either side
ROWS_CASES = [
    _slice("rows-n64", 12, 20, ROWS(1)),
    _slice("rows-n65", 12, 20, ROWS(1), n=65),
    _slice("rows-n63", 12, 20, TWO(0, 1, vfirst=1), n=63),
] + [
    _slice(f"rows-du{du}", du, 8 if du % 8 == 0 else 12, ROWS((du + 1023) // 1024))
    for du in (4, 1024, 1028, 2048, 2052, 3072, 4096)
] + [
    _slice("rows-du4100", 4100, 12, TWO(0, 1, vfirst=1)),
    # row bytes 48, 1024, 1040, 2064: the last LDS-DMA chunk ragged, absent, one lane
    _slice("rows-rb48-f32", 4, 8, ROWS(1), dtypes=("f32",)), _slice("rows-rb48-bf16", 4, 20, ROWS(1), dtypes=("bf16",)),
    _slice("rows-rb1024-f32", 4, 252, ROWS(1), dtypes=("f32",)), _slice("rows-rb1024-bf16", 4, 508, ROWS(1), dtypes=("bf16",)),
    _slice("rows-rb1040-f32", 4, 256, ROWS(1), dtypes=("f32",)), _slice("rows-rb1040-bf16", 4, 516, ROWS(1), dtypes=("bf16",)),
    _slice("rows-rb2064-f32", 4, 512, ROWS(1), dtypes=("f32",)), _slice("rows-rb2064-bf16", 4, 1028, ROWS(1), dtypes=("bf16",)),
    # the LDS budget in float32: 51 KiB of row + 256 bytes of segment sums fit 52 KiB, 52 KiB of row do not
    _slice("rows-lds-fits", 4096, 8960, ROWS(4), dtypes=("f32",)),
    _slice("rows-lds-over", 4096, 8964, TWO(0, 1, vfirst=1), dtypes=("f32",)),
    _slice("rows-lds-13248", 4096, 9152, TWO(0, 1, vfirst=1), dtypes=("f32",)),
    _slice("rows-lds-13252", 4096, 9156, TWO(0, 1, vfirst=1), dtypes=("f32",)),
    _slice("rows-bf16-nseg65", 8, 16640, dict(ROWS(1), tree=True), dtypes=("bf16",)),
    _slice("rows-bf16-rowbytes8", 8, 12, TWO(0, 1, vfirst=1), dtypes=("bf16",)),
    _slice("rows-net-shift", 12, 20, TWO(0, 1, vfirst=1), shift={"net": 1}),
] + [
    _slice(f"rows-mask-{r}", 40, 56, ROWS(1), recipe=r) for r in ("runs4@1", "runs4@2", "runs4@3", "singletons", "runs357")
] + [
    fcase("rows-upper-half", 1028, 12, "runs357", _UPPER_TOTAL, _UPPER_TOTAL - 70, 64, ROWS(2), pin=9),
    fcase("rows-div", 8, 1024, "runs8", 200, 100, 64, ROWS(1), pin=32, specials=DIV_SPECIALS),
    fcase("rows-div-small", 8, 1024, "runs8", 200, 100, 64, ROWS(1), pin=32, specials=DIV_SMALL),
]

# b. the role map of the two-role kernel: whole draws on both sides of nU + nV = 8192
ROLE_CASES = [
    fcase("roles-8200", 4, 4, "u_first", 8200, 0, 8200, TWO(1, 1, vfirst=0, nU=17, nV=8200), pin=4101),
    fcase("roles-6000", 1024, 4, "u_first", 6000, 0, 6000, TWO(1, 1, vfirst=0, nU=3000, nV=6000), pin=5999),
    fcase("roles-8100", 4, 4, "u_first", 8100, 0, 8100, TWO(1, 1, vfirst=1, nU=16, nV=8100), pin=0),
    fcase("roles-8200-proposal", 4, 4, "u_first", 8200, 0, 8200, TWO(1, 1, vfirst=0, nU=17, nV=0), want_lw=False),
    fcase("roles-8200-weights", 4, 4, "u_first", 8200, 0, 8200, TWO(1, 1, vfirst=0, nU=0, nV=8200), want_us=False),
]

# c. log-density geometry through dv (weights only, the other part as small as the kernel permits, 3 rows)
LOGPDF_D = (1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 259, 1023, 1024, 1025, 2049, 3073, 16384, 16385, 16640)
STRADDLE_D = (1025, 2049, 3073)


def _weights(id, du, dv, recipe="u_first", **kw):
    return fcase(id, du, dv, recipe, 3, 0, 3, TWO(1, 0, vfirst=0, nU=0, nV=3, tree=dv > 16384), want_us=False, **kw)


WEIGHT_CASES = [_weights(f"lw-d{d}", max(1, 4 - d), d, net_A=d in (257, 1025)) for d in LOGPDF_D] + \
               [_weights(f"lw-d{d}-runs357", d, d, "runs357") for d in STRADDLE_D] + \
               [_weights("lw-dv0", 4, 0, net_A=False)]

# e. proposal fallbacks and the pin
PROPOSAL_CASES = [
    fcase("prop-half18", 12, 4, "runs4@2", 3, 0, 3, TWO(1, 0, vfirst=1)),                 # half % 4 != 0, du % 4 == 0
    fcase("prop-us-shift", 8, 8, "runs8", 5, 0, 5, TWO(1, 0, vfirst=1), shift={"us": 1}),
    fcase("prop-usnew-shift", 8, 8, "runs8", 5, 0, 5, TWO(1, 0, vfirst=1), shift={"us_new": 1}),
    fcase("prop-odd-total", 3, 5, "singletons", 5, 0, 5, TWO(1, 0, vfirst=1), pin=2),     # 15 elements: the last counter padded
    fcase("prop-slice-scalar", 3, 5, "singletons", 11, 3, 5, TWO(0, 0, vfirst=1), pin=4),
    fcase("prop-slice-us-shift", 8, 8, "runs8", 11, 3, 5, TWO(0, 0, vfirst=1), shift={"us": 1}),
    fcase("prop-n1", 8, 8, "runs357", 1, 0, 1, TWO(1, 1, vfirst=1)),
    fcase("prop-pin-upper", 8, 8, "runs357", 6, 0, 6, TWO(1, 1, vfirst=1), pin=4),
    fcase("prop-pin-shift", 8, 8, "runs357", 6, 0, 6, TWO(1, 1, vfirst=1), pin=4, shift={"pin": 1}),
    fcase("pin-without-usnew", 8, 8, "runs357", 6, 0, 6, TWO(1, 1, vfirst=0, nU=0), pin=4, want_us=False),
] + [
    # the two-role kernel's 16-byte network loads on every recipe, and at the end of the row (the D - 4 clamp)
    fcase(f"two-role-mask-{r}", 40, 56, r, 6, 0, 6, TWO(1, 1, vfirst=1), pin=3) for r in RECIPES
] + [
    fcase(f"two-role-mask-{r}", 8, 8, r, 5, 0, 5, TWO(1, 1, vfirst=1)) for r in TAILS
]

# f. the largest draw the check admits: a scalar-path slice of its last three rows (du = 3)
BOUNDARY_CASES = [fcase("wrap-last3", 3, 1, "u_first", _LAST3_TOTAL, _LAST3_TOTAL - 3, 3, TWO(0, 0, vfirst=1))]
FIRST_REFUSED_TOTAL = _LAST3_TOTAL + 1

FINISH_CASES = ROWS_CASES + ROLE_CASES + WEIGHT_CASES + PROPOSAL_CASES + BOUNDARY_CASES


def expand(cases):
    """-> [(case, dtype, mode)], ids for pytest.mark.parametrize."""
    out = [(c, dt, m) for c in cases for dt in c.dtypes for m in c.modes]
    return out, [f"{c.id}-{dt}-mode{m}" for c, dt, m in out]


def _rng(case, dtype, mode):
    return np.random.default_rng(zlib.crc32(f"{case.id}/{dtype}/{mode}".encode()))


def _net(rng, rows, D, dtype):
    """-> (float32 values, what the device is handed: the same float32 or the bfloat16 bit patterns)."""
    from oracle import em
    net = rng.normal(size=(rows, D)).astype(f32)
    if dtype == "f32":
        return net, net
    bits = em.to_bf16_bits(net)
    return em.from_bf16_bits(bits), bits


def _mean(mode, base, s):
    """base + drift * dt as oracle/em.py rounds it, for one element."""
    from oracle import em
    b, s = np.array([base], f32), np.array([s], f32)
    return (b + (em._drift(mode, CX, CS, b, s) * DT).astype(f32)).astype(f32)[0]


def _apply_specials(specials, mode, base_cols, net, off, target):
    """The division-branch layout: element j of the summed part gets a base and a network value constant over the rows, and
    a target that makes df exactly 0 (the float32 mean the oracle computes), |df| = 2^31 or df = 2^-40 (mean 0)."""
    for j, kind in specials:
        b, s = (f32(0.0), f32(0.0)) if kind == "tiny" else (f32(0.25), f32(0.5))      # 0.5: exact in bfloat16
        base_cols[..., j] = b
        net[:, off[j]] = s
        m = _mean(mode, b, s)
        target[j] = {"zero": m, "big": f32(2.0 ** 31), "tiny": f32(2.0 ** -40)}[kind]
        assert kind != "tiny" or m == 0.0


@functools.lru_cache(maxsize=4)
def finish_inputs(case_id, dtype, mode):
    """Inputs and expected outputs of a case: us, net and net_A's source carry one spare row beyond n."""
    import oracle as O
    from oracle import em
    c = FINISH_BY_ID[case_id]
    rng = _rng(c, dtype, mode)
    u_off, v_off, role = mask_tables(c.du, c.dv, c.recipe)
    n, rows, D = c.n, c.n + 1, c.du + c.dv
    net, net_dev = _net(rng, rows, D, dtype)
    us = rng.normal(size=(rows, c.du)).astype(f32) if c.want_us else None
    A = rng.integers(0, rows, n).astype(np.int32) if c.A else None
    net_A = rng.permutation(rows)[:n].astype(np.int32) if c.net_A else None
    vv = rng.normal(size=(2, c.dv)).astype(f32)              # rows of a (T + 1, dv) path: dword aligned only for odd dv
    pin_val = rng.normal(size=c.du).astype(f32) if c.pin is not None else None
    if c.specials:
        _apply_specials(c.specials, mode, vv[0], net, v_off, vv[1])
        if dtype == "bf16":
            net_dev = em.to_bf16_bits(net)
            assert np.array_equal(em.from_bf16_bits(net_dev).view(np.uint32), net.view(np.uint32))
    key = O.PRNGKey(1000 + zlib.crc32(c.id.encode()) % 1000)
    z = _slice_draw(int(key[0]), int(key[1]), c.n_total, c.du, c.row0, n) if c.want_us else None
    want_us, want_lw = em.finish(None if us is None else (us if A is not None else us[:n]), A,
                                 net[net_A] if net_A is not None else net[:n], mode, CX, CS, DT, SD, vv[1], vv[0], key,
                                 c.n_total, c.row0, -1 if c.pin is None else c.pin, pin_val, u_off, v_off,
                                 want_us=c.want_us, want_lw=c.want_lw, z=z)
    return NS(case=c, us=us, A=A, net=net, net_dev=net_dev, net_A=net_A, vv=vv, pin_val=pin_val, key=key, z=z,
              want_us=want_us, want_lw=want_lw, tables=(u_off, v_off, role))


def finish_ptrs_host(case, dtype):
    """Made-up device addresses with the case's misalignments, for the plan function on a machine without a GPU."""
    esz = {"f32": 4, "bf16": 2}
    at = lambda k, name, size=4: 0x20000000 * (k + 1) + size * int(case.shift.get(name, 0))
    return dict(us=at(0, "us") if case.want_us else None, net=at(1, "net", esz[dtype]), v=at(2, "v"), v_prev=at(3, "v_prev"),
                pin=at(4, "pin") if case.pin is not None else None, us_new=at(5, "us_new") if case.want_us else None,
                lw=at(6, "lw") if case.want_lw else None)


def plan_finish(mask_ref, case, dtype, mode, p, n_total=None, row0=None, n=None, pin=None):
    """fbsmi_em_finish_plan for the pointer values p -> (status, plan)."""
    from fbs_amd import _lib
    plan = _lib.EMPlanStruct()
    pin = (-1 if case.pin is None else case.pin) if pin is None else pin
    rc = _lib.lib().fbsmi_em_finish_plan(mask_ref, p["us"], p["net"], DTYPES.index(dtype), mode, p["v"], p["v_prev"],
                                         case.n_total if n_total is None else n_total, case.row0 if row0 is None else row0,
                                         case.n if n is None else n, pin, p["pin"], p["us_new"], p["lw"], C.byref(plan))
    return rc, plan


def check_plan(plan, want, what):
    """Every field the table names must equal the plan's."""
    from fbs_amd import _lib
    got = {"kernel": _lib.EM_KERNELS[plan.kernel], "tree": plan.nseg > 64}
    got.update({k: getattr(plan, k) for k in ("pair", "vec", "ku", "nU", "nV", "vfirst", "nseg", "grid")})
    bad = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not bad, f"{what}: the plan differs from the case table (got, want): {bad}"


# ---- fbsmi_em_transition_logpdf --------------------------------------------------------------------------------------------
def tcase(id, du, dv, recipe="u_first", n=3, dtypes=DTYPES, modes=MODES, specials=()):
    return NS(id=id, du=du, dv=dv, recipe=recipe, n=n, dtypes=dtypes, modes=modes, specials=tuple(specials),
              plan=dict(kernel="translp", nV=n, tree=du > 16384))


TRANS_CASES = [tcase(f"tl-d{d}", d, max(0, 4 - d)) for d in LOGPDF_D] + \
              [tcase(f"tl-d{d}-runs357", d, d, "runs357") for d in STRADDLE_D] + \
              [tcase("tl-n1", 259, 0, n=1), tcase("tl-div", 1024, 8, "runs8", specials=DIV_SPECIALS),
               tcase("tl-div-small", 1024, 8, "runs8", n=16, specials=DIV_SMALL)] + \
              [tcase(f"tl-mask-{r}", 40, 56, r) for r in RECIPES] + [tcase(f"tl-mask-{r}", 8, 8, r) for r in TAILS[:3]]


@functools.lru_cache(maxsize=4)
def trans_inputs(case_id, dtype, mode):
    from oracle import em
    c = TRANS_BY_ID[case_id]
    rng = _rng(c, dtype, mode)
    u_off, v_off, role = mask_tables(c.du, c.dv, c.recipe)
    rows = c.n + 1
    net, net_dev = _net(rng, rows, c.du + c.dv, dtype)
    us = rng.normal(size=(rows, c.du)).astype(f32)
    uu = rng.normal(size=(2, c.du)).astype(f32)              # the target is row 1 of a (T + 1, du) path
    if c.specials:
        _apply_specials(c.specials, mode, us, net, u_off, uu[1])
        if dtype == "bf16":
            net_dev = em.to_bf16_bits(net)
    want = em.transition_logpdf(us[:c.n], net[:c.n], mode, CX, CS, DT, SD, uu[1], u_off)
    return NS(case=c, us=us, net=net, net_dev=net_dev, uu=uu, want=want, tables=(u_off, v_off, role))


def plan_trans(mask_ref, case, dtype, mode, us, net, u, lw, n=None):
    from fbs_amd import _lib
    plan = _lib.EMPlanStruct()
    rc = _lib.lib().fbsmi_em_transition_logpdf_plan(mask_ref, us, net, DTYPES.index(dtype), mode, u, case.n if n is None else n,
                                                    lw, C.byref(plan))
    return rc, plan


# ---- fbsmi_em_concat -------------------------------------------------------------------------------------------------------
# float32 inputs whose bfloat16 rounding is an edge: (bits, bfloat16 bits the header's rule gives)
BF16_EDGES = (
    (0x3F808000, 0x3F80),     # a tie, to even (down)
    (0x3F818000, 0x3F82),     # a tie, to even (up, from an odd mantissa)
    (0x7F800001, 0x7FC0),     # NaN whose payload the rounding increment would turn into +inf
    (0x7FFFFFFF, 0x7FFF),     # NaN that the increment would carry into the sign bit (-0.0)
    (0xFFFF8000, 0xFFFF),     # negative NaN that the increment would carry out of the word (+0.0)
    (0x7FC00000, 0x7FC0),     # the default NaN
    (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),       # +-inf
    (0x7F7FFFFF, 0x7F80),     # the largest finite float rounds to +inf
    (0x00000001, 0x0000), (0x00008000, 0x0000), (0x00018000, 0x0002), (0x807FFFFF, 0x8080),       # denormals
)


def ccase(id, du, dv, recipe="u_first", vec=1, shift=None, edges=False):
    return NS(id=id, du=du, dv=dv, recipe=recipe, shift=shift or {}, edges=edges, n=3,
              plan=dict(kernel="concat", vec=vec, ku=(du + dv + 4095) // 4096))


def _split(D):
    """An image of D floats in two parts of at least 4 where it can be (the 16-byte variant needs both)."""
    du = max(4, (D // 2) & ~3) if D >= 8 else D - 1
    return du, D - du


CONCAT_CASES = [ccase(f"cat-D{D}", *_split(D), recipe="runs357", vec=int(D >= 8)) for D in (4, 8, 4092, 4096, 4100, 8196)] + \
               [ccase(f"cat-du{du}-dv{dv}", du, dv, "singletons", vec=int(du == 4 and dv == 4))
                for du in (1, 3, 4) for dv in (0, 3, 4)] + \
               [ccase("cat-img-shift", 40, 56, "runs8", vec=0, shift={"img": 1}),
                ccase("cat-role-shift", 40, 56, "runs8", vec=0, shift={"role": 1}),
                ccase("cat-D-odd", 41, 56, "runs8", vec=0)] + \
               [ccase(f"cat-mask-{r}", 40, 56, r) for r in RECIPES + ENDS] + \
               [ccase(f"cat-mask-{r}", 8, 8, r) for r in TAILS] + \
               [ccase("cat-bf16-edges", 16, 16, "runs4@2", edges=True), ccase("cat-bf16-edges-scalar", 15, 16, "runs357", vec=0, edges=True)]


@functools.lru_cache(maxsize=4)
def concat_inputs(case_id):
    from oracle import em
    c = CONCAT_BY_ID[case_id]
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    u_off, v_off, role = mask_tables(c.du, c.dv, c.recipe)
    rows = c.n + 1
    us = rng.normal(size=(rows, c.du)).astype(f32)
    vp = rng.normal(size=c.dv).astype(f32)
    if c.edges:                                   # the edge patterns in both sources, at every phase of a group of four
        bits = np.array([b for b, _ in BF16_EDGES], np.uint32)
        us.view(np.uint32)[1, :] = np.resize(bits, c.du)
        us.view(np.uint32)[2, :] = np.resize(np.roll(bits, 1), c.du)
        vp.view(np.uint32)[:] = np.resize(np.roll(bits, 2), c.dv)
    A = rng.integers(0, rows, c.n).astype(np.int32)
    want = {False: em.concat(us, None, vp, role), True: em.concat(us, A, vp, role)}
    return NS(case=c, us=us, vp=vp, A=A, want=want, tables=(u_off, v_off, role))


def plan_concat(mask_ref, us, v_prev, n, out_dtype, img):
    from fbs_amd import _lib
    plan = _lib.EMPlanStruct()
    rc = _lib.lib().fbsmi_em_concat_plan(mask_ref, us, v_prev, n, DTYPES.index(out_dtype), img, C.byref(plan))
    return rc, plan


# h. the valid call every refusal spoils in one way
REFUSAL_CASE = fcase("refusal-base", 8, 8, "runs8", 6, 0, 6, TWO(1, 1, vfirst=1), pin=2)
FINISH_BY_ID = {c.id: c for c in FINISH_CASES + [REFUSAL_CASE]}
TRANS_BY_ID = {c.id: c for c in TRANS_CASES}
CONCAT_BY_ID = {c.id: c for c in CONCAT_CASES}
assert len(FINISH_BY_ID) == len(FINISH_CASES) + 1 and len(TRANS_BY_ID) == len(TRANS_CASES) and len(CONCAT_BY_ID) == len(CONCAT_CASES)

# h. refusals of fbsmi_em_finish: (id, what is spoilt in REFUSAL_CASE, a word of the message)
REFUSALS = (
    ("u_off-misaligned", dict(mask_shift={"u_off": 1}), "16-byte"),
    ("v_off-misaligned", dict(mask_shift={"v_off": 1}), "16-byte"),
    ("image-below-4", dict(du=2, dv=1), "fewer than 4"),
    ("us_new-is-us", dict(alias=True), "alias"),
    ("pin-row-past-n", dict(pin=6), "pin"),
    ("pin-without-value", dict(pin=2, no_pin_value=True), "pin"),
    ("rows-past-n_total", dict(n_total=5), "bad arguments"),
    ("weights-without-v", dict(no_v=True), "weights need v"),
)
