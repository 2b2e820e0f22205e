"""What the edge tests of the trainer's kernels share (tests/test_train_edges_host.py, tests/test_gpu_train_edges.py): a
mirror of the host dispatch of fbs_amd/csrc/fbsmi_train.hip, the tables of shapes with the branch each is there for, and the
special float32 values of the bfloat16 store.  Plain numpy; a helper, not a test file.

The mirror is written from include/fbsmi.h and the host code of the entries, not generated from them: when a constant of
the kernels changes, the table test fails and says which shape no longer reaches its branch.
"""
import numpy as np

import train_restate as R

f32 = np.float32

BLOCK = 256              # threads of a workgroup
CHUNK = 2048             # elements of a row that one workgroup reduces per round: eight per thread
ROW_GROUPS = 64          # workgroups one row spreads over before they loop
FLAT_GROUPS = 4096       # workgroups of the flat kernels before they loop


def _cdiv(a, b):
    return -(-a // b)


def noise_dispatch(D, aligned=True):
    """fbsmi_dsm_noise_batched -> (vec, bpr, loops): the 16-byte path, the workgroups of a row, and the largest number of
    rounds a thread of them makes (a thread owns elements i and i + ceil(D / 2); four consecutive i on the 16-byte path)."""
    vec = D % 8 == 0 and aligned
    half = (D + 1) // 2
    work = half // 4 if vec else half
    bpr = min(_cdiv(work, BLOCK), ROW_GROUPS)
    return vec, bpr, _cdiv(work, bpr * BLOCK)


def loss_dispatch(B, D, aligned=True):
    """fbsmi_dsm_loss_batched -> (vec, nch, wpr, loops, R): the 16-byte path, the chunks of a row, its workgroups, the
    largest number of chunks one of them takes, and the rows a thread of the finishing launch folds."""
    vec = D % 8 == 0 and aligned
    nch = _cdiv(D, CHUNK)
    wpr = min(nch, ROW_GROUPS)
    rows = 1
    while rows * BLOCK < B:
        rows *= 2
    return vec, nch, wpr, _cdiv(nch, wpr), rows


def adam_dispatch(n, aligned=True):
    """fbsmi_adam_ema_step -> (vec, groups, sweeps, tail): the 16-byte path, the workgroups, the largest number of rounds a
    thread makes in the main loop (four elements a round on the 16-byte path, one otherwise), and the elements left to the
    scalar loop behind the 16-byte one (none without it: there the scalar loop is the main loop)."""
    vec = bool(aligned)
    groups = min(_cdiv(_cdiv(n, 4) if vec else n, BLOCK), FLAT_GROUPS)
    main = n // 4 if vec else n
    return vec, groups, _cdiv(main, groups * BLOCK), n - 4 * main if vec else 0


def row_branch(vec, groups, loops):
    """('vec' | 'scalar', 'one' | 'several' | 'looping') of a row kernel."""
    return "vec" if vec else "scalar", "looping" if loops > 1 else ("several" if groups > 1 else "one")


# ---- shapes ----
# those of tests/test_gpu_train_kernels.py
OLD_DS = (1, 2, 3, 63, 64, 65, 257, 784, 2049, 64 * 2048 + 1)
OLD_BS = (1, 2, 5)

# D -> (the loss's branch, the noise's branch, what the length is there for)
ROW_LENGTHS = {
    2048: (("vec", "one"), ("vec", "one"), "exactly one full chunk"),
    2056: (("vec", "several"), ("vec", "several"), "a second chunk of 8 elements: 255 threads take the zero branch"),
    3072: (("vec", "several"), ("vec", "several"), "32 x 32 x 3, two chunks"),
    12288: (("vec", "several"), ("vec", "several"), "64 x 64 x 3, six chunks"),
    2052: (("scalar", "several"), ("scalar", "several"), "a multiple of 4 but not of 8 falls to the scalar path"),
    64 * 2048 + 8: (("vec", "looping"), ("vec", "looping"),
                    "65 chunks: the loss's 64 workgroups loop; half / 4 = 64 * 256 + 1: so do the noise's"),
}
assert 64 * 256 * 8 + 8 == 64 * 2048 + 8
BIG_DS = (12288, 64 * 2048 + 8)          # run at B = 2 only
EDGE_BS = (1, 5)

# (B, D) -> (vec, chunks of a row, rows per thread of the finishing launch)
ROW_COUNTS = {
    (256, 3): (False, 1, 1), (257, 3): (False, 1, 2), (600, 3): (False, 1, 4),
    (256, 2049): (False, 2, 1), (257, 2049): (False, 2, 2), (600, 2049): (False, 2, 4),
    (257, 4104): (True, 3, 2),
}

ALIGN_DS = (64, 784, 3072)
ALIGN_B = 3

# n, aligned -> (vec, workgroups, sweeps, tail)
ADAM_LONG = {
    (4096 * 256 * 4, True): (True, 4096, 1, 0),
    (4096 * 256 * 4 + 1029, True): (True, 4096, 2, 1),
    (4096 * 256 + 3, False): (False, 4096, 2, 0),
    (1025, False): (False, 5, 1, 0),
}


# ---- the bfloat16 store ----
def special_values():
    """float32 bit patterns at which a float32 -> bfloat16 rounding can go wrong, as a uint32 array: ties with the kept
    mantissa even and odd, one ulp either side of a tie, the last value that stays finite and the first that rounds to
    infinity, infinities, zeros, subnormals, the smallest normal, and NaNs down to the payload the plain add-and-shift
    carries out of the exponent."""
    pos = [
        0x3f808000,            # tie, kept mantissa even: down
        0x3f818000,            # tie, kept mantissa odd: up
        0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,       # one ulp either side of both
        0x3f800000, 0x3f80ffff, 0x3f7fffff,                   # exact, just under the next, across a binade
        0x7f7f7fff,            # the largest float32 that rounds to the largest finite bfloat16
        0x7f7f8000,            # a tie on an odd mantissa: rounds up into infinity
        0x7f7fffff,            # the largest finite float32
        0x7f800000,            # infinity
        0x00000000,            # zero
        0x00000001, 0x00007fff, 0x00008000, 0x00008001, 0x00018000, 0x007fffff,       # subnormals, ties among them
        0x00800000,            # the smallest normal
    ]
    nans = [0x7fc00000, 0x7fc00001, 0x7fffffff, 0xffffffff, 0x7fff8000, 0xffc00000]   # quiet NaNs
    return np.array(pos + [p | 0x80000000 for p in pos] + nans, np.uint32)


def special_f32(n):
    """special_values() as float32, tiled to n elements."""
    v = special_values().view(f32)
    return np.resize(v, n).copy()


def bf16_ties_away(x):
    """the mistake: ties away from zero (add half, truncate)"""
    u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x8000) >> 16) << 16) & 0xffffffff).astype(np.uint32).view(f32).reshape(np.shape(x))


def bf16_truncate(x):
    """the mistake: drop the low half"""
    u = np.ascontiguousarray(x, f32).view(np.uint32)
    return (u & np.uint32(0xffff0000)).view(f32).reshape(np.shape(x))


def same_or_both_nan(got, want):
    """equal bits where `want` is not NaN, NaN where it is"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    nan = np.isnan(want)
    return bool(np.all(np.where(nan, np.isnan(got), got.view(np.uint32) == want.view(np.uint32))))


# ---- the mode-1 quotient ----
def quotient_rows(D):
    """(6, D) float32 numerators xt - F x0 on both sides of the range in which the kernel takes its short division
    (|a| in [2^-60, 2^60]): zeros, subnormals, [2^-61, 2^-60), [2^-60, 2^-59), (2^59, 2^60], [2^61, 2^62); both signs, the
    bound itself first."""
    rng = np.random.default_rng(606)
    m = (1.0 + rng.integers(0, 2 ** 23, D) * 2.0 ** -23)                # [1, 2), exact in float32
    m[0] = 1.0
    sign = np.where(np.arange(D) % 2 == 0, 1.0, -1.0)
    sub = rng.integers(1, 2 ** 23, D).astype(np.uint32)
    sub[:3] = (1, 2 ** 23 - 1, 2 ** 22)
    rows = np.stack([
        np.zeros(D),
        sub.view(f32).astype(np.float64),
        m * 2.0 ** -61,
        m * 2.0 ** -60,
        m * 2.0 ** 59,
        m * 2.0 ** 61,
    ]) * sign
    rows[4, :2] = (2.0 ** 60, -2.0 ** 60)                                # the upper bound is inside
    out = rows.astype(f32)
    assert np.array_equal(out.astype(np.float64), rows)
    return out


def in_short_division_range(a):
    a = np.abs(np.asarray(a, np.float64))
    return (a >= 2.0 ** -60) & (a <= 2.0 ** 60)


def sq_at(t):
    return R.lin_tables([t], 1)[1][0]
