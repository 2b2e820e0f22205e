"""CPU: what tests/test_gpu_train_edges.py rests on -- every shape of tests/train_edges.py lands in the branch of
fbs_amd/csrc/fbsmi_train.hip it is listed for and the shapes together cover the branches; the bfloat16 reference equals an
independent rounding on the special values and tells the two obvious mistakes apart; the clip restatement at a squared norm
of 0, inf and NaN; the extended inputs leave the old ones as they were."""
import os
import re

import numpy as np
import pytest
import torch

import train_edges as E
import train_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mirror_constants_are_the_kernels():
    """The mirror is written by hand; its four constants are read back from the source so that a change there fails here."""
    src = open(os.path.join(ROOT, "fbs_amd", "csrc", "fbsmi_train.hip")).read()
    dev = open(os.path.join(ROOT, "fbs_amd", "csrc", "fbsmi_device.h")).read()
    num = lambda name, text: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert num("kItems", src) * num("kBlock", dev) == E.CHUNK and num("kBlock", dev) == E.BLOCK
    assert re.search(r"constexpr int kChunk = kBlock \* kItems;", src)
    assert num("kMaxRowGroups", src) == E.ROW_GROUPS and num("kMaxFlatGroups", src) == E.FLAT_GROUPS


def test_row_lengths_land_in_their_branches():
    for D, (loss_branch, noise_branch, why) in E.ROW_LENGTHS.items():
        for B in ((2,) if D in E.BIG_DS else E.EDGE_BS):
            vec, nch, wpr, loops, rows = E.loss_dispatch(B, D)
            assert E.row_branch(vec, wpr, loops) == loss_branch, (D, why)
            assert rows == 1
        vec, bpr, loops = E.noise_dispatch(D)
        assert E.row_branch(vec, bpr, loops) == noise_branch, (D, why)
    # the particular reasons
    assert E.loss_dispatch(1, 2048)[1:4] == (1, 1, 1) and E.noise_dispatch(2048) == (True, 1, 1)
    assert E.loss_dispatch(1, 2056)[1] == 2 and 2056 - 2048 == 8
    assert E.loss_dispatch(1, 3072)[1] == 2 and E.loss_dispatch(1, 12288)[1] == 6
    assert 2052 % 4 == 0 and E.loss_dispatch(1, 2052)[:2] == (False, 2)
    assert E.loss_dispatch(2, 64 * 2048 + 8) == (True, 65, 64, 2, 1)
    assert E.noise_dispatch(64 * 256 * 8 + 8) == (True, 64, 2)
    assert E.noise_dispatch(64 * 256 * 8) == (True, 64, 1)                       # one less does not loop
    # every configuration's own row length is on the 16-byte path with several chunks
    for side in (32, 64, 128):
        vec, nch = E.loss_dispatch(16, side * side * 3)[:2]
        assert vec and nch > 1 and E.noise_dispatch(side * side * 3)[0]


def test_row_counts_land_in_their_branches():
    for (B, D), (vec, nch, rows) in E.ROW_COUNTS.items():
        got = E.loss_dispatch(B, D)
        assert (got[0], got[1], got[4]) == (vec, nch, rows), (B, D)
    seen = {(min(nch, 2), rows) for (vec, nch, rows) in E.ROW_COUNTS.values()}
    assert seen >= {(c, r) for c in (1, 2) for r in (1, 2, 4)}


def test_alignment_cases_leave_the_vector_path():
    for D in E.ALIGN_DS:
        assert E.loss_dispatch(E.ALIGN_B, D)[0] and not E.loss_dispatch(E.ALIGN_B, D, aligned=False)[0]
        assert E.noise_dispatch(D)[0] and not E.noise_dispatch(D, aligned=False)[0]
    assert E.loss_dispatch(E.ALIGN_B, 3072)[1] > 1 and E.loss_dispatch(E.ALIGN_B, 784)[1] == 1


def test_old_and_new_shapes_cover_every_row_branch():
    every = {(p, g) for p in ("vec", "scalar") for g in ("one", "several", "looping")}
    ds = E.OLD_DS + tuple(E.ROW_LENGTHS)
    loss = {E.row_branch(v, w, l) for v, _, w, l, _ in (E.loss_dispatch(1, D) for D in ds)}
    noise = {E.row_branch(*E.noise_dispatch(D)) for D in ds}
    assert loss == every and noise == every
    # and the old shapes alone did not: the 16-byte path beyond one chunk is what the new ones add
    old_loss = {E.row_branch(v, w, l) for v, _, w, l, _ in (E.loss_dispatch(1, D) for D in E.OLD_DS)}
    old_noise = {E.row_branch(*E.noise_dispatch(D)) for D in E.OLD_DS}
    assert every - old_loss == {("vec", "several"), ("vec", "looping")} == every - old_noise
    assert {E.loss_dispatch(B, 3)[4] for B in E.OLD_BS} == {1}


def test_adam_lengths_land_in_their_branches():
    for (n, aligned), want in E.ADAM_LONG.items():
        assert E.adam_dispatch(n, aligned) == want, (n, aligned)
    assert max(E.adam_dispatch(n)[2] for n in (1, 3, 4, 5, 255, 256, 257, 1025)) == 1      # the old lengths: one sweep
    assert E.adam_dispatch(1029) == (True, 2, 1, 1)


# ---- bfloat16 ----
def test_bf16_reference_equals_an_independent_rounding():
    v = E.special_values()
    x = v.view(np.float32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    got = R.bf16_round_full(x)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 6
    assert np.array_equal(np.isnan(x), np.isnan(want))                            # a NaN in gives a NaN out, nothing else does
    fin = ~np.isnan(want)
    assert np.array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32))
    assert (got.view(np.uint32) & 0xffff == 0).all()                              # representable in bfloat16
    # the cases by hand
    one = lambda u: int(R.bf16_round_full(np.array([u], np.uint32).view(np.float32)).view(np.uint32)[0])
    assert one(0x3f808000) == 0x3f800000 and one(0x3f818000) == 0x3f820000
    assert one(0xbf808000) == 0xbf800000 and one(0xbf818000) == 0xbf820000
    assert one(0x7f7f7fff) == 0x7f7f0000 and one(0x7f7f8000) == 0x7f800000 and one(0xff7f8000) == 0xff800000
    assert one(0x80000000) == 0x80000000 and one(0x00007fff) == 0 and one(0x00008001) == 0x00010000


def test_bf16_reference_discriminates():
    x = E.special_values().view(np.float32)
    fin = ~np.isnan(x)
    want = R.bf16_round_full(x)
    for wrong in (E.bf16_ties_away, E.bf16_truncate):
        bad = wrong(x)
        differ = np.flatnonzero(bad[fin].view(np.uint32) != want[fin].view(np.uint32))
        assert differ.size >= 2, wrong.__name__
        assert not E.same_or_both_nan(bad, want)
    # ties away differs exactly on the ties with an even kept mantissa; truncation wherever the dropped half reaches a half
    u = x.view(np.uint32)
    away = E.bf16_ties_away(x).view(np.uint32) != want.view(np.uint32)
    assert np.array_equal(away & fin, ((u & 0x1ffff) == 0x8000) & fin)
    # the old function takes the NaN 0x7fffffff to a finite value; on everything that is not a NaN the two agree
    old = R.bf16_round(x)
    k = int(np.flatnonzero(u == 0x7fffffff)[0])
    assert np.isfinite(old[k]) and np.isnan(want[k])
    assert np.array_equal(old[fin].view(np.uint32), want[fin].view(np.uint32))
    rnd = np.random.default_rng(3).normal(size=4096).astype(np.float32)
    assert np.array_equal(R.bf16_round(rnd).view(np.uint32), R.bf16_round_full(rnd).view(np.uint32))
    assert E.same_or_both_nan(want, want) and E.special_f32(100).size == 100


# ---- inputs ----
def test_extended_inputs_keep_the_old_ones():
    assert np.array_equal(R.idx_of(5), R.IDX) and np.array_equal(R.idx_of(2), R.IDX[:2])
    assert np.array_equal(R.times_of(5), R.TIMES)
    i600, t600 = R.idx_of(600), R.times_of(600)
    assert i600.dtype == np.int32 and np.array_equal(i600[:5], R.IDX) and np.array_equal(t600[:5], R.TIMES)
    assert i600.min() == 0 and i600.max() == R.NDATA - 1 and t600.min() == 0.02 and t600.max() == 2.0
    assert np.array_equal(R.idx_of(257), i600[:257])
    # B = 5 of a shape as the parent computed it: the generator is consumed in the same order
    D = 65
    rng = np.random.default_rng(1000 + D)
    data = rng.uniform(0, 1, (R.NDATA, D)).astype(np.float32)
    net = rng.normal(size=(5, D)).astype(np.float32)
    c = R.case(D)
    assert np.array_equal(c["data"], data) and np.array_equal(c["net"], net) and np.array_equal(c["idx"], R.IDX)
    xt, xi = R.noise_f32(data, None, c["keys"], c["F"], c["sq"])
    assert np.array_equal(c["xt"], xt) and np.array_equal(c["xi"], xi)
    big = R.case(3, 257)
    assert "xt" not in big and big["xt_idx"].shape == (257, 3) and np.array_equal(big["xi"], big["xi_idx"])
    assert np.array_equal(big["x0_idx"], big["data"][big["idx"]])


def test_quotient_rows_straddle_the_short_division_range():
    q = E.quotient_rows(72)
    inside = E.in_short_division_range(q)
    assert not inside[:3].any() and inside[3:5].all() and not inside[5].any()
    assert q[3, 0] == 2.0 ** -60 and q[4, 0] == 2.0 ** 60 and q[2, 0] == 2.0 ** -61 and q[5, 0] == 2.0 ** 61
    assert (np.abs(q[1]) < 2.0 ** -126).all() and (q[1] != 0).all() and (q[:, 1::2] <= 0).all()
    assert E.sq_at(0.02).dtype == np.float32 and 0.0 < E.sq_at(0.02) < 0.1          # sqrt(1 - exp(-r)), r ~ 9e-4


# ---- the clip at a given squared norm ----
def test_clip_restatement_at_zero_inf_and_nan():
    g = np.array([0.5, -2.0, 3.0])
    assert np.array_equal(R.clip_by_global_norm_f64(g, 1.0, gnorm2=0.0), g)
    z = R.clip_by_global_norm_f64(g, 1.0, gnorm2=np.inf)
    assert np.array_equal(z, np.zeros(3))
    assert np.isnan(R.clip_by_global_norm_f64(g, 1.0, gnorm2=np.nan)).all()
    # from g itself: all zeros stay, one NaN spreads to every entry
    assert np.array_equal(R.clip_by_global_norm_f64(np.zeros(3), 1.0), np.zeros(3))
    assert np.isnan(R.clip_by_global_norm_f64(np.array([1.0, np.nan, 2.0]), 1.0)).all()
    # and the given norm is used as g's own would be
    assert np.array_equal(R.clip_by_global_norm_f64(g, 1.0, gnorm2=float(np.sum(g * g))), R.clip_by_global_norm_f64(g, 1.0))
