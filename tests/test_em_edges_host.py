"""CPU: the case tables of tests/em_edges.py reach the branches they were written for -- fbsmi_em_*_plan (host arithmetic
on pointer VALUES, no GPU) answers the kernel, flags and counts each table names --, and the pieces the GPU comparison
stands on are right: the synthetic masks, the draw by index, oracle/em.py's z argument and bfloat16 rounding, its tree sum
past 64 segments, and the oracle itself against float64 on every case."""
import ctypes as C
import math

import numpy as np
import pytest

import em_edges as E

f32 = np.float32


# ---- the plan of every case --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.FINISH_CASES, ids=[c.id for c in E.FINISH_CASES])
def test_finish_cases_plan_what_their_table_says(case):
    from fbs_amd import _lib
    mask = E.host_mask(case.du, case.dv)
    for dtype in case.dtypes:
        for mode in case.modes:
            rc, plan = E.plan_finish(C.byref(mask), case, dtype, mode, E.finish_ptrs_host(case, dtype))
            assert rc == 0, _lib.lib().fbsmi_last_error()
            E.check_plan(plan, case.plan, f"{case.id} {dtype}")
            if plan.kernel == _lib.EM_KERNELS.index("rows"):
                esz = 4 if dtype == "f32" else 2
                assert plan.lnet_bytes == -(-(case.du + case.dv) * esz // 1024) * 1024 and plan.grid == case.n
                assert plan.lds_bytes == plan.lnet_bytes + 4 * (64 if plan.nseg <= 64 else 2 * plan.nseg) <= 52 * 1024
            else:
                assert plan.grid == plan.nU + plan.nV and plan.lds_bytes == 4 * (64 if plan.nseg <= 64 else 2 * plan.nseg)


def test_finish_plan_sits_on_both_sides_of_every_condition():
    """The table has a rows-kernel case and a two-role case that differ in ONE condition of the dispatch, for each of them."""
    by = E.FINISH_BY_ID
    kern = lambda i: by[i].plan["kernel"]
    for rows, two in (("rows-n64", "rows-n63"), ("rows-du4096", "rows-du4100"), ("rows-lds-fits", "rows-lds-over"),
                      ("rows-rb48-bf16", "rows-bf16-rowbytes8"), ("rows-n64", "rows-net-shift")):
        assert kern(rows) == "rows" and kern(two) == "finish", (rows, two)
    assert sorted({c.plan["ku"] for c in E.ROWS_CASES if c.plan["kernel"] == "rows"}) == [1, 2, 3, 4]
    assert {c.plan["vfirst"] for c in E.ROLE_CASES} == {0, 1}
    assert {(c.plan["pair"], c.plan["vec"]) for c in E.FINISH_CASES if c.plan["kernel"] == "finish"} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c.plan["tree"] for c in E.ROWS_CASES) and any(c.plan["tree"] for c in E.WEIGHT_CASES)
    assert any(c.plan["tree"] for c in E.TRANS_CASES)
    up = by["rows-upper-half"]
    assert up.row0 * up.du > 1 << 31 and up.n_total * up.du <= E.MAX_DRAW
    last = by["wrap-last3"]
    assert last.n_total * last.du == E.MAX_DRAW and (last.n * last.du) % 4 and last.row0 + last.n == last.n_total


@pytest.mark.parametrize("case", E.TRANS_CASES, ids=[c.id for c in E.TRANS_CASES])
def test_transition_logpdf_cases_plan_what_their_table_says(case):
    mask = E.host_mask(case.du, case.dv)
    rc, plan = E.plan_trans(C.byref(mask), case, "f32", 0, 0x1000, 0x2000, 0x3004, 0x4000)
    assert rc == 0
    E.check_plan(plan, dict(case.plan, nseg=(case.du + 255) // 256, grid=case.n), case.id)


@pytest.mark.parametrize("case", E.CONCAT_CASES, ids=[c.id for c in E.CONCAT_CASES])
def test_concat_cases_plan_what_their_table_says(case):
    for out_dtype in E.DTYPES:
        esz = 4 if out_dtype == "f32" else 2
        mask = E.host_mask(case.du, case.dv, case.shift)
        rc, plan = E.plan_concat(C.byref(mask), 0x1000, 0x2000, case.n, out_dtype, 0x30000 + esz * case.shift.get("img", 0))
        assert rc == 0
        E.check_plan(plan, dict(case.plan, grid=case.n * case.plan["ku"]), f"{case.id} {out_dtype}")
    assert {c.plan["vec"] for c in E.CONCAT_CASES} == {0, 1} and {c.plan["ku"] for c in E.CONCAT_CASES} == {1, 2, 3}


def test_plans_refuse_what_the_entry_points_refuse():
    """Status and message without a launch: the refusals of tests/test_gpu_em_edges.py, the first draw past 2^32 - 4, and
    the calls that do nothing."""
    from fbs_amd import _lib
    L = _lib.lib()
    base = E.REFUSAL_CASE
    for rid, spoil, word in E.REFUSALS:
        c = E.fcase(rid, spoil.get("du", base.du), spoil.get("dv", base.dv), "runs8", spoil.get("n_total", base.n_total), 0,
                    base.n, {}, pin=spoil.get("pin"))
        p = E.finish_ptrs_host(c, "f32")
        if spoil.get("alias"):
            p["us_new"] = p["us"]
        if spoil.get("no_pin_value"):
            p["pin"] = None
        if spoil.get("no_v"):
            p["v"] = None
        mask = E.host_mask(c.du, c.dv, spoil.get("mask_shift"))
        rc, plan = E.plan_finish(C.byref(mask), c, "f32", 0, p)
        assert rc == -1 and plan.kernel == 0, rid
        assert word.encode() in L.fbsmi_last_error(), (rid, L.fbsmi_last_error())
    last = E.FINISH_BY_ID["wrap-last3"]
    mask = E.host_mask(last.du, last.dv)
    p = E.finish_ptrs_host(last, "f32")
    rc, plan = E.plan_finish(C.byref(mask), last, "f32", 0, p, n_total=E.FIRST_REFUSED_TOTAL, row0=E.FIRST_REFUSED_TOTAL - 3)
    assert rc == -1 and b"2^32 - 4" in L.fbsmi_last_error()
    rc, plan = E.plan_finish(C.byref(mask), last, "f32", 0, p, n=0)
    assert rc == 0 and plan.kernel == 0 and plan.grid == 0
    rc, plan = E.plan_finish(C.byref(mask), last, "f32", 0, dict(p, us_new=None, lw=None))
    assert rc == 0 and plan.kernel == 0
    rc, plan = E.plan_concat(C.byref(mask), 0x1000, 0x2000, 0, "f32", 0x3000)
    assert rc == 0 and plan.kernel == 0
    rc, plan = E.plan_trans(C.byref(mask), E.TRANS_CASES[0], "f32", 0, 0x1000, 0x2000, 0x3000, 0x4000, n=0)
    assert rc == 0 and plan.kernel == 0
    mask = E.host_mask(8, 8, {"u_off": 1})
    rc, plan = E.plan_trans(C.byref(mask), E.TRANS_CASES[0], "f32", 0, 0x1000, 0x2000, 0x3000, 0x4000)
    assert rc == -1 and b"16-byte" in L.fbsmi_last_error()


# ---- the synthetic masks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("du,dv", [(40, 56), (8, 8), (1025, 1025), (12, 4)])
def test_masks_partition_the_image_and_have_the_runs_their_recipe_names(du, dv):
    from oracle import em
    D = du + dv
    for recipe in E.RECIPES + E.TAILS + (E.ENDS if min(du, dv) > 8 else ()):
        if "tail" in recipe and (du % 4 or dv % 4):
            continue
        u_off, v_off, role = E.mask_tables(du, dv, recipe)
        assert sorted(np.concatenate([u_off, v_off]).tolist()) == list(range(D)), recipe
        assert np.array_equal(role[u_off], np.arange(du)) and np.array_equal(~role[v_off], np.arange(dv)), recipe
        rng = np.random.default_rng(0)
        us, vp = rng.normal(size=(2, du)).astype(f32), rng.normal(size=dv).astype(f32)
        img = em.concat(us, None, vp, role)
        assert np.array_equal(img[:, u_off], us) and np.array_equal(img[1, v_off], vp), recipe
    if (du, dv) != (40, 56):
        return
    runs = lambda r: (E.run_lengths(E.mask_tables(du, dv, r)[0]), E.run_lengths(E.mask_tables(du, dv, r)[1]))
    assert all((x == 1).all() for x in runs("singletons")[:1]) and (runs("singletons")[1][:-1] == 1).all()
    ru, rv = runs("runs357")
    assert set(ru[:-1].tolist()) <= {3, 5, 7} and set(rv[:-1].tolist()) <= {3, 5, 7} and len(ru) > 6
    role = E.mask_tables(du, dv, "runs357")[2]
    ends = np.flatnonzero(np.diff((role >= 0).astype(int)) != 0) + 1
    assert ends.size > 10 and (ends[:-1] % 4 != 0).all(), "a run of runs357 ends on a multiple of 4"   # the last: a part ran out
    for j in (1, 2, 3):
        u_off = E.mask_tables(du, dv, f"runs4@{j}")[0]
        starts = u_off[np.concatenate([[0], np.flatnonzero(np.diff(u_off) != 1) + 1])]
        assert (E.run_lengths(u_off) == 4).all() and (starts % 4 == j).all()
        for part, name in ((0, "u"), (1, "v")):
            t = E.mask_tables(du, dv, f"{name}_tail@{j}")[part]
            assert t[-4] == D - j and sorted(t[-4:].tolist()) == list(range(D - 4, D))
            role = E.mask_tables(du, dv, f"{name}_end@{j}")[2]
            size = (du, dv)[part]
            e = int(np.flatnonzero((role if part == 0 else ~role) == size - j)[0])
            assert e % 4 == 0 and ((role[e:e + j] >= 0) == (part == 0)).all() and ((role[e + j:e + 4] >= 0) == (part == 1)).all()
    assert E.mask_tables(du, dv, "u_first")[0][-1] == du - 1 and E.mask_tables(du, dv, "u_last")[0][0] == dv


# ---- the draw by index, the z argument, bfloat16, the tree sum -----------------------------------------------------------------
@pytest.mark.parametrize("n_total", [1, 2, 1001, 4096])
def test_draw_by_index_equals_the_oracle_draw(n_total, oracle):
    key = oracle.PRNGKey(4242 + n_total)
    idx = np.arange(n_total, dtype=np.uint64)
    assert np.array_equal(E.bits_at(key, n_total, idx), oracle.random_bits(key, n_total))
    assert np.array_equal(E.normal_at(key, n_total, idx).view(np.uint32), oracle.normal(key, (n_total,)).view(np.uint32))
    o = oracle.threefry2x32(key, 7, n_total)
    a, b = E.threefry2x32_np(key, np.array([7], np.uint32), np.array([n_total], np.uint32))
    assert (int(a[0]), int(b[0])) == (int(o[0]), int(o[1]))


def test_finish_with_z_equals_the_full_draw(oracle):
    from oracle import em
    u_off, v_off, role = E.mask_tables(5, 7, "runs357")
    rng = np.random.default_rng(1)
    n_total, row0, n = 11, 3, 5
    us, net = rng.normal(size=(n, 5)).astype(f32), rng.normal(size=(n, 12)).astype(f32)
    v, vp, pin = rng.normal(size=7).astype(f32), rng.normal(size=7).astype(f32), rng.normal(size=5).astype(f32)
    key = oracle.PRNGKey(9)
    z = E.normal_at(key, n_total * 5, row0 * 5 + np.arange(n * 5, dtype=np.uint64)).reshape(n, 5)
    for mode in (0, 1):
        a = em.finish(us, None, net, mode, E.CX, E.CS, E.DT, E.SD, v, vp, key, n_total, row0, 2, pin, u_off, v_off)
        b = em.finish(us, None, net, mode, E.CX, E.CS, E.DT, E.SD, v, vp, None, None, row0, 2, pin, u_off, v_off, z=z)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_bf16_rounding_is_nearest_even_and_keeps_nan():
    from oracle import em
    bits = np.array([b for b, _ in E.BF16_EDGES], np.uint32)
    want = np.array([w for _, w in E.BF16_EDGES], np.uint16)
    got = em.to_bf16_bits(bits.view(f32))
    assert np.array_equal(got, want), [hex(x) for x in got]
    plain = ((bits.astype(np.uint64) + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(bits.view(f32))
    assert np.array_equal(plain[~nan], want[~nan]) and (plain[nan] != want[nan]).sum() >= 3    # payloads the formula loses
    assert np.isnan(em.from_bf16_bits(got[nan])).all()
    x = np.random.default_rng(0).normal(size=4096).astype(f32)                                  # nearest: within half a step
    back = em.from_bf16_bits(em.to_bf16_bits(x)).astype(np.float64)
    assert (np.abs(back - x) <= np.abs(x.astype(np.float64)) * 2.0 ** -8).all()


def test_tree_sum_rows_is_orc_sum_past_64_segments(oracle):
    from oracle import em
    rng = np.random.default_rng(0)
    for d in (16384, 16385, 16640, 16897):
        x = rng.normal(size=(3, d)).astype(f32)
        want = np.array([oracle.tree_sum(r) for r in x], f32)
        assert np.array_equal(em.tree_sum_rows(x).view(np.uint32), want.view(np.uint32)), d


# ---- the oracle against float64 on every case -----------------------------------------------------------------------------------
def _f64_terms(mode, target, base, s):
    """norm.logpdf(target; base + drift * dt, sd) per element in float64, from the float32 inputs."""
    base, s = base.astype(np.float64), s.astype(np.float64)
    drift = s if mode == 1 else float(E.CX) * base + float(E.CS) * s
    m = base + drift * float(E.DT)
    sd = float(E.SD)
    return -0.5 * (math.log(2.0 * math.pi * sd * sd) + ((target.astype(np.float64) - m) / sd) ** 2)


def _ratio(lw, terms):
    """|float32 tree sum - float64 sum| per row over its allowance (ceil(log2 d) + 8) 2^-24 sum |term|: the pairwise-sum
    bound plus the handful of roundings per term."""
    d = terms.shape[1]
    allow = (math.ceil(math.log2(d)) + 8 if d > 1 else 8) * 2.0 ** -24 * np.abs(terms).sum(axis=1)
    return np.abs(lw.astype(np.float64) - terms.sum(axis=1)) / allow


WORST = {}


@pytest.mark.parametrize("case", [c for c in E.FINISH_CASES if c.want_lw and c.dv], ids=lambda c: c.id)
def test_oracle_weights_stay_inside_the_float64_bound(case, oracle):
    for dtype in case.dtypes:
        for mode in case.modes:
            x = E.finish_inputs(case.id, dtype, mode)
            net = x.net[x.net_A] if x.net_A is not None else x.net[:case.n]
            v_off = x.tables[1]
            terms = _f64_terms(mode, x.vv[1][None, :], np.broadcast_to(x.vv[0][None, :], (case.n, case.dv)), net[:, v_off])
            r = _ratio(x.want_lw, terms)
            WORST["lw"] = max(WORST.get("lw", 0.0), float(r.max()))
            assert r.max() <= 1.0, (case.id, dtype, mode, float(r.max()))
            if case.want_us and case.n * case.du <= 1 << 20:
                u_off = x.tables[0]
                src = (x.us[x.A] if x.A is not None else x.us[:case.n]).astype(np.float64)
                s = net[:, u_off].astype(np.float64)
                drift = s if mode == 1 else float(E.CX) * src + float(E.CS) * s
                want = src + drift * float(E.DT) + float(E.SD) * x.z.astype(np.float64)
                if case.pin is not None:
                    want[case.pin] = x.pin_val
                assert np.allclose(x.want_us, want, rtol=1e-5, atol=1e-6), (case.id, dtype, mode)


@pytest.mark.parametrize("case", E.TRANS_CASES, ids=lambda c: c.id)
def test_oracle_transition_logpdf_stays_inside_the_float64_bound(case, oracle):
    for dtype in case.dtypes:
        for mode in case.modes:
            x = E.trans_inputs(case.id, dtype, mode)
            terms = _f64_terms(mode, x.uu[1][None, :], x.us[:case.n], x.net[:case.n][:, x.tables[0]])
            r = _ratio(x.want, terms)
            WORST["tl"] = max(WORST.get("tl", 0.0), float(r.max()))
            assert r.max() <= 1.0, (case.id, dtype, mode, float(r.max()))


def test_report_the_worst_ratio_to_the_bound():
    """Printed with -s; DESIGN.md quotes it."""
    print("worst |float32 oracle - float64| / bound:", WORST)
