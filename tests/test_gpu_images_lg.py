"""The image tier against the analytic linear-Gaussian model (tests/lg_image_model.py).

With a Gaussian prior on the image the score is linear, and ``ScoreBridge`` runs the discretised model of
``LinearGaussianBridge`` up to the permutation of a mask.  Part 2 compares every step function of the image tier with
``lg_tables`` of the permuted prior in float64, to a first-order rounding bound computed next to the reference
(|got - ref| <= 2 bound), and the analytic tier's closures with the same reference.  Part 3 compares the lockstep samplers
with exact (Kalman) and reference (analytic-tier chains) distributions at 5 sqrt(2) standard errors, the standard errors
taken from the reference side only.  The tests without the ``gpu`` mark check the helper itself and need no GPU.

Measured ratios are printed by every test (run with -s) and recorded in DESIGN.md, section 4.12.
"""
import math

import numpy as np
import pytest
import torch

from lg_image_model import (LGImageModel, StepRef, U32, bootstrap_filter_np, inpaint_mask, kalman_filter, log_mean_exp,
                            log_mean_exp_se, perm, prior, ssm_of)

gpu = pytest.mark.gpu

T2 = 6                                   # steps of the per-step comparison
STEPS = (0, 3, T2 - 1)
NS = (1, 5, 65)
B2 = 3                                   # ensembles of the batched step functions, one mask each
CASES = {
    "a": ("inpaint-3", (8, 8, 1)),       # du = 9, dv = 55
    "b": ("supr-2", (6, 6, 3)),          # three channels, a random mask per ensemble
    "c": ("inpaint-17", (20, 20, 1)),    # du = 289 > 256: the second trip of the p += kBlock loops
    "d": ("inpaint-2", (20, 20, 3)),     # dv = 1188 > 1024: the second round of the log-weight loop, the LDS segment tree
    "e": ("inpaint-3", (7, 9, 2)),       # not square, odd sides, two channels (ImageRestore accepts it)
}
SIGMA = 5 * math.sqrt(2)


# ---------------------------------------------------------------------------------------------------
# without a GPU: the helper
# ---------------------------------------------------------------------------------------------------
def test_prior_is_built_to_show_layout_mistakes():
    w, h, c = 4, 5, 3
    m0, cov0 = prior((w, h, c))
    assert np.linalg.eigvalsh(cov0).min() > 0.04 and np.ptp(m0) > 0.5
    at = lambda r, col, ch: (r * h + col) * c + ch
    assert abs(cov0[at(0, 0, 0), at(1, 0, 0)] - cov0[at(0, 0, 0), at(0, 1, 0)]) > 0.05      # rows and columns differ
    offd = [cov0[at(0, 0, i), at(0, 0, j)] for i in range(c) for j in range(i)]
    assert len({round(x, 6) for x in offd}) == len(offd)                                    # distinct channel couplings
    model = LGImageModel((w, h, c), np.linspace(0, 2.0, 4))
    mask = inpaint_mask((w, h, c), 2, 1)
    p = perm(mask, c)
    du = model.du_of(mask)
    assert np.abs(cov0[np.ix_(p[:du], p[du:])]).max() > 0.1                                 # the posterior depends on y
    # the score function is -(F^2 cov0 + Q I)^{-1} (x - F m0), and the tables' drift is cx x + cs score in the mask's order
    from fbs_amd.sdes.linear import discretise_linear_sde_np
    x = torch.from_numpy(np.random.default_rng(0).normal(size=(3, w, h, c)).astype(np.float32))
    tab = model.tables(mask)
    for k in (0, 2):
        tf = 2.0 - model.ts[k]
        F, Q = discretise_linear_sde_np(model.sde, tf, 0.0)
        want = -np.linalg.solve(F ** 2 * cov0 + Q * np.eye(cov0.shape[0]), (x.numpy().reshape(3, -1).astype(np.float64) - F * m0).T).T
        got = model.score_fn()(x, tf).numpy().reshape(3, -1)
        np.testing.assert_allclose(got, want.astype(np.float32), rtol=2e-6, atol=1e-7)
        cx, cs = model.coef(k)
        z = x.numpy().reshape(3, -1).astype(np.float64)[:, p]
        np.testing.assert_allclose(z @ tab["G"][k].T + tab["g"][k], cx * z + cs * want[:, p], rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("shape,hole,shift", [((8, 8, 1), 3, 2), ((5, 9, 2), 3, 1), ((6, 6, 3), 2, 0)])
def test_perm_is_the_order_of_unpack(shape, hole, shift):
    """``ImageRestore.unpack`` and ``concat`` run on the CPU (only the mask's random draw needs the GPU), so does this."""
    from fbs_amd.images import ImageRestore
    ds = ImageRestore(f"inpaint-{hole}", shape, device="cpu")
    mask = inpaint_mask(shape, hole, shift)
    img = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape)
    x, y = ds.unpack(img, mask)
    p = perm(mask, shape[2])
    assert sorted(p.tolist()) == list(range(img.numel()))
    assert np.array_equal(torch.cat([x.reshape(-1), y.reshape(-1)]).numpy(), img.reshape(-1).numpy()[p])
    assert torch.equal(ds.concat(x.unsqueeze(0), y, mask)[0], img)


def test_kalman_filter_is_joint_gaussian_conditioning():
    """Three steps: the filter's mean, covariance and log-likelihood against conditioning the joint Gaussian of
    (u_3, v_1, v_2, v_3) built from the same recursion as one linear map of independent standard normals."""
    shape = (4, 4, 1)
    model = LGImageModel(shape, np.linspace(0, 2.0, 4))
    tab = model.tables(inpaint_mask(shape, 2, 1))
    du, dv = tab["du"], tab["dv"]
    rng = np.random.default_rng(3)
    vs = rng.normal(size=(4, dv))
    ne = du + 3 * (du + dv)                               # u_0, then (zeta_k, eta_k) per step
    Mu, cu = np.zeros((du, ne)), np.zeros(du)
    Mu[:, :du] = np.eye(du)
    Mv, cv = [], []
    for k, (A, b, H, d, sd) in enumerate(ssm_of(tab, vs)):
        o = du + k * (du + dv)
        Mk = H @ Mu
        Mk[:, o + du:o + du + dv] = sd * np.eye(dv)
        Mv.append(Mk)
        cv.append(H @ cu + d)
        Mu, cu = A @ Mu, A @ cu + b
        Mu[:, o:o + du] = sd * np.eye(du)
    Mv, cv, obs = np.concatenate(Mv, 0), np.concatenate(cv), vs[1:].reshape(-1)
    Svv, Suv = Mv @ Mv.T, Mu @ Mv.T
    e = obs - cv
    want_m = cu + Suv @ np.linalg.solve(Svv, e)
    want_P = Mu @ Mu.T - Suv @ np.linalg.solve(Svv, Suv.T)
    want_ll = -0.5 * (e @ np.linalg.solve(Svv, e) + np.linalg.slogdet(Svv)[1] + e.size * math.log(2 * math.pi))
    m, P, ll = kalman_filter(tab, vs)
    np.testing.assert_allclose(m, want_m, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(P, want_P, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(ll, want_ll, rtol=1e-11)


# ---------------------------------------------------------------------------------------------------
# the sampler-level model, and its reference filter (no GPU)
# ---------------------------------------------------------------------------------------------------
S_SHAPE, S_HOLE, S_T = (5, 5, 1), 2, 8   # du = 4, dv = 21: smaller than inpaint-3 on (8, 8, 1), and u and v still couple
S_B, S_NF = 64, 256                      # ensembles, particles of the filters
S_MREF = 1024                            # replicates of the reference filter
_sampler_cache = {}


def _sampler_model(shift):
    """The model, y0 (observed part of a draw from the prior) and an observation path vs (reverse time) made by exact
    forward noising of y0, all on the host and from fixed seeds; float32 values, as the GPU gets them."""
    if shift not in _sampler_cache:
        from fbs_amd.sdes.linear import discretise_linear_sde_np
        ts = np.linspace(0, 2.0, S_T + 1)
        model = LGImageModel(S_SHAPE, ts)
        mask = inpaint_mask(S_SHAPE, S_HOLE, shift)
        tab = model.tables(mask)
        rng = np.random.default_rng(11)
        img = model.m0 + np.linalg.cholesky(model.cov0) @ rng.standard_normal(model.D)
        y0 = img[perm(mask, S_SHAPE[2])][tab["du"]:].astype(np.float32)
        ys = [y0.astype(np.float64)]
        for k in range(S_T):
            F, Q = discretise_linear_sde_np(model.sde, ts[k + 1], ts[k])
            ys.append(F * ys[-1] + math.sqrt(Q) * rng.standard_normal(y0.size))
        vs = np.stack(ys[::-1], 0).astype(np.float32)
        _sampler_cache[shift] = dict(model=model, mask=mask, tab=tab, y0=y0, vs=vs, ts=ts, ref={})
    return _sampler_cache[shift]


def _reference_filter(sm, kind):
    """(Kalman mean, Kalman log-likelihood, SE of the mean over S_B ensembles, SE of log mean exp over S_B ensembles,
    the replicates): the exact answer, and the spread of S_MREF replicates of the float64 numpy bootstrap filter."""
    if kind not in sm["ref"]:
        m, _, ll = kalman_filter(sm["tab"], sm["vs"])
        pm, pl = bootstrap_filter_np(sm["tab"], sm["vs"], 5, S_MREF, S_NF, kind)
        sm["ref"][kind] = (m, ll, pm.std(0, ddof=1) / math.sqrt(S_B), log_mean_exp_se(pl, S_B), pm, pl)
    return sm["ref"][kind]


MASK_SEED = 200                          # the key of the sampler-level mask; its shift is a draw of randint(key, (), 0, 3)


@pytest.mark.parametrize("kind", ("stratified", "systematic"))
def test_reference_filter_alone_passes(kind, oracle):
    """The reference replicates, averaged in groups of S_B as the GPU test averages its ensembles, agree with the Kalman
    filter within the GPU test's threshold, and their two disjoint halves agree with each other."""
    sm = _sampler_model(int(oracle.randint(oracle.PRNGKey(MASK_SEED), (), 0, S_SHAPE[0] - S_HOLE)))
    m, ll, se_m, se_ll, pm, pl = _reference_filter(sm, kind)
    worst_m = worst_ll = 0.0
    for g in range(S_MREF // S_B):
        grp = slice(g * S_B, (g + 1) * S_B)
        worst_m = max(worst_m, (np.abs(pm[grp].mean(0) - m) / se_m).max())
        worst_ll = max(worst_ll, abs(log_mean_exp(pl[grp]) - ll) / se_ll)
    print(f"\n[lg-image] reference filter {kind}: {S_MREF // S_B} groups, largest |difference| / SE  mean={worst_m:.2f}  "
          f"loglik={worst_ll:.2f}  std of the log-likelihood estimates {pl.std():.3f}")
    assert worst_m <= SIGMA and worst_ll <= SIGMA
    h1, h2 = pm[:S_MREF // 2], pm[S_MREF // 2:]
    se_half = pm.std(0, ddof=1) / math.sqrt(S_MREF // 2)
    assert (np.abs(h1.mean(0) - h2.mean(0)) <= SIGMA * se_half).all()
    l1, l2 = pl[:S_MREF // 2], pl[S_MREF // 2:]
    assert abs(log_mean_exp(l1) - log_mean_exp(l2)) <= SIGMA * log_mean_exp_se(pl, S_MREF // 2)


# ---------------------------------------------------------------------------------------------------
# part 2: every step function against float64
# ---------------------------------------------------------------------------------------------------
_case_cache = {}


def _distinct_masks(ds, oracle):
    """B2 different masks of the task: the draws of keys 200, 201, ... that differ from those before them."""
    masks, seen = [], set()
    for seed in range(200, 240):
        m = ds.gen_mask(oracle.PRNGKey(seed))
        ident = tuple(m.unobs_inds_ravelled.tolist())
        if ident not in seen:
            seen.add(ident)
            masks.append(m)
        if len(masks) == B2:
            return masks
    raise AssertionError("fewer than B2 different masks in forty draws")


def _case(name, dev, oracle, bf16=False):
    key = (name, bf16)
    if key not in _case_cache:
        from fbs_amd.images import ImageRestore
        from fbs_amd.score import ScoreBridge
        task, shape = CASES[name]
        ts = np.linspace(0, 2.0, T2 + 1)
        base = _case_cache.get((name, not bf16))
        model = base["model"] if base else LGImageModel(shape, ts)
        ds = ImageRestore(task, shape, device=dev)
        masks = base["masks"] if base else _distinct_masks(ds, oracle)
        sb = ScoreBridge(model.score_fn(torch.bfloat16 if bf16 else torch.float32), ds, model.sde, ts, chunk=4096)
        br = base["br"] if base else model.bridge(masks[0], dev)
        tabs = base["tabs"] if base else [br.tables64] + [model.tables(m) for m in masks[1:]]
        _case_cache[key] = dict(model=model, ds=ds, masks=masks, sb=sb, br=br, tabs=tabs, ts=ts, shape=shape,
                                du=tabs[0]["du"], dv=tabs[0]["dv"], bf16=bf16)
    return _case_cache[key]


class Ratios:
    """Largest |got - ref| / bound per quantity; ``check`` asserts |got - ref| <= 2 bound elementwise (a zero bound, the
    pinned row, asks for equality)."""

    def __init__(self, case):
        self.case, self.r = case, {}

    def check(self, what, got, ref, bound, ctx=()):
        got = got.detach().cpu().numpy().astype(np.float64).reshape(np.shape(ref))
        err = np.abs(got - ref)
        assert np.isfinite(got).all(), (what, ctx)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        self.r[what] = max(self.r.get(what, 0.0), float(ratio.max()))
        assert (err <= 2 * bound).all(), (self.case, what, ctx, "largest error / bound", float(ratio.max()))

    def report(self, title):
        print(f"\n[lg-image] case {self.case} {title}: largest error / bound  " +
              "  ".join(f"{k}={v:.3f}" for k, v in self.r.items()))


def _inputs(c, n, k, nens=1):
    """us (nens, n, du), v_prev, v (nens, dv) float32: particles around the prior mean, a plausible observation step."""
    rng = np.random.default_rng(1000 * n + 10 * k + nens)
    du, dv = c["du"], c["dv"]
    us = (0.3 + 0.8 * rng.standard_normal((nens, n, du))).astype(np.float32)
    v_prev = (0.2 + 0.7 * rng.standard_normal((nens, dv))).astype(np.float32)
    v = (v_prev + 0.3 * rng.standard_normal((nens, dv))).astype(np.float32)
    return us, v_prev, v


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _step_ref(c, b, k, U, v_prev):
    return StepRef(c["tabs"][b], k, *c["model"].coef(k), U, v_prev, bf16=c["bf16"])


def _closures_against_float64(c, name, dev, oracle, ns=NS, cross_tier=True):
    sb, br, mask, ts = c["sb"], c["br"], c["masks"][0], c["ts"]
    du, dv, ch = c["du"], c["dv"], c["shape"][2]
    img, lg = Ratios(name), Ratios(name)
    for n in ns:
        for k in STEPS:
            us, v_prev, v = _inputs(c, n, k)
            us, v_prev, v = us[0], v_prev[0], v[0]
            key = oracle.PRNGKey(7000 + 10 * n + k)
            u_tgt = (us[0] + 0.2 * np.random.default_rng(k).standard_normal(du)).astype(np.float32)   # one target (p, c)
            R = _step_ref(c, 0, k, us, v_prev)
            zeta = oracle.normal(key, (n, du))
            p_ref, p_bd = R.proposal(zeta)
            l_ref, l_bd = R.logpdf(v, "v")
            t_ref, t_bd = R.logpdf(u_tgt, "u")
            us_t, vp_t, v_t = _t(us, dev).reshape(n, -1, ch), _t(v_prev, dev).reshape(-1, ch), _t(v, dev).reshape(-1, ch)
            ut_t = _t(u_tgt, dev).reshape(-1, ch)
            ctx = (n, k)
            img.check("transition_sampler", sb.transition_sampler(us_t, vp_t, ts[k], key, mask), p_ref, p_bd, ctx)
            img.check("likelihood_logpdf", sb.likelihood_logpdf(v_t, us_t, vp_t, ts[k], mask), l_ref, l_bd, ctx)
            img.check("transition_logpdf", sb.transition_logpdf(ut_t, us_t, vp_t, ts[k], mask), t_ref, t_bd, ctx)
            if cross_tier:      # the analytic tier on the same inputs: the same reference, its own dot product's rounding added
                u2, vp1 = _t(us, dev), _t(v_prev, dev)
                lg.check("transition_sampler", br.transition_sampler(u2, vp1, ts[k], key), p_ref, p_bd + R.lg_proposal_extra(), ctx)
                lg.check("likelihood_logpdf", br.likelihood_logpdf(_t(v, dev), u2, vp1, ts[k]), *R.logpdf(v, "v", tree=False), ctx)
                lg.check("transition_logpdf", br.transition_logpdf(_t(u_tgt, dev), u2, vp1, ts[k]), *R.logpdf(u_tgt, "u", tree=False), ctx)
    img.report("ScoreBridge closures" + (" (bf16 score)" if c["bf16"] else ""))
    if cross_tier:
        lg.report("LinearGaussianBridge closures")


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_closures_against_float64(name, dev, oracle):
    """``ScoreBridge.transition_sampler``, ``likelihood_logpdf`` and ``transition_logpdf`` against G z + g of ``lg_tables``,
    and the ``LinearGaussianBridge`` closures on the same inputs against the same reference: the two tiers state one model.
    The analytic tier's bound adds the rounding of its own float32 dot product over D terms (``StepRef.lg_dot``) and sums the
    terms in index order; nothing else differs."""
    _closures_against_float64(_case(name, dev, oracle), name, dev, oracle)


def _fused_steps_against_float64(c, name, dev, oracle, ns=NS):
    sb, mask, ts = c["sb"], c["masks"][0], c["ts"]
    du, ch = c["du"], c["shape"][2]
    rt = Ratios(name)
    for n in ns:
        for k in STEPS:
            us, v_prev, v = _inputs(c, n, k)
            us, v_prev, v = us[0], v_prev[0], v[0]
            rng = np.random.default_rng(n + k)
            A = rng.integers(0, n, n).astype(np.int32)
            pin_row, pin_val = int(rng.integers(0, n)), rng.standard_normal(du).astype(np.float32)
            key = oracle.PRNGKey(8000 + 10 * n + k)
            zeta = oracle.normal(key, (n, du))
            us_t, vp_t, v_t = _t(us, dev).reshape(n, -1, ch), _t(v_prev, dev).reshape(-1, ch), _t(v, dev).reshape(-1, ch)
            # fused_step: gather by A, propose, pin, weigh the gathered particles
            R = _step_ref(c, 0, k, us[A], v_prev)
            p_ref, p_bd = R.proposal(zeta)
            p_ref[pin_row], p_bd[pin_row] = pin_val, 0.0
            got_us, got_lw = sb.fused_step(us_t, _t(A, dev), v_t, vp_t, ts[k], key, mask,
                                           pin=(pin_row, _t(pin_val, dev).reshape(-1, ch)))
            rt.check("fused_step.us", got_us, p_ref, p_bd, (n, k))
            rt.check("fused_step.lw", got_lw, *R.logpdf(v, "v"), (n, k))
            # fused_weight_then_propose: weigh the particles as they are, then propose from row inds[r] with noise row r
            inds = ((np.arange(n) * 7 + 3) % n)[::-1].astype(np.int32).copy()
            got_us, got_lw, got_inds = sb.fused_weight_then_propose(us_t, v_t, vp_t, ts[k], key, mask, lambda lw: _t(inds, dev))
            assert np.array_equal(got_inds.cpu().numpy(), inds)
            rt.check("weight_then_propose.lw", got_lw, *_step_ref(c, 0, k, us, v_prev).logpdf(v, "v"), (n, k))
            rt.check("weight_then_propose.us", got_us, *_step_ref(c, 0, k, us[inds], v_prev).proposal(zeta), (n, k))
    rt.report("fused_step, fused_weight_then_propose")


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_steps_against_float64(name, dev, oracle):
    _fused_steps_against_float64(_case(name, dev, oracle), name, dev, oracle)


def _batched_steps_against_float64(c, name, dev, oracle, ns=NS):
    sb, masks, ts = c["sb"], c["masks"], c["ts"]
    du, dv, ch = c["du"], c["dv"], c["shape"][2]
    rt = Ratios(name)
    for n in ns:
        for k in STEPS:
            us, v_prev, v = _inputs(c, n, k, B2)
            rng = np.random.default_rng(3 * n + k)
            A = rng.integers(0, n, (B2, n)).astype(np.int32)
            pin_rows = np.array([0, n - 1, -1], np.int32)
            pin_vals = rng.standard_normal((B2, du)).astype(np.float32)
            keys = oracle.split(oracle.PRNGKey(9000 + 10 * n + k), B2)
            inds = np.stack([((np.arange(n) * (5 + 2 * b) + 1 + b) % n)[::-1] for b in range(B2)], 0).astype(np.int32)
            us_t = _t(us, dev).reshape(B2, n, -1, ch)
            vp_t, v_t = _t(v_prev, dev).reshape(B2, -1, ch), _t(v, dev).reshape(B2, -1, ch)
            got_us, got_lw = sb.fused_step_batched(us_t, _t(A, dev), v_t, vp_t, ts[k], keys, masks,
                                                   pins=(_t(pin_rows, dev), _t(pin_vals, dev).reshape(B2, -1, ch)))
            w_us, w_lw, w_inds = sb.fused_weight_then_propose_batched(us_t, v_t, vp_t, ts[k], keys, masks,
                                                                      lambda lw: _t(inds, dev))
            assert np.array_equal(w_inds.cpu().numpy(), inds)
            for b in range(B2):
                zeta = oracle.normal(keys[b], (n, du))
                R = _step_ref(c, b, k, us[b][A[b]], v_prev[b])
                p_ref, p_bd = R.proposal(zeta)
                if pin_rows[b] >= 0:
                    p_ref[pin_rows[b]], p_bd[pin_rows[b]] = pin_vals[b], 0.0
                rt.check("fused_step_batched.us", got_us[b], p_ref, p_bd, (n, k, b))
                rt.check("fused_step_batched.lw", got_lw[b], *R.logpdf(v[b], "v"), (n, k, b))
                rt.check("weight_then_propose_batched.lw", w_lw[b], *_step_ref(c, b, k, us[b], v_prev[b]).logpdf(v[b], "v"),
                         (n, k, b))
                # a non-identity resampling: row r reads particle AND network row inds[b][r] (net_by_A), noise row r
                rt.check("weight_then_propose_batched.us", w_us[b],
                         *_step_ref(c, b, k, us[b][inds[b]], v_prev[b]).proposal(zeta), (n, k, b))
    rt.report("fused_step_batched, fused_weight_then_propose_batched")


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_batched_steps_against_float64(name, dev, oracle):
    """One mask per ensemble (three shifts of the hole, or three random super-resolution masks), random ancestors, pins on
    the first row, the last row and none."""
    c = _case(name, dev, oracle)
    assert len({tuple(m.unobs_inds_ravelled.tolist()) for m in c["masks"]}) > 1, "the masks of the batch must differ"
    _batched_steps_against_float64(c, name, dev, oracle)


@gpu
def test_bf16_score_against_float64(dev, oracle):
    """Case b with a score returned in bfloat16: the reference drift is rebuilt from the float64 score rounded to float32
    and to bfloat16 (``oracle.em.to_bf16_bits``); the bounds are unchanged, the kernels widen bfloat16 exactly."""
    c = _case("b", dev, oracle, bf16=True)
    _closures_against_float64(c, "b/bf16", dev, oracle, ns=(5, 65), cross_tier=False)
    _fused_steps_against_float64(c, "b/bf16", dev, oracle, ns=(5,))
    _batched_steps_against_float64(c, "b/bf16", dev, oracle, ns=(5, 65))


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_samplers_are_the_analytic_tiers(name, dev, oracle):
    """``fwd_ys_sampler`` is the analytic tier's on the same key, bit for bit.  ``fwd_sampler`` draws its noise in image
    order, the analytic tier in the mask's order, and the SDE is scalar: so the image path equals the analytic tier's own
    ``fwd_sampler`` on the same key started at the image in image order; and its unpacked parts follow the float64 recursion
    path[k + 1] = F[k] path[k] + sqQ[k] xi[k] of ``lg_tables`` (three roundings per step and the rounded tables: 5 u per
    step on |F x| + |sqQ xi|, carried forward)."""
    c = _case(name, dev, oracle)
    sb, br, ds, mask, tab = c["sb"], c["br"], c["ds"], c["masks"][0], c["tabs"][0]
    du, dv, ch = c["du"], c["dv"], c["shape"][2]
    D = du + dv
    rng = np.random.default_rng(17)
    x0 = _t(rng.standard_normal(du).astype(np.float32), dev).reshape(-1, ch)
    y0 = _t(rng.standard_normal(dv).astype(np.float32), dev).reshape(-1, ch)
    key = oracle.PRNGKey(77)
    assert torch.equal(sb.fwd_ys_sampler(key, y0).reshape(T2 + 1, dv), br.fwd_ys_sampler(key, y0.reshape(-1)))
    path = sb.fwd_sampler(key, x0, y0, mask)
    assert tuple(path.shape) == (T2 + 1,) + c["shape"]
    img0 = ds.concat(x0.unsqueeze(0), y0, mask)[0].reshape(-1)
    assert torch.equal(path.reshape(T2 + 1, D), br.fwd_sampler(key, img0[:du], img0[du:]))
    xi = oracle.normal(key, (T2, D)).astype(np.float64)
    ref, bound = img0.cpu().numpy().astype(np.float64), np.zeros(D)
    p = perm(mask, ch)
    px, py = ds.unpack(path, mask)
    got = torch.cat([px.reshape(T2 + 1, du), py.reshape(T2 + 1, dv)], 1).cpu().numpy().astype(np.float64)
    for k in range(T2):
        a, b = tab["F"][k] * ref, tab["sqQ"][k] * xi[k]
        ref, bound = a + b, tab["F"][k] * bound + 5 * U32 * (np.abs(a) + np.abs(b))
        assert (np.abs(got[k + 1] - ref[p]) <= 2 * bound[p]).all(), k


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_perm_is_the_order_of_unpack_and_of_the_mask_tables(name, dev, oracle):
    c = _case(name, dev, oracle)
    ch = c["shape"][2]
    for mask in c["masks"]:
        img = torch.arange(int(np.prod(c["shape"])), dtype=torch.float32, device=dev).reshape(c["shape"])
        x, y = c["ds"].unpack(img, mask)
        p = perm(mask, ch)
        assert np.array_equal(torch.cat([x.reshape(-1), y.reshape(-1)]).cpu().numpy(), img.reshape(-1).cpu().numpy()[p])
        em = c["sb"]._em_mask(mask)
        assert np.array_equal(torch.cat([em.u_off, em.v_off]).cpu().numpy(), p)


# ---------------------------------------------------------------------------------------------------
# part 3: the lockstep samplers against exact and reference distributions
# ---------------------------------------------------------------------------------------------------
def _sampler_setup(dev, oracle):
    """The image tier and the analytic tier on the sampler-level model; the mask is ``ImageRestore``'s own."""
    from fbs_amd.images import ImageRestore
    from fbs_amd.score import ScoreBridge
    ds = ImageRestore(f"inpaint-{S_HOLE}", S_SHAPE, device=dev)
    mask = ds.gen_mask(oracle.PRNGKey(MASK_SEED))
    sm = _sampler_model(int(mask.shift))
    assert np.array_equal(perm(mask, 1), perm(sm["mask"], 1))
    if "gpu" not in sm:
        sb = ScoreBridge(sm["model"].score_fn(), ds, sm["model"].sde, sm["ts"], chunk=1 << 15)
        sm["gpu"] = dict(ds=ds, mask=mask, sb=sb, br=sm["model"].bridge(mask, dev), y0=_t(sm["y0"], dev).reshape(-1, 1),
                         vs=_t(sm["vs"], dev).reshape(S_T + 1, -1, 1))
    return sm, sm["gpu"]


def _report(title, **ratios):
    print(f"\n[lg-image] {title}: largest |difference| / SE  " + "  ".join(f"{k}={v:.2f}" for k, v in ratios.items()))


@gpu
@pytest.mark.parametrize("kind", ("stratified", "systematic"))
def test_bootstrap_filter_batched_against_kalman(kind, dev, oracle):
    """64 ensembles of 256 particles on one observation path: the mean of the final particles against the exact filtering
    mean, and log mean_b exp(-nell_b) against the exact log-likelihood log p(vs[1:] | vs[0]) -- ``-nell`` is the logarithm of
    the filter's unbiased estimate of that likelihood (sum over the steps of logsumexp(lw) - log n).  The standard errors
    are the spread of 1024 replicates of a float64 numpy bootstrap filter of the same model, over sqrt(64)."""
    from fbs_amd import samplers
    sm, g = _sampler_setup(dev, oracle)
    m, ll, se_m, se_ll, _, _ = _reference_filter(sm, kind)
    sb = g["sb"]
    vss = g["vs"].unsqueeze(0).expand(S_B, -1, -1, -1).contiguous()
    keys = oracle.split(oracle.PRNGKey(901), S_B)
    us, nell = samplers.bootstrap_filter_batched(sb.transition_sampler, sb.likelihood_logpdf, vss, sm["ts"], sb.ref_sampler,
                                                 keys, S_NF, getattr(samplers, kind), mask_=g["mask"])
    assert tuple(us.shape) == (S_B, S_NF, sm["tab"]["du"], 1)
    d_m = np.abs(us.double().mean((0, 1)).reshape(-1).cpu().numpy() - m) / se_m
    d_ll = abs(log_mean_exp(-nell.double().cpu().numpy()) - ll) / se_ll
    _report(f"bootstrap_filter_batched {kind}", mean=d_m.max(), loglik=d_ll)
    assert (d_m <= SIGMA).all() and d_ll <= SIGMA, (d_m, d_ll)


@gpu
@pytest.mark.parametrize("kind", ("stratified", "systematic"))
def test_pmcmc_filter_step_batched_log_ell_against_kalman(kind, dev, oracle):
    """``log_ell`` of the weigh-resample-propose filter is the same estimate of log p(vs[1:] | vs[0])."""
    from fbs_amd import samplers
    sm, g = _sampler_setup(dev, oracle)
    _, ll, _, se_ll, _, _ = _reference_filter(sm, kind)
    sb = g["sb"]
    vss = g["vs"].unsqueeze(0).expand(S_B, -1, -1, -1).contiguous()
    u0s = torch.stack([sb.ref_sampler(oracle.PRNGKey(500 + b), None, S_NF) for b in range(S_B)], 0)
    keys = oracle.split(oracle.PRNGKey(902), S_B)
    us, log_ell = samplers.pmcmc_filter_step_batched(keys, vss, u0s, sm["ts"], sb.transition_sampler, sb.likelihood_logpdf,
                                                     getattr(samplers, kind), S_NF, mask_=g["mask"])
    d_ll = abs(log_mean_exp(log_ell.double().cpu().numpy()) - ll) / se_ll
    _report(f"pmcmc_filter_step_batched {kind}", loglik=d_ll)
    assert torch.isfinite(us).all() and d_ll <= SIGMA, d_ll


G_N, G_BURN, G_KEEP = 16, 20, 100        # particles, sweeps dropped and kept per chain
G_REF_SEED = 31                          # the key of the reference chains


def _halves_of_reference(ref):
    """ref (sweeps, chains, du): largest |difference| / SE between the two halves of the reference chains, for the mean and
    for the second moment about the pooled mean; the SE of a half against a half is that of all chains times sqrt(2)."""
    ref = np.asarray(ref, np.float64)
    C = ref.shape[1]
    centre = ref.mean((0, 1))
    out = {}
    for what, r_ in (("mean", ref.mean(0)), ("var", ((ref - centre) ** 2).mean(0))):
        se = r_.std(0, ddof=1) / math.sqrt(C)
        out[what + "_ref_halves"] = (np.abs(r_[:C // 2].mean(0) - r_[C // 2:].mean(0)) / (se * math.sqrt(2))).max()
    return out


@pytest.mark.parametrize("explicit_final", (False, True))
def test_reference_chains_alone_pass(explicit_final, oracle):
    """The chains the Gibbs GPU tests use as their reference, run by the C oracle on the CPU (the fused engine equals it bit
    for bit, test_gpu_lg.py) with the same key: their two halves agree within the GPU tests' threshold."""
    sm = _sampler_model(int(oracle.randint(oracle.PRNGKey(MASK_SEED), (), 0, S_SHAPE[0] - S_HOLE)))
    m, cov, du = sm["model"].permuted(sm["mask"])
    om = oracle.make_lg(m, cov, oracle.sde_lin(0.02, 5.0, 0.0, 2.0), sm["ts"], du)
    ref = oracle.gibbs_chains_lg(om, oracle.PRNGKey(G_REF_SEED), np.zeros((S_B, du), np.float32), sm["y0"],
                                 np.zeros((S_B, S_T + 1), np.int32), G_N, G_BURN + G_KEEP, True, explicit_final)[3]
    out = _halves_of_reference(ref[G_BURN:])
    _report(f"reference chains, explicit_final={explicit_final}", **out)
    assert max(out.values()) <= SIGMA, out
G_MARG_BURN, G_MARG_KEEP = 6, 12         # marg_y draws a 100-sub-step Doob bridge per chain and sweep on the host loop: fewer sweeps


def _moments_against_reference(title, got, ref):
    """got, ref (sweeps, chains, du): per-coordinate mean, and second moment about the reference's mean, of the image tier's
    chains against the reference chains'; the standard errors are the spread over the REFERENCE chains only.  The two
    halves of the reference chains must agree with each other within the same threshold."""
    got, ref = (np.asarray(a, np.float64) for a in (got, ref))
    C = ref.shape[1]
    assert got.shape == ref.shape
    centre = ref.mean((0, 1))
    stat = lambda x: (x.mean(0), ((x - centre) ** 2).mean(0))                      # per chain
    (gm, gv), (rm, rv) = stat(got), stat(ref)
    out = {}
    for what, g_, r_ in (("mean", gm, rm), ("var", gv, rv)):
        se = r_.std(0, ddof=1) / math.sqrt(C)
        out[what] = (np.abs(g_.mean(0) - r_.mean(0)) / se).max()
    out.update(_halves_of_reference(ref))
    _report(title, **out)
    assert out["mean_ref_halves"] <= SIGMA and out["var_ref_halves"] <= SIGMA, out
    assert out["mean"] <= SIGMA and out["var"] <= SIGMA, out


@gpu
@pytest.mark.parametrize("flags", ({"explicit_final": False}, {"explicit_final": True}, {"marg_y": True}),
                         ids=("eb", "eb-ef", "eb-marg_y"))
def test_gibbs_kernel_batched_against_the_analytic_chains(flags, dev, oracle):
    """64 chains of ``gibbs_kernel_batched`` against 64 chains of the fused analytic-tier sweep on the permuted model, the
    same particles, steps and flags: the law both target has no closed form, the analytic tier's chain is its reference
    sampler (bit-exact against the C oracle, and on the closed-form posterior in test_gpu_lg.py)."""
    from fbs_amd.samplers import gibbs_kernel_batched
    sm, g = _sampler_setup(dev, oracle)
    sb, br, du = g["sb"], g["br"], sm["tab"]["du"]
    ef, marg = flags.get("explicit_final", False), flags.get("marg_y", False)
    burn, keep = (G_MARG_BURN, G_MARG_KEEP) if marg else (G_BURN, G_KEEP)
    nsw = burn + keep
    h = br.sweep_handle(G_N, True, ef, nchains=S_B, marg_y=marg)
    _, _, _, ref = h.chain(oracle.PRNGKey(G_REF_SEED), np.zeros((S_B, du), np.float32), sm["y0"], np.zeros((S_B, S_T + 1), np.int32), nsw)
    key = oracle.PRNGKey(32)
    x0s, bs = torch.zeros((S_B, du, 1), device=dev), np.zeros((S_B, S_T + 1), np.int32)
    got = []
    for _ in range(nsw):
        key, sub = oracle.split(key)
        x0s, _, bsn, _ = gibbs_kernel_batched(oracle.split(sub, S_B), x0s, g["y0"], None, bs, sm["ts"], sb.fwd_sampler,
                                              sm["model"].sde, sb.unpack, G_N, sb.transition_sampler, sb.transition_logpdf,
                                              sb.likelihood_logpdf, marg_y=marg, explicit_backward=True, explicit_final=ef,
                                              mask_=g["mask"])
        bs = bsn.cpu().numpy()
        got.append(x0s.reshape(S_B, du))
    got = torch.stack(got, 0).cpu().numpy()
    _moments_against_reference(f"gibbs_kernel_batched {flags}", got[burn:], ref.cpu().numpy()[burn:])


P_N, P_BURN, P_KEEP = 64, 20, 100


@gpu
@pytest.mark.parametrize("delta", (None, 0.005))
def test_pmcmc_kernel_batched_against_the_analytic_chains(delta, dev, oracle):
    """64 chains of ``pmcmc_kernel_batched`` against 64 chains of the fused analytic-tier pMCMC engine.  Both draw their
    initial particles from the analytic tier's ``ref_sampler`` (p(u | v) at the terminal time; the image tier's own draws
    N(0, I), another target), start at the same observation paths and at log_ell = -1e30, so the first proposal is taken."""
    from fbs_amd.samplers import pmcmc_kernel_batched, stratified
    sm, g = _sampler_setup(dev, oracle)
    sb, br, du, dv = g["sb"], g["br"], sm["tab"]["du"], sm["tab"]["dv"]
    n = P_BURN + P_KEEP
    yss = torch.stack([sb.fwd_ys_sampler(oracle.PRNGKey(600 + b), g["y0"]) for b in range(S_B)], 0)
    ell0 = np.full(S_B, -1e30, np.float32)
    hp = br.pmcmc_handle(P_N, "stratified", nchains=S_B, delta=delta)
    out = hp.chain(oracle.PRNGKey(41), np.zeros((S_B, du), np.float32), ell0, yss.reshape(S_B, S_T + 1, dv), sm["y0"], n)
    ref, ref_acc = out[4].cpu().numpy(), out[5].is_accepted.cpu().numpy()

    def ref_sampler(key_, yT, nsamples):
        return br.ref_sampler(key_, yT.reshape(-1), nsamples).reshape(nsamples, du, 1)

    key = oracle.PRNGKey(42)
    uTs, ells = torch.zeros((S_B, du, 1), device=dev), _t(ell0, dev)
    got, acc = [], []
    for _ in range(n):
        key, sub = oracle.split(key)
        uTs, ells, yss, st = pmcmc_kernel_batched(oracle.split(sub, S_B), uTs, ells, yss, g["y0"], sm["ts"], sb.fwd_ys_sampler,
                                                  sm["model"].sde, ref_sampler, sb.transition_sampler, sb.likelihood_logpdf,
                                                  stratified, P_N, delta=delta, mask_=g["mask"])
        got.append(uTs.reshape(S_B, du))
        acc.append(st.is_accepted)
    got, acc = torch.stack(got, 0).cpu().numpy(), torch.stack(acc, 0).cpu().numpy()
    print(f"\n[lg-image] pmcmc delta={delta}: acceptance rate image tier {acc[1:].mean():.3f}, analytic tier {ref_acc[1:].mean():.3f}")
    assert acc[0].all(), "the first proposal replaces log_ell = -1e30"
    assert any(row.any() and not row.all() for row in acc[1:]), "no batch holds both accepted and rejected proposals"
    _moments_against_reference(f"pmcmc_kernel_batched delta={delta}", got[P_BURN:], ref[P_BURN:])
