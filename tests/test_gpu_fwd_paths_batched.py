"""GPU: the forward noising paths of B ensembles in lockstep.  ScoreBridge.fwd_sampler_batched / fwd_ys_sampler_batched
(fbsmi_linear_path_batched, fbsmi_em_fwd_step_batched) equal the loop of fwd_sampler / fwd_ys_sampler over the ensembles,
unpacked and flipped, bit for bit; the drift network is called ceil(B / chunk) times per step for all ensembles; the batched
samplers use them when handed the bridge's own closures, with unchanged results, and run the per-ensemble loop otherwise.
The drift and score functions are row-wise: a row's output does not depend on which rows share its call."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# D = 64; D = 147 (odd, so T * D is odd for odd T and the rows of b >= 1 are unaligned), c = 3; a scattered (strided) mask
SHAPES = {"inpaint-8x8x1": ("inpaint-3", (8, 8, 1)), "inpaint-7x7x3": ("inpaint-3", (7, 7, 3)), "supr-8x8x1": ("supr-2", (8, 8, 1))}


def _eq(got, want, what):
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got.detach().cpu().numpy(), want.detach().cpu().numpy(), err_msg=str(what))


def _model(dev, T, shape="inpaint-8x8x1", mode="score", chunk=2, rows=True, drift_dtype=torch.float32):
    """-> (dataset, bridge, sde, ts, score calls, forward-drift calls); each list records the rows of every call."""
    from fbs_amd.images import ImageRestore
    from fbs_amd.score import ScoreBridge
    from fbs_amd.sdes import StationaryLinLinearSDE
    task, image_shape = SHAPES[shape]
    ts = np.linspace(0, 2.0, T + 1)
    sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=2.0)
    ds = ImageRestore(task, image_shape, device=dev)
    calls, fwd_calls = [], []
    table = torch.from_numpy(np.random.default_rng(5).normal(size=image_shape).astype(np.float32)).to(dev)

    def score_fn(x, t):
        calls.append(int(x.shape[0]))
        return (0.25 * x.roll(1, 2) - 0.5 * x) * float(t)

    def drift(x, t):                                     # elementwise in x and t plus a fixed per-position table
        return ((table - 0.5 * x) * float(0.3 + t) + 0.125 * torch.tanh(x)).to(drift_dtype)

    def one_row(x, t):                                   # x (w, h, c), as euler_maruyama hands it over
        fwd_calls.append(1)
        return drift(x, t)

    def many_rows(x, t):                                 # x (rows, w, h, c)
        assert x.dtype == torch.float32 and tuple(x.shape[1:]) == tuple(image_shape)
        fwd_calls.append(int(x.shape[0]))
        return drift(x, t)

    kw = dict(mode="drift", fwd_drift_fn=one_row) if mode == "drift" else {}
    if mode == "drift" and rows:
        kw["fwd_drift_rows_fn"] = many_rows
    return ds, ScoreBridge(score_fn, ds, sde, ts, chunk=chunk, **kw), sde, ts, calls, fwd_calls


def _inputs(oracle, dev, ds, B, seed=0):
    from fbs_amd import ops
    keys = np.asarray(oracle.split(oracle.PRNGKey(31 + B + 100 * seed), B), np.uint32).reshape(B, 2)
    masks = [ds.gen_mask(oracle.PRNGKey(200 + b)) for b in range(B)]
    y0s = [ds.unpack(ops.uniform(oracle.PRNGKey(300 + b), ds.image_shape, device=dev), masks[b])[1] for b in range(B)]
    x0s = torch.from_numpy(np.random.default_rng(B).normal(size=(B,) + tuple(ds.unobs_shape)).astype(np.float32)).to(dev)
    return keys, x0s, y0s, masks


def _loop_paths(sb, keys, x0s, y0, mask):
    """flip(unpack(fwd_sampler)) per ensemble, stacked -> us (T + 1, B, p, c), vs (T + 1, B, q, c)."""
    parts = [sb.unpack(sb.fwd_sampler(keys[b], x0s[b], y0(b), mask_=mask(b)), mask(b)) for b in range(len(keys))]
    return tuple(torch.stack([torch.flip(p[i], [0]) for p in parts], 1) for i in range(2))


def _check_against_loop(sb, keys, x0s, y0s, masks):
    """Per-ensemble and shared masks, per-ensemble and shared y0, both layouts, with and without the observed half."""
    B = len(keys)
    for shared_mask in (False, True):
        for shared_y0 in (False, True):
            mask = (lambda b: masks[0]) if shared_mask else (lambda b: masks[b])
            y0 = (lambda b: y0s[0]) if shared_y0 else (lambda b: y0s[b])
            us, vs = _loop_paths(sb, keys, x0s, y0, mask)
            m_arg = masks[0] if shared_mask else masks
            y_arg = y0s[0] if shared_y0 else (torch.stack(y0s, 0) if shared_mask else y0s)     # a tensor (B, q, c), or a list
            what = (shared_mask, shared_y0)
            got = sb.fwd_sampler_batched(keys, x0s, y_arg, m_arg)
            _eq(got[0], us, ("us",) + what)
            _eq(got[1], vs, ("vs",) + what)
            got = sb.fwd_sampler_batched(keys, x0s, y_arg, m_arg, batch_major=True)
            assert got[0].is_contiguous() and got[1].is_contiguous()
            _eq(got[0], us.transpose(0, 1), ("us batch-major",) + what)
            _eq(got[1], vs.transpose(0, 1), ("vs batch-major",) + what)
            for bm in (False, True):
                got = sb.fwd_sampler_batched(keys, x0s, y_arg, m_arg, want_vs=False, batch_major=bm)
                assert got[1] is None
                _eq(got[0], us.transpose(0, 1) if bm else us, ("us alone", bm) + what)


@pytest.mark.parametrize("T", (1, 2, 5))
@pytest.mark.parametrize("B", (1, 3, 5))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_linear_kernel_equals_the_loop(oracle, dev, shape, B, T):
    ds, sb, sde, ts, _, _ = _model(dev, T, shape)
    keys, x0s, y0s, masks = _inputs(oracle, dev, ds, B)
    assert sb._em_mask(masks[0]).D == int(np.prod(ds.image_shape))
    _check_against_loop(sb, keys, x0s, y0s, masks)
    # the NULL-mask form: the observation alone, in forward order
    want = torch.stack([sb.fwd_ys_sampler(keys[b], y0s[b]) for b in range(B)], 0)
    _eq(sb.fwd_ys_sampler_batched(keys, y0s), want, "ys, one y0 per ensemble")
    _eq(sb.fwd_ys_sampler_batched(keys, torch.stack(y0s, 0)), want, "ys, y0s as one tensor")
    want = torch.stack([sb.fwd_ys_sampler(keys[b], y0s[0]) for b in range(B)], 0)
    _eq(sb.fwd_ys_sampler_batched(keys, y0s[0]), want, "ys, one shared y0")


@pytest.mark.parametrize("drift_dtype", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
@pytest.mark.parametrize("T", (1, 2, 5))
@pytest.mark.parametrize("B", (1, 3, 5))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_step_kernel_equals_the_loop(oracle, dev, shape, B, T, drift_dtype):
    ds, sb, sde, ts, _, fwd_calls = _model(dev, T, shape, mode="drift", drift_dtype=drift_dtype)
    keys, x0s, y0s, masks = _inputs(oracle, dev, ds, B)
    _check_against_loop(sb, keys, x0s, y0s, masks)
    assert all(r in (1, 2) for r in fwd_calls)           # the loop's one-row calls and the chunks of chunk = 2


def test_network_call_counts(oracle, dev):
    """chunk = 2 and B = 5: every step is calls of 2, 2 and 1 rows; T steps per set of paths."""
    T, B = 4, 5
    ds, sb, sde, ts, _, fwd_calls = _model(dev, T, mode="drift", chunk=2)
    keys, x0s, y0s, masks = _inputs(oracle, dev, ds, B)
    sb.fwd_sampler_batched(keys, x0s, y0s, masks)
    assert fwd_calls == [2, 2, 1] * T
    del fwd_calls[:]
    sb.fwd_sampler_batched(keys, x0s, y0s[0], masks[0], want_vs=False, batch_major=True)
    assert fwd_calls == [2, 2, 1] * T
    del fwd_calls[:]
    sb.chunk = 8                                          # one call per step once the chunk holds every ensemble
    sb.fwd_sampler_batched(keys, x0s, y0s, masks)
    assert fwd_calls == [5] * T


# ---------------------------------------------------------------------------------------------------
# the samplers
# ---------------------------------------------------------------------------------------------------
TS, NP, BS = 4, 5, 3                                      # steps, particles, ensembles of the end-to-end runs


def _stacked(loop, i):
    return torch.stack([torch.as_tensor(o[i]) for o in loop], 0)


def _gibbs_both(oracle, dev, mode, explicit_final, rows=True, wrap=False, chunk=2):
    """gibbs_kernel_batched against the loop of gibbs_kernel -> forward-drift calls of (the loop, the batched call)."""
    from fbs_amd.samplers import gibbs_kernel, gibbs_kernel_batched
    ds, sb, sde, ts, calls, fwd_calls = _model(dev, TS, mode=mode, chunk=chunk, rows=rows)
    keys, x0s, y0s, masks = _inputs(oracle, dev, ds, BS)
    rng = np.random.default_rng(7)
    us_stars = torch.from_numpy(rng.normal(size=(BS, TS + 1) + tuple(ds.unobs_shape)).astype(np.float32)).to(dev)
    bs_stars = rng.integers(0, NP, (BS, TS + 1)).astype(np.int32)
    cl = (sb.transition_sampler, sb.transition_logpdf, sb.likelihood_logpdf)
    loop = [gibbs_kernel(keys[b], x0s[b], y0s[b], us_stars[b], bs_stars[b], ts, sb.fwd_sampler, sde, sb.unpack, NP, *cl,
                         explicit_final=explicit_final, mask_=masks[b]) for b in range(BS)]
    n_loop = list(fwd_calls)
    del fwd_calls[:]
    fwd = (lambda *a, **k: sb.fwd_sampler(*a, **k)) if wrap else sb.fwd_sampler
    spy = _spy(sb)
    got = gibbs_kernel_batched(keys, x0s, y0s, us_stars, bs_stars, ts, fwd, sde, sb.unpack, NP, *cl,
                               explicit_final=explicit_final, mask_=masks)
    torch.cuda.synchronize()
    for i, what in enumerate(("x0", "us_star", "bs_star", "acc")):
        _eq(got[i], _stacked(loop, i), what)
    return n_loop, list(fwd_calls), spy


def _spy(sb):
    """Count the calls of the bridge's batched forward samplers (instance attributes: the bridge's own fwd_sampler /
    fwd_ys_sampler stay what they are)."""
    seen = {"fwd": 0, "ys": 0}
    fwd, ys = sb.fwd_sampler_batched, sb.fwd_ys_sampler_batched

    def fwd_spy(*a, **k):
        seen["fwd"] += 1
        return fwd(*a, **k)

    def ys_spy(*a, **k):
        seen["ys"] += 1
        return ys(*a, **k)

    sb.fwd_sampler_batched, sb.fwd_ys_sampler_batched = fwd_spy, ys_spy
    return seen


@pytest.mark.parametrize("explicit_final", (False, True))
def test_gibbs_kernel_drift_mode_equals_the_loop(oracle, dev, explicit_final):
    n_loop, n_batched, spy = _gibbs_both(oracle, dev, "drift", explicit_final)
    assert n_loop == [1] * (2 * TS * BS)                  # two paths per sweep and ensemble, one row per call
    assert n_batched == [2, 1] * (2 * TS)                 # 2 T ceil(B / chunk) calls for all ensembles
    assert spy["fwd"] == 2


def _init_both(oracle, dev, mode, rows=True, wrap=False, marg_y=False, method="filter"):
    from fbs_amd.samplers import gibbs_init, gibbs_init_batched
    ds, sb, sde, ts, calls, fwd_calls = _model(dev, TS, mode=mode, rows=rows)
    keys, x0s, y0s, masks = _inputs(oracle, dev, ds, BS)
    args = (sde, sb.unpack, sb.transition_sampler, sb.transition_logpdf, sb.likelihood_logpdf, NP)
    loop = [gibbs_init(keys[b], y0s[b], tuple(ds.unobs_shape), ts, sb.fwd_sampler, *args, method=method, marg_y=marg_y,
                       mask_=masks[b]) for b in range(BS)]
    n_loop = list(fwd_calls)
    del fwd_calls[:]
    fwd = (lambda *a, **k: sb.fwd_sampler(*a, **k)) if wrap else sb.fwd_sampler
    spy = _spy(sb)
    got = gibbs_init_batched(keys, y0s, tuple(ds.unobs_shape), ts, fwd, *args, method=method, marg_y=marg_y, mask_=masks)
    torch.cuda.synchronize()
    _eq(got[0], _stacked(loop, 0), "approx_x0")
    _eq(got[1], _stacked(loop, 1), "approx_us_star")
    return n_loop, list(fwd_calls), spy


def test_gibbs_init_drift_mode_equals_the_loop(oracle, dev):
    n_loop, n_batched, spy = _init_both(oracle, dev, "drift")
    assert n_loop == [1] * (2 * TS * BS)
    assert n_batched == [2, 1] * (2 * TS)
    assert spy["fwd"] == 2


@pytest.mark.parametrize("explicit_final", (False, True))
def test_gibbs_kernel_score_mode_equals_the_loop(oracle, dev, explicit_final):
    _, _, spy = _gibbs_both(oracle, dev, "score", explicit_final)
    assert spy["fwd"] == 2                                # the preamble's paths and the postamble's, one launch each


@pytest.mark.parametrize("method,marg_y", (("filter", False), ("filter", True), ("smoother", True)))
def test_gibbs_init_score_mode_equals_the_loop(oracle, dev, method, marg_y):
    _, _, spy = _init_both(oracle, dev, "score", marg_y=marg_y, method=method)
    assert spy["fwd"] == (2 if method == "filter" else 1)


@pytest.mark.parametrize("wrap", (False, True), ids=("own", "wrapped"))
@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("delta", (None, 0.005))
def test_pmcmc_kernel_score_mode_equals_the_loop(oracle, dev, delta, shared, wrap):
    from fbs_amd.samplers import pmcmc_kernel, pmcmc_kernel_batched, stratified
    ds, sb, sde, ts, _, _ = _model(dev, TS, chunk=7)
    keys, _, y0s, masks = _inputs(oracle, dev, ds, BS)
    if shared:
        y0s, masks = [y0s[0]] * BS, [masks[0]] * BS
    yss = torch.stack([sb.fwd_ys_sampler(oracle.PRNGKey(400 + b), y0s[b]) for b in range(BS)], 0)
    uTs = torch.zeros((BS,) + tuple(ds.unobs_shape), device=dev)
    log_ells = torch.full((BS,), -1e9, device=dev)        # every proposal is accepted: the returned paths ARE the proposals
    tail = (sde, sb.ref_sampler, sb.transition_sampler, sb.likelihood_logpdf, stratified, NP)
    loop = [pmcmc_kernel(keys[b], uTs[b], log_ells[b], yss[b], y0s[b], ts, sb.fwd_ys_sampler, *tail, delta=delta,
                         mask_=masks[b]) for b in range(BS)]
    fwd_ys = (lambda *a, **k: sb.fwd_ys_sampler(*a, **k)) if wrap else sb.fwd_ys_sampler
    spy = _spy(sb)
    got = pmcmc_kernel_batched(keys, uTs, log_ells, yss, y0s[0] if shared else y0s, ts, fwd_ys, *tail, delta=delta,
                               mask_=masks[0] if shared else masks)
    torch.cuda.synchronize()
    for i, what in enumerate(("uT", "log_ell", "ys")):
        _eq(got[i], _stacked(loop, i).to(dev), what)
    for f in got[3]._fields:
        _eq(getattr(got[3], f), torch.stack([getattr(o[3], f) for o in loop], 0), f)
    assert bool(got[3].is_accepted.all())
    assert spy["ys"] == (0 if wrap else 1)                # both pCN draws of all ensembles are ONE call of 2 B paths


# ---------------------------------------------------------------------------------------------------
# fallbacks: the per-ensemble loop, with the loop's call counts
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,wrap", ((True, True), (False, False)), ids=("wrapped", "no-rows-fn"))
def test_fallbacks_equal_the_loop(oracle, dev, rows, wrap):
    """A lambda around fwd_sampler is not the bridge's own method, and drift mode without fwd_drift_rows_fn has nothing to
    batch: both give the loop's results with the loop's one-row forward calls."""
    for run in (lambda: _gibbs_both(oracle, dev, "drift", True, rows=rows, wrap=wrap),
                lambda: _init_both(oracle, dev, "drift", rows=rows, wrap=wrap)):
        n_loop, n_batched, spy = run()
        assert n_loop == n_batched == [1] * (2 * TS * BS)
        assert spy["fwd"] == (0 if wrap else 2)
    if wrap:
        _, _, spy = _gibbs_both(oracle, dev, "score", False, wrap=True)
        assert spy["fwd"] == 0
