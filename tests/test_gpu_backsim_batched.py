"""GPU: the image backward passes batched over ensembles.

* fbsmi_em_translp_batched against fbsmi_em_transition_logpdf called per ensemble, and fbsmi_backsim_pick_batched against
  ops.normalise + ops.categorical + a row gather per ensemble, bit for bit, read through batch-major and time-major strides;
* bootstrap_backward_smoother_batched and backward_sampling_pass_batched against the loops of their namesakes, with a score
  whose output row depends on its own input row only (the model of tests/test_gpu_smc_batched.py);
* gibbs_init_batched(method='smoother', smoother='lockstep' / 'reuse') against the loop of gibbs_init, with the network
  calls each makes; the launches of a backward pass; the fallbacks; the driver's --batch_init with --init_method smoother."""
import collections
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# du: 9; 81 with a different random mask per ensemble; exactly one 256-element segment; 1083 = a second round of the
# workgroup (4 x 256 elements per round) and a ragged tail
TASKS = {"inpaint-3": (8, 8, 1), "supr-2": (6, 6, 3), "inpaint-16": (20, 20, 1), "inpaint-19": (20, 20, 3)}
DU = {"inpaint-3": 9, "supr-2": 81, "inpaint-16": 256, "inpaint-19": 1083}
COEF = dict(cx=0.3, cs=1.2, dt=0.002, sd=0.07)
SLOTS = 3               # time slots of the stored arrays the kernels read slices of
UNSUPPORTED = -3


def _masks(oracle, dev, task, B, shared):
    from fbs_amd.images import ImageRestore
    from fbs_amd.score import EMMask, EMMaskBatch
    shape = TASKS[task]
    ds = ImageRestore(task, shape, device=dev)
    masks = [ds.gen_mask(oracle.PRNGKey(40 + b)) for b in range(1 if shared else B)]
    if task == "supr-2" and not shared and B > 1:
        assert not torch.equal(masks[0].unobs_inds_ravelled, masks[1].unobs_inds_ravelled)
    ems = [EMMask(m, shape[2], dev) for m in masks]
    mb = EMMaskBatch(ems)
    assert mb.du == DU[task] and mb.nmasks == (1 if shared else B)
    return mb, (lambda b: ems[0 if shared else b])


def _stored(x, major):
    """x (B, SLOTS, ...) -> (the array as stored batch-major or time-major, b -> its slice [b, :] as a view)."""
    if major == "batch":
        return x, x
    tm = x.transpose(0, 1).contiguous()                                             # (SLOTS, B, ...)
    return tm, tm.transpose(0, 1)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------
# fbsmi_em_translp_batched
# ---------------------------------------------------------------------------------------------------
def _check_translp(oracle, dev, task, B, n, shared):
    from fbs_amd import _lib
    mb, em = _masks(oracle, dev, task, B, shared)
    du, D = mb.du, mb.D
    g = torch.Generator(device="cpu").manual_seed(1000 * B + n)
    us_all = torch.randn((B, SLOTS, n, du), generator=g).to(dev)
    u_all = (0.5 * torch.randn((B, SLOTS, du), generator=g)).to(dev)
    net32 = torch.randn((B * n, D), generator=g).to(dev)
    t = 1                                                                           # the time slice the call reads
    for net in (net32, net32.to(torch.bfloat16)):
        net_dt = 0 if net.dtype == torch.float32 else 1
        for mode in (0, 1):
            want = torch.full((B, n), float("nan"), device=dev)
            for b in range(B):
                us_b, u_b, net_b = us_all[b, t].contiguous(), u_all[b, t + 1].contiguous(), net[b * n:(b + 1) * n].contiguous()
                _lib.call("fbsmi_em_transition_logpdf", em(b).ref, us_b.data_ptr(), net_b.data_ptr(), net_dt, mode, COEF["cx"],
                          COEF["cs"], COEF["dt"], COEF["sd"], u_b.data_ptr(), n, want[b].data_ptr(), 0)
            assert torch.isfinite(want).all()
            for major in ("batch", "time"):
                us_store, us_view = _stored(us_all, major)
                us_t = us_view[:, t]
                assert us_t.data_ptr() == us_store.data_ptr() + 4 * (t * n * du if major == "batch" else t * B * n * du)
                got = torch.full((B, n), float("nan"), device=dev)
                _lib.call("fbsmi_em_translp_batched", mb.ref, us_t.data_ptr(), us_t.stride(0) if B > 1 else n * du,
                          net.data_ptr(), net_dt, mode, COEF["cx"], COEF["cs"], COEF["dt"], COEF["sd"],
                          u_all[:, t + 1].data_ptr(), u_all.stride(0), B, n, got.data_ptr(), 0)
                torch.cuda.synchronize()
                assert torch.equal(_bits(got), _bits(want)), (task, B, n, shared, net_dt, mode, major)


@pytest.mark.parametrize("n", (1, 2, 5, 64, 65, 1024))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("task", sorted(TASKS))
def test_translp_batched_equals_the_single_entry_point(oracle, dev, task, B, n):
    _check_translp(oracle, dev, task, B, n, shared=False)


@pytest.mark.parametrize("task", ("inpaint-3", "inpaint-19"))
def test_translp_batched_shared_mask(oracle, dev, task):
    """nmasks = 1: one mask for all three ensembles."""
    _check_translp(oracle, dev, task, 3, 5, shared=True)


def test_translp_through_the_bridge(oracle, dev):
    """ScoreBridge.transition_logpdf_batched, with and without a kept network output, equals the closure per ensemble and
    reads slices of stored arrays in place."""
    ds, sb, sde, ts, calls = _model(dev)
    B, n = 3, 5
    masks = [ds.gen_mask(oracle.PRNGKey(60 + b)) for b in range(B)]
    g = torch.Generator(device="cpu").manual_seed(3)
    uss = torch.randn((B, SLOTS, n, 9, 1), generator=g).to(dev)
    traj = torch.randn((B, SLOTS, 9, 1), generator=g).to(dev)
    vp = torch.randn((B, 55, 1), generator=g).to(dev)
    want = torch.stack([sb.transition_logpdf(traj[b, 2], uss[b, 1].contiguous(), vp[b], ts[1], masks[b]) for b in range(B)], 0)
    del calls[:]
    got = sb.transition_logpdf_batched(traj[:, 2], uss[:, 1], vp, ts[1], masks)
    assert calls == [7, 7, 1] and tuple(got.shape) == (B, n)
    assert torch.equal(_bits(got), _bits(want))
    kept = sb._buf["net"].clone()
    del calls[:]
    again = sb.transition_logpdf_batched(traj[:, 2], uss[:, 1], vp, ts[1], masks, net=kept)
    assert calls == [] and torch.equal(_bits(again), _bits(want))
    with pytest.raises(ValueError):
        sb.transition_logpdf_batched(traj[:, 2], uss[:, 1], vp, ts[1], masks, net=kept[:-1])


def test_more_than_1024_rows_is_refused_without_a_launch(oracle, dev):
    from fbs_amd import _lib
    mb, _ = _masks(oracle, dev, "inpaint-3", 1, True)
    L = _lib.lib()
    x = torch.zeros(16, device=dev)
    sentinel = torch.full((1, 1025), 7.0, device=dev)
    rc = L.fbsmi_em_translp_batched(mb.ref, x.data_ptr(), 0, x.data_ptr(), 0, 0, 0.1, 0.2, 0.01, 0.1, x.data_ptr(), 0, 1, 1025,
                                    sentinel.data_ptr(), 0)
    assert rc == UNSUPPORTED and b"1024" in L.fbsmi_last_error()
    idx = torch.full((1,), -5, dtype=torch.int32, device=dev)
    rc = L.fbsmi_backsim_pick_batched(x.data_ptr(), sentinel.data_ptr(), None, x.data_ptr(), 0, 1, 1025, 1, idx.data_ptr(), 1,
                                      x.data_ptr(), 1, 0)
    assert rc == UNSUPPORTED and b"1024" in L.fbsmi_last_error()
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all()) and int(idx[0]) == -5 and bool((x == 0).all())


# ---------------------------------------------------------------------------------------------------
# fbsmi_backsim_pick_batched
# ---------------------------------------------------------------------------------------------------
def _pick_reference(ops, keys, lw, log_w, us_t):
    rows, idx = [], []
    for b in range(lw.shape[0]):
        g = lw[b]
        if log_w is not None:
            g = g - torch.max(g)                                                    # csmc.py:206
            g = g + log_w[b]                                                        # :207
        i = ops.categorical(keys[b], ops.normalise(g, log_space=False))
        idx.append(i)
        rows.append(us_t[b][i.long()])
    return torch.stack(rows, 0), torch.stack(idx, 0)


@pytest.mark.parametrize("du", (9, 1083))
@pytest.mark.parametrize("n", (1, 2, 5, 64, 65, 1024))
@pytest.mark.parametrize("B", (1, 3))
def test_pick_batched_equals_normalise_categorical_gather(oracle, dev, B, n, du):
    from fbs_amd import ops
    g = torch.Generator(device="cpu").manual_seed(77 * B + n + du)
    us_all = torch.randn((B, SLOTS, n, du), generator=g).to(dev)
    lw = (3.0 * torch.randn((B, n), generator=g)).to(dev)
    log_w = ops.normalise_batched((2.0 * torch.randn((B, n), generator=g)).to(dev), log_space=True)
    t = 1
    for trial in range(3):                                                          # three draws per shape
        keys = oracle.split(oracle.PRNGKey(9000 + 31 * n + trial), B)
        for lg in (None, log_w):
            want_rows, want_idx = _pick_reference(ops, keys, lw, lg, us_all[:, t])
            assert want_idx.dtype == torch.int32
            for major in ("batch", "time"):
                _, us_view = _stored(us_all, major)
                out_all = torch.full((B, SLOTS, du), float("nan"), device=dev)
                idx_all = torch.full((B, SLOTS), -1, dtype=torch.int32, device=dev)
                rows, idx = ops.backsim_pick_batched(keys, lw, us_view[:, t], log_w=lg, out=out_all[:, t], idx=idx_all[:, t])
                torch.cuda.synchronize()
                where = (B, n, du, trial, lg is not None, major)
                assert rows.data_ptr() == out_all[:, t].data_ptr() and idx.data_ptr() == idx_all[:, t].data_ptr()
                assert torch.equal(idx_all[:, t], want_idx), where
                assert torch.equal(_bits(out_all[:, t]), _bits(want_rows)), where
                # the slots on either side are untouched
                assert bool(torch.isnan(out_all[:, t - 1]).all()) and bool(torch.isnan(out_all[:, t + 1]).all()), where
                assert bool((idx_all[:, t - 1] == -1).all()) and bool((idx_all[:, t + 1] == -1).all()), where
        rows, idx = ops.backsim_pick_batched(keys, lw, us_all[:, t].contiguous())     # fresh outputs
        want_rows, want_idx = _pick_reference(ops, keys, lw, None, us_all[:, t])
        assert tuple(rows.shape) == (B, du) and torch.equal(idx, want_idx) and torch.equal(_bits(rows), _bits(want_rows))


@pytest.mark.parametrize("n", (1, 5, 65, 1024))
def test_pick_batched_one_finite_weight(oracle, dev, n):
    """A row whose weights are all -inf but one: that one is picked, with and without log_w."""
    from fbs_amd import ops
    B, du = 3, 9
    g = torch.Generator(device="cpu").manual_seed(n)
    us = torch.randn((B, n, du), generator=g).to(dev)
    only = [0, n - 1, n // 2]
    lw = torch.full((B, n), float("-inf"), device=dev)
    for b in range(B):
        lw[b, only[b]] = -3.5 * (b + 1)
    log_w = ops.normalise_batched(torch.randn((B, n), generator=g).to(dev), log_space=True)
    keys = oracle.split(oracle.PRNGKey(5 + n), B)
    for lg in (None, log_w):
        rows, idx = ops.backsim_pick_batched(keys, lw, us, log_w=lg)
        want_rows, want_idx = _pick_reference(ops, keys, lw, lg, us)
        assert idx.tolist() == only and torch.equal(idx, want_idx)
        assert torch.equal(_bits(rows), _bits(want_rows))
        assert torch.equal(rows, us[torch.arange(B, device=dev), torch.tensor(only, device=dev)])


# ---------------------------------------------------------------------------------------------------
# the passes equal the loops (the model of tests/test_gpu_smc_batched.py: T = 4, N = 5, chunk = 7, a row-wise score)
# ---------------------------------------------------------------------------------------------------
T = 4
N = 5


def _model(dev, chunk=7):
    from fbs_amd.images import ImageRestore
    from fbs_amd.score import ScoreBridge
    from fbs_amd.sdes import StationaryLinLinearSDE
    ts = np.linspace(0, 2.0, T + 1)
    sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=2.0)
    ds = ImageRestore("inpaint-3", (8, 8, 1), device=dev)
    calls = []

    def score_fn(x, t):                                  # row-wise: a row's output does not depend on its neighbours
        calls.append(int(x.shape[0]))
        return (0.25 * x.roll(1, 2) - 0.5 * x) * float(t)

    return ds, ScoreBridge(score_fn, ds, sde, ts, chunk=chunk), sde, ts, calls


def _inputs(oracle, dev, ds, sb, B, shared, seed=0):
    """keys, masks, y0s, observation paths in reverse time (B, T + 1, q, c); `shared`: one mask and one y0 for all."""
    from fbs_amd import ops
    keys = oracle.split(oracle.PRNGKey(1000 * seed + 41 + B), B)
    masks = [ds.gen_mask(oracle.PRNGKey(200 + (0 if shared else b))) for b in range(B)]
    if shared:
        masks = [masks[0]] * B
    y0s = [ds.unpack(ops.uniform(oracle.PRNGKey(300 + (0 if shared else b)), (8, 8, 1), device=dev), masks[b])[1]
           for b in range(B)]
    yss = torch.stack([sb.fwd_ys_sampler(oracle.PRNGKey(1000 * seed + 400 + b), y0s[b]) for b in range(B)], 0)
    return keys, masks, y0s, torch.flip(yss, [1])


def _bits_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), what


def _lockstep_calls(B, n=N, chunk=7):
    """The network calls of one lockstep step repeated T times: chunks of `chunk` rows over the flat B * n rows."""
    rows = B * n
    return ([chunk] * (rows // chunk) + ([rows % chunk] if rows % chunk else [])) * T


def _filtered(oracle, dev, ds, sb, B, shared, nparticles=N):
    """keys, masks, vss and the stored particles of a lockstep filter, (B, T + 1, n, 9, 1)."""
    from fbs_amd.samplers import bootstrap_filter_batched, stratified
    keys, masks, _, vss = _inputs(oracle, dev, ds, sb, B, shared)
    uss, _ = bootstrap_filter_batched(sb.transition_sampler, sb.likelihood_logpdf, vss, sb.ts, sb.ref_sampler,
                                      oracle.split(oracle.PRNGKey(17), B), nparticles, stratified, return_last=False,
                                      mask_=masks[0] if shared else masks)
    return keys, masks, vss, uss


@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("B", (3, 1))
def test_backward_smoother_lockstep_equals_the_loop(oracle, dev, B, shared):
    from fbs_amd.samplers import bootstrap_backward_smoother_batched
    from fbs_amd.samplers.smc import bootstrap_backward_smoother
    ds, sb, sde, ts, calls = _model(dev)
    keys, masks, vss, uss = _filtered(oracle, dev, ds, sb, B, shared)
    loop = torch.stack([bootstrap_backward_smoother(keys[b], uss[b], vss[b], ts, sb.transition_logpdf, mask_=masks[b])
                        for b in range(B)], 0)
    mask_kw = masks[0] if shared else masks
    del calls[:]
    got = bootstrap_backward_smoother_batched(keys, uss, vss, ts, sb.transition_logpdf, mask_=mask_kw)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, T + 1, 9, 1)
    _bits_equal(got, loop, "trajectories")
    assert calls == _lockstep_calls(B), calls
    # every point of a trajectory is one of the filter's particles of its time
    for b in range(B):
        for k in range(T + 1):
            assert bool((uss[b, k] == got[b, k]).flatten(1).all(1).any()), (b, k)
    # the network outputs of the filter's inputs, kept: no network call at all
    mb = sb.em_mask_batch(mask_kw, B)
    kept = torch.stack([sb._network_batched(uss[:, t].contiguous().reshape(B, N, -1), None,
                                            vss[:, t].contiguous().reshape(B, -1), ts[t], mb).clone() for t in range(T)], 0)
    del calls[:]
    reuse = bootstrap_backward_smoother_batched(keys, uss, vss, ts, sb.transition_logpdf, network_outputs=kept, mask_=mask_kw)
    torch.cuda.synchronize()
    assert calls == []
    _bits_equal(reuse, loop, "trajectories from kept network outputs")


@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("B", (3, 1))
def test_backward_sampling_pass_lockstep_equals_the_loop(oracle, dev, B, shared):
    from fbs_amd import ops
    from fbs_amd.samplers import backward_sampling_pass_batched
    from fbs_amd.samplers.csmc.csmc import backward_sampling_pass
    ds, sb, sde, ts, calls = _model(dev)
    keys, masks, vss, uss = _filtered(oracle, dev, ds, sb, B, shared)
    g = torch.Generator(device="cpu").manual_seed(11 + B)
    log_wss = torch.stack([ops.normalise_batched((1.5 * torch.randn((B, N), generator=g)).to(dev), log_space=True)
                           for _ in range(T + 1)], 1)                               # (B, T + 1, n), each row normalised
    loop = [backward_sampling_pass(keys[b], sb.transition_logpdf, vss[b], ts, uss[b], log_wss[b], mask_=masks[b])
            for b in range(B)]
    del calls[:]
    xs, Bs = backward_sampling_pass_batched(keys, sb.transition_logpdf, vss, ts, uss, log_wss,
                                            mask_=masks[0] if shared else masks)
    torch.cuda.synchronize()
    assert tuple(xs.shape) == (B, T + 1, 9, 1) and tuple(Bs.shape) == (B, T + 1) and Bs.dtype == torch.int32
    _bits_equal(xs, torch.stack([o[0] for o in loop], 0), "paths")
    _bits_equal(Bs, torch.stack([o[1] for o in loop], 0), "indices")
    assert calls == _lockstep_calls(B), calls
    assert bool(((Bs >= 0) & (Bs < N)).all())
    for b in range(B):
        for k in range(T + 1):
            assert torch.equal(xs[b, k], uss[b, k, int(Bs[b, k])]), (b, k)


# ---------------------------------------------------------------------------------------------------
# gibbs_init_batched(method='smoother', smoother=...)
# ---------------------------------------------------------------------------------------------------
def _init_both(oracle, dev, B, shared, smoother, marg_y):
    from fbs_amd.samplers import gibbs_init, gibbs_init_batched
    ds, sb, sde, ts, calls = _model(dev)
    keys, masks, y0s, _ = _inputs(oracle, dev, ds, sb, B, shared)
    args = (ts, sb.fwd_sampler, sde, sb.unpack, sb.transition_sampler, sb.transition_logpdf, sb.likelihood_logpdf, N)
    loop = [gibbs_init(keys[b], y0s[b], (9, 1), *args, method="smoother", marg_y=marg_y, mask_=masks[b]) for b in range(B)]
    del calls[:]
    got = gibbs_init_batched(keys, y0s[0] if shared else y0s, (9, 1), *args, method="smoother", marg_y=marg_y,
                             smoother=smoother, mask_=masks[0] if shared else masks)
    torch.cuda.synchronize()
    return got, loop, list(calls)


def _check_init(got, loop, B):
    assert tuple(got[0].shape) == (B, 9, 1) and tuple(got[1].shape) == (B, T + 1, 9, 1)
    _bits_equal(got[0], torch.stack([o[0] for o in loop], 0), "approx_x0")
    _bits_equal(got[1], torch.stack([o[1] for o in loop], 0), "approx_us_star")


@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("marg_y", (True, False))
@pytest.mark.parametrize("smoother", ("lockstep", "reuse"))
@pytest.mark.parametrize("B", (3, 1))
def test_gibbs_init_smoother_modes_equal_the_loop(oracle, dev, B, smoother, marg_y, shared):
    got, loop, calls = _init_both(oracle, dev, B, shared, smoother, marg_y)
    _check_init(got, loop, B)
    per_pass = _lockstep_calls(B)
    if B == 3:
        assert per_pass == [7, 7, 1] * T
    assert calls[:len(per_pass)] == per_pass, calls                                  # the filter, in lockstep
    assert calls[len(per_pass):] == (per_pass if smoother == "lockstep" else []), calls


def test_gibbs_init_smoother_default_is_the_loop(oracle, dev):
    got, loop, calls = _init_both(oracle, dev, 3, False, "loop", True)
    _check_init(got, loop, 3)
    assert calls == [7, 7, 1] * T + [N] * (3 * T), calls


def test_gibbs_init_reuse_above_the_store_cap_runs_lockstep(oracle, dev, monkeypatch):
    from fbs_amd.samplers import gibbs_batched
    store = T * 3 * N * 64 * 4                                                       # (T, B * n, D) float32
    monkeypatch.setattr(gibbs_batched, "LOCKSTEP_STORE_BYTES", store - 1)
    got, loop, calls = _init_both(oracle, dev, 3, False, "reuse", True)
    _check_init(got, loop, 3)
    assert calls == [7, 7, 1] * T + [7, 7, 1] * T, calls
    monkeypatch.setattr(gibbs_batched, "LOCKSTEP_STORE_BYTES", store)
    got, loop, calls = _init_both(oracle, dev, 3, False, "reuse", True)
    _check_init(got, loop, 3)
    assert calls == [7, 7, 1] * T, calls


# ---------------------------------------------------------------------------------------------------
# launch counts
# ---------------------------------------------------------------------------------------------------
def _count_calls(monkeypatch, fn):
    from fbs_amd import _lib
    counts = collections.Counter()
    real = _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", counting)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(_lib, "call", real)
    return counts


def test_a_backward_pass_is_two_launches_per_step(oracle, dev, monkeypatch):
    from fbs_amd import ops
    from fbs_amd.samplers import (backward_sampling_pass_batched, bootstrap_backward_smoother_batched, gibbs_init_batched)
    ds, sb, sde, ts, calls = _model(dev)
    B = 3
    keys, masks, vss, uss = _filtered(oracle, dev, ds, sb, B, False)
    log_wss = ops.normalise_batched(torch.zeros((B * (T + 1), N), device=dev), log_space=True).reshape(B, T + 1, N)
    single = ("fbsmi_em_transition_logpdf", "fbsmi_categorical", "fbsmi_normalise", "fbsmi_em_concat", "fbsmi_gather_rows")
    smooth = _count_calls(monkeypatch, lambda: bootstrap_backward_smoother_batched(keys, uss, vss, ts, sb.transition_logpdf,
                                                                                   mask_=masks))
    assert smooth["fbsmi_em_translp_batched"] == T and smooth["fbsmi_backsim_pick_batched"] == T, smooth
    assert smooth["fbsmi_em_concat_batched"] == T and smooth["fbsmi_randint_batched"] == 1, smooth
    sample = _count_calls(monkeypatch, lambda: backward_sampling_pass_batched(keys, sb.transition_logpdf, vss, ts, uss, log_wss,
                                                                              mask_=masks))
    assert sample["fbsmi_em_translp_batched"] == T and sample["fbsmi_backsim_pick_batched"] == T + 1, sample
    for counts in (smooth, sample):
        for name in single:
            assert counts[name] == 0, (name, counts)
    y0s = [ds.unpack(ops.uniform(oracle.PRNGKey(300 + b), (8, 8, 1), device=dev), masks[b])[1] for b in range(B)]
    init = _count_calls(monkeypatch, lambda: gibbs_init_batched(
        keys, y0s, (9, 1), ts, sb.fwd_sampler, sde, sb.unpack, sb.transition_sampler, sb.transition_logpdf,
        sb.likelihood_logpdf, N, method="smoother", smoother="reuse", mask_=masks))
    assert init["fbsmi_em_translp_batched"] == T and init["fbsmi_backsim_pick_batched"] == T, init
    assert init["fbsmi_em_concat_batched"] == T, init                                # the filter's: none in the backward pass
    for name in single:
        assert init[name] == 0, (name, init)


# ---------------------------------------------------------------------------------------------------
# fallbacks: the loop of the single function, one network call per ensemble and step
# ---------------------------------------------------------------------------------------------------
def _fallback_closures(sb):
    wrapped = lambda u, us, v_prev, t_prev, mask_: sb.transition_logpdf(u, us, v_prev, t_prev, mask_)
    with_extra = lambda u, us, v_prev, t_prev, mask_, extra: sb.transition_logpdf(u, us, v_prev, t_prev, mask_)
    return (("wrapped", wrapped, {}), ("extra keyword", with_extra, {"extra": 1}))


def test_fallbacks_run_the_loop(oracle, dev):
    from fbs_amd import ops
    from fbs_amd.samplers import backward_sampling_pass_batched, bootstrap_backward_smoother_batched
    from fbs_amd.samplers.csmc.csmc import backward_sampling_pass
    from fbs_amd.samplers.smc import bootstrap_backward_smoother
    ds, sb, sde, ts, calls = _model(dev)
    B = 2
    keys, masks, vss, uss = _filtered(oracle, dev, ds, sb, B, False)
    log_wss = ops.normalise_batched(torch.linspace(-2, 1, B * (T + 1) * N, device=dev).reshape(-1, N),
                                    log_space=True).reshape(B, T + 1, N)
    for what, closure, extra in _fallback_closures(sb):
        loop = torch.stack([bootstrap_backward_smoother(keys[b], uss[b], vss[b], ts, closure, mask_=masks[b], **extra)
                            for b in range(B)], 0)
        del calls[:]
        got = bootstrap_backward_smoother_batched(keys, uss, vss, ts, closure, mask_=masks, **extra)
        torch.cuda.synchronize()
        _bits_equal(got, loop, what)
        assert calls == [N] * (B * T), (what, calls)
        loop = [backward_sampling_pass(keys[b], closure, vss[b], ts, uss[b], log_wss[b], mask_=masks[b], **extra)
                for b in range(B)]
        del calls[:]
        xs, Bs = backward_sampling_pass_batched(keys, closure, vss, ts, uss, log_wss, mask_=masks, **extra)
        torch.cuda.synchronize()
        _bits_equal(xs, torch.stack([o[0] for o in loop], 0), what)
        _bits_equal(Bs, torch.stack([o[1] for o in loop], 0), what)
        assert calls == [N] * (B * T), (what, calls)


def test_fallback_more_than_1024_rows(oracle, dev):
    from fbs_amd.samplers import bootstrap_backward_smoother_batched
    from fbs_amd.samplers.smc import bootstrap_backward_smoother
    ds, sb, sde, ts, calls = _model(dev, chunk=2048)
    B, n = 2, 1025
    keys, masks, _, vss = _inputs(oracle, dev, ds, sb, B, False)
    g = torch.Generator(device="cpu").manual_seed(1)
    uss = torch.randn((B, T + 1, n, 9, 1), generator=g).to(dev)
    loop = torch.stack([bootstrap_backward_smoother(keys[b], uss[b], vss[b], ts, sb.transition_logpdf, mask_=masks[b])
                        for b in range(B)], 0)
    del calls[:]
    got = bootstrap_backward_smoother_batched(keys, uss, vss, ts, sb.transition_logpdf, mask_=masks)
    torch.cuda.synchronize()
    _bits_equal(got, loop, "trajectories")
    assert calls == [n] * (B * T), calls


def test_gibbs_init_with_a_foreign_transition_logpdf(oracle, dev):
    """The filter advances in lockstep, its network outputs are not kept for a closure that is not the bridge's own, and
    the smoother runs the loop."""
    from fbs_amd.samplers import gibbs_init, gibbs_init_batched
    ds, sb, sde, ts, calls = _model(dev)
    B = 2
    keys, masks, y0s, _ = _inputs(oracle, dev, ds, sb, B, False)
    wrapped = _fallback_closures(sb)[0][1]
    args = (ts, sb.fwd_sampler, sde, sb.unpack, sb.transition_sampler, wrapped, sb.likelihood_logpdf, N)
    loop = [gibbs_init(keys[b], y0s[b], (9, 1), *args, method="smoother", mask_=masks[b]) for b in range(B)]
    del calls[:]
    got = gibbs_init_batched(keys, y0s, (9, 1), *args, method="smoother", smoother="reuse", mask_=masks)
    torch.cuda.synchronize()
    _check_init(got, loop, B)
    assert calls == _lockstep_calls(B) + [N] * (B * T), calls


# ---------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------
COMMON = ["--ny0s", "3", "--nsamples", "2", "--nparticles", "4", "--test_nsteps", "3", "--dim", "8", "--fp32", "--quiet"]


def test_driver_batch_init_smoother_writes_the_same_file_set(tmp_path, dev):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import imgs_restore
    args = COMMON + ["--method", "gibbs-eb-ef", "--init_method", "smoother", "--batch", "2"]
    seq, bat, lock = tmp_path / "seq", tmp_path / "bat", tmp_path / "lock"
    imgs_restore.main(args + ["--outdir", str(seq)])
    out = imgs_restore.main(args + ["--batch_init", "--outdir", str(bat)])          # smoother='reuse'
    assert out.shape == (2, 28, 28, 1) and np.isfinite(out).all()
    imgs_restore.main(args + ["--batch_init", "--init_smoother", "lockstep", "--outdir", str(lock)])
    names = sorted(os.listdir(seq))
    assert len(names) == 9
    for other in (bat, lock):
        assert sorted(os.listdir(other)) == names
        for f in names:
            a, b = np.load(seq / f), np.load(other / f)
            if f.endswith(".npz"):
                assert np.array_equal(a["test_img"], b["test_img"])
            else:
                assert a.shape == b.shape and np.isfinite(b).all(), f
