"""GPU: the image twisted SMC batched over ensembles (fbs_amd/twisted.py make_image_twisted_batched; the step kernels
fbsmi_tw_img_*_batched and fbsmi_categorical_batched of fbs_amd/csrc/fbsmi_batch.hip).

Kernel level: every kernel against the float64 restatement of its specification within first-order rounding bounds
(tests/tw_img_restate.py: nothing here is measured or tuned), and against the composition of make_image_twisted's closures
at the tolerances of tests/test_gpu_images_e2e.py:147-158.  Host level: an ensemble does not depend on B; a teacher-forced
float64 replay of every step of every ensemble from the run's own trace; the fallback; the driver."""
import os
import sys

import numpy as np
import pytest
import torch

from tw_img_restate import U32, TwStep, depth, step_scalars

pytestmark = pytest.mark.gpu

TEND, NSTEPS, N = 2.0, 6, 5
C, G = 0.6, 0.8
SHAPES = [("inpaint-4", (9, 9, 1)),      # D = 81, odd: one ragged segment, an odd Threefry draw of n * D
          ("inpaint-5", (20, 20, 1)),    # D = 400: two segments, the second ragged; dv = 375
          ("supr-2", (12, 12, 2)),       # a scattered mask with two channels
          ("supr-2", (20, 20, 3))]       # D = 1200 > 4 * 256: a second, ragged round of the row loop
F32, BF16 = torch.float32, torch.bfloat16
NET_DT = {F32: 0, BF16: 1}


def _sde():
    from fbs_amd.sdes import StationaryLinLinearSDE
    return StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=TEND)


def coupling(x, t):
    """s(x, t) = -c x + g * mean over the image's own pixels: every output pixel depends on every input pixel."""
    return -C * x + G * x.reshape(x.shape[0], -1).mean(1).reshape((-1,) + (1,) * (x.dim() - 1))


def rolled(x, t):
    """A row-wise stand-in whose output row has the same bits whichever rows share its call: elementwise arithmetic on
    shifted copies of the row."""
    f = x.reshape(x.shape[0], -1)
    return (-C * f + G * torch.tanh(f.roll(1, 1)) * f.roll(-3, 1)).reshape(x.shape)


def through_bf16(fn):
    """fn with its output rounded to bfloat16 (as a bfloat16 network returns it), the gradient passing unrounded."""
    def score(x, t):
        o = fn(x, t)
        return o + (o.to(BF16).float() - o).detach()
    return score


class Case:
    def __init__(self, task, shape, B, per_mask, dev, n=N, seed=0):
        from fbs_amd import ops
        from fbs_amd.images import ImageRestore
        from fbs_amd.score import EMMask, EMMaskBatch
        self.dev, self.shape, self.B, self.n, self.D = dev, tuple(shape), B, n, int(np.prod(shape))
        self.sde, self.ts = _sde(), np.linspace(0, TEND, NSTEPS + 1)
        self.ds = ImageRestore(task, shape, device=dev)
        nm = B if per_mask else 1
        uniq = [self.ds.gen_mask(ops.PRNGKey(40 + i)) for i in range(nm)]
        self.masks = [uniq[b if per_mask else 0] for b in range(B)]
        self.mask_arg = list(uniq) if per_mask else uniq[0]
        ems = [EMMask(m, shape[2], dev) for m in uniq]
        self.mb = EMMaskBatch(ems)
        self.roles = [ems[b if per_mask else 0].role.cpu().numpy() for b in range(B)]
        rng = np.random.default_rng(seed)
        self.dv = self.mb.dv
        self.y = torch.from_numpy(rng.normal(size=(B, self.dv)).astype(np.float32)).to(dev)
        self.ys = [self.y[b].reshape(-1, shape[2]) for b in range(B)]
        self.X = torch.from_numpy(rng.normal(size=(B * n, self.D)).astype(np.float32)).to(dev)
        self.keys = np.stack([ops.PRNGKey(900 + b) for b in range(B)], 0)
        self.rng = rng

    def rows(self, t, b):
        return t.reshape(self.B, self.n, -1)[b].double().cpu().numpy()


def _new(dev, *shape):
    return torch.empty(shape, dtype=F32, device=dev)


def k_cotangent(c, net, sc, X=None):
    from fbs_amd import _lib, ops
    cx, cs, dt, _, var_y = sc
    ct = _new(c.dev, c.B * c.n, c.D)
    X = c.X if X is None else X
    _lib.call("fbsmi_tw_img_cotangent_batched", c.mb.ref, X.data_ptr(), net.data_ptr(), NET_DT[net.dtype], cx, cs, dt, var_y,
              c.y.data_ptr(), c.B, c.n, ct.data_ptr(), ops._stream())
    return ct


def k_propose(c, net, vjp, sc, keys, out_dtype=None, sd=None, X=None):
    from fbs_amd import _lib, ops
    cx, cs, dt, sd0, var_y = sc
    R = c.B * c.n
    X = c.X if X is None else X
    xn, tl, pl = _new(c.dev, R, c.D), _new(c.dev, c.B, c.n), _new(c.dev, c.B, c.n)
    copy = torch.empty((R, c.D), dtype=out_dtype, device=c.dev) if out_dtype is not None else None
    kd = ops.keys_to_device(keys, c.dev)
    _lib.call("fbsmi_tw_img_propose_batched", c.mb.ref, X.data_ptr(), net.data_ptr(), NET_DT[net.dtype], vjp.data_ptr(), cx, cs,
              dt, sd0 if sd is None else sd, var_y, c.y.data_ptr(), kd.data_ptr(), c.B, c.n, xn.data_ptr(), tl.data_ptr(),
              pl.data_ptr(), NET_DT[out_dtype] if out_dtype is not None else 0, copy.data_ptr() if copy is not None else None,
              ops._stream())
    return xn, tl, pl, copy


def k_twist(c, X, net, sc, tl=None, pl=None, lpg=None):
    from fbs_amd import _lib, ops
    cx, cs, dt, _, var_y = sc
    lp = _new(c.dev, c.B, c.n)
    lw = _new(c.dev, c.B, c.n) if tl is not None else None
    p = lambda t: t.data_ptr() if t is not None else None
    _lib.call("fbsmi_tw_img_twist_batched", c.mb.ref, X.data_ptr(), net.data_ptr(), NET_DT[net.dtype], cx, cs, dt, var_y,
              c.y.data_ptr(), p(tl), p(pl), p(lpg), c.B, c.n, lp.data_ptr(), p(lw), ops._stream())
    return lp, lw


def _vjp(score, X4, t, ct):
    x = X4.detach().requires_grad_(True)
    with torch.enable_grad():
        out = score(x, t)
        return torch.autograd.grad(out, x, grad_outputs=ct.reshape(out.shape))[0].reshape(ct.shape).contiguous()


def _within(got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: largest error / bound = {worst:.3f}, largest error = {float(err.max()):.3e}")
    assert (err <= bound).all(), (what, worst, float(err.max()))


@pytest.mark.parametrize("per_mask", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("task,shape", SHAPES)
def test_step_kernels_against_the_restatement_and_the_closures(task, shape, B, per_mask, dev):
    from fbs_amd import ops
    from fbs_amd.twisted import make_image_twisted
    c = Case(task, shape, B, per_mask, dev)
    n, D, k = c.n, c.D, 3
    t = float(c.ts[k])
    s_fwd = TEND - t
    sc = step_scalars(c.sde, c.ts, k)
    dt = sc[2]
    X4 = c.X.reshape((B * n,) + c.shape)
    Z = [ops.normal(c.keys[b], (n,) + c.shape, device=dev) for b in range(B)]
    for net_dt in (F32, BF16):
        score = coupling if net_dt == F32 else through_bf16(coupling)
        tw = make_image_twisted(score, c.ds, c.sde, c.ts, n)
        with torch.no_grad():
            net = score(X4, s_fwd).reshape(B * n, D).to(net_dt).contiguous()
        steps = [TwStep(c.roles[b], *sc) for b in range(B)]
        # ---- cotangent, and the network's vector-Jacobian product (torch, float32: an INPUT of the proposal)
        ct = k_cotangent(c, net, sc)
        vjp = _vjp(score, X4, s_fwd, ct)
        # ---- proposal: the bits do not depend on whether, or in which dtype, the network-input copy is written
        xn, tl, pl, _ = k_propose(c, net, vjp, sc, c.keys)
        for out_dt in (F32, BF16):
            xn2, tl2, pl2, copy = k_propose(c, net, vjp, sc, c.keys, out_dtype=out_dt)
            assert torch.equal(xn2, xn) and torch.equal(tl2, tl) and torch.equal(pl2, pl), out_dt
            assert torch.equal(copy, xn.to(out_dt)), out_dt                      # torch's conversion, bit for bit
        m32 = k_propose(c, net, vjp, sc, c.keys, sd=0.0)[0]                     # sd = 0: x_new IS the float32 mean m
        # ---- twist, alone and with the weights
        lp, none = k_twist(c, c.X, net, sc)
        assert none is None
        tl_in, pl_in, lpg = (torch.from_numpy(c.rng.normal(size=(B, n)).astype(np.float32) * 50).to(dev) for _ in range(3))
        lp2, lw = k_twist(c, c.X, net, sc, tl_in, pl_in, lpg)
        assert torch.equal(lp2, lp)
        for b in range(B):
            st, yb = steps[b], c.y[b].double().cpu().numpy()
            Xb, Sb, Vb, Zb = c.rows(c.X, b), c.rows(net.float(), b), c.rows(vjp, b), Z[b].reshape(n, D).double().cpu().numpy()
            ref, bound = st.cotangent(Xb, Sb, yb)
            _within(c.rows(ct, b), ref, bound, "ct")
            ref, bound, m, E_m = st.propose(Xb, Sb, Vb, yb, Zb)
            _within(c.rows(xn, b), ref, bound, "x_new")
            _within(c.rows(m32, b), m, E_m, "m")
            # the draw: x_new = fl(m + fl(sd z)) with z the bits of ops.normal(key, (n,) + shape) -- two roundings
            xb, nz = c.rows(xn, b), sc[3] * Zb
            _within(xb - c.rows(m32, b), nz, U32 * (np.abs(nz) + np.abs(xb) * (1 + 2.0 ** -20)), "x_new - m = sd z")
            rtl, Etl, rpl, Epl = st.logpdfs(Xb, Sb, Vb, yb, xb)
            _within(tl[b].double().cpu().numpy(), rtl, Etl, "tl")
            _within(pl[b].double().cpu().numpy(), rpl, Epl, "pl")
            rlp, Elp = st.twist(Xb, Sb, yb)
            _within(lp[b].double().cpu().numpy(), rlp, Elp, "lp")
            rlw, Elw = st.weights(lp[b].double().cpu().numpy(), Elp * 0, tl_in[b].cpu().numpy(), pl_in[b].cpu().numpy(),
                                  lpg[b].cpu().numpy())
            _within(lw[b].double().cpu().numpy(), rlw, Elw, "lw")                # from the kernel's own float32 lp
            # ---- the closures of make_image_twisted, at the tolerances of test_gpu_images_e2e.py:147-158
            uv, y2, mk = X4[b * n:(b + 1) * n], c.ys[b], c.masks[b]
            got_cd = (m32.reshape(B, n, D)[b].double() - uv.reshape(n, D).double()) / dt
            want_cd = tw.reverse_cond_drift(uv, t, y2, mk).reshape(n, D).double()
            assert torch.allclose(got_cd, want_cd, rtol=2e-5, atol=2e-5), (got_cd - want_cd).abs().max().item()
            want_prop = tw.twisting_prop_sampler(c.keys[b], uv, t, y2, mask_=mk).reshape(n, D)
            assert torch.allclose(xn.reshape(B, n, D)[b], want_prop, rtol=2e-5, atol=2e-5)
            assert torch.allclose(lp[b], tw.twisting_logpdf(y2, uv, t, mask_=mk), rtol=2e-5, atol=1e-3)
            u_new = xn.reshape((B, n) + c.shape)[b].contiguous()
            assert torch.allclose(tl[b].double(), tw.transition_logpdf(u_new, uv, t).double(), rtol=1e-4, atol=5e-2)
            assert torch.allclose(pl[b].double(), tw.twisting_prop_logpdf(u_new, uv, t, y2, mask_=mk).double(), rtol=1e-4,
                                  atol=5e-2)


def test_gather_equals_torch_indexing(dev):
    from fbs_amd import _lib, ops
    rng = np.random.default_rng(1)
    for B, n, D in ((1, 1, 7), (3, 5, 81), (2, 65, 1200)):
        X = torch.from_numpy(rng.normal(size=(B, n, D)).astype(np.float32)).to(dev)
        lp = torch.from_numpy(rng.normal(size=(B, n)).astype(np.float32)).to(dev)
        A = torch.from_numpy(rng.integers(0, n, size=(B, n)).astype(np.int32)).to(dev)
        if n > 1:
            A[B - 1, 0], A[0, n - 1] = n + 3, -2                                  # out of range: clamped into the ensemble
        Xp, lpg = torch.full_like(X, float("nan")), torch.full_like(lp, float("nan"))
        _lib.call("fbsmi_tw_img_gather_batched", X.data_ptr(), lp.data_ptr(), A.data_ptr(), B, n, D, Xp.data_ptr(),
                  lpg.data_ptr(), ops._stream())
        Ac = A.long().clamp(0, n - 1)
        rows = torch.arange(B, device=dev)[:, None]
        assert torch.equal(Xp, X[rows, Ac]) and torch.equal(lpg, lp[rows, Ac]), (B, n, D)
        Xq = torch.full_like(X, float("nan"))                                      # lp_prev_g is optional
        _lib.call("fbsmi_tw_img_gather_batched", X.data_ptr(), None, A.data_ptr(), B, n, D, Xq.data_ptr(), None, ops._stream())
        assert torch.equal(Xq, Xp)


@pytest.mark.parametrize("n", [1, 2, 65, 1024])
def test_categorical_batched_equals_categorical(n, dev):
    from fbs_amd import ops
    rng = np.random.default_rng(n)
    B = 4
    w = rng.random((B, n)).astype(np.float32)
    w[1] = 0.0
    w[1, n // 2] = 1.0                                                             # a one-hot row
    w[2] /= w[2].sum()
    wt = torch.from_numpy(w).to(dev)
    for rep in range(3):
        keys = np.stack([ops.PRNGKey(100 * rep + b) for b in range(B)], 0)
        got = ops.categorical_batched(keys, wt)
        want = torch.stack([ops.categorical(keys[b], wt[b]) for b in range(B)])
        assert got.dtype == torch.int32 and torch.equal(got, want), (n, rep, got, want)
    assert int(got[1]) == n // 2


def _run_setup(task, shape, B, dev, n, score, chunk=4096, seed=5, nsteps=NSTEPS):
    from fbs_amd import ops
    from fbs_amd.images import ImageRestore
    from fbs_amd.twisted import make_image_twisted_batched
    sde, ts = _sde(), np.linspace(0, TEND, nsteps + 1)
    ds = ImageRestore(task, shape, device=dev)
    masks = [ds.gen_mask(ops.PRNGKey(60 + b)) for b in range(B)]
    rng = np.random.default_rng(seed)
    ys = [torch.from_numpy(rng.normal(size=tuple(ds.unpack(torch.zeros(shape, device=dev), m)[1].shape)).astype(np.float32)).to(dev)
          for m in masks]
    keys = np.stack([ops.PRNGKey(700 + b) for b in range(B)], 0)
    tw = make_image_twisted_batched(score, ds, sde, ts, n, chunk=chunk)
    return tw, ds, sde, ts, masks, ys, keys


def test_an_ensemble_does_not_depend_on_B(dev):
    """Ensemble b of a B = 3 run with chunk = 2 (chunks straddle ensembles) is bit-equal, at every trace entry, to the same
    ensemble run alone through the lockstep path; the score function sees [2, 2, ..., tail] rows per pass and
    2 * nsteps + 1 passes per chunk column."""
    from fbs_amd.samplers import stratified
    B, n, nsteps = 3, 5, 4
    calls = []

    def score(x, t):
        calls.append(int(x.shape[0]))
        return rolled(x, t)

    tw, ds, sde, ts, masks, ys, keys = _run_setup("inpaint-5", (12, 12, 2), B, dev, n, score, chunk=2, nsteps=nsteps)
    trace = []
    uvs, log_ws = tw.twisted_smc_batched(keys, ys, masks, stratified, trace=trace)
    R = B * n
    per_pass = [2] * (R // 2) + ([R % 2] if R % 2 else [])
    assert calls == per_pass * (2 * nsteps + 1), calls
    assert len(trace) == nsteps + 1 and trace[0][0] is None
    assert uvs.shape == (B, n, 12, 12, 2) and log_ws.shape == (B, n) and torch.isfinite(uvs).all()
    for b in range(B):
        del calls[:]
        alone = []
        u1, l1 = tw.twisted_smc_batched(keys[b:b + 1], [ys[b]], [masks[b]], stratified, trace=alone)
        assert calls == ([2] * (n // 2) + [n % 2]) * (2 * nsteps + 1), calls
        assert torch.equal(u1[0], uvs[b]) and torch.equal(l1[0], log_ws[b]), b
        for k, (full, one) in enumerate(zip(trace, alone)):
            for j, (f, o) in enumerate(zip(full, one)):
                assert (f is None and o is None) or torch.equal(f[b], o[0]), (b, k, j)
    assert torch.equal(trace[-1][1].reshape(uvs.shape), uvs) and torch.equal(trace[-1][3], log_ws)


def test_teacher_forced_float64_replay_of_every_step(dev):
    """Coupling score, B = 3, a mask and an observation per ensemble, (12, 12, 2) inpaint-5, n = 8, 6 steps.  From the run's
    own trace, for EVERY step and ensemble: the ancestors are stratified(exp(log_ws_prev[b]), key_resampling) bit for bit;
    X_new, lp and the normalised log_ws equal the float64 step from the traced float32 X and ancestors within the
    restatement's bounds.  The network is not part of the specification: its float32 values (and its vector-Jacobian
    product, on the cotangent the kernel itself returns for these inputs) are replayed by the same torch calls on the same
    rows, and enter the float64 step as the inputs they are for the kernels.

    The normalised log-weights: log_ws = lw - lse(lw), lse being 1-Lipschitz in the largest error of lw; the kernel's own
    logsumexp adds the subtraction of the maximum (u), exp and log (2 ulp each), the tree sum (depth(n) u relative, absolute
    on the logarithm), the sum with the maximum and the final subtraction:
        E = E_lw[i] + max_j E_lw[j] + (depth(n) + 8) u + 2 u |lse| + u |log_ws[i]|."""
    from fbs_amd import ops
    from fbs_amd.samplers import stratified
    from fbs_amd.score import EMMask, EMMaskBatch
    from fbs_amd.twisted import twisted_filter_key_schedule
    B, n, shape = 3, 8, (12, 12, 2)
    D = int(np.prod(shape))
    tw, ds, sde, ts, masks, ys, keys = _run_setup("inpaint-5", shape, B, dev, n, coupling)
    trace = []
    uvs, log_ws = tw.twisted_smc_batched(keys, ys, masks, stratified, trace=trace)
    assert len(trace) == NSTEPS + 1
    ks = twisted_filter_key_schedule(keys, NSTEPS)
    ems = [EMMask(m, shape[2], dev) for m in masks]
    c = Case.__new__(Case)                                                         # the kernel callers' view of this run
    c.dev, c.B, c.n, c.D, c.mb = dev, B, n, D, EMMaskBatch(ems)
    c.y = torch.stack([y.reshape(-1) for y in ys], 0).contiguous()
    roles = [e.role.cpu().numpy() for e in ems]
    rows = lambda t_, b: t_.reshape(B, n, -1)[b].double().cpu().numpy()
    vec = lambda t_, b: t_[b].double().cpu().numpy()

    def normalised(lw, E):
        mx = lw.max()
        lse = mx + np.log(np.exp(lw - mx).sum())
        out = lw - lse
        return out, E + E.max() + (depth(n) + 8) * U32 + 2 * U32 * abs(lse) + U32 * np.abs(out)

    # entry 0: the initial particles are ops.normal(key_init, (n,) + shape) bit for bit
    _, X, lp, lws = trace[0]
    for b in range(B):
        assert torch.equal(X[b], ops.normal(ks["init"][b], (n,) + shape, device=dev).reshape(n, D)), b
    with torch.no_grad():
        net = coupling(X.reshape((B * n,) + shape), TEND - float(ts[0])).reshape(B * n, D)
    sc = step_scalars(sde, ts, 0)
    for b in range(B):
        rlp, Elp = TwStep(roles[b], *sc).twist(rows(X, b), rows(net, b), vec(c.y, b))
        _within(vec(lp, b), rlp, Elp, ("lp", 0, b))
        rl, El = normalised(rlp, Elp)
        _within(vec(lws, b), rl, El, ("log_ws", 0, b))
    for k in range(NSTEPS):
        A, X_new, lp_new, lws_new = trace[k + 1]
        _, X_prev, lp_prev, lws_prev = trace[k]
        s_fwd = TEND - float(ts[k + 1])
        sc = step_scalars(sde, ts, k + 1)
        for b in range(B):
            want = stratified(ops.math_map("exp", lws_prev[b].contiguous()), ks["resampling"][k, b])
            assert torch.equal(A[b], want), ("ancestors", k, b)
        Ac = A.long().clamp(0, n - 1)
        bi = torch.arange(B, device=dev)[:, None]
        Xp, lpg = X_prev[bi, Ac].contiguous(), lp_prev[bi, Ac]
        Xp4 = Xp.reshape((B * n,) + shape)
        with torch.no_grad():
            net_p = coupling(Xp4, s_fwd).reshape(B * n, D).contiguous()
            net_n = coupling(X_new.reshape((B * n,) + shape), s_fwd).reshape(B * n, D).contiguous()
        vjp = _vjp(coupling, Xp4, s_fwd, k_cotangent(c, net_p, sc, X=Xp.reshape(B * n, D)))
        for b in range(B):
            st, yb = TwStep(roles[b], *sc), vec(c.y, b)
            Z = ops.normal(ks["prop"][k, b], (n,) + shape, device=dev).reshape(n, D).double().cpu().numpy()
            Xb, Sb, Vb = rows(Xp, b), rows(net_p, b), rows(vjp, b)
            ref, bound, _, _ = st.propose(Xb, Sb, Vb, yb, Z)
            _within(rows(X_new, b), ref, bound, ("X_new", k, b))
            rlp, Elp = st.twist(rows(X_new, b), rows(net_n, b), yb)
            _within(vec(lp_new, b), rlp, Elp, ("lp", k, b))
            rtl, Etl, rpl, Epl = st.logpdfs(Xb, Sb, Vb, yb, rows(X_new, b))
            g = vec(lpg, b)
            lw = ((rtl + rlp) - rpl) - g
            Elw = Etl + Elp + Epl + 3 * U32 * (np.abs(rtl) + np.abs(rlp) + np.abs(rpl) + np.abs(g))
            rl, El = normalised(lw, Elw)
            _within(vec(lws_new, b), rl, El, ("log_ws", k, b))
    assert torch.equal(trace[-1][1].reshape(uvs.shape), uvs) and torch.equal(trace[-1][3], log_ws)


def test_masks_of_two_sizes_run_the_loop(dev):
    """Masks of different (du, dv) cannot advance in lockstep: the result is that of the loop of
    make_image_twisted(...).conditional_sampler over the ensembles, bit for bit."""
    from fbs_amd import ops
    from fbs_amd.images import ImageRestore
    from fbs_amd.samplers import stratified
    from fbs_amd.twisted import make_image_twisted, make_image_twisted_batched
    shape, n = (12, 12, 2), 6
    sde, ts = _sde(), np.linspace(0, TEND, 5)
    ds = ImageRestore("inpaint-5", shape, device=dev)
    masks = [ds.gen_mask(ops.PRNGKey(1)), ImageRestore("inpaint-4", shape, device=dev).gen_mask(ops.PRNGKey(2)),
             ds.gen_mask(ops.PRNGKey(3))]
    rng = np.random.default_rng(2)
    ys = [torch.from_numpy(rng.normal(size=(int(m.obs_inds_ravelled.numel()), shape[2])).astype(np.float32)).to(dev) for m in masks]
    keys = np.stack([ops.PRNGKey(30 + b) for b in range(3)], 0)
    got = make_image_twisted_batched(coupling, ds, sde, ts, n).conditional_sampler_batched(keys, ys, masks, stratified)
    single = make_image_twisted(coupling, ds, sde, ts, n)
    want = torch.stack([single.conditional_sampler(keys[b], ys[b], stratified, mask_=masks[b]) for b in range(3)], 0)
    assert got.shape == (3,) + shape and torch.equal(got, want)
    # and masks of one size take the lockstep path: a valid, finite draw of the same shape
    same = make_image_twisted_batched(coupling, ds, sde, ts, n).conditional_sampler_batched(
        keys, [ys[0], ys[2], ys[2]], [masks[0], masks[2], masks[2]], stratified)
    assert same.shape == (3,) + shape and torch.isfinite(same).all()


def test_driver_batch_writes_the_files_of_the_sequential_run(tmp_path, dev):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import imgs_restore
    common = ["--task", "inpaint", "--rect_size", "15", "--method", "twisted", "--nsamples", "2", "--ny0s", "2",
              "--nparticles", "6", "--test_nsteps", "5", "--dim", "8", "--fp32", "--quiet"]
    found = {}
    for batch in (1, 3):
        out_dir = tmp_path / f"b{batch}"
        out = imgs_restore.main(common + ["--batch", str(batch), "--outdir", str(out_dir)])
        assert out.shape == (2, 28, 28, 1) and np.isfinite(out).all()
        found[batch] = {}
        for f in sorted(os.listdir(out_dir)):
            z = np.load(out_dir / f)
            arrs = {k: z[k] for k in z.files} if f.endswith(".npz") else {"": z}
            assert all(np.isfinite(a).all() for a in arrs.values()), f
            found[batch][f] = {k: a.shape for k, a in arrs.items()}
    assert found[3] == found[1] and any(f.endswith("-twisted.npy") for f in found[3]), found
    assert sum(f.endswith("-twisted.npy") for f in found[3]) == 2
