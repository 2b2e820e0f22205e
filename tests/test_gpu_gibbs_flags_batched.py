"""GPU: the Gibbs sweeps batched under every flag.  The four new kernels of fbs_amd/csrc/fbsmi_batch.hip equal their
single-ensemble entry points per row and the oracle, on uint32 views; ``gibbs_kernel_batched(explicit_backward=False)``
equals the loop of ``gibbs_kernel`` bit for bit and calls the network in the lockstep pattern, also in groups under the
stored-particle cap; the sweep's tail and the ``marg_y`` bridges are one launch each; and the chains of
``explicit_backward=False`` have the moments of the analytic tier's chains on the linear-Gaussian image model."""
import collections

import numpy as np
import pytest
import torch

from test_gpu_gibbs_batched import T, _assert_equal, _inputs, _model

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- fbsmi_force_move_batched -------------------------------------------------------------------------------------------
def _fm_weights(kind, n, k, rng):
    w = np.zeros(n, np.float32)
    if kind == "uniform":
        w[:] = np.float32(1.0) / np.float32(n)
    elif kind == "one-hot at k":                          # the w_k >= 1 branch: rest = 1 / n
        w[k] = 1.0
    elif kind == "one-hot elsewhere":
        w[(k + 1) % n] = 1.0
    elif kind == "w_k just below one":
        if n > 1:
            w[:] = np.float32(2.0 ** -23) / np.float32(n - 1)
        w[k] = np.float32(1.0) - np.float32(2.0 ** -23)
    else:                                                 # a row with zeros
        w = rng.random(n).astype(np.float32)
        w[rng.random(n) < 0.5] = 0.0
        w[(k + 1) % n] += np.float32(0.5)
        w = (w / w.sum(dtype=np.float32)).astype(np.float32)
    return w


FM_KINDS = ("uniform", "one-hot at k", "one-hot elsewhere", "w_k just below one", "zeros")


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("n", (1, 2, 5, 64, 65, 1000, 1024))
def test_force_move_batched(n, B, oracle, dev):
    from fbs_amd import ops
    from fbs_amd.samplers.gibbs import force_move
    rng = np.random.default_rng(1000 * n + B)
    for t, kind in enumerate(FM_KINDS):
        for where in ("first", "last", "random"):
            ks = np.array([0 if where == "first" else (n - 1 if where == "last" else int(rng.integers(0, n)))
                           for _ in range(B)], np.int32)
            keys = oracle.split(oracle.PRNGKey(17 * t + n), B)
            w = np.stack([_fm_weights(kind, n, int(ks[b]), rng) for b in range(B)], 0)
            wt = _up(w, dev)
            only_i = ops.force_move_batched(keys, wt, _up(ks, dev))                      # out_alpha null
            got_i, got_a = ops.force_move_batched(keys, wt, ks, return_alpha=True)       # out_alpha given
            assert only_i.dtype == torch.int32 and tuple(only_i.shape) == (B,) and got_a.dtype == torch.float32
            np.testing.assert_array_equal(_np(only_i), _np(got_i), err_msg=f"{kind} {where}")
            for b in range(B):
                si, sa = force_move(keys[b], wt[b], int(ks[b]))
                oi, oa = oracle.force_move(keys[b], w[b], int(ks[b]))
                what = f"{kind}, k {where} = {ks[b]}, n = {n}, row {b}"
                assert int(got_i[b]) == int(si) == oi, what
                assert _bits(_np(got_a[b])) == _bits(_np(sa)) == _bits(oa), what


def test_force_move_batched_refuses_before_any_launch(dev):
    from fbs_amd import ops
    keys = np.zeros((3, 2), np.uint32)
    with pytest.raises(NotImplementedError, match="1024"):
        ops.force_move_batched(keys, torch.zeros((3, 1025), device=dev), np.zeros(3, np.int32))
    with pytest.raises(RuntimeError):
        ops.force_move_batched(np.zeros((0, 2), np.uint32), torch.zeros((0, 8), device=dev), np.zeros(0, np.int32))
    torch.cuda.synchronize()


def test_force_move_batched_clamps_k(oracle, dev):
    """k outside [0, n) is clamped before it addresses memory: the entry is that of the nearest valid k."""
    from fbs_amd import ops
    n = 5
    keys = oracle.split(oracle.PRNGKey(3), 2)
    w = _up(np.stack([_fm_weights("zeros", n, 0, np.random.default_rng(b)) for b in range(2)], 0), dev)
    got = ops.force_move_batched(keys, w, np.array([-7, 1 << 30], np.int32))
    want = ops.force_move_batched(keys, w, np.array([0, n - 1], np.int32))
    np.testing.assert_array_equal(_np(got), _np(want))


# ---- fbsmi_randint_batched ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", ((0, 1), (0, 5), (0, 100), (3, 1024)))
@pytest.mark.parametrize("n", (1, 5, 257, 1000))
def test_randint_batched(n, lo, hi, oracle, dev):
    from fbs_amd import ops
    for B in (1, 3):
        keys = oracle.split(oracle.PRNGKey(n + hi), B)
        got = ops.randint_batched(keys, n, lo, hi, device=dev)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, n)
        for b in range(B):
            np.testing.assert_array_equal(_np(got[b]), _np(ops.randint(keys[b], (n,), lo, hi, device=dev)))
            np.testing.assert_array_equal(_np(got[b]), oracle.randint(keys[b], (n,), lo, hi))


# ---- fbsmi_backscan_batched ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("du", (1, 9, 289))
@pytest.mark.parametrize("n", (1, 5, 65, 1024))
@pytest.mark.parametrize("Tn", (0, 1, 4, 33))
def test_backscan_batched(Tn, n, du, oracle, dev):
    from fbs_amd import ops
    from fbs_amd.samplers.csmc.csmc import backward_scanning_pass
    B = 3
    rng = np.random.default_rng(Tn * 10000 + n * 10 + du)
    keys = oracle.split(oracle.PRNGKey(Tn + n + du), B)
    lw = (rng.normal(size=(B, n)) * 3).astype(np.float32)
    As = rng.integers(0, n, (Tn, B, n)).astype(np.int32)
    As[:, 1, :] = n // 2                                                         # ensemble 1: everything maps to one row
    uss = rng.random((Tn + 1, B, n, du), dtype=np.float32)
    lw_t, As_t, uss_t = _up(lw, dev), _up(As, dev), _up(uss, dev)
    path, Bs = ops.backscan_batched(keys, lw_t, As_t, uss_t)
    assert tuple(path.shape) == (B, Tn + 1, du) and tuple(Bs.shape) == (B, Tn + 1) and Bs.dtype == torch.int32
    for b in range(B):
        want_x, want_b = oracle.backward_scanning_pass(keys[b], As[:, b], uss[:, b], lw[b])
        np.testing.assert_array_equal(_np(Bs[b]), want_b, err_msg=f"Bs of ensemble {b}")
        np.testing.assert_array_equal(_bits(_np(path[b])), _bits(want_x), err_msg=f"path of ensemble {b}")
        if Tn > 0:                                                               # the single-ensemble pass needs a step
            sx, sb_ = backward_scanning_pass(keys[b], As_t[:, b].contiguous(), uss_t[:, b].contiguous(), lw_t[b])
            np.testing.assert_array_equal(_np(Bs[b]), _np(sb_))
            np.testing.assert_array_equal(_bits(_np(path[b])), _bits(_np(sx)))
    if Tn > 0:
        assert (_np(Bs[1])[:-1] == n // 2).all()


def test_backscan_batched_clamps_ancestors(oracle, dev):
    from fbs_amd import ops
    B, n, Tn, du = 2, 5, 3, 2
    keys = oracle.split(oracle.PRNGKey(5), B)
    lw = torch.zeros((B, n), device=dev)
    As = np.zeros((Tn, B, n), np.int32)
    As[:, 0, :], As[:, 1, :] = -3, 1 << 30
    uss = _up(np.arange((Tn + 1) * B * n * du, dtype=np.float32).reshape(Tn + 1, B, n, du), dev)
    path, Bs = ops.backscan_batched(keys, lw, _up(As, dev), uss)
    assert (_np(Bs[0])[:-1] == 0).all() and (_np(Bs[1])[:-1] == n - 1).all()
    for b in range(B):
        for k in range(Tn + 1):
            assert torch.equal(path[b, k], uss[k, b, int(Bs[b, k])])


# ---- fbsmi_affine_em_path_batched ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsub", (1, 100))
@pytest.mark.parametrize("Tn", (1, 4))
@pytest.mark.parametrize("D", (1, 9, 55, 1188))
def test_bridge_path_batched(D, Tn, nsub, oracle, dev):
    from fbs_amd.sdes import StationaryLinLinearSDE, doob_bridge_simulator, doob_bridge_simulator_batched
    from fbs_amd.sdes.linear import doob_bridge_tables
    sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=2.0)
    ts = np.linspace(0, 2.0, Tn + 1)
    tab = doob_bridge_tables(sde, ts, nsub)
    Bmax = 3
    keys = oracle.split(oracle.PRNGKey(D + Tn + nsub), Bmax)
    shape = (D, 1) if D > 1 else (1,)
    x0 = np.stack([oracle.normal(oracle.PRNGKey(400 + b), (D,)) for b in range(Bmax)], 0).reshape((Bmax,) + shape)
    xT = np.stack([oracle.normal(oracle.PRNGKey(500 + b), (D,)) for b in range(Bmax)], 0).reshape((Bmax,) + shape)
    x0_t, xT_t = _up(x0, dev), _up(xT, dev)
    for replace in (False, True):
        want = [oracle.doob_bridge_np(keys[b], tab["A"], tab["B"], tab["S"], tab["ddt"], x0[b], xT[b], Tn, nsub, replace)
                .reshape((Tn + 1,) + shape) for b in range(Bmax)]
        single = [_np(doob_bridge_simulator(keys[b], sde, x0_t[b], xT_t[b], ts, integration_nsteps=nsub, replace=replace))
                  for b in range(Bmax)]
        for b in range(Bmax):
            np.testing.assert_array_equal(_bits(single[b]), _bits(want[b]))
        for B in (1, 3):
            for reverse in (False, True):
                for time_major in (False, True):
                    got = doob_bridge_simulator_batched(keys[:B], sde, x0_t[:B], xT_t[:B], ts, integration_nsteps=nsub,
                                                        replace=replace, reverse=reverse, time_major=time_major)
                    assert tuple(got.shape) == (((Tn + 1, B) if time_major else (B, Tn + 1)) + shape)
                    got = _np(got.transpose(0, 1) if time_major else got)
                    for b in range(B):
                        g = got[b][::-1] if reverse else got[b]
                        np.testing.assert_array_equal(_bits(g), _bits(single[b]),
                                                      err_msg=f"B={B} replace={replace} reverse={reverse} time_major={time_major}")


# ---- sweeps without explicit_backward -----------------------------------------------------------------------------------
def _both(oracle, dev, B, nparticles, shared, **flags):
    """The loop of gibbs_kernel and gibbs_kernel_batched on the model of tests/test_gpu_gibbs_batched.py (row-wise score,
    chunk 7, T = 4); shared: one mask and one observation for all ensembles -> (batched, loop, network calls)."""
    from fbs_amd.samplers import gibbs_kernel, gibbs_kernel_batched
    ds, sb, sde, ts, calls = _model(dev, 7)
    keys, x0s, y0s, us_stars, bs_stars, masks = _inputs(oracle, dev, ds, B, nparticles)
    cl = (sb.transition_sampler, sb.transition_logpdf, sb.likelihood_logpdf)
    mask = (lambda b: masks[0]) if shared else (lambda b: masks[b])
    y0 = (lambda b: y0s[0]) if shared else (lambda b: y0s[b])
    loop = [gibbs_kernel(keys[b], x0s[b], y0(b), us_stars[b], bs_stars[b], ts, sb.fwd_sampler, sde, sb.unpack, nparticles,
                         *cl, mask_=mask(b), **flags) for b in range(B)]
    del calls[:]
    got = gibbs_kernel_batched(keys, x0s, y0s[0] if shared else y0s, us_stars, bs_stars, ts, sb.fwd_sampler, sde, sb.unpack,
                               nparticles, *cl, mask_=masks[0] if shared else masks, **flags)
    torch.cuda.synchronize()
    return got, loop, list(calls)


def _lockstep_calls(B, rows, rounds):
    per_round = -(-(B * rows) // 7)
    return ([7] * (per_round - 1) + [B * rows - 7 * (per_round - 1)]) * rounds


@pytest.mark.parametrize("shared", (False, True), ids=("masks", "one-mask"))
@pytest.mark.parametrize("B", (3, 1))
@pytest.mark.parametrize("marg_y", (False, True))
@pytest.mark.parametrize("explicit_final", (False, True))
def test_sweep_without_explicit_backward_equals_the_loop(oracle, dev, explicit_final, marg_y, B, shared):
    nparticles = 5
    got, loop, calls = _both(oracle, dev, B, nparticles, shared, explicit_backward=False, explicit_final=explicit_final,
                             marg_y=marg_y)
    _assert_equal(got, loop, B)
    rows = nparticles + (1 if explicit_final else 0)
    # T + ef rounds of ceil(B rows / 7) calls that straddle the ensembles, not `rows` rows B T times
    assert calls == _lockstep_calls(B, rows, T + (1 if explicit_final else 0)), calls


@pytest.mark.parametrize("explicit_final", (False, True))
def test_sweep_in_groups_under_the_store_cap(oracle, dev, explicit_final, monkeypatch):
    """The cap lowered to two ensembles' worth of stored particles: three ensembles run as a group of two and one of one."""
    from fbs_amd.samplers import gibbs_batched
    nparticles, B = 5, 3
    rows = nparticles + (1 if explicit_final else 0)
    monkeypatch.setattr(gibbs_batched, "LOCKSTEP_STORE_BYTES", 2 * 4 * (T + 1) * rows * 9)
    got, loop, calls = _both(oracle, dev, B, nparticles, False, explicit_backward=False, explicit_final=explicit_final)
    _assert_equal(got, loop, B)
    rounds = T + (1 if explicit_final else 0)
    assert calls == _lockstep_calls(2, rows, rounds) + _lockstep_calls(1, rows, rounds), calls
    # one ensemble alone above the cap: the loop, same bits
    monkeypatch.setattr(gibbs_batched, "LOCKSTEP_STORE_BYTES", 4 * (T + 1) * rows * 9 - 1)
    got, loop, calls = _both(oracle, dev, B, nparticles, False, explicit_backward=False, explicit_final=explicit_final)
    _assert_equal(got, loop, B)
    assert calls == [rows] * (B * rounds), calls


# ---- launch routes ------------------------------------------------------------------------------------------------------
SINGLE = ("fbsmi_force_move", "fbsmi_randint", "fbsmi_affine_em_path")


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


def test_the_tail_and_the_bridges_are_one_launch_each(oracle, dev, monkeypatch):
    from fbs_amd.samplers import gibbs_init_batched, gibbs_kernel_batched
    ds, sb, sde, ts, _ = _model(dev, 7)
    B, nparticles = 3, 5
    keys, x0s, y0s, us_stars, bs_stars, masks = _inputs(oracle, dev, ds, B, nparticles)
    cl = (sb.transition_sampler, sb.transition_logpdf, sb.likelihood_logpdf)
    sweep = _count_calls(monkeypatch, lambda: gibbs_kernel_batched(
        keys, x0s, y0s, us_stars, bs_stars, ts, sb.fwd_sampler, sde, sb.unpack, nparticles, *cl, marg_y=True,
        explicit_backward=True, mask_=masks))
    for name in SINGLE:
        assert sweep[name] == 0, (name, sweep)
        assert sweep[name + "_batched"] == 1, (name, sweep)
    init = _count_calls(monkeypatch, lambda: gibbs_init_batched(
        keys, y0s, (9, 1), ts, sb.fwd_sampler, sde, sb.unpack, *cl, nparticles, method="filter", marg_y=True, mask_=masks))
    for name in SINGLE:
        assert init[name] == 0, (name, init)
    assert init["fbsmi_affine_em_path_batched"] == 1, init
    scan = _count_calls(monkeypatch, lambda: gibbs_kernel_batched(
        keys, x0s, y0s, us_stars, bs_stars, ts, sb.fwd_sampler, sde, sb.unpack, nparticles, *cl, marg_y=True,
        explicit_backward=False, mask_=masks))
    assert scan["fbsmi_backscan_batched"] == 1 and scan["fbsmi_affine_em_path_batched"] == 1, scan
    assert scan["fbsmi_backtrace"] == scan["fbsmi_categorical"] == scan["fbsmi_affine_em_path"] == 0, scan


def test_gibbs_init_batched_marg_y_equals_the_loop(oracle, dev):
    from fbs_amd.samplers import gibbs_init, gibbs_init_batched
    ds, sb, sde, ts, _ = _model(dev, 7)
    B, nparticles = 3, 5
    keys, _, y0s, _, _, masks = _inputs(oracle, dev, ds, B, nparticles)
    cl = (sb.transition_sampler, sb.transition_logpdf, sb.likelihood_logpdf)
    for method in ("filter", "smoother"):
        loop = [gibbs_init(keys[b], y0s[b], (9, 1), ts, sb.fwd_sampler, sde, sb.unpack, *cl, nparticles, method=method,
                           marg_y=True, mask_=masks[b]) for b in range(B)]
        got = gibbs_init_batched(keys, y0s, (9, 1), ts, sb.fwd_sampler, sde, sb.unpack, *cl, nparticles, method=method,
                                 marg_y=True, mask_=masks)
        for i in range(2):
            want = torch.stack([o[i] for o in loop], 0)
            assert torch.equal(got[i].contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), (method, i)


# ---- anchor: the chains of explicit_backward=False against the analytic tier's ------------------------------------------
@pytest.mark.parametrize("explicit_final", (False, True), ids=("gibbs", "gibbs-ef"))
def test_chains_without_explicit_backward_against_the_analytic_chains(explicit_final, dev, oracle):
    """The design of tests/test_gpu_images_lg.py (inpaint-2 on 5x5x1, 8 steps, 64 chains, 16 particles, 20 + 100 sweeps, fixed
    keys): ``gibbs_kernel_batched(explicit_backward=False)`` against ``LGSweep.chain`` with the same flags on the permuted
    model; per-coordinate mean of x0 and second moment about the reference mean within 5 sqrt(2) SE, SE from the spread over
    the reference chains, whose two halves must meet the same threshold (also checked on the CPU,
    tests/test_gibbs_flags_batched_host.py)."""
    import test_gpu_images_lg as L
    from fbs_amd.samplers import gibbs_kernel_batched
    sm, g = L._sampler_setup(dev, oracle)
    sb, br, du = g["sb"], g["br"], sm["tab"]["du"]
    nsw = L.G_BURN + L.G_KEEP
    h = br.sweep_handle(L.G_N, False, explicit_final, nchains=L.S_B)
    _, _, _, ref = h.chain(oracle.PRNGKey(L.G_REF_SEED), np.zeros((L.S_B, du), np.float32), sm["y0"],
                           np.zeros((L.S_B, L.S_T + 1), np.int32), nsw)
    key = oracle.PRNGKey(32)
    x0s, bs = torch.zeros((L.S_B, du, 1), device=dev), np.zeros((L.S_B, L.S_T + 1), np.int32)
    got = []
    for _ in range(nsw):
        key, sub = oracle.split(key)
        x0s, _, bsn, _ = gibbs_kernel_batched(oracle.split(sub, L.S_B), x0s, g["y0"], None, bs, sm["ts"], sb.fwd_sampler,
                                              sm["model"].sde, sb.unpack, L.G_N, sb.transition_sampler,
                                              sb.transition_logpdf, sb.likelihood_logpdf, explicit_backward=False,
                                              explicit_final=explicit_final, mask_=g["mask"])
        bs = bsn.cpu().numpy()
        got.append(x0s.reshape(L.S_B, du))
    got = torch.stack(got, 0).cpu().numpy()
    L._moments_against_reference(f"gibbs_kernel_batched explicit_backward=False explicit_final={explicit_final}",
                                 got[L.G_BURN:], ref.cpu().numpy()[L.G_BURN:])
