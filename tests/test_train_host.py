"""CPU: the trainer's host side -- fbsmi_uniform_host, the declarations and refusals of fbs_amd/csrc/fbsmi_train.hip, the
schedules, the checkpoint round trip, and the restatements of tests/train_restate.py telling the obvious mistakes apart."""
import ctypes
import os
import re

import numpy as np
import pytest

import train_restate as R

ARG = -1
P = 0x1000          # a non-null pointer value: the refusals below never dereference it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fbsmi_uniform_host", "fbsmi_dsm_noise_batched", "fbsmi_dsm_loss_workspace_bytes", "fbsmi_dsm_loss_batched",
         "fbsmi_sqnorm_workspace_bytes", "fbsmi_sqnorm", "fbsmi_adam_ema_step")


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257])
def test_uniform_host_equals_the_oracle(oracle, n):
    from fbs_amd.sdes.losses import uniform_host
    key = oracle.PRNGKey(40 + n)
    assert np.array_equal(uniform_host(key, n).view(np.uint32), oracle.uniform(key, (n,)).view(np.uint32))


def test_times_follow_jax_uniform(oracle):
    from fbs_amd import ops
    from fbs_amd.sdes.losses import training_times
    key = ops.PRNGKey(5)
    lo, hi = np.float32(1e-5), np.float32(2.0)
    want = np.sort(np.maximum(lo, oracle.uniform(key, (6,)) * (hi - lo) + lo))
    ts = training_times(key, 7, 0., 2., True, True)
    assert ts.dtype == np.float32 and np.array_equal(ts[:-1], want) and ts[-1] == 2.0
    tp = training_times(key, 7, 0., 2., True, False)
    assert tp.shape == (8,) and tp[0] == 0.0 and np.array_equal(tp[1:-1], want) and tp[-1] == 2.0
    assert np.array_equal(training_times(key, 1, 0., 2., True, True), np.array([2.0], np.float32))
    np.testing.assert_allclose(training_times(key, 8, 0., 2., False, True), np.linspace(0.25, 2., 8), rtol=1e-7)
    np.testing.assert_allclose(training_times(key, 4, 0., 2., False, False), np.linspace(0., 2., 5), rtol=1e-7)


def test_entries_declared_bound_and_exported():
    from fbs_amd import _lib
    L = ctypes.CDLL(_lib.build())
    header = open(os.path.join(ROOT, "include", "fbsmi.h")).read()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
        assert re.search(r"\b%s\(" % n, header), n
    assert any(p.endswith("fbsmi_train.hip") for p in _lib._SRC)
    assert _lib.lib().fbsmi_abi_version() == 1


def test_noise_refusals():
    from fbs_amd import _lib
    L = _lib.lib()
    f = L.fbsmi_dsm_noise_batched
    ok = [P, None, P, P, P, 3, 8, 0, P, None]                # data idx keys F sq B D out_dtype xt stream
    for hole in (0, 2, 3, 4, 8):
        a = list(ok)
        a[hole] = None
        assert f(*a) == ARG and b"null" in L.fbsmi_last_error()
    for pos, bad in ((5, 0), (6, 0), (6, 2 ** 32 - 3), (7, 2), (7, -1), (5, 2 ** 31)):
        a = list(ok)
        a[pos] = bad
        assert f(*a) == ARG, (pos, bad)
    a = list(ok)
    a[5], a[6] = 2 ** 26, 2 ** 20                            # 64 workgroups per row: 2^32 workgroups
    assert f(*a) == ARG and b"grid" in L.fbsmi_last_error()


def test_loss_refusals():
    from fbs_amd import _lib
    L = _lib.lib()
    f = L.fbsmi_dsm_loss_batched
    # net net_dtype mode keys xt data idx F sq gc inv B D dnet row_sums loss workspace stream
    ok0 = [P, 0, 0, P, None, None, None, None, P, P, 0.1, 3, 8, P, None, P, P, None]
    ok1 = [P, 0, 1, None, P, P, None, P, P, P, 0.1, 3, 8, P, None, P, P, None]
    for ok, holes in ((ok0, (0, 3, 8, 9, 13, 15, 16)), (ok1, (0, 4, 5, 7, 8, 9, 13, 15, 16))):
        for hole in holes:
            a = list(ok)
            a[hole] = None
            assert f(*a) == ARG, hole
        for pos, bad in ((1, 2), (2, 2), (2, -1), (11, 0), (12, 0), (12, 2 ** 32 - 3)):
            a = list(ok)
            a[pos] = bad
            assert f(*a) == ARG, (pos, bad)
        a = list(ok)
        a[11], a[12] = 2 ** 26, 2 ** 20
        assert f(*a) == ARG and b"grid" in L.fbsmi_last_error()
    assert L.fbsmi_dsm_loss_workspace_bytes(5, 2048) == 5 * 4 and L.fbsmi_dsm_loss_workspace_bytes(5, 2049) == 5 * 2 * 4
    assert L.fbsmi_dsm_loss_workspace_bytes(0, 8) == 0 and L.fbsmi_dsm_loss_workspace_bytes(1, 2 ** 32 - 3) == 0


def test_sqnorm_adam_and_uniform_refusals():
    from fbs_amd import _lib
    L = _lib.lib()
    assert L.fbsmi_sqnorm(None, 8, P, P, None) == ARG and L.fbsmi_sqnorm(P, 8, None, P, None) == ARG
    assert L.fbsmi_sqnorm(P, 8, P, None, None) == ARG and L.fbsmi_sqnorm(P, 0, P, P, None) == ARG
    assert L.fbsmi_sqnorm_workspace_bytes(2049) == 8 and L.fbsmi_sqnorm_workspace_bytes(0) == 0
    f = L.fbsmi_adam_ema_step
    # p g m v ema n lr b1 b2 eps bc1 bc2 gnorm2 max_norm ema_mode decay stream
    ok = [P, P, P, P, P, 8, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, None, 1.0, 2, 0.99, None]
    for hole in range(5):
        a = list(ok)
        a[hole] = None
        assert f(*a) == ARG, hole
    for pos, bad in ((5, 0), (14, 3), (14, -1), (10, 0.0), (11, 0.0)):
        a = list(ok)
        a[pos] = bad
        assert f(*a) == ARG, (pos, bad)
    a = list(ok)
    a[12], a[13] = P, 0.0
    assert f(*a) == ARG
    assert L.fbsmi_uniform_host(1, 2, 4, None) == ARG and L.fbsmi_uniform_host(1, 2, -1, P) == ARG
    assert L.fbsmi_uniform_host(1, 2, 0, None) == 0


def test_schedules_against_hand_values():
    from fbs_amd.train import constant_schedule, cosine_decay_schedule, exponential_decay
    cos = cosine_decay_schedule(2e-4, 100, 1e-2)
    assert cos(0) == pytest.approx(2e-4, rel=1e-15)
    assert cos(50) == pytest.approx(2e-4 * (0.99 * 0.5 + 0.01), rel=1e-14)
    assert cos(25) == pytest.approx(2e-4 * (0.99 * 0.5 * (1 + 2 ** -0.5) + 0.01), rel=1e-14)
    assert cos(100) == pytest.approx(2e-6, rel=1e-12) and cos(1000) == cos(100)
    ex = exponential_decay(1e-3, 10, 0.96)
    assert ex(0) == 1e-3 and ex(10) == pytest.approx(0.96e-3, rel=1e-15) and ex(5) == pytest.approx(1e-3 * 0.96 ** 0.5, rel=1e-15)
    assert constant_schedule(0.05)(0) == 0.05 and constant_schedule(0.05)(12345) == 0.05
    for k in (0, 1, 7, 99, 100, 150):
        assert cos(k) == pytest.approx(R.cosine_f64(k, 2e-4, 100, 1e-2), rel=1e-14)
        assert ex(k) == pytest.approx(R.exponential_f64(k, 1e-3, 10, 0.96), rel=1e-14)


def test_ipf_losses_name_themselves():
    from fbs_amd.sdes import StationaryConstLinearSDE, make_linear_sde_law_loss
    sde = StationaryConstLinearSDE(a=-0.5, b=1.)
    for lt in ('ipf', 'ipf-score'):
        with pytest.raises(NotImplementedError, match=lt):
            make_linear_sde_law_loss(sde, None, loss_type=lt)


def _small_unet():
    from fbs_amd.unet import UNet
    return UNet(dt=0.01, dim=8, in_channels=1, upsampling='pixel_shuffle', dim_mults=(1, 2))


def test_checkpoint_round_trip(tmp_path):
    """FlatParams -> export_flat_params order -> np.savez -> load_flat_params into a fresh UNet: bit-equal vectors."""
    import torch
    from fbs_amd.train import FlatParams, save_checkpoint
    torch.manual_seed(3)
    net = _small_unet()
    before = net.export_flat_params()
    fp = FlatParams(net)
    assert torch.equal(net.export_flat_params(), before) and torch.equal(fp.export(), before)
    assert all(p.data_ptr() == fp.flat.data_ptr() + 4 * o for p, o in zip(fp.params, fp.offsets))
    assert all(o % 4 == 0 for o in fp.offsets)
    ema = fp.flat * 0.5                                               # 0.5 x is exact
    path = str(tmp_path / "checkpoints" / "mnist_lin_0.npz")
    save_checkpoint(path, fp, ema)
    z = np.load(path)
    assert z["param"].dtype == np.float32 and z["param"].shape == (net.num_flat_params(),)
    fresh = _small_unet()
    fresh.load_flat_params(z["param"])
    assert torch.equal(fresh.export_flat_params(), before)
    fresh.load_flat_params(z["ema_param"])
    assert torch.equal(fresh.export_flat_params(), before * 0.5)


def test_flat_grads_alias_and_are_repaired():
    import torch
    from fbs_amd.train import FlatParams
    torch.manual_seed(4)
    net = _small_unet()
    fp = FlatParams(net)
    fp.zero_grad()
    net(torch.randn(2, 8, 8, 1), torch.tensor([0.3, 0.5])).square().sum().backward()
    assert fp.sync_grads() == 0 and float(fp.grad.abs().sum()) > 0
    want = fp.grad.clone()
    for p in fp.params[:3]:
        p.grad = p.grad.clone()                                       # break the aliasing
    fp.grad.zero_()
    for p, o in zip(fp.params[3:], fp.offsets[3:]):
        fp.grad[o:o + p.numel()].copy_(want[o:o + p.numel()])
    assert fp.sync_grads() == 3 and torch.equal(fp.grad, want)
    assert all(p.grad.data_ptr() == fp.grad.data_ptr() + 4 * o for p, o in zip(fp.params, fp.offsets))
    v = [p._version for p in fp.params]
    fp.mark_updated()
    assert all(p._version > v0 for p, v0 in zip(fp.params, v))


def test_reference_loss_vanishes_at_the_true_score():
    """The reference's own loss test: with nn the conditional score of a single x0 the loss is zero."""
    rng = np.random.default_rng(0)
    B, D = 6, 11
    x0 = np.tile(rng.normal(size=(1, D)), (B, 1)).astype(np.float32)
    F, sq, _ = R.lin_tables(np.linspace(0.1, 2.0, B), B * D)
    xt = F[:, None].astype(np.float64) * x0 + sq[:, None].astype(np.float64) * rng.normal(size=(B, D))
    Q = sq.astype(np.float64) ** 2
    net = R.cond_score_t_0(xt, F[:, None].astype(np.float64), Q[:, None], x0.astype(np.float64))
    assert R.loss_f64(net, xt, x0, F, sq) < 1e-12


def test_restatements_tell_the_mistakes_apart():
    rng = np.random.default_rng(1)
    B, D = 4, 9
    x0, net = rng.normal(size=(B, D)), rng.normal(size=(B, D))
    F, sq, _ = R.lin_tables([0.2, 0.6, 1.1, 2.0], B * D)
    xt = F[:, None] * x0 + sq[:, None] * rng.normal(size=(B, D))
    good = R.loss_f64(net, xt, x0, F, sq)
    for mistake in ('no_q', 'sq_for_q'):
        assert abs(R.loss_f64(net, xt, x0, F, sq, mistake) - good) > 1e-2 * good, mistake
    p, g, m, v = (rng.normal(size=50) for _ in range(4))
    v = v * v
    pg, mg, vg = R.adam_f64(p, g, m, v, 1e-2, 0.9, 0.999, 1e-2, 3)
    for mistake in ('eps_in_sqrt', 'count_from_1'):
        pb = R.adam_f64(p, g, m, v, 1e-2, 0.9, 0.999, 1e-2, 3, mistake)[0]
        assert np.max(np.abs((pb - p) - (pg - p)) / np.abs(pg - p)) > 1e-3, mistake
    big = 3.0 * g
    assert np.linalg.norm(R.clip_by_global_norm_f64(big, 1.0)) == pytest.approx(1.0, rel=1e-12)
    assert np.max(np.abs(R.clip_by_global_norm_f64(big, 1.0, 'by_value') - R.clip_by_global_norm_f64(big, 1.0))) > 0.1
    assert np.array_equal(R.clip_by_global_norm_f64(g * 1e-3, 1.0), g * 1e-3)
    assert [R.ema_mode_of(c, 3, 2) for c in range(7)] == [1, 1, 1, 0, 2, 0, 2]
    assert np.array_equal(R.ema_f64(m, p, 0, 0.9), m) and np.array_equal(R.ema_f64(m, p, 1, 0.9), p)
    np.testing.assert_allclose(R.ema_f64(m, p, 2, 0.9), 0.9 * m + 0.1 * p, rtol=1e-12)   # 1 - 0.9 is not 0.1 to the bit


def test_ema_kernel_chooses_the_reference_regimes():
    import torch
    from fbs_amd.train import make_adam_kernel
    lin = torch.nn.Linear(2, 2)
    _, ema_kernel = make_adam_kernel(lin, None, 1e-3)
    assert [ema_kernel(c, 3, 2, 0.99) for c in range(7)] == [R.ema_mode_of(c, 3, 2) for c in range(7)]


def test_closed_form_run_converges_in_float64():
    theta, first, last = R.closed_form_run()
    assert abs(theta - 1.0) < 1e-3 and last < 1e-4 * first
