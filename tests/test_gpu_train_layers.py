"""GPU: the score-matching trainer through its layers -- the loss on the autograd tape, a training run with a closed form,
one step on the smallest UNet in both layouts, the inference caches after a fused update, and examples/imgs_train.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import train_restate as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-5


def _const_sde():
    from fbs_amd.sdes import StationaryConstLinearSDE
    return StationaryConstLinearSDE(a=-0.5, b=1.)


@pytest.mark.parametrize("save_mem", [True, False], ids=["save_mem", "paths"])
@pytest.mark.parametrize("with_idx", [False, True], ids=["all", "idx"])
def test_parameter_gradients_through_the_function(dev, save_mem, with_idx):
    """A linear nn_fn with three parameters: their gradients through the autograd.Function against a float64 torch
    evaluation of the reference's formula (linear.py:338-340) on the same x_t.  Fixed time grids: t >= 0.4."""
    from fbs_amd import ops
    from fbs_amd.sdes import make_linear_sde_law_loss
    rng = np.random.default_rng(5)
    data = torch.from_numpy(rng.uniform(0.2, 1.0, (7, 4, 3, 1)).astype(np.float32)).to(dev)
    idx = torch.tensor([3, 0, 3, 6, 1], dtype=torch.int32, device=dev) if with_idx else None
    n = 5 if with_idx else 7

    def nn_fn(x, t, param):
        tt = t.to(x.dtype).reshape((-1,) + (1,) * (x.dim() - 1))
        return param[0] * x + param[1] + param[2] * tt

    loss_fn = make_linear_sde_law_loss(_const_sde(), nn_fn, t0=0., T=2., nsteps=3, random_times=False, save_mem=save_mem)
    param = torch.tensor([0.7, 0.3, -0.2], dtype=torch.float32, device=dev, requires_grad=True)
    rec = {}
    loss = loss_fn(param, ops.PRNGKey(11), data, idx, debug=rec)
    assert loss.dim() == 0 and loss.is_cuda and loss.requires_grad
    loss.backward()
    rows = rec["xt"].shape[0]
    assert rows == (n if save_mem else 3 * n)
    # float64, the reference's form: mean_b(mean_e((net - cond_score)^2) Q_b)
    xt = rec["xt"].double().reshape(rows, -1)
    flat = data.double().reshape(7, -1)
    x0 = flat[idx.long()] if with_idx else flat[:n]
    if not save_mem:
        x0 = x0.repeat(3, 1)                                   # rows are ordered (step, sample)
    F, Q, t = rec["F"].double(), rec["sq"].double() ** 2, rec["ts"].double()
    p64 = param.detach().double().requires_grad_(True)
    net = nn_fn(xt, t, p64)
    cs = -(xt - F[:, None] * x0) / Q[:, None]
    ref = torch.mean(torch.mean((net - cs) ** 2, dim=1) * Q)
    ref.backward()
    rl = abs(float(loss.detach()) - float(ref.detach())) / float(ref.detach())
    rg = (param.grad.double() - p64.grad).abs() / p64.grad.abs()
    print(f"save_mem={save_mem} idx={with_idx}: loss rel {rl:.2e}, gradient rel {rg.cpu().numpy()}")
    assert rl < REL and float(rg.max()) < REL
    # the row sums the kernel kept are the rows of the same formula
    S = rec["row_sums"].double() / xt.shape[1]
    want = torch.mean((net - cs) ** 2, dim=1) * Q
    assert float(((S - want.detach()).abs() / want.detach()).max()) < REL


class _ThetaModel(torch.nn.Module):
    """nn(x, t) = -(x - F(t) theta) / Q(t) for the constant SDE a = -0.5, b = 1: F = exp(-t / 2), Q = 1 - exp(-t)."""

    def __init__(self):
        super().__init__()
        self.theta = torch.nn.Parameter(torch.zeros(()))

    def forward(self, x, t):
        shp = (-1,) + (1,) * (x.dim() - 1)
        F, Q = torch.exp(-0.5 * t).reshape(shp), (1.0 - torch.exp(-t)).reshape(shp)
        return -(x - F * self.theta) / Q


def test_closed_form_training_run(dev):
    """Every data row is c = 1: the loss is (theta - c)^2 mean(F^2 / Q), the noise cancels.  200 adam steps at lr 0.05 from
    theta = 0 (the float64 restatement reaches |theta - c| = 2.8e-5 and a loss ratio of 8e-10)."""
    from fbs_amd import ops
    from fbs_amd.sdes import make_linear_sde_law_loss
    from fbs_amd.train import make_adam_kernel
    model = _ThetaModel().to(dev)
    loss_fn = make_linear_sde_law_loss(_const_sde(), lambda x, t, param: model(x, t), t0=0., T=2., random_times=False,
                                       save_mem=True)
    step, _ = make_adam_kernel(model, loss_fn, 0.05)
    data = torch.ones((8, 4, 4, 1), dtype=torch.float32, device=dev)
    losses = [step(k, data) for k in ops.split(ops.PRNGKey(1), 200)]
    first, last = float(losses[0]), float(loss_fn(None, ops.PRNGKey(2), data).detach())
    theta = float(model.theta.detach())
    ts = np.linspace(0.25, 2.0, 8)
    w = float(np.mean(np.exp(-ts) / (1 - np.exp(-ts))))
    print(f"theta {theta:.8f}, first loss {first:.6g} (closed form {w:.6g}), last {last:.3g}, ratio {last / first:.3g}")
    assert abs(first - w) < 1e-5 * w                           # theta = 0, c = 1: the closed form itself
    assert abs(theta - 1.0) < 1e-3 and last < 1e-4 * first
    assert step.state["count"] == 200


def _small_unet(dev, seed):
    from fbs_amd.unet import UNet
    torch.manual_seed(seed)
    return UNet(dt=0.01, dim=8, in_channels=1, upsampling='pixel_shuffle', dim_mults=(1, 2)).to(dev)


def _forward(net, x, t, bf16):
    net.eval()
    with torch.no_grad():
        if bf16:
            with torch.autocast('cuda', dtype=torch.bfloat16):
                return net(x, t).float()
        return net(x, t)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("save_mem", [True, False], ids=["save_mem", "paths"])
def test_one_unet_step_and_the_caches_after_it(dev, tmp_path, save_mem, bf16):
    """One step on the smallest UNet the class builds (8 x 8 x 1, batch 4): a finite loss, every parameter changed; then a
    no-grad forward of the trained module equals, bit for bit, that of a fresh module loaded from the saved checkpoint --
    although the same module's inference caches were filled before the update, which torch's version counters never saw."""
    from fbs_amd import ops
    from fbs_amd.sdes import StationaryLinLinearSDE, make_linear_sde_law_loss
    from fbs_amd.train import make_adam_kernel, save_checkpoint
    net = _small_unet(dev, 21)
    rng = np.random.default_rng(8)
    data = torch.from_numpy(rng.uniform(0, 1, (16, 8, 8, 1)).astype(np.float32)).to(dev)
    x, t = torch.from_numpy(rng.normal(size=(4, 8, 8, 1)).astype(np.float32)).to(dev), torch.tensor([0.1, 0.5, 1.0, 1.9], device=dev)
    sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5., t0=0., T=2.)
    lib_convs = torch.backends.cudnn.enabled

    def nn_fn(x_, t_, p_):
        # the differentiable pass: grad on (so unet.py keeps libfbsmi's network kernels out), library convolutions off
        assert torch.is_grad_enabled() and not torch.backends.cudnn.enabled
        return net(x_, t_)

    loss_fn = make_linear_sde_law_loss(sde, nn_fn, t0=0., T=2., nsteps=2, random_times=True, save_mem=save_mem)
    step, ema_kernel = make_adam_kernel(net, loss_fn, 1e-3, grad_clip=1.0)
    fp = step.params
    before = fp.flat.clone()
    # fill the per-version weight caches now that the parameters live in the flat buffer (the caches are keyed by address
    # and by compute dtype too, one slot each): from here to the forward after the step nothing but the fused update's raw
    # pointer writes the weights, and the forward after it asks for the same dtype
    stale = _forward(net, x, t, bf16)
    ema_kernel(0, 300, 2, 0.99)
    idx = torch.tensor([9, 2, 15, 4], dtype=torch.int32, device=dev)
    loss = step(ops.PRNGKey(3), data, idx)
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    assert torch.backends.cudnn.enabled == lib_convs
    for (name, p), o in zip(net.named_parameters(), fp.offsets):
        assert not torch.equal(fp.flat[o:o + p.numel()], before[o:o + p.numel()]), name
    assert torch.equal(step.state["ema"], fp.flat)                      # count 0 < 300: the EMA is the new parameters
    assert bool(torch.isfinite(fp.flat).all()) and float(step.state["gnorm2"]) > 0
    path = str(tmp_path / "ck" / "mnist_lin_0.npz")
    save_checkpoint(path, fp, step.state["ema"])
    fresh = _small_unet(dev, 99)
    fresh.load_flat_params(np.load(path)["param"])
    got, want = _forward(net, x, t, bf16), _forward(fresh, x, t, bf16)
    assert got.dtype == want.dtype and got.device == want.device
    assert torch.equal(got, want), "stale inference weights after the fused update"
    assert not torch.equal(got, stale)


def test_imgs_train_example_writes_a_loadable_checkpoint(dev, tmp_path):
    spec = importlib.util.spec_from_file_location("imgs_train", os.path.join(ROOT, "examples", "imgs_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ck = mod.main(["--synthetic", "32", "--nepochs", "1", "--resolution", "8", "--dim", "8", "--dim_mults", "1,2",
                   "--batch_size", "4", "--save_mem", "--grad_clip", "--check_nsteps", "4", "--ckpt_dir", str(tmp_path / "ck"),
                   "--outdir", str(tmp_path / "figs"), "--quiet"])
    assert ck is not None and os.path.basename(ck) == "mnist_lin_0.npz"
    z = np.load(ck)
    fresh = _small_unet(dev, 1)
    for name in ("param", "ema_param"):
        assert z[name].dtype == np.float32 and np.all(np.isfinite(z[name]))
        fresh.load_flat_params(z[name])
        assert np.array_equal(fresh.export_flat_params().numpy(), z[name])
    out = np.load(str(tmp_path / "figs" / "mnist_lin_backward_test.npy"))
    assert out.shape == (7, 8, 8, 1) and np.all(np.isfinite(out))
