"""GPU: fbsmi_em_propose_batched -- the proposal half of a weight -> resample -> propose step, reading the network's output
rows through the ancestors -- against oracle/em.py and against the single-ensemble fbsmi_em_finish(net_A = A), ensemble by
ensemble and bit for bit; ScoreBridge.fused_weight_then_propose_batched against fused_weight_then_propose with one network
evaluation per step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TASKS = {"inpaint-3": (8, 8, 1), "supr-2": (6, 6, 3)}
COEF = dict(cx=np.float32(0.3), cs=np.float32(1.2), dt=np.float32(0.002), sd=np.float32(0.07))


def _setup(oracle, dev, task, B, shared):
    from fbs_amd.images import ImageRestore
    from fbs_amd.score import EMMask, EMMaskBatch
    from oracle import em
    shape = TASKS[task]
    ds = ImageRestore(task, shape, device=dev)
    masks = [ds.gen_mask(oracle.PRNGKey(40 + b)) for b in range(1 if shared else B)]
    ems = [EMMask(m, shape[2], dev) for m in masks]
    tabs = [em.element_tables(m.unobs_inds_ravelled.cpu().numpy(), m.obs_inds_ravelled.cpu().numpy(), shape[2])
            for m in masks]
    return EMMaskBatch(ems), ems, tabs


def _bf16_tensor(bits, dev):
    return torch.from_numpy(bits.view(np.int16)).to(dev).view(torch.bfloat16)


def _ancestors(which, B, n, rng):
    if which == "random":                                # with repeats
        return rng.integers(0, n, (B, n)).astype(np.int32)
    if which == "constant":                              # every row the same ancestor, another one per ensemble
        return np.repeat(rng.integers(0, n, (B, 1)), n, 1).astype(np.int32)
    return np.tile(np.arange(n - 1, -1, -1, dtype=np.int32), (B, 1))      # reversed


def _check(oracle, dev, task, B, n, shared=False):
    from fbs_amd import _lib
    from oracle import em
    mb, ems, tabs = _setup(oracle, dev, task, B, shared)
    one = lambda b: 0 if shared else b
    assert mb.nmasks == (1 if shared else B)
    du, D = mb.du, mb.D
    rng = np.random.default_rng(100 * B + n)
    us = rng.normal(size=(B, n, du)).astype(np.float32)
    net32 = rng.normal(size=(B * n, D)).astype(np.float32)                # a stand-in network output, distinct rows
    keys = oracle.split(oracle.PRNGKey(9 + n), B)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ust, kt = t(us), t(keys.view(np.int32))
    c = [float(COEF[k]) for k in ("cx", "cs", "dt", "sd")]
    for which in ("random", "constant", "reversed"):
        A = _ancestors(which, B, n, rng)
        At = t(A)
        for net_dt in (0, 1):
            if net_dt == 0:
                net_t, net_host = t(net32), net32
            else:
                bits = em.to_bf16_bits(net32)
                net_t, net_host = _bf16_tensor(bits, dev), em.from_bf16_bits(bits)
            for mode in (0, 1):
                un = torch.full((B, n, du), float("nan"), device=dev)
                _lib.call("fbsmi_em_propose_batched", mb.ref, ust.data_ptr(), At.data_ptr(), net_t.data_ptr(), net_dt, mode,
                          *c, kt.data_ptr(), B, n, un.data_ptr(), 0)
                single = torch.full((B, n, du), float("nan"), device=dev)
                for b in range(B):
                    net_b = net_t[b * n:(b + 1) * n]
                    _lib.call("fbsmi_em_finish", ems[one(b)].ref, ust[b].data_ptr(), At[b].data_ptr(), net_b.data_ptr(),
                              At[b].data_ptr(), net_dt, mode, *c, None, None, int(keys[b][0]), int(keys[b][1]), n, 0, n, -1,
                              None, single[b].data_ptr(), None, 0)
                torch.cuda.synchronize()
                gun = un.cpu().numpy()
                for b in range(B):
                    u_off, v_off, _ = tabs[one(b)]
                    wun, _ = em.finish(us[b], A[b], net_host[b * n:(b + 1) * n][A[b]], mode, COEF["cx"], COEF["cs"],
                                       COEF["dt"], COEF["sd"], None, None, keys[b], n, 0, None, None, u_off, v_off,
                                       want_lw=False)
                    where = (task, B, n, b, which, net_dt, mode)
                    assert np.array_equal(gun[b].view(np.uint32), wun.view(np.uint32)), ("oracle", where)
                assert torch.equal(un.view(torch.int32), single.view(torch.int32)), ("single", task, B, n, which, net_dt, mode)


@pytest.mark.parametrize("n", (1, 5, 65))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("task", sorted(TASKS))
def test_em_propose_batched_equals_oracle_and_single(oracle, dev, task, B, n):
    _check(oracle, dev, task, B, n)


@pytest.mark.parametrize("task", sorted(TASKS))
def test_em_propose_batched_shared_mask(oracle, dev, task):
    """nmasks = 1: one mask for all three ensembles."""
    _check(oracle, dev, task, 3, 5, shared=True)


def test_em_propose_batched_clamps_the_ancestors(oracle, dev):
    """Ancestors outside the ensemble are clamped into it before they address us or net, as in the other batched kernels."""
    from fbs_amd import _lib
    mb, _, _ = _setup(oracle, dev, "inpaint-3", 2, False)
    B, n = 2, 5
    g = torch.Generator(device="cpu").manual_seed(5)
    us = torch.randn((B, n, mb.du), generator=g).to(dev)
    net = torch.randn((B * n, mb.D), generator=g).to(dev)
    keys = torch.from_numpy(oracle.split(oracle.PRNGKey(4), B).view(np.int32)).to(dev)
    wild = torch.tensor([[-3, 0, 7, 4, 100], [5, -1, 2, 9, 1]], dtype=torch.int32, device=dev)
    c = [float(COEF[k]) for k in ("cx", "cs", "dt", "sd")]
    outs = []
    for A in (wild, wild.clamp(0, n - 1)):
        un = torch.full((B, n, mb.du), float("nan"), device=dev)
        _lib.call("fbsmi_em_propose_batched", mb.ref, us.data_ptr(), A.data_ptr(), net.data_ptr(), 0, 0, *c, keys.data_ptr(),
                  B, n, un.data_ptr(), 0)
        outs.append(un)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("shared", (False, True))
def test_fused_weight_then_propose_batched_equals_the_single_method(oracle, dev, shared):
    """A row-wise stand-in score, chunks of 7 rows straddling ensembles of 5: every ensemble has the bits of its own
    fused_weight_then_propose, and the network runs once per step -- ceil(B n / chunk) calls, not twice that."""
    from fbs_amd import ops
    from fbs_amd.images import ImageRestore
    from fbs_amd.samplers import stratified
    from fbs_amd.score import ScoreBridge
    from fbs_amd.sdes import StationaryLinLinearSDE
    B, n, T = 3, 5, 4
    ts = np.linspace(0, 2.0, T + 1)
    sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=2.0)
    ds = ImageRestore("inpaint-3", (8, 8, 1), device=dev)
    calls = []
    sb = ScoreBridge(lambda x, t: (calls.append(x.shape[0]), (0.25 * x.roll(1, 2) - 0.5 * x) * t)[1], ds, sde, ts, chunk=7)
    masks = [ds.gen_mask(oracle.PRNGKey(60 + (0 if shared else b))) for b in range(B)]
    if shared:
        masks = [masks[0]] * B
    g = torch.Generator(device="cpu").manual_seed(3)
    us = torch.randn((B, n, 9, 1), generator=g).to(dev)
    v, vp = torch.randn((B, 55, 1), generator=g).to(dev), torch.randn((B, 55, 1), generator=g).to(dev)
    keys = oracle.split(oracle.PRNGKey(78), B)
    kres = oracle.split(oracle.PRNGKey(79), B)

    def resample(lw):
        return ops.resample_batched(ops.normalise_batched(lw), kres, "stratified")

    un, lw, inds = sb.fused_weight_then_propose_batched(us, v, vp, ts[1], keys, masks[0] if shared else masks, resample)
    assert calls == [7, 7, 1], calls                                      # one evaluation of the 15 rows
    assert un.shape == (B, n, 9, 1) and lw.shape == (B, n) and inds.shape == (B, n) and inds.dtype == torch.int32
    del calls[:]
    for b in range(B):
        wun, wlw, winds = sb.fused_weight_then_propose(us[b], v[b], vp[b], ts[1], keys[b], masks[b],
                                                       lambda l: stratified(ops.normalise(l), kres[b]))
        assert torch.equal(inds[b], winds), b
        assert torch.equal(lw[b].view(torch.int32), wlw.view(torch.int32)), b
        assert torch.equal(un[b].view(torch.int32), wun.view(torch.int32)), b
    assert calls == [5] * B
