"""GPU: fbsmi_em_concat_batched / fbsmi_em_finish_batched against oracle/em.py, ensemble by ensemble and bit for bit -- the
comparison smoke() makes for the single-ensemble step.  inpaint-3 on (8, 8, 1) has du = 9, so n * du is odd for odd n (the
tail of the paired Threefry draw); supr-2 on (6, 6, 3) has a different random mask per ensemble."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TASKS = {"inpaint-3": (8, 8, 1), "supr-2": (6, 6, 3)}
LONG = {"inpaint-4": (20, 20, 3)}          # dv = 1152: five 256-element segments, two rounds of the workgroup
COEF = dict(cx=np.float32(0.3), cs=np.float32(1.2), dt=np.float32(0.002), sd=np.float32(0.07))


def _setup(oracle, dev, task, B, shared):
    from fbs_amd.images import ImageRestore
    from fbs_amd.score import EMMask, EMMaskBatch
    from oracle import em
    shape = {**TASKS, **LONG}[task]
    ds = ImageRestore(task, shape, device=dev)
    masks = [ds.gen_mask(oracle.PRNGKey(40 + b)) for b in range(1 if shared else B)]
    if task == "supr-2" and not shared and B > 1:
        assert not torch.equal(masks[0].unobs_inds_ravelled, masks[1].unobs_inds_ravelled)
    mb = EMMaskBatch([EMMask(m, shape[2], dev) for m in masks])
    tabs = [em.element_tables(m.unobs_inds_ravelled.cpu().numpy(), m.obs_inds_ravelled.cpu().numpy(), shape[2])
            for m in masks]
    return mb, (lambda b: tabs[0 if shared else b])


def _bf16_tensor(bits, dev):
    return torch.from_numpy(bits.view(np.int16)).to(dev).view(torch.bfloat16)


def _check(oracle, dev, task, B, n, shared=False):
    from fbs_amd import _lib
    from oracle import em
    mb, tab = _setup(oracle, dev, task, B, shared)
    assert mb.nmasks == (1 if shared else B)
    du, dv, D = mb.du, mb.dv, mb.D
    rng = np.random.default_rng(100 * B + n)
    us = rng.normal(size=(B, n, du)).astype(np.float32)
    v, vp = rng.normal(size=(B, dv)).astype(np.float32), rng.normal(size=(B, dv)).astype(np.float32)
    A = rng.integers(0, n, (B, n)).astype(np.int32)
    keys = oracle.split(oracle.PRNGKey(7 + n), B)
    pin_row = np.array([(0, n - 1, -1)[b % 3] for b in range(B)], np.int32)          # mixed within one call
    pin_val = rng.normal(size=(B, du)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ust, vt, vpt, At, prt, pvt = t(us), t(v), t(vp), t(A), t(pin_row), t(pin_val)
    kt = t(keys.view(np.int32))
    ptr = lambda x: x.data_ptr() if x is not None else None

    for use_A in (True, False):
        Ab = A if use_A else None
        want_img = np.concatenate([em.concat(us[b], None if Ab is None else Ab[b], vp[b], tab(b)[2]) for b in range(B)], 0)
        for out_dt in (0, 1):
            img = torch.empty((B * n, D), dtype=torch.float32 if out_dt == 0 else torch.bfloat16, device=dev)
            _lib.call("fbsmi_em_concat_batched", mb.ref, ust.data_ptr(), ptr(At if use_A else None), vpt.data_ptr(), B, n,
                      out_dt, img.data_ptr(), 0)
            torch.cuda.synchronize()
            if out_dt == 0:
                assert np.array_equal(img.cpu().numpy().view(np.uint32), want_img.view(np.uint32)), "concat f32"
            else:
                assert np.array_equal(img.view(torch.int16).cpu().numpy().view(np.uint16), em.to_bf16_bits(want_img)), "concat bf16"
        net32 = (want_img * np.float32(0.5) + np.float32(0.125)).astype(np.float32)   # a stand-in network output
        for net_dt in (0, 1):
            if net_dt == 0:
                net_t, net_host = t(net32), net32
            else:
                bits = em.to_bf16_bits(net32)
                net_t, net_host = _bf16_tensor(bits, dev), em.from_bf16_bits(bits)
            for mode in (0, 1):
                un = torch.full((B, n, du), float("nan"), device=dev)
                lw = torch.full((B, n), float("nan"), device=dev)
                _lib.call("fbsmi_em_finish_batched", mb.ref, ust.data_ptr(), ptr(At if use_A else None), net_t.data_ptr(),
                          net_dt, mode, float(COEF["cx"]), float(COEF["cs"]), float(COEF["dt"]), float(COEF["sd"]),
                          vt.data_ptr(), vpt.data_ptr(), kt.data_ptr(), B, n, prt.data_ptr(), pvt.data_ptr(), un.data_ptr(),
                          lw.data_ptr(), 0)
                torch.cuda.synchronize()
                gun, glw = un.cpu().numpy(), lw.cpu().numpy()
                for b in range(B):
                    wun, wlw = em.finish(us[b], None if Ab is None else Ab[b], net_host[b * n:(b + 1) * n], mode, COEF["cx"],
                                         COEF["cs"], COEF["dt"], COEF["sd"], v[b], vp[b], keys[b], n, 0, int(pin_row[b]),
                                         pin_val[b], tab(b)[0], tab(b)[1])
                    where = (task, B, n, b, use_A, net_dt, mode)
                    assert np.array_equal(gun[b].view(np.uint32), wun.view(np.uint32)), ("particles", where)
                    assert np.array_equal(glw[b].view(np.uint32), wlw.view(np.uint32)), ("log-weights", where)
                    if pin_row[b] >= 0:
                        assert np.array_equal(gun[b, pin_row[b]], pin_val[b])
    # a weights-only call: no us_new, no keys, no pins
    lw = torch.full((B, n), float("nan"), device=dev)
    net_t = t(net32)
    _lib.call("fbsmi_em_finish_batched", mb.ref, ust.data_ptr(), None, net_t.data_ptr(), 0, 0, float(COEF["cx"]),
              float(COEF["cs"]), float(COEF["dt"]), float(COEF["sd"]), vt.data_ptr(), vpt.data_ptr(), None, B, n, None, None,
              None, lw.data_ptr(), 0)
    torch.cuda.synchronize()
    for b in range(B):
        _, wlw = em.finish(None, None, net32[b * n:(b + 1) * n], 0, COEF["cx"], COEF["cs"], COEF["dt"], COEF["sd"], v[b],
                           vp[b], None, n, 0, None, None, tab(b)[0], tab(b)[1], want_us=False)
        assert np.array_equal(lw[b].cpu().numpy().view(np.uint32), wlw.view(np.uint32)), ("weights only", task, B, n, b)


@pytest.mark.parametrize("n", (1, 5, 64, 101))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("task", sorted(TASKS))
def test_em_batched_equals_oracle(oracle, dev, task, B, n):
    _check(oracle, dev, task, B, n)


def test_em_batched_shared_mask(oracle, dev):
    """nmasks = 1: one mask for all three ensembles."""
    _check(oracle, dev, "inpaint-3", 3, 5, shared=True)


def test_em_batched_long_observed_part(oracle, dev):
    """An observed part longer than one round of the workgroup (1024 elements): the segment sums meet in the LDS tree."""
    _check(oracle, dev, "inpaint-4", 2, 3)


def test_fused_step_batched_equals_fused_step(oracle, dev):
    """ScoreBridge.fused_step_batched with a row-wise stand-in score, chunks that straddle ensembles: every ensemble has
    the bits of its own fused_step."""
    from fbs_amd.images import ImageRestore
    from fbs_amd.score import ScoreBridge
    from fbs_amd.sdes import StationaryLinLinearSDE
    B, n, T = 3, 5, 4
    ts = np.linspace(0, 2.0, T + 1)
    sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=2.0)
    ds = ImageRestore("inpaint-3", (8, 8, 1), device=dev)
    calls = []
    sb = ScoreBridge(lambda x, t: (calls.append(x.shape[0]), (0.25 * x.roll(1, 2) - 0.5 * x) * t)[1], ds, sde, ts, chunk=7)
    masks = [ds.gen_mask(oracle.PRNGKey(60 + b)) for b in range(B)]
    g = torch.Generator(device="cpu").manual_seed(3)
    us = torch.randn((B, n, 9, 1), generator=g).to(dev)
    v, vp = torch.randn((B, 55, 1), generator=g).to(dev), torch.randn((B, 55, 1), generator=g).to(dev)
    A = torch.randint(0, n, (B, n), generator=g).to(torch.int32).to(dev)
    pin_val = torch.randn((B, 9, 1), generator=g).to(dev)
    pin_row = torch.tensor([0, n - 1, -1], dtype=torch.int32, device=dev)
    keys = oracle.split(oracle.PRNGKey(77), B)
    un, lw = sb.fused_step_batched(us, A, v, vp, ts[1], keys, masks, pins=(pin_row, pin_val))
    assert calls == [7, 7, 1] and un.shape == (B, n, 9, 1) and lw.shape == (B, n)
    for b in range(B):
        pin = None if int(pin_row[b]) < 0 else (int(pin_row[b]), pin_val[b])
        wun, wlw = sb.fused_step(us[b], A[b], v[b], vp[b], ts[1], keys[b], masks[b], pin=pin)
        assert torch.equal(un[b].view(torch.int32), wun.view(torch.int32)), b
        assert torch.equal(lw[b].view(torch.int32), wlw.view(torch.int32)), b
    none, lw0 = sb.fused_step_batched(us, None, v, vp, ts[0], None, masks, want_us=False)
    assert none is None
    for b in range(B):
        assert torch.equal(lw0[b], sb.likelihood_logpdf(v[b], us[b], vp[b], ts[0], masks[b]))
