"""GPU: fbsmi_normalise_batched / fbsmi_cond_killing_batched (one workgroup per ensemble, everything in LDS) against the CPU
oracle and against the single-ensemble entry points, bit for bit, at every size where the kernels change shape: one row,
below / at / above a wave, above a logsumexp tile (256), the largest ensemble (1024), one and many workgroups."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BS = (1, 3, 70)
NS = (1, 2, 63, 64, 65, 101, 257, 1024)
KINDS = ("collapsed", "equal", "spread", "zeros")


def _row(kind, n, rng):
    """Log-weights of one ensemble."""
    if kind == "collapsed":                       # one finite log-weight, the rest -inf
        lw = np.full(n, -np.inf, np.float32)
        lw[rng.integers(0, n)] = np.float32(rng.uniform(-30, 30))
        return lw
    if kind == "equal":
        return np.full(n, np.float32(rng.uniform(-5, 5)), np.float32)
    lw = rng.uniform(-40, 40, n).astype(np.float32)
    if kind == "zeros" and n > 1:                 # exact zero weights among positive ones
        dead = rng.random(n) < 0.35
        dead[rng.integers(0, n)] = False
        lw[dead] = -np.inf
    return lw


def _ensembles(B, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([_row(KINDS[(b + seed) % 4], n, rng) for b in range(B)], 0), rng


def _seeds(B):
    return range(4) if B == 1 else (B,)           # a single ensemble takes every kind in turn


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("B", BS)
def test_normalise_batched_equals_oracle(oracle, dev, B, n):
    from fbs_amd import ops
    for seed in _seeds(B):
        lw, _ = _ensembles(B, n, seed)
        t = torch.from_numpy(lw).to(dev)
        for log_space in (True, False):
            out, lse = ops.normalise_batched(t, log_space=log_space, return_lse=True)
            single = torch.stack([ops.normalise(t[b], log_space=log_space) for b in range(B)], 0)
            torch.cuda.synchronize()
            got, got_lse = out.cpu().numpy(), lse.cpu().numpy()
            for b in range(B):
                want = oracle.normalise(lw[b], log_space)
                assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), (B, n, b, log_space, seed)
                want_lse = np.float32(oracle.logsumexp(lw[b]))
                assert got_lse[b].view(np.uint32) == want_lse.view(np.uint32), (B, n, b, seed)
            assert torch.equal(out.view(torch.int32), single.view(torch.int32))
            assert torch.equal(ops.normalise_batched(t, log_space=log_space), out)      # out_lse is optional


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("B", BS)
def test_cond_killing_batched_equals_oracle_and_single(oracle, dev, B, n):
    from fbs_amd import ops
    from fbs_amd.samplers.csmc.resamplings import killing
    for seed in _seeds(B):
        lw, rng = _ensembles(B, n, seed)
        w = np.stack([oracle.normalise(lw[b], False) for b in range(B)], 0)
        if "zeros" in [KINDS[(b + seed) % 4] for b in range(B)] and n > 4:
            assert (w == 0).any()
        keys = oracle.split(oracle.PRNGKey(1000 + 17 * n + B + seed), B)               # distinct keys per ensemble
        i = rng.integers(0, n, B).astype(np.int32)
        j = rng.integers(0, n, B).astype(np.int32)
        i[0], j[0] = (0, n - 1) if seed % 2 == 0 else (n - 1, 0)
        if B > 1:
            i[1], j[1] = n - 1, 0
        wt = torch.from_numpy(w).to(dev)
        got = ops.cond_killing_batched(keys, wt, torch.from_numpy(i).to(dev), torch.from_numpy(j).to(dev))
        single = torch.stack([killing(keys[b], wt[b], int(i[b]), int(j[b]), True) for b in range(B)], 0)
        torch.cuda.synchronize()
        assert got.dtype == torch.int32 and got.shape == (B, n)
        g = got.cpu().numpy()
        for b in range(B):
            want = oracle.cond_killing(keys[b], w[b], int(i[b]), int(j[b]), True)
            assert np.array_equal(g[b], np.asarray(want, np.int32)), (B, n, b, seed)
            assert g[b, j[b]] == i[b]
        assert torch.equal(got, single)
        # the same keys as an int32 device tensor
        assert torch.equal(ops.cond_killing_batched(ops.keys_to_device(keys, dev), wt, torch.from_numpy(i).to(dev),
                                                    torch.from_numpy(j).to(dev)), got)
