"""GPU: fbsmi_resample_batched (one workgroup per ensemble, the CDF in LDS) against the CPU oracle and against the
single-ensemble resamplers, bit for bit, at every size where the LDS tree and the search change shape: one row, below / at /
above a wave, above a 256-element tile, the largest workgroup (1024), one and many workgroups."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BS = (1, 3, 70)
NS = (1, 2, 63, 64, 65, 101, 257, 1024)
KINDS = ("collapsed", "equal", "spread", "zeros")         # the weight kinds of tests/test_gpu_batched_prims.py


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


def _weights(oracle, B, n, seed):
    rng = np.random.default_rng(seed)
    kinds = [KINDS[(b + seed) % 4] for b in range(B)]
    w = np.stack([oracle.normalise(_row(k, n, rng), False) for k in kinds], 0)
    if "zeros" in kinds and n > 4:
        assert (w == 0).any()
    return w


def _seeds(B):
    return range(4) if B == 1 else (B,)           # a single ensemble takes every kind in turn


@pytest.mark.parametrize("kind", ("stratified", "systematic"))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("B", BS)
def test_resample_batched_equals_oracle_and_single(oracle, dev, B, n, kind):
    from fbs_amd import ops
    from fbs_amd import samplers
    single_fn, oracle_fn = getattr(samplers, kind), getattr(oracle, kind)
    for seed in _seeds(B):
        w = _weights(oracle, B, n, seed)
        keys = oracle.split(oracle.PRNGKey(2000 + 17 * n + B + seed), B)               # distinct keys per ensemble
        assert len({tuple(k) for k in keys}) == B
        wt = torch.from_numpy(w).to(dev)
        got = ops.resample_batched(wt, keys, kind)
        single = torch.stack([single_fn(wt[b], keys[b]) for b in range(B)], 0)
        on_device = ops.resample_batched(wt, ops.keys_to_device(keys, dev), kind)      # the same keys as a device tensor
        torch.cuda.synchronize()
        assert got.dtype == torch.int32 and got.shape == (B, n)
        g = got.cpu().numpy()
        assert g.min() >= 0 and g.max() < n
        for b in range(B):
            want = np.asarray(oracle_fn(w[b], keys[b]), np.int32)
            assert np.array_equal(g[b], want), (kind, B, n, b, seed)
        assert np.array_equal(g, single.cpu().numpy().astype(np.int32)), (kind, B, n, seed)
        assert torch.equal(on_device, got)


def test_resample_batched_refuses_what_has_no_kernel(dev):
    from fbs_amd import ops
    w = torch.full((2, 8), 0.125, device=dev)
    keys = ops.split(ops.PRNGKey(1), 2)
    for kind in ("multinomial", "killing"):
        with pytest.raises(RuntimeError):
            ops.resample_batched(w, keys, kind)
    with pytest.raises(ValueError):
        ops.resample_batched(w, keys, "residual")
    with pytest.raises(ValueError):
        ops.resample_batched(w[0], keys, "stratified")
    with pytest.raises(ValueError):
        ops.resample_batched(w, keys[:1], "stratified")
