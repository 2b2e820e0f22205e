"""CPU: the host side of the Gibbs sweeps batched under every flag -- the four new entry points of fbs_amd/csrc/fbsmi_batch.hip
are exported and refuse bad calls before any HIP call, the key schedule of ``explicit_backward=False`` equals the oracle's
chain of splits for ``csmc_kernel`` while the default call returns the dictionary it always did, the group planner of the
stored-particle cap, and the reference chains of the GPU anchor test agree with themselves."""
import ctypes

import numpy as np
import pytest

ARG, UNSUPPORTED = -1, -3
P = 0x1000          # a non-null pointer value: the refusals below never dereference it
NAMES = ("fbsmi_force_move_batched", "fbsmi_randint_batched", "fbsmi_backscan_batched", "fbsmi_affine_em_path_batched")


def test_library_has_the_four_symbols():
    from fbs_amd import _lib
    L = ctypes.CDLL(_lib.build())
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES
    assert _lib.lib().fbsmi_abi_version() == 1


def test_force_move_and_randint_refusals():
    from fbs_amd import _lib
    L = _lib.lib()
    fm, ri = L.fbsmi_force_move_batched, L.fbsmi_randint_batched
    assert fm(P, P, P, 3, 1025, P, None, None) == UNSUPPORTED and b"1024" in L.fbsmi_last_error()
    assert fm(P, P, P, 0, 8, P, None, None) == ARG
    assert fm(P, P, P, 3, 0, P, P, None) == ARG
    assert fm(P, P, P, 2 ** 31, 8, P, None, None) == ARG
    for hole in range(3):
        a = [P, P, P]
        a[hole] = None
        assert fm(*a, 3, 8, P, None, None) == ARG
    assert fm(P, P, P, 3, 8, None, None, None) == ARG
    assert ri(P, 0, 8, 0, 5, P, None) == ARG
    assert ri(P, 3, -1, 0, 5, P, None) == ARG
    assert ri(None, 3, 8, 0, 5, P, None) == ARG
    assert ri(P, 3, 8, 0, 5, None, None) == ARG
    assert ri(P, 3, 2 ** 32 - 3, 0, 5, P, None) == ARG
    assert ri(P, 2 ** 31 - 1, 257, 0, 5, P, None) == ARG          # two workgroups per row: too many for one grid
    assert ri(P, 3, 0, 0, 5, None, None) == 0                     # nothing to draw, nothing launched


def test_backscan_and_bridge_path_refusals():
    from fbs_amd import _lib
    L = _lib.lib()
    bs, ap = L.fbsmi_backscan_batched, L.fbsmi_affine_em_path_batched

    def backscan(keys=P, lw=P, As=P, uss=P, B=3, n=8, T=4, du=9, Bs=P, path=P):
        return bs(keys, lw, As, uss, B, n, T, du, Bs, path, None)

    assert backscan(n=1025) == UNSUPPORTED and b"1024" in L.fbsmi_last_error()
    for name in ("keys", "lw", "As", "uss", "Bs", "path"):
        assert backscan(**{name: None}) == ARG, name
    for name in ("B", "n", "du"):
        assert backscan(**{name: 0}) == ARG, name
    assert backscan(T=-1) == ARG

    def path(keys=P, A=P, Bt=P, S=P, ddt=P, target=P, x0=P, T=4, nsub=3, D=9, B=3, out=P, slot=27, ens=9):
        return ap(keys, A, Bt, S, ddt, target, x0, T, nsub, D, 1, B, out, slot, ens, 1, None)

    for name in ("keys", "A", "Bt", "S", "ddt", "target", "x0", "out"):
        assert path(**{name: None}) == ARG, name
    assert path(T=-1) == ARG and path(nsub=0) == ARG and path(D=0) == ARG and path(B=0) == ARG
    assert path(nsub=2 ** 20, D=2 ** 12) == ARG                   # an interval's draw of 2^32 elements
    assert path(slot=-1) == ARG and path(ens=-1) == ARG
    assert path(B=2 ** 31 - 1, D=65) == ARG                       # two workgroups per ensemble: too many for one grid


def test_key_schedule_without_explicit_backward_equals_the_oracles_splits(oracle):
    """gibbs.py:126, csmc.py:29 (csmc_kernel), :150, :157, :136 for B = 3 sweeps of T = 4 steps, by the oracle's split."""
    from fbs_amd import ops
    from fbs_amd.samplers.gibbs_batched import sweep_key_schedule
    B, T = 3, 4
    keys = ops.split(ops.PRNGKey(2025), B)
    sk = sweep_key_schedule(keys, T, explicit_backward=False)
    assert set(sk) == {"fwd", "bridge", "bwd", "init", "resampling", "transition"}
    assert sk["resampling"].shape == (T, B, 2) and sk["transition"].shape == (T, B, 2)
    assert all(a.dtype == np.uint32 for a in sk.values())
    for b in range(B):
        key_fwd, key_csmc, key_bridge = oracle.split(keys[b], 3)                  # gibbs.py:126
        k_fwd, k_bwd = oracle.split(key_csmc, 2)                                  # csmc.py:29
        key_init, key_scan = oracle.split(k_fwd, 2)                               # :150
        step = oracle.split(key_scan, T)                                          # :157
        for name, want in (("fwd", key_fwd), ("bridge", key_bridge), ("bwd", k_bwd), ("init", key_init)):
            np.testing.assert_array_equal(sk[name][b], want, err_msg=name)
        for k in range(T):
            k_res, k_tr = oracle.split(step[k], 2)                                # :136
            np.testing.assert_array_equal(sk["resampling"][k, b], k_res)
            np.testing.assert_array_equal(sk["transition"][k, b], k_tr)


def test_default_key_schedule_is_unchanged(oracle):
    from fbs_amd import ops
    from fbs_amd.samplers.gibbs_batched import sweep_key_schedule
    B, T = 2, 3
    keys = ops.split(ops.PRNGKey(7), B)
    sk = sweep_key_schedule(keys, T)
    assert list(sk) == ["fwd", "bridge", "x0", "us", "bs", "init", "resampling", "transition"]
    named = sweep_key_schedule(keys, T, explicit_backward=True)
    assert list(named) == list(sk) and all(np.array_equal(named[k], sk[k]) for k in sk)
    for b in range(B):
        key_fwd, key_csmc, key_bridge = oracle.split(keys[b], 3)                  # gibbs.py:126
        k_fwd, k_x0, k_us, k_bs = oracle.split(key_csmc, 4)                       # :147
        key_init, key_scan = oracle.split(k_fwd, 2)
        step = oracle.split(key_scan, T)
        for name, want in (("fwd", key_fwd), ("bridge", key_bridge), ("x0", k_x0), ("us", k_us), ("bs", k_bs),
                           ("init", key_init)):
            np.testing.assert_array_equal(sk[name][b], want, err_msg=name)
        for k in range(T):
            k_res, k_tr = oracle.split(step[k], 2)
            np.testing.assert_array_equal(sk["resampling"][k, b], k_res)
            np.testing.assert_array_equal(sk["transition"][k, b], k_tr)


@pytest.mark.parametrize("B", (1, 2, 3, 7, 64))
@pytest.mark.parametrize("per", (1, 10, 33))
@pytest.mark.parametrize("cap", (33, 34, 65, 100, 1 << 31))
def test_group_planner(B, per, cap):
    from fbs_amd.samplers.gibbs_batched import lockstep_groups
    groups = lockstep_groups(B, per, cap)
    covered = [b for s, e in groups for b in range(s, e)]
    assert covered == list(range(B))                                              # all of range(B), in order, once
    assert all(0 < e - s and (e - s) * per <= cap for s, e in groups)             # never above the cap
    largest = min(B, cap // per)
    assert all(e - s == largest for s, e in groups[:-1]) and groups[-1][1] - groups[-1][0] <= largest
    if B * per <= cap:
        assert groups == [(0, B)]


def test_group_planner_sends_one_oversized_ensemble_to_the_loop():
    from fbs_amd.samplers import gibbs_batched
    assert gibbs_batched.lockstep_groups(1, 101, 100) == "loop"
    assert gibbs_batched.lockstep_groups(5, (1 << 31) + 1, gibbs_batched.LOCKSTEP_STORE_BYTES) == "loop"
    assert gibbs_batched.lockstep_groups(5, 1 << 31, gibbs_batched.LOCKSTEP_STORE_BYTES) == [(b, b + 1) for b in range(5)]
    assert gibbs_batched.LOCKSTEP_STORE_BYTES == 1 << 31


@pytest.mark.parametrize("explicit_final", (False, True))
def test_reference_chains_without_explicit_backward_alone_pass(explicit_final, oracle):
    """The chains the GPU anchor test of ``explicit_backward=False`` uses as its reference, run by the C oracle with the same
    key and design (tests/test_gpu_images_lg.py): their two halves agree within that test's threshold, 5 sqrt(2) SE."""
    import test_gpu_images_lg as L
    sm = L._sampler_model(int(oracle.randint(oracle.PRNGKey(L.MASK_SEED), (), 0, L.S_SHAPE[0] - L.S_HOLE)))
    m, cov, du = sm["model"].permuted(sm["mask"])
    om = oracle.make_lg(m, cov, oracle.sde_lin(0.02, 5.0, 0.0, 2.0), sm["ts"], du)
    ref = oracle.gibbs_chains_lg(om, oracle.PRNGKey(L.G_REF_SEED), np.zeros((L.S_B, du), np.float32), sm["y0"],
                                 np.zeros((L.S_B, L.S_T + 1), np.int32), L.G_N, L.G_BURN + L.G_KEEP, False, explicit_final)[3]
    out = L._halves_of_reference(ref[L.G_BURN:])
    L._report(f"reference chains, explicit_backward=False, explicit_final={explicit_final}", **out)
    assert max(out.values()) <= L.SIGMA, out
