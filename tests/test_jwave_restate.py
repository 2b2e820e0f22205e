"""The one-wave search for J (tests/jwave_restate.py, the algorithm of wave_tree_J in fbsmi_lg.hip) against the oracle's own J
of the same step, on the CPU: every tile count the kernel takes, a few steps each of the 2-D toy at its own observation and
at y0 = 20 (both keep the oracle's log-weights finite, see test_gpu_lg_paired.py::test_queue_empty_and_nearly_full)."""
import numpy as np
import pytest

from helpers import toy_2d
from jwave_restate import K_BLOCK, oracle_steps, restate_J

T = 4


def _model(O, toy):
    return O.make_lg(toy["m0"], toy["cov0"], O.sde_const(-0.5, 1.0), np.linspace(0, 1.0, T + 1), toy["du"])


def _steps(O, N, y0, bs, seed):
    toy = toy_2d()
    rng = np.random.default_rng(N + seed)
    x0 = rng.normal(size=toy["du"]).astype(np.float32)
    key = O.split(O.PRNGKey(31), 2)[seed % 2]
    y0 = toy["y0"] if y0 is None else np.asarray(y0, np.float32)
    return oracle_steps(O, _model(O, toy), key, x0, y0, np.asarray(bs, np.int32), N)


@pytest.mark.parametrize("y0", [None, [20.0]], ids=["own_y0", "y0_20"])
@pytest.mark.parametrize("nb", [2, 4, 8, 32, 64, 128, 256])
def test_restated_J_is_the_oracles(nb, y0, oracle):
    N = nb * K_BLOCK
    bs = np.random.default_rng(nb).integers(0, N, T + 1)
    for s, st in enumerate(_steps(oracle, N, y0, bs, 0)):
        assert np.isfinite(st["w"]).all()
        assert restate_J(st["w"], st["i_ref"], st["u3"], N) == st["J"], f"step {s}"


@pytest.mark.parametrize("N", [512, 2048])
def test_reference_index_on_tile_and_lane_edges(N, oracle):
    """i* on the first and last tile, the first and last lane of the wave and the first and last of a lane's four leaves."""
    bs = [0, 255, 256, N - 1, N // 2 + 77]
    for s, st in enumerate(_steps(oracle, N, None, bs, 1)):
        assert restate_J(st["w"], st["i_ref"], st["u3"], N) == st["J"], f"step {s}"


def test_every_u3_lands_where_the_oracles_search_does(oracle):
    """One step's weights, the search repeated for uniforms over (0, 1) and at its ends, against the oracle's searchsorted over
    the oracle's cumsum of the same J_prob: every leaf of a small tree is reached, not only the few that a sweep's keys give."""
    N = 1024
    st = _steps(oracle, N, None, [5, 700, 1023, 0, 256], 0)[2]
    F = np.float32
    w, i_ref = st["w"], st["i_ref"]
    jp = oracle.div(F(1) - oracle.div(w, np.full(N, w.max(), F)), np.full(N, F(N), F))
    jp[i_ref] = F(0)
    jp[i_ref] = max(F(1) - oracle.tree_sum(jp), F(0))
    cdf = oracle.cumsum(jp)
    us = np.concatenate([np.linspace(0, 1, 301, dtype=F)[:-1], [F(1) - F(2) ** -24, F(2) ** -24]]).astype(F)
    for u in us:
        want = int(oracle.searchsorted(cdf, cdf[-1] * (F(1) - u))[0])
        assert restate_J(w, i_ref, u, N) == want, f"u3 = {u}"
