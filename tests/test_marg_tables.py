"""No GPU: the Doob bridge's coefficient tables shared by doob_bridge_simulator and the fused marg_y sweep
(fbs_amd.sdes.linear.doob_bridge_tables) against the loop the closure-tier tests build by hand, and the new ABI entry."""
import os
import re

import numpy as np
import pytest

from marg_restate import bridge_tables_by_hand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sdes():
    from fbs_amd.sdes import StationaryConstLinearSDE, StationaryLinLinearSDE
    return [StationaryConstLinearSDE(-0.5, 1.0), StationaryLinLinearSDE(0.02, 4.0, 0.0, 1.0)]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("T,nsub,Tend", [(10, 20, 1.0), (12, 100, 1.0), (5, 7, 2.0), (1, 1, 1.0)])
def test_shared_tables_equal_the_hand_built_ones(which, T, nsub, Tend):
    """float64 on the host, rounded once: the float32 tables are the hand-built float64 ones cast to float32, to the bit."""
    from fbs_amd.sdes.linear import doob_bridge_tables
    sde = _sdes()[which]
    ts = np.linspace(0.0, Tend, T + 1)
    got = doob_bridge_tables(sde, ts, nsub)
    want = bridge_tables_by_hand(sde, ts, nsub)
    assert got["nsub"] == nsub
    for name, n in (("A", T * nsub), ("B", T * nsub), ("S", T * nsub), ("ddt", T)):
        assert got[name].dtype == np.float32 and got[name].shape == (n,) and got[name].flags["C_CONTIGUOUS"], name
        np.testing.assert_array_equal(got[name].view(np.uint32), want[name].astype(np.float32).view(np.uint32), err_msg=name)


def test_set_bridge_is_declared_and_bound():
    from fbs_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fbsmi.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fbsmi_lg_sweep_set_bridge\s*\(\s*fbsmi_lg_sweep\s*\*\s*\w+\s*,\s*const\s+fbsmi_doob_bridge\s*\*", text)
    m = re.search(r"typedef\s+struct\s+fbsmi_doob_bridge\s*\{(.*?)\}\s*fbsmi_doob_bridge\s*;", text, flags=re.S)
    assert m, "fbsmi_doob_bridge is not declared"
    fields = re.findall(r"(int32_t|const\s+float\s*\*)\s*(\w+)\s*;", m.group(1))
    assert [f[1] for f in fields] == ["nsub", "A", "B", "S", "ddt"]
    assert [f[0] for f in _lib.DoobBridgeStruct._fields_] == ["nsub", "A", "B", "S", "ddt"]
    res, args = _lib.SIGNATURES["fbsmi_lg_sweep_set_bridge"]
    assert res is _lib.C.c_int and len(args) == 2
    assert _lib.lib().fbsmi_abi_version() == 1
    assert hasattr(_lib.lib(), "fbsmi_lg_sweep_set_bridge")
