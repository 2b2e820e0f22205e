"""CPU: the fused backward simulation's entry points are declared in include/fbsmi.h and bound in fbs_amd._lib with the
same arity, and the size predicate of the Python dispatch refuses what fbsmi_lg_backsim_create refuses."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fbsmi_lg_backsim_create", "fbsmi_lg_backsim_destroy", "fbsmi_lg_backsim_run")


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fbsmi.h")).read(), flags=re.S)
    return {name: args for name, args in re.findall(r"\b(fbsmi_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


@pytest.mark.parametrize("name", NAMES)
def test_symbol_declared_and_bound_with_matching_arity(name):
    from fbs_amd import _lib
    decl = _declarations()
    assert name in decl, f"{name} is not declared in include/fbsmi.h"
    assert name in _lib.SIGNATURES, f"{name} is not in fbs_amd._lib.SIGNATURES"
    nargs = len([a for a in decl[name].split(",") if a.strip() and a.strip() != "void"])
    assert len(_lib.SIGNATURES[name][1]) == nargs


def test_library_exports_the_backsim_symbols():
    import ctypes
    from fbs_amd import _lib
    L = ctypes.CDLL(_lib.build())
    for name in NAMES:
        assert hasattr(L, name)


def test_fused_backsim_supported_refuses_what_the_engine_refuses():
    from fbs_amd.linear_gaussian import LinearGaussianBridge

    def model(du, dv):   # the predicate reads the dimensions alone: no device needed
        m = object.__new__(LinearGaussianBridge)
        m.du, m.dv = du, dv
        return m

    assert model(2, 2).fused_backsim_supported(1)
    assert model(128, 128).fused_backsim_supported(131072)
    assert not model(2, 2).fused_backsim_supported(0)
    assert not model(2, 2).fused_backsim_supported(131073)
    assert not model(129, 2).fused_backsim_supported(100)
    assert not model(2, 129).fused_backsim_supported(100)
