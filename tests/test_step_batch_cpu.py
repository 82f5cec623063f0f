"""CPU-side checks of the mixed step (include/llama2_hip.h: l2_step_batch): the symbol is exported, declared and in the binding's ABI
list, the ABI version did not move, the Python layer wraps it, and null arguments are refused with L2_E_ARG before anything needs a
GPU."""
import ctypes as C
import os
import re

import pytest

import __graft_entry__ as graft
from llama2_ts_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "l2_step_batch"


@pytest.fixture(scope="module")
def built():
    graft.build()
    return runtime.lib()


def test_symbol_is_exported_declared_and_listed(built):
    hdr = open(os.path.join(ROOT, "include", "llama2_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, hdr)
    assert hasattr(C.CDLL(runtime.LIB_PATH), NAME)
    assert NAME in runtime.ABI_SYMBOLS


def test_abi_version_stays_5(built):
    assert built.l2_abi_version() == 5          # the surface only adds: a binding detects the call by its symbol


def test_context_has_the_wrapper():
    assert callable(getattr(runtime.Context, "step_batch", None))


def test_null_context_and_null_arrays_are_refused_without_a_device(built):
    L = built
    one = (C.c_int32 * 1)(0)
    n1 = (C.c_int32 * 1)(1)
    picks = (C.c_int32 * 1)(-7)
    t = (C.c_double * 1)(0.0)
    rng = (C.c_uint64 * 1)(5)
    assert L.l2_step_batch(None, 1, one, n1, one, one, None, None, None, picks, None) == -1
    assert b"null" in L.l2_last_error()
    assert L.l2_step_batch(None, 1, one, n1, one, one, t, t, rng, picks, None) == -1
    assert L.l2_step_batch(None, 1, None, None, None, None, None, None, None, None, None) == -1
    assert b"null" in L.l2_last_error()
    assert L.l2_step_batch(None, 0, one, n1, one, one, None, None, None, picks, None) == -1
    assert picks[0] == -7 and rng[0] == 5
