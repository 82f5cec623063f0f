"""CPU-side checks of the batched sampled decode (include/llama2_hip.h: l2_decode_sample_batch, option keys 12 / 13): the symbol is
exported and declared, the Python layer wraps it, and null arguments are refused with L2_E_ARG before anything needs a GPU."""
import ctypes as C
import os
import re

import pytest

import __graft_entry__ as graft
from llama2_ts_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    graft.build()
    return runtime.lib()


def test_sample_batch_symbol_is_exported_declared_and_listed(built):
    hdr = open(os.path.join(ROOT, "include", "llama2_hip.h")).read()
    assert re.search(r"\bl2_decode_sample_batch\s*\(", hdr)
    assert hasattr(C.CDLL(runtime.LIB_PATH), "l2_decode_sample_batch")
    assert "l2_decode_sample_batch" in runtime.ABI_SYMBOLS
    assert built.l2_abi_version() == 5          # the surface only adds: no version step


def test_batch_sampled_option_keys():
    hdr = open(os.path.join(ROOT, "include", "llama2_hip.h")).read()
    assert re.search(r"L2_OPT_BATCH_SAMPLED_TOKENS\s*=\s*12\b", hdr)
    assert re.search(r"L2_OPT_BATCH_SAMPLED_SERIAL\s*=\s*13\b", hdr)
    assert runtime.OPT_BATCH_SAMPLED_TOKENS == 12 and runtime.OPT_BATCH_SAMPLED_SERIAL == 13


def test_context_has_decode_sample_batch():
    assert callable(getattr(runtime.Context, "decode_sample_batch", None))


def test_null_context_and_arrays_are_refused_without_a_device(built):
    L = built
    one = (C.c_int32 * 1)(0)
    dbl = (C.c_double * 1)(0.9)
    rng = (C.c_uint64 * 1)(42)
    toks = (C.c_int32 * 4)()
    assert L.l2_decode_sample_batch(None, 1, one, one, one, 4, dbl, dbl, rng, toks) == -1
    assert b"null" in L.l2_last_error()
    assert L.l2_decode_sample_batch(None, 1, one, one, one, 4, None, None, None, None) == -1
    assert L.l2_decode_sample_batch(None, 1, None, None, None, 4, dbl, dbl, rng, toks) == -1
    assert rng[0] == 42
