"""CPU-side checks of the batched-decode surface (include/llama2_hip.h: l2_seq_reserve .. l2_read_seq_cache): the symbols are
exported, the Python layer wraps them, and null or out-of-range arguments are refused with L2_E_ARG before anything needs a GPU."""
import ctypes as C
import os
import re

import pytest

import __graft_entry__ as graft
from llama2_ts_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["l2_seq_reserve", "l2_seq_prefill", "l2_forward_batch", "l2_decode_greedy_batch", "l2_read_seq_cache"]


@pytest.fixture(scope="module")
def built():
    graft.build()
    return runtime.lib()


def test_batch_symbols_are_exported_and_declared(built):
    hdr = open(os.path.join(ROOT, "include", "llama2_hip.h")).read()
    raw = C.CDLL(runtime.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(raw, name), name
        assert name in runtime.ABI_SYMBOLS, name
    assert re.search(r"L2_OPT_SEQS\s*=\s*11\b", hdr) and runtime.OPT_SEQS == 11
    assert built.l2_abi_version() == 5          # the surface only adds: no version step


def test_context_has_the_batch_wrappers():
    for name in ("seq_reserve", "seq_prefill", "forward_batch", "decode_greedy_batch", "read_seq_cache"):
        assert callable(getattr(runtime.Context, name, None)), name


def test_null_and_out_of_range_arguments_are_refused_without_a_device(built):
    L = built
    one = (C.c_int32 * 1)(0)
    out = (C.c_float * 4)()
    toks = (C.c_int32 * 4)()
    assert L.l2_seq_reserve(None, 4) == -1
    assert L.l2_seq_prefill(None, 0, one, 1, 0, None) == -1
    assert L.l2_forward_batch(None, 1, one, one, one, None) == -1
    assert L.l2_decode_greedy_batch(None, 1, one, one, one, 4, toks) == -1
    assert L.l2_read_seq_cache(None, 0, runtime.S_KEY_CACHE, -1, out, 4) == -1
    assert b"null" in L.l2_last_error()
