"""CPU-side checks of the per-token log-probabilities (include/llama2_hip.h: l2_seq_score_batch, l2_step_batch_logprobs): both symbols
are exported, declared and in the binding's ABI list, the ABI version did not move, the Python layer wraps them, the argument errors
that need no context are refused with L2_E_ARG before anything is written (a target outside [-1, V) needs a context to know V:
tests/test_score_gpu.py::test_errors_and_repeatability), and the scheduler asks for the logprobs form only in steps
that hold a request that wants it -- against a pure-Python stand-in of the step whose picks do not depend on that form."""
import ctypes as C
import hashlib
import inspect
import math
import os
import re
import types

import numpy as np
import pytest

import __graft_entry__ as graft
from llama2_ts_amd import runtime, serve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("l2_seq_score_batch", "l2_step_batch_logprobs")
E_ARG = -1
MASK = (1 << 64) - 1
V = 29


@pytest.fixture(scope="module")
def built():
    graft.build()
    return runtime.lib()


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_declared_and_listed(built, name):
    hdr = open(os.path.join(ROOT, "include", "llama2_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
    assert hasattr(C.CDLL(runtime.LIB_PATH), name)
    assert name in runtime.ABI_SYMBOLS


def test_abi_version_stays_5(built):
    assert built.l2_abi_version() == 5


def test_wrappers_exist():
    assert callable(getattr(runtime.Context, "seq_score_batch", None))
    assert "logprobs" in inspect.signature(runtime.Context.step_batch).parameters
    assert "logprobs" in inspect.signature(serve.Scheduler.submit).parameters
    assert "logprobs" in serve.Result.__slots__


def test_score_arguments_are_refused_without_a_device(built):
    L = built
    lp = (C.c_double * 1)(7.0)
    am = (C.c_int32 * 1)(-7)
    ids = (C.c_int32 * 20)(*([-7] * 20))
    tlp = (C.c_double * 20)(*([7.0] * 20))
    one = (C.c_int32 * 1)(0)
    n1 = (C.c_int32 * 1)(1)
    tg = (C.c_int32 * 1)(0)
    assert L.l2_seq_score_batch(None, 1, one, n1, one, one, None, 0, lp, am, None, None) == E_ARG
    assert b"null" in L.l2_last_error()
    assert L.l2_seq_score_batch(None, 1, one, n1, one, one, tg, 0, None, am, None, None) == E_ARG
    assert b"null" in L.l2_last_error()
    assert L.l2_seq_score_batch(None, 1, one, n1, one, one, tg, 21, lp, am, ids, tlp) == E_ARG
    assert b"top_k 21" in L.l2_last_error()
    assert L.l2_seq_score_batch(None, 1, one, n1, one, one, tg, -1, lp, am, ids, tlp) == E_ARG
    assert b"top_k -1" in L.l2_last_error()
    assert L.l2_seq_score_batch(None, 1, one, n1, one, one, tg, 5, lp, am, None, tlp) == E_ARG
    assert b"top_ids_out" in L.l2_last_error()
    assert L.l2_seq_score_batch(None, 1, one, n1, one, one, tg, 5, lp, am, ids, None) == E_ARG
    assert b"top_lp_out" in L.l2_last_error()
    assert L.l2_seq_score_batch(None, 1, one, n1, one, one, tg, 0, lp, am, None, None) == E_ARG
    assert b"null context" in L.l2_last_error()
    assert L.l2_seq_score_batch(None, 1, None, None, None, None, tg, 0, lp, am, None, None) == E_ARG
    assert lp[0] == 7.0 and am[0] == -7 and list(ids) == [-7] * 20 and list(tlp) == [7.0] * 20


def test_step_logprobs_arguments_are_refused_without_a_device(built):
    L = built
    one = (C.c_int32 * 1)(0)
    n1 = (C.c_int32 * 1)(1)
    picks = (C.c_int32 * 1)(-7)
    plp = (C.c_double * 1)(7.0)
    ids = (C.c_int32 * 20)(*([-7] * 20))
    tlp = (C.c_double * 20)(*([7.0] * 20))
    rng = (C.c_uint64 * 1)(5)
    t = (C.c_double * 1)(0.5)
    assert L.l2_step_batch_logprobs(None, 1, one, n1, one, one, None, None, None, picks, None, 0, None, None, None) == E_ARG
    assert b"pick_lp_out" in L.l2_last_error()
    assert L.l2_step_batch_logprobs(None, 1, one, n1, one, one, t, t, rng, picks, None, 21, plp, ids, tlp) == E_ARG
    assert b"top_k 21" in L.l2_last_error()
    assert L.l2_step_batch_logprobs(None, 1, one, n1, one, one, t, t, rng, picks, None, 3, plp, None, None) == E_ARG
    assert b"top_ids_out" in L.l2_last_error()
    assert L.l2_step_batch_logprobs(None, 1, one, n1, one, one, t, t, rng, picks, None, 3, plp, ids, tlp) == E_ARG
    assert b"null context" in L.l2_last_error()
    assert L.l2_step_batch_logprobs(None, 1, one, n1, one, one, None, None, None, None, None, 0, plp, None, None) == E_ARG
    assert picks[0] == -7 and plp[0] == 7.0 and rng[0] == 5 and list(ids) == [-7] * 20 and list(tlp) == [7.0] * 20


# ---- the scheduler against a stand-in of the step ---------------------------------------------------------------------------------

def xorshift_u32(state):
    state ^= state >> 12
    state ^= (state << 25) & MASK
    state ^= state >> 27
    return state, ((state * 0x2545F4914F6CDD1D) >> 32) & 0xFFFFFFFF


class StubContext:
    """step_batch's contract on the host: per-sequence token histories; a row's logits are a hash of its history (so a pick and its
    log-probability depend on what was fed, not on how it was chunked), the pick their argmax or one xorshift* draw."""

    def __init__(self, slots, seq_len):
        self.slots, self.cfg = slots, types.SimpleNamespace(seq_len=seq_len, vocab_size=V)
        self.hist = [[] for _ in range(slots)]
        self.calls, self.lp_calls = 0, []

    def get_option(self, key):
        assert key == runtime.OPT_SEQS
        return self.slots

    def step_batch(self, seqs, runs, pos0, temperature=0.0, topp=1.0, rng=None, logits=False, logprobs=None):
        n = len(seqs)
        temp = list(np.broadcast_to(np.asarray(temperature, dtype=np.float64), (n,)))
        self.calls += 1
        picks, after, lg = [], [], np.zeros((n, V), dtype=np.float32)
        for i, s in enumerate(seqs):
            h = self.hist[s]
            if pos0[i] == 0:
                del h[:]
            assert pos0[i] == len(h)
            h.extend(int(t) for t in runs[i])
            seed = hashlib.sha256(np.asarray(h, dtype=np.int64).tobytes()).digest()
            lg[i] = np.frombuffer(seed[:V], dtype=np.uint8).astype(np.float32) / 16.0
            st = None if rng is None else int(rng[i])
            tok = int(np.argmax(lg[i]))
            if temp[i] != 0.0:
                st, u = xorshift_u32(st)
                tok = u % V
            picks.append(tok)
            after.append(st)
        out = (picks, after, lg) if logits else (picks, after)
        if logprobs is None:
            return out
        self.lp_calls.append(self.calls)
        k = int(logprobs)
        x = lg.astype(np.float64)
        lse = x.max(1) + np.log(np.exp(x - x.max(1, keepdims=True)).sum(1))
        lp = x - lse[:, None]
        order = np.array([np.lexsort((np.arange(V), -x[i]))[:k] for i in range(n)], dtype=np.int32).reshape(n, k)
        return out + ((lp[np.arange(n), picks], order, np.take_along_axis(lp, order.astype(np.int64), 1)),)


def _run(reqs, logprobs_of, slots=3, max_rows=8):
    ctx = StubContext(slots, 40)
    sch = serve.Scheduler(ctx, max_rows=max_rows)
    ids = [sch.submit(p, steps, temperature=t, seed=sd, logprobs=logprobs_of(i)) for i, (p, steps, t, sd) in enumerate(reqs)]
    res = sch.run()
    return ctx, [res[i] for i in ids]


REQS = [([5, 6, 7], 12, 0.0, 1), ([8] * 9, 20, 0.8, 7), ([3, 4], 9, 0.0, 3), ([9, 10, 11, 12, 13], 25, 1.1, 11), ([2], 6, 0.5, 5)]


def test_scheduler_asks_for_logprobs_only_where_a_request_does():
    plain_ctx, plain = _run(REQS, lambda i: None)
    assert plain_ctx.lp_calls == []
    assert all(r.logprobs is None for r in plain)
    want = {0: 4, 2: 0}                                  # two early, short requests ask: top 4 and the pick's lp alone
    ctx, got = _run(REQS, lambda i: want.get(i))
    assert 0 < len(ctx.lp_calls) < ctx.calls              # the steps without those requests take the plain form
    for i, (a, b) in enumerate(zip(plain, got)):
        assert a.tokens_fed == b.tokens_fed and a.rng_state == b.rng_state and a.finish == b.finish, i
        if i not in want:
            assert b.logprobs is None
            continue
        n_picks = len(b.tokens_fed) - len(REQS[i][0])     # one pick per position after the prompt (the last pick included, BOS too)
        assert len(b.logprobs) == n_picks, (i, len(b.logprobs), n_picks)
        for lp, top in b.logprobs:
            assert len(top) == want[i] and lp <= 0.0 and not math.isnan(lp)
            assert all(t[1] <= 0.0 for t in top) and [t[1] for t in top] == sorted((t[1] for t in top), reverse=True)


def test_scheduler_refuses_a_logprobs_count_outside_the_range():
    sch = serve.Scheduler(StubContext(1, 8), max_rows=4)
    with pytest.raises(ValueError):
        sch.submit([3], 4, logprobs=21)
    with pytest.raises(ValueError):
        sch.submit([3], 4, logprobs=-1)
