"""Constrained decoding without a device (include/llama2_hip.h: l2_step_batch_constrained; runtime.pack_mask; serve.Scheduler's
allowed= / logit_bias=): the symbol, the mask packing against a plain bit loop, the argument refusals that need no context, and the
scheduler against a stand-in context that applies the constraints on the host."""
import ctypes as C
import hashlib
import inspect
import os
import re
import types

import numpy as np
import pytest

import __graft_entry__ as graft
from llama2_ts_amd import runtime, serve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
V = 29
BOS = 1


@pytest.fixture(scope="module")
def built():
    graft.build()
    return runtime.lib()


def test_symbol_is_exported_declared_and_listed(built):
    hdr = open(os.path.join(ROOT, "include", "llama2_hip.h")).read()
    assert re.search(r"\bint\s+l2_step_batch_constrained\s*\(", hdr)
    assert hasattr(C.CDLL(runtime.LIB_PATH), "l2_step_batch_constrained")
    assert "l2_step_batch_constrained" in runtime.ABI_SYMBOLS
    assert built.l2_abi_version() == 5
    for fn in (runtime.Context.step_batch, serve.Scheduler.submit_constrained, serve.Scheduler.submit_n):
        p = inspect.signature(fn).parameters
        assert p["allowed"].default is None and p["logit_bias"].default is None, fn


def bit_loop(ids, v):
    words = [0] * ((v + 31) // 32)
    for j in ids:
        words[j >> 5] |= 1 << (j & 31)
    return words


@pytest.mark.parametrize("v", [1, 31, 32, 33, 97, 512, 2083])
def test_pack_mask_against_a_bit_loop(v):
    rng = np.random.default_rng(v)
    sets = [[0], [v - 1], list(range(v)), [], sorted({int(t) for t in rng.integers(0, v, max(1, v // 3))}),
            [int(t) for t in rng.integers(0, v, 7)]]                  # the last: unsorted, maybe repeated
    for ids in sets:
        want = bit_loop(ids, v)
        got = runtime.pack_mask(ids, v)
        assert got.dtype == np.uint32 and got.shape == ((v + 31) // 32,)
        assert got.tolist() == want, (v, ids)
        flags = np.zeros(v, dtype=bool)
        flags[ids] = True
        assert runtime.pack_mask(flags, v).tolist() == want, (v, ids)
        assert runtime.pack_mask(set(ids), v).tolist() == want
        assert runtime.pack_mask(np.asarray(ids, dtype=np.int64), v).tolist() == want
    for bad in ([v], [-1], [0, v + 40]):
        with pytest.raises(ValueError):
            runtime.pack_mask(bad, v)
    with pytest.raises(ValueError):
        runtime.pack_mask(np.ones(v + 1, dtype=bool), v)


def test_context_free_arguments_are_refused(built):
    L = built
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    seqs, one, tok, p0 = i32(0, 1), i32(1, 1), i32(5, 6), i32(0, 0)
    picks = i32(-9, -9)
    lp = (C.c_double * 2)(9.0, 9.0)
    ids = i32(*([-9] * 6))
    tlp = (C.c_double * 6)(*([9.0] * 6))
    mask = (C.c_uint32 * 2)(0xffffffff, 0xffffffff)
    f32 = lambda *v: (C.c_float * len(v))(*v)

    def call(n=2, top_k=0, plp=None, tids=None, ttlp=None, mask_of=None, n_masks=0, masks=None, bc=None, bi=None, bv=None):
        return L.l2_step_batch_constrained(None, n, seqs, one, tok, p0, None, None, None, picks, None, top_k, plp, tids, ttlp,
                                           mask_of, n_masks, masks, bc, bi, bv)

    cases = {
        "top_k without pick_lp_out": dict(top_k=3, tids=ids, ttlp=tlp),
        "top_k 21": dict(top_k=21, plp=lp, tids=ids, ttlp=tlp),
        "top_k with a null top array": dict(top_k=3, plp=lp, tids=ids),
        "n 0": dict(n=0),
        "n 65": dict(n=65),
        "n_masks -1": dict(n_masks=-1, mask_of=i32(-1, -1), masks=mask),
        "n_masks > n": dict(n_masks=3, mask_of=i32(-1, -1), masks=mask),
        "n_masks with a null mask_of_row": dict(n_masks=1, masks=mask),
        "n_masks with null masks": dict(n_masks=1, mask_of=i32(0, -1)),
        "mask_of_row with null masks": dict(n_masks=0, mask_of=i32(-1, -1)),
        "mask index n_masks": dict(n_masks=1, mask_of=i32(0, 1), masks=mask),
        "mask index -2": dict(n_masks=1, mask_of=i32(0, -2), masks=mask),
        "bias_count 257": dict(bc=i32(0, 257), bi=i32(*range(257)), bv=f32(*([0.5] * 257))),
        "bias_count -1": dict(bc=i32(-1, 1), bi=i32(3), bv=f32(0.5)),
        "bias with null ids": dict(bc=i32(1, 0), bv=f32(0.5)),
        "bias with null values": dict(bc=i32(1, 0), bi=i32(3)),
        "bias +inf": dict(bc=i32(1, 1), bi=i32(3, 4), bv=f32(0.5, float("inf"))),
        "bias -inf": dict(bc=i32(1, 1), bi=i32(3, 4), bv=f32(float("-inf"), 0.5)),
        "bias NaN": dict(bc=i32(0, 1), bi=i32(3), bv=f32(float("nan"))),
    }
    for name, kw in cases.items():
        assert call(**kw) == E_ARG, name
        assert b"null context" not in L.l2_last_error(), name       # refused by its own check, before the context is looked at
    # well-formed constraints get as far as the context check
    assert call(plp=lp, top_k=3, tids=ids, ttlp=tlp, mask_of=i32(0, -1), n_masks=1, masks=mask, bc=i32(1, 0), bi=i32(3), bv=f32(0.5)) == E_ARG
    assert b"null context" in L.l2_last_error()
    assert call() == E_ARG and b"null context" in L.l2_last_error()
    assert list(picks) == [-9, -9] and list(lp) == [9.0, 9.0] and list(ids) == [-9] * 6 and list(tlp) == [9.0] * 6


# ---- the scheduler against a stand-in context ------------------------------------------------------------------------------------

class StubContext:
    """step_batch's contract on the host (tests/test_serve_cpu.py's stand-in, plus the constraints): a row's pick is a hash of its
    sequence's fed history, taken among the row's allowed ids when it has a mask; a biased id gets a second chance."""

    def __init__(self, slots, seq_len):
        self.slots, self.cfg = slots, types.SimpleNamespace(seq_len=seq_len, vocab_size=V)
        self.hist = [[] for _ in range(slots)]
        self.keywords = []                       # per call: the constraint keywords it was given

    def get_option(self, key):
        assert key == runtime.OPT_SEQS
        return self.slots

    def step_batch(self, seqs, runs, pos0, temperature=0.0, topp=1.0, rng=None, logits=False, **kw):
        assert set(kw) <= {"allowed", "logit_bias"}, kw
        self.keywords.append(sorted(kw))
        n = len(seqs)
        allowed = kw.get("allowed") or [None] * n
        bias = kw.get("logit_bias") or [None] * n
        assert len(allowed) == n and len(bias) == n
        picks = []
        for i, s in enumerate(seqs):
            h = self.hist[s]
            assert pos0[i] <= len(h)
            del h[pos0[i]:]                      # a restart, at 0 or (prefix reuse) after the rows the slot keeps
            h.extend(int(t) for t in runs[i])
            key = int.from_bytes(hashlib.sha256(np.asarray(h, dtype=np.int64).tobytes()).digest()[:8], "little")
            ids = sorted(set(range(V) if allowed[i] is None else allowed[i]))
            assert ids and all(0 <= t < V for t in ids)
            tok = ids[key % len(ids)]
            if bias[i]:
                fav = max(bias[i], key=lambda t: bias[i][t])
                if fav in ids and (key >> 20) % 3 == 0:
                    tok = fav
            picks.append(tok)
        return (picks, list(rng)) + ((np.zeros((n, V), dtype=np.float32),) if logits else ())


A_SET, B_SET = [2, 3, 5, 7, 11], [4, 6, 8, 10, 12]


def make_grammar(log, n_prompt):
    """Alternate between two disjoint sets; BOS is allowed from the seventh pick on."""
    def grammar(fed):
        log.append(list(fed))
        k = len(fed) - 1 - n_prompt              # picks made so far
        return (A_SET, B_SET)[k % 2] + ([BOS] if k >= 6 else [])
    return grammar


def requests(n=24):
    rng = np.random.default_rng(11)
    out = []
    for i in range(n):
        prompt = [int(t) for t in rng.integers(2, V, int(rng.integers(0, 30)))]
        out.append((prompt, int(rng.integers(1, 64)), i % 4))      # kind 0: plain, 1: callable, 2: static set, 3: bias only
    return out


def submit(sch, prompt, steps, kind, log):
    if kind == 1:
        return sch.submit_constrained(prompt, steps, allowed=make_grammar(log, len(prompt)))
    if kind == 2:
        return sch.submit_constrained(prompt, steps, allowed=iter(B_SET), logit_bias={8: 2.5, 3: 9.0})
    if kind == 3:
        return sch.submit_constrained(prompt, steps, logit_bias={17: 1.0})
    return sch.submit(prompt, steps)


def picks_of(res, prompt):
    return res.tokens_fed[1 + len(prompt):] + ([BOS] if res.finish == "bos" else [])


@pytest.mark.parametrize("prefix_cache", [False, True])
def test_scheduler_constraints(prefix_cache):
    reqs = requests()
    ctx = StubContext(5, 64)
    sch = serve.Scheduler(ctx, max_rows=24, prefix_cache=prefix_cache)
    if prefix_cache:
        ctx.seq_fork = lambda src, dsts, rows: [ctx.hist.__setitem__(d, ctx.hist[src][:rows]) for d in dsts]
    logs = [[] for _ in reqs]
    rids = [submit(sch, p, steps, kind, logs[i]) for i, (p, steps, kind) in enumerate(reqs)]
    res = sch.run()
    seen_constrained = 0
    for i, (prompt, steps, kind) in enumerate(reqs):
        got = res[rids[i]]
        picks = picks_of(got, prompt) if len(got.tokens_fed) > len(prompt) else []
        # alone: the same request on a fresh stand-in
        solo_ctx, solo_log = StubContext(1, 64), []
        solo = serve.Scheduler(solo_ctx, max_rows=8)
        rid = submit(solo, prompt, steps, kind, solo_log)
        want = solo.run()[rid]
        assert (got.tokens_fed, got.finish) == (want.tokens_fed, want.finish), i
        if kind == 0:
            assert solo_ctx.keywords and all(k == [] for k in solo_ctx.keywords)      # no constrained request: no new keyword
        if kind == 1:
            made = max(0, len(got.tokens_fed) - len(prompt))      # one pick per fed position from the prompt's last on; a request
            assert len(picks) == (made if got.finish == "bos" or not made else made - 1)      # ended by steps never feeds its last
            assert logs[i] == solo_log and len(logs[i]) == made, i                   # once per real pick
            for k, (fed, t) in enumerate(zip(logs[i], picks)):
                assert fed == [BOS] + prompt + picks[:k], (i, k)
                assert t in (A_SET, B_SET)[k % 2] or (t == BOS and k >= 6), (i, k, t)
            seen_constrained += len(picks)
        if kind == 2:
            assert all(t in B_SET for t in picks), i
            seen_constrained += len(picks)
    assert seen_constrained > 50
    assert any("allowed" in k for k in ctx.keywords) and any("logit_bias" in k for k in ctx.keywords)


def test_a_prompt_chunk_is_not_constrained_and_plain_steps_pass_no_keyword():
    ctx = StubContext(2, 64)
    sch = serve.Scheduler(ctx, max_rows=4)
    log = []
    prompt = [3, 4, 5, 6, 7, 8, 9, 10, 11]
    a = sch.submit_constrained(prompt, 14, allowed=make_grammar(log, len(prompt)))
    sch.step()                                   # rows 0 .. 3 of the prompt: the pick is thrown away
    sch.step()                                   # rows 4 .. 7
    assert ctx.keywords == [[], []] and log == []
    sch.step()                                   # rows 8, 9: the prompt's last position, the first real pick
    assert ctx.keywords[-1] == ["allowed"] and log == [[BOS] + prompt]
    res = sch.run()[a]
    assert len(log) == 14 - len(prompt)
    # a callable that returns None leaves that pick unconstrained: the step passes no keyword
    ctx2 = StubContext(1, 64)
    sch2 = serve.Scheduler(ctx2, max_rows=4)
    calls = []
    b = sch2.submit_constrained([3], 6, allowed=lambda fed: calls.append(len(fed)) or None)
    sch2.run()
    assert calls == [2, 3, 4, 5, 6][:len(calls)] and calls and all(k == [] for k in ctx2.keywords)
    assert res.tokens_fed[:10] == [BOS] + prompt
