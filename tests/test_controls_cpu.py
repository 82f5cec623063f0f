"""Sampling controls without a device (include/llama2_hip.h: l2_step_batch_sampling, l2_debug_sample_controls; serve.Scheduler's
submit_sampling): the symbols and signatures, the argument refusals that need no context, the numpy statement of the rules
(tests/controls_ref.py) against the definitions spelled out element by element, and the scheduler against a stand-in context that
applies that statement on the host."""
import ctypes as C
import hashlib
import inspect
import os
import re
import types

import numpy as np
import pytest

import __graft_entry__ as graft
import controls_ref as R
from llama2_ts_amd import runtime, serve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
V = 29
BOS = 1
CONTROLS = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, top_k=0, min_p=0.0)


@pytest.fixture(autouse=True)
def feature_present():
    """Every test here is about the sampling controls: without the entry point and the scheduler call none of them may pass."""
    assert "l2_step_batch_sampling" in runtime.ABI_SYMBOLS and hasattr(serve.Scheduler, "submit_sampling")


@pytest.fixture(scope="module")
def built():
    graft.build()
    return runtime.lib()


def test_symbols_are_exported_declared_and_listed(built):
    hdr = open(os.path.join(ROOT, "include", "llama2_hip.h")).read()
    raw = C.CDLL(runtime.LIB_PATH)
    for name in ("l2_step_batch_sampling", "l2_debug_sample_controls"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(raw, name), name
        assert name in runtime.ABI_SYMBOLS
    assert "typedef struct l2_sample_controls" in hdr
    assert built.l2_abi_version() == 5 and "#define L2_ABI_VERSION 5" in hdr
    fields = [f for f, _ in runtime.SampleControls._fields_]
    assert fields == ["hist_count", "hist_ids", "repetition", "presence", "frequency", "sample_top_k", "min_p"]
    assert C.sizeof(runtime.SampleControls) == 7 * C.sizeof(C.c_void_p)


def test_python_signatures_carry_the_keywords_with_neutral_defaults():
    p = inspect.signature(runtime.Context.step_batch).parameters
    names = list(p)
    new = ["history", "repetition_penalty", "presence_penalty", "frequency_penalty", "top_k", "min_p"]
    assert names[-6:] == new and all(p[k].default is None for k in new)
    assert names[:names.index("history")] == ["self", "seqs", "runs", "pos0", "temperature", "topp", "rng", "logits", "logprobs", "allowed", "logit_bias"]
    assert callable(runtime.debug_sample_controls)
    p = inspect.signature(serve.Scheduler.submit_sampling).parameters
    assert list(p) == ["self", "prompt_ids", "steps", "temperature", "topp", "seed", "logprobs", "allowed", "logit_bias"] + list(CONTROLS)
    assert {k: p[k].default for k in CONTROLS} == CONTROLS
    assert (p["temperature"].default, p["topp"].default, p["seed"].default, p["logprobs"].default) == (0.0, 1.0, 1, None)
    p = inspect.signature(serve.Scheduler.submit_n).parameters
    assert list(p)[-5:] == list(CONTROLS) and {k: p[k].default for k in CONTROLS} == CONTROLS
    # the pinned signatures stay
    assert list(inspect.signature(serve.Scheduler.submit).parameters) == ["self", "prompt_ids", "steps", "temperature", "topp", "seed", "logprobs"]
    assert list(inspect.signature(serve.Scheduler.submit_constrained).parameters)[-2:] == ["allowed", "logit_bias"]


def test_context_free_arguments_are_refused(built):
    L = built
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    f64 = lambda *v: (C.c_double * len(v))(*v)
    seqs, one, tok, p0 = i32(0, 1), i32(1, 1), i32(5, 6), i32(0, 0)
    picks = i32(-9, -9)
    lp = f64(9.0, 9.0)
    ids = i32(*([-9] * 6))
    tlp = f64(*([9.0] * 6))
    inf, nan = float("inf"), float("nan")
    addr = lambda a: None if a is None else C.cast(a, C.c_void_p).value

    def call(n=2, temp=None, sc=True, **kw):
        st = (C.c_uint64 * 2)(11, 22)
        s = runtime.SampleControls(*[addr(kw.get(f)) for f, _ in runtime.SampleControls._fields_])
        rc = L.l2_step_batch_sampling(None, n, seqs, one, tok, p0, temp, None if temp is None else f64(0.9, 0.9), None if temp is None else st,
                                      picks, None, 3, lp, ids, tlp, None, 0, None, None, None, None, C.byref(s) if sc else None)
        assert list(st) == [11, 22]
        return rc

    sampling = f64(0.9, 0.0)
    cases = {
        "n 0": dict(n=0),
        "n 65": dict(n=65),
        "count -1": dict(hist_count=i32(0, -1), hist_ids=i32(3)),
        "count with null ids": dict(hist_count=i32(0, 2)),
        "repetition 0": dict(repetition=f64(1.0, 0.0)),
        "repetition -1.5": dict(repetition=f64(-1.5, 1.0)),
        "repetition inf": dict(repetition=f64(inf, 1.0)),
        "repetition NaN": dict(repetition=f64(1.0, nan)),
        "presence inf": dict(presence=f64(inf, 0.0)),
        "presence NaN": dict(presence=f64(0.0, nan)),
        "frequency -inf": dict(frequency=f64(0.0, -inf)),
        "frequency NaN": dict(frequency=f64(nan, 0.0)),
        "top_k -1": dict(sample_top_k=i32(0, -1)),
        "min_p 1.5": dict(min_p=f64(0.0, 1.5)),
        "min_p -0.1": dict(min_p=f64(-0.1, 0.0)),
        "min_p NaN": dict(min_p=f64(nan, 0.0)),
        "top_k with temperature < 0": dict(temp=f64(-0.9, 0.0), sample_top_k=i32(5, 0)),
        "min_p with temperature < 0": dict(temp=f64(0.9, -0.5), min_p=f64(0.0, 0.25)),
    }
    for name, kw in cases.items():
        assert call(**kw) == E_ARG, name
        assert b"null context" not in L.l2_last_error(), name       # refused by its own check, before the context is looked at
    # well-formed controls get as far as the context check; so do a greedy row's top_k / min_p under any temperature of the others
    ok = dict(hist_count=i32(2, 0), hist_ids=i32(3, 3), repetition=f64(1.3, 0.7), presence=f64(-0.5, 0.0), frequency=f64(0.25, 0.0),
              sample_top_k=i32(5, 40), min_p=f64(1.0, 0.05))
    for kw in (ok, dict(ok, temp=sampling), dict(temp=f64(-0.9, 0.0), sample_top_k=i32(0, 7), min_p=f64(0.0, 0.5)), dict(), dict(sc=False)):
        assert call(**kw) == E_ARG
        assert b"null context" in L.l2_last_error()
    assert list(picks) == [-9, -9] and list(lp) == [9.0, 9.0] and list(ids) == [-9] * 6 and list(tlp) == [9.0] * 6

    # the diagnostic: its own bounds, refused before any device is touched, outputs at their sentinels
    x = (C.c_float * 8)(*range(8))
    pen, tr = (C.c_float * 8)(*([7.0] * 8)), (C.c_float * 8)(*([7.0] * 8))

    def dbg(n=2, v=4, logits=x, temp=None, sc=True, **kw):
        s = runtime.SampleControls(*[addr(kw.get(f)) for f, _ in runtime.SampleControls._fields_])
        return L.l2_debug_sample_controls(0, n, v, logits, temp, C.byref(s) if sc else None, pen, tr)

    big = i32(0, 65537)
    dcases = {
        "null logits": dict(logits=None), "null sc": dict(sc=False), "n 0": dict(n=0), "n 65": dict(n=65), "vocab 0": dict(v=0),
        "vocab above the sampler's limit": dict(v=256 * 1024 + 1),
        "count 65537": dict(hist_count=big, hist_ids=(C.c_int32 * 65537)()),
        "history id == vocab": dict(hist_count=i32(1, 1), hist_ids=i32(3, 4)),
        "history id -1": dict(hist_count=i32(1, 1), hist_ids=i32(-1, 2)),
        "repetition 0": dict(repetition=f64(0.0, 1.0)), "min_p 2": dict(min_p=f64(2.0, 0.0)), "top_k -3": dict(sample_top_k=i32(-3, 0)),
        "temperature NaN": dict(temp=f64(nan, 0.0)),
        "min_p with temperature < 0": dict(temp=f64(-1.0, 0.0), min_p=f64(0.5, 0.0)),
    }
    for name, kw in dcases.items():
        assert dbg(**kw) == E_ARG, name
    assert list(pen) == [7.0] * 8 and list(tr) == [7.0] * 8


# ---- the numpy statement against the definitions, element by element ---------------------------------------------------------------

def planted_row(v, seed):
    rng = np.random.default_rng(seed)
    x = (rng.integers(-24, 25, v) / 4.0).astype(np.float32)      # a coarse grid: many exact ties
    if v > 6:
        x[[1, 4]] = -np.inf
        x[2], x[5] = 0.0, -0.0
    return x


def test_reference_penalties_follow_the_formula():
    x = np.array([2.0, -2.0, 0.0, -0.0, 3.0, -np.inf, np.nan, 1.0], dtype=np.float32)
    hist = [0, 1, 1, 2, 3, 5, 6, 0, 0]
    got = R.penalise(x, hist, 1.25, 0.5, 0.125)
    want = x.copy()
    want[0] = np.float32(np.float64(np.float32(2.0 / 1.25)) - (0.5 + 0.125 * 3))
    want[1] = np.float32(np.float64(np.float32(-2.0 * 1.25)) - (0.5 + 0.125 * 2))
    want[2] = want[3] = np.float32(0.0 - (0.5 + 0.125))            # +0 and -0 are not > 0: multiplied
    assert got[[0, 1, 2, 3]].tolist() == want[[0, 1, 2, 3]].tolist()
    assert got[4] == 3.0 and got[7] == 1.0 and np.isneginf(got[5]) and np.isnan(got[6])
    # repetition alone keeps the sign of zero and writes nothing else
    only = R.penalise(x, hist, 0.5)
    assert only[0] == 4.0 and only[1] == -1.0 and np.signbit(only[3]) and not np.signbit(only[2])
    assert np.array_equal(R.penalise(x, hist).view(np.uint32), x.view(np.uint32))
    assert np.array_equal(R.penalise(x, [], 1.5, 1.0, 1.0).view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("v", [1, 2, 7, 64, 97])
def test_reference_truncation_follows_the_definitions(v):
    x = planted_row(v, v)
    order = sorted(range(v), key=lambda j: (-float(x[j] + np.float32(0.0)), j))      # descending value, equal values by ascending id
    for k in sorted({1, 2, v // 2, v - 1, v, v + 5}):
        keep = R.top_k_survivors(x, k)
        want = np.zeros(v, dtype=bool)
        want[order[:k] if 0 < k < v else order] = True
        assert keep.tolist() == want.tolist(), (v, k)
    for temp, mp in ((0.5, 0.25), (2.0, 1.0), (1.0, 0.05)):
        got = R.truncate(x, temp, 0, mp)
        s = [np.float32(np.float64(t) / temp) for t in x]
        smax = max(s)
        for j in range(v):
            stay = (np.float64(s[j]) - np.float64(smax)) >= np.log(mp) if np.isfinite(s[j]) else False
            assert (got[j] == x[j] and np.signbit(got[j]) == np.signbit(x[j])) if stay else np.isneginf(got[j]), (v, temp, mp, j)
    both = R.truncate(x, 0.5, 3, 0.25)
    a, b = R.truncate(x, 0.5, 3, 0.0), R.truncate(x, 0.5, 0, 0.25)
    assert np.array_equal(np.isneginf(both), np.isneginf(a) | np.isneginf(b))
    assert np.array_equal(R.truncate(x, 0.0, 3, 0.25).view(np.uint32), x.view(np.uint32))      # a greedy row ignores stage B
    nanrow = np.array([np.nan, 1.0, np.nan, 2.0], dtype=np.float32)
    assert R.top_k_survivors(nanrow, 2).tolist() == [True, False, False, True]                 # NaN at index 0 ranks first, elsewhere last


# ---- the scheduler against a stand-in context ------------------------------------------------------------------------------------

class StubContext:
    """step_batch's contract on the host with the sampling controls applied by tests/controls_ref.py: a row's logits are a hash of
    its sequence's fed history; its pick is the argmax of the penalised row (greedy) or a hash-chosen survivor of the truncated one."""

    def __init__(self, slots, seq_len):
        self.slots, self.cfg = slots, types.SimpleNamespace(seq_len=seq_len, vocab_size=V)
        self.hist = [[] for _ in range(slots)]
        self.calls = []                          # per call: (positional arguments, keywords) as given
        self.controlled = []                     # per row that carried a control: (tokens its sequence holds, the row's controls)

    def get_option(self, key):
        assert key == runtime.OPT_SEQS
        return self.slots

    def step_batch(self, seqs, runs, pos0, temperature=0.0, topp=1.0, rng=None, logits=False, **kw):
        assert set(kw) <= {"history", "repetition_penalty", "presence_penalty", "frequency_penalty", "top_k", "min_p", "allowed"}, kw
        self.calls.append(((list(seqs), [list(r) for r in runs], list(pos0), list(temperature), list(topp), list(rng), logits),
                           {k: list(v) for k, v in kw.items()}))
        n = len(seqs)
        col = lambda name, off: [off if v is None else v for v in kw.get(name) or [None] * n]
        hist, rep, pres, freq = col("history", None), col("repetition_penalty", 1.0), col("presence_penalty", 0.0), col("frequency_penalty", 0.0)
        top_k, min_p, allowed = col("top_k", 0), col("min_p", 0.0), col("allowed", None)
        picks = []
        for i, s in enumerate(seqs):
            h = self.hist[s]
            assert pos0[i] <= len(h)
            del h[pos0[i]:]
            h.extend(int(t) for t in runs[i])
            digest = hashlib.sha256(np.asarray(h, dtype=np.int64).tobytes()).digest()
            x = (np.frombuffer(digest[:V], dtype=np.uint8).astype(np.float32) - 128.0) / 16.0
            given = {k: kw[k][i] for k in kw if k != "allowed" and kw[k][i] is not None}
            if given:
                self.controlled.append((list(h), given))
            if hist[i] is not None:
                assert list(hist[i]) == h[1:] and h[0] == BOS, (i, hist[i], h)      # everything fed after BOS, this step's included
            else:
                assert (rep[i], pres[i], freq[i]) == (1.0, 0.0, 0.0)
            x = R.penalise(x, hist[i], rep[i], pres[i], freq[i])
            if allowed[i] is not None:
                ban = np.ones(V, dtype=bool)
                ban[list(allowed[i])] = False
                x[ban] = -np.inf
            if temperature[i] == 0.0:
                assert top_k[i] == 0 and min_p[i] == 0.0
                picks.append(int(np.argmax(x)))
            else:
                alive = np.flatnonzero(~np.isneginf(R.truncate(x, temperature[i], top_k[i], min_p[i])))
                picks.append(int(alive[int.from_bytes(digest[8:16], "little") % alive.size]))
        return (picks, list(rng)) + ((np.zeros((n, V), dtype=np.float32),) if logits else ())


KINDS = [
    {},                                                                     # plain, through submit
    dict(repetition_penalty=1.3),
    dict(presence_penalty=0.75, temperature=0.8, topp=0.9),
    dict(frequency_penalty=0.5, top_k=4, temperature=1.2),
    dict(top_k=1, temperature=0.9, topp=0.9),
    dict(min_p=0.2, temperature=0.7),
    dict(repetition_penalty=0.8, presence_penalty=-0.25, frequency_penalty=0.125, top_k=6, min_p=0.05, temperature=1.0, allowed=list(range(1, 20))),
    dict(top_k=5, min_p=0.3),                                               # greedy: stage B is ignored, no keyword travels
]


def requests(n=32):
    rng = np.random.default_rng(23)
    stem = [int(t) for t in rng.integers(2, V, 7)]
    out = []
    for i in range(n):
        own = [int(t) for t in rng.integers(2, V, int(rng.integers(0, 24)))]
        out.append(((stem if i % 3 == 0 else []) + own, int(rng.integers(1, 60)), KINDS[i % len(KINDS)]))
    return out


def submit(sch, prompt, steps, kind, seed=5):
    if not kind:
        return sch.submit(prompt, steps)
    return sch.submit_sampling(prompt, steps, seed=seed, **kind)


def attach_fork(ctx):
    ctx.seq_fork = lambda src, dsts, rows: [ctx.hist.__setitem__(d, ctx.hist[src][:rows]) for d in dsts]


@pytest.mark.parametrize("prefix_cache", [False, True])
def test_scheduler_controls(prefix_cache):
    reqs = requests()
    ctx = StubContext(5, 64)
    attach_fork(ctx)
    sch = serve.Scheduler(ctx, max_rows=24, prefix_cache=prefix_cache)
    rids = [submit(sch, p, steps, kind) for p, steps, kind in reqs]
    res = sch.run()
    for i, (prompt, steps, kind) in enumerate(reqs):
        solo_ctx = StubContext(1, 64)
        solo = serve.Scheduler(solo_ctx, max_rows=8)
        rid = submit(solo, prompt, steps, kind)
        want = solo.run()[rid]
        got = res[rids[i]]
        assert (got.tokens_fed, got.finish) == (want.tokens_fed, want.finish), i
        neutral = not kind or (kind.get("temperature", 0.0) == 0.0 and not any(k.endswith("penalty") for k in kind))
        if neutral:
            assert all(not kw for _, kw in solo_ctx.calls) and not solo_ctx.controlled, i
    # every row that carried a control was a real pick: its sequence held the whole prompt, and the history was checked by the stand-in
    assert len(ctx.controlled) > 100
    known = {tuple([BOS] + p[:p.index(BOS)] if BOS in p else [BOS] + p) for p, _, kind in reqs if kind}
    for held, given in ctx.controlled:
        assert any(len(held) >= len(k) and tuple(held[:len(k)]) == k for k in known), held
    seen = set().union(*[set(kw) for _, kw in ctx.calls])
    assert seen >= {"history", "repetition_penalty", "presence_penalty", "frequency_penalty", "top_k", "min_p"}
    if prefix_cache:
        assert sch.rows_reused > 0


@pytest.mark.parametrize("prefix_cache", [False, True])
def test_neutral_settings_make_the_calls_of_submit(prefix_cache):
    reqs = requests(20)
    logs = []
    for neutral in (False, True):
        ctx = StubContext(4, 64)
        attach_fork(ctx)
        sch = serve.Scheduler(ctx, max_rows=16, prefix_cache=prefix_cache)
        for i, (p, steps, _) in enumerate(reqs):
            t, tp = ((0.0, 1.0), (0.9, 0.9))[i % 2]
            if neutral:
                sch.submit_sampling(p, steps, temperature=t, topp=tp, seed=7 + i, **CONTROLS)
            else:
                sch.submit(p, steps, temperature=t, topp=tp, seed=7 + i)
        res = sch.run()
        logs.append((ctx.calls, [(r.tokens_fed, r.finish, r.rng_state) for _, r in sorted(res.items())]))
    assert logs[0] == logs[1] and logs[0][0] and all(not kw for _, kw in logs[0][0])


def test_a_prompt_chunk_carries_no_controls():
    ctx = StubContext(2, 64)
    sch = serve.Scheduler(ctx, max_rows=4)
    prompt = [3, 4, 5, 6, 7, 8, 9, 10, 11]
    a = sch.submit_sampling(prompt, 14, temperature=0.9, seed=3, repetition_penalty=1.2, frequency_penalty=0.5, top_k=3, min_p=0.1)
    sch.step()                                   # rows 0 .. 3 of the prompt: the pick is thrown away
    sch.step()                                   # rows 4 .. 7
    assert [kw for _, kw in ctx.calls] == [{}, {}] and not ctx.controlled
    sch.step()                                   # rows 8, 9: the prompt's last position, the first real pick
    kw = ctx.calls[-1][1]
    assert kw == dict(history=[prompt], repetition_penalty=[1.2], frequency_penalty=[0.5], top_k=[3], min_p=[0.1])
    res = sch.run()[a]
    hists = [kw["history"][0] for _, kw in ctx.calls[2:]]
    assert hists == [res.tokens_fed[1:len(prompt) + 1 + k] for k in range(len(hists))] and len(hists) == 14 - len(prompt)
    # a second request in its prompt beside a generating one: None in every column of its row
    ctx2 = StubContext(2, 64)
    sch2 = serve.Scheduler(ctx2, max_rows=3)
    sch2.submit_sampling([5], 8, repetition_penalty=1.5)
    sch2.step()
    sch2.submit_sampling(list(range(2, 14)), 20, temperature=0.9, top_k=2, presence_penalty=1.0)
    sch2.step()
    args, kw = ctx2.calls[-1]
    assert len(args[0]) == 2 and kw == dict(history=[[5, kw["history"][0][1]], None], repetition_penalty=[1.5, None])
    with pytest.raises(ValueError):
        sch2.submit_sampling([5], 8, repetition_penalty=0.0)
    with pytest.raises(ValueError):
        sch2.submit_sampling([5], 8, temperature=-1.0, top_k=3)
    with pytest.raises(ValueError):
        sch2.submit_sampling([5], 8, min_p=1.5)
