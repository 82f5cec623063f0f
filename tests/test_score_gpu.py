"""Per-token log-probabilities on the device (include/llama2_hip.h: l2_seq_score_batch, l2_step_batch_logprobs; csrc/logprob.hip.h).
Scoring is held to the reference's greedy goldens (argmax, and lps against a numpy fp64 log-softmax of its kept logits), to the
last-row logits that l2_seq_prefill_batch returns for the same prefixes on a twin context, and to the oracle on random tokens; the
state it leaves to l2_seq_prefill_batch's.  The row kernel itself is held to numpy on the exact logits l2_step_batch_logprobs hands
back, the step's other outputs to l2_step_batch on a twin, the argmax and non-finite rules to the reference's edge models."""
import json
import os

import numpy as np
import pytest

import argmax_cases as A
import oracle_lib as O
from llama2_ts_amd import runtime, serve

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
E_ARG, E_STATE = -1, -4


def load_gold(name):
    meta = json.load(open(os.path.join(GOLD, name + ".json")))
    return meta, np.load(os.path.join(GOLD, name + ".npz"))


def new_ctx(hdr, seed, n_seqs, opts=None):
    ctx = runtime.Context(hdr)
    ctx.synth_fill(seed)
    ctx.seq_reserve(n_seqs)
    for k, v in (opts or {}).items():
        ctx.set_option(k, v)
    return ctx


def code_of(fn, *args, **kw):
    with pytest.raises(runtime.L2Error) as e:
        fn(*args, **kw)
    return e.value.code


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def top_order(x, k):
    """The k largest logits' ids: descending value, equal values by ascending id."""
    return np.lexsort((np.arange(x.size), -np.asarray(x, dtype=np.float64)))[:k]


@pytest.mark.parametrize("name", ["tiny", "stories15M", "stories110M", "tinylong", "llama2_7b_L2"])
def test_greedy_goldens(name):
    """tokens_fed scored as one run at position 0, each row's target the next fed token."""
    meta, g = load_gold(name)
    hdr = meta["header"]
    fed = meta["tokens_fed"][:hdr[6]]
    R = len(fed)
    ctx = new_ctx(hdr, meta["seed"], 1)
    lp, am, ids, tlp = ctx.seq_score_batch([0], [fed], 0, top_k=3)
    assert lp.shape == (R,) and ids.shape == (R, 3)
    assert am[:R - 1].tolist() == fed[1:] == meta["argmax"][:R - 1], name
    assert np.isnan(lp[R - 1]) and (ids[:, 0] == am).all()
    for i, p in enumerate(meta["logit_positions"]):
        if p >= R - 1:
            continue
        want = log_softmax(g["logits"][i])
        assert abs(lp[p] - want[fed[p + 1]]) <= 2e-4, (name, p, lp[p], want[fed[p + 1]])
        assert np.abs(tlp[p] - want[ids[p]]).max() <= 2e-4, (name, p)
    ctx.close()


RUN_LENGTHS = (1, 2, 15, 16, 17, 64, 65, 255, 300)


def test_packed_shuffled_runs_against_the_last_row_logits():
    """Runs of many lengths in one shuffled call (sequence 0 among them, runs straddling the 256-row launch boundary, a suffix at pos0 > 0
    after a prefill); sampled rows' lps against the log-softmax of l2_seq_prefill_batch's last-row logits for the same prefix."""
    meta, _ = load_gold("stories110M")
    hdr, fed = meta["header"], meta["tokens_fed"]
    rng = np.random.default_rng(7)
    order = [int(i) for i in rng.permutation(len(RUN_LENGTHS))]
    seqs = [int(s) for s in rng.permutation(len(RUN_LENGTHS) + 1)]         # one sequence more: the suffix run
    runs, pos0 = [fed[:RUN_LENGTHS[i]] for i in order], [0] * len(order)
    pre = 40                                                                # the suffix: rows 40 .. 139 after a prefill of 0 .. 39
    runs.insert(3, fed[pre:pre + 100]); pos0.insert(3, pre)
    assert 0 in seqs
    ctx = new_ctx(hdr, meta["seed"], 64)
    ctx.seq_prefill_batch([seqs[3]], [fed[:pre]], 0)
    lp, am, ids, tlp = ctx.seq_score_batch(seqs, runs, pos0, top_k=4)
    R = sum(len(r) for r in runs)
    first = np.cumsum([0] + [len(r) for r in runs])
    assert any(first[i] < 256 < first[i + 1] for i in range(len(runs))) and R > 512
    picks = []                                                              # (run, offset in run, packed row)
    for i, r in enumerate(runs):
        for o in {0, 15, 16, len(r) - 1}:
            if 0 <= o < len(r):
                picks.append((i, o, first[i] + o))
        for b in (255, 256, 511, 512):
            if first[i] <= b < first[i + 1]:
                picks.append((i, b - first[i], b))
    picks = sorted(set(picks), key=lambda t: t[2])
    twin = new_ctx(hdr, meta["seed"], 64)
    for c0 in range(0, len(picks), 64):
        grp = picks[c0:c0 + 64]
        prefixes = [fed[:pos0[i] + o + 1] for i, o, _ in grp]
        lg = twin.seq_prefill_batch(list(range(len(grp))), prefixes, 0)
        for (i, o, r), row in zip(grp, lg):
            want = log_softmax(row)
            tgt = runs[i][o + 1] if o + 1 < len(runs[i]) else None
            if tgt is None:
                assert np.isnan(lp[r])
            else:
                assert abs(lp[r] - want[tgt]) <= 2e-5, (i, o, r)
            assert am[r] == runtime.argmax(row), (i, o, r)
            assert ids[r].tolist() == top_order(row, 4).tolist() and np.abs(tlp[r] - want[ids[r]]).max() <= 2e-5, (i, o, r)
    twin.close()
    ctx.close()


def test_random_token_runs_against_the_oracle():
    """Random tokens (64-row launch sequences on this shape), every row held to the oracle's logits within 2e-4."""
    hdr = tuple(load_gold("tiny")[0]["header"])
    seed = 5
    rng = np.random.default_rng(3)
    runs = [[int(t) for t in rng.integers(0, hdr[5], n)] for n in (37, 1, 64, 50)]
    ctx = new_ctx(hdr, seed, 4)
    lp, am, _, _ = ctx.seq_score_batch([2, 0, 3, 1], runs, 0)
    r = 0
    for run in runs:
        orc = O.Oracle(hdr, seed)
        for p, tok in enumerate(run):
            want = log_softmax(orc.forward(tok, p))
            if p + 1 < len(run):
                assert abs(lp[r] - want[run[p + 1]]) <= 2e-4, (r, p)
            assert am[r] == int(np.argmax(want)) or abs(want[am[r]] - want.max()) <= 2e-4
            r += 1
        orc.close()
    ctx.close()


def test_state_after_scoring_is_that_of_the_packed_prefill():
    meta, _ = load_gold("stories15M")
    hdr, fed = meta["header"], meta["tokens_fed"]
    d, L, S = hdr[0], hdr[2], hdr[6]
    seqs, runs, pos0 = [1, 0, 2], [fed[:100], fed[:7], fed[:200]], [0, 0, 0]
    a = new_ctx(hdr, meta["seed"], 3, {runtime.OPT_CHECK_POS: 1})
    b = new_ctx(hdr, meta["seed"], 3, {runtime.OPT_CHECK_POS: 1})
    a.seq_score_batch(seqs, runs, pos0, top_k=2)
    b.seq_prefill_batch(seqs, runs, pos0)
    for s in seqs:
        for name in ("key_cache", "value_cache"):
            assert np.array_equal(a.read_seq_cache(s, name), b.read_seq_cache(s, name)), (s, name)
    nxt = [[fed[len(r)]] for r in runs]
    ends = [len(r) for r in runs]
    pa, _ = a.step_batch(seqs, nxt, ends)
    pb, _ = b.step_batch(seqs, nxt, ends)
    assert pa == pb == [meta["argmax"][e] for e in ends]
    # the next positions moved as the prefill's did: one past each run's end continues, beyond it is a skip-ahead on both
    assert code_of(a.seq_score_batch, [0], [[5]], [ends[1] + 3]) == code_of(b.seq_prefill_batch, [0], [[5]], [ends[1] + 3]) == E_STATE
    a.close()
    b.close()


def test_step_logprobs_match_numpy_and_leave_the_step_alone():
    """The kernel on the exact logits it read (l2_step_batch_logprobs with logits_out), greedy and sampled rows mixed, and every
    other output bit-identical to l2_step_batch on a twin context."""
    meta, _ = load_gold("stories15M")
    hdr, fed = meta["header"], meta["tokens_fed"]
    d, L, S = hdr[0], hdr[2], hdr[6]
    seqs = [3, 0, 5, 1, 4, 2]
    runs = [fed[:9], [fed[20]], fed[:70], [fed[33]], fed[:2], [fed[50]]]
    pos0 = [0, 20, 0, 33, 0, 50]
    temp = [0.0, 0.9, 0.0, 1.3, 0.7, 0.0]
    topp = [1.0, 0.9, 1.0, 0.0, 0.95, 1.0]
    rng = [11, 22, 33, 44, 55, 66]
    a = new_ctx(hdr, meta["seed"], 6)
    b = new_ctx(hdr, meta["seed"], 6)
    for c in (a, b):
        c.seq_prefill_batch([0, 1, 2], [fed[:20], fed[:33], fed[:50]], 0)
    pa, ra, la, (plp, ids, tlp) = a.step_batch(seqs, runs, pos0, temp, topp, rng, logits=True, logprobs=20)
    pb, rb, lb = b.step_batch(seqs, runs, pos0, temp, topp, rng, logits=True)
    assert pa == pb and ra == rb and np.array_equal(la, lb)
    for s in seqs:
        for name in ("key_cache", "value_cache"):
            assert np.array_equal(a.read_seq_cache(s, name), b.read_seq_cache(s, name)), (s, name)
    for i in range(len(seqs)):
        want = log_softmax(la[i])
        assert abs(plp[i] - want[pa[i]]) <= 1e-10, i
        assert ids[i].tolist() == top_order(la[i], 20).tolist(), i
        assert np.abs(tlp[i] - want[ids[i]]).max() <= 1e-10, i
        if temp[i] == 0.0:
            assert ids[i, 0] == pa[i]
    # top_k 0 and 5 give the same pick lps, and the same ids as the head of the 20
    _, _, (p0_, i0_, t0_) = a.step_batch(seqs, runs, pos0, temp, topp, rng, logprobs=0)
    _, _, (p5_, i5_, t5_) = a.step_batch(seqs, runs, pos0, temp, topp, rng, logprobs=5)
    assert np.array_equal(p0_, plp) and np.array_equal(p5_, plp) and i0_.shape == (6, 0)
    assert np.array_equal(i5_, ids[:, :5]) and np.array_equal(t5_, tlp[:, :5])
    a.close()
    b.close()


def _upload(ctx, tensors):
    for kind, layers, count in runtime.tensor_shapes(ctx.cfg):
        per = tensors[kind].reshape(max(layers, 1), -1)
        for layer in range(max(layers, 1)):
            ctx.upload(kind, layer if layers else -1, per[layer])


# V % 4 != 0 (the kernel's scalar row reads) on a shape the batch path takes: argmax_cases' own `odd` shape (dim 66) is refused by it
ODD_BATCH = (64, 176, 2, 4, 4, -517, 48)


def key_order(x, k):
    """The k largest argmax_keys (kernels.hip.h) of a logits row: descending value with -0 == +0, a NaN below -inf except at index 0
    (above everything: the reference's reduce() never leaves it), equal values by ascending index."""
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    v = np.where(nan, -np.inf, x.astype(np.float64) + 0.0)
    rank = np.where(nan, 0, 1)
    rank[0] = 2 if nan[0] else 1
    return np.lexsort((np.arange(x.size), -v, -rank))[:k]


def non_finite(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.isnan(x).any() or np.isposinf(x).any() or not (x > -np.inf).any())


def close_lps(got, want, tol):
    """-inf where numpy has -inf, within tol elsewhere."""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    ninf = np.isneginf(want)
    return bool(np.array_equal(np.isneginf(got), ninf) and np.abs(got[~ninf] - want[~ninf]).max(initial=0.0) <= tol)


@pytest.mark.parametrize("shape", ["vec", "odd_batch"])
@pytest.mark.parametrize("case", A.CASES)
def test_argmax_edge_models(case, shape, monkeypatch):
    """The reference's edge models (ties, +-0, +-inf, NaN at index 0, all NaN) with 16-byte row reads (`vec`, V = 2048: the REAL
    reference's picks) and scalar ones (V = 517: the oracle's picks, which reproduce the reference's): scoring gives the reference's
    argmax at every position; the step, on the exact logits it hands back, the full top-k in key order (ties by ascending index) and
    the lps of numpy's log-softmax; and both follow the non-finite rule."""
    monkeypatch.setitem(A.SHAPES, "odd_batch", ODD_BATCH)
    if shape == "vec":
        meta = json.load(open(os.path.join(GOLD, "argmax_%s_vec.json" % case)))
        fed, picks = meta["tokens_fed"], meta["picks"]
        _, _, want_logits = A.oracle_run(case, shape, len(picks))
    else:
        fed, picks, want_logits = A.oracle_run(case, shape, 16)
    n = len(picks)
    ctx = runtime.Context(A.SHAPES[shape])
    _upload(ctx, A.tensors_of(case, shape))
    ctx.seq_reserve(n)
    lp, am, ids, tlp = ctx.seq_score_batch([0], [fed[:n]], 0, targets=picks, top_k=6)
    assert am.tolist() == picks, (case, shape)
    assert (ids[:, 0] == am).all()
    for r in range(n):
        x = np.asarray(want_logits[r], dtype=np.float64)
        if non_finite(x):
            assert np.isnan(lp[r]) and np.isnan(tlp[r]).all(), (case, shape, r)
        else:
            want = log_softmax(x)
            assert close_lps(lp[r], want[picks[r]], 2e-4) and close_lps(tlp[r], want[ids[r]], 2e-4), (case, shape, r)
    # the step: position p is the last row of a prefix run on sequence p
    spicks, _, lg, (plp, sids, stlp) = ctx.step_batch(list(range(n)), [fed[:p + 1] for p in range(n)], 0, logits=True, logprobs=6)
    assert spicks == picks, (case, shape)
    for r in range(n):
        assert sids[r].tolist() == key_order(lg[r], 6).tolist(), (case, shape, r)
        if non_finite(lg[r]):
            assert np.isnan(plp[r]) and np.isnan(stlp[r]).all(), (case, shape, r)
        else:
            want = log_softmax(lg[r])
            assert close_lps(plp[r], want[spicks[r]], 1e-10) and close_lps(stlp[r], want[sids[r]], 1e-10), (case, shape, r)
    ctx.close()


@pytest.mark.parametrize("hdr", [(64, 176, 2, 4, 4, 128256, 64), (64, 176, 2, 4, 4, 517, 64), (64, 176, 2, 4, 4, -517, 64)],
                         ids=["V128256", "V517", "V517_unshared"])
def test_vocabulary_sizes(hdr):
    """Scalar and vector row reads, a large vocabulary, an unshared classifier: the step's lps on its exact logits, and the scoring
    call's rows against the packed prefill's last-row logits."""
    V = abs(hdr[5])
    ctx = new_ctx(hdr, 9, 3)
    rng = np.random.default_rng(1)
    runs = [[int(t) for t in rng.integers(0, V, n)] for n in (20, 1, 33)]
    picks, _, lg, (plp, ids, tlp) = ctx.step_batch([0, 1, 2], runs, 0, logits=True, logprobs=20)
    for i in range(3):
        want = log_softmax(lg[i])
        assert picks[i] == runtime.argmax(lg[i]) == ids[i, 0]
        assert abs(plp[i] - want[picks[i]]) <= 1e-10 and ids[i].tolist() == top_order(lg[i], 20).tolist()
        assert np.abs(tlp[i] - want[ids[i]]).max() <= 1e-10
    twin = new_ctx(hdr, 9, 3)
    targets = [int(t) for t in rng.integers(-1, V, sum(len(r) for r in runs))]
    lp, am, sids, _ = twin.seq_score_batch([0, 1, 2], runs, 0, targets=targets, top_k=20)
    ends = np.cumsum([len(r) for r in runs]) - 1
    for i, r in enumerate(ends):
        want = log_softmax(lg[i])
        assert am[r] == picks[i] and sids[r].tolist() == ids[i].tolist()
        assert (np.isnan(lp[r]) if targets[r] < 0 else abs(lp[r] - want[targets[r]]) <= 2e-5)
    twin.close()
    ctx.close()


def test_errors_and_repeatability():
    meta, _ = load_gold("tiny")
    hdr, fed = meta["header"], meta["tokens_fed"]
    V = hdr[5]
    ctx = runtime.Context(hdr)
    ctx.synth_fill(meta["seed"])
    assert code_of(ctx.seq_score_batch, [0], [fed[:5]]) == E_STATE               # before seq_reserve
    ctx.seq_reserve(2)
    import ctypes as C
    L = runtime.lib()
    s = (C.c_int32 * 1)(0)
    nt = (C.c_int32 * 1)(4)
    tok = (C.c_int32 * 4)(*fed[:4])
    p0 = (C.c_int32 * 1)(0)
    tg = (C.c_int32 * 4)(5, 6, 7, -1)
    bad = (C.c_int32 * 4)(5, V, 7, -1)
    low = (C.c_int32 * 4)(5, -2, 7, -1)
    lp = (C.c_double * 4)(*([9.0] * 4))
    am = (C.c_int32 * 4)(*([-9] * 4))
    ids = (C.c_int32 * 80)(*([-9] * 80))
    tlp = (C.c_double * 80)(*([9.0] * 80))
    assert L.l2_seq_score_batch(ctx._h, 1, s, nt, tok, p0, None, 0, lp, am, None, None) == E_ARG
    assert L.l2_seq_score_batch(ctx._h, 1, s, nt, tok, p0, tg, 0, None, am, None, None) == E_ARG
    assert L.l2_seq_score_batch(ctx._h, 1, s, nt, tok, p0, bad, 0, lp, am, None, None) == E_ARG
    assert L.l2_seq_score_batch(ctx._h, 1, s, nt, tok, p0, low, 0, lp, am, None, None) == E_ARG
    assert L.l2_seq_score_batch(ctx._h, 1, s, nt, tok, p0, tg, 21, lp, am, ids, tlp) == E_ARG
    assert L.l2_seq_score_batch(ctx._h, 1, s, nt, tok, p0, tg, 3, lp, am, None, tlp) == E_ARG
    assert list(lp) == [9.0] * 4 and list(am) == [-9] * 4 and list(ids) == [-9] * 80 and list(tlp) == [9.0] * 80
    one = (C.c_int32 * 1)(1)
    picks = (C.c_int32 * 1)(-9)
    assert L.l2_step_batch_logprobs(ctx._h, 1, s, one, tok, p0, None, None, None, picks, None, 0, None, None, None) == E_ARG
    assert L.l2_step_batch_logprobs(ctx._h, 1, s, one, tok, p0, None, None, None, picks, None, 21, lp, ids, tlp) == E_ARG
    assert picks[0] == -9 and list(lp) == [9.0] * 4
    # the context still decodes; an L2_OPT_CHECK_POS skip-ahead is refused
    assert ctx.step_batch([0], [fed[:6]], 0)[0] == [meta["argmax"][5]]
    ctx.set_option(runtime.OPT_CHECK_POS, 1)
    assert code_of(ctx.seq_score_batch, [1], [fed[3:6]], 3) == E_STATE
    ctx.set_option(runtime.OPT_CHECK_POS, 0)
    # the same call twice: bit-identical
    one_ = ctx.seq_score_batch([1, 0], [fed[:40], fed[:33]], 0, top_k=20)
    two_ = ctx.seq_score_batch([1, 0], [fed[:40], fed[:33]], 0, top_k=20)
    for x, y in zip(one_, two_):
        assert np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)
    ctx.close()


@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_scheduler_logprobs(temperature):
    meta, _ = load_gold("stories15M")
    hdr = meta["header"]
    out = []
    for lp_k in (None, 5):
        ctx = new_ctx(hdr, meta["seed"], 4)
        sch = serve.Scheduler(ctx, max_rows=48, keep_logits=True)
        rids = [sch.submit(p, 40, temperature=temperature, topp=0.9, seed=100 + i, logprobs=lp_k)
                for i, p in enumerate([[5, 6, 7], [9] * 20, [3], [40, 41, 42, 43, 44, 45]])]
        res = sch.run()
        out.append([res[r] for r in rids])
        ctx.close()
    for a, b in zip(*out):
        assert a.tokens_fed == b.tokens_fed and a.rng_state == b.rng_state and a.logprobs is None
        assert len(b.logprobs) == len(b.logits)
        for (lp, top), row in zip(b.logprobs, b.logits):
            want = log_softmax(row)
            assert len(top) == 5 and [t for t, _ in top] == top_order(row, 5).tolist()
            assert np.abs(np.array([v for _, v in top]) - want[[t for t, _ in top]]).max() <= 1e-10
        picks = b.tokens_fed[len(b.tokens_fed) - len(b.logprobs) + 1:] + ([1] if b.finish == "bos" else [])
        for (lp, _), row, t in zip(b.logprobs, b.logits, picks):
            assert abs(lp - log_softmax(row)[t]) <= 1e-10
