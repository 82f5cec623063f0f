"""Sampling controls on the device (include/llama2_hip.h: l2_step_batch_sampling, l2_debug_sample_controls; csrc/controls.hip.h).
First the two rewriting launches alone, through the diagnostic, bit for bit against tests/controls_ref.py over vocabulary sizes,
history shapes and planted edges.  Then one mixed call per shape of tests/test_constrain_gpu.py that carries every row kind under
every sampler setting: its visible logits are held to the plain step's on a twin context passed through stage A and the constraints,
its picks and rng states to the oracle's sampler fed the truncated rows (with the stated fall-through rule), its log-probabilities
to a host fp64 log-softmax of the visible rows; then the refusals, and the scheduler against each request run alone."""
import numpy as np
import pytest

import controls_ref as R
import oracle_lib as O
import test_constrain_gpu as TC
from llama2_ts_amd import runtime, serve

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -4
BOS = 1
MARGIN = 1e-9
SHAPES, SETTINGS = TC.SHAPES, TC.SETTINGS


def same_bits(got, want):
    """Bit for bit, a NaN for a NaN (the payload of a NaN that went through a multiply is the hardware's)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)))


# ---- the two launches alone ------------------------------------------------------------------------------------------------------
VOCABS = [1, 2, 63, 64, 65, 97, 1024, 1025, 2083, 32000]
LENGTHS = [0, 1, 2, 63, 64, 65, 1024, 1025, 2048]
PENALTIES = [(1.25, 0.0, 0.0), (0.75, 0.0, 0.0), (1.0, 0.5, 0.0), (1.0, 0.0, 0.375), (1.5, -0.25, 0.125), (0.5, 1.0, -0.0625)]


def grid_row(rng, v):
    """Logits on a grid of 1/8 (many exact ties), with +0 / -0 and -inf entries planted."""
    x = (rng.integers(-48, 49, v) / 8.0).astype(np.float32)
    if v >= 8:
        x[rng.choice(v, 3, replace=False)] = -np.inf
        a, b = rng.choice(v, 2, replace=False)
        x[a], x[b] = 0.0, -0.0
    return x


def history_of(rng, v, length, kind):
    if kind == "repeat":
        return [int(rng.integers(0, v))] * length
    if kind == "distinct":                       # all ids distinct while the vocabulary has that many
        return [int(t) for t in np.resize(rng.permutation(v), length)]
    h = [int(t) for t in rng.integers(0, v, length)]
    h[::2] = [0] * len(h[::2])                   # ids 0 and V - 1, each many times, among others
    h[1::3] = [v - 1] * len(h[1::3])
    return h


def tie_ks(x):
    """k inside and at both ends of the largest tie group of the row's ranking (and one past each end)."""
    keys = np.sort(R.rank_keys(x))[::-1]
    vals, first, counts = np.unique(-keys, return_index=True, return_counts=True)
    g = int(np.argmax(counts))
    a, b = int(first[g]), int(first[g] + counts[g])
    return sorted({k for k in (a, a + 1, (a + b) // 2, b - 1, b, b + 1) if 1 <= k})


def kernel_rows(v):
    """Row specifications for one vocabulary size: dict(x, hist, rep, pres, freq, temp, k, mp)."""
    rng = np.random.default_rng(1000 + v)
    rows = []
    add = lambda x, hist=(), pen=(1.0, 0.0, 0.0), temp=0.0, k=0, mp=0.0: rows.append(
        dict(x=np.asarray(x, dtype=np.float32), hist=list(hist), rep=pen[0], pres=pen[1], freq=pen[2], temp=temp, k=k, mp=mp))
    # histories: every length under every kind; penalties cycle (rep below and above 1, each alone, all together); a third truncate
    for li, length in enumerate(LENGTHS):
        for ki, kind in enumerate(("repeat", "distinct", "ends")):
            i = 3 * li + ki
            trunc = dict(temp=(0.5, 1.0, 2.0)[i % 3], k=(0, 3, 0)[ki], mp=(0.0, 0.0, 0.125)[ki]) if i % 2 else {}
            add(grid_row(rng, v), history_of(rng, v, length, kind), PENALTIES[i % len(PENALTIES)], **trunc)
    # a min_p row whose maximum is itself penalised (it stays the maximum, or another entry takes over)
    for pen in ((1.5, 0.0, 0.0), (1.0, 2.0, 0.5)):
        x = grid_row(rng, v)
        top = int(np.argmax(x))
        add(x, [top, top, int(rng.integers(0, v))], pen, temp=0.5, mp=0.25)
    # ties across the k-th rank
    x = grid_row(rng, v)
    for k in tie_ks(x):
        add(x, temp=1.0, k=k)
    # k at the edges, alone and with min_p; min_p alone, 1.0 included
    x = grid_row(rng, v)
    for k in (1, 2, v - 1, v, v + 5):
        add(x, temp=2.0, k=k)
        add(x, temp=0.5, k=k, mp=0.0625)
    for mp in (0.03125, 0.3, 1.0):
        add(grid_row(rng, v), temp=(1.0, 0.25, 4.0)[rows.__len__() % 3], mp=mp)
    # fewer finite entries than k; all entries equal; every entry -inf but one; a greedy row that asks for truncation (ignored)
    few = np.full(v, -np.inf, dtype=np.float32)
    few[rng.choice(v, min(v, 3), replace=False)] = [1.5, -2.0, 1.5][:min(v, 3)]
    add(few, temp=1.0, k=5)
    add(few, temp=1.0, k=2, mp=0.5)
    for k in (1, 2, v - 1):
        add(np.full(v, -0.75, dtype=np.float32), temp=1.0, k=k, mp=1.0)
    add(grid_row(rng, v), [0, v - 1], (1.25, 0.5, 0.5), temp=0.0, k=3, mp=0.5)
    assert len(rows) <= 64
    return rows


def reference_rows(rows):
    pen = [R.penalise(r["x"], r["hist"], r["rep"], r["pres"], r["freq"]) for r in rows]
    for r, p in zip(rows, pen):
        if r["temp"] != 0.0 and r["mp"] > 0.0:      # no case may hang on the last place of log(min_p)
            assert R.min_p_clearance(p, r["temp"], r["mp"]) > MARGIN, (r["temp"], r["mp"])
    return pen, [R.truncate(p, r["temp"], r["k"], r["mp"]) for r, p in zip(rows, pen)]


@pytest.mark.parametrize("v", VOCABS)
def test_the_two_launches_match_the_numpy_statement(v):
    rows = kernel_rows(v)
    want_pen, want_tr = reference_rows(rows)
    col = lambda key: [r[key] for r in rows]
    got_pen, got_tr = runtime.debug_sample_controls(np.stack(col("x")), col("temp"), history=col("hist"), repetition_penalty=col("rep"),
                                                    presence_penalty=col("pres"), frequency_penalty=col("freq"), top_k=col("k"), min_p=col("mp"))
    changed = cut = 0
    for i, r in enumerate(rows):
        assert same_bits(got_pen[i], want_pen[i]), (v, i, "stage A", r["rep"], r["pres"], r["freq"], len(r["hist"]))
        assert same_bits(got_tr[i], want_tr[i]), (v, i, "stage B", r["temp"], r["k"], r["mp"])
        changed += not same_bits(want_pen[i], r["x"])
        cut += int(np.isneginf(want_tr[i]).sum() - np.isneginf(want_pen[i]).sum()) > 0
    assert changed >= 10 and cut >= (8 if v > 2 else 0), (changed, cut)
    # the same rows with nothing switched on come back as they went in
    n = len(rows)
    p2, t2 = runtime.debug_sample_controls(np.stack(col("x")), col("temp"), history=col("hist"), top_k=[0] * n, min_p=[None] * n)
    assert all(same_bits(p2[i], r["x"]) and same_bits(t2[i], r["x"]) for i, r in enumerate(rows))


# ---- the mixed step ------------------------------------------------------------------------------------------------------------------
KINDS = ["none", "rep", "pres", "freq", "pen3", "pen_bias_mask", "k1", "k5", "kV", "mp05", "mp1", "all"]
PRE = TC.PRE


def rows_of(V, S):
    """The call's rows: every kind under every setting; row i is a prompt run when i % 3 == 1, else a decode row."""
    rng = np.random.default_rng(V + 1)
    third = sorted(int(t) for t in rng.choice(np.arange(1, V), V // 3, replace=False))
    rows = []
    for kind in KINDS:
        for temp, topp in SETTINGS:
            i = len(rows)
            base = [int(t) for t in rng.integers(0, V, 1 + i % (S - 8))]
            hist = (base + base[:3] * 2 + [third[0], third[0]])[:S]          # repeats whatever V is; an allowed id among them
            row = dict(kind=kind, temp=temp, topp=topp, n_tok=2 + 3 * (i % 5) if i % 3 == 1 else 1, seed=2000 + 13 * i,
                       allowed=None, bias=None, hist=None, rep=None, pres=None, freq=None, k=None, mp=None)
            if kind in ("rep", "pen3", "pen_bias_mask", "all"):
                row["rep"] = (1.3, 0.8)[i % 2]
            if kind in ("pres", "pen3", "pen_bias_mask", "all"):
                row["pres"] = (0.75, -0.5)[i % 2]
            if kind in ("freq", "pen3", "pen_bias_mask", "all"):
                row["freq"] = 0.375
            if row["rep"] or row["pres"] or row["freq"]:
                row["hist"] = hist
            if kind in ("pen_bias_mask", "all"):
                row["allowed"] = third
                row["bias"] = {0: 5.0, third[0]: 3.0, third[-1]: -2.0, third[len(third) // 2]: 9.5}      # id 0 is not allowed
            row["k"] = {"k1": 1, "k5": 5, "kV": V, "all": 5}.get(kind)
            row["mp"] = {"mp05": 0.05, "mp1": 1.0, "all": 0.05}.get(kind)
            rows.append(row)
    return rows


def controls_kw(rows):
    return dict(history=[r["hist"] for r in rows], repetition_penalty=[r["rep"] for r in rows], presence_penalty=[r["pres"] for r in rows],
                frequency_penalty=[r["freq"] for r in rows], top_k=[r["k"] for r in rows], min_p=[r["mp"] for r in rows])


def visible_row(x, row):
    """x' of a row from the plain step's x: stage A, then the constraints' rewrite."""
    pen = R.penalise(x, row["hist"], row["rep"] or 1.0, row["pres"] or 0.0, row["freq"] or 0.0)
    return TC.expected_row(pen, row)


def sampled_row(xp, row):
    return R.truncate(xp, row["temp"], row["k"] or 0, row["mp"] or 0.0)


_RUNS = {}


def run_shape(name):
    """The controlled call on one context and the plain logprobs call on its twin, for top_k 0 and 5 (fresh rng seeds each); computed
    once per shape and read by every test of it."""
    if name in _RUNS:
        return _RUNS[name]
    hdr = SHAPES[name]
    V, S = abs(hdr[5]), hdr[6]
    rows = rows_of(V, S)
    n = len(rows)
    rng = np.random.default_rng(6)
    seqs = [int(s) for s in rng.permutation(n)]
    a, b = TC.new_ctx(hdr, 21, n), TC.new_ctx(hdr, 21, n)
    dec = [i for i, r in enumerate(rows) if r["n_tok"] == 1]
    pre = [[int(t) for t in rng.integers(0, V, PRE)] for _ in dec]
    runs = [[int(t) for t in rng.integers(0, V, r["n_tok"])] for r in rows]
    pos0 = [PRE if r["n_tok"] == 1 else 0 for r in rows]
    temp, topp = [r["temp"] for r in rows], [r["topp"] for r in rows]
    allowed, bias = [r["allowed"] for r in rows], [r["bias"] for r in rows]
    out = dict(V=V, rows=rows, calls=[])
    for k in (0, 5):
        seeds = [r["seed"] + k for r in rows]
        for c in (a, b):
            c.seq_prefill_batch([seqs[i] for i in dec], pre, 0)
        pa, ra, la, lpa = a.step_batch(seqs, runs, pos0, temp, topp, seeds, logits=True, logprobs=k, allowed=allowed, logit_bias=bias, **controls_kw(rows))
        pb, rb, lb, lpb = b.step_batch(seqs, runs, pos0, temp, topp, seeds, logits=True, logprobs=k)
        out["calls"].append(dict(k=k, seeds=seeds, a=(pa, ra, la, lpa), b=(pb, rb, lb, lpb)))
    out["caches_equal"] = all(np.array_equal(a.read_seq_cache(s, nm), b.read_seq_cache(s, nm)) for s in seqs for nm in ("key_cache", "value_cache"))
    ends = [p + r["n_tok"] for p, r in zip(pos0, rows)]
    nxt = [[int(t)] for t in rng.integers(0, V, n)]
    out["skip"] = [TC._code(c, [seqs[1]], [nxt[1]], [ends[1] + 1]) for c in (a, b)]
    out["follow"] = [c.step_batch(seqs, nxt, ends)[0] for c in (a, b)]
    # nothing switched on, through the new entry point: an all-neutral sc, then sc = NULL; the twin makes the plain call each time
    seeds = [r["seed"] + 9 for r in rows]
    ends1 = [e + 1 for e in ends]
    neutral = dict(history=[[3, 3, 4]] * n, repetition_penalty=[1.0] * n, presence_penalty=[0.0] * n, frequency_penalty=[None] * n,
                   top_k=[0] * n, min_p=[0.0] * n)
    out["neutral_a"] = a.step_batch(seqs, nxt, ends1, temp, topp, seeds, logits=True, logprobs=3, **neutral)
    out["neutral_b"] = b.step_batch(seqs, nxt, ends1, temp, topp, seeds, logits=True, logprobs=3)
    out["null_a"] = raw_step(a, seqs, nxt, [e + 1 for e in ends1], temp, topp, seeds, None)
    pn, rn, ln = b.step_batch(seqs, nxt, [e + 1 for e in ends1], temp, topp, seeds, logits=True)
    out["null_b"] = (pn, rn, ln)
    a.close()
    b.close()
    _RUNS[name] = out
    return out


def raw_step(ctx, seqs, runs, pos0, temp, topp, seeds, sc):
    """l2_step_batch_sampling itself with no constraints and the given l2_sample_controls pointer (None: NULL)."""
    n = len(seqs)
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    s, nt, tok, p0 = i32(seqs), i32([len(r) for r in runs]), i32(np.concatenate(runs)), i32(pos0)
    t, tp, st = np.asarray(temp, dtype=np.float64), np.asarray(topp, dtype=np.float64), np.array(seeds, dtype=np.uint64)
    picks = np.zeros(n, dtype=np.int32)
    lg = np.empty((n, ctx.cfg.vocab_size), dtype=np.float32)
    rc = runtime.lib().l2_step_batch_sampling(ctx._h, n, s.ctypes.data, nt.ctypes.data, tok.ctypes.data, p0.ctypes.data, t.ctypes.data, tp.ctypes.data,
                                              st.ctypes.data, picks.ctypes.data, lg.ctypes.data, 0, None, None, None, None, 0, None, None, None, None, sc)
    assert rc == 0, runtime.lib().l2_last_error()
    return picks.tolist(), [int(v) for v in st], lg


@pytest.mark.parametrize("name", list(SHAPES))
def test_visible_logits_are_the_plain_rows_penalised_then_constrained(name):
    run = run_shape(name)
    rows = run["rows"]
    assert any(r["n_tok"] > 1 for r in rows[:4]) and rows[0]["n_tok"] == 1      # a prompt run in front of decode rows: ord[] reorders
    for call in run["calls"]:
        (pa, ra, la, lpa), (pb, rb, lb, lpb) = call["a"], call["b"]
        for i, row in enumerate(rows):
            want, ok = visible_row(lb[i], row)
            assert np.array_equal(la[i].view(np.uint32), want.view(np.uint32)), (name, i, row["kind"])
            if row["kind"] in ("k1", "k5", "kV", "mp05", "mp1"):                # truncation alone is invisible
                assert np.array_equal(la[i].view(np.uint32), lb[i].view(np.uint32)), (name, i)
            if row["kind"] == "none":                                           # every output is the plain call's
                assert pa[i] == pb[i] and ra[i] == rb[i], (name, i)
                assert all(np.array_equal(x[i], y[i]) for x, y in zip(lpa, lpb)), (name, i)
        for kind in ("rep", "pres", "freq", "pen3", "all"):
            assert all(not np.array_equal(la[i], lb[i]) for i, r in enumerate(rows) if r["kind"] == kind), (name, kind)
    assert run["caches_equal"]
    assert run["skip"] == [E_STATE, E_STATE] and run["follow"][0] == run["follow"][1]
    na, nb = run["neutral_a"], run["neutral_b"]
    assert na[0] == nb[0] and na[1] == nb[1] and np.array_equal(na[2].view(np.uint32), nb[2].view(np.uint32))
    assert all(np.array_equal(x, y) for x, y in zip(na[3], nb[3]))
    na, nb = run["null_a"], run["null_b"]
    assert na[0] == nb[0] and na[1] == nb[1] and np.array_equal(na[2].view(np.uint32), nb[2].view(np.uint32))


@pytest.mark.parametrize("name", list(SHAPES))
def test_picks_are_the_oracle_sampler_on_the_truncated_rows(name):
    run = run_shape(name)
    rows = run["rows"]
    fell, kept = 0, 0
    for call in run["calls"]:
        pa, ra, la, _ = call["a"]
        for i, row in enumerate(rows):
            st = O.Rng(call["seeds"][i])
            if row["temp"] == 0.0:
                want = O.argmax(la[i])                                          # a greedy row ignores stage B
                assert ra[i] == call["seeds"][i]
            else:
                if row["mp"]:
                    assert R.min_p_clearance(la[i], row["temp"], row["mp"]) > MARGIN, (name, i)
                xs = sampled_row(la[i], row)
                truncated = not np.array_equal(xs.view(np.uint32), la[i].view(np.uint32))
                want = O.next_token(xs, row["temp"], row["topp"], st)[0]
                assert ra[i] == int(st.state.value), (name, i)                  # the draw was made, whatever became of the pick
                if np.isneginf(xs[want]):
                    assert want == 0, (name, i, want)                           # only the reference's `return 0` steps outside
                    want = O.argmax(xs)
                    fell += 1
                    assert row["kind"] != "k1" or 0.0 < row["topp"] < 1.0
                elif truncated or row["allowed"] is not None:
                    kept += 1
                    assert not (row["kind"] == "k1" and 0.0 < row["topp"] < 1.0), (name, i)
                assert not np.isneginf(xs[pa[i]]), (name, i)                    # every pick is a survivor
                if row["kind"] in ("k1", "mp1"):
                    assert pa[i] == O.argmax(la[i])
            assert pa[i] == want, (name, i, row["kind"], row["temp"], row["topp"])
            if row["allowed"] is not None:
                assert pa[i] in row["allowed"], (name, i)
    # top_k = 1 falls through under top-p every time (2 settings x 2 calls), never under plain `sample`
    assert fell >= 4 and kept >= 4, (fell, kept)


@pytest.mark.parametrize("name", list(SHAPES))
def test_logprobs_are_those_of_the_visible_rows(name):
    run = run_shape(name)
    rows = run["rows"]
    for call in run["calls"]:
        k = call["k"]
        pa, _, la, (plp, ids, tlp) = call["a"]
        _, _, lb, (plp_b, ids_b, tlp_b) = call["b"]
        assert ids.shape == (len(rows), k)
        for i, row in enumerate(rows):
            want = TC.log_softmax(la[i])
            assert TC.close_lps(plp[i], want[pa[i]], 1e-10) and np.isfinite(plp[i]), (name, i)
            if k:
                assert ids[i].tolist() == TC.top_order(la[i], k).tolist(), (name, i, row["kind"])
                assert TC.close_lps(tlp[i], want[ids[i]], 1e-10), (name, i)
            if row["kind"] in ("k1", "k5", "kV", "mp05", "mp1") and k:          # untouched by top_k / min_p: the twin's lists
                assert np.array_equal(ids[i], ids_b[i]) and np.array_equal(tlp[i], tlp_b[i]), (name, i)


def test_refusals_leave_the_context_alone():
    hdr = SHAPES["V97"]
    V, S = 97, hdr[6]
    a, b = TC.new_ctx(hdr, 3, 3), TC.new_ctx(hdr, 3, 3)
    for c in (a, b):
        c.seq_prefill_batch([0, 1, 2], [[5, 6, 7]] * 3, 0)
    seqs, runs, pos = [0, 1, 2], [[8], [9], [10]], [3, 3, 3]
    temp, topp, seeds = [0.9, 0.0, 0.9], [0.9, 1.0, 1.0], [11, 22, 33]
    pen = dict(repetition_penalty=[1.3, 1.3, 1.3])
    refused = [
        dict(pen, history=[[4, V], [5], [6]]),                                  # a history id equal to V
        dict(pen, history=[[4], [-1], [6]]),
        dict(pen, history=[[4], [5] * (S + 1), [6]]),                           # a count above seq_len
        dict(top_k=[None, None, 3], temperature=[0.9, 0.0, -0.9]),              # a truncating row with a negative temperature
        dict(min_p=[0.5, None, None], temperature=[-0.9, 0.0, 0.9]),
    ]
    for kw in refused:
        t = kw.pop("temperature", temp)
        assert TC._code(a, seqs, runs, pos, t, topp, seeds, **kw) == E_ARG, kw
    ok = dict(pen, history=[[4, V - 1], [5] * S, []], top_k=[3, 3, None], min_p=[None, 0.5, 0.5])
    got = a.step_batch(seqs, runs, pos, [0.9, 0.0, -0.9], topp, seeds, logits=True, **dict(ok, top_k=[3, 3, None], min_p=[None, 0.5, None]))
    assert np.isfinite(got[2]).all()                                            # a negative temperature that truncates nothing is served
    pa = a.step_batch(seqs, runs, pos, temp, topp, seeds, logits=True, **ok)
    pb = b.step_batch(seqs, runs, pos, temp, topp, seeds, logits=True, **ok)
    assert pa[0] == pb[0] and pa[1] == pb[1] and np.array_equal(pa[2].view(np.uint32), pb[2].view(np.uint32))
    for s in range(3):
        for nm in ("key_cache", "value_cache"):
            assert np.array_equal(a.read_seq_cache(s, nm), b.read_seq_cache(s, nm))
    nxt = [[int(t)] for t in pa[0]]
    assert a.step_batch(seqs, nxt, [4, 4, 4])[0] == b.step_batch(seqs, nxt, [4, 4, 4])[0]
    a.close()
    b.close()


# ---- the scheduler on the device -------------------------------------------------------------------------------------------------
CONTROL_SETS = [
    dict(repetition_penalty=1.3),
    dict(presence_penalty=0.5, frequency_penalty=0.25, top_k=8),
    dict(top_k=1),
    dict(min_p=0.1, repetition_penalty=0.9),
    dict(repetition_penalty=1.2, presence_penalty=0.25, frequency_penalty=0.125, top_k=5, min_p=0.05),
]


def alone(ctx, prompt, steps, temp, topp, seed, grammar, bias, controls):
    """The request through a plain loop of controlled steps on sequence 0: the known tokens as one run, then a pick per position."""
    known = ([BOS] + prompt)[:steps]
    fed, rng, token, run, finish = [], seed, None, known, "steps"
    pen = any(controls.get(k, off) != off for k, off in (("repetition_penalty", 1.0), ("presence_penalty", 0.0), ("frequency_penalty", 0.0)))
    while True:
        pos = len(fed)
        fed += run
        if len(fed) > len(prompt):
            kw = dict(allowed=[grammar(fed)]) if grammar else {}
            if bias:
                kw["logit_bias"] = [bias]
            if pen:
                kw["history"] = [fed[1:]]
            for k, v in controls.items():
                if not (k in ("top_k", "min_p") and temp == 0.0):
                    kw[k] = [v]
            picks, after = ctx.step_batch([0], [run], [pos], temp, topp, [rng], **kw)
            token, rng = picks[0], after[0] if temp != 0.0 else rng
            if token == BOS:
                finish = "bos"
                break
        else:
            ctx.step_batch([0], [run], [pos])
        if len(fed) >= steps:
            break
        run = [token]
    return fed, finish, rng


@pytest.mark.parametrize("prefix_cache", [False, True])
def test_scheduler_with_controls_and_a_grammar_callable(prefix_cache):
    hdr = SHAPES["tiny"]
    V = hdr[5]
    rng = np.random.default_rng(41)
    stem = [int(t) for t in rng.integers(2, V, 9)]
    reqs = []
    for i in range(24):
        own = [int(t) for t in rng.integers(2, V, int(rng.integers(0, 8)))]
        prompt = (stem if i % 3 == 0 else []) + own
        steps = len(prompt) + 1 + int(rng.integers(4, 16))
        temp, topp = SETTINGS[i % 4]
        reqs.append((prompt, steps, temp, topp, int(rng.integers(1, 1 << 50)), i % 2 == 0, {17: 3.0, 305: 1.5} if i % 8 in (2, 3) else None,
                     CONTROL_SETS[i % len(CONTROL_SETS)]))
    ctx = TC.new_ctx(hdr, 7, 8)
    ctx.set_option(runtime.OPT_CHECK_POS, 0)
    sch = serve.Scheduler(ctx, max_rows=24, prefix_cache=prefix_cache)
    rids = [sch.submit_sampling(p, steps, temperature=t, topp=tp, seed=sd, allowed=TC.grammar_for(len(p)) if con else None, logit_bias=bias, **cs)
            for p, steps, t, tp, sd, con, bias, cs in reqs]
    res = sch.run()
    ctx.close()
    solo = TC.new_ctx(hdr, 7, 1)
    solo.set_option(runtime.OPT_CHECK_POS, 0)
    for rid, (p, steps, t, tp, sd, con, bias, cs) in zip(rids, reqs):
        got = res[rid]
        fed, finish, st = alone(solo, p, steps, t, tp, sd, TC.grammar_for(len(p)) if con else None, bias, cs)
        assert (got.tokens_fed, got.finish, got.rng_state) == (fed, finish, st), rid
        if con:
            picks = got.tokens_fed[1 + len(p):] + ([BOS] if got.finish == "bos" else [])
            for k, tok in enumerate(picks):
                assert tok in (TC.SET_A, TC.SET_B)[k % 2] or (tok == BOS and k >= 6), (rid, k, tok)
    solo.close()
    if prefix_cache:
        assert sch.rows_reused > 0
