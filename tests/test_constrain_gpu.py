"""Constrained decoding on the device (include/llama2_hip.h: l2_step_batch_constrained; csrc/constrain.hip.h).  One mixed call per
shape carries every row kind (no mask, a shared mask, singletons with and without id 0, a third of the vocabulary, the full mask,
bias lists on an unmasked and on a masked row) under every sampler setting, decode rows and prompt runs interleaved so that the
packing order is not the call order.  Its logits are held element by element to the plain step's on a twin context, its picks and
rng states to the oracle's sampler fed the constrained rows (with the stated fall-through rule), its log-probabilities to a host fp64
log-softmax of those rows; then the refusals, and the scheduler with a grammar callable against each request run alone."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from llama2_ts_amd import runtime, serve

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -4
BOS = 1
SHAPES = {
    "V97": (16, 48, 2, 4, 4, 97, 40),            # V odd: scalar stores, a last mask word with one live bit
    "tiny": (64, 176, 2, 4, 4, 512, 64),         # V % 4 == 0: 16-byte stores, whole mask words
    "V2083": (64, 176, 1, 4, 4, -2083, 32),      # 66 mask words, V crosses a 1024-element sampler tile
    "V32000": (64, 176, 1, 4, 4, 32000, 32),     # the real vocabulary width, W = 1000
}
SETTINGS = [(0.0, 1.0), (0.9, 1.0), (0.9, 0.9), (1.5, 0.5)]      # greedy, `sample`, `sample_topp` twice
KINDS = ["none", "shared", "shared", "single", "zero", "third", "full", "bias", "mask_bias"]
PRE = 6                                          # rows a decode row's sequence holds before the call


def new_ctx(hdr, seed, n_seqs):
    ctx = runtime.Context(hdr)
    ctx.synth_fill(seed)
    ctx.seq_reserve(n_seqs)
    ctx.set_option(runtime.OPT_CHECK_POS, 1)
    return ctx


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max()
    return x - (m + np.log(np.exp(x - m).sum()))


def top_order(x, k):
    """The k largest logits' ids: descending value, equal values (the -inf ones) by ascending id."""
    return np.lexsort((np.arange(x.size), -np.asarray(x, dtype=np.float64)))[:k]


def close_lps(got, want, tol):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    ninf = np.isneginf(want)
    return bool(np.array_equal(np.isneginf(got), ninf) and np.abs(got[~ninf] - want[~ninf]).max(initial=0.0) <= tol)


def rows_of(V):
    """The call's rows: every kind under every setting; row i is a prompt run when i % 3 == 1, else a decode row."""
    rng = np.random.default_rng(V)
    third = sorted(int(t) for t in rng.choice(np.arange(1, V), V // 3, replace=False))
    sets = {"none": None, "shared": [0, 5, V - 1], "single": [V - 1], "zero": [0], "third": third, "full": list(range(V)),
            "bias": None, "mask_bias": third}
    rows = []
    for kind in KINDS:
        for temp, topp in SETTINGS:
            i = len(rows)
            bias = None
            if kind == "bias":
                bias = {3: 2.5, V - 1: -4.0, 0: 0.75, 40: 11.0}
            if kind == "mask_bias":
                bias = {0: 5.0, third[0]: 3.0, third[-1]: -2.0, third[len(third) // 2]: 9.5}      # id 0 is not allowed
            n_tok = 2 + 3 * (i % 5) if i % 3 == 1 else 1
            rows.append(dict(kind=kind, allowed=sets[kind], bias=bias, temp=temp, topp=topp, n_tok=n_tok, seed=1000 + 17 * i))
    return rows


_RUNS = {}


def run_shape(name):
    """The constrained call on one context and the plain logprobs call on its twin, for top_k 0 and 5 (fresh rng seeds each); computed
    once per shape and read by every test of it."""
    if name in _RUNS:
        return _RUNS[name]
    hdr = SHAPES[name]
    V = abs(hdr[5])
    rows = rows_of(V)
    n = len(rows)
    rng = np.random.default_rng(5)
    seqs = [int(s) for s in rng.permutation(n)]
    a, b = new_ctx(hdr, 21, n), new_ctx(hdr, 21, n)
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
        pa, ra, la, lpa = a.step_batch(seqs, runs, pos0, temp, topp, seeds, logits=True, logprobs=k, allowed=allowed, logit_bias=bias)
        pb, rb, lb, lpb = b.step_batch(seqs, runs, pos0, temp, topp, seeds, logits=True, logprobs=k)
        out["calls"].append(dict(k=k, seeds=seeds, a=(pa, ra, la, lpa), b=(pb, rb, lb, lpb)))
    out["caches_equal"] = all(np.array_equal(a.read_seq_cache(s, nm), b.read_seq_cache(s, nm)) for s in seqs for nm in ("key_cache", "value_cache"))
    # next positions: one past each run's end is a skip-ahead on both, the end itself continues on both with the same picks
    ends = [p + r["n_tok"] for p, r in zip(pos0, rows)]
    nxt = [[int(t)] for t in rng.integers(0, V, n)]
    out["skip"] = [_code(c, [seqs[1]], [nxt[1]], [ends[1] + 1]) for c in (a, b)]
    out["follow"] = [c.step_batch(seqs, nxt, ends)[0] for c in (a, b)]
    # no constraint at all through the constrained entry point: the plain step's outputs
    seeds = [r["seed"] + 9 for r in rows]
    ends1 = [e + 1 for e in ends]
    out["null_a"] = a.step_batch(seqs, nxt, ends1, temp, topp, seeds, logits=True, logprobs=3, allowed=[None] * n, logit_bias=[None] * n)
    out["null_b"] = b.step_batch(seqs, nxt, ends1, temp, topp, seeds, logits=True, logprobs=3)
    a.close()
    b.close()
    _RUNS[name] = out
    return out


def _code(ctx, *args, **kw):
    try:
        ctx.step_batch(*args, **kw)
    except runtime.L2Error as e:
        return e.code
    return 0


def expected_row(x, row):
    """x' of the issue: -inf where the mask forbids, one fp32 add at biased allowed ids, x elsewhere."""
    want = np.array(x, dtype=np.float32, copy=True)
    ok = np.ones(want.size, dtype=bool)
    if row["allowed"] is not None:
        ok[:] = False
        ok[row["allowed"]] = True
    for j, v in (row["bias"] or {}).items():
        if ok[j]:
            want[j] = np.float32(x[j]) + np.float32(v)
    want[~ok] = -np.inf
    return want, ok


@pytest.mark.parametrize("name", list(SHAPES))
def test_logits_are_the_plain_rows_rewritten(name):
    run = run_shape(name)
    rows = run["rows"]
    assert any(r["n_tok"] > 1 for r in rows[:4]) and rows[0]["n_tok"] == 1      # a prompt run in front of decode rows: ord[] reorders
    for call in run["calls"]:
        (pa, ra, la, lpa), (pb, rb, lb, lpb) = call["a"], call["b"]
        for i, row in enumerate(rows):
            want, ok = expected_row(lb[i], row)
            assert np.array_equal(la[i].view(np.uint32), want.view(np.uint32)), (name, i, row["kind"])
            assert np.isneginf(la[i][~ok]).all() and np.isfinite(la[i][ok]).all()
            if row["kind"] in ("none", "full"):      # every output is the plain call's
                assert pa[i] == pb[i] and ra[i] == rb[i], (name, i)
                assert all(np.array_equal(x[i], y[i]) for x, y in zip(lpa, lpb)), (name, i)
        biased = [i for i, r in enumerate(rows) if r["bias"]]
        assert any(not np.array_equal(la[i], lb[i]) for i in biased)
    assert run["caches_equal"]
    assert run["skip"] == [E_STATE, E_STATE] and run["follow"][0] == run["follow"][1]
    na, nb = run["null_a"], run["null_b"]
    assert na[0] == nb[0] and na[1] == nb[1] and np.array_equal(na[2], nb[2]) and all(np.array_equal(x, y) for x, y in zip(na[3], nb[3]))


@pytest.mark.parametrize("name", list(SHAPES))
def test_picks_are_the_oracle_sampler_on_the_constrained_rows(name):
    run = run_shape(name)
    rows = run["rows"]
    fell, kept = 0, 0
    for call in run["calls"]:
        pa, ra, la, _ = call["a"]
        for i, row in enumerate(rows):
            st = O.Rng(call["seeds"][i])
            if row["temp"] == 0.0:
                want = O.argmax(la[i])
                assert ra[i] == call["seeds"][i]
            else:
                want = O.next_token(la[i], row["temp"], row["topp"], st)[0]
                assert ra[i] == int(st.state.value), (name, i)      # the draw was made, whatever became of the pick
                if row["allowed"] is not None:
                    if want not in row["allowed"]:
                        assert want == 0, (name, i, want)           # only the reference's `return 0` steps outside
                        want = O.argmax(la[i])
                        fell += 1
                        assert row["kind"] != "single" or 0.0 < row["topp"] < 1.0
                    else:
                        kept += 1
                        assert not (row["kind"] == "single" and 0.0 < row["topp"] < 1.0), (name, i)
            assert pa[i] == want, (name, i, row["kind"], row["temp"], row["topp"])
            if row["allowed"] is not None:
                assert pa[i] in row["allowed"], (name, i)
            if row["kind"] in ("single", "zero"):
                assert pa[i] == row["allowed"][0]
    # the singleton without id 0 falls through under top-p every time (2 settings x 2 calls), never under plain `sample`
    assert fell >= 4 and kept >= 4, (fell, kept)


@pytest.mark.parametrize("name", list(SHAPES))
def test_logprobs_are_those_of_the_constrained_rows(name):
    run = run_shape(name)
    rows = run["rows"]
    for call in run["calls"]:
        k = call["k"]
        pa, _, la, (plp, ids, tlp) = call["a"]
        assert ids.shape == (len(rows), k)
        for i, row in enumerate(rows):
            want = log_softmax(la[i])
            assert close_lps(plp[i], want[pa[i]], 1e-10) and np.isfinite(plp[i]), (name, i)
            if k:
                assert ids[i].tolist() == top_order(la[i], k).tolist(), (name, i, row["kind"])
                assert close_lps(tlp[i], want[ids[i]], 1e-10), (name, i)
                if row["allowed"] is not None:
                    m = min(k, len(row["allowed"]))      # the allowed ids first; the rest -inf, by ascending id
                    assert set(ids[i, :m].tolist()) <= set(row["allowed"]) and np.isfinite(tlp[i, :m]).all()
                    assert np.isneginf(tlp[i, m:]).all(), (name, i)
            if row["kind"] in ("single", "zero"):      # one allowed token: probability 1
                assert abs(plp[i]) <= 1e-10
    # pick lps do not depend on top_k
    same = [i for i, r in enumerate(rows) if r["temp"] == 0.0]
    assert np.array_equal(run["calls"][0]["a"][3][0][same], run["calls"][1]["a"][3][0][same])


def test_refusals_leave_the_context_alone():
    hdr = SHAPES["V97"]
    V, W = 97, 4
    ctx = new_ctx(hdr, 3, 3)
    ctx.seq_prefill_batch([0, 1, 2], [[5, 6, 7]] * 3, 0)
    before = [ctx.read_seq_cache(s, nm) for s in range(3) for nm in ("key_cache", "value_cache")]
    L = runtime.lib()
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    f64 = lambda *v: (C.c_double * len(v))(*v)
    seqs, one, tok, p0 = i32(0, 1, 2), i32(1, 1, 1), i32(8, 9, 10), i32(3, 3, 3)
    temp, topp = f64(0.9, 0.0, 0.9), f64(0.9, 1.0, 1.0)
    full = runtime.pack_mask(range(V), V).tolist()
    high = [0, 0, 0, 0xfffffffe]                                  # only bits at or above V: allows no token
    picks = i32(-9, -9, -9)

    def call(t=temp, mask_of=None, masks=(), bc=None, bi=None, bv=None):
        st = (C.c_uint64 * 3)(11, 22, 33)
        m = (C.c_uint32 * max(1, len(masks)))(*masks)
        rc = L.l2_step_batch_constrained(ctx._h, 3, seqs, one, tok, p0, t, topp, st, picks, None, 0, None, None, None,
                                         mask_of, len(masks) // W, m if mask_of is not None else None, bc, bi, bv)
        assert rc != 0 or list(picks) != [-9, -9, -9]
        if rc:
            assert list(st) == [11, 22, 33] and list(picks) == [-9, -9, -9]
        return rc

    assert call(mask_of=i32(0, -1, 1), masks=full + high) == E_ARG                 # an empty mask that a row names
    assert call(mask_of=i32(0, -1, -1), masks=full + [0] * W) == 0                 # one that no row names is accepted
    picks[:] = [-9, -9, -9]
    assert call(bc=i32(0, 2, 0), bi=i32(4, V), bv=(C.c_float * 2)(1.0, 1.0)) == E_ARG          # a bias id equal to V
    assert call(bc=i32(1, 2, 0), bi=i32(3, 4, 4), bv=(C.c_float * 3)(1.0, 1.0, 2.0)) == E_ARG  # a repeated bias id
    assert call(bc=i32(1, 1, 0), bi=i32(4, 4), bv=(C.c_float * 2)(1.0, 1.0)) == 0              # the same id in two rows is fine
    picks[:] = [-9, -9, -9]
    assert call(t=f64(-0.9, 0.0, 0.9), mask_of=i32(0, -1, -1), masks=full) == E_ARG            # a masked row, temperature < 0
    assert call(t=f64(-0.9, 0.0, 0.9), mask_of=i32(-1, 0, 0), masks=full) == 0                 # an unmasked one may have it
    picks[:] = [-9, -9, -9]
    ctx.set_option(runtime.OPT_CHECK_POS, 0)
    assert call(mask_of=i32(0, 1, 2), masks=full * 3) == 0
    after = [ctx.read_seq_cache(s, nm) for s in range(3) for nm in ("key_cache", "value_cache")]
    S, d, Ly = hdr[6], hdr[0], hdr[2]
    for x, y in zip(before, after):      # the refused calls wrote nothing; the accepted ones rewrote row 3 alone
        x, y = x.reshape(Ly, S, d), y.reshape(Ly, S, d)
        assert np.array_equal(x[:, :3], y[:, :3]) and np.array_equal(x[:, 4:], y[:, 4:])
    ctx.close()


# ---- the scheduler on the device -------------------------------------------------------------------------------------------------
SET_A, SET_B = list(range(10, 40)), list(range(300, 330))


def grammar_for(n_prompt):
    """Alternate between two disjoint id sets; BOS may end the request from the seventh pick on."""
    def grammar(fed):
        k = len(fed) - 1 - n_prompt
        return (SET_A, SET_B)[k % 2] + ([BOS] if k >= 6 else [])
    return grammar


def alone(ctx, prompt, steps, temp, topp, seed, grammar, bias):
    """The request through a plain loop of constrained steps on sequence 0: the known tokens as one run, then a pick per position."""
    known = ([BOS] + prompt)[:steps]
    fed, rng, token, run, finish = [], seed, None, known, "steps"
    while True:
        pos = len(fed)
        fed += run
        real = len(fed) > len(prompt)
        if real:
            kw = dict(allowed=[grammar(fed)]) if grammar else {}
            if bias:
                kw["logit_bias"] = [bias]
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
def test_scheduler_with_a_grammar_callable(prefix_cache):
    hdr = SHAPES["tiny"]
    V = hdr[5]
    rng = np.random.default_rng(31)
    stem = [int(t) for t in rng.integers(2, V, 9)]
    reqs = []
    for i in range(24):
        own = [int(t) for t in rng.integers(2, V, int(rng.integers(0, 8)))]
        prompt = (stem if i % 3 == 0 else []) + own
        steps = len(prompt) + 1 + int(rng.integers(4, 16))
        temp, topp = SETTINGS[i % 4]
        reqs.append((prompt, steps, temp, topp, int(rng.integers(1, 1 << 50)), i % 2 == 0, {17: 3.0, 305: 1.5} if i % 8 in (2, 3) else None))
    ctx = new_ctx(hdr, 7, 8)
    ctx.set_option(runtime.OPT_CHECK_POS, 0)
    sch = serve.Scheduler(ctx, max_rows=24, prefix_cache=prefix_cache)
    rids = [sch.submit_constrained(p, steps, temperature=t, topp=tp, seed=sd, allowed=grammar_for(len(p)) if con else None, logit_bias=bias)
            for p, steps, t, tp, sd, con, bias in reqs]
    res = sch.run()
    ctx.close()
    solo = new_ctx(hdr, 7, 1)
    solo.set_option(runtime.OPT_CHECK_POS, 0)
    for rid, (p, steps, t, tp, sd, con, bias) in zip(rids, reqs):
        got = res[rid]
        fed, finish, st = alone(solo, p, steps, t, tp, sd, grammar_for(len(p)) if con else None, bias)
        assert (got.tokens_fed, got.finish, got.rng_state) == (fed, finish, st), rid
        if con:
            picks = got.tokens_fed[1 + len(p):] + ([BOS] if got.finish == "bos" else [])
            for k, tok in enumerate(picks):
                assert tok in (SET_A, SET_B)[k % 2] or (tok == BOS and k >= 6), (rid, k, tok)
            assert len(picks) >= 4
    solo.close()
    if prefix_cache:
        assert sch.rows_reused > 0
