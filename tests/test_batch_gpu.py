"""Batched greedy decode of independent sequences over one copy of the weights (include/llama2_hip.h: l2_seq_reserve ..
l2_read_seq_cache; csrc/batch.hip.h, batch_host.hip.h).  Every row of every batch follows a trajectory with a known answer -- the
REAL reference's greedy run on the synthetic checkpoint (tests/golden/<model>.json) or the C oracle run per sequence -- and is held
to the project's bars: tokens exact, logits within 1e-4 of the reference where it kept them and within 1e-5 of the same sequence run
through l2_forward, caches within 1e-6."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import argmax_cases as A
import oracle_lib as O
from llama2_ts_amd import runtime

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-4
E_ARG, E_CONFIG, E_STATE = -1, -2, -4


def load_gold(name):
    meta = json.load(open(os.path.join(GOLD, name + ".json")))
    return meta, np.load(os.path.join(GOLD, name + ".npz"))


def new_ctx(meta, n_seqs):
    ctx = runtime.Context(meta["header"])
    ctx.synth_fill(meta["seed"])
    ctx.seq_reserve(n_seqs)
    return ctx


def code_of(fn, *args):
    with pytest.raises(runtime.L2Error) as e:
        fn(*args)
    return e.value.code


def start_rows(ctx, meta, offsets):
    """Sequence s holds the golden's first offsets[s] fed tokens (l2_seq_prefill); returns the first tokens to feed."""
    fed = meta["tokens_fed"]
    for s, off in enumerate(offsets):
        if off:
            ctx.seq_prefill(s, fed[:off], 0)
    return [fed[off] for off in offsets]


@pytest.mark.parametrize("name", ["tiny", "stories15M", "stories110M"])
def test_staggered_forward_batch_follows_the_reference(name):
    """8 sequences, sequence s joins at call 3 s from BOS at position 0: every call mixes rows at different positions, in a different
    row order each call.  Every row's logits are the reference's where it kept them and those of the same sequence run through
    l2_forward; its argmax is the reference's next token."""
    meta, g = load_gold(name)
    fed, picks = meta["tokens_fed"], meta["argmax"]
    keep = {p: i for i, p in enumerate(meta["logit_positions"])}
    n_seq, calls = 8, 3 * 7 + 12
    solo = runtime.Context(meta["header"]); solo.synth_fill(meta["seed"])
    want = [np.array(solo.forward(fed[p], p), copy=True) for p in range(calls)]
    solo.close()
    ctx = new_ctx(meta, n_seq)
    rng = np.random.default_rng(7)
    for call in range(calls):
        seqs = [s for s in range(n_seq) if call >= 3 * s]
        rng.shuffle(seqs)
        pos = [call - 3 * s for s in seqs]
        lg = ctx.forward_batch(seqs, [fed[p] for p in pos], pos)
        assert lg.shape == (len(seqs), ctx.cfg.vocab_size)
        for i, (s, p) in enumerate(zip(seqs, pos)):
            assert runtime.argmax(lg[i]) == picks[p], (name, call, s, p)
            assert np.abs(lg[i] - want[p]).max() <= 1e-5, (name, call, s, p)
            if p in keep:
                assert np.abs(lg[i] - g["logits"][keep[p]]).max() <= TOL, (name, call, s, p)
    ctx.close()


def _greedy_110m(graph, offsets, steps):
    meta, _ = load_gold("stories110M")
    ctx = new_ctx(meta, len(offsets))
    ctx.set_option(runtime.OPT_USE_GRAPH, graph)
    first = start_rows(ctx, meta, offsets)
    seqs = list(range(len(offsets)))
    toks = ctx.decode_greedy_batch(seqs, first, offsets, steps)
    caches = [(ctx.read_seq_cache(s, "key_cache"), ctx.read_seq_cache(s, "value_cache")) for s in seqs]
    ctx.close()
    return meta, toks, caches


def test_decode_greedy_batch_stories110M_graph_and_eager():
    """8 sequences prefilled to different golden offsets (sequence 0 among them), then 256 device-resident greedy steps: every row's
    tokens are the reference's.  Replayed hipGraphs and eager launches give bit-identical tokens and caches."""
    offsets, steps = [0, 37, 128, 255, 300, 511, 640, 700], 256
    meta, toks, caches = _greedy_110m(1, offsets, steps)
    picks = meta["argmax"]
    for s, off in enumerate(offsets):
        assert toks[s].tolist() == picks[off:off + steps], (s, off)
    _, toks_e, caches_e = _greedy_110m(0, offsets, steps)
    assert np.array_equal(toks, toks_e)
    for (k, v), (ke, ve) in zip(caches, caches_e):
        assert k.tobytes() == ke.tobytes() and v.tobytes() == ve.tobytes()


def test_tinylong_batch_crosses_every_attention_level():
    """S = 1280: rows below, across and far beyond the decode path's split levels (144 / 256 cached rows), the last one ending at
    position 1279."""
    meta, _ = load_gold("tinylong")
    offsets = [0, 130, 250, 600, 1000, 1200]
    steps = 1280 - max(offsets)
    ctx = new_ctx(meta, len(offsets))
    first = start_rows(ctx, meta, offsets)
    toks = ctx.decode_greedy_batch(list(range(len(offsets))), first, offsets, steps)
    for s, off in enumerate(offsets):
        assert toks[s].tolist() == meta["argmax"][off:off + steps], (s, off)
    ctx.close()


def test_7b_width_sequences_to_the_end_of_the_context():
    """llama2_7b_L2 (d = 4096, h = 11008): four sequences prefilled to 100 / 1000 / 1900 / 2040, decoded to position 2047."""
    meta, _ = load_gold("llama2_7b_L2")
    offsets = [100, 1000, 1900, 2040]
    steps = 2048 - max(offsets)
    ctx = new_ctx(meta, len(offsets))
    first = start_rows(ctx, meta, offsets)
    toks = ctx.decode_greedy_batch([0, 1, 2, 3], first, offsets, steps)
    for s, off in enumerate(offsets):
        assert toks[s].tolist() == meta["argmax"][off:off + steps], (s, off)
    ctx.close()


def test_full_7b_eight_staggered_sequences():
    """Full 32-layer llama2_7b: 8 sequences at staggered golden offsets, 64 batch steps, against the 1024-step fixture."""
    meta, _ = load_gold("llama2_7b")
    offsets = [0, 17, 64, 130, 255, 400, 700, 900]
    steps = 64
    ctx = new_ctx(meta, len(offsets))
    mib = ctx.get_option(runtime.OPT_WEIGHT_MIB)
    first = start_rows(ctx, meta, offsets)
    toks = ctx.decode_greedy_batch(list(range(8)), first, offsets, steps)
    for s, off in enumerate(offsets):
        assert toks[s].tolist() == meta["argmax"][off:off + steps], (s, off)
    assert ctx.get_option(runtime.OPT_WEIGHT_MIB) <= mib, "batching must not add a copy of the weights"
    ctx.close()


@pytest.mark.parametrize("hdr", [(256, 512, 2, 4, 4, 1007, 64), (128, 384, 2, 2, 2, -600, 96)])
def test_random_first_tokens_match_the_oracle(hdr):
    """6 sequences with different first tokens, 40 steps, on a shape whose vocab is not a multiple of 16 and on an unshared classifier:
    per-step logits (l2_forward_batch) within 1e-4 of the C oracle run per sequence, picks and the device loop's tokens exact."""
    seed, n, steps = 3, 6, 40
    V = abs(hdr[5])
    firsts = [int(t) for t in np.random.default_rng(11).choice(V, n, replace=False)]
    orc = O.Oracle(hdr, seed)
    want_logits, want_toks = [], []
    for t0 in firsts:
        tok, ls, ts = t0, [], []
        for p in range(steps):
            lg = np.array(orc.forward(tok, p), copy=True)
            ls.append(lg)
            tok = O.argmax(lg)
            ts.append(tok)
        want_logits.append(ls); want_toks.append(ts)
    orc.close()
    ctx = runtime.Context(hdr); ctx.synth_fill(seed); ctx.seq_reserve(2 * n)
    toks = list(firsts)
    for p in range(steps):
        lg = ctx.forward_batch(list(range(n)), toks, [p] * n)
        for i in range(n):
            assert np.abs(lg[i] - want_logits[i][p]).max() <= TOL, (hdr, i, p)
            toks[i] = runtime.argmax(lg[i])
            assert toks[i] == want_toks[i][p], (hdr, i, p)
    got = ctx.decode_greedy_batch(list(range(n, 2 * n))[::-1], firsts[::-1], [0] * n, steps)[::-1]
    assert got.tolist() == want_toks
    ctx.close()


def test_isolation_of_sequences_and_of_the_context_state():
    """After a batch run every sequence's cache is what a fresh context that ran that sequence alone holds; reserved sequences that
    were in no call keep their caches byte for byte; and a sequence-0 decode through l2_forward interrupted by a batch run of the
    other sequences continues exactly as without it."""
    meta, g = load_gold("stories15M")
    fed, picks = meta["tokens_fed"], meta["argmax"]
    S, d, L = meta["header"][6], meta["header"][0], meta["header"][2]
    ctx = new_ctx(meta, 10)
    for p in range(100):                                  # sequence 0 through the single-sequence path
        ctx.forward(fed[p], p)
    idle = {s: (ctx.read_seq_cache(s, "key_cache").tobytes(), ctx.read_seq_cache(s, "value_cache").tobytes()) for s in (8, 9)}
    firsts, steps = [5, 77, 901, 1234, 3, 31999, 42], 20
    out = ctx.decode_greedy_batch(list(range(1, 8)), firsts, [0] * 7, steps)
    lg = np.array(ctx.forward(fed[100], 100), copy=True)
    assert runtime.argmax(lg) == picks[100]
    ctl = runtime.Context(meta["header"]); ctl.synth_fill(meta["seed"])
    for p in range(101):
        want = np.array(ctl.forward(fed[p], p), copy=True)
    assert lg.tobytes() == want.tobytes(), "a batch run changed what sequence 0's next l2_forward returns"
    for s in (8, 9):
        assert (ctx.read_seq_cache(s, "key_cache").tobytes(), ctx.read_seq_cache(s, "value_cache").tobytes()) == idle[s], s
    for i, s in enumerate(range(1, 8)):
        seq = [firsts[i]] + out[i, :-1].tolist()
        for p, t in enumerate(seq):
            ctl.forward(t, p)
        for name in ("key_cache", "value_cache"):
            a = ctx.read_seq_cache(s, name).reshape(L, S, d)[:, :steps]
            b = ctl.read_state(name).reshape(L, S, d)[:, :steps]
            assert np.abs(a - b).max() <= 1e-6, (s, name)
    ctl.close(); ctx.close()


def _upload(ctx, tensors):
    for kind, layers, count in runtime.tensor_shapes(ctx.cfg):
        per = tensors[kind].reshape(max(layers, 1), -1)
        for layer in range(max(layers, 1)):
            ctx.upload(kind, layer if layers else -1, per[layer])


@pytest.mark.parametrize("case", A.CASES)
def test_argmax_edges_through_the_batch_loop(case):
    """The argmax edge models (tests/argmax_cases.py: exact ties across tiles, +-0, +-inf, NaN, all NaN, NaN at index 0) at the `vec`
    shape, as 4 sequences at different start positions: the batch loop picks what the REAL reference picked."""
    meta = json.load(open(os.path.join(GOLD, "argmax_%s_vec.json" % case)))
    fed, picks = meta["tokens_fed"], meta["picks"]
    ctx = runtime.Context(A.SHAPES["vec"])
    _upload(ctx, A.tensors_of(case, "vec"))
    ctx.seq_reserve(4)
    starts = [0, 2, 5, 7]
    steps = len(picks) - max(starts)
    for s, p in enumerate(starts):
        if p:
            ctx.seq_prefill(s, fed[:p], 0)
    got = ctx.decode_greedy_batch([3, 1, 0, 2], [fed[starts[s]] for s in (3, 1, 0, 2)], [starts[s] for s in (3, 1, 0, 2)], steps)
    for i, s in enumerate((3, 1, 0, 2)):
        assert got[i].tolist() == picks[starts[s]:starts[s] + steps], (case, s)
    ctx.close()


def test_shapes_the_batch_path_does_not_cover_are_refused():
    """The `odd` argmax shape (dims not multiples of 16), a grouped-query context and a loopback tensor-parallel rank: L2_E_CONFIG
    with the reason, and the contexts stay usable."""
    odd = runtime.Context(A.SHAPES["odd"]); odd.synth_fill(1)
    assert code_of(odd.seq_reserve, 4) == E_CONFIG
    assert b"multiple of 16" in runtime.lib().l2_last_error()
    assert odd.get_option(runtime.OPT_SEQS) == 0
    odd.forward(1, 0)
    odd.close()
    gqa = runtime.Context((64, 176, 2, 4, 2, 512, 64), flags=runtime.F_GQA)
    assert code_of(gqa.seq_reserve, 2) == E_CONFIG
    assert b"grouped-query" in runtime.lib().l2_last_error()
    gqa.close()
    hdr, G = (64, 176, 2, 4, 4, 512, 64), 2
    gid = bytes([G, 99] + [5] * 126)
    codes, errs = [None] * G, [None] * G

    def rank_main(r):
        try:
            c = runtime.Context(hdr, tp_rank=r, tp_size=G, nccl_id=gid)
            try:
                c.seq_reserve(2)
            except runtime.L2Error as e:
                codes[r] = (e.code, runtime.lib().l2_last_error())
            c.close()
        except BaseException as e:
            errs[r] = e

    os.environ["L2_TP_LOOPBACK"] = "1"
    try:
        ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(G)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        assert not any(t.is_alive() for t in ts), "a rank hung"
    finally:
        del os.environ["L2_TP_LOOPBACK"]
    for e in errs:
        if e is not None:
            raise e
    for code, text in codes:
        assert code == E_CONFIG and b"tensor-parallel" in text


def test_bad_arguments_return_their_codes_and_the_context_still_decodes():
    meta, _ = load_gold("tiny")
    fed, picks = meta["tokens_fed"], meta["argmax"]
    V, S = meta["header"][5], meta["header"][6]
    ctx = runtime.Context(meta["header"]); ctx.synth_fill(meta["seed"])
    assert code_of(ctx.forward_batch, [0], [1], [0]) == E_STATE                       # before the reserve
    assert code_of(ctx.decode_greedy_batch, [0], [1], [0], 4) == E_STATE
    assert code_of(ctx.seq_prefill, 0, [1, 2], 0) == E_STATE
    assert code_of(ctx.read_seq_cache, 0, "key_cache") == E_STATE
    assert code_of(ctx.seq_reserve, 0) == E_ARG and code_of(ctx.seq_reserve, 65) == E_ARG
    assert ctx.get_option(runtime.OPT_SEQS) == 0
    ctx.seq_reserve(4)
    assert ctx.get_option(runtime.OPT_SEQS) == 4
    assert code_of(ctx.seq_reserve, 4) == E_STATE                                      # once per context
    assert code_of(ctx.set_option, runtime.OPT_SEQS, 2) == E_ARG
    bad = [([4], [1], [0]), ([-1], [1], [0]), ([0], [V], [0]), ([0], [-1], [0]), ([0], [1], [S]), ([0], [1], [-1]),
           ([1, 1], [1, 2], [0, 0]), ([0, 1, 2, 3, 0], [1] * 5, [0] * 5)]
    for seqs, toks, pos in bad:
        assert code_of(ctx.forward_batch, seqs, toks, pos) == E_ARG, (seqs, toks, pos)
        assert code_of(ctx.decode_greedy_batch, seqs, toks, pos, 2) == E_ARG, (seqs, toks, pos)
    assert code_of(ctx.decode_greedy_batch, [0, 1], [1, 1], [0, S - 3], 4) == E_ARG       # pos + steps > S
    assert code_of(ctx.seq_prefill, 4, [1], 0) == E_ARG and code_of(ctx.seq_prefill, 1, [V], 0) == E_ARG
    assert code_of(ctx.seq_prefill, 1, [1] * 3, S - 2) == E_ARG
    assert code_of(ctx.read_seq_cache, 4, "key_cache") == E_ARG and code_of(ctx.read_seq_cache, 0, "q") == E_ARG
    L = runtime.lib()
    three = (C.c_int32 * 1)(0)
    assert L.l2_forward_batch(ctx._h, 1, None, three, three, None) == E_ARG
    assert L.l2_forward_batch(ctx._h, 1, three, None, three, None) == E_ARG
    assert L.l2_forward_batch(ctx._h, 1, three, three, None, None) == E_ARG
    assert L.l2_decode_greedy_batch(ctx._h, 1, three, three, three, 2, None) == E_ARG
    assert L.l2_seq_prefill(ctx._h, 1, None, 1, 0, None) == E_ARG
    assert L.l2_read_seq_cache(ctx._h, 1, runtime.S_KEY_CACHE, -1, None, 4) == E_ARG
    assert L.l2_forward_batch(ctx._h, 0, three, three, three, None) == E_ARG
    assert L.l2_decode_greedy_batch(ctx._h, 1, three, three, three, -1, (C.c_int32 * 4)()) == E_ARG      # negative steps
    ctx.set_option(runtime.OPT_CHECK_POS, 1)                                               # the position rule, per sequence
    assert code_of(ctx.forward_batch, [2], [1], [5]) == E_STATE
    ctx.set_option(runtime.OPT_CHECK_POS, 0)
    toks = ctx.decode_greedy_batch([2, 0], [fed[0], fed[0]], [0, 0], 20)
    assert toks[0].tolist() == picks[:20] and toks[1].tolist() == picks[:20]
    ctx.close()


def test_exact_attention_option_is_honoured():
    """L2_OPT_EXACT_ATTENTION switches the batch attention to the reference's t-sequential fp32 accumulate, as on the decode kernel:
    the batch loop still follows the reference, and its caches match the single-sequence path's under the same option."""
    meta, _ = load_gold("stories15M")
    ctx = new_ctx(meta, 3)
    ctx.set_option(runtime.OPT_EXACT_ATTENTION, 1)
    offsets = [0, 40, 90]
    first = start_rows(ctx, meta, offsets)
    toks = ctx.decode_greedy_batch([0, 1, 2], first, offsets, 60)
    for s, off in enumerate(offsets):
        assert toks[s].tolist() == meta["argmax"][off:off + 60], (s, off)
    ctx.close()
