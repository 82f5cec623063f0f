"""Per-sequence temperature / top-p sampling in the batched decode loop (include/llama2_hip.h: l2_decode_sample_batch; csrc/sampler.hip
row forms, batch.hip.h bt_pick_kernel).  Every row is held to the exactness contract: its tokens and final rng state are what the
reference's sampler (the C oracle's orc_next_token, llama2.ts:476-493) returns when it is fed the batch path's own logits -- those of
l2_forward_batch for the same rows in the same order on a second context -- and, where the REAL reference was run with -t / -p / -s
(tests/golden/cli_temp.json, cli_topp.json), the reference's own tokens."""
import json
import os

import numpy as np
import pytest

import argmax_cases as A
import oracle_lib as O
from llama2_ts_amd import runtime

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
E_ARG, E_CONFIG, E_STATE = -1, -2, -4


def load_meta(name):
    return json.load(open(os.path.join(GOLD, name + ".json")))


def sampled_run(name):
    meta = load_meta(name)
    argv = dict(zip(meta["argv"][::2], meta["argv"][1::2]))
    return meta, float(argv.get("-t", 1.0)), float(argv.get("-p", 1.0)), int(argv["-s"])


def code_of(fn, *args):
    with pytest.raises(runtime.L2Error) as e:
        fn(*args)
    return e.value.code


def new_ctx(hdr, seed, n_seqs):
    ctx = runtime.Context(hdr)
    ctx.synth_fill(seed)
    ctx.seq_reserve(n_seqs)
    return ctx


def oracle_replay(ref, seqs, firsts, pos0, steps, temps, topps, seeds):
    """Step the rows through l2_forward_batch on `ref` (same rows, same order) and pick with the oracle's sampler."""
    n = len(seqs)
    rngs = [O.Rng(s) for s in seeds]
    toks, pos = list(firsts), list(pos0)
    out = np.zeros((n, steps), dtype=np.int32)
    for k in range(steps):
        lg = ref.forward_batch(seqs, toks, pos)
        for i in range(n):
            toks[i], _ = O.next_token(lg[i], temps[i], topps[i], rngs[i])
            out[i, k] = toks[i]
            pos[i] += 1
    return out, [r.state.value for r in rngs]


def check_against_oracle(hdr, seed, seqs, firsts, pos0, steps, temps, topps, seeds, prefill=None, n_seqs=None):
    """decode_sample_batch on one context, the oracle fed the batch logits on a second one with the same weights and prefill."""
    n_seqs = n_seqs or (max(seqs) + 1)
    ctxs = []
    for _ in range(2):
        c = new_ctx(hdr, seed, n_seqs)
        if prefill:
            prefill(c)
        ctxs.append(c)
    ctx, ref = ctxs
    got, rng_after = ctx.decode_sample_batch(seqs, firsts, pos0, steps, temps, topps, seeds)
    want, rng_want = oracle_replay(ref, seqs, firsts, pos0, steps, temps, topps, seeds)
    for i in range(len(seqs)):
        assert got[i].tolist() == want[i].tolist(), (hdr, i, temps[i], topps[i])
        assert rng_after[i] == rng_want[i], (hdr, i)
    sampled = sum(steps for t in temps if t != 0)
    counters = (ctx.get_option(runtime.OPT_BATCH_SAMPLED_TOKENS), ctx.get_option(runtime.OPT_BATCH_SAMPLED_SERIAL))
    ctx.close(); ref.close()
    return got, counters, sampled


def test_reference_sampled_runs_as_batch_rows():
    """stories15M, 8 sequences: three rows replay cli_temp (t 0.9, seed 42 from BOS), three replay cli_topp (prompt by seq_prefill, then
    t 1.0, p 0.9, seed 7), two greedy rows start at golden offsets.  19 steps on every row, then 20 more on the cli_temp rows; and the
    same in ragged chunks that carry the rng state.  Identical seeds in one batch: the rows' rng states are kept apart."""
    mt, t_t, p_t, s_t = sampled_run("cli_temp")
    mp, t_p, p_p, s_p = sampled_run("cli_topp")
    gold = load_meta("stories15M")
    ft, fp = mt["tokens_fed"], mp["tokens_fed"]
    offs = [10, 100]
    seqs = [5, 0, 7, 2, 6, 1, 3, 4]                       # rows 0-2 cli_temp, 3-5 cli_topp, 6-7 greedy
    kinds = ["t", "t", "t", "p", "p", "p", "g", "g"]
    temps = [t_t] * 3 + [t_p] * 3 + [0.0, 0.0]
    topps = [p_t] * 3 + [p_p] * 3 + [0.5, 0.0]
    for chunks in ([19], [1, 2, 5, 11]):
        ctx = new_ctx(mt["header"], mt["seed"], 8)
        for i, k in enumerate(kinds):
            if k == "p":
                ctx.seq_prefill(seqs[i], fp[:4], 0)
            elif k == "g":
                ctx.seq_prefill(seqs[i], gold["tokens_fed"][:offs[i - 6]], 0)
        firsts = [ft[0]] * 3 + [fp[4]] * 3 + [gold["tokens_fed"][o] for o in offs]
        pos = [0] * 3 + [4] * 3 + list(offs)
        rng = [s_t] * 3 + [s_p] * 3 + [123, 456]
        got = [[] for _ in seqs]
        for n in chunks:
            toks, rng = ctx.decode_sample_batch(seqs, firsts, pos, n, temps, topps, rng)
            for i in range(8):
                got[i] += toks[i].tolist()
            firsts = toks[:, -1].tolist()
            pos = [p + n for p in pos]
        assert rng[6:] == [123, 456], "greedy rows take no draw"
        for i in range(3):
            assert got[i] == ft[1:20], ("cli_temp", i, chunks)
        for i in range(3, 6):
            assert got[i] == fp[5:], ("cli_topp", i, chunks)
        for i in (6, 7):
            o = offs[i - 6]
            assert got[i] == gold["argmax"][o:o + 19], ("greedy", i)
        # the cli_temp rows continue alone for the rest of the fixture
        rest, _ = ctx.decode_sample_batch(seqs[:3], firsts[:3], pos[:3], len(ft) - 20, temps[:3], topps[:3], rng[:3])
        for i in range(3):
            assert got[i] + rest[i].tolist() == ft[1:], ("cli_temp continued", i, chunks)
        assert ctx.get_option(runtime.OPT_BATCH_SAMPLED_TOKENS) == 3 * 39 + 3 * 19
        ctx.close()


MIXED_T = [0.3, 1.7, 1.0, 0.8, 2.5, -0.8, 0.05, 1e6, 3e7, 0.0]
MIXED_P = [0.0, 0.05, 0.5, 0.9, 0.999, 1.0]


def test_mixed_settings_against_the_oracle_fed_the_batch_logits():
    """16 staggered rows on stories15M, 48 steps, every row with its own temperature (incl. negative, tiny, huge, 0), topp (0 .. 1) and
    seed (up to 2^63 + 11): tokens and final rng states exact; counter 12 counts the sampled tokens, counter 13 stays within the
    allowance of equal probabilities by the thousand (huge temperatures)."""
    meta = load_meta("stories15M")
    fed = meta["tokens_fed"]
    n, steps = 16, 48
    seqs = list(range(n))[::-1]
    pos0 = [3 * s for s in seqs]
    temps = [MIXED_T[i % len(MIXED_T)] for i in range(n)]
    topps = [MIXED_P[i % len(MIXED_P)] for i in range(n)]
    seeds = [2 ** 63 + 11 if i == 3 else 1000 + 7 * i for i in range(n)]

    def prefill(c):
        for s in seqs:
            if 3 * s:
                c.seq_prefill(s, fed[:3 * s], 0)
    got, (c12, c13), sampled = check_against_oracle(meta["header"], meta["seed"], seqs, [fed[p] for p in pos0], pos0, steps, temps, topps,
                                                    seeds, prefill)
    assert c12 == sampled
    huge = sum(steps for t in temps if abs(t) >= 1e6)
    assert c13 <= 1 + huge // 4, (c13, huge)


@pytest.mark.parametrize("V,n", [(1000, 64), (5121, 17), (50257, 33), (128256, 64), (128256, 1)])
def test_vocabularies_and_tile_forms(V, n):
    """Header (64, 176, 1, 4, 4, V, 16): vocabularies of 1 to 126 sampler tiles, row counts that reach the 1-, 2- and 4-tile GEMM forms;
    plain sampling, top-p and a negative temperature side by side, against the oracle fed the batch logits."""
    hdr = (64, 176, 1, 4, 4, V, 16)
    steps = 8
    seqs = list(range(n))
    firsts = [int(t) for t in np.random.default_rng(V + n).integers(0, V, n)]
    settings = [(0.9, 1.0), (1.0, 0.9), (-0.7, 0.0), (1.3, 0.3), (0.0, 0.9)]
    temps = [settings[i % 5][0] for i in range(n)]
    topps = [settings[i % 5][1] for i in range(n)]
    seeds = [77 + i for i in range(n)]
    check_against_oracle(hdr, 5, seqs, firsts, [0] * n, steps, temps, topps, seeds)


def _run_110m(graph):
    meta = load_meta("stories110M")
    fed = meta["tokens_fed"]
    offs = [0, 37, 128, 255, 300, 511, 640, 700]
    ctx = new_ctx(meta["header"], meta["seed"], 8)
    ctx.set_option(runtime.OPT_USE_GRAPH, graph)
    for s, o in enumerate(offs):
        if o:
            ctx.seq_prefill(s, fed[:o], 0)
    temps = [0.9, 1.0, 0.0, 1.2, 0.7, 2.0, 0.8, 1.0]
    topps = [1.0, 0.9, 0.0, 0.5, 0.95, 0.0, 0.7, 0.99]
    toks, rng = ctx.decode_sample_batch(list(range(8)), [fed[o] for o in offs], offs, 128, temps, topps, [3 + s for s in range(8)])
    caches = [(ctx.read_seq_cache(s, "key_cache").tobytes(), ctx.read_seq_cache(s, "value_cache").tobytes()) for s in range(8)]
    ctx.close()
    return toks, rng, caches


def test_graph_replay_and_eager_launches_are_bit_identical():
    """stories110M, 8 rows, 128 steps, mixed settings: the replayed recording and eager launches give the same tokens, rng states and
    caches bit for bit."""
    a, b = _run_110m(1), _run_110m(0)
    assert np.array_equal(a[0], b[0])
    assert a[1] == b[1]
    assert a[2] == b[2]


def _mixed_15m():
    meta = load_meta("stories15M")
    ctx = new_ctx(meta["header"], meta["seed"], 6)
    temps, topps = [0.9, 1.0, 0.6, 1.4, 0.0, 1.0], [1.0, 0.9, 0.3, 0.0, 0.0, 0.99]
    toks, rng = ctx.decode_sample_batch(list(range(6)), [1] * 6, [0] * 6, 40, temps, topps, [42, 7, 9, 11, 13, 15])
    c = (ctx.get_option(runtime.OPT_BATCH_SAMPLED_TOKENS), ctx.get_option(runtime.OPT_BATCH_SAMPLED_SERIAL))
    ctx.close()
    return toks, rng, c


def test_forced_serial_branch_gives_the_same_tokens(monkeypatch):
    """L2_SAMPLER_FORCE_SERIAL=1: every sampled token takes the reference's loop as written; tokens and rng equal the default run's."""
    base = _mixed_15m()
    monkeypatch.setenv("L2_TEST_HOOKS", "1")
    monkeypatch.setenv("L2_SAMPLER_FORCE_SERIAL", "1")
    forced = _mixed_15m()
    assert np.array_equal(base[0], forced[0])
    assert base[1] == forced[1]
    assert forced[2][0] == 5 * 40 and forced[2][1] == forced[2][0]


def test_greedy_rows_equal_the_greedy_batch():
    """All temperatures 0: the tokens of decode_greedy_batch, the rng states untouched."""
    meta = load_meta("stories15M")
    fed = meta["tokens_fed"]
    offs = [0, 5, 50, 200]
    out = []
    for sampled in (True, False):
        ctx = new_ctx(meta["header"], meta["seed"], 4)
        for s, o in enumerate(offs):
            if o:
                ctx.seq_prefill(s, fed[:o], 0)
        if sampled:
            toks, rng = ctx.decode_sample_batch([3, 1, 0, 2], [fed[offs[s]] for s in (3, 1, 0, 2)], [offs[s] for s in (3, 1, 0, 2)], 30, 0.0, 0.9,
                                                [5, 6, 7, 2 ** 64 - 1])
            assert rng == [5, 6, 7, 2 ** 64 - 1]
            assert ctx.get_option(runtime.OPT_BATCH_SAMPLED_TOKENS) == 0
        else:
            toks = ctx.decode_greedy_batch([3, 1, 0, 2], [fed[offs[s]] for s in (3, 1, 0, 2)], [offs[s] for s in (3, 1, 0, 2)], 30)
        out.append(toks)
        ctx.close()
    assert np.array_equal(out[0], out[1])
    for i, s in enumerate((3, 1, 0, 2)):
        assert out[0][i].tolist() == meta["argmax"][offs[s]:offs[s] + 30]


def _upload(ctx, tensors):
    for kind, layers, count in runtime.tensor_shapes(ctx.cfg):
        per = tensors[kind].reshape(max(layers, 1), -1)
        for layer in range(max(layers, 1)):
            ctx.upload(kind, layer if layers else -1, per[layer])


@pytest.mark.parametrize("case", A.CASES)
def test_argmax_edges_beside_sampled_rows(case):
    """The argmax edge models (ties, +-0, +-inf, NaN, all NaN, NaN at index 0): temperature-0 rows beside sampled rows pick what the
    REAL reference picked."""
    meta = json.load(open(os.path.join(GOLD, "argmax_%s_vec.json" % case)))
    fed, picks = meta["tokens_fed"], meta["picks"]
    ctx = runtime.Context(A.SHAPES["vec"])
    _upload(ctx, A.tensors_of(case, "vec"))
    ctx.seq_reserve(6)
    starts = {0: 0, 1: 2, 2: 5, 3: 7}
    steps = len(picks) - max(starts.values())
    for s, p in starts.items():
        if p:
            ctx.seq_prefill(s, fed[:p], 0)
    seqs = [3, 4, 1, 0, 5, 2]
    firsts = [fed[starts[s]] if s in starts else 1 for s in seqs]
    pos = [starts.get(s, 0) for s in seqs]
    temps = [0.0 if s in starts else 0.9 for s in seqs]
    topps = [0.0] * 6
    got, _ = ctx.decode_sample_batch(seqs, firsts, pos, steps, temps, topps, [1 + i for i in range(6)])
    for i, s in enumerate(seqs):
        if s in starts:
            assert got[i].tolist() == picks[starts[s]:starts[s] + steps], (case, s)
    ctx.close()


def test_isolation_and_interleaving():
    """After batch sampling, l2_decode_sample on the context still reproduces cli_temp and its counter is untouched; sequences not in
    a call keep their caches bit for bit; greedy and sampled batch calls alternate and continue correctly; L2_OPT_CHECK_POS accepts a
    continuation and refuses a skip ahead."""
    mt, t_t, p_t, s_t = sampled_run("cli_temp")
    ft = mt["tokens_fed"]
    ctx = new_ctx(mt["header"], mt["seed"], 6)
    ref = new_ctx(mt["header"], mt["seed"], 6)
    idle = (ctx.read_seq_cache(5, "key_cache").tobytes(), ctx.read_seq_cache(5, "value_cache").tobytes())
    seqs, temps, topps = [1, 2, 3, 4], [0.9, 0.0, 1.0, 0.7], [1.0, 0.0, 0.9, 0.5]
    toks, pos, rng, want = [1, 9, 99, 999], [0] * 4, [42, 5, 6, 7], [[] for _ in range(4)]
    ref_toks, ref_pos, ref_rng = list(toks), list(pos), [O.Rng(s) for s in rng]
    got = [[] for _ in range(4)]
    for call in range(6):
        n = 3 + call
        if call % 2:
            out = ctx.decode_greedy_batch(seqs, toks, pos, n)
            tt = [0.0] * 4
        else:
            out, rng = ctx.decode_sample_batch(seqs, toks, pos, n, temps, topps, rng)
            tt = temps
        for k in range(n):
            lg = ref.forward_batch(seqs, ref_toks, ref_pos)
            for i in range(4):
                ref_toks[i], _ = O.next_token(lg[i], tt[i], topps[i], ref_rng[i])
                want[i].append(ref_toks[i])
                ref_pos[i] += 1
        for i in range(4):
            got[i] += out[i].tolist()
        toks = out[:, -1].tolist()
        pos = [p + n for p in pos]
    assert got == want
    assert rng == [r.state.value for r in ref_rng]
    assert (ctx.read_seq_cache(5, "key_cache").tobytes(), ctx.read_seq_cache(5, "value_cache").tobytes()) == idle
    # the single-sequence sampler on sequence 0 of the same context
    assert ctx.get_option(runtime.OPT_SAMPLED_TOKENS) == 0
    single, _ = ctx.decode_sample(ft[0], 0, len(ft) - 1, t_t, p_t, s_t)
    assert single.tolist() == ft[1:]
    assert ctx.get_option(runtime.OPT_SAMPLED_TOKENS) == len(ft) - 1
    # L2_OPT_CHECK_POS
    ctx.set_option(runtime.OPT_CHECK_POS, 1)
    ctx.decode_sample_batch([1], [toks[0]], [pos[0]], 2, 0.9, 1.0, [rng[0]])
    assert code_of(ctx.decode_sample_batch, [1], [toks[0]], [pos[0] + 5], 2, 0.9, 1.0, [rng[0]]) == E_STATE
    ctx.close(); ref.close()


def test_7b_width_rows_to_the_end_of_the_context():
    """llama2_7b_L2 (d = 4096, h = 11008): 4 rows prefilled to 2032 .. 2020, 16 steps ending at position 2047, plain and top-p."""
    meta = load_meta("llama2_7b_L2")
    fed = meta["tokens_fed"]
    offs = [2032, 2030, 2025, 2020]
    assert len(fed) > max(offs)

    def prefill(c):
        for s, o in enumerate(offs):
            c.seq_prefill(s, fed[:o], 0)
    _, (c12, _), sampled = check_against_oracle(meta["header"], meta["seed"], [0, 1, 2, 3], [fed[o] for o in offs], offs, 16,
                                                [0.9, 1.0, 0.8, 1.1], [1.0, 0.9, 0.0, 0.6], [1, 2, 3, 4], prefill)
    assert c12 == sampled


def test_full_7b_eight_rows():
    """Full 32-layer llama2_7b: 8 rows at staggered golden offsets, 16 steps, mixed settings, against the oracle fed the batch logits."""
    meta = load_meta("llama2_7b")
    fed = meta["tokens_fed"]
    offs = [0, 17, 64, 130, 255, 400, 700, 900]

    def prefill(c):
        for s, o in enumerate(offs):
            if o:
                c.seq_prefill(s, fed[:o], 0)
    check_against_oracle(meta["header"], meta["seed"], list(range(8)), [fed[o] for o in offs], offs, 16,
                         [0.9, 1.0, 0.0, 0.7, 1.5, 1.0, 0.3, -1.0], [1.0, 0.9, 0.0, 0.5, 0.0, 0.99, 0.8, 0.0], [11 + s for s in range(8)], prefill)


def test_bad_arguments_return_their_codes_and_the_context_still_decodes():
    meta = load_meta("stories15M")
    hdr, seed = meta["header"], meta["seed"]
    early = runtime.Context(hdr); early.synth_fill(seed)
    assert code_of(early.decode_sample_batch, [0], [1], [0], 4, 0.9, 1.0, [1]) == E_STATE
    early.close()
    ctx = new_ctx(hdr, seed, 4)
    nan = float("nan")
    assert code_of(ctx.decode_sample_batch, [0, 1], [1, 1], [0, 0], 4, [0.9, nan], 1.0, [1, 2]) == E_ARG
    assert code_of(ctx.decode_sample_batch, [0, 1], [1, 1], [0, 0], 4, 0.9, [nan, 0.5], [1, 2]) == E_ARG
    assert code_of(ctx.decode_sample_batch, [0, 1, 2, 3, 0], [1] * 5, [0] * 5, 4, 0.9, 1.0, [1] * 5) == E_ARG    # n > n_seqs
    assert code_of(ctx.decode_sample_batch, [0, 0], [1, 1], [0, 0], 4, 0.9, 1.0, [1, 2]) == E_ARG                # duplicate
    S = hdr[6]
    assert code_of(ctx.decode_sample_batch, [0], [1], [S - 2], 4, 0.9, 1.0, [1]) == E_ARG                        # past seq_len
    import ctypes as C
    L = runtime.lib()
    one = (C.c_int32 * 1)(0); tok = (C.c_int32 * 1)(1); d = (C.c_double * 1)(0.9); r = (C.c_uint64 * 1)(5); out = (C.c_int32 * 4)()
    assert L.l2_decode_sample_batch(ctx._h, 1, one, tok, one, 4, None, d, r, out) == E_ARG
    assert L.l2_decode_sample_batch(ctx._h, 1, one, tok, one, 4, d, None, r, out) == E_ARG
    assert L.l2_decode_sample_batch(ctx._h, 1, one, tok, one, 4, d, d, None, out) == E_ARG
    assert L.l2_decode_sample_batch(ctx._h, 1, one, tok, one, 4, d, d, r, None) == E_ARG
    assert L.l2_decode_sample_batch(ctx._h, 0, one, tok, one, 4, d, d, r, out) == E_ARG
    assert r[0] == 5
    toks, _ = ctx.decode_sample_batch([0], [1], [0], 8, 0.0, 0.0, [1])
    assert toks[0].tolist() == meta["argmax"][:8]
    ctx.close()
    big = (64, 176, 1, 4, 4, 256 * 1024 + 16, 8)
    ctx = new_ctx(big, 3, 2)
    assert code_of(ctx.decode_sample_batch, [0, 1], [1, 2], [0, 0], 2, [0.0, 0.9], 1.0, [1, 2]) == E_CONFIG
    greedy, rng = ctx.decode_sample_batch([0, 1], [1, 2], [0, 0], 2, 0.0, 1.0, [1, 2])
    assert rng == [1, 2]
    assert np.array_equal(greedy, ctx.decode_greedy_batch([0, 1], [1, 2], [0, 0], 2))
    ctx.close()
