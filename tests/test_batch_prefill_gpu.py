"""Packed prompt ingestion for many sequences (include/llama2_hip.h: l2_seq_prefill_batch; csrc/batch_host.hip.h, batch.hip.h:
bp_attn_mfma_kernel).  Every prompt is a prefix of a trajectory with a known answer -- the REAL reference's fed tokens
(tests/golden/<model>.json) or the C oracle run per sequence -- and is held to the batch path's bars: last-position argmax exact,
logits within 1e-4 of the reference where it kept them and within 1e-5 of l2_seq_prefill on the same sequence in a second context,
caches within 1e-6 of that context's, and a following batched greedy decode that reproduces the reference's picks."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from llama2_ts_amd import runtime

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-4
E_ARG, E_STATE = -1, -4
LENGTHS = (1, 3, 15, 16, 17, 31, 64, 65, 100, 255)
# head_size 128 at a context past the MFMA attention's 150 KiB LDS bound (about 2 400 keys): dim, hidden, layers, heads, kv heads, vocab, seq_len
LONG_HS128 = (256, 512, 1, 2, 2, 512, 3072)


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


def code_of(fn, *args):
    with pytest.raises(runtime.L2Error) as e:
        fn(*args)
    return e.value.code


def written(ctx, s, name, L, S, d, upto):
    return ctx.read_seq_cache(s, name).reshape(L, S, d)[:, :upto]


def check_against_seq_prefill(meta, ctx, seqs, prompts, pos0, lg, opts=None, logit_tol=1e-5, cache_tol=1e-6):
    """The same prompts through l2_seq_prefill, one sequence at a time, in a second context: logits and the written cache rows."""
    hdr = meta["header"]
    d, L, S = hdr[0], hdr[2], hdr[6]
    ref = new_ctx(hdr, meta["seed"], max(seqs) + 1, opts)
    want = [np.array(ref.seq_prefill(s, p, p0), copy=True) for s, p, p0 in zip(seqs, prompts, pos0)]
    for i, s in enumerate(seqs):
        assert np.abs(lg[i] - want[i]).max() <= logit_tol, (s, float(np.abs(lg[i] - want[i]).max()))
        end = pos0[i] + len(prompts[i])
        for name in ("key_cache", "value_cache") if cache_tol is not None else ():
            a, b = written(ctx, s, name, L, S, d, end), written(ref, s, name, L, S, d, end)
            assert np.abs(a - b).max() <= cache_tol, (s, name)
    ref.close()
    return want


def mixed_prompts(meta, decode_steps, rng):
    fed = meta["tokens_fed"]
    S = meta["header"][6]
    lens = [n for n in LENGTHS if n + decode_steps <= min(len(fed), S)]
    lens = [lens[i] for i in rng.permutation(len(lens))]
    return lens, [fed[:n] for n in lens]


@pytest.mark.parametrize("name", ["tiny", "stories15M", "stories110M"])
def test_mixed_prompts_follow_the_reference(name):
    """Prompts of mixed lengths (golden prefixes) in shuffled sequence order, more rows than one launch sequence holds (64 on tiny,
    whose hidden size keeps the 16-row-tile kernels; 256 elsewhere), so prompts straddle launch sequences.  Then 8 batched greedy
    steps from every prompt's end follow the reference."""
    meta, g = load_gold(name)
    fed, picks = meta["tokens_fed"], meta["argmax"]
    keep = {p: i for i, p in enumerate(meta["logit_positions"])}
    steps = 8
    rng = np.random.default_rng(5)
    lens, prompts = mixed_prompts(meta, steps, rng)
    assert sum(lens) > (64 if name == "tiny" else 256)
    n = len(lens)
    seqs = [int(s) for s in rng.permutation(n)]
    ctx = new_ctx(meta["header"], meta["seed"], n)
    lg = ctx.seq_prefill_batch(seqs, prompts, [0] * n)
    assert lg.shape == (n, ctx.cfg.vocab_size)
    for i, L_ in enumerate(lens):
        assert runtime.argmax(lg[i]) == picks[L_ - 1], (name, i, L_)
        if L_ - 1 in keep:
            assert np.abs(lg[i] - g["logits"][keep[L_ - 1]]).max() <= TOL, (name, L_)
    check_against_seq_prefill(meta, ctx, seqs, prompts, [0] * n, lg)
    toks = ctx.decode_greedy_batch(seqs, [fed[L_] for L_ in lens], lens, steps)
    for i, L_ in enumerate(lens):
        assert toks[i].tolist() == picks[L_:L_ + steps], (name, i, L_)
    ctx.close()


def test_stories15M_prompt_fed_to_several_sequences():
    """The reference's "Once upon a time" run (-i): its prompt fed to four sequences in one call (sequence 0 among them), then the
    generated continuation through the batch loop, row for row the reference's."""
    meta, g = load_gold("stories15M_prompt")
    fed, picks = meta["tokens_fed"], meta["argmax"]
    P = next(p for p in range(len(fed) - 1) if all(fed[q + 1] == picks[q] for q in range(p, len(fed) - 1))) + 1   # forced positions
    assert P >= 4
    keep = {p: i for i, p in enumerate(meta["logit_positions"])}
    ctx = new_ctx(meta["header"], meta["seed"], 5)
    seqs = [3, 0, 4, 1]
    lg = ctx.seq_prefill_batch(seqs, [fed[:P]] * 4, 0)
    for i in range(4):
        assert runtime.argmax(lg[i]) == picks[P - 1]
        if P - 1 in keep:
            assert np.abs(lg[i] - g["logits"][keep[P - 1]]).max() <= TOL
    steps = len(fed) - P
    toks = ctx.decode_greedy_batch(seqs, [fed[P]] * 4, [P] * 4, steps)
    for i in range(4):
        assert toks[i].tolist() == picks[P:P + steps], i
    ctx.close()


def test_7b_width_prompts_to_the_end_of_the_context():
    """llama2_7b_L2 (head_size 128, MFMA attention): one 2047-token prompt from position 0, a continuation 1900 .. 2039 of a sequence
    l2_seq_prefill filled to 1900, and a 17-token prompt, in one call; the long ones end near position 2047."""
    meta, g = load_gold("llama2_7b_L2")
    fed, picks = meta["tokens_fed"], meta["argmax"]
    keep = {p: i for i, p in enumerate(meta["logit_positions"])}
    ctx = new_ctx(meta["header"], meta["seed"], 3)
    ctx.seq_prefill(1, fed[:1900], 0)
    seqs, prompts, pos0 = [2, 1, 0], [fed[:2047], fed[1900:2040], fed[:17]], [0, 1900, 0]
    lg = ctx.seq_prefill_batch(seqs, prompts, pos0)
    for i, end in enumerate((2047, 2040, 17)):
        assert runtime.argmax(lg[i]) == picks[end - 1], (i, end)
        if end - 1 in keep:
            assert np.abs(lg[i] - g["logits"][keep[end - 1]]).max() <= TOL, end
    hdr = meta["header"]
    d, L, S = hdr[0], hdr[2], hdr[6]
    ref = new_ctx(hdr, meta["seed"], 3)
    ref.seq_prefill(1, fed[:1900], 0)
    for i, (s, p, p0) in enumerate(zip(seqs, prompts, pos0)):
        want = ref.seq_prefill(s, p, p0)
        assert np.abs(lg[i] - want).max() <= 1e-5, s
        for name in ("key_cache", "value_cache"):
            a = written(ctx, s, name, L, S, d, p0 + len(p))[:, -64:]
            b = written(ref, s, name, L, S, d, p0 + len(p))[:, -64:]
            assert np.abs(a - b).max() <= 1e-6, (s, name)
    ref.close()
    toks = ctx.decode_greedy_batch([2, 1], [fed[2047], fed[2040]], [2047, 2040], 1)
    assert toks[:, 0].tolist() == [picks[2047], picks[2040]]
    ctx.close()


def test_head_size_128_past_the_lds_bound_takes_the_decode_attention():
    """head_size 128 with prompts ending past position 2 400, where the 16-query tile's scores no longer fit the 150 KiB LDS bound and
    the launch sequence takes the decode kernel per (head, row): logits against the C oracle run token by token and l2_seq_prefill."""
    hdr, seed = LONG_HS128, 7
    rng = np.random.default_rng(3)
    V = hdr[5]
    long_p = [int(t) for t in rng.integers(0, V, 2600)]
    short_p = [int(t) for t in rng.integers(0, V, 40)]
    orc = O.Oracle(hdr, seed)
    for p, t in enumerate(long_p):
        want = np.array(orc.forward(t, p), copy=True)
    orc.close()
    ctx = new_ctx(hdr, seed, 2)
    ctx.seq_prefill(1, long_p[:2500], 0)
    lg = ctx.seq_prefill_batch([0, 1], [long_p, long_p[2500:]], [0, 2500])
    for i in range(2):
        assert np.abs(lg[i] - want).max() <= TOL, i
        assert runtime.argmax(lg[i]) == O.argmax(want)
    lg2 = ctx.seq_prefill_batch([1, 0], [short_p, long_p[2590:]], [2600, 2590])
    ref = new_ctx(hdr, seed, 2)
    ref.seq_prefill(1, long_p, 0)
    ref.seq_prefill(0, long_p[:2590], 0)
    for i, (s, p, p0) in enumerate(((1, short_p, 2600), (0, long_p[2590:], 2590))):
        assert np.abs(lg2[i] - ref.seq_prefill(s, p, p0)).max() <= 1e-5, s
    ref.close(); ctx.close()


def test_exact_attention_option_is_honoured():
    """L2_OPT_EXACT_ATTENTION: the decode kernel's attention form per (head, row), as l2_seq_prefill takes it: logits and caches against
    l2_seq_prefill under the same option, argmax against the reference."""
    meta, _ = load_gold("stories110M")
    picks = meta["argmax"]
    lens, prompts = mixed_prompts(meta, 0, np.random.default_rng(9))
    n = len(lens)
    opts = {runtime.OPT_EXACT_ATTENTION: 1}
    ctx = new_ctx(meta["header"], meta["seed"], n, opts)
    seqs = list(range(n))[::-1]
    lg = ctx.seq_prefill_batch(seqs, prompts, 0)
    for i, L_ in enumerate(lens):
        assert runtime.argmax(lg[i]) == picks[L_ - 1], L_
    check_against_seq_prefill(meta, ctx, seqs, prompts, [0] * n, lg, opts)
    ctx.close()


def test_f32_mfma_option_against_seq_prefill():
    """L2_OPT_PREFILL_F32_MFMA (fp32 accumulate, opt-in): within the 1e-4 logit bar of l2_seq_prefill with the option on; tokens compared
    where that prefill's tokens are the reference's."""
    meta, _ = load_gold("stories110M")
    picks = meta["argmax"]
    lens, prompts = mixed_prompts(meta, 0, np.random.default_rng(13))
    n = len(lens)
    opts = {runtime.OPT_PREFILL_F32_MFMA: 1}
    ctx = new_ctx(meta["header"], meta["seed"], n, opts)
    seqs = list(range(n))
    lg = ctx.seq_prefill_batch(seqs, prompts, 0)
    want = check_against_seq_prefill(meta, ctx, seqs, prompts, [0] * n, lg, opts, logit_tol=TOL, cache_tol=None)
    agree = 0
    for i, L_ in enumerate(lens):
        if runtime.argmax(want[i]) == picks[L_ - 1]:
            assert runtime.argmax(lg[i]) == picks[L_ - 1], L_
            agree += 1
    assert agree >= 1
    ctx.close()


def test_both_weight_sources(monkeypatch):
    """The row-major tensors (L2_ONE_COPY=0 keeps them) and the repacked copies a decode step leaves as the only ones: the same tokens
    and logits within 1e-5 of each other and of the reference's picks."""
    meta, _ = load_gold("stories110M")
    picks = meta["argmax"]
    lens, prompts = mixed_prompts(meta, 0, np.random.default_rng(17))
    n = len(lens)
    seqs = list(range(n))
    packed = new_ctx(meta["header"], meta["seed"], n)
    packed.forward(meta["tokens_fed"][0], 0)                # a decode step: the repacked copies are the only weights from here on
    lg_p = packed.seq_prefill_batch(seqs, prompts, 0)
    packed.close()
    monkeypatch.setenv("L2_ONE_COPY", "0")
    rowmajor = new_ctx(meta["header"], meta["seed"], n)
    lg_r = rowmajor.seq_prefill_batch(seqs, prompts, 0)
    rowmajor.close()
    for i, L_ in enumerate(lens):
        assert runtime.argmax(lg_p[i]) == picks[L_ - 1] and runtime.argmax(lg_r[i]) == picks[L_ - 1], L_
        assert np.abs(lg_p[i] - lg_r[i]).max() <= 1e-5, L_


def test_continuation_isolation_and_position_rule():
    """pos0 > 0 on sequences that already hold decoded rows; reserved sequences not named keep their caches byte for byte; sequence 0
    through the packed call leaves the single-sequence logits alone; L2_OPT_CHECK_POS accepts continuations and refuses a skip-ahead."""
    meta, _ = load_gold("stories15M")
    fed, picks = meta["tokens_fed"], meta["argmax"]
    ctx = new_ctx(meta["header"], meta["seed"], 6)
    ctx.set_option(runtime.OPT_CHECK_POS, 1)
    toks = ctx.decode_greedy_batch([1, 2], [fed[0]] * 2, [0, 0], 20)      # rows 0 .. 19 of sequences 1, 2: decoded
    assert toks[0].tolist() == picks[:20]
    ctx.seq_prefill(4, fed[:50], 0)
    ctx.forward(fed[0], 0)                                                 # sequence 0's own logits (position 0)
    logits0 = ctx.read_state("logits").tobytes()
    idle = {s: (ctx.read_seq_cache(s, "key_cache").tobytes(), ctx.read_seq_cache(s, "value_cache").tobytes()) for s in (3, 5)}
    lg = ctx.seq_prefill_batch([2, 0, 1, 4], [fed[20:40], fed[1:90], fed[20:25], fed[50:51]], [20, 1, 20, 50])
    for i, end in enumerate((40, 90, 25, 51)):
        assert runtime.argmax(lg[i]) == picks[end - 1], (i, end)
    assert ctx.read_state("logits").tobytes() == logits0, "the packed call changed sequence 0's single-sequence logits"
    for s in (3, 5):
        assert (ctx.read_seq_cache(s, "key_cache").tobytes(), ctx.read_seq_cache(s, "value_cache").tobytes()) == idle[s], s
    assert code_of(ctx.seq_prefill_batch, [1, 3], [fed[25:30], fed[10:12]], [25, 10]) == E_STATE      # sequence 3 holds no rows
    assert code_of(ctx.seq_prefill_batch, [2], [fed[41:45]], [41]) == E_STATE                        # 40 is next
    lg = ctx.seq_prefill_batch([2, 1, 3], [fed[40:45], fed[25:30], fed[:3]], [40, 25, 0])            # continuations and a fresh start
    assert [runtime.argmax(r) for r in lg] == [picks[44], picks[29], picks[2]]
    toks = ctx.decode_greedy_batch([0, 2, 4], [fed[90], fed[45], fed[51]], [90, 45, 51], 10)
    assert toks.tolist() == [picks[90:100], picks[45:55], picks[51:61]]
    ctx.close()


def test_random_prompts_against_the_oracle():
    """stories110M, random prompts of 5 .. 70 tokens (one straddles nothing, all in one launch sequence) against the C oracle run token
    by token per sequence: last-position logits within 1e-4, argmax exact."""
    meta, _ = load_gold("stories110M")
    hdr, seed = meta["header"], meta["seed"]
    rng = np.random.default_rng(21)
    lens = [5, 33, 70, 20]
    prompts = [[int(t) for t in rng.integers(0, hdr[5], n)] for n in lens]
    orc = O.Oracle(hdr, seed)
    want = []
    for p in prompts:
        for pos, t in enumerate(p):
            lg = np.array(orc.forward(t, pos), copy=True)
        want.append(lg)
    orc.close()
    ctx = new_ctx(hdr, seed, 4)
    got = ctx.seq_prefill_batch([1, 3, 0, 2], prompts, 0)
    for i in range(4):
        assert np.abs(got[i] - want[i]).max() <= TOL, i
        assert runtime.argmax(got[i]) == O.argmax(want[i]), i
    ctx.close()


def test_bad_arguments_return_their_codes_and_the_context_still_decodes():
    meta, _ = load_gold("tiny")
    fed, picks = meta["tokens_fed"], meta["argmax"]
    V, S = meta["header"][5], meta["header"][6]
    ctx = runtime.Context(meta["header"]); ctx.synth_fill(meta["seed"])
    assert code_of(ctx.seq_prefill_batch, [0], [[1, 2]], 0) == E_STATE                     # before the reserve
    ctx.seq_reserve(4)
    L = runtime.lib()
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    one, two = i32(0), i32(2)
    assert L.l2_seq_prefill_batch(ctx._h, 1, None, two, i32(1, 2), one, None) == E_ARG
    assert L.l2_seq_prefill_batch(ctx._h, 1, one, None, i32(1, 2), one, None) == E_ARG
    assert L.l2_seq_prefill_batch(ctx._h, 1, one, two, None, one, None) == E_ARG
    assert L.l2_seq_prefill_batch(ctx._h, 1, one, two, i32(1, 2), None, None) == E_ARG
    assert L.l2_seq_prefill_batch(ctx._h, 0, one, i32(1), i32(1), one, None) == E_ARG       # n = 0
    bad = [([0, 1, 2, 3, 0], [[1]] * 5, [0] * 5),                     # n > n_seqs
           ([4], [[1]], [0]), ([-1], [[1]], [0]),                     # sequence out of range
           ([1, 1], [[1], [2]], [0, 0]),                              # named twice
           ([1], [[]], [0]),                                          # n_tokens < 1
           ([1], [[V]], [0]), ([1], [[1, -1]], [0]),                  # token out of range
           ([1], [[1] * 3], [S - 2]), ([1], [[1]], [-1])]             # past seq_len / negative position
    for seqs, prompts, pos0 in bad:
        assert code_of(ctx.seq_prefill_batch, seqs, prompts, pos0) == E_ARG, (seqs, prompts, pos0)
    assert L.l2_seq_prefill_batch(ctx._h, 2, i32(0, 1), i32(2, 0), i32(1, 2), i32(0, 0), None) == E_ARG   # n_tokens 0
    ctx.set_option(runtime.OPT_CHECK_POS, 1)
    assert code_of(ctx.seq_prefill_batch, [0, 2], [[1], [1]], [0, 5]) == E_STATE
    ctx.set_option(runtime.OPT_CHECK_POS, 0)
    for s in range(4):      # nothing was written by the refused calls: every sequence still decodes the reference's run
        lg = ctx.seq_prefill_batch([s], [fed[:10]], 0)
        assert runtime.argmax(lg[0]) == picks[9]
    toks = ctx.decode_greedy_batch([3, 1, 0, 2], [fed[10]] * 4, [10] * 4, 20)
    assert all(r == picks[10:30] for r in toks.tolist())
    ctx.close()
