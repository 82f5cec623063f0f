"""The mixed step of continuous batching (include/llama2_hip.h: l2_step_batch; csrc/batch_host.hip.h): decode rows (runs of one token)
and prompt runs in one call, one pick per row on the device.  Decode rows continue golden trajectories, prompt runs are golden
prefixes; greedy picks are held to the reference's argmax, logits to the reference where it kept them (1e-4), to l2_forward_batch for
the decode rows and to l2_seq_prefill_batch for the runs on a second context (1e-5), and the caches to that context's (1e-6).  Sampled
rows are held to the oracle's sampler fed the call's own logits."""
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
E_ARG, E_CONFIG, E_STATE = -1, -2, -4
PROMPT_LENGTHS = (1, 15, 16, 17, 65, 255)
LONG_HS128 = (256, 512, 1, 2, 2, 512, 3072)      # head_size 128, context past the MFMA attention's 150 KiB LDS bound


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


def written(ctx, s, name, L, S, d, upto):
    return ctx.read_seq_cache(s, name).reshape(L, S, d)[:, :upto]


def mixed_plan(meta, rng, n_decode):
    """Prompt runs (golden prefixes at 0) and decode rows (golden tokens at staggered positions, their sequences filled before), shuffled."""
    fed = meta["tokens_fed"]
    S = meta["header"][6]
    top = min(len(fed), S) - 1
    lens = [n for n in PROMPT_LENGTHS if n <= top]
    lens += [n for n in (31, 47, 63) if n <= top and sum(lens) + n_decode <= 64]      # tiny: more rows than one 64-row launch sequence
    dpos = sorted({int(p) for p in rng.integers(1, top, n_decode)})
    rows = [("p", L_) for L_ in lens] + [("d", p) for p in dpos]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    seqs = [int(s) for s in rng.permutation(len(rows))]
    runs = [fed[:v] if k == "p" else [fed[v]] for k, v in rows]
    pos0 = [0 if k == "p" else v for k, v in rows]
    ends = [v - 1 if k == "p" else v for k, v in rows]       # the position each row's pick is made at
    return seqs, runs, pos0, ends


def fill_decode_sequences(ctx, meta, seqs, runs, pos0):
    fed = meta["tokens_fed"]
    pre = [(s, p) for s, r, p in zip(seqs, runs, pos0) if p > 0]
    if pre:
        ctx.seq_prefill_batch([s for s, _ in pre], [fed[:p] for _, p in pre], 0)


def check_against_two_calls(meta, ctx, seqs, runs, pos0, lg, opts=None, logit_tol=1e-5, cache_tol=1e-6):
    """A second context: the same earlier fills, l2_forward_batch for the decode rows and l2_seq_prefill_batch for the runs."""
    hdr = meta["header"]
    d, L, S = hdr[0], hdr[2], hdr[6]
    ref = new_ctx(hdr, meta["seed"], ctx.get_option(runtime.OPT_SEQS), opts)
    fill_decode_sequences(ref, meta, seqs, runs, pos0)
    dec = [i for i, r in enumerate(runs) if len(r) == 1]
    pro = [i for i, r in enumerate(runs) if len(r) > 1]
    want = {}
    if dec:
        w = ref.forward_batch([seqs[i] for i in dec], [runs[i][0] for i in dec], [pos0[i] for i in dec])
        want.update({i: w[k] for k, i in enumerate(dec)})
    if pro:
        w = ref.seq_prefill_batch([seqs[i] for i in pro], [runs[i] for i in pro], [pos0[i] for i in pro])
        want.update({i: w[k] for k, i in enumerate(pro)})
    for i, s in enumerate(seqs):
        assert np.abs(lg[i] - want[i]).max() <= logit_tol, (i, s, float(np.abs(lg[i] - want[i]).max()))
        end = pos0[i] + len(runs[i])
        for name in ("key_cache", "value_cache") if cache_tol is not None else ():
            a, b = written(ctx, s, name, L, S, d, end), written(ref, s, name, L, S, d, end)
            assert np.abs(a - b).max() <= cache_tol, (s, name)
    ref.close()
    return want


@pytest.mark.parametrize("name", ["tiny", "stories15M", "stories110M"])
def test_mixed_rows_follow_the_reference(name):
    """Decode rows and prompt runs of lengths 1 .. 255 in one shuffled call, more rows than one launch sequence holds."""
    meta, g = load_gold(name)
    picks = meta["argmax"]
    keep = {p: i for i, p in enumerate(meta["logit_positions"])}
    rng = np.random.default_rng(31)
    seqs, runs, pos0, ends = mixed_plan(meta, rng, 8)
    assert sum(len(r) for r in runs) > (64 if name == "tiny" else 256)
    ctx = new_ctx(meta["header"], meta["seed"], len(seqs))
    fill_decode_sequences(ctx, meta, seqs, runs, pos0)
    got, rng_after, lg = ctx.step_batch(seqs, runs, pos0, logits=True)
    assert rng_after is None
    for i, e in enumerate(ends):
        assert got[i] == picks[e] == runtime.argmax(lg[i]), (name, i, e)
        if e in keep:
            assert np.abs(lg[i] - g["logits"][keep[e]]).max() <= TOL, (name, e)
    check_against_two_calls(meta, ctx, seqs, runs, pos0, lg)
    # the next step continues every row from its own pick (all decode rows now)
    nxt, _ = ctx.step_batch(seqs, [[p] for p in got], [e + 1 for e in ends])
    assert nxt == [picks[e + 1] for e in ends]
    ctx.close()


def test_sampled_rows_are_the_oracle_sampler_on_the_calls_logits(monkeypatch):
    meta, _ = load_gold("stories15M")
    rng = np.random.default_rng(41)
    seqs, runs, pos0, _ = mixed_plan(meta, rng, 10)
    n = len(seqs)
    temp = [0.9, 1.0, 0.0] + [float(v) for v in rng.uniform(0.2, 1.6, n - 3)]      # cli_temp's and cli_topp's settings, then random
    topp = [1.0, 0.9, 0.9] + [float(v) for v in rng.choice([0.0, 0.5, 0.9, 0.99, 1.0], n - 3)]
    temp[5] = 0.0
    seeds = [42, 7] + [int(v) for v in rng.integers(1, 1 << 62, n - 2)]

    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = new_ctx(meta["header"], meta["seed"], n)
        fill_decode_sequences(ctx, meta, seqs, runs, pos0)
        before = ctx.get_option(runtime.OPT_BATCH_SAMPLED_TOKENS)
        out = ctx.step_batch(seqs, runs, pos0, temp, topp, seeds, logits=True)
        assert ctx.get_option(runtime.OPT_BATCH_SAMPLED_TOKENS) - before == sum(1 for t in temp if t != 0.0)
        ctx.close()
        return out

    got, after, lg = run({})
    for i in range(n):
        r = O.Rng(seeds[i])
        want, _ = O.next_token(lg[i], temp[i], topp[i], r) if temp[i] != 0.0 else (O.argmax(lg[i]), None)
        assert got[i] == want, (i, temp[i], topp[i])
        assert after[i] == (int(r.state.value) if temp[i] != 0.0 else seeds[i]), i
    got2, after2, _ = run({"L2_TEST_HOOKS": "1", "L2_SAMPLER_FORCE_SERIAL": "1"})
    assert got2 == got and after2 == after


def test_head_size_128_decode_rows_past_the_lds_bound_beside_prompts():
    """Decode rows at 2 500 - 3 000 (past the 16-query tile's LDS bound) and prompt runs at 0 in one call: both attention forms run."""
    hdr, seed = LONG_HS128, 7
    rng = np.random.default_rng(3)
    V = hdr[5]
    fed = [1] + [int(t) for t in rng.integers(2, V, 3070)]
    meta = {"header": hdr, "seed": seed, "tokens_fed": fed}
    seqs = [2, 0, 3, 1]
    runs = [[fed[2500]], fed[:40], fed[:17], [fed[2999]]]
    pos0 = [2500, 0, 0, 2999]
    ctx = new_ctx(hdr, seed, 4)
    fill_decode_sequences(ctx, meta, seqs, runs, pos0)
    got, _, lg = ctx.step_batch(seqs, runs, pos0, logits=True)
    assert got == [runtime.argmax(r) for r in lg]
    check_against_two_calls(meta, ctx, seqs, runs, pos0, lg)
    ctx.close()


def test_7b_width_decode_rows_near_the_end_of_the_context():
    meta, g = load_gold("llama2_7b_L2")
    fed, picks = meta["tokens_fed"], meta["argmax"]
    keep = {p: i for i, p in enumerate(meta["logit_positions"])}
    seqs, runs, pos0 = [1, 0, 2], [[fed[2040]], fed[:64], [fed[2046]]], [2040, 0, 2046]
    ctx = new_ctx(meta["header"], meta["seed"], 3)
    fill_decode_sequences(ctx, meta, seqs, runs, pos0)
    got, _, lg = ctx.step_batch(seqs, runs, pos0, logits=True)
    assert got == [picks[2040], picks[63], picks[2046]]
    for i, e in enumerate((2040, 63, 2046)):
        if e in keep:
            assert np.abs(lg[i] - g["logits"][keep[e]]).max() <= TOL, e
    check_against_two_calls(meta, ctx, seqs, runs, pos0, lg)
    ctx.close()


def test_exact_attention_option_is_honoured():
    meta, _ = load_gold("stories110M")
    picks = meta["argmax"]
    seqs, runs, pos0, ends = mixed_plan(meta, np.random.default_rng(9), 6)
    opts = {runtime.OPT_EXACT_ATTENTION: 1}
    ctx = new_ctx(meta["header"], meta["seed"], len(seqs), opts)
    fill_decode_sequences(ctx, meta, seqs, runs, pos0)
    got, _, lg = ctx.step_batch(seqs, runs, pos0, logits=True)
    assert got == [picks[e] for e in ends]
    check_against_two_calls(meta, ctx, seqs, runs, pos0, lg, opts)
    ctx.close()


def test_f32_mfma_option_against_the_two_calls():
    meta, _ = load_gold("stories110M")
    seqs, runs, pos0, _ = mixed_plan(meta, np.random.default_rng(13), 6)
    opts = {runtime.OPT_PREFILL_F32_MFMA: 1}
    ctx = new_ctx(meta["header"], meta["seed"], len(seqs), opts)
    fill_decode_sequences(ctx, meta, seqs, runs, pos0)
    got, _, lg = ctx.step_batch(seqs, runs, pos0, logits=True)
    assert got == [runtime.argmax(r) for r in lg]
    check_against_two_calls(meta, ctx, seqs, runs, pos0, lg, opts, logit_tol=TOL, cache_tol=None)
    ctx.close()


def test_refused_calls_write_nothing_and_the_context_still_decodes():
    meta, _ = load_gold("tiny")
    fed, picks = meta["tokens_fed"], meta["argmax"]
    hdr = meta["header"]
    V, S, d, L_ = hdr[5], hdr[6], hdr[0], hdr[2]
    ctx = runtime.Context(hdr); ctx.synth_fill(meta["seed"])
    assert code_of(ctx.step_batch, [0], [[1, 2]], 0) == E_STATE                               # before the reserve
    ctx.seq_reserve(4)
    ctx.seq_prefill_batch([1, 2], [fed[:10], fed[:10]], 0)
    caches = {s: (ctx.read_seq_cache(s, "key_cache").tobytes(), ctx.read_seq_cache(s, "value_cache").tobytes()) for s in range(4)}
    Lb = runtime.lib()
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    f64 = lambda *v: (C.c_double * len(v))(*v)
    one, n1 = i32(1), i32(1)
    picks_s = i32(-7, -7)
    rng_s = (C.c_uint64 * 2)(11, 12)
    t, p = f64(0.9, 0.9), f64(1.0, 1.0)
    calls = [(i32(1), None, i32(fed[10]), i32(10), t, p, rng_s, picks_s),          # null n_tokens
             (None, n1, i32(fed[10]), i32(10), t, p, rng_s, picks_s),              # null seqs
             (one, n1, None, i32(10), t, p, rng_s, picks_s),                       # null tokens
             (one, n1, i32(fed[10]), None, t, p, rng_s, picks_s),                  # null pos0
             (one, n1, i32(fed[10]), i32(10), t, p, rng_s, None),                  # null picks_out
             (one, n1, i32(fed[10]), i32(10), None, p, rng_s, picks_s),            # some but not all settings
             (one, n1, i32(fed[10]), i32(10), t, None, rng_s, picks_s),
             (one, n1, i32(fed[10]), i32(10), t, p, None, picks_s),
             (one, n1, i32(fed[10]), i32(10), f64(float("nan")), p, rng_s, picks_s),   # NaN
             (one, n1, i32(fed[10]), i32(10), t, f64(float("nan")), rng_s, picks_s),
             (i32(1, 1), i32(1, 1), i32(3, 4), i32(10, 10), t, p, rng_s, picks_s),    # named twice
             (i32(4), n1, i32(3), i32(0), t, p, rng_s, picks_s),                   # sequence out of range
             (one, i32(0), i32(3), i32(10), t, p, rng_s, picks_s),                 # n_tokens 0
             (one, n1, i32(V), i32(10), t, p, rng_s, picks_s),                     # token out of range
             (one, i32(2), i32(3, 3), i32(S - 1), t, p, rng_s, picks_s)]           # past seq_len
    for k, (s, nt, tok, p0, tt, pp, rr, out) in enumerate(calls):
        n = 2 if k == 10 else 1
        assert Lb.l2_step_batch(ctx._h, n, s, nt, tok, p0, tt, pp, rr, out, None) == E_ARG, k
    assert Lb.l2_step_batch(ctx._h, 0, one, n1, i32(3), i32(10), t, p, rng_s, picks_s, None) == E_ARG            # n = 0
    assert Lb.l2_step_batch(ctx._h, 5, i32(0, 1, 2, 3, 0), i32(1, 1, 1, 1, 1), i32(3, 3, 3, 3, 3), i32(0, 0, 0, 0, 0),
                            None, None, None, picks_s, None) == E_ARG                                               # n > n_seqs
    ctx.set_option(runtime.OPT_CHECK_POS, 1)
    assert code_of(ctx.step_batch, [1, 3], [[fed[10]], [fed[5]]], [10, 5], [0.9, 0.9], 1.0, [11, 12]) == E_STATE   # 3 holds no rows
    assert code_of(ctx.step_batch, [1, 2], [[fed[11]], fed[10:12]], [11, 10]) == E_STATE                        # 10 is next on 1
    assert list(picks_s) == [-7, -7] and list(rng_s) == [11, 12]
    for s in range(4):
        assert (ctx.read_seq_cache(s, "key_cache").tobytes(), ctx.read_seq_cache(s, "value_cache").tobytes()) == caches[s], s
    got, _ = ctx.step_batch([2, 1, 0], [[fed[10]], fed[10:12], fed[:12]], [10, 10, 0])
    assert got == [picks[10], picks[11], picks[11]]
    ctx.set_option(runtime.OPT_CHECK_POS, 0)
    for pos in range(12, 16):      # l2_forward continues sequence 0 from the step's cache rows
        assert runtime.argmax(np.array(ctx.forward(fed[pos], pos), copy=True)) == picks[pos], pos
    ctx.close()
    big = (64, 176, 1, 4, 4, 256 * 1024 + 16, 8)
    ctx = new_ctx(big, 3, 2)
    assert code_of(ctx.step_batch, [0, 1], [[1], [2, 3]], 0, [0.0, 0.9], 1.0, [1, 2]) == E_CONFIG
    greedy, after = ctx.step_batch([0, 1], [[1], [2, 3]], 0, [0.0, 0.0], 1.0, [1, 2])
    assert after == [1, 2]
    want = ctx.seq_prefill_batch([0, 1], [[1], [2, 3]], 0)
    assert greedy == [runtime.argmax(r) for r in want]
    ctx.close()
