"""One launch for attention and the streaming-form wo on one GPU (csrc/attention.hip.h: attn_wo_stream_kernel) against the two launches it
replaces (L2_ATTN_WO_STREAM=0).

The fused launch changes WHEN things run, never what is computed: its attention role is the tile kernel's own body and its wo role adds the
same products in the same order into the same accumulators as the streaming GEMV.  So every check here is equality of bit patterns
between a default context and one with the switch off, both run with L2_ATTN_SPLIT_ROWS at the end of the fused range (so both use the
same attention form at every position): logits, xb, xb2, att and both caches.  The CPU oracle bounds the small shapes as in
test_hip_parity.py (TOL, equal argmax).

Shapes (header order: dim, hidden, layers, heads, kv heads, vocab, seq_len):
  * (1024, 2816, 2, 8, 8, -1000, 300), L2_SMALL_MAX=0: two column batches per row.  The library's geometry gives a 1024-wide row ONE batch
    of four sub-batches (U = 4), which is never repacked, and the repacked kernels exist for rows wider than their staging round only;
    the fused launch reads the repacked copy only, so this shape runs with L2_TUNE_U=2 and L2_TUNE_NWAVES=2 in BOTH contexts (the
    existing tuning switches): two batches per row, a repacked copy, 512 row groups on 52 ten-wave workgroups (the last one has idle waves).
  * (2048, 5632, 1, 16, 16, -777, 160), L2_SMALL_MAX=0: four batches; one layer, the hard case for the hand-off tags.
  * llama2_7b_L2: the flagship's width, eight batches (a wave holds 128 VGPRs of weights).
"""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from llama2_ts_amd import configs, runtime

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-4            # north_star: logits within 1e-4 fp32 (test_hip_parity.py)
RANGE_END = 256       # cached rows up to which the step takes the fused launch (csrc/llama2_hip.hip: kAwoStreamRows)

SMALL = {
    "d1024": ((1024, 2816, 2, 8, 8, -1000, 300), {"L2_SMALL_MAX": "0", "L2_TUNE_U": "2", "L2_TUNE_NWAVES": "2"}, 11),
    "d2048": ((2048, 5632, 1, 16, 16, -777, 160), {"L2_SMALL_MAX": "0"}, 12),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def upload_from_oracle(ctx, orc):
    for kind, layers, count in runtime.tensor_shapes(ctx.cfg):
        for layer in range(max(layers, 1)):
            a = orc.weights(kind, layer if layers else -1)
            assert a.size == count
            ctx.upload(kind, layer if layers else -1, a)


def new_ctx(hdr, env, orc=None, seed=None):
    """A context created under `env` (the library reads its development switches when a context is created)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = runtime.Context(hdr)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if orc is not None:
        upload_from_oracle(ctx, orc)
    else:
        ctx.synth_fill(seed)
    return ctx


def pair(hdr, env, orc=None, seed=None):
    base = dict(env, L2_ATTN_SPLIT_ROWS=str(RANGE_END))
    fused = new_ctx(hdr, base, orc, seed)
    plain = new_ctx(hdr, dict(base, L2_ATTN_WO_STREAM="0"), orc, seed)
    for c in (fused, plain):
        c.set_option(runtime.OPT_KEEP_STATE, 1)
    return fused, plain


def check_step(fused, plain, tok, pos, where):
    """One position through both contexts: logits, xb, xb2, att bit for bit; which path each took.  Returns the logits."""
    a = np.array(fused.forward(tok, pos), copy=True)
    b = np.array(plain.forward(tok, pos), copy=True)
    assert same_bits(a, b), (where, pos, "logits", float(np.abs(a - b).max()))
    for nm in ("xb", "xb2", "att"):
        assert same_bits(fused.read_state(nm), plain.read_state(nm)), (where, pos, nm)
    assert fused.get_option(runtime.OPT_ATTN_WO_STREAM) == (1 if pos + 1 <= RANGE_END else 0), (where, pos)
    assert plain.get_option(runtime.OPT_ATTN_WO_STREAM) == 0, (where, pos)
    return a


def check_caches(fused, plain, where):
    for nm in ("key_cache", "value_cache"):
        assert same_bits(fused.read_state(nm), plain.read_state(nm)), (where, nm)


@pytest.fixture(scope="module")
def small():
    """Per small shape: the oracle, the fused and the plain context, fed every position once (shared by the tests below)."""
    made = {}

    def get(name):
        if name not in made:
            hdr, env, seed = SMALL[name]
            orc = O.Oracle(hdr, seed)
            fused, plain = pair(hdr, env, orc=orc)
            made[name] = (orc, fused, plain)
        return made[name]
    yield get
    for orc, fused, plain in made.values():
        fused.close(); plain.close(); orc.close()


@pytest.mark.parametrize("name", list(SMALL))
def test_every_position_bit_for_bit_and_within_the_oracle(small, name):
    """Every position 0 .. S - 1 through forward: one tile round, the second (beyond 128 rows), the end of the fused range (256 rows) and
    the two launches with 8 splits behind it."""
    hdr = SMALL[name][0]
    orc, fused, plain = small(name)
    S = hdr[6]
    tok, worst = 1, 0.0
    for pos in range(S):
        got = check_step(fused, plain, tok, pos, name)
        want = orc.forward(tok, pos)
        err = float(np.abs(got - want).max())
        worst = max(worst, err)
        assert err <= TOL, (name, pos, err)
        assert runtime.argmax(got) == O.argmax(want), (name, pos)
        tok = runtime.argmax(got)
    check_caches(fused, plain, name)
    print("\n[%s] %d positions bit for bit, max|dlogit| vs the oracle %.3g" % (name, S, worst))


def test_7b_width_bit_for_bit():
    """llama2_7b_L2: the first 40 positions, then 120 - 150 and 250 - 262 (both sides of the fused range's end), the positions in between
    fed by the device loop."""
    meta = json.load(open(os.path.join(GOLD, "llama2_7b_L2.json")))
    fused, plain = pair(meta["header"], {}, seed=meta["seed"])
    fed, want = meta["tokens_fed"], meta["argmax"]
    pos = 0
    for lo, hi in ((0, 40), (120, 151), (250, 263)):
        if lo > pos:
            ta, tb = fused.decode_greedy(fed[pos], pos, lo - pos).tolist(), plain.decode_greedy(fed[pos], pos, lo - pos).tolist()
            assert ta == tb == want[pos:lo], (pos, lo)
        for p in range(lo, hi):
            got = check_step(fused, plain, fed[p], p, "llama2_7b_L2")
            assert runtime.argmax(got) == want[p], p
        pos = hi
    check_caches(fused, plain, "llama2_7b_L2")
    fused.close(); plain.close()


@pytest.mark.parametrize("name", list(SMALL))
def test_tags_are_fresh_in_every_run_and_every_call(small, name):
    """The hand-off tags come from {run nonce, pos, layer}: a second run over the same positions, and one position fed twice in a row, must
    not be served granules of the launch before (the one-layer shape has nothing but the nonce to tell two calls apart)."""
    hdr = SMALL[name][0]
    _, fused, plain = small(name)
    S = hdr[6]
    want = plain.decode_greedy(1, 0, S).tolist()
    for queue in (1, 0):      # the library's own queue, then replayed hipGraphs
        fused.set_option(runtime.OPT_AQL_QUEUE, queue)
        first = fused.decode_greedy(1, 0, S).tolist()
        assert fused.get_option(runtime.OPT_AQL_QUEUE) == queue
        assert fused.get_option(runtime.OPT_ATTN_WO_STREAM) == 1
        again = fused.decode_greedy(1, 0, S).tolist()
        assert first == want and again == want, (name, queue)
        # one position twice in a row, different tokens
        pos, other = 7, (want[6] + 1) % abs(hdr[5])
        a1 = np.array(fused.forward(want[pos - 1], pos), copy=True)
        a2 = np.array(fused.forward(other, pos), copy=True)
        b2 = np.array(plain.forward(other, pos), copy=True)
        assert same_bits(a2, b2), (name, queue)
        assert not same_bits(a1, a2), (name, queue)
        fused.forward(want[pos - 1], pos); plain.forward(want[pos - 1], pos)      # (the row of the greedy stream back in both caches)
    fused.set_option(runtime.OPT_AQL_QUEUE, 1)
    assert plain.get_option(runtime.OPT_ATTN_WO_STREAM) == 0


@pytest.mark.parametrize("how", ["L2_PACKED=0", "exact", "L2_ATTN_SPLITS=8"])
def test_fallbacks_keep_the_two_launches(small, how):
    """No repacked copy, the reference's own value accumulate, a forced split count: the step is the two launches, its tokens the plain context's."""
    hdr, env, seed = SMALL["d1024"]
    orc, _, plain = small("d1024")
    extra = {} if how == "exact" else dict([how.split("=")])
    ctx = new_ctx(hdr, dict(env, **extra), orc=orc)
    if how == "exact":
        ctx.set_option(runtime.OPT_EXACT_ATTENTION, 1)
    want = plain.decode_greedy(1, 0, 8).tolist()
    assert ctx.decode_greedy(1, 0, 8).tolist() == want, how
    assert ctx.get_option(runtime.OPT_ATTN_WO_STREAM) == 0, how
    ctx.forward(1, 0)
    assert ctx.get_option(runtime.OPT_ATTN_WO_STREAM) == 0, how
    ctx.close()


def test_every_cu_holding_stale_lines_changes_nothing():
    """The coherence rule's adversary (L2_DEBUG_POLLUTE=1: every CU pulls every mutable line, the granules among them, into its L1 behind
    every launch) on the library's own queue against replayed hipGraphs without it: llama2_7b_L2, 24 tokens."""
    meta = json.load(open(os.path.join(GOLD, "llama2_7b_L2.json")))
    ref = new_ctx(meta["header"], {}, seed=meta["seed"])
    ref.set_option(runtime.OPT_AQL_QUEUE, 0)
    want = ref.decode_greedy(1, 0, 24).tolist()
    assert ref.get_option(runtime.OPT_ATTN_WO_STREAM) == 1
    ref.close()
    adv = new_ctx(meta["header"], {"L2_DEBUG_POLLUTE": "1"}, seed=meta["seed"])
    got = adv.decode_greedy(1, 0, 24).tolist()
    assert adv.get_option(runtime.OPT_AQL_QUEUE) == 1, "the library's own queue was not in use: this run did not test the no-acquire dispatch"
    assert adv.get_option(runtime.OPT_ATTN_WO_STREAM) == 1
    adv.close()
    assert got == want == meta["argmax"][:24]
