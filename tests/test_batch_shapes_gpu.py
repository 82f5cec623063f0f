"""The prompt / batch kernels over the shapes of tests/batch_shapes.py (head sizes 4 .. 256, both GEMM families, both attention forms, the
repacked weights), every leg against the C oracle run token by token per sequence (tests/oracle_lib.py) and against l2_forward on a second
context.  The calls of every leg are DATA (batch_shapes.leg_calls); tests/test_batch_plan_cpu.py proves on the CPU that they reach every
instance of the prompt / batch kernel families.  Bars, all the project's own:
  logits   within 1e-4 of the oracle; argmax equal wherever the oracle's top-two gap exceeds 2e-4; within 1e-5 of l2_forward
  caches   every written row of every layer within 1e-4 of the oracle's and within 1e-6 of the l2_forward context's
  bits     layer-0 key / value rows depend on embedding -> rmsnorm -> GEMM -> RoPE only, where DESIGN.md section 2 gives the GPU and the
           oracle the same rounding points: >= 99.9 % of the written elements bit-identical to the oracle's, the rest within 1e-6
  contracts  after EVERY call, rows below pos0 of every continued (or forked) sequence and every sequence it did not name keep their bytes; l2_seq_score_batch leaves the caches
           bit for bit as l2_seq_prefill_batch does
L2_OPT_PREFILL_F32_MFMA legs (fp32 accumulate, not the reference's arithmetic) are held to the oracle bars only."""
import functools

import numpy as np
import pytest

import batch_shapes as B
import oracle_lib as O
from llama2_ts_amd import runtime

TOL, TOL_FWD, TOL_CACHE_FWD, TOL_LP, GAP = 1e-4, 1e-5, 1e-6, 2e-4, 2e-4
BIT_SHARE, BIT_REST = 0.999, 1e-6


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The oracle over every token stream of a shape: logits [stream][pos][V], caches [stream][L][S][d].  CPU only."""
    hdr = B.SHAPES[name]
    d, L, S = hdr[0], hdr[2], hdr[6]
    toks = B.streams(name)
    orc = O.Oracle(hdr, B.SEED)
    logits = np.empty((B.N_STREAMS, S, orc.V), dtype=np.float32)
    kc = np.empty((B.N_STREAMS, L, S, d), dtype=np.float32)
    vc = np.empty_like(kc)
    for s in range(B.N_STREAMS):
        for p in range(S):
            logits[s, p] = orc.forward(int(toks[s, p]), p)
        kc[s] = orc.state("key_cache").reshape(L, S, d)
        vc[s] = orc.state("value_cache").reshape(L, S, d)
    orc.close()
    for a in (logits, kc, vc):
        a.setflags(write=False)
    l64 = logits.astype(np.float64)
    lsm = l64 - (np.log(np.exp(l64 - l64.max(axis=2, keepdims=True)).sum(axis=2, keepdims=True)) + l64.max(axis=2, keepdims=True))
    top2 = np.sort(logits, axis=2)[:, :, -2:]
    return {"logits": logits, "key_cache": kc, "value_cache": vc, "lsm": lsm, "clear": (top2[:, :, 1] - top2[:, :, 0]) > GAP,
            "argmax": logits.argmax(axis=2)}


@functools.lru_cache(maxsize=None)
def forward_run(name, exact=0):
    """The same streams through l2_forward, one sequence at a time, on a context of its own."""
    hdr = B.SHAPES[name]
    d, L, S = hdr[0], hdr[2], hdr[6]
    toks = B.streams(name)
    ctx = runtime.Context(hdr)
    ctx.synth_fill(B.SEED)
    if exact:
        ctx.set_option(runtime.OPT_EXACT_ATTENTION, 1)
    logits = np.empty((B.N_STREAMS, S, ctx.cfg.vocab_size), dtype=np.float32)
    kc = np.empty((B.N_STREAMS, L, S, d), dtype=np.float32)
    vc = np.empty_like(kc)
    for s in range(B.N_STREAMS):
        for p in range(S):
            ctx.forward(int(toks[s, p]), p, out=logits[s, p])
        kc[s] = ctx.read_state("key_cache").reshape(L, S, d)
        vc[s] = ctx.read_state("value_cache").reshape(L, S, d)
    ctx.close()
    return {"logits": logits, "key_cache": kc, "value_cache": vc}


def caches(ctx, s, hdr):
    d, L, S = hdr[0], hdr[2], hdr[6]
    return {n: ctx.read_seq_cache(s, n).reshape(L, S, d) for n in ("key_cache", "value_cache")}


class Leg:
    """Runs the calls of one leg on a fresh context and holds every result to the bars."""

    def __init__(self, name, leg, kinds=None):
        self.name, self.leg, self.hdr = name, leg, B.SHAPES[name]
        self.calls = B.leg_calls(name, leg)
        self.opts = {k: v for c in self.calls for k, v in c["opts"].items()}
        self.f32, self.exact = bool(self.opts.get("f32")), bool(self.opts.get("exact"))
        self.ref = oracle_run(name)
        self.fwd = None if self.f32 else forward_run(name, int(self.exact))
        self.toks = B.streams(name)
        self.kinds = kinds or {}
        self.ctx = runtime.Context(self.hdr)
        self.ctx.synth_fill(B.SEED)
        self.ctx.seq_reserve(B.N_SEQS)
        if self.exact:
            self.ctx.set_option(runtime.OPT_EXACT_ATTENTION, 1)
        if self.f32:
            self.ctx.set_option(runtime.OPT_PREFILL_F32_MFMA, 1)
        self.end = {}                      # sequence -> rows written
        self.d_orc = self.d_fwd = 0.0
        self.weight_mib = None
        self.snap = None                   # every sequence's caches after the last call

    def run_tokens(self, s, pos0, n):
        return self.toks[s % B.N_STREAMS, pos0:pos0 + n]

    def check_logits(self, got, s, pos, what):
        st = s % B.N_STREAMS
        want = self.ref["logits"][st, pos]
        e = float(np.abs(got - want).max())
        self.d_orc = max(self.d_orc, e)
        assert e <= TOL, (self.name, self.leg, what, s, pos, e)
        if self.ref["clear"][st, pos]:
            assert int(np.argmax(got)) == int(self.ref["argmax"][st, pos]), (self.name, self.leg, what, s, pos, "argmax")
        if self.fwd is not None:
            e = float(np.abs(got - self.fwd["logits"][st, pos]).max())
            self.d_fwd = max(self.d_fwd, e)
            assert e <= TOL_FWD, (self.name, self.leg, what, s, pos, e, "against l2_forward")

    def check_score(self, call, res):
        lp, am, ids, tlp = res
        r = 0
        for s, pos0, n in call["runs"]:
            st = s % B.N_STREAMS
            for k in range(n):
                pos = pos0 + k
                lsm = self.ref["lsm"][st, pos]
                if k + 1 < n:
                    tgt = int(self.toks[st, pos + 1])
                    e = abs(float(lp[r]) - float(lsm[tgt]))
                    self.d_orc = max(self.d_orc, e)
                    assert e <= TOL_LP, (self.name, "score lp", s, pos, e)
                else:
                    assert np.isnan(lp[r]), (self.name, "score: a target of -1 gives NaN", s, pos)
                if self.ref["clear"][st, pos]:
                    assert int(am[r]) == int(self.ref["argmax"][st, pos]) == int(ids[r, 0]), (self.name, "score argmax", s, pos)
                want = np.sort(lsm)[::-1][:3]
                assert np.abs(tlp[r] - want).max() <= TOL_LP, (self.name, "score top lps", s, pos)
                assert np.abs(tlp[r] - lsm[ids[r]]).max() <= TOL_LP and len(set(ids[r].tolist())) == 3, (self.name, "score top ids", s, pos)
                r += 1
        assert r == lp.size

    def run_call(self, call):
        ctx, kind, runs = self.ctx, self.kinds.get(call["kind"], call["kind"]), call["runs"]
        if self.snap is None:
            self.snap = self.snapshot()
        before = self.snap
        seqs, pos0 = [s for s, _, _ in runs], [p for _, p, _ in runs]
        toks = [self.run_tokens(*r) for r in runs]
        if kind == "decode_step":
            (s, p0, n), = runs
            self.check_logits(ctx.forward(int(toks[0][0]), p0), s, p0, kind)
            assert ctx.get_option(runtime.OPT_PACKED_MIB) > 0, "the shape was meant to repack its weights"
            self.weight_mib = ctx.get_option(runtime.OPT_WEIGHT_MIB)
        elif kind == "forward_batch":
            lg = ctx.forward_batch(seqs, [int(t[0]) for t in toks], pos0)
            for i, (s, p0, n) in enumerate(runs):
                self.check_logits(lg[i], s, p0, kind)
        elif kind == "prefill_batch":
            lg = ctx.seq_prefill_batch(seqs, toks, pos0)
            for i, (s, p0, n) in enumerate(runs):
                self.check_logits(lg[i], s, p0 + n - 1, kind)
        elif kind == "score":
            self.check_score(call, ctx.seq_score_batch(seqs, toks, pos0, top_k=3))
        elif kind == "step_batch":
            picks, _, lg = ctx.step_batch(seqs, toks, pos0, logits=True)
            for i, (s, p0, n) in enumerate(runs):
                self.check_logits(lg[i], s, p0 + n - 1, kind)
                assert picks[i] == int(np.argmax(lg[i])) or not self.ref["clear"][s % B.N_STREAMS, p0 + n - 1], (self.name, kind, s, "pick")
        elif kind == "fork":      # rows 0 .. n-1 of the source, byte for byte, and a sequence that continues there
            (s, p0, n), = runs
            ctx.seq_fork(call["src"], [s], n)
            src, dst = caches(ctx, call["src"], self.hdr), caches(ctx, s, self.hdr)
            assert all(dst[k][:, :n].tobytes() == src[k][:, :n].tobytes() for k in dst), (self.name, self.leg, "fork", s)
        elif kind == "prefill":
            (s, p0, n), = runs
            lg = ctx.prefill(toks[0], p0) if s == 0 else ctx.seq_prefill(s, toks[0], p0)
            self.check_logits(lg, s, p0 + n - 1, kind)
        else:
            raise KeyError(kind)
        for s, p0, n in runs:
            self.end[s] = max(self.end.get(s, 0), p0 + n)
        # every sequence the call did not name keeps its bytes; so do the rows below pos0 of every one it continued
        after = self.snap = self.snapshot()
        first = {s: p0 for s, p0, _ in runs}
        for s in range(B.N_SEQS):
            for name in after[s]:
                keep = first.get(s, self.hdr[6])
                assert after[s][name][:, :keep].tobytes() == before[s][name][:, :keep].tobytes(), \
                    (self.name, self.leg, kind, "rows the call had no business with changed", s, name, keep)

    def snapshot(self):
        return [caches(self.ctx, s, self.hdr) for s in range(B.N_SEQS)]

    def finish(self):
        """Every written cache row against the oracle and l2_forward, the layer-0 rows bit for bit; sequences no call named still as reserved."""
        same = total = 0
        rest = d_co = d_cf = 0.0
        for s in range(B.N_SEQS):
            got = caches(self.ctx, s, self.hdr)
            n, st = self.end.get(s, 0), s % B.N_STREAMS
            for name, a in got.items():
                if n == 0:
                    assert not a.any(), (self.name, self.leg, s, name, "a sequence no call named is not as reserved")
                    continue
                want = self.ref[name][st][:, :n]
                d_co = max(d_co, float(np.abs(a[:, :n] - want).max()))
                if self.fwd is not None:
                    d_cf = max(d_cf, float(np.abs(a[:, :n] - self.fwd[name][st][:, :n]).max()))
                    eq = a[0, :n].view(np.uint32) == want[0].view(np.uint32)
                    same += int(eq.sum()); total += eq.size
                    if not eq.all():
                        rest = max(rest, float(np.abs(a[0, :n] - want[0])[~eq].max()))
        share = same / total if total else float("nan")
        print("\nSWEEP %-12s %-14s rows %4d  max|dlogit| oracle %.3g  l2_forward %.3g  cache oracle %.3g  l2_forward %.3g  layer-0 bit-identical %.6f (%d of %d, rest <= %.3g)"
              % (self.name, self.leg, sum(self.end.values()), self.d_orc, self.d_fwd, d_co, d_cf, share, same, total, rest))
        assert d_co <= TOL, (self.name, self.leg, "caches against the oracle", d_co)
        if self.fwd is not None:
            assert d_cf <= TOL_CACHE_FWD, (self.name, self.leg, "caches against l2_forward", d_cf)
            assert share >= BIT_SHARE and rest <= BIT_REST, (self.name, self.leg, "layer-0 rows against the oracle, bit level", share, rest)
        if self.weight_mib is not None:
            assert self.ctx.get_option(runtime.OPT_WEIGHT_MIB) <= self.weight_mib, "the batch calls brought row-major weights back"
            assert self.ctx.get_option(runtime.OPT_PACKED_MIB) > 0

    def run(self, keep=False):
        """Every call, then the caches.  The context is closed unless `keep` is set and everything passed."""
        try:
            for call in self.calls:
                self.run_call(call)
            self.finish()
        except BaseException:
            self.ctx.close()
            raise
        if not keep:
            self.ctx.close()
        return self


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(B.SHAPES))
@pytest.mark.parametrize("leg", [leg for leg in B.LEGS if leg != "score"])
def test_leg_against_the_oracle_and_l2_forward(name, leg):
    """forward_batch: 1, 16, 17, 32, 33 and 64 rows at different positions in shuffled order, a sequence joining late.  prefill_batch: ragged
    runs (1, 3, 15, 16, 17, 31 and longer, every tile size 1 .. 16) of 63 / 64 / 65 / 129 / 193 / 257 rows in all, continuing the sequences
    of the calls before.  prefill_one: l2_prefill and l2_seq_prefill of 2, 17, 33, 65 tokens and the whole context, continuations at
    positions 2 and 17.  step_batch: decode rows at positions 13 .. 18 beside prompt runs that cross the launch-sequence boundary, and a
    sequence forked from another (l2_seq_fork) that continues at the fork point."""
    Leg(name, leg).run()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(B.SHAPES))
def test_score_leg_and_its_caches_equal_prefill_batch(name):
    """l2_seq_score_batch with top_k = 3 over the packing of the prefill_batch leg: lps and top lps against a numpy fp64 log-softmax of
    the oracle's logits at 2e-4; and every cache byte as l2_seq_prefill_batch with the same arguments leaves it."""
    score = Leg(name, "score").run(keep=True)
    fill = None
    try:
        fill = Leg(name, "score", kinds={"score": "prefill_batch"})
        for call in fill.calls:
            fill.run_call(call)
        for s in range(B.N_SEQS):
            a, b = caches(score.ctx, s, score.hdr), caches(fill.ctx, s, fill.hdr)
            assert all(a[n].tobytes() == b[n].tobytes() for n in a), (name, s, "scoring and prefill leave different caches")
    finally:
        score.ctx.close()
        if fill is not None:
            fill.ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,leg", [(n, "exact") for n in B.EXACT_SHAPES] + [(n, "f32") for n in B.F32_SHAPES])
def test_option_leg(name, leg):
    """L2_OPT_EXACT_ATTENTION: the plan says rows-form attention for every launch sequence, and every bar holds (l2_forward under the same
    option).  L2_OPT_PREFILL_F32_MFMA at 64, 128 and 256 rows: logits and caches within 1e-4 of the oracle."""
    if leg == "exact":
        for call in B.leg_calls(name, leg):
            for _q, p, _i in B.plans_of(B.SHAPES[name], call):
                assert p["attn"] and all(a["family"] in (B.AT_PF_TILE, B.AT_BT_TILE) for a in p["attn"]), (name, p["attn"])
    Leg(name, leg).run()
