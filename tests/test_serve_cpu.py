"""The continuous-batching scheduler (llama2_ts_amd.serve) driven by a pure-Python stand-in for runtime.Context.step_batch.

The stand-in picks each row's token by hashing its sequence's whole fed history (so a pick depends on what was fed where, not on how
it was chunked) and draws from a Python xorshift* (llama2.ts:348-355) only when the row's temperature is not 0.  Each request's result
must equal the same request run alone through a plain transcription of llama2.ts:462-500 on a fresh stand-in."""
import hashlib
import types

import numpy as np
import pytest

from llama2_ts_amd import runtime, serve

MASK = (1 << 64) - 1
V = 29          # small: BOS (1) comes up now and then


def xorshift_u32(state):
    state ^= state >> 12
    state ^= (state << 25) & MASK
    state ^= state >> 27
    return state, ((state * 0x2545F4914F6CDD1D) >> 32) & 0xFFFFFFFF


class StubContext:
    """step_batch's contract on the host: caches are per-sequence token histories, logits a one-hot of the pick."""

    def __init__(self, slots, seq_len):
        self.slots, self.cfg = slots, types.SimpleNamespace(seq_len=seq_len, vocab_size=V)
        self.hist = [[] for _ in range(slots)]
        self.calls = self.rows = self.draws = self.starts = 0
        self.max_rows_seen = 0

    def get_option(self, key):
        assert key == runtime.OPT_SEQS
        return self.slots

    def step_batch(self, seqs, runs, pos0, temperature=0.0, topp=1.0, rng=None, logits=False):
        n = len(seqs)
        assert len(set(seqs)) == n, "a sequence twice in one call"
        assert len(runs) == n and len(pos0) == n
        temp = list(np.broadcast_to(np.asarray(temperature, dtype=np.float64), (n,)))
        rows = sum(len(r) for r in runs)
        self.calls += 1
        self.rows += rows
        self.max_rows_seen = max(self.max_rows_seen, rows)
        picks, after, lg = [], [], np.zeros((n, V), dtype=np.float32)
        for i, s in enumerate(seqs):
            assert 0 <= s < self.slots and len(runs[i]) >= 1
            h = self.hist[s]
            if pos0[i] == 0:
                del h[:]
                self.starts += 1
            assert pos0[i] == len(h), "sequence %d fed at %d, %d rows written" % (s, pos0[i], len(h))
            h.extend(int(t) for t in runs[i])
            assert len(h) <= self.cfg.seq_len
            key = int.from_bytes(hashlib.sha256(np.asarray(h, dtype=np.int64).tobytes()).digest()[:8], "little")
            st = None if rng is None else int(rng[i])
            if temp[i] != 0.0:
                st, u = xorshift_u32(st)
                self.draws += 1
                key ^= u
            tok = key % V
            picks.append(tok)
            after.append(st)
            lg[i, tok] = 1.0
        return (picks, after, lg) if logits else (picks, after)


def reference_loop(ctx, seq, prompt, steps, temperature, seed):
    """llama2.ts:462-500 for one request: BOS at pos 0, the prompt forced, then a pick per position; stop at steps or at BOS."""
    token, pos, fed, rng, finish = 1, 0, [], seed, "steps"
    while pos < steps:
        fed.append(token)
        if pos < len(prompt):
            ctx.step_batch([seq], [[token]], [pos], 0.0, 1.0, [rng])       # transformer(); the prompt token is forced
            nxt = prompt[pos]
        else:
            picks, after = ctx.step_batch([seq], [[token]], [pos], temperature, 0.9, [rng])
            nxt, rng = picks[0], after[0] if temperature != 0.0 else rng
        pos += 1
        if nxt == 1:
            finish = "bos"
            break
        token = nxt
    return fed, finish, rng


def random_requests(rng, k, seq_len, max_prompt=40):
    reqs = []
    for _ in range(k):
        p = [int(t) for t in rng.integers(2, V, int(rng.integers(0, max_prompt)))]
        steps = int(rng.integers(0, seq_len + 1))
        temp = 0.0 if rng.random() < 0.4 else 0.9
        reqs.append((p, steps, temp, int(rng.integers(1, 1 << 62))))
    return reqs


def check_against_reference(reqs, results, seq_len):
    draws = 0
    for rid, (p, steps, temp, seed) in enumerate(reqs):
        ref = StubContext(1, seq_len)
        fed, finish, st = reference_loop(ref, 0, p, steps, temp, seed)
        draws += ref.draws
        got = results[rid]
        assert got.tokens_fed == fed, rid
        assert got.finish == finish, rid
        assert got.rng_state == st, rid
    return draws


@pytest.mark.parametrize("slots,max_rows,seed", [(4, 4, 0), (4, 9, 1), (8, 24, 2), (3, 64, 3), (16, 16, 4)])
def test_each_request_runs_the_reference_loop(slots, max_rows, seed):
    seq_len = 64
    rng = np.random.default_rng(seed)
    reqs = random_requests(rng, 40, seq_len)
    ctx = StubContext(slots, seq_len)
    s = serve.Scheduler(ctx, max_rows=max_rows)
    for p, steps, temp, sd in reqs:
        s.submit(p, steps, temperature=temp, topp=0.9, seed=sd)
    results = s.run()
    assert sorted(results) == list(range(len(reqs)))
    draws = check_against_reference(reqs, results, seq_len)
    assert ctx.draws == draws, "one draw per sampled token"
    assert ctx.max_rows_seen <= max_rows
    assert ctx.starts == sum(1 for _, steps, _, _ in reqs if steps > 0), "every request starts its slot at 0 exactly once"
    assert {r.finish for r in results.values()} == {"bos", "steps"}
    assert ctx.calls == s.calls and s.idle


def test_edge_cases():
    seq_len = 32
    reqs = [([5, 6, 7, 8, 9], 3, 0.0, 1),            # steps <= len(prompt): feeds 3 tokens, never draws
            ([5, 6, 7, 8, 9], 5, 0.9, 2),            # steps == len(prompt)
            ([5, 6, 7, 8, 9], 6, 0.9, 3),            # one pick
            ([], seq_len, 0.9, 4),                   # steps == seq_len, no prompt
            ([3] * 30, seq_len, 0.0, 5),             # a prompt longer than max_rows
            ([4, 5, 1, 7], 20, 0.9, 6),              # a BOS inside the prompt ends the loop there
            ([2, 3], 0, 0.9, 7)]                     # steps 0: nothing fed
    ctx = StubContext(3, seq_len)
    s = serve.Scheduler(ctx, max_rows=8)
    for p, steps, temp, sd in reqs:
        s.submit(p, steps, temperature=temp, topp=0.9, seed=sd)
    results = s.run()
    draws = check_against_reference(reqs, results, seq_len)
    assert ctx.draws == draws
    assert results[0].tokens_fed == [1, 5, 6] and results[0].rng_state == 1
    assert results[1].tokens_fed == [1, 5, 6, 7, 8] and results[1].rng_state == 2
    assert results[5].tokens_fed == [1, 4, 5] and results[5].finish == "bos" and results[5].rng_state == 6
    assert results[6].tokens_fed == [] and results[6].finish == "steps"
    assert ctx.max_rows_seen <= 8


def test_bos_pick_stops_and_is_not_fed():
    seq_len = 200
    ctx = StubContext(2, seq_len)
    s = serve.Scheduler(ctx, max_rows=2)
    rids = [s.submit([], seq_len, temperature=0.9, seed=sd) for sd in range(1, 9)]
    results = s.run()
    bos = [results[r] for r in rids if results[r].finish == "bos"]
    assert bos, "no request met BOS"
    for r in bos:
        assert 1 not in r.tokens_fed[1:] and len(r.tokens_fed) < seq_len


def test_submissions_between_steps_and_keep_logits():
    seq_len = 48
    rng = np.random.default_rng(11)
    reqs = random_requests(rng, 24, seq_len)
    ctx = StubContext(5, seq_len)
    s = serve.Scheduler(ctx, max_rows=12, keep_logits=True)
    pending = list(reqs)
    finished = {}
    while pending or not s.idle:
        for _ in range(int(rng.integers(0, 4))):
            if pending:
                p, steps, temp, sd = pending.pop(0)
                s.submit(p, steps, temperature=temp, topp=0.9, seed=sd)
        got = s.step()
        assert not set(got) & set(finished)
        finished.update(got)
    assert finished == s.results and len(finished) == len(reqs)
    check_against_reference(reqs, finished, seq_len)
    for rid, (p, steps, _, _) in enumerate(reqs):
        r = finished[rid]
        P = len(p)
        picks = [int(np.argmax(row)) for row in r.logits]
        assert len(picks) == max(0, len(r.tokens_fed) - P)
        assert picks[:-1] == r.tokens_fed[P + 1:] if picks else True


def test_deterministic_and_rules():
    seq_len = 40
    reqs = random_requests(np.random.default_rng(7), 20, seq_len)
    outs = []
    for _ in range(2):
        ctx = StubContext(4, seq_len)
        s = serve.Scheduler(ctx, max_rows=10)
        for p, steps, temp, sd in reqs:
            s.submit(p, steps, temperature=temp, topp=0.9, seed=sd)
        res = s.run()
        outs.append(([(r.tokens_fed, r.finish, r.rng_state) for _, r in sorted(res.items())], ctx.calls, ctx.rows))
    assert outs[0] == outs[1]
    with pytest.raises(ValueError):
        serve.Scheduler(StubContext(4, seq_len), max_rows=3)
    with pytest.raises(ValueError):
        serve.Scheduler(StubContext(4, seq_len)).submit([2], seq_len + 1)
