"""The continuous-batching scheduler (llama2_ts_amd.serve) on the device: golden runs of the REAL reference's CLI, mixed with random
requests and submitted at different steps, come out token for token; sampled requests' picks are the oracle's sampler fed the logits
each pick was made from, with the request's own rng."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from llama2_ts_amd import runtime, serve
from test_cli_gpu import reference_run

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def golden_request(name):
    """(prompt ids, steps, temperature, topp, seed, tokens_fed) of a golden run of the reference."""
    meta = json.load(open(os.path.join(GOLD, name + ".json")))
    flags = dict(zip(meta["argv"][::2], meta["argv"][1::2]))
    fed, picks = meta["tokens_fed"], meta["argmax"]
    if name == "stories15M_prompt":      # reference tokenizer: the forced positions are those the greedy picks do not explain
        P = next(p for p in range(len(fed) - 1) if all(fed[q + 1] == picks[q] for q in range(p, len(fed) - 1)))
        prompt = fed[1:P + 1]
    else:
        _, prompt, _ = reference_run(name)
    steps = min(int(flags["-n"]), meta["header"][6])
    return prompt, steps, float(flags.get("-t", "1.0")), float(flags.get("-p", "1.0")), int(flags.get("-s", "1")), fed


def test_golden_requests_mixed_with_random_ones():
    names = ["cli_greedy", "cli_prompt", "cli_temp", "cli_topp", "stories15M_prompt"]
    gold = {n: golden_request(n) for n in names}
    meta = json.load(open(os.path.join(GOLD, "cli_greedy.json")))
    hdr = meta["header"]
    assert all(json.load(open(os.path.join(GOLD, n + ".json")))["header"] == hdr for n in names)
    rng = np.random.default_rng(17)
    extra = []
    for _ in range(20):
        p = [int(t) for t in rng.integers(3, hdr[5], int(rng.integers(0, 60)))]
        extra.append((p, int(rng.integers(8, 120)), [0.0, 0.9][int(rng.integers(0, 2))], 0.9, int(rng.integers(1, 1 << 40))))
    order = [("x", e) for e in extra[:6]] + [("g", n) for n in names[:2]] + [("x", e) for e in extra[6:14]] + \
            [("g", n) for n in names[2:]] + [("x", e) for e in extra[14:]]
    ctx = runtime.Context(hdr)
    ctx.synth_fill(meta["seed"])
    ctx.seq_reserve(8)
    s = serve.Scheduler(ctx, max_rows=24)
    rid_of = {}
    k = 0
    while k < len(order) or not s.idle:
        for _ in range(3 if k < 10 else 1):      # a burst, then one submission per step
            if k < len(order):
                kind, what = order[k]
                if kind == "g":
                    p, steps, t, tp, sd, _ = gold[what]
                    rid_of[what] = s.submit(p, steps, temperature=t, topp=tp, seed=sd)
                else:
                    s.submit(*what[:2], temperature=what[2], topp=what[3], seed=what[4])
                k += 1
        s.step()
    res = s.results
    assert len(res) == len(order)
    for n in names:
        r = res[rid_of[n]]
        assert r.tokens_fed == gold[n][5], n
        assert r.finish == "steps", n
    ctx.close()


def test_sampled_picks_are_the_oracle_sampler_on_the_kept_logits():
    meta = json.load(open(os.path.join(GOLD, "stories110M.json")))
    hdr = meta["header"]
    rng = np.random.default_rng(23)
    ctx = runtime.Context(hdr)
    ctx.synth_fill(meta["seed"])
    ctx.seq_reserve(16)
    s = serve.Scheduler(ctx, max_rows=64, keep_logits=True)
    reqs = {}
    for _ in range(40):
        p = [int(t) for t in rng.integers(3, hdr[5], int(rng.integers(0, 80)))]
        t = [0.0, 0.9, 1.0, 0.5][int(rng.integers(0, 4))]
        tp = [1.0, 0.9, 0.5][int(rng.integers(0, 3))]
        sd = int(rng.integers(1, 1 << 50))
        steps = len(p) + 1 + int(rng.integers(1, 40))
        reqs[s.submit(p, steps, temperature=t, topp=tp, seed=sd)] = (p, steps, t, tp, sd)
    res = s.run()
    for rid, (p, steps, t, tp, sd) in reqs.items():
        r = res[rid]
        P = len(p)
        assert r.tokens_fed[:P + 1] == [1] + p
        assert len(r.logits) == len(r.tokens_fed) - P
        st = O.Rng(sd)
        for j, lg in enumerate(r.logits):
            want = O.next_token(lg, t, tp, st)[0] if t != 0.0 else O.argmax(lg)
            if j + 1 < len(r.logits):
                assert r.tokens_fed[P + 1 + j] == want, (rid, j)
            else:
                assert (r.finish == "bos") == (want == 1), rid
                if r.finish == "steps":
                    assert len(r.tokens_fed) == steps
        assert r.rng_state == int(st.state.value), rid
    ctx.close()
