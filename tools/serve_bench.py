"""Continuous batching (llama2_ts_amd.serve over l2_step_batch) against static batching with the existing calls, one process, synthetic
weights (l2_synth_fill, the golden's seed).

Workload (seeded): --requests requests, all submitted at once; prompts of 8-128 random tokens and generations of 16-256 tokens, both
uniform; half greedy, half at temperature 0.9 / top-p 0.9.  For every slot count in --slots:
  static     groups of `slots` requests in order: l2_seq_prefill_batch of [1] + prompt[:-1], then l2_decode_sample_batch from prompt[-1]
             for the group's longest generation; each row is cut at its own length or at BOS.
  continuous serve.Scheduler with each --max-rows value (>= slots).
Reported per form: generated tok/s, time to first token and per-token latency (median, p99; host clock -- the static form sees a token
when its call returns), steps and the histogram of rows per step (continuous), and how many requests' tokens agree with the static form.

--step-compare: a pure-decode l2_step_batch against the l2_decode_sample_batch step (t 0.9, p 0.9), B = 16 and 64, sequence s at 4 s
(tools/batch_bench.py's placements); and one step of 16 decode rows + 48 prompt rows (3 x 16) against l2_forward_batch of the 16 rows
followed by l2_seq_prefill_batch of the 48.
--trace-step: only a few mixed steps on a head_size-128 shape whose decode rows sit past the prompt tiles' 150 KiB LDS bound, beside
short prompt runs (run it under rocprofv3 --kernel-trace --stats to see which attention kernels ran).

    python tools/serve_bench.py --model stories110M [--slots 16,64] [--max-rows 64,256] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from llama2_ts_amd import configs, runtime, serve  # noqa: E402


def pct(v, q):
    return round(float(np.percentile(v, q)) * 1e3, 3) if len(v) else None


def workload(n, V, seed):
    rng = np.random.default_rng(seed)
    reqs = []
    for i in range(n):
        p = [int(t) for t in rng.integers(3, V, int(rng.integers(8, 129)))]
        g = int(rng.integers(16, 257))
        sampled = i % 2 == 1
        reqs.append({"prompt": p, "gen": g, "t": 0.9 if sampled else 0.0, "p": 0.9 if sampled else 1.0, "seed": 1000 + i})
    return reqs


def run_static(ctx, reqs, slots):
    t0 = time.perf_counter()
    picks, ttft, lat = [], [], []
    for g0 in range(0, len(reqs), slots):
        grp = reqs[g0:g0 + slots]
        seqs = list(range(len(grp)))
        ctx.seq_prefill_batch(seqs, [[1] + r["prompt"][:-1] for r in grp], 0)
        steps = max(r["gen"] for r in grp)
        c0 = time.perf_counter()
        toks, _ = ctx.decode_sample_batch(seqs, [r["prompt"][-1] for r in grp], [len(r["prompt"]) for r in grp], steps,
                                          [r["t"] for r in grp], [r["p"] for r in grp], [r["seed"] for r in grp])
        c1 = time.perf_counter()
        for i, r in enumerate(grp):
            row = toks[i, :r["gen"]].tolist()
            if 1 in row:
                row = row[:row.index(1) + 1]
            picks.append(row[:-1])      # the picks that would be fed: the last is BOS or ends the request
            ttft.append(c1 - t0)
        lat += [(c1 - c0) / steps] * sum(len(p) + 1 for p in picks[-len(grp):])
    dt = time.perf_counter() - t0
    gen = sum(len(p) + 1 for p in picks)
    return picks, {"form": "static", "slots": slots, "seconds": round(dt, 3), "generated": gen, "tok_s": round(gen / dt, 1),
                   "ttft_ms_median": pct(ttft, 50), "ttft_ms_p99": pct(ttft, 99),
                   "token_ms_median": pct(lat, 50), "token_ms_p99": pct(lat, 99)}


class Recorder:
    """step_batch with the rows of every call counted."""

    def __init__(self, ctx):
        self.ctx, self.rows = ctx, []

    def get_option(self, k):
        return self.ctx.get_option(k)

    @property
    def cfg(self):
        return self.ctx.cfg

    def step_batch(self, *a, **kw):
        self.rows.append(sum(len(r) for r in a[1]))
        return self.ctx.step_batch(*a, **kw)


def run_continuous(ctx, reqs, slots, max_rows):
    rec = Recorder(ctx)
    s = serve.Scheduler(rec, max_rows=max_rows, slots=slots)
    rids = [s.submit(r["prompt"], len(r["prompt"]) + r["gen"], temperature=r["t"], topp=r["p"], seed=r["seed"]) for r in reqs]
    P = {rid: len(r["prompt"]) for rid, r in zip(rids, reqs)}
    seen = {rid: 0 for rid in rids}
    last = {}
    ttft, lat = [], []
    t0 = time.perf_counter()
    while not s.idle:
        done = s.step()
        now = time.perf_counter()
        live = [(r.rid, len(r.fed)) for r in s.active] + [(rid, len(res.tokens_fed)) for rid, res in done.items()]
        for rid, nfed in live:
            k = max(0, nfed - P[rid])
            if k > seen[rid]:
                if seen[rid] == 0:
                    ttft.append(now - t0)
                else:
                    lat.append((now - last[rid]) / (k - seen[rid]))
                seen[rid], last[rid] = k, now
    dt = time.perf_counter() - t0
    res = s.results
    picks = [res[rid].tokens_fed[P[rid] + 1:] for rid in rids]         # the picks that were fed (the last pick never is)
    gen = sum(len(p) + 1 for p in picks)
    hist = np.bincount(np.asarray(rec.rows)).tolist()
    return picks, {"form": "continuous", "slots": slots, "max_rows": max_rows, "seconds": round(dt, 3), "generated": gen,
                   "tok_s": round(gen / dt, 1), "ttft_ms_median": pct(ttft, 50), "ttft_ms_p99": pct(ttft, 99),
                   "token_ms_median": pct(lat, 50), "token_ms_p99": pct(lat, 99), "steps": len(rec.rows),
                   "rows_per_step_hist": {str(k): v for k, v in enumerate(hist) if v}}


def step_compare(ctx, fed, reserved, reps=32):
    out = []
    for B in (16, 64):
        if B > reserved:
            break
        seqs = list(range(B))
        pos0 = [4 * s for s in seqs]
        for s in seqs:
            if pos0[s]:
                ctx.seq_prefill(s, fed[:pos0[s]], 0)
        first = [fed[p] for p in pos0]
        seeds = [1000 + s for s in seqs]
        ctx.decode_sample_batch(seqs, first, pos0, 2, 0.9, 0.9, seeds)        # records the sampled step of B rows
        t0 = time.perf_counter()
        ctx.decode_sample_batch(seqs, first, pos0, reps, 0.9, 0.9, seeds)
        loop = (time.perf_counter() - t0) / reps
        ctx.step_batch(seqs, [[t] for t in first], pos0, 0.9, 0.9, seeds)     # warm-up
        toks, pos, rng = list(first), list(pos0), list(seeds)
        t0 = time.perf_counter()
        for _ in range(reps):
            picks, rng = ctx.step_batch(seqs, [[t] for t in toks], pos, 0.9, 0.9, rng)
            toks, pos = picks, [p + 1 for p in pos]
        step = (time.perf_counter() - t0) / reps
        out.append({"B": B, "decode_sample_batch_step_ms": round(loop * 1e3, 3), "step_batch_ms": round(step * 1e3, 3),
                    "ratio": round(step / loop, 4)})
    mixed = None
    if reserved >= 19:
        dseq, dpos = list(range(16)), [4 * s for s in range(16)]
        pseq, prom = [16, 17, 18], [fed[:16], fed[16:32], fed[32:48]]
        times = {"step": [], "two_calls": []}
        for rep in range(6):
            t0 = time.perf_counter()
            ctx.step_batch(dseq + pseq, [[fed[p]] for p in dpos] + prom, dpos + [0, 0, 0])
            t1 = time.perf_counter()
            ctx.forward_batch(dseq, [fed[p] for p in dpos], dpos)
            ctx.seq_prefill_batch(pseq, prom, 0)
            t2 = time.perf_counter()
            if rep:
                times["step"].append(t1 - t0)
                times["two_calls"].append(t2 - t1)
        a, b = float(np.median(times["step"])), float(np.median(times["two_calls"]))
        mixed = {"rows": "16 decode + 3 x 16 prompt", "step_ms": round(a * 1e3, 3), "forward_batch_plus_seq_prefill_batch_ms": round(b * 1e3, 3),
                 "ratio": round(a / b, 4)}
    return {"pure_decode": out, "mixed_16_plus_48": mixed}


def trace_step():
    hdr, seed = (256, 512, 1, 2, 2, 512, 3072), 7
    rng = np.random.default_rng(3)
    fed = [1] + [int(t) for t in rng.integers(2, hdr[5], 3000)]
    ctx = runtime.Context(hdr)
    ctx.synth_fill(seed)
    ctx.seq_reserve(4)
    ctx.seq_prefill_batch([1, 2], [fed[:2600], fed[:2800]], 0)
    for _ in range(3):
        picks, _ = ctx.step_batch([1, 0, 2, 3], [[fed[2600]], fed[:40], [fed[2800]], fed[:17]], [2600, 0, 2800, 0])
    ctx.close()
    return {"tool": "serve_bench", "trace_step": "decode rows at 2600 and 2800 (head_size 128) beside prompt runs of 40 and 17 at 0, 3 steps",
            "picks": picks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="stories110M", choices=["llama2_7b", "stories110M"])
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--slots", default="16,64")
    ap.add_argument("--max-rows", default="64,256")
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--step-compare", action="store_true")
    ap.add_argument("--no-serve", action="store_true", help="skip the static / continuous comparison")
    ap.add_argument("--trace-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_step:
        res = trace_step()
    else:
        meta = json.load(open(os.path.join(ROOT, "tests", "golden", args.model + ".json")))
        hdr = configs.header(args.model)
        V = abs(hdr[5])
        slots = [int(v) for v in args.slots.split(",")]
        ctx = runtime.Context(hdr)
        ctx.synth_fill(meta["seed"])
        ctx.seq_reserve(max(slots))
        res = {"tool": "serve_bench", "model": args.model, "requests": args.requests, "workload_seed": args.seed,
               "workload": "prompts 8-128, generations 16-256 (uniform); odd requests t 0.9 / p 0.9, even greedy"}
        if not args.no_serve:
            reqs = workload(args.requests, V, args.seed)
            runs = []
            for sl in slots:
                st_picks, st = run_static(ctx, reqs, sl)
                runs.append(st)
                for mr in [int(v) for v in args.max_rows.split(",")]:
                    if mr < sl:
                        continue
                    co_picks, co = run_continuous(ctx, reqs, sl, mr)
                    co["agree_with_static"] = sum(a == b for a, b in zip(st_picks, co_picks))
                    co["x_static_tok_s"] = round(co["tok_s"] / st["tok_s"], 3)
                    runs.append(co)
            res["runs"] = runs
        if args.step_compare:
            res["step_compare"] = step_compare(ctx, meta["tokens_fed"], max(slots))
        ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
