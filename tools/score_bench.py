"""Per-token log-probabilities (l2_seq_score_batch, l2_step_batch_logprobs): what they cost, one process, synthetic weights
(l2_synth_fill, seed 1) or a checkpoint (--checkpoint).  Host clock around synchronised calls; every shape is run once before it is
timed, and the forms under comparison alternate rep by rep.

Scoring rate: l2_seq_score_batch tok/s against l2_seq_prefill_batch on the same rows (random tokens at position 0), B x L = 16 x 256,
64 x 64 and 1 x 1024, and against an l2_forward loop with a host log-softmax (64 tokens).
Step overhead (--no-step skips it): a pure-decode l2_step_batch against l2_step_batch_logprobs at top_k 0 and 20, B = 16 and 64
(sequence s at position 4 s + 64, greedy rows).
--compare-f32: the 16 x 256 rows scored with and without L2_OPT_PREFILL_F32_MFMA: mean and max |d lp|, perplexity under both, and the
rows whose argmax differs.
--trace: one 16 x 256 scoring call and one B = 16 logprobs step only, for `rocprofv3 --kernel-trace --stats`.

    python tools/score_bench.py --model llama2_7b [--reps 5] [--compare-f32] [--checkpoint model.bin] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from llama2_ts_amd import configs, runtime  # noqa: E402

CASES = ((16, 256), (64, 64), (1, 1024))


def rows_of(V, B, L, seed):
    rng = np.random.default_rng(seed)
    return [[1] + [int(t) for t in rng.integers(3, V, L - 1)] for _ in range(B)]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def scoring(ctx, V, reps):
    out = []
    for B, L in CASES:
        runs = rows_of(V, B, L, 10 + B)
        seqs = list(range(B))
        score = lambda: ctx.seq_score_batch(seqs, runs, 0)
        prefill = lambda: ctx.seq_prefill_batch(seqs, runs, 0)
        score(); prefill()
        ts, tp = [], []
        for _ in range(reps):
            ts.append(timed(score))
            tp.append(timed(prefill))
        R = B * L
        s, p = float(np.median(ts)), float(np.median(tp))
        out.append({"B": B, "L": L, "rows": R, "score_tok_s": round(R / s, 1), "prefill_tok_s": round(R / p, 1),
                    "score_over_prefill": round(p / s, 4), "score_ms": round(s * 1e3, 3), "prefill_ms": round(p * 1e3, 3)})
    return out


def forward_loop(ctx, V, n=64):
    """The way to per-position log-probabilities before: one l2_forward per token, the log-softmax on the host."""
    toks = rows_of(V, 1, n, 3)[0]
    ctx.forward(toks[0], 0)
    t0 = time.perf_counter()
    for p, t in enumerate(toks):
        x = ctx.forward(t, p).astype(np.float64)
        m = x.max()
        lp = x - (m + np.log(np.exp(x - m).sum()))
        if p + 1 < n:
            _ = lp[toks[p + 1]]
    dt = time.perf_counter() - t0
    return {"tokens": n, "tok_s": round(n / dt, 1)}


def step_overhead(ctx, V, reps):
    out = []
    rng = np.random.default_rng(4)
    for B in (16, 64):
        seqs = list(range(B))
        pos = [4 * s + 64 for s in seqs]
        hist = [[1] + [int(t) for t in rng.integers(3, V, p)] for p in pos]
        ctx.seq_prefill_batch(seqs, [h[:p] for h, p in zip(hist, pos)], 0)
        runs = [[h[p]] for h, p in zip(hist, pos)]
        forms = {"step": lambda: ctx.step_batch(seqs, runs, pos),
                 "logprobs_k0": lambda: ctx.step_batch(seqs, runs, pos, logprobs=0),
                 "logprobs_k20": lambda: ctx.step_batch(seqs, runs, pos, logprobs=20)}
        for f in forms.values():
            f()
        t = {k: [] for k in forms}
        for _ in range(reps):
            for k, f in forms.items():
                t[k].append(timed(f))
        ms = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
        out.append({"B": B, "step_ms": round(ms["step"], 4), "k0_ms": round(ms["logprobs_k0"], 4), "k20_ms": round(ms["logprobs_k20"], 4),
                    "k0_over_step": round(ms["logprobs_k0"] / ms["step"], 4), "k20_over_step": round(ms["logprobs_k20"] / ms["step"], 4)})
    return out


def compare_f32(ctx, V):
    B, L = CASES[0]
    runs = rows_of(V, B, L, 10 + B)
    seqs = list(range(B))
    ctx.set_option(runtime.OPT_PREFILL_F32_MFMA, 0)
    lp0, am0, _, _ = ctx.seq_score_batch(seqs, runs, 0)
    ctx.set_option(runtime.OPT_PREFILL_F32_MFMA, 1)
    lp1, am1, _, _ = ctx.seq_score_batch(seqs, runs, 0)
    ctx.set_option(runtime.OPT_PREFILL_F32_MFMA, 0)
    ok = ~np.isnan(lp0)
    d = np.abs(lp1[ok] - lp0[ok])
    return {"rows": int(ok.sum()), "mean_abs_dlp": float(d.mean()), "max_abs_dlp": float(d.max()),
            "ppl_f64": float(np.exp(-lp0[ok].mean())), "ppl_f32": float(np.exp(-lp1[ok].mean())),
            "argmax_differs": [int(r) for r in np.nonzero(am0 != am1)[0]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="stories110M", choices=["llama2_7b", "stories110M"])
    ap.add_argument("--checkpoint", default=None, help="a llama2.c checkpoint instead of synthetic weights")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compare-f32", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.checkpoint:
        ctx = runtime.load_checkpoint(args.checkpoint)
        V = ctx.cfg.vocab_size
        res = {"tool": "score_bench", "checkpoint": os.path.basename(args.checkpoint)}
    else:
        hdr = configs.header(args.model)
        ctx = runtime.Context(hdr)
        ctx.synth_fill(1)
        V = abs(hdr[5])
        res = {"tool": "score_bench", "model": args.model, "weights": "l2_synth_fill seed 1"}
    ctx.seq_reserve(64)
    if args.trace:
        B, L = CASES[0]
        ctx.seq_score_batch(list(range(B)), rows_of(V, B, L, 10 + B), 0)
        ctx.step_batch(list(range(16)), [[5]] * 16, [64 + 4 * s for s in range(16)], logprobs=20)
        res["trace"] = "one 16 x 256 scoring call, one B = 16 logprobs step (top_k 20)"
    else:
        res["scoring"] = scoring(ctx, V, args.reps)
        res["forward_loop"] = forward_loop(ctx, V)
        s16 = res["scoring"][0]["score_tok_s"]
        res["score_16x256_over_forward_loop"] = round(s16 / res["forward_loop"]["tok_s"], 2)
        if not args.no_step:
            res["step"] = step_overhead(ctx, V, max(args.reps, 9))
        if args.compare_f32:
            res["compare_f32"] = compare_f32(ctx, V)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
