"""Aggregate decode rate of the batched greedy loop (l2_decode_greedy_batch) against the batch-1 device loop, one process, synthetic
weights (l2_synth_fill, the golden's seed).

For B = 1, 2, 4, ..., 64 (as many as the device memory reserves) the first B sequences, sequence s prefilled with the golden's first
p_s = 4 s fed tokens (distinct, all below 256), run 64 batch steps; the timed run's tokens are checked against
tests/golden/<model>.json (exit status 1 on a mismatch).  Prints ONE JSON line: per B the step time, aggregate and per-sequence
tok/s, weight bytes per step / step time as a fraction of 8 TB/s, GEMM flops / step time as a fraction of the 78.6 TF fp64 matrix
peak, and the ratio to the batch-1 device loop (l2_bench_decode) measured in the same process.

    python tools/batch_bench.py --model llama2_7b [--steps 64] [--out file.json]

With --temperature T (and --topp P) every B is also timed through the sampled loop (l2_decode_sample_batch: the same setting on every
row, seed 1000 + s for sequence s), in the same process.  The sampled run's first 8 steps are checked by replaying them through
l2_forward_batch on the same context (same rows, same order) and the C oracle's sampler (tests/oracle_lib.py); exit status 1 on a
mismatch.  Without the flags the tool times the greedy loop only, as before.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from llama2_ts_amd import configs, runtime  # noqa: E402

HBM_BPS, FP64_MFMA_FLOPS = 8.0e12, 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama2_7b", choices=["llama2_7b", "stories110M"])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batches", default="1,2,4,8,16,32,64", help="row counts to time (comma list)")
    ap.add_argument("--eager", action="store_true", help="eager launches instead of the replayed hipGraph (L2_OPT_USE_GRAPH = 0)")
    ap.add_argument("--temperature", type=float, default=None, help="also time the sampled loop at this temperature (every row)")
    ap.add_argument("--topp", type=float, default=1.0, help="top-p of the sampled loop (0 < p < 1: sample_topp)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    O = None
    if args.temperature is not None:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib as O  # noqa: E402
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", args.model + ".json")))
    hdr = configs.header(args.model)
    d, h, L, _H, _kv, V, _S = hdr
    V = abs(V)
    fed, picks = meta["tokens_fed"], meta["argmax"]
    steps = args.steps
    ctx = runtime.Context(hdr)
    ctx.synth_fill(meta["seed"])
    if args.eager:
        ctx.set_option(runtime.OPT_USE_GRAPH, 0)
    reserved = 0
    want = max(int(v) for v in args.batches.split(","))
    for n in [v for v in (64, 32, 16, 8, 4, 2, 1) if v <= want]:
        try:
            ctx.seq_reserve(n)
            reserved = n
            break
        except runtime.L2Error as e:
            if e.code != -3:
                raise
    offsets = [4 * s for s in range(reserved)]
    for s, off in enumerate(offsets):
        if off:
            ctx.seq_prefill(s, fed[:off], 0)
    # batch-1 device loop (the library's greedy loop, l2_bench_decode) from BOS: sequence 0's own cache, rewritten below
    ctx.bench_decode(fed[0], 0, 8)
    b1_ms = ctx.bench_decode(fed[0], 0, steps)
    b1_ok = ctx.bench_tokens(steps).tolist() == picks[:steps]
    b1 = steps / (b1_ms / 1e3)
    mat = L * (4 * d * d + 3 * d * h) + V * d            # matrix elements streamed per step (every layer + the classifier)
    rows, ok = [], b1_ok
    for B in [int(v) for v in args.batches.split(",")]:
        if B > reserved:
            break
        seqs = list(range(B))
        first = [fed[offsets[s]] for s in seqs]
        pos0 = [offsets[s] for s in seqs]
        ctx.decode_greedy_batch(seqs, first, pos0, 2)      # records the step of B rows
        t0 = time.perf_counter()
        toks = ctx.decode_greedy_batch(seqs, first, pos0, steps)
        dt = time.perf_counter() - t0
        good = all(toks[s].tolist() == picks[offsets[s]:offsets[s] + steps] for s in seqs)
        ok = ok and good
        step_s = dt / steps
        row = {"B": B, "step_ms": round(step_s * 1e3, 3), "agg_tok_s": round(B / step_s, 1), "per_seq_tok_s": round(1 / step_s, 1),
               "hbm_frac": round(mat * 4 / step_s / HBM_BPS, 4), "fp64_mfma_frac": round(2.0 * B * mat / step_s / FP64_MFMA_FLOPS, 4),
               "x_batch1": round(B / step_s / b1, 2), "tokens_match": good}
        if O is not None:
            seeds = [1000 + s for s in seqs]
            ctx.decode_sample_batch(seqs, first, pos0, 2, args.temperature, args.topp, seeds)     # records the sampled step of B rows
            t0 = time.perf_counter()
            stoks, _ = ctx.decode_sample_batch(seqs, first, pos0, steps, args.temperature, args.topp, seeds)
            sdt = time.perf_counter() - t0
            # the timed run's first 8 steps against the oracle's sampler fed l2_forward_batch's logits (same rows, same order)
            rngs, toks, pos, sgood = [O.Rng(v) for v in seeds], list(first), list(pos0), True
            for k in range(min(8, steps)):
                lg = ctx.forward_batch(seqs, toks, pos)
                for i in range(B):
                    toks[i], _ = O.next_token(lg[i], args.temperature, args.topp, rngs[i])
                    sgood = sgood and toks[i] == int(stoks[i, k])
                    pos[i] += 1
            ok = ok and sgood
            sstep = sdt / steps
            row.update({"sampled_step_ms": round(sstep * 1e3, 3), "sampled_agg_tok_s": round(B / sstep, 1),
                        "sampled_over_greedy": round(sstep / step_s, 4), "sampled_tokens_match": sgood})
        rows.append(row)
    res = {"tool": "batch_bench", "model": args.model, "steps": steps, "positions": "sequence s starts at 4 s (0 .. %d)" % offsets[-1],
           "launches": "eager" if args.eager else "hipGraph",
           "sampled": None if O is None else {"temperature": args.temperature, "topp": args.topp, "seeds": "1000 + s"}, "batch1_device_loop_tok_s": round(b1, 1), "batch1_tokens_match": b1_ok, "reserved": reserved, "rows": rows, "parity": ok}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
