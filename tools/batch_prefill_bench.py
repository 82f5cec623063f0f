"""Packed prompt ingestion (l2_seq_prefill_batch) against a loop of l2_seq_prefill over the same prompts, one process, synthetic
weights (l2_synth_fill, the golden's seed).

Cells: B prompts x L tokens for B in --batches and L in --lengths, plus the mixed set (one 256-token prompt and 15 prompts of 8 .. 40
tokens).  Sequence i takes prompt i at position 0; the tokens are random (fixed seed).  Per cell the two forms alternate, --reps
times each after one warm-up of each; both calls block until the device has finished, so the host clock around them is device time
plus the call's host work.  The median of each form gives prompt tok/s and the ratio loop / packed.  Every rep's last-position
argmax of both forms is compared row by row (exit status 1 on a mismatch).  Prints ONE JSON line.

    python tools/batch_prefill_bench.py --model llama2_7b [--batches 1,4,16,64] [--lengths 8,16,64,256] [--mixed 1] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from llama2_ts_amd import configs, runtime  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama2_7b", choices=["llama2_7b", "stories110M"])
    ap.add_argument("--batches", default="1,4,16,64", help="prompt counts (comma list)")
    ap.add_argument("--lengths", default="8,16,64,256", help="prompt lengths (comma list)")
    ap.add_argument("--mixed", type=int, default=1, help="also time the mixed set (one 256-token prompt, 15 of 8 .. 40 tokens)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", args.model + ".json")))
    hdr = configs.header(args.model)
    V = abs(hdr[5])
    rng = np.random.default_rng(1234)
    cells = [("%dx%d" % (B, L), [L] * B) for B in (int(v) for v in args.batches.split(",") if v) for L in (int(v) for v in args.lengths.split(",") if v)]
    if args.mixed:
        cells.append(("mixed", [256] + [int(v) for v in rng.integers(8, 41, 15)]))
    ctx = runtime.Context(hdr)
    ctx.synth_fill(meta["seed"])
    ctx.seq_reserve(max(len(lens) for _, lens in cells))
    rows, ok = [], True
    for name, lens in cells:
        prompts = [[int(t) for t in rng.integers(0, V, n)] for n in lens]
        seqs = list(range(len(lens)))

        def packed():
            return ctx.seq_prefill_batch(seqs, prompts, 0)

        def loop():
            return np.stack([ctx.seq_prefill(s, p, 0) for s, p in zip(seqs, prompts)])

        packed(); loop()      # warm-up (allocations, LDS opt-in)
        tp, tl, same = [], [], True
        for _ in range(args.reps):
            for fn, acc in ((packed, tp), (loop, tl)):
                t0 = time.perf_counter()
                lg = fn()
                acc.append((time.perf_counter() - t0) * 1e3)
                if fn is packed:
                    a = lg.argmax(axis=1)
                else:
                    same = same and bool(np.array_equal(a, lg.argmax(axis=1)))
        ok = ok and same
        mp, ml, tokens = statistics.median(tp), statistics.median(tl), sum(lens)
        rows.append(dict(cell=name, prompts=len(lens), tokens=tokens, packed_ms=round(mp, 3), loop_ms=round(ml, 3),
                         packed_tok_s=round(tokens / mp * 1e3, 1), loop_tok_s=round(tokens / ml * 1e3, 1), speedup=round(ml / mp, 3),
                         packed_ms_all=[round(v, 3) for v in tp], loop_ms_all=[round(v, 3) for v in tl], tokens_match=same))
        print("%-8s packed %9.2f ms  loop %9.2f ms  x%.2f  %s" % (name, mp, ml, ml / mp, "ok" if same else "TOKEN MISMATCH"), file=sys.stderr)
    ctx.close()
    line = json.dumps(dict(tool="batch_prefill_bench", model=args.model, reps=args.reps, tokens_ok=ok, cells=rows))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
