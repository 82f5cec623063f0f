"""Constrained decoding (l2_step_batch_constrained): what a token mask costs a decode step.  One process, synthetic weights
(l2_synth_fill, seed 1), decode-only steps at B = 16 and 64 (sequence s at position 4 s + 64, every row t 0.9 / top-p 0.9), the C
entry points called directly with arrays built once, so the host clock brackets the blocking library call and nothing else.

Forms, alternating step by step after a warm-up:
  plain     l2_step_batch
  distinct  l2_step_batch_constrained, every row under its own mask of a third of the vocabulary (B masks uploaded)
  shared    l2_step_batch_constrained, one such mask named by every row (1 mask uploaded)
Each repeat gives one median per form; the result holds the median of those and their spread (min .. max).

--plain-lib PATH times the plain form alone through another build of the library (say the parent commit's), for an A/B of the
unconstrained step: run this tool alternately with and without it.
--trace: warm-up, then 20 constrained steps (distinct masks) at B = 16 only, for `rocprofv3 --kernel-trace --stats`.

    python tools/constrain_bench.py [--model llama2_7b] [--steps 200] [--warmup 20] [--repeats 3] [--plain-lib lib.so] [--out file.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from llama2_ts_amd import configs, runtime  # noqa: E402


def check(L, rc):
    if rc != 0:
        raise RuntimeError("libllama2hip: %s (code %d)" % (L.l2_last_error().decode("utf8", "replace"), rc))


def open_lib(path):
    L = C.CDLL(path)
    L.l2_last_error.restype = C.c_char_p
    vp, i32 = C.c_void_p, C.c_int
    L.l2_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.l2_destroy.argtypes = [vp]
    L.l2_destroy.restype = None
    L.l2_synth_fill.argtypes = [vp, C.c_uint32]
    L.l2_seq_reserve.argtypes = [vp, i32]
    L.l2_seq_prefill_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.l2_step_batch.argtypes = [vp] + [i32] + [vp] * 9
    if hasattr(L, "l2_step_batch_constrained"):
        L.l2_step_batch_constrained.argtypes = [vp, i32] + [vp] * 9 + [i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    return L


def forms_for(L, h, V, B, plain_only):
    """{name: zero-argument callable} over arrays that live as long as the callables."""
    rng = np.random.default_rng(B)
    seqs = np.arange(B, dtype=np.int32)
    pos = (4 * seqs + 64).astype(np.int32)
    hist = [np.concatenate(([1], rng.integers(3, V, int(p)))).astype(np.int32) for p in pos]
    nt = pos.copy()
    zero = np.zeros(B, dtype=np.int32)
    fed = np.ascontiguousarray(np.concatenate([x[:p] for x, p in zip(hist, pos)]), dtype=np.int32)
    check(L, L.l2_seq_prefill_batch(h, B, seqs.ctypes.data, nt.ctypes.data, fed.ctypes.data, zero.ctypes.data, None))
    tok = np.array([x[p] for x, p in zip(hist, pos)], dtype=np.int32)
    one = np.ones(B, dtype=np.int32)
    temp, topp = np.full(B, 0.9), np.full(B, 0.9)
    st = np.arange(1, B + 1, dtype=np.uint64)
    picks = np.zeros(B, dtype=np.int32)
    masks = np.stack([runtime.pack_mask(rng.choice(np.arange(1, V), V // 3, replace=False), V) for _ in range(B)])
    own, same = np.arange(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    keep = (seqs, pos, tok, one, temp, topp, st, picks, masks, own, same)
    head = (h, B, seqs.ctypes.data, one.ctypes.data, tok.ctypes.data, pos.ctypes.data, temp.ctypes.data, topp.ctypes.data, st.ctypes.data,
            picks.ctypes.data, None)

    def plain(_keep=keep):
        check(L, L.l2_step_batch(*head))

    def distinct(_keep=keep):
        check(L, L.l2_step_batch_constrained(*head, 0, None, None, None, own.ctypes.data, B, masks.ctypes.data, None, None, None))

    def shared(_keep=keep):
        check(L, L.l2_step_batch_constrained(*head, 0, None, None, None, same.ctypes.data, 1, masks.ctypes.data, None, None, None))

    return {"plain": plain} if plain_only else {"plain": plain, "distinct": distinct, "shared": shared}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def measure(forms, steps, warmup, repeats):
    for _ in range(warmup):
        for f in forms.values():
            f()
    med = {k: [] for k in forms}
    for _ in range(repeats):
        t = {k: [] for k in forms}
        for _ in range(steps):
            for k, f in forms.items():
                t[k].append(timed(f))
        for k in forms:
            med[k].append(float(np.median(t[k])) * 1e3)
    out = {}
    for k, v in med.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
    for k in forms:
        if k != "plain":
            out[k + "_over_plain"] = round(out[k + "_ms"] / out["plain_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama2_7b", choices=["llama2_7b", "stories110M"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--plain-lib", default=None, help="time the plain step alone through this build of the library")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    path = args.plain_lib or runtime.LIB_PATH
    L = open_lib(path)
    hdr = configs.header(args.model)
    V = abs(hdr[5])
    h = C.c_void_p()
    check(L, L.l2_create((C.c_int32 * 7)(*hdr), 0, C.byref(h)))
    check(L, L.l2_synth_fill(h, 1))
    check(L, L.l2_seq_reserve(h, 64))
    res = {"tool": "constrain_bench", "model": args.model, "weights": "l2_synth_fill seed 1", "library": os.path.basename(path) if args.plain_lib else "this build",
           "steps": args.steps, "repeats": args.repeats}
    if args.trace:
        f = forms_for(L, h, V, 16, False)
        for _ in range(args.warmup):
            f["plain"]()
        for _ in range(20):
            f["distinct"]()
        res["trace"] = "20 constrained steps, B = 16, every row under its own one-third mask, t 0.9 / top-p 0.9"
    else:
        res["rows"] = []
        for B in (16, 64):
            r = {"B": B}
            r.update(measure(forms_for(L, h, V, B, args.plain_lib is not None), args.steps, args.warmup, args.repeats))
            res["rows"].append(r)
    L.l2_destroy(h)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
