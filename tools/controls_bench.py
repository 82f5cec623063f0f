"""Sampling controls (l2_step_batch_sampling): what penalties, top-k and min-p cost a decode step.  One process, synthetic weights
(l2_synth_fill, seed 1), decode-only steps at B = 16 and 64 (sequence s at position 4 s + 64, every row t 0.9 / top-p 0.9), the C
entry points called directly with arrays built once, so the host clock brackets the blocking library call and nothing else.

Forms, alternating step by step after a warm-up:
  plain       l2_step_batch
  neutral     l2_step_batch_sampling with an l2_sample_controls that switches nothing on (no launch joins the step)
  penalties   every row penalised (repetition 1.3, presence 0.5, frequency 0.25) over a 256-token history
  controlled  the same, plus top_k = 40 and min_p = 0.05 on every row (all three launches)
Each repeat gives one median per form; the result holds the median of those and their spread (min .. max).

--plain-lib PATH times the plain form alone through another build of the library (say the parent commit's), for an A/B of the
unchanged step: run this tool alternately with and without it.
--trace: warm-up, then 20 controlled steps at B = 16 only, for `rocprofv3 --kernel-trace --stats`.

    python tools/controls_bench.py [--model llama2_7b] [--steps 200] [--warmup 20] [--repeats 3] [--plain-lib lib.so] [--out file.json]
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

HISTORY = 256


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
    if hasattr(L, "l2_step_batch_sampling"):
        L.l2_step_batch_sampling.argtypes = [vp, i32] + [vp] * 9 + [i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, C.POINTER(runtime.SampleControls)]
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
    head = (h, B, seqs.ctypes.data, one.ctypes.data, tok.ctypes.data, pos.ctypes.data, temp.ctypes.data, topp.ctypes.data, st.ctypes.data,
            picks.ctypes.data, None)
    tail = (0, None, None, None, None, 0, None, None, None, None)      # no logprobs, no constraints
    seen = [[int(t) for t in rng.integers(3, V, HISTORY // 2)] * 2 for _ in range(B)]      # 256 tokens, every id twice
    pen = dict(history=seen, repetition_penalty=[1.3] * B, presence_penalty=[0.5] * B, frequency_penalty=[0.25] * B)
    sets = {"neutral": runtime.sample_controls(B, history=seen, top_k=[0] * B), "penalties": runtime.sample_controls(B, **pen),
            "controlled": runtime.sample_controls(B, top_k=[40] * B, min_p=[0.05] * B, **pen)}
    keep = (seqs, pos, tok, one, temp, topp, st, picks, sets)

    def plain(_keep=keep):
        check(L, L.l2_step_batch(*head))

    def form(name):
        sc = sets[name][0]
        return lambda _keep=keep: check(L, L.l2_step_batch_sampling(*head, *tail, C.byref(sc)))

    out = {"plain": plain}
    if not plain_only:
        out.update({name: form(name) for name in sets})
    return out


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
    res = {"tool": "controls_bench", "model": args.model, "weights": "l2_synth_fill seed 1", "library": os.path.basename(path) if args.plain_lib else "this build",
           "steps": args.steps, "repeats": args.repeats, "history": HISTORY}
    if args.trace:
        f = forms_for(L, h, V, 16, False)
        for _ in range(args.warmup):
            f["plain"]()
        for _ in range(20):
            f["controlled"]()
        res["trace"] = "20 controlled steps, B = 16, 256-token histories, top_k 40, min_p 0.05, t 0.9 / top-p 0.9"
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
