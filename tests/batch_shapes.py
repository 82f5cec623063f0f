"""The shape sweep of the prompt / batch kernels: its shapes, token streams, legs and their calls as DATA, shared by the CPU plan test
(tests/test_batch_plan_cpu.py: which kernel instances the table reaches, proven through l2_debug_batch_plan) and the GPU test
(tests/test_batch_shapes_gpu.py: the same calls run against the C oracle).  A call feeds sequence s the tokens pos0 .. pos0 + len - 1 of
its stream (teacher forced), so a call is fully described by (kind, [(sequence, pos0, len)], options).

Header order: dim, hidden, layers, heads, kv heads, vocab, seq_len.  The shapes are the smallest that still reach each form."""
import ctypes as C
import functools

import numpy as np

SEED = 7              # synth_fill seed of every shape
TOKEN_SEED = 11       # default_rng seed of the token streams
N_STREAMS = 7         # token streams per shape; sequence s of a context is fed stream s % N_STREAMS (no divisor of 64: a kernel that reads
                      # the cache of sequence s +- 1, 2, 4, 8, 16 or 32 reads another stream's)
N_SEQS = 64           # sequences a sweep context reserves

SHAPES = {
    "hs4_k1": (16, 48, 2, 4, 4, 97, 40),                # LR 4; K is one 16-column block (three of four split-K waves idle); vocab % 16 != 0
    "hs16_reg_k1": (32, 64, 1, 2, 2, -64, 40),          # register-blocked GEMMs with one K batch; wo has 2 row tiles: RT 1 at four chunks
    "hs20": (80, 176, 2, 4, 4, -263, 72),               # LR 8 partly filled; heads cross 16-row tiles in the RoPE epilogue; tile GEMMs
    "hs32_reg": (64, 192, 2, 2, 2, 301, 272),           # LR 8 full; register-blocked; wo has 4 row tiles: RT 4 at four chunks; prompts > 192
    "hs36": (144, 400, 1, 4, 4, -129, 72),              # LR 16 partly filled; head size no multiple of 16
    "hs96_reg": (192, 512, 1, 2, 2, 263, 80),           # LR 32 with eight waves, partly filled; register-blocked
    "hs192": (384, 1008, 1, 2, 2, -211, 72),            # LR 64 partly filled; tile GEMMs
    "hs256_reg": (512, 640, 1, 2, 2, 300, 80),          # LR 64 full; register-blocked
    "hs64_tile": (128, 336, 2, 2, 2, -257, 96),         # MFMA attention <64> with tile GEMMs and 64-row launch sequences
    "hs128_tile": (256, 432, 1, 2, 2, 300, 96),         # MFMA attention <128> with tile GEMMs
    "packed": (1280, 2560, 1, 10, 10, -320, 48),        # prompt and batch GEMMs reading the repacked copy (one decode step first)
}
EXACT_SHAPES = ("hs64_tile", "hs128_tile", "hs32_reg")
F32_SHAPES = ("hs32_reg", "hs96_reg", "hs256_reg")
LEGS = ("forward_batch", "prefill_batch", "prefill_one", "step_batch", "score")
OPTION_LEGS = ("exact", "f32")

# l2_debug_batch_plan (csrc/prefill_host.hip.h)
CALL_PROMPT, CALL_PACKED, CALL_BATCH = 0, 1, 2
POLICY_PROMPT, POLICY_BATCH = 0, 1
FLAG_EXACT, FLAG_F32, FLAG_PF3, FLAG_PF_ATTN = 1, 2, 4, 8
FAM_TILE, FAM_REG = 0, 1
AT_PF_MFMA, AT_BP_MFMA, AT_PF_TILE, AT_BT_TILE = 0, 1, 2, 3
GEMM_FAMILY = {FAM_TILE: "pf_gemm_kernel", FAM_REG: "pf_gemm3_kernel"}
ATTN_FAMILY = {AT_PF_MFMA: "pf_attn_mfma_kernel", AT_BP_MFMA: "bp_attn_mfma_kernel", AT_PF_TILE: "pf_attn_tile_kernel", AT_BT_TILE: "bt_attn_tile_kernel"}
PF_T = 64


def head_size(hdr):
    return hdr[0] // hdr[3]


def flags_of(opts):
    return FLAG_PF3 | FLAG_PF_ATTN | (FLAG_EXACT if opts.get("exact") else 0) | (FLAG_F32 if opts.get("f32") else 0)


def plan(hdr, call, policy, m, nd=0, last_pos=15, flags=FLAG_PF3 | FLAG_PF_ATTN):
    """l2_debug_batch_plan as a dict, or None when the library refuses the arguments (more rows than a launch sequence holds).
    `instances`: the kernel instances the launch sequence runs, as (family name, template arguments)."""
    from llama2_ts_amd import runtime
    L = runtime.lib()
    L.l2_debug_batch_plan.argtypes = [C.c_int] * 10 + [C.c_void_p]
    L.l2_debug_batch_plan.restype = C.c_int
    out = (C.c_int * 48)()
    rc = L.l2_debug_batch_plan(hdr[0], hdr[1], head_size(hdr), hdr[6], call, policy, m, nd, last_pos, flags, out)
    if rc != 0:
        return None
    o = list(out)
    p = {"can_prefill": bool(o[0]), "step": o[1], "chunks": o[2], "tt": o[3], "rows_seen": o[4], "last_tile_valid": o[5], "gemms": [], "attn": []}
    if not p["can_prefill"]:
        return p
    for g in range(5):
        fam, mode, tr, f32, chunks = o[8 + 5 * g:13 + 5 * g]
        p["gemms"].append({"family": fam, "mode": mode, "tr": tr, "f32": f32, "chunks": chunks})
    for k in range(o[6]):
        fam, a, nw, nt, rows, lds = o[33 + 6 * k:39 + 6 * k]
        p["attn"].append({"family": fam, "a": a, "nw": nw, "nt": nt, "rows": rows, "lds": lds})
    p["instances"] = instances(p)
    return p


def instances(p, classifier=True):
    """(family, template arguments) of every launch of a plan: pf_gemm_kernel<MODE, 4, TT>, pf_gemm3_kernel<MODE, 4, RT, 4, F32>,
    {pf,bp}_attn_mfma_kernel<HS>, {pf,bt}_attn_tile_kernel<LR, NW, NT>."""
    out = set()
    for g in p["gemms"][:5 if classifier else 4]:
        if g["family"] == FAM_TILE:
            out.add(("pf_gemm_kernel", (g["mode"], 4, g["tr"])))
        else:
            out.add(("pf_gemm3_kernel", (g["mode"], 4, g["tr"], 4, g["f32"])))
    for a in p["attn"]:
        if a["family"] in (AT_PF_MFMA, AT_BP_MFMA):
            out.add((ATTN_FAMILY[a["family"]], (a["a"],)))
        else:
            out.add((ATTN_FAMILY[a["family"]], (a["a"], a["nw"], a["nt"])))
    return out


def reaches_prompt_kernels(hdr):
    return plan(hdr, CALL_PROMPT, POLICY_PROMPT, 1)["can_prefill"]


@functools.lru_cache(maxsize=None)
def streams(name):
    hdr = SHAPES[name]
    return np.random.default_rng(TOKEN_SEED).integers(0, abs(hdr[5]), (N_STREAMS, hdr[6])).astype(np.int32)


# ---- the calls of every leg ----------------------------------------------------------------------------------------------------
# A call: {"kind", "runs": [(sequence, pos0, len)], "opts": {...}}.  kinds: forward_batch (len 1 each), prefill_batch, score, step_batch
# (len 1: a decode row), prefill (l2_prefill on sequence 0, l2_seq_prefill elsewhere), decode_step (one l2_forward on sequence 0: leaves the
# repacked weights as the only copy where the shape repacks), fork (l2_seq_fork of rows 0 .. len-1 of sequence "src" into the run's sequence).
RUN_LENGTHS = (1, 3, 15, 16, 17, 31, 33, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 40)
PACKED_TOTALS = (63, 64, 65, 129, 193, 257)      # rows per call: around the 64-row launch sequence, past 64, 128, 192, 256 on the 256-row one


class _Packer:
    """Deals run lengths to sequences (shuffled), continuing each sequence where its last run ended."""

    def __init__(self, S, seed, seqs):
        self.S, self.rng, self.seqs = S, np.random.default_rng(seed), list(seqs)
        self.pos = {s: 0 for s in self.seqs}
        self.k = 0

    def call(self, total, lengths=RUN_LENGTHS, fresh=False):
        runs, left = [], total
        order = [self.seqs[i] for i in self.rng.permutation(len(self.seqs))]
        fed = [s for s in order if 0 < self.pos[s] < self.S]
        if fed and not fresh:      # every call after the first continues at least one sequence
            order.remove(fed[0]); order.insert(0, fed[0])
        for s in order:
            if left == 0:
                break
            if fresh and self.pos[s] > 0:
                continue
            n = min(lengths[self.k % len(lengths)], self.S - self.pos[s], left)
            if n <= 0:
                continue
            self.k += 1
            runs.append((s, self.pos[s], n))
            self.pos[s] += n
            left -= n
        assert left == 0, "the sequences cannot hold %d more rows" % left
        return runs


FORWARD_BATCH_ROWS = (1, 16, 17, 32, 33, 64)      # rows of the l2_forward_batch calls: both sides of every 16-row tile, and all four tiles full


def _forward_batch_calls(hdr):
    rng = np.random.default_rng(1)
    late = N_SEQS - 1                            # joins late: position 0 while the others are at 1 .. 24
    pos = {s: 1 + (5 * s) % 21 for s in range(late)}
    calls = [{"kind": "prefill_batch", "runs": [(s, 0, pos[s]) for s in range(late)]}]
    pos[late] = 0
    for n in FORWARD_BATCH_ROWS:
        rows = ([late] if n >= 17 else []) + [int(s) for s in rng.permutation(late)]
        rows = [rows[i] for i in rng.permutation(n)]      # n distinct sequences (from 17 rows on the late one among them), shuffled
        calls.append({"kind": "forward_batch", "runs": [(s, pos[s], 1) for s in rows]})
        for s in rows:
            pos[s] += 1
    return calls


def _packed_calls(hdr, kind):
    pk = _Packer(hdr[6], 2, range(N_SEQS - 1))   # sequence 63 is named in no call
    return [{"kind": kind, "runs": pk.call(t)} for t in PACKED_TOTALS]


PREFILL_ONE_LENGTHS = (2, 17, 33, 65)      # and the whole context; those that fit


def _prefill_one_calls(hdr):
    S = hdr[6]
    calls, seq = [], 0
    for n in PREFILL_ONE_LENGTHS + (S,):
        if n <= S:
            calls.append({"kind": "prefill", "runs": [(0, 0, n)]})                 # l2_prefill: sequence 0, from the start each time
            seq += 1
            calls.append({"kind": "prefill", "runs": [(seq, 0, n)]})               # l2_seq_prefill: a fresh sequence each
    # continuations at positions that are no multiple of 16: after 17 rows, and of the two-row sequence
    calls.append({"kind": "prefill", "runs": [(0, 0, 17)]})
    calls.append({"kind": "prefill", "runs": [(0, 17, min(S - 17, 20))]})
    calls.append({"kind": "prefill", "runs": [(2, 17, min(S - 17, 21))]})          # sequence 2 holds 17 rows
    calls.append({"kind": "prefill", "runs": [(1, 2, min(S - 2, 35))]})            # sequence 1 holds 2 rows
    return calls


def _step_batch_calls(hdr):
    S = hdr[6]
    dec = list(range(6))                                                           # decode rows at 13 .. 18: both sides of the 16-boundary
    forked = N_SEQS - 1                                                            # (same stream as sequence 0: 63 % 7 == 0)
    calls = [{"kind": "prefill_batch", "runs": [(s, 0, 13 + s) for s in dec]},
             {"kind": "fork", "src": 0, "runs": [(forked, 0, 13)]}]                # l2_seq_fork: rows 0 .. 12 of sequence 0 into sequence 63
    pk = _Packer(S, 4, range(6, N_SEQS - 1))
    order = [(s, 13 + s, 1) for s in dec] + pk.call(262, fresh=True)               # the runs cross the 64- and the 256-row boundary
    order = [order[i] for i in pk.rng.permutation(len(order))]
    calls.append({"kind": "step_batch", "runs": order})
    order = [(s, 14 + s, 1) for s in dec[::2]] + pk.call(70) + [(forked, 13, 5)]   # continuations at pos0 > 0 (the forked one too) beside decode rows
    calls.append({"kind": "step_batch", "runs": [order[i] for i in pk.rng.permutation(len(order))]})
    calls.append({"kind": "step_batch", "runs": [(s, 15 + s, 1) for s in dec[::2]] + [(1, 15, 1), (forked, 18, 1)]})      # decode rows only
    return calls


F32_ROWS = (64, 128, 256)


def _f32_calls(hdr):
    S = hdr[6]
    pk = _Packer(S, 5, range(1, N_SEQS - 1))
    calls = [{"kind": "prefill_batch", "runs": pk.call(t), "opts": {"f32": 1}} for t in F32_ROWS]
    for n in F32_ROWS:
        if n <= S:
            calls.append({"kind": "prefill", "runs": [(0, 0, n)], "opts": {"f32": 1}})
    return calls


def _exact_calls(hdr):
    S = hdr[6]
    pk = _Packer(S, 6, range(1, N_SEQS - 1))
    calls = [{"kind": "prefill_batch", "runs": pk.call(t), "opts": {"exact": 1}} for t in (65, 257)]
    calls.append({"kind": "prefill", "runs": [(0, 0, min(S, 65))], "opts": {"exact": 1}})
    order = [(s, pk.pos[s], 1) for s in list(pk.pos)[:5] if 0 < pk.pos[s] < S] + [(N_SEQS - 1, 0, min(S, 37))]
    calls.append({"kind": "step_batch", "runs": order, "opts": {"exact": 1}})
    return calls


@functools.lru_cache(maxsize=None)
def leg_calls(name, leg):
    hdr = SHAPES[name]
    if leg == "forward_batch":
        calls = _forward_batch_calls(hdr)
    elif leg == "prefill_batch":
        calls = _packed_calls(hdr, "prefill_batch")
    elif leg == "score":
        calls = _packed_calls(hdr, "score")
    elif leg == "prefill_one":
        calls = _prefill_one_calls(hdr)
    elif leg == "step_batch":
        calls = _step_batch_calls(hdr)
    elif leg == "f32":
        calls = _f32_calls(hdr)
    elif leg == "exact":
        calls = _exact_calls(hdr)
    else:
        raise KeyError(leg)
    for c in calls:
        c.setdefault("opts", {})
    if name == "packed":
        calls = [{"kind": "decode_step", "runs": [(0, 0, 1)], "opts": {}}] + calls
    return calls


def case_table():
    """(shape, leg) of every GPU case."""
    out = [(n, leg) for n in SHAPES for leg in LEGS]
    out += [(n, "exact") for n in EXACT_SHAPES] + [(n, "f32") for n in F32_SHAPES]
    return out


# ---- the launch sequences of a call ----------------------------------------------------------------------------------------------
def launch_sequences(hdr, call):
    """The plan queries of one call: dicts of call, policy, m, nd, last_pos, flags, cls (rows of each classifier slice, [] when the call's
    logits come from the decode classifier), tiles (nvalid of every attention tile).

    This is a RESTATEMENT in Python of how the host cuts a call into launch sequences; nothing but review holds the two together.  When
    one of these changes, re-check this function against it: csrc/batch_host.hip.h bp_plan (rows per launch sequence, tiles starting at a
    run's first row in the launch sequence, maxp), bt_step (decode rows packed first), bp_enqueue (ndk, the classifier of a scoring launch
    sequence and of the runs' last rows), bt_classify (64-row slices), l2_seq_prefill (one token: the batch step; the one-row classifier);
    csrc/prefill_host.hip.h l2_prefill (one token: l2_forward) and prefill_chunk (last_pos)."""
    flags = flags_of(call["opts"])
    step = plan(hdr, CALL_PROMPT, POLICY_PROMPT, 1, flags=flags)["step"]
    kind, runs = call["kind"], call["runs"]
    slices = lambda n: [min(PF_T, n - s0) for s0 in range(0, n, PF_T)]
    if kind in ("decode_step", "fork"):
        return []
    if kind == "forward_batch":
        return [{"call": CALL_BATCH, "policy": POLICY_BATCH, "m": len(runs), "nd": 0, "last_pos": 15, "flags": flags, "cls": slices(len(runs)), "tiles": []}]
    if kind == "prefill":
        (s, pos0, n), = runs
        if n == 1:
            return [] if s == 0 else [{"call": CALL_BATCH, "policy": POLICY_BATCH, "m": 1, "nd": 0, "last_pos": 15, "flags": flags, "cls": [1], "tiles": []}]
        out = []
        for done in range(0, n, step):
            m = min(step, n - done)
            out.append({"call": CALL_PROMPT, "policy": POLICY_PROMPT, "m": m, "nd": 0, "last_pos": pos0 + done + ((m + 15) & ~15) - 1, "flags": flags,
                        "cls": [], "tiles": [min(16, m - t) for t in range(0, m, 16)]})
        if s != 0:
            out[-1]["cls"] = [1]
        return out
    if kind == "step_batch":
        runs = [r for r in runs if r[2] == 1] + [r for r in runs if r[2] > 1]
        nd = sum(1 for r in runs if r[2] == 1)
    else:
        nd = 0
    first = np.concatenate([[0], np.cumsum([r[2] for r in runs])])
    R = int(first[-1])
    out = []
    for k in range((R + step - 1) // step):
        r0, r1 = k * step, min(k * step + step, R)
        tiles, maxp = [], 0
        for i, (s, pos0, n) in enumerate(runs):
            lo, hi = max(int(first[i]), r0), min(int(first[i + 1]), r1)
            for t in range(lo, hi, 16):
                if i >= nd:
                    tiles.append(min(16, hi - t))
                    maxp = max(maxp, pos0 + t - int(first[i]))
        m = r1 - r0
        out.append({"call": CALL_PACKED, "policy": POLICY_PROMPT, "m": m, "nd": nd if k == 0 else 0, "last_pos": maxp + 15, "flags": flags,
                    "cls": slices(m) if kind == "score" else [], "tiles": tiles})
    if kind != "score":
        out[-1]["cls"] = slices(len(runs))
    return out


def plans_of(hdr, call):
    """[(query, plan, instances)] of every launch sequence of a call, the classifier slices' instances included."""
    out = []
    for q in launch_sequences(hdr, call):
        p = plan(hdr, q["call"], q["policy"], q["m"], q["nd"], q["last_pos"], q["flags"])
        assert p is not None and p["can_prefill"], (hdr, q)
        inst = instances(p, classifier=False)
        for rows in q["cls"]:
            c = plan(hdr, CALL_BATCH, POLICY_BATCH, rows, flags=q["flags"])
            inst.add(("pf_gemm_kernel", (c["gemms"][4]["mode"], 4, c["gemms"][4]["tr"])))
        out.append((q, p, inst))
    return out
