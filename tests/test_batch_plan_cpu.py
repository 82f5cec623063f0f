"""The launch plan of the prompt / batch paths is a pure function (csrc/prefill_host.hip.h: plan_gemm / plan_attention, reachable through
l2_debug_batch_plan without a GPU), as the decode GEMVs' geometry is (tests/test_geo_cpu.py).  Read off the built library's gfx950 code
objects (symbol names only): every instance the plan selects exists; no instance of the prompt / batch GEMM and attention families exists
that nothing selects; and the case table of the shape sweep (tests/batch_shapes.py, run on the GPU by tests/test_batch_shapes_gpu.py)
selects every one of them and reaches every runtime branch the plan reports -- so an edit of that table cannot quietly drop coverage.
A fourth test holds the sweep's token streams to few near-ties of the oracle's two largest logits (the argmax is not asserted there)."""
import re

import numpy as np
import pytest

import batch_shapes as B
import code_objects
from llama2_ts_amd import configs

FAMILIES = {
    "pf_gemm_kernel": r"14pf_gemm_kernelILi(\d+)ELi(\d+)ELi(\d+)EE",
    "pf_gemm3_kernel": r"15pf_gemm3_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE",
    "pf_attn_mfma_kernel": r"19pf_attn_mfma_kernelILi(\d+)EE",
    "bp_attn_mfma_kernel": r"19bp_attn_mfma_kernelILi(\d+)EE",
    "pf_attn_tile_kernel": r"19pf_attn_tile_kernelILi(\d+)ELi(\d+)ELi(\d+)EE",
    "bt_attn_tile_kernel": r"19bt_attn_tile_kernelILi(\d+)ELi(\d+)ELi(\d+)EE",
}
# headers the batch GPU tests write inline in their parametrizations (tests/test_batch_gpu.py, tests/test_score_gpu.py); the ones they
# keep in constants are imported by walk_headers
INLINE_TEST_HEADERS = [(256, 512, 2, 4, 4, 1007, 64), (128, 384, 2, 2, 2, -600, 96), (64, 176, 2, 4, 4, 128256, 64), (64, 176, 2, 4, 4, 517, 64),
                       (64, 176, 2, 4, 4, -517, 64)]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    names = code_objects.kernel_names(tmp_path_factory.mktemp("co"))
    inst = {(fam, tuple(int(v) for v in ((m,) if isinstance(m, str) else m))) for fam, rx in FAMILIES.items() for n in names for m in re.findall(rx, n)}
    assert len(inst) > 40 and all(any(i[0] == fam for i in inst) for fam in FAMILIES), sorted(inst)
    return inst


def admissible_random_headers(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        H = int(rng.choice([1, 2, 3, 4, 5, 6, 8, 10, 16]))
        hs = 4 * int(rng.integers(1, 65))
        d = H * hs
        if d % 16 or d > 4096:
            continue
        h = 16 * int(rng.integers(d // 32 + 1, d // 4 + 2))
        out.append((d, h, 1, H, H, int(rng.integers(17, 700)) * int(rng.choice([-1, 1])), int(rng.choice([24, 64, 300, 2048, 3072]))))
    return out


def walk_headers():
    import test_batch_prefill_gpu
    import test_hip_parity as T
    import test_score_gpu
    import test_step_batch_gpu
    out = [configs.header(n) for n in configs.CONFIGS] + INLINE_TEST_HEADERS + list(B.SHAPES.values())
    out += [test_batch_prefill_gpu.LONG_HS128, test_step_batch_gpu.LONG_HS128, test_score_gpu.ODD_BATCH]
    out += T._random_headers(14, 20261003) + T.WIDE_SHAPES
    return out, admissible_random_headers(300, 15)


def walk(hdr, rows):
    """Every instance the plan selects for a header: the three calls with the policy each runs under, exact / fp32 on and off, `rows`
    launch-sequence sizes, with and without decode rows, a short and the longest context."""
    used = set()
    if not B.reaches_prompt_kernels(hdr):
        return used
    S = hdr[6]
    for exact in (0, 1):
        for f32 in (0, 2):
            flags = B.FLAG_PF3 | B.FLAG_PF_ATTN | exact | f32
            for call, policy in ((B.CALL_PROMPT, B.POLICY_PROMPT), (B.CALL_PACKED, B.POLICY_PROMPT), (B.CALL_BATCH, B.POLICY_BATCH)):
                for m in rows:
                    for nd in ((0, min(m, 3)) if call == B.CALL_PACKED else (0,)):
                        for last_pos in {15, S - 1 + 15}:
                            p = B.plan(hdr, call, policy, m, nd, last_pos, flags)
                            if p is None:      # more rows than this shape's launch sequence holds
                                assert m > (64 if call == B.CALL_BATCH else B.plan(hdr, call, policy, 1, 0, 15, flags)["step"]), (hdr, call, m)
                                continue
                            used |= p["instances"]
    return used


def test_every_selected_instance_exists_and_none_is_dead(built):
    listed, random = walk_headers()
    used = set()
    for hdr in listed + random:
        got = walk(hdr, range(1, 257))
        assert got <= built, ("selected, not in the library", hdr, sorted(got - built))
        used |= got
    dead = sorted(built - used)
    assert not dead, "instantiated, never selected: %s" % dead
    print("\n%d instances of the prompt / batch families, all selected; %d + %d headers walked" % (len(built), len(listed), len(random)))


def shape_reach(name):
    """What the cases of one shape reach: instances, runtime branches of the plan, and the features the shape table names."""
    hdr, hs = B.SHAPES[name], B.head_size(B.SHAPES[name])
    r = {"inst": set(), "chunks": set(), "tt": set(), "step": set(), "partial": set(), "nvalid": set(), "feat": set()}
    for leg in [leg for n, leg in B.case_table() if n == name]:
        for call in B.leg_calls(name, leg):
            for q, p, inst in B.plans_of(hdr, call):
                r["inst"] |= inst
                r["chunks"].add(p["chunks"]); r["tt"].add(p["tt"]); r["step"].add(p["step"]); r["partial"].add(p["last_tile_valid"] < 16)
                r["nvalid"] |= set(q["tiles"])
                reg = p["step"] == 256
                for a in p["attn"]:
                    if a["family"] in (B.AT_PF_TILE, B.AT_BT_TILE):
                        r["feat"].add(("rows attention", a["a"], "full" if hs == 4 * a["a"] else "partly filled"))
                        if call["opts"].get("exact") and hs in (64, 128):
                            r["feat"].add(("exact attention", hs, "reg" if reg else "tile"))
                    else:
                        assert not call["opts"].get("exact"), (name, leg, "the exact accumulate must take the rows form", p["attn"])
                        r["feat"].add(("mfma attention", B.ATTN_FAMILY[a["family"]], a["a"], "reg" if reg else "tile"))
                        if q["nd"]:
                            r["feat"].add("decode rows beside mfma tiles")
                wo = p["gemms"][1]
                if wo["family"] == B.FAM_REG:
                    r["feat"].add(("wo", "RT", wo["tr"], "chunks", wo["chunks"], "f32", wo["f32"]))
    return r


FEATURES = {("rows attention", 4, "partly filled"), ("rows attention", 4, "full"), ("rows attention", 8, "partly filled"), ("rows attention", 8, "full"),
            ("rows attention", 16, "partly filled"), ("rows attention", 16, "full"), ("rows attention", 32, "partly filled"), ("rows attention", 32, "full"),
            ("rows attention", 64, "partly filled"), ("rows attention", 64, "full"),
            ("mfma attention", "pf_attn_mfma_kernel", 64, "tile"), ("mfma attention", "bp_attn_mfma_kernel", 64, "tile"),
            ("mfma attention", "pf_attn_mfma_kernel", 128, "tile"), ("mfma attention", "bp_attn_mfma_kernel", 128, "tile"),
            ("mfma attention", "pf_attn_mfma_kernel", 128, "reg"), ("mfma attention", "bp_attn_mfma_kernel", 128, "reg"),
            ("exact attention", 64, "tile"), ("exact attention", 128, "tile"), "decode rows beside mfma tiles",
            ("wo", "RT", 1, "chunks", 4, "f32", 0), ("wo", "RT", 4, "chunks", 4, "f32", 0), ("wo", "RT", 2, "chunks", 2, "f32", 0),
            ("wo", "RT", 1, "chunks", 3, "f32", 0), ("wo", "RT", 1, "chunks", 1, "f32", 0),
            ("wo", "RT", 4, "chunks", 4, "f32", 1), ("wo", "RT", 2, "chunks", 2, "f32", 1), ("wo", "RT", 1, "chunks", 1, "f32", 1)}


def closure_gaps(built, names):
    """What the cases of the shapes `names` leave unreached (empty: the closure holds)."""
    rs = [shape_reach(n) for n in names]
    union = lambda k: set().union(*[r[k] for r in rs])
    gaps = [("instance", i) for i in sorted(built - union("inst"))]
    gaps += [("chunks", c) for c in {1, 2, 3, 4} - union("chunks")] + [("TT", t) for t in {1, 2, 4} - union("tt")]
    gaps += [("launch sequence rows", s) for s in {64, 256} - union("step")] + [("partly valid last tile", v) for v in {False, True} - union("partial")]
    gaps += [("tile nvalid", v) for v in set(range(1, 17)) - union("nvalid")] + [("feature", f) for f in sorted(FEATURES - union("feat"), key=str)]
    return gaps


def test_the_case_table_of_the_sweep_selects_every_instance_and_branch(built):
    for name in B.SHAPES:
        assert B.reaches_prompt_kernels(B.SHAPES[name]), name
        assert shape_reach(name)["inst"] <= built, (name, sorted(shape_reach(name)["inst"] - built))
    gaps = closure_gaps(built, list(B.SHAPES))
    assert not gaps, "no case of the sweep reaches: %s" % gaps
    print("\nthe sweep's %d cases select all %d instances" % (len(B.case_table()), len(built)))


@pytest.mark.parametrize("dropped", list(B.SHAPES))
def test_the_closure_notices_a_dropped_shape(built, dropped):
    """Every row of the shape table is there for something only it reaches."""
    gaps = closure_gaps(built, [n for n in B.SHAPES if n != dropped])
    print("\nwithout %s: %s" % (dropped, gaps))
    assert gaps


def test_the_row_counts_of_the_sweep_are_the_ones_fixed_in_advance():
    """The legs' row counts do not drift: l2_forward_batch at 1, 16, 17, 32, 33 and 64 rows with distinct sequences, shuffled, at different
    positions, one joining at position 0; packed calls of 63 / 64 / 65 / 129 / 193 / 257 rows with runs of 1, 3, 15, 16, 17, 31 and longer,
    continuations among them; one-sequence prompts of 2, 17, 33, 65 tokens and the whole context where they fit, continued at positions that
    are no multiple of 16; a mixed step with decode rows on both sides of position 16 whose runs cross the launch-sequence boundary; the
    fp32 leg at 64, 128 and 256 rows."""
    for name, hdr in B.SHAPES.items():
        S = hdr[6]
        body = lambda leg: [c for c in B.leg_calls(name, leg) if c["kind"] != "decode_step"]
        fb = [c for c in body("forward_batch") if c["kind"] == "forward_batch"]
        assert [len(c["runs"]) for c in fb] == [1, 16, 17, 32, 33, 64] == list(B.FORWARD_BATCH_ROWS), name
        for c in fb:
            seqs = [s for s, _, _ in c["runs"]]
            assert len(set(seqs)) == len(seqs) and all(n == 1 for _, _, n in c["runs"]) and seqs != sorted(seqs) or len(seqs) == 1, name
            assert len(seqs) < 16 or len({p for _, p, _ in c["runs"]}) > 4, (name, "rows at different positions")
        assert any(p == 0 for c in fb for _, p, _ in c["runs"]) and max(len(c["runs"]) for c in fb) == B.N_SEQS, (name, "a late sequence; every sequence")
        for leg in ("prefill_batch", "score"):
            calls = body(leg)
            assert [sum(n for _, _, n in c["runs"]) for c in calls] == [63, 64, 65, 129, 193, 257], (name, leg)
            assert {1, 3, 15, 16, 17, 31} <= {n for c in calls for _, _, n in c["runs"]} and any(n > 31 for c in calls for _, _, n in c["runs"]), (name, leg)
            assert all(any(p > 0 for _, p, _ in c["runs"]) for c in calls[1:]), (name, leg, "later calls continue sequences")
            assert [c["runs"] for c in calls] == [c["runs"] for c in body("prefill_batch")], (name, "scoring takes the prefill leg's packing")
        one = body("prefill_one")
        for seq0 in (True, False):
            fresh = {n for c in one for s, p, n in c["runs"] if p == 0 and (s == 0) == seq0}
            assert fresh >= {n for n in (2, 17, 33, 65, S) if n <= S}, (name, seq0, fresh)
            assert any(p % 16 for c in one for s, p, n in c["runs"] if (s == 0) == seq0), (name, seq0, "a continuation off the 16-row grid")
        step = B.plan(hdr, B.CALL_PROMPT, B.POLICY_PROMPT, 1)["step"]
        mixed = [c for c in body("step_batch") if c["kind"] == "step_batch"]
        dec = {p for _, p, n in mixed[0]["runs"] if n == 1}
        assert {15, 16} <= dec and sum(n for _, _, n in mixed[0]["runs"]) > step and any(n > 1 for _, _, n in mixed[0]["runs"]), name
        assert any(c["kind"] == "fork" for c in body("step_batch")), name
        if name in B.F32_SHAPES:
            f32 = [c for c in body("f32") if c["kind"] == "prefill_batch"]
            assert [sum(n for _, _, n in c["runs"]) for c in f32] == [64, 128, 256] and all(c["opts"] == {"f32": 1} for c in body("f32")), name
        if name in B.EXACT_SHAPES:
            assert all(c["opts"] == {"exact": 1} for c in body("exact")), name
    assert set(B.EXACT_SHAPES) == {"hs64_tile", "hs128_tile", "hs32_reg"} and set(B.F32_SHAPES) == {"hs32_reg", "hs96_reg", "hs256_reg"}


def test_plan_of_the_named_shapes():
    """What the shape table of tests/batch_shapes.py says of each shape, as the plan states it."""
    step = lambda n: B.plan(B.SHAPES[n], B.CALL_PROMPT, B.POLICY_PROMPT, 1)["step"]
    assert {n for n in B.SHAPES if step(n) == 256} == {"hs16_reg_k1", "hs32_reg", "hs96_reg", "hs256_reg", "packed"}
    lr = {n: B.plan(B.SHAPES[n], B.CALL_BATCH, B.POLICY_BATCH, 5)["attn"][0] for n in B.SHAPES}
    assert {n: (a["a"], a["nw"], a["nt"]) for n, a in lr.items()} == {
        "hs4_k1": (4, 4, 16), "hs16_reg_k1": (4, 4, 16), "hs20": (8, 4, 16), "hs32_reg": (8, 4, 16), "hs36": (16, 4, 16), "hs96_reg": (32, 8, 8),
        "hs192": (64, 4, 16), "hs256_reg": (64, 4, 16), "hs64_tile": (16, 4, 16), "hs128_tile": (32, 8, 8), "packed": (32, 8, 8)}
    for n, hs in (("hs64_tile", 64), ("hs128_tile", 128)):
        p = B.plan(B.SHAPES[n], B.CALL_PACKED, B.POLICY_PROMPT, 64, 0, 31)
        assert p["step"] == 64 and [(a["family"], a["a"]) for a in p["attn"]] == [(B.AT_BP_MFMA, hs)]
        assert all(g["family"] == B.FAM_TILE for g in p["gemms"])
    wo = lambda n, m, f=0: B.plan(B.SHAPES[n], B.CALL_PACKED, B.POLICY_PROMPT, m, 0, 15, B.FLAG_PF3 | B.FLAG_PF_ATTN | f)["gemms"][1]
    assert (wo("hs16_reg_k1", 256)["tr"], wo("hs32_reg", 256)["tr"], wo("hs32_reg", 128)["tr"], wo("hs32_reg", 192)["tr"]) == (1, 4, 2, 1)
    assert wo("hs32_reg", 256, B.FLAG_F32)["f32"] == 1


def test_sweep_streams_have_few_near_ties():
    """The argmax bar of the sweep skips rows whose two largest oracle logits lie within 2e-4 (twice the logit bar): at most 2 % of the fed
    rows of any shape."""
    import test_batch_shapes_gpu as G
    for name in B.SHAPES:
        ref = G.oracle_run(name)
        top2 = np.sort(ref["logits"].reshape(-1, ref["logits"].shape[-1]), axis=1)[:, -2:]
        ties = int(((top2[:, 1] - top2[:, 0]) <= 2e-4).sum())
        print("%s: %d / %d near-ties" % (name, ties, top2.shape[0]))
        assert ties <= 0.02 * top2.shape[0], (name, ties, top2.shape[0])
