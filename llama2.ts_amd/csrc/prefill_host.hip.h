// prefill_host.hip.h -- host side of batched prompt ingestion: the launch plan (plan_gemm, plan_attention, l2_debug_batch_plan), THE layer
// launch sequence every prompt / batch path enqueues (pf_layers: its activations, row addressing, GEMM policy and attention are arguments), and
// its first caller, l2_prefill (prefill_chunk).  The batch step and the packed path call it from batch_host.hip.h.
// Part of the one translation unit llama2_hip.hip (included there, in order); not a stand-alone header.
#pragma once

// ---- prefill -----------------------------------------------------------------
// The launch plan of the prompt / batch paths.  Which kernel instance a launch sequence runs is a pure function of the shape, the options
// and the call (plan_gemm, plan_attention below); the launchers carry out what it returns and decide nothing themselves, so that
// l2_debug_batch_plan -- no GPU, no context -- tells a CPU test exactly which instances a list of shapes reaches (tests/test_batch_plan_cpu.py,
// as l2_debug_pick_geo does for the decode GEMVs).
struct PlanShape { int d, h, hs, S; };
struct PlanOpts { bool exact, pf_f32, pf3, pf_attn; };      // L2_OPT_EXACT_ATTENTION, L2_OPT_PREFILL_F32_MFMA, the L2_PF3 / L2_PF_ATTN development switches
static PlanShape plan_shape(const l2_ctx* c) { return {c->d, c->h, c->hs, c->S}; }
static PlanOpts plan_opts(const l2_ctx* c) { return {c->opt_exact != 0, c->opt_pf_f32 != 0, c->pf3 != 0, c->pf_attn != 0}; }

// Shapes the 16x16 tiles and the vector attention kernel cover (a one-GPU context with one cache head per query head).
static bool plan_can_prefill(const PlanShape& s) { return (s.d % 16 == 0) && (s.h % 16 == 0) && (s.hs % 4 == 0) && s.hs <= 256; }
static bool can_prefill(const l2_ctx* c) { return !c->tp_path && c->kvd == c->d && plan_can_prefill(plan_shape(c)) && attn_vec(c); }

// Shapes the register-blocked GEMMs cover: whole batches of two 16-column blocks (n % 32) of both input widths (qkv's 3 d / 16 row
// tiles always come in threes).  stories15M (288 / 768) qualifies; the test shapes with hidden sizes like 176 keep the 16-row-tile kernels.
static bool plan_pf3(const PlanShape& s, const PlanOpts& o) { return o.pf3 && s.d % 32 == 0 && s.h % 32 == 0; }

// Rows of one launch sequence of the prompt paths: several 64-token chunks where the register-blocked GEMMs apply, else one.
static int plan_step(const PlanShape& s, const PlanOpts& o) { return plan_pf3(s, o) ? PF_S * PF_T : PF_T; }

// Which of the two a launch sequence's GEMMs go through.  PF_GEMM_PROMPT: l2_prefill, l2_seq_prefill, l2_seq_prefill_batch,
// l2_seq_score_batch and the mixed step (l2_step_batch, l2_step_batch_logprobs), pure-decode calls of it included.  PF_GEMM_BATCH:
// the batch step (l2_forward_batch, l2_decode_greedy_batch, l2_decode_sample_batch) and every row classifier.  They DIFFER at 33 .. 64 rows
// where plan_pf3: q / k / v is pf_gemm3_kernel<..., 3> under PROMPT and the 16-row-tile kernel under BATCH, and only PROMPT looks at
// L2_OPT_PREFILL_F32_MFMA -- kept as found; merging them changes which kernel a batch step launches and wants a
// measurement of its own.
enum PfGemm { PF_GEMM_PROMPT, PF_GEMM_BATCH };

// Token rows the kernels of a launch sequence of n rows see (whole 16-row MFMA tiles): `tt` tiles of 16 (1, 2 or 4) in a sequence of up to
// PF_T rows, else `chunks` whole chunks of PF_T (> 1 only on the register-blocked path).
struct PfTiles { int chunks, tt, nt; };
static PfTiles pf_tiles(int n) {
  const int chunks = (n + PF_T - 1) / PF_T, tt = (n > 32) ? 4 : (n > 16) ? 2 : 1;
  return {chunks, tt, (chunks > 1) ? chunks * PF_T : 16 * tt};
}

// One GEMM of a launch sequence.  PF_FAM_TILE: pf_gemm_kernel<mode, 4, tr> (tr = TT: tiles of 16 tokens, 1, 2 or 4), one 16-row weight tile
// per workgroup, four waves split K (the eight-wave instances spilled and were never launched: removed; the LDS-tile variant -- short
// chunks over row-major tensors only -- went in round 5: 8 instances, one of them at 256 VGPRs + 134 AGPRs, for chunks of at most 32 tokens).
// PF_FAM_REG: the register-blocked pf_gemm3_kernel<mode, 4, tr, 4, f32> (tr = RT: row tiles per wave), `chunks` 64-token chunks per launch.
enum { PF_FAM_TILE = 0, PF_FAM_REG = 1 };
struct GemmPick { int family, mode, tr, f32, chunks; };

// The GEMM `mode` (`rows` weight rows) of a launch sequence whose token rows are `t`, under policy g.
static GemmPick plan_gemm(const PlanShape& s, const PlanOpts& o, PfGemm g, int mode, int rows, const PfTiles& t) {
  const bool qkv = (mode == MODE_QKV || mode == MODE_QKV_ROWS);
  const int tiles = rows / 16;
  if (mode != MODE_CLS_ROWS && plan_pf3(s, o) && t.tt == 4) {
    if (g == PF_GEMM_BATCH) {
      // the register-blocked form where prefill takes it for one 64-row chunk (q / k / v keep the 16-row-tile kernel)
      if (!qkv) return {PF_FAM_REG, mode, 1, 0, 1};
    } else if (o.pf_f32) {
      // L2_OPT_PREFILL_F32_MFMA (opt-in): the same blocking on v_mfma_f32_16x16x4_f32 -- fp32 accumulate, NOT the reference's arithmetic.  A
      // result tile is four registers, not eight, and an MFMA takes 32 cycles, not 64: with the fp64 form's row tiles per wave the operand
      // fragments (re-read from L2 by every wave) would need ~24 B / clock / CU, so with FOUR chunks in the launch (enough workgroups either
      // way) a wave takes more row tiles: q / k / v four, w1 / w3 two pairs (7B, 256 tokens: 6 510 -> 6 940 tok/s); with fewer chunks the
      // fp64 form's counts (more tiles per wave at 128 tokens left CUs idle: 5 520 -> 4 910)
      if (qkv) return {PF_FAM_REG, mode, (t.chunks == 4 && tiles % 4 == 0) ? 4 : 3, 1, t.chunks};
      if (mode == MODE_W13) return {PF_FAM_REG, mode, (t.chunks == 4 && tiles % 2 == 0) ? 2 : 1, 1, t.chunks};
      return {PF_FAM_REG, mode, (t.chunks == 4 && tiles % 4 == 0) ? 4 : (t.chunks == 2 && tiles % 2 == 0) ? 2 : 1, 1, t.chunks};
    } else {
      // row tiles per wave: conversions per MFMA are 16 (R + 64) / (64 R) for R rows per workgroup, so as many as still leave >= 256
      // workgroups: qkv 3 (3 d / 16 tiles), w1 / w3 one pair (688 pairs at 7B), wo / w2 (d / 16 tiles) 1, 2 or 4 with the chunk count
      if (qkv) return {PF_FAM_REG, mode, 3, 0, t.chunks};      // (QKV_ROWS: packed prompts, batch_host.hip.h)
      if (mode == MODE_W13) return {PF_FAM_REG, mode, 1, 0, t.chunks};
      return {PF_FAM_REG, mode, (t.chunks == 4 && tiles % 4 == 0) ? 4 : (t.chunks == 2 && tiles % 2 == 0) ? 2 : 1, 0, t.chunks};
    }
  }
  return {PF_FAM_TILE, mode, t.tt, 0, 1};
}

// register-blocked form (prefill.hip.h: pf_gemm3_kernel): RT row tiles per wave, 4 waves split K, `chunks` 64-token chunks per launch
template <int MODE, int RT, bool F32 = false>
static void launch_pf3(const PfArgs& a, int chunks, hipStream_t st) {
  constexpr int NW = 4;
  const size_t lds = (size_t)4 * NW * 4 * 64 * (F32 ? 4 : 8);
  hipLaunchKernelGGL((pf_gemm3_kernel<MODE, NW, RT, 4, F32>), dim3(a.rows / (16 * RT), chunks), dim3(64 * NW), lds, st, a);
}

// The instances of pf_gemm3_kernel the library holds: exactly the points plan_gemm can return (tests/test_batch_plan_cpu.py holds the two
// to each other: every selected instance exists, none exists that nothing selects).
template <int MODE, int RT, bool F32>
static constexpr bool pf3_built() {
  if (MODE == MODE_QKV || MODE == MODE_QKV_ROWS) return F32 ? (RT == 3 || RT == 4) : RT == 3;
  if (MODE == MODE_W13) return F32 ? (RT == 1 || RT == 2) : RT == 1;
  if (MODE == MODE_WO || MODE == MODE_W2) return RT == 1 || RT == 2 || RT == 4;
  return false;
}

// Launch what plan_gemm picked.  A pick the library holds no instance of is an error, never another kernel.
template <int MODE>
static hipError_t launch_gemm(const PfArgs& a, const GemmPick& g, hipStream_t st) {
  if (g.mode != MODE) return hipErrorInvalidValue;
  if (g.family == PF_FAM_TILE) {
    const dim3 grid((a.rows + 15) / 16);
    if (g.tr == 4) hipLaunchKernelGGL((pf_gemm_kernel<MODE, 4, 4>), grid, dim3(256), 0, st, a);
    else if (g.tr == 2) hipLaunchKernelGGL((pf_gemm_kernel<MODE, 4, 2>), grid, dim3(256), 0, st, a);
    else if (g.tr == 1) hipLaunchKernelGGL((pf_gemm_kernel<MODE, 4, 1>), grid, dim3(256), 0, st, a);
    else return hipErrorInvalidValue;
    return hipSuccess;
  }
#define L2_PF3(RT, F32) if (g.tr == RT && (g.f32 != 0) == F32) { if constexpr (pf3_built<MODE, RT, F32>()) { launch_pf3<MODE, RT, F32>(a, g.chunks, st); return hipSuccess; } }
  L2_PF3(1, false) L2_PF3(2, false) L2_PF3(3, false) L2_PF3(4, false)
  L2_PF3(1, true) L2_PF3(2, true) L2_PF3(3, true) L2_PF3(4, true)
#undef L2_PF3
  return hipErrorInvalidValue;
}

// Attention of a launch sequence.  AT_PF_MFMA / AT_BP_MFMA: 16 queries per workgroup on the fp64 MFMA (pf_attn_mfma_kernel<a> for one
// sequence's run, bp_attn_mfma_kernel<a> over ragged tiles; a = head size, 64 or 128), its longest tile needing `lds` bytes.  AT_PF_TILE /
// AT_BT_TILE: the decode kernel per (head, row) (pf_attn_tile_kernel<a, nw, nt> / bt_attn_tile_kernel<a, nw, nt>, a = lanes per cache row):
// other head sizes, the exact accumulate, very long contexts, and the decode rows of a mixed step.  `rows`: the rows it covers, the
// launch sequence's first `rows` for the decode form, the rest for the tiles.
// The rows form's template point <lr, nw, nt> (launch.hip.h: attn_lr, launch_attn_tile): 4 waves x 16 tiles for heads up to 64 floats and
// beyond 128, 8 waves x 8 tiles for 65 .. 128.  The decode step's launcher keeps its own text; prefill_chunk holds the two to each other.
struct AttnTilePick { int lr, nw, nt; };
static AttnTilePick attn_tile_pick(int hs) { const int nw = (hs > 64 && hs <= 128) ? 8 : 4; return {attn_lr(hs), nw, nw == 8 ? 8 : 16}; }      // (lr: launch.hip.h's own attn_lr)

enum { AT_PF_MFMA = 0, AT_BP_MFMA = 1, AT_PF_TILE = 2, AT_BT_TILE = 3 };
enum PlanCall { CALL_PROMPT = 0, CALL_PACKED = 1, CALL_BATCH = 2 };      // prefill_chunk; bp_enqueue; bt_forward
struct AttnPick { int family, a, nw, nt, rows; size_t lds; };
static bool plan_attn_mfma(const PlanShape& s, const PlanOpts& o, size_t lds) { return o.pf_attn && !o.exact && (s.hs == 64 || s.hs == 128) && lds <= 150 * 1024; }

// The attention launches (one or two: `out`) of a launch sequence of m rows, the first nd of them decode rows (CALL_PACKED: the mixed
// step), whose longest 16-row tile ends at position last_pos (padding rows included).
static int plan_attention(const PlanShape& s, const PlanOpts& o, int call, int m, int nd, int last_pos, AttnPick out[2]) {
  const AttnTilePick tp = attn_tile_pick(s.hs);
  const size_t tlds = attn_tile_lds(s.S, 1, tp.nw, tp.nt), mlds = pf_attn_lds(last_pos);
  if (call == CALL_BATCH) { out[0] = {AT_BT_TILE, tp.lr, tp.nw, tp.nt, m, tlds}; return 1; }
  const bool mfma = plan_attn_mfma(s, o, mlds);
  if (call == CALL_PROMPT) {
    out[0] = mfma ? AttnPick{AT_PF_MFMA, s.hs, 4, 0, m, mlds} : AttnPick{AT_PF_TILE, tp.lr, tp.nw, tp.nt, m, tlds};
    return 1;
  }
  int k = 0;
  const int nrow = mfma ? nd : m;
  if (nrow > 0) out[k++] = {AT_BT_TILE, tp.lr, tp.nw, tp.nt, nrow, tlds};
  if (mfma && m > nd) out[k++] = {AT_BP_MFMA, s.hs, 4, 0, m - nd, mlds};
  return k;
}

// What a launch sequence would run (pure: no context, no GPU).  call: 0 one sequence's prompt run (l2_prefill, l2_seq_prefill), 1 packed
// rows (l2_seq_prefill_batch, l2_seq_score_batch, l2_step_batch), 2 the batch step; policy: 0 PF_GEMM_PROMPT, 1 PF_GEMM_BATCH; m rows, the
// first nd of them decode rows; last_pos: the last position of the longest 16-row tile (prompt: pos0 + m rounded up to 16, less one; packed:
// the highest tile's first position + 15); flags: 1 exact attention, 2 fp32 MFMA, 4 L2_PF3, 8 L2_PF_ATTN.  out:
//   [0] the shape reaches the prompt kernels  [1] rows of a launch sequence (64 / 256)  [2] chunks  [3] tiles of 16 (tt)  [4] rows the kernels
//   see  [5] valid rows of the last 16-row tile  [6] attention launches;  [8 + 5 g ...] GEMM g (q/k/v, wo, w1/w3, w2, the row classifier over a
//   slice of min(m, 64) rows): family, MODE, TT or RT, F32, chunks;  [33 + 6 k ...] attention launch k: family, HS or LR, NW, NT, rows, LDS bytes.
extern "C" int l2_debug_batch_plan(int d, int h, int hs, int seq_len, int call, int policy, int m, int nd, int last_pos, int flags, int out[48]) {
  if (!out || d <= 0 || h <= 0 || hs <= 0 || seq_len <= 0 || call < CALL_PROMPT || call > CALL_BATCH || policy < 0 || policy > 1) return L2_E_ARG;
  const PlanShape s = {d, h, hs, seq_len};
  const PlanOpts o = {(flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0};
  for (int i = 0; i < 48; ++i) out[i] = 0;
  out[0] = plan_can_prefill(s); out[1] = plan_step(s, o);
  if (!out[0]) return L2_OK;
  if (m < 1 || m > (call == CALL_BATCH ? (int)PF_T : out[1]) || nd < 0 || nd > m || last_pos < 0) return L2_E_ARG;
  const PfGemm g = policy ? PF_GEMM_BATCH : PF_GEMM_PROMPT;
  const PfTiles t = pf_tiles(m);
  out[2] = t.chunks; out[3] = t.tt; out[4] = t.nt; out[5] = (m - 1) % 16 + 1;
  const int qkv = call == CALL_PROMPT ? MODE_QKV : MODE_QKV_ROWS;
  const GemmPick gp[5] = {plan_gemm(s, o, g, qkv, 3 * d, t), plan_gemm(s, o, g, MODE_WO, d, t), plan_gemm(s, o, g, MODE_W13, h, t),
                          plan_gemm(s, o, g, MODE_W2, d, t), plan_gemm(s, o, PF_GEMM_BATCH, MODE_CLS_ROWS, 16, pf_tiles(m < PF_T ? m : (int)PF_T))};
  for (int i = 0; i < 5; ++i) { int* p = out + 8 + 5 * i; p[0] = gp[i].family; p[1] = gp[i].mode; p[2] = gp[i].tr; p[3] = gp[i].f32; p[4] = gp[i].chunks; }
  AttnPick ap[2];
  out[6] = plan_attention(s, o, call, m, nd, last_pos, ap);
  for (int k = 0; k < out[6]; ++k) { int* p = out + 33 + 6 * k; p[0] = ap[k].family; p[1] = ap[k].a; p[2] = ap[k].nw; p[3] = ap[k].nt; p[4] = ap[k].rows; p[5] = (int)ap[k].lds; }
  return L2_OK;
}

// The weights of one prompt GEMM: the row-major tensors of layer l, or -- once they have been given back (one copy of the weights:
// ensure_packed) -- the decode step's repacked copy of this phase with the geometry it was packed for.
template <int MODE>
static void pf_weights(const l2_ctx* c, int l, PfArgs& a, int k0, int k1, int k2) {
  a.w0 = a.w1 = a.w2 = nullptr; a.wp = nullptr; a.pk_wstride = 0; a.pk_groups = 0;
  if (c->released[k0]) {
    const l2_ctx::Packed& p = c->packed[MODE];
    a.wp = p.buf + p.layer_elems * (size_t)l;
    a.pk_wstride = p.grid * p.nwaves;
    a.pk_groups = (int)(p.layer_elems / (2 * (size_t)(MODE == MODE_W2 ? c->h : c->d)));      // layer_elems = groups * 2 rows * n
    return;
  }
  a.w0 = c->w[k0] + c->layer_elems[k0] * l;
  if (k1 >= 0) a.w1 = c->w[k1] + c->layer_elems[k1] * l;
  if (k2 >= 0) a.w2 = c->w[k2] + c->layer_elems[k2] * l;
}

// An activation set (ctx.hip.h: PfActs) of PF_S * PF_T rows, allocated at its first use.
static int pf_acts_ensure(const l2_ctx* c, PfActs& A) {
  if (A.x) return L2_OK;
  const size_t d = c->d, h = c->h, ROWS = (size_t)PF_S * PF_T;
  HIPCHK(hipMalloc(&A.x, ROWS * d * 4)); HIPCHK(hipMalloc(&A.xn, ROWS * (d > h ? d : h) * 4));
  HIPCHK(hipMalloc(&A.q, ROWS * d * 4)); HIPCHK(hipMalloc(&A.xb, ROWS * d * 4)); HIPCHK(hipMalloc(&A.hb, ROWS * h * 4));
  HIPCHK(hipMemset(A.xb, 0, ROWS * d * 4)); HIPCHK(hipMemset(A.q, 0, ROWS * d * 4));
  return L2_OK;
}

// Where the rows of a launch sequence sit in the caches: row t at position pos0 + t of one sequence's slabs (PfRun: MODE_QKV), or each row at
// its own (sequence, position) of the row tables (AttnRows, its loff filled per layer: MODE_QKV_ROWS).
struct PfRun { int pos0; float *kc, *vc; };
static void pf_address(PfArgs& a, const PfRun& r, size_t loff) { a.pos0 = r.pos0; a.kc = r.kc + loff; a.vc = r.vc + loff; }
static void pf_address(PfArgs& a, const AttnRows& r, size_t loff) { a.row_seq = r.seq; a.row_pos = r.pos; a.seq_kc = r.kc; a.seq_vc = r.vc; a.seq_loff = loff; }

template <PfGemm G, int MODE>
static hipError_t pf_gemm(const l2_ctx* c, const PfArgs& a, const PfTiles& t, hipStream_t st) {
  return launch_gemm<MODE>(a, plan_gemm(plan_shape(c), plan_opts(c), G, MODE, a.rows, t), st);
}

// pf_attn_mfma_kernel / bp_attn_mfma_kernel (k64 / k128: its two head sizes) with `lds` bytes of LDS.
template <class Args>
static int launch_attn_mfma(const AttnPick& at, void (*k64)(Args), void (*k128)(Args), dim3 grid, const Args& a, hipStream_t st) {
  if (at.a != 64 && at.a != 128) return fail(L2_E_HIP, "no MFMA attention instance for head size %d", at.a);
  void (*k)(Args) = at.a == 128 ? k128 : k64;
  LCHK(lds_opt_in(k, at.lds));
  hipLaunchKernelGGL(k, grid, dim3(256), at.lds, st, a);
  LCHK(hipGetLastError());
  return L2_OK;
}

// THE launch sequence: embed and every layer over m rows (tokens `tok`, on the device) of the activation set A, every GEMM seeing all of
// them.  `rows`: where they sit in the caches (above; its type picks the q / k / v epilogue).  G: the GEMM policy (PfGemm).  attn(l, loff):
// the caller's attention of layer l, A.q -> A.xb, the layer's slab starting loff floats into a sequence's cache; returns an L2 code.
template <PfGemm G, class Rows, class Attn>
static int pf_layers(const l2_ctx* c, const PfActs& A, const int* tok, int m, const Rows& rows, const Attn& attn, hipStream_t st) {
  constexpr int QKV = std::is_same<Rows, AttnRows>::value ? MODE_QKV_ROWS : MODE_QKV;
  const PfTiles t = pf_tiles(m);
  const size_t d = c->d;
  hipLaunchKernelGGL(pf_embed_kernel, dim3(t.nt), dim3(256), 0, st, A.x, c->w[L2_T_TOKEN_EMBEDDING], tok, c->d, m);
  LCHK(hipGetLastError());
  for (int l = 0; l < c->L; ++l) {
    const size_t loff = (size_t)l * c->S * c->d;
    PfArgs a;
    memset(&a, 0, sizeof(a));
    a.fr = c->w[L2_T_FREQ_REAL]; a.fi = c->w[L2_T_FREQ_IMAG]; a.head_size = c->hs; a.dim = c->d; a.nvalid = m;
    a.x = A.x;
    pf_address(a, rows, loff);
    // rmsnorm + q,k,v + RoPE + every row's cache row (llama2.ts:216-240)
    hipLaunchKernelGGL(pf_norm_kernel, dim3(t.nt), dim3(256), 0, st, A.xn, A.x, c->w[L2_T_RMS_ATT] + d * l, c->d);
    pf_weights<MODE_QKV>(c, l, a, L2_T_WQ, L2_T_WK, L2_T_WV);
    a.xin = A.xn; a.out = A.q; a.n = c->d; a.rows = 3 * c->d;
    LCHK((pf_gemm<G, QKV>(c, a, t, st)));
    LCHK(hipGetLastError());
    // attention (llama2.ts:244-267)
    const int rc = attn(l, loff);
    if (rc) return rc;
    // wo + residual (llama2.ts:270-273)
    pf_weights<MODE_WO>(c, l, a, L2_T_WO, -1, -1); a.xin = A.xb; a.n = c->d; a.rows = c->d;
    LCHK((pf_gemm<G, MODE_WO>(c, a, t, st)));
    // rmsnorm + w1,w3 + SwiGLU (llama2.ts:276-289)
    hipLaunchKernelGGL(pf_norm_kernel, dim3(t.nt), dim3(256), 0, st, A.xn, A.x, c->w[L2_T_RMS_FFN] + d * l, c->d);
    pf_weights<MODE_W13>(c, l, a, L2_T_W1, L2_T_W3, -1);
    a.xin = A.xn; a.out = A.hb; a.n = c->d; a.rows = c->h;
    LCHK((pf_gemm<G, MODE_W13>(c, a, t, st)));
    // w2 + residual (llama2.ts:292-295)
    pf_weights<MODE_W2>(c, l, a, L2_T_W2, -1, -1); a.xin = A.hb; a.n = c->h; a.rows = c->d;
    LCHK((pf_gemm<G, MODE_W2>(c, a, t, st)));
    LCHK(hipGetLastError());
  }
  return L2_OK;
}

// One launch sequence for up to PF_S chunks of PF_T prompt positions (n tokens at pos0 ...).  `kc` / `vc`: the sequence's cache slabs
// ([L][S][d]; l2_prefill: the context's own, l2_seq_prefill: a reserved sequence's).
static int prefill_chunk(l2_ctx* c, const int32_t* tokens, int n, int pos0, float* kc, float* vc) {
  hipStream_t st = c->stream;
  constexpr size_t ROWS = (size_t)PF_S * PF_T;
  int rc = pf_acts_ensure(c, c->pf);
  if (rc) return rc;
  if (!c->pf_tok) HIPCHK(hipMalloc(&c->pf_tok, ROWS * sizeof(int)));
  int32_t tk[ROWS] = {0};
  for (int i = 0; i < n; ++i) tk[i] = tokens[i];
  HIPCHK(hipMemcpyAsync(c->pf_tok, tk, sizeof(tk), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));   // tk is on the stack
  AttnPick ap[2];
  plan_attention(plan_shape(c), plan_opts(c), CALL_PROMPT, n, 0, pos0 + ((n + 15) & ~15) - 1, ap);
  const AttnPick at = ap[0];
  const auto attn = [&](int l, size_t loff) -> int {
    if (at.family == AT_PF_MFMA) {      // 16 queries per workgroup on the fp64 MFMA (prefill.hip.h: pf_attn_mfma_kernel)
      PfAttnArgs pa;
      pa.q = c->pf.q; pa.kc = kc + loff; pa.vc = vc + loff; pa.xb = c->pf.xb;
      pa.dim = c->d; pa.head_size = c->hs; pa.seq_len = c->S; pa.pos0 = pos0; pa.nvalid = n;
      pa.inv_sqrt_hs = 1.0 / sqrt((double)c->hs);
      return launch_attn_mfma(at, pf_attn_mfma_kernel<64>, pf_attn_mfma_kernel<128>, dim3(c->H, (n + 15) / 16), pa, st);
    }
    // one workgroup per (head, query): the decode kernel, through the decode step's launcher -- which must take the planned instance
    const int lnw = attn_nw(c), lnt = lnw == 8 ? 8 : 16;      // (launch_attn_tile's own waves and tiles)
    if (at.family != AT_PF_TILE || at.nw != lnw || at.nt != lnt || at.lds != attn_tile_lds(c->S, 1, lnw, lnt))
      return fail(L2_E_HIP, "prompt attention: the plan and launch_attn_tile disagree");
    AttnArgs aa;
    c->cur_splits = 1; c->cur_fused = false;
    fill_attn_args(c, l, aa);
    aa.q = c->pf.q; aa.xb = c->pf.xb; aa.att = nullptr; aa.pos_plus1 = 1; aa.kc = kc + loff; aa.vc = vc + loff;
    LCHK(launch_attn_tile(c, aa, n, pos0, st));
    return L2_OK;
  };
  return pf_layers<PF_GEMM_PROMPT>(c, c->pf, c->pf_tok, n, PfRun{pos0, kc, vc}, attn, st);
}

extern "C" int l2_prefill(l2_ctx* c, const int32_t* tokens, int n_tokens, int pos0, float* logits_out) {
  if (!c || !tokens) return fail(L2_E_ARG, "null argument");
  if (n_tokens <= 0 || pos0 < 0 || pos0 + n_tokens > c->S) return fail(L2_E_ARG, "positions %d..%d outside [0, seq_len=%d)", pos0, pos0 + n_tokens - 1, c->S);
  for (int i = 0; i < n_tokens; ++i) if (tokens[i] < 0 || tokens[i] >= c->V) return fail(L2_E_ARG, "token %d outside [0, vocab_size=%d)", tokens[i], c->V);
  int rc = ensure_ready(c);
  if (rc) return rc;
  // a single token: the decode step streams the weights once at full rate; the 16-token tile pass does not (7.7 against 4.3 ms at 7B)
  if (n_tokens == 1 || !can_prefill(c)) {   // and shapes the 16x16 tiles do not cover: the reference's own one-token-per-call loop
    for (int i = 0; i < n_tokens; ++i) { rc = l2_forward(c, tokens[i], pos0 + i, (i == n_tokens - 1) ? logits_out : nullptr); if (rc) return rc; }
    return L2_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  if (c->opt_pos_check && pos0 != 0 && pos0 > c->next_pos)
    return fail(L2_E_STATE, "L2_CHECK_POS: pos %d skips ahead of the sequence (cache rows 0 .. %d have been written)", pos0, c->next_pos - 1);
  if (pos0 + n_tokens > c->next_pos || pos0 == 0) c->next_pos = pos0 + n_tokens;
  const int step = plan_step(plan_shape(c), plan_opts(c));      // positions per launch sequence: several 64-token chunks where the register-blocked GEMMs apply
  int done = 0;
  while (done < n_tokens) {
    const int n = (n_tokens - done < step) ? n_tokens - done : step;
    rc = prefill_chunk(c, tokens + done, n, pos0 + done, c->kc, c->vc);
    if (rc) return rc;
    done += n;
  }
  // logits of the last position only (llama2.ts:299-302): the decode classifier on the last row of the chunk
  const int last = (n_tokens - 1) % step;
  c->h_tokpos[0] = tokens[n_tokens - 1]; c->h_tokpos[1] = pos0 + n_tokens - 1; c->h_tokpos[2] = 0; c->h_tokpos[3] = 0;
  HIPCHK(hipMemcpyAsync(c->tokpos, c->h_tokpos, 4 * sizeof(int), hipMemcpyHostToDevice, c->stream));
  PhaseArgs a = cls_args(c, true);
  a.in = c->pf.x + (size_t)last * c->d;
  LCHK(launch_phase<MODE_CLS>(c, a, c->stream));
  if (!(c->opt_zero_copy && !c->tp_path))
    HIPCHK(hipMemcpyAsync(c->h_logits, c->logits, (size_t)c->V * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->ran_forward = true;
  if (logits_out) memcpy(logits_out, c->h_logits, (size_t)c->V * 4);
  return L2_OK;
}
