// batch_host.hip.h -- host side of batched decode (batch.hip.h): l2_seq_reserve, l2_seq_prefill, l2_seq_prefill_batch, l2_forward_batch,
// l2_decode_greedy_batch, l2_decode_sample_batch, l2_step_batch, l2_seq_score_batch, l2_step_batch_logprobs, l2_step_batch_constrained,
// l2_step_batch_sampling, l2_debug_sample_controls, l2_read_seq_cache, l2_seq_fork.
// The batch step (bt_forward) and the packed launch sequences (bp_enqueue) are prefill_host.hip.h's pf_layers with row tables, their own
// activation sets and attention; what they share -- argument checks, the row classifier, the decode-form attention, the row sampler's
// staging and read-back -- is one helper each, here.
// Part of the one translation unit llama2_hip.hip (included there, in order); not a stand-alone header.
#pragma once

enum { BT_MAX = 64 };   // rows of a batch step: four 16-row MFMA tiles
enum { BP_ROWS = PF_S * PF_T };   // prompt rows of one packed launch sequence (l2_seq_prefill_batch)

// Independent sequences sharing the context's weights.  Sequence 0's caches are the context's own (c->kc / c->vc); the others are
// allocated by l2_seq_reserve.  The batch step has activations and tables of its own: the single-sequence state (RunState buffers,
// tokpos, recorded graphs, AQL programs) is never touched by it.
struct BatchState {
  int n_seqs = 0;
  std::vector<float*> kc, vc;             // [n_seqs] cache slabs ([L][S][d] each); entry 0 = the context's own
  std::vector<int> next_pos;              // L2_OPT_CHECK_POS, sequences 1 ..; sequence 0 uses c->next_pos
  float** d_kc = nullptr;                 // device copies of kc / vc (the kernels index them by sequence)
  float** d_vc = nullptr;
  int* tab = nullptr;                     // device [4][BT_MAX]: sequence, token, position, start position of every row
  int* h_tab = nullptr;                   // pinned staging of tab
  int* out = nullptr;                     // device [BT_MAX][S]: tokens picked by row r at position p -> out[r][p - start[r]]
  PfActs act;                             // [BT_MAX] rows: the batch step's activations
  float* logits = nullptr;                // [BT_MAX][V]
  hipGraphExec_t g[BT_MAX + 1] = {};      // the recorded step per row count
  hipGraphExec_t gs[BT_MAX + 1] = {};     // the recorded sampled step per row count (forward + row sampler + bt_pick_kernel)
  l2s::RowSampler* smp = nullptr;         // the row sampler's buffers: allocated at the first l2_decode_sample_batch
  unsigned long long smp_stats[2] = {};   // {tokens sampled, of those by the serial loop} over every l2_decode_sample_batch
  std::vector<uintptr_t> sig;             // what the recorded steps baked in (weight addresses, options)
  // Packed prompts (l2_seq_prefill_batch), allocated at its first call: activations of one launch sequence, and the call's tables
  PfActs pact;                            // [BP_ROWS] rows
  int* ptab = nullptr;                    // device: bp_tables' layout, ptab_cap ints
  size_t ptab_cap = 0;
  // Log-probabilities (logprob.hip.h), allocated at the first call that asks for them
  float* slogits = nullptr;               // [BP_ROWS][V]: the logits of every row of one packed launch sequence (l2_seq_score_batch)
  char* lpbuf = nullptr;                  // device: a call's targets and outputs (lp_bufs' layout), lpbuf_cap bytes
  size_t lpbuf_cap = 0;
  // Constrained picks (constrain.hip.h), allocated at the first call that carries a mask or a bias list
  unsigned* csbuf = nullptr;              // device: a call's row tables, masks and bias pairs (cs_tables' layout), csbuf_cap words
  size_t csbuf_cap = 0;
  // Sampling controls (controls.hip.h), allocated at the first call that penalises or truncates a row
  char* scbuf = nullptr;                  // device: a call's control tables and history ids (sc_tables' layout), scbuf_cap bytes
  size_t scbuf_cap = 0;
  int* sccount = nullptr;                 // [BT_MAX][V] occurrence counts of the penalty launch: zeroed here once, left zero by every launch
  float* tlogits = nullptr;               // [BT_MAX][V] the rows as the row sampler reads them when some row truncates (x'')
  int* seq_of() const { return tab; }
  int* tok_of() const { return tab + BT_MAX; }
  int* pos_of() const { return tab + 2 * BT_MAX; }
  int* start_of() const { return tab + 3 * BT_MAX; }
};

static void bt_drop_graphs(BatchState* b) {
  for (auto& g : b->g) if (g) { hipGraphExecDestroy(g); g = nullptr; }
  for (auto& g : b->gs) if (g) { hipGraphExecDestroy(g); g = nullptr; }
}

static void batch_free(l2_ctx* c) {
  BatchState* b = c->bt;
  if (!b) return;
  bt_drop_graphs(b);
  for (size_t s = 1; s < b->kc.size(); ++s) { if (b->kc[s]) hipFree(b->kc[s]); if (b->vc[s]) hipFree(b->vc[s]); }
  void* dev[] = {b->d_kc, b->d_vc, b->tab, b->out, b->act.x, b->act.xn, b->act.q, b->act.xb, b->act.hb, b->logits, b->pact.x, b->pact.xn, b->pact.q,
                 b->pact.xb, b->pact.hb, b->ptab, b->slogits, b->lpbuf, b->csbuf, b->scbuf, b->sccount, b->tlogits};
  for (void* p : dev) if (p) hipFree(p);
  if (b->h_tab) hipHostFree(b->h_tab);
  if (b->smp) { l2s::destroy_rows(b->smp); delete b->smp; }
  delete b;
  c->bt = nullptr;
}

// The shapes the batch path covers: those of the prompt GEMMs (prefill_host.hip.h: can_prefill), named one by one.
static const char* bt_refusal(const l2_ctx* c) {
  if (c->tp_path) return "tensor-parallel contexts are not covered by the batch path";
  if (c->KVH != c->H || c->kvd != c->d) return "grouped-query attention (n_kv_heads < n_heads honoured) is not covered by the batch path";
  if (c->d % 16) return "dim is not a multiple of 16 (the MFMA tiles of the batch GEMMs)";
  if (c->h % 16) return "hidden_dim is not a multiple of 16 (the MFMA tiles of the batch GEMMs)";
  if (!can_prefill(c)) return "head_size is not a multiple of 4 or exceeds 256 (the vector attention kernel)";
  return nullptr;
}

extern "C" int l2_seq_reserve(l2_ctx* c, int n_seqs) {
  if (!c) return fail(L2_E_ARG, "null context");
  if (n_seqs < 1 || n_seqs > BT_MAX) return fail(L2_E_ARG, "n_seqs %d outside [1, %d]", n_seqs, (int)BT_MAX);
  if (c->bt) return fail(L2_E_STATE, "l2_seq_reserve was already called on this context (%d sequences)", c->bt->n_seqs);
  if (const char* why = bt_refusal(c)) return fail(L2_E_CONFIG, "%s", why);
  HIPCHK(hipSetDevice(c->device));
  BatchState* b = new BatchState();
  c->bt = b;
  b->n_seqs = n_seqs;
  b->kc.assign(n_seqs, nullptr); b->vc.assign(n_seqs, nullptr); b->next_pos.assign(n_seqs, 0);
  b->kc[0] = c->kc; b->vc[0] = c->vc;
  const size_t slab = (size_t)c->L * c->S * c->d * sizeof(float), R = BT_MAX, wide = (size_t)(c->d > c->h ? c->d : c->h);
  bool ok = true;
  auto dev = [&](void** p, size_t bytes) { if (ok && hipMalloc(p, bytes) != hipSuccess) ok = false; if (ok) ok = hipMemset(*p, 0, bytes) == hipSuccess; };
  for (int s = 1; s < n_seqs; ++s) { dev((void**)&b->kc[s], slab); dev((void**)&b->vc[s], slab); }
  dev((void**)&b->d_kc, R * sizeof(float*)); dev((void**)&b->d_vc, R * sizeof(float*));
  dev((void**)&b->tab, 4 * R * sizeof(int)); dev((void**)&b->out, R * c->S * sizeof(int));
  dev((void**)&b->act.x, R * c->d * 4); dev((void**)&b->act.xn, R * wide * 4); dev((void**)&b->act.q, R * c->d * 4);
  dev((void**)&b->act.xb, R * c->d * 4); dev((void**)&b->act.hb, R * c->h * 4); dev((void**)&b->logits, R * c->V * 4);
  if (ok && hipHostMalloc((void**)&b->h_tab, 4 * R * sizeof(int), 0) != hipSuccess) ok = false;
  if (ok) {
    float* tk[BT_MAX] = {}; float* tv[BT_MAX] = {};
    for (int s = 0; s < n_seqs; ++s) { tk[s] = b->kc[s]; tv[s] = b->vc[s]; }
    ok = hipMemcpy(b->d_kc, tk, sizeof(tk), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(b->d_vc, tv, sizeof(tv), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    const hipError_t e = hipGetLastError();
    batch_free(c);
    return fail(L2_E_HIP, "l2_seq_reserve: device memory for %d sequences: %s", n_seqs, hipGetErrorString(e));
  }
  return L2_OK;
}

// A sequence's next position (L2_OPT_CHECK_POS: cache rows 0 .. next - 1 have been written); sequence 0's is the context's own.
static int bt_next(const l2_ctx* c, int s) { return s == 0 ? c->next_pos : c->bt->next_pos[s]; }
static void bt_set_next(l2_ctx* c, int s, int next) { if (s == 0) c->next_pos = next; else c->bt->next_pos[s] = next; }

// What every batch call checks first: the context, its arrays (`arrays`: all of them given), the reserved sequences, n.
static int bt_check_call(const l2_ctx* c, bool arrays, int n) {
  if (!c) return fail(L2_E_ARG, "null context");
  if (!arrays) return fail(L2_E_ARG, "null argument");
  if (!c->bt) return fail(L2_E_STATE, "no sequences reserved: call l2_seq_reserve first");
  if (n < 1 || n > c->bt->n_seqs) return fail(L2_E_ARG, "n = %d outside [1, n_seqs = %d]", n, c->bt->n_seqs);
  return L2_OK;
}

// Row i of a call names sequence s: a reserved one, named by no earlier row (`seen`, [BT_MAX]).
static int bt_check_seq(const BatchState* b, bool* seen, int i, int s) {
  if (s < 0 || s >= b->n_seqs) return fail(L2_E_ARG, "row %d: sequence %d outside [0, n_seqs = %d)", i, s, b->n_seqs);
  if (seen[s]) return fail(L2_E_ARG, "row %d: sequence %d appears twice in one call", i, s);
  seen[s] = true;
  return L2_OK;
}

// L2_CHECK_POS: a call may rewind or restart sequence s, not skip ahead of what it has written.
static int bt_check_pos(const l2_ctx* c, int s, int pos) {
  const int next = bt_next(c, s);
  if (c->opt_pos_check && pos != 0 && pos > next)
    return fail(L2_E_STATE, "L2_CHECK_POS: sequence %d, pos %d skips ahead of the sequence (cache rows 0 .. %d have been written)", s, pos, next - 1);
  return L2_OK;
}

// Arguments of a batch call, all checked before anything touches the GPU.
static int bt_check(l2_ctx* c, int n, const int32_t* seqs, const int32_t* tokens, const int32_t* pos, int steps) {
  if (int rc = bt_check_call(c, seqs && tokens && pos, n)) return rc;
  if (steps < 0) return fail(L2_E_ARG, "steps %d < 0", steps);
  bool seen[BT_MAX] = {};
  for (int i = 0; i < n; ++i) {
    if (int rc = bt_check_seq(c->bt, seen, i, seqs[i])) return rc;
    if (tokens[i] < 0 || tokens[i] >= c->V) return fail(L2_E_ARG, "row %d: token %d outside [0, vocab_size=%d)", i, tokens[i], c->V);
    if (pos[i] < 0 || pos[i] >= c->S) return fail(L2_E_ARG, "row %d: pos %d outside [0, seq_len=%d)", i, pos[i], c->S);
    if (pos[i] + (steps > 0 ? steps : 1) > c->S) return fail(L2_E_ARG, "row %d: pos %d + steps %d runs past seq_len=%d", i, pos[i], steps, c->S);
    if (int rc = bt_check_pos(c, seqs[i], pos[i])) return rc;
  }
  return L2_OK;
}

// Per-row sampling settings (null: every row greedy): no NaN, and -- when a row draws (*any) -- a vocabulary the row sampler can hold.
static int bt_check_sampling(const l2_ctx* c, int n, const double* temperature, const double* topp, bool* any) {
  *any = false;
  for (int i = 0; temperature && i < n; ++i) {
    if (!(temperature[i] == temperature[i]) || !(topp[i] == topp[i])) return fail(L2_E_ARG, "row %d: temperature / topp is NaN", i);
    if (temperature[i] != 0.0) *any = true;
  }
  if (*any && c->V > l2s::MAX_VOCAB) return fail(L2_E_CONFIG, "device sampler supports vocabularies up to %d", (int)l2s::MAX_VOCAB);
  return L2_OK;
}

// Weights of the batch classifier: the row-major matrix (wcls, or the embedding table when shared), or -- once wcls has been given back
// -- the decode classifier's repacked copy.
static void bt_cls_weights(const l2_ctx* c, PfArgs& a) {
  a.w0 = a.w1 = a.w2 = nullptr; a.wp = nullptr; a.pk_wstride = 0; a.pk_groups = 0;
  if (!c->shared && c->released[L2_T_WCLS]) {
    const l2_ctx::Packed& p = c->packed[MODE_CLS];
    a.wp = p.buf; a.pk_wstride = p.grid * p.nwaves; a.pk_groups = (int)(p.layer_elems / (2 * (size_t)c->d));
    return;
  }
  a.w0 = c->w[L2_T_WCLS];
}

static hipError_t launch_bt_attn(const l2_ctx* c, const AttnArgs& a, const AttnRows& r, int n, hipStream_t st) {
  const AttnTilePick t = attn_tile_pick(c->hs);
  const size_t lds = attn_tile_lds(c->S, 1, t.nw, t.nt);
  const dim3 grid(c->H, n), block(64 * t.nw);
#define L2_BT(LR, NW, NT) do { if (t.nw != NW || t.nt != NT) return hipErrorInvalidValue; \
                               hipError_t e_ = lds_opt_in(&bt_attn_tile_kernel<LR, NW, NT>, lds); if (e_ != hipSuccess) return e_; \
                               hipLaunchKernelGGL((bt_attn_tile_kernel<LR, NW, NT>), grid, block, lds, st, a, r); } while (0)
  switch (t.lr) {      // the instances launch_attn_tile uses
    case 4: L2_BT(4, 4, 16); break;
    case 8: L2_BT(8, 4, 16); break;
    case 16: L2_BT(16, 4, 16); break;
    case 32: L2_BT(32, 8, 8); break;
    case 64: L2_BT(64, 4, 16); break;
    default: return hipErrorInvalidValue;
  }
#undef L2_BT
  return hipGetLastError();
}

// Attention in the decode form, one workgroup per (head, row), over n rows of the row tables `r` at layer l (its slab loff floats into a
// sequence's cache): A.q -> A.xb, each row over its own sequence's cache (llama2.ts:244-267).
static int bt_attn_rows(const l2_ctx* c, int l, const PfActs& A, const AttnRows& r, size_t loff, int n, hipStream_t st) {
  AttnArgs aa;
  fill_attn_args(c, l, aa);      // (its split count is the single-sequence step's: the kernel runs one workgroup per (head, row), one split)
  aa.q = A.q; aa.xb = A.xb; aa.att = nullptr; aa.tokpos = nullptr; aa.part = nullptr; aa.counter = nullptr;
  const AttnRows ar = {r.seq, r.pos, r.kc, r.vc, loff};
  LCHK(launch_bt_attn(c, aa, ar, n, st));
  return L2_OK;
}

// Final rmsnorm + classifier (llama2.ts:299-302): the residual rows `x` normed into `xn` (norm_rows of them: what the caller's launch
// sequence holds, padding included), then the logits of the first n into out [n][V], 64 rows (pf_gemm_kernel<MODE_CLS_ROWS>'s four tiles) a slice.
static int bt_classify(const l2_ctx* c, const float* x, float* xn, float* out, int norm_rows, int n, hipStream_t st) {
  hipLaunchKernelGGL(pf_norm_kernel, dim3(norm_rows), dim3(256), 0, st, xn, x, c->w[L2_T_RMS_FINAL], c->d);
  for (int s0 = 0; s0 < n; s0 += PF_T) {
    const int ms = std::min(n - s0, (int)PF_T);
    PfArgs a;
    memset(&a, 0, sizeof(a));
    bt_cls_weights(c, a);
    a.xin = xn + (size_t)s0 * c->d; a.out = out + (size_t)s0 * c->V; a.n = c->d; a.rows = c->V; a.dim = c->d; a.nvalid = ms;
    LCHK(launch_gemm<MODE_CLS_ROWS>(a, plan_gemm(plan_shape(c), plan_opts(c), PF_GEMM_BATCH, MODE_CLS_ROWS, a.rows, pf_tiles(ms)), st));
  }
  LCHK(hipGetLastError());
  return L2_OK;
}

// The forward part of one batch step of n rows (tables already on the device): embed, the layers, final norm, classifier -> b->logits.
static int bt_forward(l2_ctx* c, int n, hipStream_t st) {
  BatchState* b = c->bt;
  const AttnRows rows = {b->seq_of(), b->pos_of(), b->d_kc, b->d_vc, 0};
  const auto attn = [&](int l, size_t loff) { return bt_attn_rows(c, l, b->act, rows, loff, n, st); };
  const int rc = pf_layers<PF_GEMM_BATCH>(c, b->act, b->tok_of(), n, rows, attn, st);
  if (rc) return rc;
  return bt_classify(c, b->act.x, b->act.xn, b->logits, pf_tiles(n).nt, n, st);
}

// Every row's pick from b->logits into the token table (fed next) and b->out: its argmax (llama2.ts:364-366), or -- `sampled` -- the row
// sampler (every phase once for all n rows), then every row's pick applied.  `sampler_in`: the rows the sampler reads when they are
// not b->logits (the truncated copy of l2_step_batch_sampling, in which a greedy row is a plain copy).
static int bt_enqueue_pick(l2_ctx* c, int n, bool sampled, hipStream_t st, const float* sampler_in = nullptr) {
  BatchState* b = c->bt;
  if (sampled) {
    LCHK(l2s::enqueue_rows(*b->smp, sampler_in ? sampler_in : b->logits, n, l2s::PICK_BOTH, l2s::Pick{b->smp->pick, nullptr, nullptr}, st));
    hipLaunchKernelGGL(bt_pick_kernel, dim3(n), dim3(1024), 0, st, (const float*)b->logits, c->V, (const double*)b->smp->params, b->smp->pick,
                       b->tok_of(), b->pos_of(), (const int*)b->start_of(), b->out, c->S);
  } else {
    hipLaunchKernelGGL(bt_argmax_kernel, dim3(n), dim3(1024), 0, st, (const float*)b->logits, c->V, b->tok_of(), b->pos_of(), (const int*)b->start_of(),
                       b->out, c->S);
  }
  LCHK(hipGetLastError());
  return L2_OK;
}

// One batch step, greedy or sampled: the forward part, then every row's pick.
static int bt_enqueue(l2_ctx* c, int n, bool sampled, hipStream_t st) {
  const int rc = bt_forward(c, n, st);
  return rc ? rc : bt_enqueue_pick(c, n, sampled, st);
}

// What a recorded step baked in: every weight address it may read and the options that shape it.  A change drops the recordings.
static std::vector<uintptr_t> bt_signature(const l2_ctx* c) {
  std::vector<uintptr_t> s;
  for (int k = 0; k < L2_T_COUNT; ++k) { s.push_back((uintptr_t)c->w[k]); s.push_back(c->released[k]); }
  for (const auto& p : c->packed) { s.push_back((uintptr_t)p.buf); s.push_back((uintptr_t)p.grid); s.push_back((uintptr_t)p.nwaves); }
  s.push_back((uintptr_t)c->opt_exact);
  return s;
}

// The per-row sampling arguments of a call, in call order.
struct BtSampling { const double *temperature, *topp; uint64_t* rng_state; };

// Stage the settings and rng states of n rows (row j: the call's row ord[j]; null: j) in the row sampler's pinned tables -- the stream has
// been synchronised since the previous call's copies -- and upload them.
static int bt_sampler_upload(const l2s::RowSampler& sm, int n, const BtSampling& s, const int* ord, hipStream_t st) {
  for (int j = 0; j < n; ++j) {
    const int i = ord ? ord[j] : j;
    sm.h_params[2 * j] = s.temperature[i]; sm.h_params[2 * j + 1] = s.topp[i]; sm.h_rng[j] = s.rng_state[i];
  }
  HIPCHK(l2s::reset_rows(sm, n, st));      // "zero between tokens" holds whatever an earlier (aborted) call left
  HIPCHK(hipMemcpyAsync(sm.params, sm.h_params, 2 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(sm.rng, sm.h_rng, (size_t)n * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
  return L2_OK;
}

// The way back: enqueue the copies of the rows' rng states and counters into the pinned tables ...
static int bt_sampler_fetch(const l2s::RowSampler& sm, int n, hipStream_t st) {
  HIPCHK(hipMemcpyAsync(sm.h_rng, sm.rng, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(sm.h_stats, sm.stats, 2 * (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  return L2_OK;
}

// ... and, once the stream has been synchronised, hand the states to the caller and add the counters to smp_stats (saturating).
static void bt_sampler_finish(BatchState* b, int n, uint64_t* rng_state, const int* ord) {
  for (int j = 0; j < n; ++j) {
    rng_state[ord ? ord[j] : j] = b->smp->h_rng[j];
    for (int k = 0; k < 2; ++k) { const unsigned long long v = b->smp_stats[k] + b->smp->h_stats[2 * j + k]; b->smp_stats[k] = v < b->smp_stats[k] ? ~0ull : v; }
  }
}

// Upload the tables of n rows and run `steps` batch steps (recorded once per row count, replayed; eager with L2_OPT_USE_GRAPH = 0).
// `smp`: the sampled step with these per-row settings (the caller has made b->smp); their rng states come back advanced.
static int bt_run(l2_ctx* c, int n, const int32_t* seqs, const int32_t* tokens, const int32_t* pos, int steps, const BtSampling* smp = nullptr) {
  BatchState* b = c->bt;
  const bool sampled = smp != nullptr;
  int rc = ensure_ready(c);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  const std::vector<uintptr_t> sig = bt_signature(c);
  if (sig != b->sig) { bt_drop_graphs(b); b->sig = sig; }
  HIPCHK(hipStreamSynchronize(c->stream));      // (h_tab: the previous call's copy has completed)
  for (int i = 0; i < BT_MAX; ++i) {
    const bool live = i < n;
    b->h_tab[i] = live ? seqs[i] : 0;
    b->h_tab[BT_MAX + i] = live ? tokens[i] : 0;
    b->h_tab[2 * BT_MAX + i] = live ? pos[i] : 0;
    b->h_tab[3 * BT_MAX + i] = live ? pos[i] : 0;
  }
  HIPCHK(hipMemcpyAsync(b->tab, b->h_tab, 4 * BT_MAX * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (sampled) { rc = bt_sampler_upload(*b->smp, n, *smp, nullptr, c->stream); if (rc) return rc; }
  hipGraphExec_t* rec = sampled ? b->gs : b->g;
  if (c->opt_graph && !rec[n]) {
    hipGraph_t graph = nullptr;
    LCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    rc = bt_enqueue(c, n, sampled, c->stream);
    const hipError_t e = hipStreamEndCapture(c->stream, &graph);
    if (rc) { if (graph) hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fail(L2_E_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    const hipError_t e2 = hipGraphInstantiate(&rec[n], graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e2 != hipSuccess) { rec[n] = nullptr; return fail(L2_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e2)); }
  }
  for (int s = 0; s < steps; ++s) {
    if (c->opt_graph) HIPCHK(hipGraphLaunch(rec[n], c->stream));
    else { rc = bt_enqueue(c, n, sampled, c->stream); if (rc) return rc; }
  }
  if (sampled) { rc = bt_sampler_fetch(*b->smp, n, c->stream); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (sampled) bt_sampler_finish(b, n, smp->rng_state, nullptr);
  for (int i = 0; i < n; ++i) bt_set_next(c, seqs[i], pos[i] + steps);
  return L2_OK;
}

extern "C" int l2_forward_batch(l2_ctx* c, int n, const int32_t* seqs, const int32_t* tokens, const int32_t* pos, float* logits_out) {
  int rc = bt_check(c, n, seqs, tokens, pos, 1);
  if (rc) return rc;
  rc = bt_run(c, n, seqs, tokens, pos, 1);
  if (rc) return rc;
  if (logits_out) HIPCHK(hipMemcpy(logits_out, c->bt->logits, (size_t)n * c->V * sizeof(float), hipMemcpyDeviceToHost));
  return L2_OK;
}

// Every row's picks of `steps` steps (b->out [row][S]) into tokens_out [n][steps].
static int bt_copy_tokens(const l2_ctx* c, int32_t* tokens_out, int steps, int n) {
  HIPCHK(hipMemcpy2D(tokens_out, (size_t)steps * sizeof(int32_t), c->bt->out, (size_t)c->S * sizeof(int), (size_t)steps * sizeof(int32_t), n, hipMemcpyDeviceToHost));
  return L2_OK;
}

extern "C" int l2_decode_greedy_batch(l2_ctx* c, int n, const int32_t* seqs, const int32_t* first_tokens, const int32_t* pos0, int steps,
                                      int32_t* tokens_out) {
  int rc = bt_check(c, n, seqs, first_tokens, pos0, steps);
  if (rc) return rc;
  if (!tokens_out && steps > 0) return fail(L2_E_ARG, "null tokens_out");
  if (steps == 0) return L2_OK;
  rc = bt_run(c, n, seqs, first_tokens, pos0, steps);
  if (rc) return rc;
  return bt_copy_tokens(c, tokens_out, steps, n);
}

// The row sampler's buffers (one row per reserved sequence), allocated at the first call that samples.
static int bt_ensure_sampler(l2_ctx* c, const char* who) {
  BatchState* b = c->bt;
  if (b->smp) return L2_OK;
  l2s::RowSampler* sm = new l2s::RowSampler();
  const hipError_t e = l2s::create_rows(sm, c->V, b->n_seqs);
  if (e != hipSuccess) { delete sm; (void)hipGetLastError(); return fail(L2_E_HIP, "%s: device memory for the row sampler: %s", who, hipGetErrorString(e)); }
  b->smp = sm;
  return L2_OK;
}

extern "C" int l2_decode_sample_batch(l2_ctx* c, int n, const int32_t* seqs, const int32_t* first_tokens, const int32_t* pos0, int steps,
                                      const double* temperature, const double* topp, uint64_t* rng_state, int32_t* tokens_out) {
  int rc = bt_check(c, n, seqs, first_tokens, pos0, steps);
  if (rc) return rc;
  if (!temperature || !topp || !rng_state) return fail(L2_E_ARG, "null temperature / topp / rng_state");
  if (!tokens_out && steps > 0) return fail(L2_E_ARG, "null tokens_out");
  bool any = false;
  rc = bt_check_sampling(c, n, temperature, topp, &any);
  if (rc) return rc;
  if (steps == 0) return L2_OK;
  const BtSampling smp = {temperature, topp, rng_state};
  const bool sampler = c->V <= l2s::MAX_VOCAB;      // else every row greedy (no draw, rng states untouched) on a vocabulary the row sampler cannot hold
  if (sampler) {
    HIPCHK(hipSetDevice(c->device));
    rc = bt_ensure_sampler(c, "l2_decode_sample_batch");
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));      // (the pinned tables: the previous call's copies have completed)
  }
  rc = bt_run(c, n, seqs, first_tokens, pos0, steps, sampler ? &smp : nullptr);
  if (rc) return rc;
  return bt_copy_tokens(c, tokens_out, steps, n);
}

extern "C" int l2_seq_prefill(l2_ctx* c, int seq, const int32_t* tokens, int n_tokens, int pos0, float* logits_out) {
  if (!c || !tokens) return fail(L2_E_ARG, "null argument");
  if (!c->bt) return fail(L2_E_STATE, "no sequences reserved: call l2_seq_reserve first");
  BatchState* b = c->bt;
  if (seq < 0 || seq >= b->n_seqs) return fail(L2_E_ARG, "sequence %d outside [0, n_seqs = %d)", seq, b->n_seqs);
  if (seq == 0) return l2_prefill(c, tokens, n_tokens, pos0, logits_out);
  if (n_tokens <= 0 || pos0 < 0 || pos0 + n_tokens > c->S) return fail(L2_E_ARG, "positions %d..%d outside [0, seq_len=%d)", pos0, pos0 + n_tokens - 1, c->S);
  for (int i = 0; i < n_tokens; ++i) if (tokens[i] < 0 || tokens[i] >= c->V) return fail(L2_E_ARG, "token %d outside [0, vocab_size=%d)", tokens[i], c->V);
  if (int rc = bt_check_pos(c, seq, pos0)) return rc;
  if (n_tokens == 1) {      // one row: the batch step
    const int32_t s1[1] = {seq}, t1[1] = {tokens[0]}, p1[1] = {pos0};
    return l2_forward_batch(c, 1, s1, t1, p1, logits_out);
  }
  int rc = ensure_ready(c);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  const int step = plan_step(plan_shape(c), plan_opts(c));
  int done = 0;
  while (done < n_tokens) {
    const int n = (n_tokens - done < step) ? n_tokens - done : step;
    rc = prefill_chunk(c, tokens + done, n, pos0 + done, b->kc[seq], b->vc[seq]);
    if (rc) return rc;
    done += n;
  }
  if (pos0 + n_tokens > b->next_pos[seq] || pos0 == 0) b->next_pos[seq] = pos0 + n_tokens;
  if (logits_out) {      // the last position's logits: final norm of its row and the batch classifier (the context's own buffers stay as they are)
    rc = bt_classify(c, c->pf.x + (size_t)((n_tokens - 1) % step) * c->d, b->act.xn, b->logits, 1, 1, c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(logits_out, b->logits, (size_t)c->V * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return L2_OK;
}

// ---- packed prompts (l2_seq_prefill_batch) and the mixed step (l2_step_batch) -----------------
// The runs of a call are packed back to back, in packing order (row r: its sequence, position, token), and cut into launch sequences of up
// to BP_ROWS rows where the register-blocked GEMMs apply, else PF_T rows (the 16-row-tile kernels): prefill_chunk's launch sequence
// (pf_layers) over them, with the per-row q / k / v epilogue and attention over ragged tiles (batch.hip.h: bp_attn_mfma_kernel).  A run may straddle
// launch sequences: the later one reads the cache rows the earlier one stored.  Before the next launch sequence overwrites the residual
// rows, those of the runs whose LAST row lies in this one are gathered into b->act.x (row i: run i); one final norm and one classifier over
// those n rows give the logits.  Device tables of the call (ints), one upload:
//   [R] sequence, [R] position, [R] token of every row; [4 x tiles] every launch sequence's BpTiles; [n] gather rows (launch-relative)

// Arguments of a packed call, all checked before anything touches the GPU; *R_out: the packed rows.
static int bp_check(l2_ctx* c, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0, size_t* R_out) {
  if (int rc = bt_check_call(c, seqs && n_tokens && tokens && pos0, n)) return rc;
  bool seen[BT_MAX] = {};
  size_t R = 0;
  for (int i = 0; i < n; ++i) {
    if (int rc = bt_check_seq(c->bt, seen, i, seqs[i])) return rc;
    if (n_tokens[i] < 1) return fail(L2_E_ARG, "row %d: n_tokens %d < 1", i, n_tokens[i]);
    if (pos0[i] < 0 || (long long)pos0[i] + n_tokens[i] > c->S)
      return fail(L2_E_ARG, "row %d: positions %d..%lld outside [0, seq_len=%d)", i, pos0[i], (long long)pos0[i] + n_tokens[i] - 1, c->S);
    R += (size_t)n_tokens[i];
  }
  for (size_t r = 0; r < R; ++r) if (tokens[r] < 0 || tokens[r] >= c->V) return fail(L2_E_ARG, "token %d (packed row %zu) outside [0, vocab_size=%d)", tokens[r], r, c->V);
  for (int i = 0; i < n; ++i) if (int rc = bt_check_pos(c, seqs[i], pos0[i])) return rc;
  *R_out = R;
  return L2_OK;
}

// The device side of a call's log-probabilities (lp_bufs): per row its target, lp and argmax; per row and rank its top-k id and lp.
struct LpDev { int* target; double* lp; int* amax; int* top_ids; double* top_lp; };

// lp_rows_kernel over `rows` rows of `logits` (targets `target`), its outputs at row r0 of `o`: the one-key instance when no top-k is
// asked for (round 0 is the argmax), else the LP_TOPK_MAX-key one.
static hipError_t launch_lp_rows(const l2_ctx* c, const float* logits, int rows, const int* target, const LpDev& o, size_t r0, int k, hipStream_t st) {
  const LpRowsArgs a = {logits, target, o.lp + r0, o.amax + r0, o.top_ids + r0 * k, o.top_lp + r0 * k, c->V, k};
  if (k == 0) hipLaunchKernelGGL(lp_rows_kernel<1>, dim3(rows), dim3(1024), 0, st, a);
  else hipLaunchKernelGGL(lp_rows_kernel<LP_TOPK_MAX>, dim3(rows), dim3(1024), 0, st, a);
  return hipGetLastError();
}

// The device buffers of a call over `rows` rows with top-k `k` (grown when too small): [rows] lp, [rows][k] top lps (doubles first),
// then [rows] targets, [rows] argmax, [rows][k] top ids.
static int lp_bufs(l2_ctx* c, size_t rows, int k, LpDev& o) {
  BatchState* b = c->bt;
  const size_t need = rows * (sizeof(double) * (1 + k) + sizeof(int) * (2 + k));
  if (need > b->lpbuf_cap) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (b->lpbuf) { HIPCHK(hipFree(b->lpbuf)); b->lpbuf = nullptr; b->lpbuf_cap = 0; }
    HIPCHK(hipMalloc(&b->lpbuf, need));
    b->lpbuf_cap = need;
  }
  o.lp = reinterpret_cast<double*>(b->lpbuf);
  o.top_lp = o.lp + rows;
  o.target = reinterpret_cast<int*>(o.top_lp + rows * k);
  o.amax = o.target + rows;
  o.top_ids = o.amax + rows;
  return L2_OK;
}

// Bytes from the start of b->lpbuf to p (a column of an LpDev that lp_bufs carved out of it).
static size_t lp_span(const BatchState* b, const void* p) { return (size_t)((const char*)p - b->lpbuf); }

// Arguments of the log-probability calls that need no context: top_k in [0, LP_TOPK_MAX], its arrays given when top_k > 0.
static int lp_check_k(int top_k, const void* top_ids_out, const void* top_lp_out) {
  if (top_k < 0 || top_k > LP_TOPK_MAX) return fail(L2_E_ARG, "top_k %d outside [0, %d]", top_k, (int)LP_TOPK_MAX);
  if (top_k > 0 && (!top_ids_out || !top_lp_out)) return fail(L2_E_ARG, "top_k %d with a null top_ids_out / top_lp_out", top_k);
  return L2_OK;
}

// The plan of a packed call: host arithmetic on its arguments alone.
struct BpPlan {
  int step = 0, nl = 0;                        // rows of a launch sequence, launch sequences
  size_t n_tiles = 0;                          // attention tiles of the call
  std::vector<int> tile0, maxp, seq_a, seq_b;  // per launch sequence: its first tile ([nl + 1]), its tiles' highest pos0, the runs ending in it (seq_a .. seq_b - 1)
  std::vector<int> htab;                       // the call's device tables (layout above) as uploaded: kept until the stream has been synchronised
};

// Plan n checked runs given in packing order (R rows in all, launch sequences of `step`), the first nd of them decode rows: cut into no tile.
static void bp_plan(BpPlan& p, int step, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0, size_t R, int nd) {
  const int nl = (int)((R + step - 1) / step);
  p.step = step; p.nl = nl;
  std::vector<size_t> first(n + 1, 0);                       // first packed row of run i
  for (int i = 0; i < n; ++i) first[i + 1] = first[i] + (size_t)n_tokens[i];
  std::vector<BpTile> tiles;
  std::vector<int> gsrc(n, 0);
  p.tile0.assign(nl + 1, 0); p.maxp.assign(nl, 0); p.seq_a.assign(nl, 0); p.seq_b.assign(nl, 0);
  for (int k = 0, i0 = 0; k < nl; ++k) {
    const size_t r0 = (size_t)k * step, r1 = std::min(r0 + step, R);
    p.tile0[k] = (int)tiles.size();
    p.seq_a[k] = i0;
    for (int i = i0; i < n && first[i] < r1; ++i) {
      const size_t lo = std::max(first[i], r0), hi = std::min(first[i + 1], r1);
      for (size_t t = lo; t < hi && i >= nd; t += 16) {      // tiles start at the run's first row in this launch sequence
        const BpTile tl = {seqs[i], (int)(t - r0), pos0[i] + (int)(t - first[i]), (int)std::min<size_t>(16, hi - t)};
        tiles.push_back(tl);
        p.maxp[k] = std::max(p.maxp[k], tl.pos0);
      }
      if (first[i + 1] <= r1) { gsrc[i] = (int)(first[i + 1] - 1 - r0); i0 = i + 1; }      // its last row lies here
    }
    p.seq_b[k] = i0;
    std::sort(tiles.begin() + p.tile0[k], tiles.end(), [](const BpTile& x, const BpTile& y) { return x.pos0 > y.pos0; });   // longest first
  }
  p.tile0[nl] = (int)tiles.size();
  p.n_tiles = tiles.size();
  p.htab.assign(3 * R + 4 * tiles.size() + (size_t)n, 0);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < n_tokens[i]; ++k) { const size_t r = first[i] + k; p.htab[r] = seqs[i]; p.htab[R + r] = pos0[i] + k; p.htab[2 * R + r] = tokens[r]; }
  if (!tiles.empty()) memcpy(p.htab.data() + 3 * R, tiles.data(), tiles.size() * sizeof(BpTile));
  memcpy(p.htab.data() + 3 * R + 4 * tiles.size(), gsrc.data(), (size_t)n * sizeof(int));
}

// The plan's tables onto the device (b->ptab, grown when too small).
static int bp_upload(l2_ctx* c, const BpPlan& p) {
  BatchState* b = c->bt;
  const size_t need = p.htab.size();
  if (need > b->ptab_cap) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (b->ptab) { HIPCHK(hipFree(b->ptab)); b->ptab = nullptr; b->ptab_cap = 0; }
    HIPCHK(hipMalloc(&b->ptab, need * sizeof(int)));
    b->ptab_cap = need;
  }
  HIPCHK(hipMemcpyAsync(b->ptab, p.htab.data(), need * sizeof(int), hipMemcpyHostToDevice, c->stream));      // (htab lives past the caller's synchronise)
  return L2_OK;
}

// Enqueue the launch sequences of n checked runs given in packing order (R rows in all).  The first nd runs are decode rows (one row
// each, l2_step_batch; 0 for l2_seq_prefill_batch): they lie in the first launch sequence, are cut into no tile, and take the decode
// attention form per (head, row) -- bt_attn_tile_kernel, at any head size and position -- while the tiles of the longer runs take
// bp_attn_mfma_kernel with its LDS sized by the longest of them.  `logits`: gather every run's last row, final norm and classifier ->
// b->logits rows 0 .. n-1.  `p` receives the plan, whose htab holds the uploaded tables: the caller keeps it until the stream has been
// synchronised.  `score` (l2_seq_score_batch): after each launch sequence's layers, the final norm and the classifier of EVERY row of it
// (bt_classify: the last-row classifier's arithmetic) into b->slogits, then lp_rows_kernel over them with the targets and outputs of
// `score` at the launch sequence's first row -- all before the next launch sequence overwrites the rows.
static int bp_enqueue(l2_ctx* c, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0, size_t R, int nd,
                      bool logits, BpPlan& p, const LpDev* score = nullptr, int top_k = 0) {
  BatchState* b = c->bt;
  hipStream_t st = c->stream;
  const PfActs& P = b->pact;
  int rc = pf_acts_ensure(c, b->pact);
  if (rc) return rc;
  bp_plan(p, plan_step(plan_shape(c), plan_opts(c)), n, seqs, n_tokens, tokens, pos0, R, nd);
  rc = bp_upload(c, p);
  if (rc) return rc;
  const int* dseq = b->ptab;
  const int* dpos = b->ptab + R;
  const int* dtok = b->ptab + 2 * R;
  const BpTile* dtiles = reinterpret_cast<const BpTile*>(b->ptab + 3 * R);
  const int* dgsrc = b->ptab + 3 * R + 4 * p.n_tiles;
  for (int k = 0; k < p.nl; ++k) {
    const int r0 = k * p.step, m = (int)std::min<size_t>(p.step, R - r0), nti = p.tile0[k + 1] - p.tile0[k];
    const int ndk = k == 0 ? nd : 0;                           // decode rows of this launch sequence (its rows 0 .. ndk-1)
    AttnPick ap[2];      // the longest tile's keys size the MFMA form's LDS
    const int nap = plan_attention(plan_shape(c), plan_opts(c), CALL_PACKED, m, ndk, p.maxp[k] + 15, ap);
    const AttnRows rows = {dseq + r0, dpos + r0, b->d_kc, b->d_vc, 0};
    // attention: 16-query tiles on the fp64 MFMA (decode rows: per (head, row)), or the decode form per (head, row) for every row where
    // prefill_chunk takes it
    const auto attn = [&](int l, size_t loff) -> int {
      for (int i = 0; i < nap; ++i) {
        if (ap[i].family == AT_BT_TILE) { const int e = bt_attn_rows(c, l, P, rows, loff, ap[i].rows, st); if (e) return e; continue; }
        if (nti == 0) return fail(L2_E_HIP, "packed attention: %d tile rows planned, no tile cut", ap[i].rows);
        BpAttnArgs pa;
        pa.q = P.q; pa.xb = P.xb; pa.seq_kc = b->d_kc; pa.seq_vc = b->d_vc; pa.seq_loff = loff; pa.tiles = dtiles + p.tile0[k];
        pa.dim = c->d; pa.seq_len = c->S; pa.inv_sqrt_hs = 1.0 / sqrt((double)c->hs);
        const int e = launch_attn_mfma(ap[i], bp_attn_mfma_kernel<64>, bp_attn_mfma_kernel<128>, dim3(c->H, nti), pa, st);
        if (e) return e;
      }
      return L2_OK;
    };
    rc = pf_layers<PF_GEMM_PROMPT>(c, P, dtok + r0, m, rows, attn, st);
    if (rc) return rc;
    if (score) {      // every row of this launch sequence: final rmsnorm, classifier, log-probabilities
      rc = bt_classify(c, P.x, P.xn, b->slogits, pf_tiles(m).nt, m, st);
      if (rc) return rc;
      LCHK(launch_lp_rows(c, b->slogits, m, score->target + r0, *score, (size_t)r0, top_k, st));
    }
    // the residual rows of the runs that end here, into b->act.x rows seq_a .. seq_b - 1 (pf_embed_kernel as a row gather)
    if (logits && p.seq_b[k] > p.seq_a[k]) {
      hipLaunchKernelGGL(pf_embed_kernel, dim3(p.seq_b[k] - p.seq_a[k]), dim3(256), 0, st, b->act.x + (size_t)p.seq_a[k] * c->d, (const float*)P.x, dgsrc + p.seq_a[k],
                         c->d, p.seq_b[k] - p.seq_a[k]);
      LCHK(hipGetLastError());
    }
  }
  // final rmsnorm + classifier of every run's last row
  return logits ? bt_classify(c, b->act.x, b->act.xn, b->logits, n, n, st) : L2_OK;
}

// Each named sequence's next position as l2_seq_prefill leaves it (after the stream has been synchronised).
static void bp_set_next(l2_ctx* c, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* pos0) {
  for (int i = 0; i < n; ++i) {
    const int s = seqs[i], end = pos0[i] + n_tokens[i];
    if (end > bt_next(c, s) || pos0[i] == 0) bt_set_next(c, s, end);
  }
}

extern "C" int l2_seq_prefill_batch(l2_ctx* c, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                                    float* logits_out) {
  size_t R = 0;
  int rc = bp_check(c, n, seqs, n_tokens, tokens, pos0, &R);
  if (rc) return rc;
  rc = ensure_ready(c);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  BpPlan plan;
  rc = bp_enqueue(c, n, seqs, n_tokens, tokens, pos0, R, 0, logits_out != nullptr, plan);
  if (rc) return rc;
  if (logits_out) HIPCHK(hipMemcpyAsync(logits_out, c->bt->logits, (size_t)n * c->V * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  bp_set_next(c, n, seqs, n_tokens, pos0);
  return L2_OK;
}

// ---- teacher-forced scoring (l2_seq_score_batch) --------------------------------------------------
// l2_seq_prefill_batch's launch sequences (same packing, no last-row gather), with every row's logits and log-probabilities made inside
// them (bp_enqueue's `score`); only the per-row results come back.
extern "C" int l2_seq_score_batch(l2_ctx* c, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                                  const int32_t* targets, int top_k, double* lp_out, int32_t* argmax_out, int32_t* top_ids_out, double* top_lp_out) {
  if (!targets || !lp_out) return fail(L2_E_ARG, "null targets / lp_out");
  int rc = lp_check_k(top_k, top_ids_out, top_lp_out);
  if (rc) return rc;
  size_t R = 0;
  rc = bp_check(c, n, seqs, n_tokens, tokens, pos0, &R);
  if (rc) return rc;
  for (size_t r = 0; r < R; ++r)
    if (targets[r] < -1 || targets[r] >= c->V) return fail(L2_E_ARG, "target %d (packed row %zu) outside [-1, vocab_size=%d)", targets[r], r, c->V);
  if (top_k > c->V) return fail(L2_E_ARG, "top_k %d > vocab_size %d", top_k, c->V);
  rc = ensure_ready(c);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  BatchState* b = c->bt;
  hipStream_t st = c->stream;
  if (!b->slogits) HIPCHK(hipMalloc(&b->slogits, (size_t)BP_ROWS * c->V * sizeof(float)));
  LpDev o;
  rc = lp_bufs(c, R, top_k, o);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(o.target, targets, R * sizeof(int32_t), hipMemcpyHostToDevice, st));
  BpPlan plan;
  rc = bp_enqueue(c, n, seqs, n_tokens, tokens, pos0, R, 0, false, plan, &o, top_k);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(lp_out, o.lp, R * sizeof(double), hipMemcpyDeviceToHost, st));
  if (argmax_out) HIPCHK(hipMemcpyAsync(argmax_out, o.amax, R * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (top_k > 0) {
    HIPCHK(hipMemcpyAsync(top_ids_out, o.top_ids, R * top_k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(top_lp_out, o.top_lp, R * top_k * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  bp_set_next(c, n, seqs, n_tokens, pos0);
  return L2_OK;
}

// ---- constraints of the mixed step (l2_step_batch_constrained; kernels: constrain.hip.h) -----------
// The constraint arguments of a call, in call order (l2_step_batch_constrained; its context-free checks are cs_check_free).
struct BtConstraint {
  const int32_t* mask_of_row; int n_masks; const uint32_t* masks;
  const int32_t* bias_count; const int32_t* bias_ids; const float* bias_vals;
};

// What needs no context: n (so that the arrays can be walked), the null combinations, n_masks, every row's mask index and bias count,
// the bias values.
static int cs_check_free(int n, const BtConstraint& k) {
  if (n < 1 || n > BT_MAX) return fail(L2_E_ARG, "n = %d outside [1, %d]", n, (int)BT_MAX);
  if (k.n_masks < 0 || k.n_masks > n) return fail(L2_E_ARG, "n_masks %d outside [0, n = %d]", k.n_masks, n);
  if (!k.mask_of_row && k.n_masks != 0) return fail(L2_E_ARG, "n_masks %d with a null mask_of_row", k.n_masks);
  if ((k.n_masks > 0 || k.mask_of_row) && !k.masks) return fail(L2_E_ARG, "null masks");
  for (int i = 0; k.mask_of_row && i < n; ++i)
    if (k.mask_of_row[i] < -1 || k.mask_of_row[i] >= k.n_masks) return fail(L2_E_ARG, "row %d: mask %d outside [-1, n_masks = %d)", i, k.mask_of_row[i], k.n_masks);
  size_t nb = 0;
  for (int i = 0; k.bias_count && i < n; ++i) {
    if (k.bias_count[i] < 0 || k.bias_count[i] > CS_BIAS_MAX) return fail(L2_E_ARG, "row %d: bias_count %d outside [0, %d]", i, k.bias_count[i], (int)CS_BIAS_MAX);
    nb += (size_t)k.bias_count[i];
  }
  if (nb > 0 && (!k.bias_ids || !k.bias_vals)) return fail(L2_E_ARG, "bias_count names %zu entries, null bias_ids / bias_vals", nb);
  for (size_t j = 0; j < nb; ++j)
    if (!(fabsf(k.bias_vals[j]) < INFINITY)) return fail(L2_E_ARG, "bias value %zu is not finite (a ban is the mask's job)", j);
  return L2_OK;
}

// What needs V: a mask some row names allows a token below V, every bias id lies in [0, V) and appears once in its row, no masked row
// has a negative temperature (-inf / T would become +inf).
static int cs_check_vocab(const l2_ctx* c, int n, const BtConstraint& k, const double* temperature) {
  const int V = c->V, W = (V + 31) / 32;
  for (int i = 0; k.mask_of_row && i < n; ++i) {
    const int m = k.mask_of_row[i];
    if (m < 0) continue;
    const uint32_t* w = k.masks + (size_t)m * W;
    bool some = false;
    for (int q = 0; q < W && !some; ++q) some = (q == W - 1 && (V & 31) ? w[q] & ((1u << (V & 31)) - 1u) : w[q]) != 0;
    if (!some) return fail(L2_E_ARG, "row %d: mask %d allows no token below vocab_size=%d", i, m, V);
    if (temperature && temperature[i] < 0.0) return fail(L2_E_ARG, "row %d: a masked row with temperature %g < 0", i, temperature[i]);
  }
  size_t off = 0;
  for (int i = 0; k.bias_count && i < n; off += (size_t)k.bias_count[i], ++i) {
    const int32_t* ids = k.bias_ids + off;
    for (int j = 0; j < k.bias_count[i]; ++j) {
      if (ids[j] < 0 || ids[j] >= V) return fail(L2_E_ARG, "row %d: bias id %d outside [0, vocab_size=%d)", i, ids[j], V);
      for (int q = 0; q < j; ++q) if (ids[q] == ids[j]) return fail(L2_E_ARG, "row %d: bias id %d appears twice", i, ids[j]);
    }
  }
  return L2_OK;
}

// The call's device tables (constrain.hip.h: their layout) for rows in packing order `ord`, staged in `h`: kept by the caller until
// the stream has been synchronised.  *nb_out: the bias entries of the call.
static void cs_tables(const l2_ctx* c, int n, const BtConstraint& k, const int* ord, std::vector<uint32_t>& h, size_t* nb_out) {
  const size_t W = (size_t)(c->V + 31) / 32, mw = (size_t)k.n_masks * W;
  std::vector<size_t> off(n + 1, 0);      // the rows' lists lie back to back in call order
  for (int i = 0; i < n; ++i) off[i + 1] = off[i] + (size_t)(k.bias_count ? k.bias_count[i] : 0);
  const size_t nb = off[n];
  h.assign(3 * (size_t)n + mw + 2 * nb, 0u);
  size_t at = 0;                          // ... and in packing order on the device
  for (int j = 0; j < n; ++j) {
    const int i = ord[j], cnt = k.bias_count ? k.bias_count[i] : 0;
    h[j] = (uint32_t)(k.mask_of_row ? k.mask_of_row[i] : -1);
    h[n + j] = (uint32_t)at;
    h[2 * n + j] = (uint32_t)cnt;
    if (cnt) {
      memcpy(h.data() + 3 * n + mw + at, k.bias_ids + off[i], (size_t)cnt * 4);
      memcpy(h.data() + 3 * n + mw + nb + at, k.bias_vals + off[i], (size_t)cnt * 4);
    }
    at += (size_t)cnt;
  }
  if (mw) memcpy(h.data() + 3 * n, k.masks, mw * 4);
  *nb_out = nb;
}

// ---- sampling controls of the mixed step (l2_step_batch_sampling; kernels: controls.hip.h) ---------
static bool sc_finite(double v) { return fabs(v) < INFINITY; }      // false for a NaN too
static double sc_at(const double* a, int i, double off) { return a ? a[i] : off; }

// Row i has a history and a penalty that is not neutral: the penalty launch rewrites it.
static bool sc_penalised(const l2_sample_controls& s, int i) {
  return s.hist_count && s.hist_count[i] > 0 &&
         (sc_at(s.repetition, i, 1.0) != 1.0 || sc_at(s.presence, i, 0.0) != 0.0 || sc_at(s.frequency, i, 0.0) != 0.0);
}
// Row i samples with top-k or min-p set.
static bool sc_asks_truncation(const l2_sample_controls& s, const double* temperature, int i) {
  return temperature && temperature[i] != 0.0 && ((s.sample_top_k && s.sample_top_k[i] > 0) || sc_at(s.min_p, i, 0.0) > 0.0);
}

// What needs no context: n (so that the arrays can be walked), every count, penalty, k and min_p, the null history, a truncating
// row's temperature.  hist_max: the bound of a count when the caller knows it without a context (the diagnostic), else -1.
static int sc_check_free(int n, const l2_sample_controls& s, const double* temperature, int hist_max) {
  if (n < 1 || n > BT_MAX) return fail(L2_E_ARG, "n = %d outside [1, %d]", n, (int)BT_MAX);
  size_t nh = 0;
  for (int i = 0; i < n; ++i) {
    if (s.hist_count) {
      if (s.hist_count[i] < 0 || (hist_max >= 0 && s.hist_count[i] > hist_max))
        return fail(L2_E_ARG, "row %d: hist_count %d outside [0, %d]", i, s.hist_count[i], hist_max >= 0 ? hist_max : INT32_MAX);
      nh += (size_t)s.hist_count[i];
    }
    const double rep = sc_at(s.repetition, i, 1.0), pres = sc_at(s.presence, i, 0.0), freq = sc_at(s.frequency, i, 0.0), mp = sc_at(s.min_p, i, 0.0);
    if (!(rep > 0.0) || !sc_finite(rep)) return fail(L2_E_ARG, "row %d: repetition %g is not positive and finite", i, rep);
    if (!sc_finite(pres) || !sc_finite(freq)) return fail(L2_E_ARG, "row %d: presence %g / frequency %g is not finite", i, pres, freq);
    if (s.sample_top_k && s.sample_top_k[i] < 0) return fail(L2_E_ARG, "row %d: sample_top_k %d < 0", i, s.sample_top_k[i]);
    if (!(mp >= 0.0 && mp <= 1.0)) return fail(L2_E_ARG, "row %d: min_p %g outside [0, 1]", i, mp);
    if (sc_asks_truncation(s, temperature, i) && temperature[i] < 0.0)
      return fail(L2_E_ARG, "row %d: top-k / min-p with temperature %g < 0 (-inf / T would become +inf)", i, temperature[i]);
  }
  if (nh > 0 && !s.hist_ids) return fail(L2_E_ARG, "hist_count names %zu entries, null hist_ids", nh);
  return L2_OK;
}

// What needs the shape: every count at most hist_max, every history id in [0, V).  This is what keeps the penalty launch in bounds.
static int sc_check_shape(int V, int hist_max, int n, const l2_sample_controls& s) {
  size_t off = 0;
  for (int i = 0; s.hist_count && i < n; off += (size_t)s.hist_count[i], ++i) {
    if (s.hist_count[i] > hist_max) return fail(L2_E_ARG, "row %d: hist_count %d outside [0, %d]", i, s.hist_count[i], hist_max);
    for (int j = 0; j < s.hist_count[i]; ++j)
      if (s.hist_ids[off + j] < 0 || s.hist_ids[off + j] >= V)
        return fail(L2_E_ARG, "row %d: history id %d outside [0, vocab_size=%d)", i, s.hist_ids[off + j], V);
  }
  return L2_OK;
}

// The call's device tables (controls.hip.h: their layout) for rows in packing order `ord` (null: call order), staged in `h`: kept by
// the caller until the stream has been synchronised.  Only the penalised rows' histories travel.
struct ScPlan {
  bool penalise = false, truncate = false;      // some row is penalised; some sampling row truncates
  std::vector<char> h;
  size_t ctl_off = 0, hist_off = 0;             // byte offsets of the int table and of the ids
};
static void sc_tables(int n, int V, const l2_sample_controls& s, const double* temperature, const int* ord, ScPlan& p) {
  std::vector<size_t> off(n + 1, 0);
  size_t nh = 0;
  for (int i = 0; i < n; ++i) {
    off[i + 1] = off[i] + (size_t)(s.hist_count ? s.hist_count[i] : 0);
    if (sc_penalised(s, i)) nh += (size_t)s.hist_count[i];
  }
  p.ctl_off = 4 * (size_t)n * sizeof(double);
  p.hist_off = p.ctl_off + 4 * (size_t)n * sizeof(int);
  p.h.assign(p.hist_off + nh * sizeof(int), 0);
  double* pen = reinterpret_cast<double*>(p.h.data());
  int* ctl = reinterpret_cast<int*>(p.h.data() + p.ctl_off);
  int* ids = reinterpret_cast<int*>(p.h.data() + p.hist_off);
  size_t at = 0;
  for (int j = 0; j < n; ++j) {
    const int i = ord ? ord[j] : j;
    const bool sampling = temperature && temperature[i] != 0.0;
    const int k = sampling && s.sample_top_k && s.sample_top_k[i] < V ? s.sample_top_k[i] : 0;      // k >= V truncates nothing
    const double mp = sampling ? sc_at(s.min_p, i, 0.0) : 0.0;
    const bool tr = k > 0 || mp > 0.0;
    pen[4 * j] = sc_at(s.repetition, i, 1.0); pen[4 * j + 1] = sc_at(s.presence, i, 0.0); pen[4 * j + 2] = sc_at(s.frequency, i, 0.0);
    pen[4 * j + 3] = mp > 0.0 ? log(mp) : -INFINITY;
    ctl[4 * j] = (int)at;
    if (sc_penalised(s, i)) {
      ctl[4 * j + 1] = s.hist_count[i];
      memcpy(ids + at, s.hist_ids + off[i], (size_t)s.hist_count[i] * sizeof(int));
      at += (size_t)s.hist_count[i];
      p.penalise = true;
    }
    ctl[4 * j + 2] = k;
    ctl[4 * j + 3] = tr;                                                            // the survivor rule serves the row
    p.truncate = p.truncate || tr;
  }
}

static ControlArgs sc_args(float* logits, float* trunc, const char* tables, const ScPlan& p, int* count, const double* params, int V) {
  return ControlArgs{logits, trunc, reinterpret_cast<const double*>(tables), reinterpret_cast<const int*>(tables + p.ctl_off),
                     reinterpret_cast<const int*>(tables + p.hist_off), count, params, V};
}
// Stage A over n rows: one launch (a.count is zero and stays so: controls.hip.h).
static int sc_enqueue_penalties(const ControlArgs& a, int n, hipStream_t st) {
  hipLaunchKernelGGL(bt_penalise_rows_kernel<SC_THREADS>, dim3(n), dim3(SC_THREADS), 0, st, a);
  LCHK(hipGetLastError());
  return L2_OK;
}
// Stage B: all n rows of a.trunc, from a.logits and the row sampler's settings a.params.
static int sc_enqueue_truncation(const ControlArgs& a, int n, hipStream_t st) {
  hipLaunchKernelGGL(bt_truncate_rows_kernel<SC_THREADS>, dim3(n), dim3(SC_THREADS), 0, st, a);
  LCHK(hipGetLastError());
  return L2_OK;
}

// ---- the mixed step (l2_step_batch, l2_step_batch_logprobs, l2_step_batch_constrained, l2_step_batch_sampling) ------------
// The runs are reordered so that the one-row runs (decode rows) come first, then packed and run as above; every run's last-position
// logits then get one pick on the device: bt_argmax_kernel when no row samples, else the row sampler's phases and bt_pick_kernel.  The
// picks land in the batch step's token table (its position and start columns zeroed first, so each row's pick is also out[r][0]); only
// they, the rng states and the optional logits come back.  With pick_lp_out (l2_step_batch_logprobs), lp_rows_kernel then reads the
// picks from that table as its targets and the unscaled logits rows; without it the step enqueues nothing more.
// With constraints (l2_step_batch_constrained) two launches join that sequence, and only when a row needs them: bt_constrain_rows_kernel
// rewrites the masked and biased rows of b->logits right after the classifier, so the sampler, the pick, lp_rows_kernel and the logits
// copy all see the constrained rows; bt_allowed_pick_kernel, after the pick, replaces a sampled pick that its row's mask forbids (the
// reference's `return 0`) by the row's first maximum.
// With sampling controls (l2_step_batch_sampling) up to three more, again only when a row needs them: bt_penalise_rows_kernel before
// the constraints' rewrite; bt_truncate_rows_kernel after the sampler's settings are up, writing the copy of the rows that the row
// sampler then reads in place of b->logits; bt_survivor_pick_kernel after the pick for the rows that truncate, in front of
// bt_allowed_pick_kernel, which keeps serving the masked rows.

static int bt_step(l2_ctx* c, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                   const double* temperature, const double* topp, uint64_t* rng_state, int32_t* picks_out, float* logits_out,
                   int top_k, double* pick_lp_out, int32_t* top_ids_out, double* top_lp_out, const BtConstraint* cs = nullptr,
                   const l2_sample_controls* sc = nullptr) {
  size_t R = 0;
  int rc = bp_check(c, n, seqs, n_tokens, tokens, pos0, &R);
  if (rc) return rc;
  if (!picks_out) return fail(L2_E_ARG, "null picks_out");
  const int given = (temperature != nullptr) + (topp != nullptr) + (rng_state != nullptr);
  if (given != 0 && given != 3) return fail(L2_E_ARG, "temperature / topp / rng_state: give all three, or none for every row greedy");
  bool any = false;
  rc = bt_check_sampling(c, n, temperature, topp, &any);
  if (rc) return rc;
  if (top_k > c->V) return fail(L2_E_ARG, "top_k %d > vocab_size %d", top_k, c->V);
  bool constrain = false, redo = false;      // some row has a mask or a bias list; some row samples under a mask
  if (cs) {
    rc = cs_check_vocab(c, n, *cs, temperature);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
      const bool masked = cs->mask_of_row && cs->mask_of_row[i] >= 0;
      constrain = constrain || masked || (cs->bias_count && cs->bias_count[i] > 0);
      redo = redo || (masked && temperature && temperature[i] != 0.0);
    }
  }
  if (sc) {
    rc = sc_check_shape(c->V, c->S, n, *sc);
    if (rc) return rc;
  }

  // packing order: decode rows (runs of one row) first, then the longer runs, each group in call order
  std::vector<int> ord;
  ord.reserve(n);
  for (int i = 0; i < n; ++i) if (n_tokens[i] == 1) ord.push_back(i);
  const int nd = (int)ord.size();
  for (int i = 0; i < n; ++i) if (n_tokens[i] > 1) ord.push_back(i);
  std::vector<size_t> first(n + 1, 0);
  for (int i = 0; i < n; ++i) first[i + 1] = first[i] + (size_t)n_tokens[i];
  std::vector<int32_t> ps(n), pn(n), pp(n), ptok;
  ptok.reserve(R);
  bool identity = true;
  for (int j = 0; j < n; ++j) {
    const int i = ord[j];
    identity = identity && i == j;
    ps[j] = seqs[i]; pn[j] = n_tokens[i]; pp[j] = pos0[i];
    ptok.insert(ptok.end(), tokens + first[i], tokens + first[i + 1]);
  }

  rc = ensure_ready(c);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  BatchState* b = c->bt;
  hipStream_t st = c->stream;
  if (any) {
    rc = bt_ensure_sampler(c, "l2_step_batch");
    if (rc) return rc;
  }
  LpDev o = {};
  if (pick_lp_out) {
    rc = lp_bufs(c, (size_t)n, top_k, o);
    if (rc) return rc;
  }
  std::vector<uint32_t> cstab;      // the constraint tables as uploaded: kept until the stream has been synchronised
  size_t cs_nb = 0;
  if (constrain) {
    cs_tables(c, n, *cs, ord.data(), cstab, &cs_nb);
    if (cstab.size() > b->csbuf_cap) {
      HIPCHK(hipStreamSynchronize(st));
      if (b->csbuf) { HIPCHK(hipFree(b->csbuf)); b->csbuf = nullptr; b->csbuf_cap = 0; }
      HIPCHK(hipMalloc(&b->csbuf, cstab.size() * sizeof(uint32_t)));
      b->csbuf_cap = cstab.size();
    }
  }
  ScPlan sp;                        // the control tables as uploaded: kept until the stream has been synchronised
  if (sc) sc_tables(n, c->V, *sc, temperature, ord.data(), sp);
  if (sp.penalise || sp.truncate) {
    const size_t rowset = (size_t)BT_MAX * c->V;
    if (sp.h.size() > b->scbuf_cap) {
      HIPCHK(hipStreamSynchronize(st));
      if (b->scbuf) { HIPCHK(hipFree(b->scbuf)); b->scbuf = nullptr; b->scbuf_cap = 0; }
      HIPCHK(hipMalloc(&b->scbuf, sp.h.size()));
      b->scbuf_cap = sp.h.size();
    }
    if (sp.penalise && !b->sccount) {
      HIPCHK(hipMalloc(&b->sccount, rowset * sizeof(int)));
      HIPCHK(hipMemset(b->sccount, 0, rowset * sizeof(int)));
    }
    if (sp.truncate && !b->tlogits) HIPCHK(hipMalloc(&b->tlogits, rowset * sizeof(float)));
  }
  HIPCHK(hipStreamSynchronize(st));      // (the pinned tables: the previous call's copies have completed)
  BpPlan plan;
  rc = bp_enqueue(c, n, ps.data(), pn.data(), ptok.data(), pp.data(), R, nd, true, plan);
  if (rc) return rc;
  ControlArgs xa = {};
  if (sp.penalise || sp.truncate) {      // penalise, then add bias, then mask
    HIPCHK(hipMemcpyAsync(b->scbuf, sp.h.data(), sp.h.size(), hipMemcpyHostToDevice, st));
    xa = sc_args(b->logits, b->tlogits, b->scbuf, sp, b->sccount, any ? b->smp->params : nullptr, c->V);
    if (sp.penalise) { rc = sc_enqueue_penalties(xa, n, st); if (rc) return rc; }
  }
  const int csW = (c->V + 31) / 32;
  const int* cs_mask_of = nullptr;
  const unsigned* cs_masks = nullptr;
  if (constrain) {      // the masked and biased rows of b->logits, rewritten before anything reads them
    cs_mask_of = reinterpret_cast<const int*>(b->csbuf);
    cs_masks = b->csbuf + 3 * (size_t)n;
    HIPCHK(hipMemcpyAsync(b->csbuf, cstab.data(), cstab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    const unsigned* bias = cs_masks + (size_t)cs->n_masks * csW;
    const ConstrainArgs ca = {b->logits, cs_mask_of, cs_mask_of + n, cs_mask_of + 2 * n, cs_masks, reinterpret_cast<const int*>(bias),
                              reinterpret_cast<const float*>(bias + cs_nb), c->V, csW};
    hipLaunchKernelGGL(bt_constrain_rows_kernel, dim3((c->V + CS_COLS - 1) / CS_COLS, n), dim3(CS_THREADS), 0, st, ca);
    LCHK(hipGetLastError());
  }
  HIPCHK(hipMemsetAsync(b->tab, 0, 4 * BT_MAX * sizeof(int), st));
  if (any) { rc = bt_sampler_upload(*b->smp, n, {temperature, topp, rng_state}, ord.data(), st); if (rc) return rc; }
  if (sp.truncate) { rc = sc_enqueue_truncation(xa, n, st); if (rc) return rc; }      // the rows as the sampler reads them
  rc = bt_enqueue_pick(c, n, any, st, sp.truncate ? b->tlogits : nullptr);
  if (rc) return rc;
  if (sp.truncate) {      // a truncating row's sampled pick that did not survive becomes the first maximum of its truncated row
    const SurvivorPickArgs pa = {b->tlogits, xa.ctl, b->tok_of(), b->out, c->V, c->S};
    hipLaunchKernelGGL(bt_survivor_pick_kernel<SC_THREADS>, dim3(n), dim3(SC_THREADS), 0, st, pa);
    LCHK(hipGetLastError());
  }
  if (redo) {      // a sampled pick its row's mask forbids becomes the row's first maximum
    const AllowedPickArgs pa = {b->logits, b->smp->params, cs_mask_of, cs_masks, b->tok_of(), b->out, c->V, csW, c->S};
    hipLaunchKernelGGL(bt_allowed_pick_kernel, dim3(n), dim3(1024), 0, st, pa);
    LCHK(hipGetLastError());
  }
  std::vector<char> lpbytes;
  if (pick_lp_out) {      // after the pick: its log-probability under the unscaled logits, and the top-k
    LCHK(launch_lp_rows(c, b->logits, n, b->tok_of(), o, 0, top_k, st));
    lpbytes.resize(lp_span(b, o.top_ids + (size_t)n * top_k));      // one copy of lp_bufs' layout, up to its last column
    HIPCHK(hipMemcpyAsync(lpbytes.data(), b->lpbuf, lpbytes.size(), hipMemcpyDeviceToHost, st));
  }
  std::vector<int32_t> picks(n);
  HIPCHK(hipMemcpyAsync(picks.data(), b->tok_of(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  std::vector<float> lg;
  if (logits_out) {
    float* dst = logits_out;
    if (!identity) { lg.resize((size_t)n * c->V); dst = lg.data(); }
    HIPCHK(hipMemcpyAsync(dst, b->logits, (size_t)n * c->V * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  if (any) { rc = bt_sampler_fetch(*b->smp, n, st); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(st));
  for (int j = 0; j < n; ++j) {
    const int i = ord[j];
    picks_out[i] = picks[j];
    if (!lg.empty()) memcpy(logits_out + (size_t)i * c->V, lg.data() + (size_t)j * c->V, (size_t)c->V * sizeof(float));
    if (pick_lp_out) {      // the columns of `o`, at their offsets in the host copy
      const double* plp = reinterpret_cast<const double*>(lpbytes.data() + lp_span(b, o.lp));
      const double* tlp = reinterpret_cast<const double*>(lpbytes.data() + lp_span(b, o.top_lp));
      const int32_t* tid = reinterpret_cast<const int32_t*>(lpbytes.data() + lp_span(b, o.top_ids));
      pick_lp_out[i] = plp[j];
      for (int q = 0; q < top_k; ++q) { top_ids_out[(size_t)i * top_k + q] = tid[(size_t)j * top_k + q]; top_lp_out[(size_t)i * top_k + q] = tlp[(size_t)j * top_k + q]; }
    }
  }
  if (any) bt_sampler_finish(b, n, rng_state, ord.data());
  bp_set_next(c, n, seqs, n_tokens, pos0);
  return L2_OK;
}

extern "C" int l2_step_batch(l2_ctx* c, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                             const double* temperature, const double* topp, uint64_t* rng_state, int32_t* picks_out, float* logits_out) {
  return bt_step(c, n, seqs, n_tokens, tokens, pos0, temperature, topp, rng_state, picks_out, logits_out, 0, nullptr, nullptr, nullptr);
}

extern "C" int l2_step_batch_logprobs(l2_ctx* c, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                                      const double* temperature, const double* topp, uint64_t* rng_state, int32_t* picks_out, float* logits_out,
                                      int top_k, double* pick_lp_out, int32_t* top_ids_out, double* top_lp_out) {
  if (!pick_lp_out) return fail(L2_E_ARG, "null pick_lp_out");
  const int rc = lp_check_k(top_k, top_ids_out, top_lp_out);
  if (rc) return rc;
  return bt_step(c, n, seqs, n_tokens, tokens, pos0, temperature, topp, rng_state, picks_out, logits_out, top_k, pick_lp_out, top_ids_out, top_lp_out);
}

extern "C" int l2_step_batch_constrained(l2_ctx* c, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                                         const double* temperature, const double* topp, uint64_t* rng_state, int32_t* picks_out, float* logits_out,
                                         int top_k, double* pick_lp_out, int32_t* top_ids_out, double* top_lp_out,
                                         const int32_t* mask_of_row, int n_masks, const uint32_t* masks,
                                         const int32_t* bias_count, const int32_t* bias_ids, const float* bias_vals) {
  if (!pick_lp_out && top_k != 0) return fail(L2_E_ARG, "top_k %d with a null pick_lp_out", top_k);
  int rc = pick_lp_out ? lp_check_k(top_k, top_ids_out, top_lp_out) : L2_OK;
  if (rc) return rc;
  const BtConstraint cs = {mask_of_row, n_masks, masks, bias_count, bias_ids, bias_vals};
  rc = cs_check_free(n, cs);
  if (rc) return rc;
  return bt_step(c, n, seqs, n_tokens, tokens, pos0, temperature, topp, rng_state, picks_out, logits_out, top_k, pick_lp_out, top_ids_out, top_lp_out, &cs);
}

extern "C" int l2_step_batch_sampling(l2_ctx* c, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                                      const double* temperature, const double* topp, uint64_t* rng_state, int32_t* picks_out, float* logits_out,
                                      int top_k, double* pick_lp_out, int32_t* top_ids_out, double* top_lp_out,
                                      const int32_t* mask_of_row, int n_masks, const uint32_t* masks,
                                      const int32_t* bias_count, const int32_t* bias_ids, const float* bias_vals,
                                      const l2_sample_controls* sc) {
  if (!pick_lp_out && top_k != 0) return fail(L2_E_ARG, "top_k %d with a null pick_lp_out", top_k);
  int rc = pick_lp_out ? lp_check_k(top_k, top_ids_out, top_lp_out) : L2_OK;
  if (rc) return rc;
  const BtConstraint cs = {mask_of_row, n_masks, masks, bias_count, bias_ids, bias_vals};
  rc = cs_check_free(n, cs);
  if (rc) return rc;
  if (sc) {
    rc = sc_check_free(n, *sc, temperature, -1);
    if (rc) return rc;
  }
  return bt_step(c, n, seqs, n_tokens, tokens, pos0, temperature, topp, rng_state, picks_out, logits_out, top_k, pick_lp_out, top_ids_out, top_lp_out, &cs, sc);
}

// Diagnostic: the two rewriting launches of the sampling controls on caller-supplied rows, with buffers of its own.
extern "C" int l2_debug_sample_controls(int device, int n_rows, int vocab, const float* logits, const double* temperature,
                                        const l2_sample_controls* sc, float* penalised_out, float* truncated_out) {
  if (!logits || !sc) return fail(L2_E_ARG, "null logits / sc");
  if (vocab < 1 || vocab > (int)l2s::MAX_VOCAB) return fail(L2_E_ARG, "vocab %d outside [1, %d]", vocab, (int)l2s::MAX_VOCAB);
  int rc = sc_check_free(n_rows, *sc, temperature, SC_HIST_MAX);
  if (rc) return rc;
  for (int i = 0; temperature && i < n_rows; ++i)
    if (!(temperature[i] == temperature[i])) return fail(L2_E_ARG, "row %d: temperature is NaN", i);
  rc = sc_check_shape(vocab, SC_HIST_MAX, n_rows, *sc);
  if (rc) return rc;
  ScPlan sp;
  sc_tables(n_rows, vocab, *sc, temperature, nullptr, sp);
  std::vector<double> params(2 * (size_t)n_rows, 0.0);      // {temperature, topp}: topp is not read here
  for (int i = 0; temperature && i < n_rows; ++i) params[2 * i] = temperature[i];
  HIPCHK(hipSetDevice(device));      // (left as the thread's current device, as l2_debug_running_sums leaves it)
  const size_t elems = (size_t)n_rows * vocab;
  float *dx = nullptr, *dt = nullptr;
  int* dc = nullptr;
  char* tb = nullptr;
  double* dp = nullptr;
  hipError_t e = hipMalloc(&dx, elems * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&dt, elems * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&dc, elems * sizeof(int));
  if (e == hipSuccess) e = hipMemset(dc, 0, elems * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&tb, sp.h.size());
  if (e == hipSuccess) e = hipMalloc(&dp, params.size() * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(dx, logits, elems * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(tb, sp.h.data(), sp.h.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dp, params.data(), params.size() * sizeof(double), hipMemcpyHostToDevice);
  rc = L2_OK;
  if (e == hipSuccess) {
    const ControlArgs xa = sc_args(dx, dt, tb, sp, dc, dp, vocab);
    if (sp.penalise) rc = sc_enqueue_penalties(xa, n_rows, nullptr);
    if (!rc) rc = sc_enqueue_truncation(xa, n_rows, nullptr);
    if (!rc) e = hipDeviceSynchronize();
    if (!rc && e == hipSuccess && penalised_out) e = hipMemcpy(penalised_out, dx, elems * sizeof(float), hipMemcpyDeviceToHost);
    if (!rc && e == hipSuccess && truncated_out) e = hipMemcpy(truncated_out, dt, elems * sizeof(float), hipMemcpyDeviceToHost);
  }
  hipFree(dx); hipFree(dt); hipFree(dc); hipFree(tb); hipFree(dp);
  if (rc) return rc;
  if (e != hipSuccess) return fail(L2_E_HIP, "sample controls: %s", hipGetErrorString(e));
  return L2_OK;
}

extern "C" int l2_read_seq_cache(l2_ctx* c, int seq, int which, int layer, float* out, size_t n_floats) {
  if (!c || !out) return fail(L2_E_ARG, "null argument");
  if (!c->bt) return fail(L2_E_STATE, "no sequences reserved: call l2_seq_reserve first");
  const BatchState* b = c->bt;
  if (seq < 0 || seq >= b->n_seqs) return fail(L2_E_ARG, "sequence %d outside [0, n_seqs = %d)", seq, b->n_seqs);
  if (which != L2_S_KEY_CACHE && which != L2_S_VALUE_CACHE) return fail(L2_E_ARG, "state %d is not a cache (L2_S_KEY_CACHE / L2_S_VALUE_CACHE)", which);
  if (layer < -1 || layer >= c->L) return fail(L2_E_ARG, "layer %d out of range", layer);
  const size_t slab = (size_t)c->S * c->d, n = layer < 0 ? slab * c->L : slab;
  if (n_floats != n) return fail(L2_E_ARG, "cache has %zu floats, caller asked for %zu", n, n_floats);
  const float* src = (which == L2_S_KEY_CACHE ? b->kc[seq] : b->vc[seq]) + (layer < 0 ? 0 : slab * layer);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out, src, n * sizeof(float), hipMemcpyDeviceToHost));
  return L2_OK;
}

// ---- cache prefix reuse (l2_seq_fork) --------------------------------------------------------------
// One bt_fork_kernel launch (fork.hip.h) on the context's stream: 2 L segments, each read once and stored to every destination.  The
// checks that need no context come first (tests/test_fork_cpu.py calls them with a null one).
extern "C" int l2_seq_fork(l2_ctx* c, int src, int n_dst, const int32_t* dsts, int n_pos) {
  if (!dsts) return fail(L2_E_ARG, "null dsts");
  if (n_dst < 1 || n_dst > FK_MAX_DST) return fail(L2_E_ARG, "n_dst %d outside [1, %d]", n_dst, (int)FK_MAX_DST);
  if (n_pos < 1) return fail(L2_E_ARG, "n_pos %d < 1", n_pos);
  if (src < 0) return fail(L2_E_ARG, "src %d < 0", src);
  if (!c) return fail(L2_E_ARG, "null context");
  if (!c->bt) return fail(L2_E_STATE, "no sequences reserved: call l2_seq_reserve first");
  BatchState* b = c->bt;
  if (n_dst > b->n_seqs - 1) return fail(L2_E_ARG, "n_dst %d outside [1, n_seqs - 1 = %d]", n_dst, b->n_seqs - 1);
  if (src >= b->n_seqs) return fail(L2_E_ARG, "src %d outside [0, n_seqs = %d)", src, b->n_seqs);
  if (n_pos > c->S) return fail(L2_E_ARG, "n_pos %d outside [1, seq_len=%d]", n_pos, c->S);
  ForkArgs a;
  memset(&a, 0, sizeof(a));
  bool seen[BT_MAX] = {};
  for (int i = 0; i < n_dst; ++i) {
    const int s = dsts[i];
    if (s < 0 || s >= b->n_seqs) return fail(L2_E_ARG, "dsts[%d]: sequence %d outside [0, n_seqs = %d)", i, s, b->n_seqs);
    if (s == src) return fail(L2_E_ARG, "dsts[%d]: sequence %d is the source", i, s);
    if (seen[s]) return fail(L2_E_ARG, "dsts[%d]: sequence %d appears twice in one call", i, s);
    seen[s] = true;
    a.dst4[i >> 2] |= (unsigned)s << (8 * (i & 3));
  }
  const int have = bt_next(c, src);
  if (c->opt_pos_check && n_pos > have)
    return fail(L2_E_STATE, "L2_CHECK_POS: n_pos %d rows of sequence %d were asked for, cache rows 0 .. %d have been written", n_pos, src, have - 1);
  HIPCHK(hipSetDevice(c->device));
  a.seq_kc = b->d_kc; a.seq_vc = b->d_vc;
  a.layer_floats = (size_t)c->S * c->d;
  a.pieces = (unsigned)((size_t)n_pos * c->d / 4);      // (d % 16 == 0: bt_refusal; a layer's slab is below 4 GiB: l2_create)
  a.src = src; a.m = n_dst;
  // enough workgroups to fill the chip a few times over, each thread FK_U pieces per trip
  const unsigned per = FK_THREADS * FK_U, want = (a.pieces + per - 1) / per, cap = std::max(1u, 8192u / (2u * (unsigned)c->L));
  const dim3 grid(std::min(want, cap), 2 * c->L);
  if (dev_int("L2_FORK_NT_STORE", 0)) hipLaunchKernelGGL(bt_fork_kernel<true>, grid, dim3(FK_THREADS), 0, c->stream, a);
  else hipLaunchKernelGGL(bt_fork_kernel<false>, grid, dim3(FK_THREADS), 0, c->stream, a);
  LCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int i = 0; i < n_dst; ++i) bt_set_next(c, dsts[i], n_pos);
  return L2_OK;
}
