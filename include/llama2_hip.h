/*
 * llama2_hip.h -- C ABI of libllama2hip.so: the MI355X (gfx950) forward pass that drops in at the
 * single call `transformer(token, pos, config, state, weights)` of wizzard0/llama2.ts
 * (/root/reference/llama2.ts:468, body :205-303).
 *
 * The reference has no FFI/plugin interface (every function is module-private, llama2.ts:526 just
 * calls main()), so these entry points are what an N-API / bun:ffi / ctypes binding for that call
 * would bind; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types; every function returns 0 on success
 * or a negative L2_E_* code (l2_last_error() gives the text); nothing throws across the ABI; a
 * context is bound to one device, is not thread-safe, and distinct contexts are independent.  Host
 * pointers are only read/written during the call and never retained.
 */
#ifndef LLAMA2_HIP_H
#define LLAMA2_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 5): l2_bench_tokens, option keys 5-7, L2_TP_SOLO_ID / l2_tp_mode 5 and the L2_TP_FENCED switch joined the surface after 2 -- a
 * binding built against it refuses an older library at open() (l2_abi_version), not at the first call that is missing.
 * 4 (round 5): option key L2_OPT_AQL_QUEUE
 * 5 (round 6): option keys L2_OPT_PREFILL_F32_MFMA, L2_OPT_CHECK_POS; l2_dispatch_reason
 * The batched decode of independent sequences (l2_seq_reserve .. l2_read_seq_cache, option key L2_OPT_SEQS) joined the surface without a
 * version step: it only adds, and a binding detects it by the presence of the l2_seq_reserve symbol.  So did its sampled loop
 * (l2_decode_sample_batch, option keys L2_OPT_BATCH_SAMPLED_TOKENS / _SERIAL), detected by its own symbol, and so were the packed
 * prompts (l2_seq_prefill_batch) and the mixed step (l2_step_batch), the per-token log-probabilities (l2_seq_score_batch,
 * l2_step_batch_logprobs), constrained picks (l2_step_batch_constrained), sampling controls (l2_step_batch_sampling), and so is the cache prefix copy (its one call is declared
 * below, beside the cache read). */
#define L2_ABI_VERSION 5

enum {
  L2_OK = 0,
  L2_E_ARG = -1,     /* bad argument (null pointer, index out of range, wrong size) */
  L2_E_CONFIG = -2,  /* unsupported header (dim % n_heads, odd head_size, non-positive sizes) */
  L2_E_HIP = -3,     /* a HIP runtime call failed */
  L2_E_STATE = -4,   /* call order violated (forward before all tensors uploaded, a kept-state read without L2_OPT_KEEP_STATE) */
  L2_E_NOGPU = -5,   /* no gfx950 device visible */
  L2_E_COMM = -6     /* RCCL failure (tensor-parallel contexts) */
};

/* Tensor kinds = fields of the reference's TransformerWeights in checkpoint order
 * (readWeights, llama2.ts:112-129). */
enum {
  L2_T_TOKEN_EMBEDDING = 0, /* token_embedding_table (V,d)   llama2.ts:114 */
  L2_T_RMS_ATT = 1,         /* rms_att_weight[l] (d)         :115 */
  L2_T_WQ = 2,              /* wq[l] (d,d)                   :116 */
  L2_T_WK = 3,              /* wk[l] (d,d)                   :117 */
  L2_T_WV = 4,              /* wv[l] (d,d)                   :118 */
  L2_T_WO = 5,              /* wo[l] (d,d)                   :119 */
  L2_T_RMS_FFN = 6,         /* rms_ffn_weight[l] (d)         :120 */
  L2_T_W1 = 7,              /* w1[l] (h,d)                   :121 */
  L2_T_W2 = 8,              /* w2[l] (d,h)                   :122 */
  L2_T_W3 = 9,              /* w3[l] (h,d)                   :123 */
  L2_T_RMS_FINAL = 10,      /* rms_final_weight (d)          :124 */
  L2_T_FREQ_REAL = 11,      /* freq_cis_real (S,hs/2)        :125 */
  L2_T_FREQ_IMAG = 12,      /* freq_cis_imag (S,hs/2)        :126 */
  L2_T_WCLS = 13,           /* wcls (V,d), only when the header's vocab_size < 0  :127 */
  L2_T_COUNT = 14
};

/* RunState fields (llama2.ts:131-146) readable with l2_read_state. */
enum {
  L2_S_X = 0, L2_S_XB = 1, L2_S_XB2 = 2, L2_S_HB = 3, L2_S_HB2 = 4, L2_S_Q = 5, L2_S_K = 6, L2_S_V = 7,
  L2_S_ATT = 8, L2_S_LOGITS = 9, L2_S_KEY_CACHE = 10, L2_S_VALUE_CACHE = 11
};

/* l2_set_option keys */
enum {
  L2_OPT_EXACT_ATTENTION = 1, /* 1: value-accumulate rounds to fp32 at every timestep in t order, exactly as
                                 llama2.ts:260-265 does (the reference's own rounding points in that loop; slower; > 99.9 % of logits
                                 come out bit-identical, the rest within 1 ulp: the tree-ordered fp64 sums elsewhere remain); 0 (default):
                                 fp64 partial sums, one rounding */
  L2_OPT_USE_GRAPH = 2,       /* 1 (default): the step of a context length level is recorded once and replayed per token (as packets on the
                                 library's own queue, L2_OPT_AQL_QUEUE, or as a captured hipGraph); 0: eager launches */
  L2_OPT_KEEP_STATE = 3,      /* 1: the RunState fields that only transformer() itself reads (llama2.ts:131-146: att, k, v, hb2, xb2,
                                 the xb of the FFN half, the final-normed x) are also written out for l2_read_state (parity
                                 tests); 0 (default): they stay on chip and reading them AFTER a forward returns L2_E_STATE -- q, hb, logits and
                                 the KV caches are always there */
  L2_OPT_PACKED_MIB = 4,      /* read-only (l2_get_option): MiB of device memory held by the repacked copies of the matrices the
                                 streaming kernels read; 0 before the first step and for models that need none */
  L2_OPT_WEIGHT_MIB = 5,      /* read-only: MiB of device memory held by ALL weights right now (row-major tensors + repacked copies).  After
                                 the first step a repacked matrix exists once: its row-major tensor has been given back */
  L2_OPT_SAMPLED_TOKENS = 6,  /* read-only: tokens l2_decode_sample has picked on this context with temperature != 0 (saturates at INT_MAX) */
  L2_OPT_SAMPLED_SERIAL = 7,  /* read-only: of those, the tokens whose running sums came within the proven margin of the threshold and were
                                 therefore picked by the reference's loop run as written (csrc/sampler_margin.hip.h); the others by the
                                 margin rule */
  L2_OPT_AQL_QUEUE = 8,       /* 1 (default): the recorded step of l2_decode_greedy, l2_decode_sample AND of the blocking l2_forward is submitted as
                                 hand-written AQL packets on a queue of the library's own (csrc/aql_queue.h: barrier bit, agent-scope release, no
                                 acquire between the launches of a token); 0: a replayed hipGraph per token.  Reading it tells what the context
                                 uses now: 1 the queue, 0 hipGraphs / eager launches (switched off, L2_USE_GRAPH=0, RCCL collectives in the step,
                                 a profiler's tool library in the process, or the queue was given up: l2_dispatch_reason() says which) */
  L2_OPT_PREFILL_F32_MFMA = 9, /* 1: l2_prefill's register-blocked GEMMs accumulate in fp32 on v_mfma_f32_16x16x4_f32 -- a k-ordered fmaf chain per
                                 element instead of the reference's fp64 accumulate (llama2.ts:196-203): faster prompt ingestion, logits within
                                 1e-4 on the fixtures, NOT bit-level parity with the reference (measured exactness);
                                 0 (default): fp64 MFMA, the reference's arithmetic.  Decode is never affected */
  L2_OPT_CHECK_POS = 10,      /* 1 (or L2_CHECK_POS=1 in the environment at creation): l2_forward / l2_prefill refuse (L2_E_STATE) a position that
                                 neither restarts at 0 nor continues the sequence -- the reference's loop feeds pos = 0, 1, 2, ... (llama2.ts:464,
                                 496) and attention reads whatever rows 0 .. pos - 1 the cache holds; 0 (default): any position is accepted.
                                 Applies per sequence to the batch calls below (sequence 0 shares its position with l2_forward / l2_prefill) */
  L2_OPT_SEQS = 11,           /* read-only: sequences reserved by l2_seq_reserve (0 before it) */
  L2_OPT_BATCH_SAMPLED_TOKENS = 12, /* read-only: tokens l2_decode_sample_batch and l2_step_batch have sampled (temperature != 0), saturating */
  L2_OPT_BATCH_SAMPLED_SERIAL = 13, /* read-only: of those, the ones the margin form's serial loop picked */
  L2_OPT_ATTN_WO_STREAM = 14  /* read-only: 1 when a step of the last forward / decode call ran attention and wo as ONE launch (one GPU, streaming form) */
};

typedef struct l2_ctx l2_ctx;

int l2_abi_version(void);
int l2_device_count(void);                 /* number of visible HIP devices, or a negative code */
const char* l2_last_error(void);           /* thread-local text of the last failure */

/* Replaces readConfig + newRunState (llama2.ts:80-93, 147-163): `cfg` is the 7 header int32 verbatim
 * (sign of vocab_size kept).  Allocates weights, activations and the [L][S][d] KV caches in HBM. */
int l2_create(const int32_t cfg[7], int device, l2_ctx** out);
void l2_destroy(l2_ctx* ctx);

/* SURVEY.md 8(f4) -- checkpoints newer than the reference understands.  The reference parses n_kv_heads and ignores
 * it (llama2.ts:86, 117-118: wk / wv are always (d, d)) and reads the RoPE tables from the file (:125-126); l2_create
 * does the same.  l2_create_ex honours, on request:
 *   L2_F_GQA            n_kv_heads < n_heads: wk / wv are (n_kv_heads * head_size, d) per layer, the KV caches hold
 *                       n_kv_heads * head_size floats per position and query head h attends over cache head
 *                       h / (n_heads / n_kv_heads) -- grouped-query attention as llama2.c's run.c defines it;
 *   L2_F_GENERATE_ROPE  no freq_cis tensors will be uploaded: the tables are computed at creation the way run.c
 *                       computes them per position (fp32 powf / cosf / sinf).
 * Neither is pinned by the reference (it cannot run such checkpoints); the oracle's restatement is our own. */
enum { L2_F_GQA = 1, L2_F_GENERATE_ROPE = 2 };
int l2_create_ex(const int32_t cfg[7], int device, unsigned flags, l2_ctx** out);

/* Tensor-parallel context: rank `tp_rank` of `tp_size` owns heads / FFN rows
 * [rank*H/G, ...).  `nccl_id` is the 128-byte ncclUniqueId produced by l2_tp_unique_id on rank 0 and
 * handed to the others by the caller (e.g. over torch.distributed).  tp_size 1 == l2_create. */
int l2_tp_unique_id(void* id_out_128);
/* How this context's tensor-parallel step runs: 0 not tensor parallel, 1 eager launches with RCCL collectives (this RCCL
 * refused stream capture, or L2_USE_GRAPH=0), 2 one hipGraph per token with the RCCL collectives captured in it, 3 one hipGraph
 * per token with the one-shot peer-to-peer all-reduce, 4 loopback test group (L2_TEST_HOOKS), 5 shard-timing context (L2_TP_SOLO_ID). */
int l2_tp_mode(l2_ctx* ctx);
int l2_create_tp(const int32_t cfg[7], int device, int tp_rank, int tp_size, const void* nccl_id, l2_ctx** out);
/* Measurement only: a 128-byte id that starts with this text creates ONE rank of a tp_size group with no peers -- its shard of the
 * weights and of the step, the exchange kernels running against its own inbox (every wait satisfied at once).  It times a rank's
 * share of the step without a multi-GPU node (bench.py `tp_predicted`); what it decodes is meaningless (l2_tp_mode 5). */
#define L2_TP_SOLO_ID "L2-SOLO-SHARD-TIMING"

/* Replaces the hand-over of one Float32Array of TransformerWeights (readWeights, llama2.ts:112-129):
 * call once per array right after FileHandleReader.getF32Array returns it (llama2.ts:51-59).
 * `layer` is the index into the Float32Array[] for per-layer tensors, -1 otherwise.  The bytes are
 * copied to HBM before the call returns. */
int l2_upload(l2_ctx* ctx, int tensor_kind, int layer, const float* host, size_t n_floats);

/* Next row of SURVEY.md 8(f2): the checkpoint load path (FileHandleReader + readWeights, llama2.ts:44-68,
 * 112-129) done natively: reads the 28-byte header of the llama2.c-v0 file at `path`, creates the context and
 * streams every tensor to HBM through two pinned staging buffers (file reads overlap the host-to-device
 * copies), so host memory never holds more than 2 x 64 MiB of a 27 GB checkpoint.  Tensor-parallel ranks pass
 * their rank / size / id and receive only their slices; tp_size 1 ignores them.  `bytes_read` (optional)
 * returns the file bytes consumed.  Equivalent to l2_create + one l2_upload per Float32Array. */
int l2_load_checkpoint(const char* path, int device, int tp_rank, int tp_size, const void* nccl_id, l2_ctx** out,
                       uint64_t* bytes_read);
/* (l2_load_checkpoint also reads a llama2.c "version 1" file -- magic "ak42", 256-byte header, norms first, no freq_cis; fp32:
 * detected by its magic and loaded with L2_F_GQA | L2_F_GENERATE_ROPE.  A file without the magic is the v0 layout above.) */

/* The 7 header ints of a context (what readConfig parsed). */
int l2_get_header(l2_ctx* ctx, int32_t cfg_out[7]);

/* Fill every tensor on the device with the repo's deterministic synthetic generator (same values as
 * oracle/llama2_oracle.c:orc_synth_tensor); used by bench.py for shapes too large to ship. */
int l2_synth_fill(l2_ctx* ctx, uint32_t seed);
/* Read back part of a weight tensor (tests of l2_upload / l2_synth_fill). */
int l2_read_tensor(l2_ctx* ctx, int tensor_kind, int layer, size_t offset, float* out, size_t n_floats);

/* Replaces transformer(token, pos, p, s, w) (llama2.ts:205-303, call site :468).  Blocking: when it
 * returns, logits_out[0..V) holds state.logits for this position and the device KV cache holds rows
 * 0..pos.  pos must be 0 <= pos < seq_len; token in [0, V).  The reference's loop feeds pos = 0, 1, 2, ... (llama2.ts:464,
 * 496); any pos is accepted here -- attention then reads whatever rows 0..pos-1 the cache holds from earlier calls
 * (L2_OPT_CHECK_POS makes a position that skips ahead an error).  logits_out may be NULL (logits stay readable through l2_logits_host / l2_read_state). */
int l2_forward(l2_ctx* ctx, int token, int pos, float* logits_out);
/* Pinned host buffer (V floats) that l2_forward fills; a binding may wrap it as RunState.logits to
 * skip the copy into logits_out. */
float* l2_logits_host(l2_ctx* ctx);

/* Next row of SURVEY.md 8(f1): greedy decode (`-t 0`, argmax llama2.ts:364-366: first maximum) kept on
 * the device -- the loop llama2.ts:465-508 with temperature 0 and no prompt, minus printing.  Feeds
 * `first_token` at pos0, then each argmax; writes the `steps` chosen tokens to tokens_out[0..steps).
 * Does not stop at BOS (the caller truncates, llama2.ts:499). */
int l2_decode_greedy(l2_ctx* ctx, int first_token, int pos0, int steps, int32_t* tokens_out);

/* Rest of SURVEY.md 8(f1): the sampled branch of the loop (llama2.ts:480-493) kept on the device -- temperature
 * scaling and softmax in place of state.logits (:481-485), `sample` (:368-376) or, when 0 < topp < 1, `sample_topp`
 * (:378-394: stable descending sort, the element that crosses topp is never returned, fall-through returns id 0),
 * driven by the reference's xorshift* generator (:348-360).  `*rng_state` is the 64-bit state the reference keeps in
 * the BigInt `rng_seed` (what `-s` parsed, non-zero); it is advanced by one draw per sampled token and written back.
 * The SAME token ids come out for the same seed: what the reference's loops return is an INDEX -- the first element whose
 * sequentially accumulated running sum passes the threshold -- and the device decides every comparison those loops make from
 * tree sums plus a proven margin (csrc/margin_rule.h); a token whose running sum comes within that margin of its threshold
 * (about 4 in 100 000) is picked by the reference's loop run as written, element by element (L2_OPT_SAMPLED_SERIAL counts
 * them).  temperature == 0 is l2_decode_greedy (no draw).  Like l2_decode_greedy it does not stop at BOS. */
int l2_decode_sample(l2_ctx* ctx, int first_token, int pos0, int steps, double temperature, double topp,
                     uint64_t* rng_state, int32_t* tokens_out);

/* Diagnostic for the sampler's core: sums_out[i] = S_i with S_i = fl(S_{i-1} + values[i]) in fp64 (the reference's
 * `cumProb += x[i]` / `sum += x[i]` loops), computed on the device by the exact parallel algorithm of sampler.hip.
 * `values` must be finite and >= 0.  Tests compare it with the serial loop on adversarial vectors. */
int l2_debug_running_sums(int device, const float* values, size_t n, double* sums_out);

/* Next row of SURVEY.md 8(f3): prompt ingestion.  The reference runs one transformer() per prompt token and
 * ignores the logits (llama2.ts:471-473); this feeds `n_tokens` tokens at positions pos0 .. pos0+n_tokens-1 in
 * chunks of up to 64 (one, two or four 16-token MFMA tiles) that share every weight read (fp64 MFMA GEMMs), leaves the KV cache exactly as the n_tokens
 * separate calls would, and returns the logits of the LAST position in logits_out (may be NULL).  Shapes whose
 * dim / hidden_dim are not multiples of 16 fall back to n_tokens l2_forward calls. */
int l2_prefill(l2_ctx* ctx, const int32_t* tokens, int n_tokens, int pos0, float* logits_out);

/* Batched greedy decode: several independent sequences share every weight read.  The reference's loop decodes one sequence
 * (llama2.ts:465-508); each row of a batch step is one transformer() call (llama2.ts:205-303) of its own sequence, computed by fp64-MFMA
 * GEMMs over the rows with prefill's arithmetic (exact products, fp64 accumulation, one fp32 rounding per stored element).
 * Independent sequences sharing this context's weights.  Sequence 0 is the context's own KV cache (the one l2_forward, l2_prefill and
 * the device loops use); l2_seq_reserve allocates caches for sequences 1 .. n_seqs-1 ([L][S][d] each) plus the batch buffers.
 * 1 <= n_seqs <= 64.  Called once per context.  L2_E_CONFIG (with the reason) for shapes the batch path does not cover: tensor
 * parallel, grouped-query attention honoured, dim or hidden_dim not a multiple of 16; L2_E_HIP (nothing held, the context usable) when
 * the device memory is not there. */
int l2_seq_reserve(l2_ctx* ctx, int n_seqs);
/* l2_prefill into sequence `seq`'s cache (seq 0: exactly l2_prefill). */
int l2_seq_prefill(l2_ctx* ctx, int seq, const int32_t* tokens, int n_tokens, int pos0, float* logits_out);
/* Prompt ingestion for n sequences at once: sequence seqs[i] is fed n_tokens[i] tokens at positions pos0[i] .. pos0[i]+n_tokens[i]-1.
 * tokens holds the prompts back to back, in row order.  The cache of every named sequence ends up as l2_seq_prefill would leave it.
 * logits_out (may be NULL) receives n x V floats: row i holds the logits of sequence seqs[i]'s LAST position.
 * The prompt rows are packed densely into launch sequences of up to 256 rows (64 on shapes the register-blocked GEMMs do not cover)
 * that stream every weight once for all of them; a prompt may straddle launch sequences.  Blocking.  L2_E_STATE before l2_seq_reserve;
 * L2_E_ARG for a null pointer other than logits_out, n outside [1, n_seqs], a sequence out of range or named twice, n_tokens[i] < 1,
 * a token outside [0, vocab_size) or pos0[i] + n_tokens[i] > seq_len; L2_E_STATE for an L2_OPT_CHECK_POS skip-ahead of any sequence.
 * A refused call writes nothing.  Sequence 0 is the context's own cache; the single-sequence state (its logits among it) is left alone. */
int l2_seq_prefill_batch(l2_ctx* ctx, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                         float* logits_out);
/* One transformer() step for each of n rows: row i feeds tokens[i] at pos[i] of sequence seqs[i] (distinct within a call).
 * Blocking.  logits_out (may be NULL) receives n x V floats, row i = that sequence's logits.  L2_E_STATE before l2_seq_reserve. */
int l2_forward_batch(l2_ctx* ctx, int n, const int32_t* seqs, const int32_t* tokens, const int32_t* pos, float* logits_out);
/* Device-resident greedy loop over n sequences: row i feeds first_tokens[i] at pos0[i], then its own argmax each step
 * (first maximum, llama2.ts:364-366).  tokens_out is n x steps, row-major per sequence.  Does not stop at BOS.  pos0[i] + steps <= seq_len. */
int l2_decode_greedy_batch(l2_ctx* ctx, int n, const int32_t* seqs, const int32_t* first_tokens, const int32_t* pos0,
                           int steps, int32_t* tokens_out);
/* The sampled device loop over n sequences: row i feeds first_tokens[i] at pos0[i] of sequence seqs[i], then its own pick, `steps` times,
 * each row with its own settings (llama2.ts:476-493): temperature[i] == 0 takes the argmax (the rules of l2_decode_greedy_batch, no draw,
 * rng_state[i] left alone); otherwise logits / temperature[i] (any sign), softmax, then `sample` when topp[i] <= 0 or >= 1, else
 * `sample_topp`, with one xorshift* draw from rng_state[i] per token.  The tokens are exactly what the reference's sampler returns when
 * it is fed this path's own logits (those of l2_forward_batch for the same rows).  tokens_out is n x steps, row-major per sequence;
 * rng_state is written back only on success.  Does not stop at BOS.  Argument rules of l2_decode_greedy_batch, plus: L2_E_ARG for a null
 * temperature / topp / rng_state or a NaN setting; L2_E_CONFIG when vocab_size exceeds the device sampler's limit and a row samples.
 * Every phase of the device sampler runs once per step for all rows (the margin form of l2_decode_sample, row by row); its
 * L2_SAMPLER_FORCE_SERIAL test hook applies, the A/B forms L2_SAMPLER_CHAIN / L2_SAMPLER_SERIAL do not.  The single-sequence sampler's
 * state and L2_OPT_SAMPLED_TOKENS / _SERIAL are left alone. */
int l2_decode_sample_batch(l2_ctx* ctx, int n, const int32_t* seqs, const int32_t* first_tokens, const int32_t* pos0, int steps,
                           const double* temperature, const double* topp, uint64_t* rng_state, int32_t* tokens_out);
/* One mixed step of continuous batching: decode rows and prompt chunks in one call, one pick per row made on the device.  Sequence
 * seqs[i] is fed n_tokens[i] tokens at positions pos0[i] .. pos0[i]+n_tokens[i]-1, exactly as l2_seq_prefill_batch feeds them (tokens
 * back to back in row order; every cache ends as l2_seq_prefill would leave it).  Then row i makes ONE pick from the logits of its run's
 * last position, by the rules of l2_decode_sample_batch: temperature[i] == 0 takes the argmax (no draw, rng_state[i] left alone),
 * otherwise logits / temperature[i], softmax, then `sample` or `sample_topp` with one xorshift* draw from rng_state[i].  temperature,
 * topp and rng_state all NULL: every row greedy.  picks_out (n ints) is required; logits_out (may be NULL) receives n x V floats, row
 * i = the unscaled logits row i's pick was made from; rng_state is written back only on success.  Runs of one row (decode rows) take
 * the decode attention form per (head, row) at any head size and position, runs of two or more the prompt path's 16-query tiles.
 * Blocking, eager launches on the context's stream.  Argument rules of l2_seq_prefill_batch, plus: L2_E_ARG for a null picks_out, some
 * but not all of temperature / topp / rng_state NULL, or a NaN setting; L2_E_CONFIG when a row samples and vocab_size exceeds the
 * device sampler's limit.  A refused call writes nothing.  L2_OPT_EXACT_ATTENTION, L2_OPT_PREFILL_F32_MFMA, L2_OPT_CHECK_POS and the
 * L2_SAMPLER_FORCE_SERIAL test hook apply; sampled tokens count into L2_OPT_BATCH_SAMPLED_TOKENS / _SERIAL.  Sequence 0 is the
 * context's own cache; the single-sequence state is left alone. */
int l2_step_batch(l2_ctx* ctx, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                  const double* temperature, const double* topp, uint64_t* rng_state, int32_t* picks_out, float* logits_out);
/* Teacher-forced scoring of n sequences.  Feeds exactly as l2_seq_prefill_batch does (same packing, same launch sequences: every
 * cache and every sequence's next position ends bit for bit as that call leaves it).  For every fed row r (R = sum n_tokens rows,
 * in call order) it writes lp_out[r] = log-softmax of that position's logits at targets[r] (fp64; targets[r] == -1: NaN),
 * argmax_out[r] (may be NULL) = the first maximum (llama2.ts:364-366), and for top_k > 0 the top_k largest logits' ids / lps
 * at top_ids_out[r * top_k ..] / top_lp_out[r * top_k ..] (descending; equal logits by ascending id; entry 0 = argmax_out[r]).
 * Each row's logits come from the last-row classifier's arithmetic (fp64 MFMA, one fp32 rounding per logit); then, in fp64,
 * lse = m + log(sum_j exp(x_j - m)) with m = max_j x_j and lp = x_t - lse.  A row holding a NaN or +inf logit, or none above -inf,
 * has NaN for every lp (its argmax and top ids still follow the first-maximum rules); a -inf logit of any other row has lp -inf.
 * Argument rules of l2_seq_prefill_batch, plus L2_E_ARG for a null targets or lp_out, a target outside [-1, vocab_size), top_k
 * outside [0, 20] or above vocab_size, and top_k > 0 with a null top array.  A refused call writes nothing.  L2_OPT_CHECK_POS,
 * L2_OPT_EXACT_ATTENTION and L2_OPT_PREFILL_F32_MFMA apply as they do to l2_seq_prefill_batch.  Sequence 0 is the context's own
 * cache; the single-sequence state is left alone.  Blocking. */
int l2_seq_score_batch(l2_ctx* ctx, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                       const int32_t* targets, int top_k, double* lp_out, int32_t* argmax_out, int32_t* top_ids_out, double* top_lp_out);
/* l2_step_batch, unchanged in every output (picks, rng states, logits, caches: bit for bit), plus for each row i:
 * pick_lp_out[i] = the log-probability of picks_out[i] under the UNSCALED logits (the model's distribution, temperature and top-p
 * not applied) and, for top_k > 0, that row's top_k ids / lps at top_ids_out[i * top_k ..] / top_lp_out[i * top_k ..], by the rules
 * of l2_seq_score_batch.  Argument rules of l2_step_batch, plus L2_E_ARG for a null pick_lp_out, top_k outside [0, 20] or above
 * vocab_size, and top_k > 0 with a null top array.  Sampled tokens count into L2_OPT_BATCH_SAMPLED_TOKENS / _SERIAL. */
int l2_step_batch_logprobs(l2_ctx* ctx, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                           const double* temperature, const double* topp, uint64_t* rng_state, int32_t* picks_out, float* logits_out,
                           int top_k, double* pick_lp_out, int32_t* top_ids_out, double* top_lp_out);
/* Constrained decoding: l2_step_batch_logprobs (pick_lp_out given) or l2_step_batch (pick_lp_out NULL: no log-probabilities, top_k
 * must be 0 and the top arrays are ignored) with a token mask and / or a logit bias list per row.  For such a row the logits of its
 * run's last position are rewritten on the device, after the classifier and before anything reads them:
 *   x'[j] = -inf                    the row has a mask and bit j of it is clear
 *   x'[j] = (float)(x[j] + bias_j)  j is allowed and in the row's bias list (one fp32 add)
 *   x'[j] = x[j]                    otherwise, bit for bit
 * and everything downstream sees x' and nothing else: the argmax, temperature scaling, softmax, `sample` / `sample_topp`, logits_out,
 * pick_lp_out and the top-k lists -- the log-probabilities are those of the constrained, renormalised distribution; disallowed ids
 * have lp -inf and sort last by ascending id (l2_seq_score_batch's rule for -inf logits).  The pick is what the reference's loop
 * (llama2.ts:476-493) returns when state.logits holds x', one draw per sampled row, with ONE rule on top: if the returned id is one
 * the row's mask does not allow -- only the `return 0` of llama2.ts:375 / :393 can be, e.g. whenever the most likely token alone
 * crosses topp -- the row's pick is the first maximum of x' (llama2.ts:364-366).  The draw has still been made and rng_state[i] is
 * what the reference would leave.  When id 0 is allowed a fall-through to 0 stays 0.  A row with no mask and no bias is untouched:
 * its outputs are bit for bit those of l2_step_batch / l2_step_batch_logprobs; caches and next positions always are.
 *   masks        n_masks bit sets of W = ceil(vocab_size / 32) words each: token j is bit j & 31 of word j >> 5; bits at or above
 *                vocab_size in the last word are ignored.  0 <= n_masks <= n.
 *   mask_of_row  [n], each in [-1, n_masks): the row's mask, -1 for none; several rows may name one mask.  NULL: no row is masked
 *                (n_masks must be 0, masks is ignored).
 *   bias_count   [n], each in [0, 256]; the rows' (id, value) pairs lie back to back in row order in bias_ids / bias_vals.  NULL: no
 *                bias.
 * Indices follow the call's rows.  L2_E_ARG, nothing written, in addition to l2_step_batch's rules: an index outside its range;
 * n_masks > 0 or a non-null mask_of_row with null masks; a mask that some row names and that allows no token below vocab_size; a
 * bias id outside [0, vocab_size) or repeated within a row; a non-finite bias value (a ban is the mask's job); a non-zero bias_count
 * with a null id or value array; a masked row with a negative temperature (-inf / T would become +inf).  The options, the
 * L2_SAMPLER_FORCE_SERIAL test hook and the L2_OPT_BATCH_SAMPLED_* counters behave as in l2_step_batch.
 * Joined the surface without a version step: a binding detects it by its symbol. */
int l2_step_batch_constrained(l2_ctx* ctx, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                              const double* temperature, const double* topp, uint64_t* rng_state, int32_t* picks_out, float* logits_out,
                              int top_k, double* pick_lp_out, int32_t* top_ids_out, double* top_lp_out,
                              const int32_t* mask_of_row, int n_masks, const uint32_t* masks,
                              const int32_t* bias_count, const int32_t* bias_ids, const float* bias_vals);
/* Sampling controls of a mixed step's rows: penalties on tokens already seen, top-k and min-p.  Every array follows the call's rows;
 * a NULL array switches its control off for every row.
 *   hist_count / hist_ids      row i's history: hist_count[i] token ids, the rows' lists back to back in row order.  c_j = how often
 *                              id j occurs in it.
 *   repetition, presence, frequency   STAGE A, visible.  For every j with c_j > 0, before the bias and the mask of the row:
 *       y     = rep == 1 ? x[j] : (x[j] > 0 ? (float)((double)x[j] / rep) : (float)((double)x[j] * rep))
 *       x'[j] = presence == 0 && frequency == 0 ? y : (float)((double)y - (presence + frequency * (double)c_j))
 *     each operation rounded on its own; an id with c_j == 0 is not written (bit for bit); -inf and NaN come out as the formula gives
 *     them.  The argmax, the sampler, logits_out, pick_lp_out and the top lists all see the penalised, then constrained row x'.
 *   sample_top_k, min_p        STAGE B, sampler-only, like top-p: for a row with temperature > 0 the row sampler reads
 *       x''[j] = x'[j]   fewer than sample_top_k ids rank before j (descending value, equal values by ascending id: the order of
 *                        the top lists; sample_top_k >= vocab_size truncates nothing) AND
 *                        (double)s_j - (double)s_max >= log(min_p), s_j = (float)((double)x'[j] / T), s_max its row maximum
 *       x''[j] = -inf    otherwise
 *     while logits_out, pick_lp_out and the top lists keep reading x'.  Top-p then acts on the renormalised survivors inside the
 *     unchanged sampler.  A greedy row ignores stage B.  If the sampler's pick is an id with x'' = -inf -- only the `return 0` of
 *     llama2.ts:375 / :393 can be, e.g. every time for sample_top_k = 1 under 0 < topp < 1 -- the pick is the first maximum of x''
 *     (llama2.ts:364-366); the draw has still been made and rng_state[i] is what the reference would leave. */
typedef struct l2_sample_controls {
  const int32_t* hist_count;    /* [n] each in [0, seq_len]; NULL: no row has a history */
  const int32_t* hist_ids;      /* the rows' histories back to back in row order, ids in [0, vocab_size) */
  const double* repetition;     /* [n] > 0 and finite, 1 = off; NULL: all 1 */
  const double* presence;       /* [n] finite; NULL: all 0 */
  const double* frequency;      /* [n] finite; NULL: all 0 */
  const int32_t* sample_top_k;  /* [n] >= 0, 0 = off; NULL: off */
  const double* min_p;          /* [n] in [0, 1], 0 = off; NULL: off */
} l2_sample_controls;
/* l2_step_batch_constrained with sampling controls: every parameter of that call, in its order, then `sc`.  sc == NULL is exactly
 * l2_step_batch_constrained; a row with no history (or repetition 1, presence 0, frequency 0), sample_top_k 0 and min_p 0 is
 * untouched: its outputs are bit for bit those of that call.  Caches, next positions, the options and the
 * L2_OPT_BATCH_SAMPLED_* counters behave as there.  Up to three launches join the step, each only when a row needs it: the
 * penalties (before the bias / mask rewrite), the truncated copy of the rows (before the row sampler, which then reads the copy),
 * the fall-through of the rows that truncate (after the pick; a row that is only masked keeps l2_step_batch_constrained's own rule, so
 * no row's pick depends on what the other rows of its call ask for).
 * L2_E_ARG, nothing written and nothing launched, in addition to that call's rules: a hist_count outside [0, seq_len]; a non-zero
 * count with a null hist_ids; a history id outside [0, vocab_size); a repetition that is not positive and finite; a presence or
 * frequency that is not finite; sample_top_k < 0; min_p outside [0, 1]; a NaN; a row with sample_top_k > 0 or min_p > 0 and a
 * negative temperature.  What needs no context is checked before the context is looked at.
 * Joined the surface without a version step: a binding detects it by its symbol. */
int l2_step_batch_sampling(l2_ctx* ctx, int n, const int32_t* seqs, const int32_t* n_tokens, const int32_t* tokens, const int32_t* pos0,
                           const double* temperature, const double* topp, uint64_t* rng_state, int32_t* picks_out, float* logits_out,
                           int top_k, double* pick_lp_out, int32_t* top_ids_out, double* top_lp_out,
                           const int32_t* mask_of_row, int n_masks, const uint32_t* masks,
                           const int32_t* bias_count, const int32_t* bias_ids, const float* bias_vals,
                           const l2_sample_controls* sc);
/* Diagnostic for the two rewriting launches of the sampling controls, with no model: n_rows (1 .. 64) rows of `vocab`
 * (1 .. the device sampler's limit) caller-supplied logits go through stage A into penalised_out and through stage B into
 * truncated_out (each n_rows x vocab floats; either may be NULL).  temperature: [n_rows], NULL = every row greedy (stage B copies).
 * The rules of `sc` are those of the step, with hist_count bounded by 65 536 instead of seq_len.  Synchronous; tests compare it
 * bit for bit with a numpy statement of the rules. */
int l2_debug_sample_controls(int device, int n_rows, int vocab, const float* logits, const double* temperature,
                             const l2_sample_controls* sc, float* penalised_out, float* truncated_out);
/* Read sequence `seq`'s key / value cache (which = L2_S_KEY_CACHE / L2_S_VALUE_CACHE; layer -1 = all), like l2_read_state. */
int l2_read_seq_cache(l2_ctx* ctx, int seq, int which, int layer, float* out, size_t n_floats);
/* KV-cache prefix reuse.  Copy cache rows 0 .. n_pos-1 (every layer, keys and values) of sequence `src` into the n_dst sequences
 * dsts[0 .. n_dst): a cache row of position p depends on tokens 0 .. p only, so a sequence that starts with the same n_pos tokens as
 * `src` continues from these rows at position n_pos instead of being fed them again.  One device launch reads the source once and
 * stores it to every destination.  Afterwards rows 0 .. n_pos-1 of every destination are bit for bit the source's; every other byte
 * of every cache, and the source, are untouched.  Blocking.  Sequence 0 is the context's own cache (it may be the source or a
 * destination); the rest of the single-sequence state is left alone.
 * L2_E_ARG (nothing written) for a null context or dsts, n_dst outside [1, n_seqs - 1], src or a destination outside [0, n_seqs), a
 * destination equal to src or named twice, n_pos outside [1, seq_len]; L2_E_STATE before l2_seq_reserve.  With L2_OPT_CHECK_POS set,
 * n_pos greater than the source's next position is L2_E_STATE (those rows were never written).  On success every destination's next
 * position becomes n_pos: feeding it at n_pos is in order, skipping past it is refused.
 * Joined the surface without a version step: a binding detects it by its symbol. */
int l2_seq_fork(l2_ctx* ctx, int src, int n_dst, const int32_t* dsts, int n_pos);

/* Copy a RunState buffer to the host (parity tests).  For per-layer caches `layer` selects the
 * [S][d] slab (-1: all layers).  After a forward, X holds the final-normed x as in llama2.ts:299.
 * X, XB2, HB2, K, V and ATT need L2_OPT_KEEP_STATE (set before the forward), else L2_E_STATE. */
int l2_read_state(l2_ctx* ctx, int which, int layer, float* out, size_t n_floats);

int l2_set_option(l2_ctx* ctx, int key, int value);
int l2_get_option(l2_ctx* ctx, int key, int* value);
/* Why the library's own queue (L2_OPT_AQL_QUEUE) is not in use on this context, or "" when it is / has not been tried yet.  The text
 * lives in the context and is valid until the next call on it (l2_last_error is for failures only and is left alone). */
const char* l2_dispatch_reason(l2_ctx* ctx);

/* Measurement hooks (bench.py): HIP events on the context's own stream. */
int l2_timer_start(l2_ctx* ctx);
int l2_timer_stop(l2_ctx* ctx, float* elapsed_ms);   /* synchronises */
/* Launch only the dominant kernel (the weight-streaming GEMV of one matrix kind of one layer)
 * `iters` times back to back and return the average device time per launch.  Scratch use of the RunState
 * buffers: the activations and cache row `pos` are clobbered, call it outside a decode. */
int l2_bench_gemv(l2_ctx* ctx, int tensor_kind, int layer, int iters, float* avg_ms);
/* The same kernel timed in situ: `steps` greedy decode steps (eager launches) with a HIP start / stop event pair attached
 * to every dispatch of the rmsnorm + w1/w3 + SwiGLU kernel on the library's stream (hipExtLaunchKernelGGL: the events
 * bracket the kernel's execution, as a kernel trace does); mean duration in microseconds. */
int l2_bench_dominant_in_situ(l2_ctx* ctx, int first_token, int pos0, int steps, float* avg_us, int* launches);
/* `steps` forwards (greedy feed, device-resident), timed: total ms from the first submission to completion (the library's own queue: host
 * clock, first doorbell -> completion signal, spinning; hipGraph replays: events on the library's stream). */
int l2_bench_decode(l2_ctx* ctx, int first_token, int pos0, int steps, float* total_ms);
/* The first `n` tokens the last device-resident run (l2_bench_decode, l2_decode_greedy, l2_decode_sample) chose: lets a benchmark
 * check the very run it timed against the reference's tokens (llama2.ts:476-478 picks them on the host). */
int l2_bench_tokens(l2_ctx* ctx, int32_t* tokens_out, int n);

#ifdef __cplusplus
}
#endif
#endif
