// Device-side sampling for libllama2hip.so (gfx950): temperature scaling, softmax, sample / sample_topp and the
// xorshift* RNG of wizzard0/llama2.ts (llama2.ts:348-394, 476-493), restated so that the SAME token comes out.
//
// What makes that non-trivial: the reference's sums are sequential fp64 accumulations of fp32 values
// (softmax :189, sample :369/:373, sample_topp :385/:391) and the chosen index depends on comparing a random
// threshold against those running sums, so a tree sum (different in the last bits) can flip a token.
//
// Default form (sampler_margin.hip.h; +11 us per token for sample, +39 us for top-p at stories110M): the function returns an INDEX, so the
// running sums only have to be known well enough to decide every comparison the loop makes.  Tree sums over the whole chip plus a proven
// margin (margin_rule.h: n 2^-53 per summation order, the float spacing of every probability a tree total could round differently) decide
// it; a token whose running sum comes within the margin of its threshold (a few in a million) is picked by the reference's loop run as
// written by one lane of the same workgroup.  Launches: sample 2 (exps + tile sums -> probabilities' tile sums, the last workgroup picks);
// top-p 5 (exps; runs of the exps + their exact total by the last workgroup; probabilities + tile sort; rank merge; pick) -- the descending
// order of sample_topp needs the exact probabilities, hence the exact total there; one more launch in front (the maximum) where the
// classifier's argmax keys do not supply it.  One kernel per phase (*_rows_kernel), launched for rows 0 .. n-1 with the row on a spare grid
// dimension: l2_decode_sample is n = 1 with the launches of its mode, the batched decode launches every phase for all its rows
// (enqueue_rows, the one place that launches them; sampler.h: RowSampler).
// Exact-chain form (L2_SAMPLER_CHAIN=1 behind L2_TEST_HOOKS; the default of rounds 2-3; 4 launches for sample, 6 for top-p; +31 / +59 us):
//   exp + tile sums (the maximum comes from the classifier's argmax keys; the margin form's kernels at one row, as is the rank merge) -> runs of the exps
//   sample:  [exact total -> probabilities -> their runs] -> chain: exact running sums, threshold, search, advance
//   top-p:   [exact total -> probabilities -> sorted tiles] -> rank merge (+ tile sums) -> runs -> chain
// "runs" / "chain" are exact_sum.h: every 1024-element tile turns its elements into integer increments on the grid its
// approximate prefix predicts, one wave walks the ~50 runs of a 32 000-element vector with exact fp64 state (stretches of
// runs on one grid composed by a scan first), every prediction is checked, and the searched index is evaluated inside
// the one run that contains it.  The bracketed steps share a launch: each of their workgroups repeats the walk for the
// total instead of waiting for a launch that would hand it over.  Bit-identical to the serial loop by construction
// (tests/test_exact_sum_cpu.py on the host, l2_debug_running_sums on the GPU).  The default form keeps its first half for top-p.
// The descending stable sort of sample_topp (Array.prototype.sort is stable in V8 >= 7.0) is a bitonic sort of
// (probability, id) keys per 1024-element tile followed by one rank-by-binary-search merge of the sorted tiles out of LDS.
//
// L2_SAMPLER_SERIAL=1 keeps the straightforward form for A/B: ONE lane adds in index order (~10 cycles per element,
// ~130 us per pass over 32 000 values) inside a single 1024-thread workgroup (top-p: behind the same tile sort + rank merge).
#include "sampler.h"
#include <string.h>
#include "exact_sum.h"
#include "margin_rule.h"

#include <stdlib.h>
#include <vector>

namespace l2s {

static thread_local LaunchRecorder g_rec = nullptr;
static thread_local void* g_rec_user = nullptr;
static thread_local bool g_rec_failed = false;
void set_recorder(LaunchRecorder r, void* user) { g_rec = r; g_rec_user = user; g_rec_failed = false; }
bool recorder_failed() { return g_rec_failed; }

template <class T>
static void pack_arg(char* buf, size_t& off, const T& v) {
  off = (off + alignof(T) - 1) & ~(alignof(T) - 1);
  memcpy(buf + off, &v, sizeof(T));
  off += sizeof(T);
}
// every launch of the sampled step: HIP, or the recorder (sampler.h)
template <class... KA, class... A>
static void s_launch(void (*kernel)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... a) {
  static_assert(sizeof...(KA) == sizeof...(A), "argument count");
  if (g_rec) {
    char buf[1024];
    size_t off = 0;
    static_assert((sizeof(KA) + ... + 0) + 8 * sizeof...(KA) <= sizeof(buf), "kernel arguments exceed the packing buffer");
    (pack_arg<KA>(buf, off, static_cast<KA>(a)), ...);
    if (!g_rec(g_rec_user, reinterpret_cast<const void*>(kernel), grid, block, lds, st, buf, off)) g_rec_failed = true;
    return;
  }
  hipLaunchKernelGGL(kernel, grid, block, lds, st, a...);
}

#pragma clang fp contract(off)

constexpr int NT = 1024;     // threads of the one workgroup of the serial form
constexpr int CH = 4096;     // values staged in LDS per chunk, widened to fp64 (32 KB)
constexpr int SEG = 512;     // spacing of recorded running sums
constexpr int MAXSEG = MAX_VOCAB / SEG;

__device__ __forceinline__ float random_f32(unsigned long long* rng) {   // llama2.ts:349-360
  unsigned long long s = *rng;
  s ^= s >> 12;
  s ^= s << 25;
  s ^= s >> 27;
  *rng = s;
  const unsigned u = (unsigned)((s * 0x2545F4914F6CDD1Dull) >> 32);
  return (float)(((double)u / 256.0) / 16777216.0);      // one rounding at the Float32Array store (:358)
}

__device__ __forceinline__ void advance(int* tokpos, int* tokens_out, int next) {
  const int step = tokpos[2];
  tokens_out[step] = next;
  tokpos[0] = next; tokpos[1] = tokpos[1] + 1; tokpos[2] = step + 1;
}

// Which picker a batch row runs (llama2.ts:477-487): 0 argmax (temperature 0), 1 sample, 2 sample_topp (0 < topp < 1).
__device__ __forceinline__ int row_mode(const double* params) {
  const double t = params[0], p = params[1];
  return t == 0.0 ? 0 : (p <= 0.0 || p >= 1.0) ? 1 : 2;
}

#include "sampler_serial.hip.h"
#include "sampler_chain.hip.h"
#include "sampler_sort.hip.h"
#include "sampler_margin.hip.h"

// Stage 1 = the exps (recs / cnt), stage 2 = the probabilities, in index or in sorted order (recs2 / cnt2, cq / cm): two
// sets of run records because the fused kernels write stage 2 while other workgroups still read stage 1.
static ChainArgs chain_args(const Sampler& s, const float* x, const double* part, bool stage2) {
  ChainArgs a = {};
  a.x = x; a.V = s.V; a.G = s.G; a.part = part;
  a.recs = (const Run*)(stage2 ? s.recs2 : s.recs); a.cnt = stage2 ? s.cnt2 : s.cnt;
  a.off = s.off; a.S = s.runS; a.End = s.runEnd; a.Bad = s.runBad; a.cq = s.cq; a.cm = s.cm;
  a.params = s.params; a.rng = s.rng; a.mxkey = s.mxkey;
  return a;
}

static hipError_t launch_chain(const ChainArgs& a, int mode, hipStream_t st) {
  if (mode == CHAIN_SAMPLE) s_launch(chain_kernel<CHAIN_SAMPLE>, dim3(1), dim3(TN), 0, st, a);
  else if (mode == CHAIN_TOPP) s_launch(chain_kernel<CHAIN_TOPP>, dim3(1), dim3(TN), 0, st, a);
  else s_launch(chain_kernel<CHAIN_DEBUG>, dim3(1), dim3(TN), 0, st, a);
  return hipGetLastError();
}

// ---- buffers: one table per struct drives both allocation and release --------------------------------------------------------------
struct Buf { void** p; size_t bytes; bool zero, pinned; };
template <class T>
static Buf buf(T** p, size_t bytes, bool zero = false, bool pinned = false) { return {reinterpret_cast<void**>(p), bytes, zero, pinned}; }

static std::vector<Buf> row_bufs(RowSampler* s) {
  const size_t n = (size_t)s->rows, P = s->P, R = s->R, G = (size_t)s->G;
  return {buf(&s->probs, n * P * 4), buf(&s->run_p, n * P * 4), buf(&s->idx, n * P * 4), buf(&s->sorted, n * P * 4), buf(&s->ids, n * P * 4),
          buf(&s->rank_acc, n * P * sizeof(unsigned), true), buf(&s->part, n * G * sizeof(double)), buf(&s->part2, n * G * sizeof(double)),
          buf(&s->amb, n * G * sizeof(double)), buf(&s->part_sorted, n * G * sizeof(double), true), buf(&s->recs, n * R * sizeof(Run)),
          buf(&s->cnt, n * G * sizeof(int)), buf(&s->runS, n * R * sizeof(double)), buf(&s->runEnd, n * R * sizeof(int)),
          buf(&s->runBad, n * R * sizeof(int)), buf(&s->total, n * sizeof(double)), buf(&s->mxkey, n * sizeof(unsigned), true),
          buf(&s->ticket, n * sizeof(unsigned), true), buf(&s->params, 2 * n * sizeof(double)), buf(&s->rng, n * sizeof(unsigned long long)),
          buf(&s->stats, 2 * n * sizeof(unsigned long long), true), buf(&s->pick, 4 * n * sizeof(int), true),
          buf(&s->h_params, 2 * n * sizeof(double), false, true), buf(&s->h_rng, n * sizeof(unsigned long long), false, true),
          buf(&s->h_stats, 2 * n * sizeof(unsigned long long), false, true)};
}
// what the exact-chain form and the diagnostic hold beside one row: the probabilities, stage 2's run records, the per-element composites
static std::vector<Buf> chain_bufs(Sampler* s) {
  const size_t P = s->P, R = s->R, G = (size_t)s->G;
  return {buf(&s->probs_n, P * 4), buf(&s->recs2, R * sizeof(Run)), buf(&s->cnt2, G * sizeof(int)), buf(&s->off, (G + 1) * sizeof(int)),
          buf(&s->cq, P * sizeof(unsigned long long)), buf(&s->cm, P * sizeof(int))};
}

static void release(const std::vector<Buf>& bufs) {
  for (const Buf& b : bufs) if (*b.p) { (void)(b.pinned ? hipHostFree(*b.p) : hipFree(*b.p)); *b.p = nullptr; }
}
static hipError_t allocate(const std::vector<Buf>& bufs) {       // on failure nothing of the table is held
  for (const Buf& b : bufs) {
    hipError_t e = b.pinned ? hipHostMalloc(b.p, b.bytes, 0) : hipMalloc(b.p, b.bytes);
    if (e == hipSuccess && b.zero) e = hipMemset(*b.p, 0, b.bytes);
    if (e != hipSuccess) { release(bufs); return e; }
  }
  return hipSuccess;
}

static bool test_hook(const char* name) {                        // A/B forms and forced branches: development gate
  const char* g = getenv("L2_TEST_HOOKS");
  const char* v = getenv(name);
  return g && atoi(g) != 0 && v && atoi(v) != 0;
}

hipError_t create_rows(RowSampler* s, int V, int rows) {
  if (V <= 0 || V > MAX_VOCAB || rows <= 0) return hipErrorInvalidValue;
  s->V = V; s->rows = rows;
  s->G = (V + TILE - 1) / TILE;
  s->P = (size_t)((V + STILE - 1) / STILE) * STILE;
  s->R = (size_t)s->G * (TILE + 1);
  s->force_serial = test_hook("L2_SAMPLER_FORCE_SERIAL");
  const hipError_t e = allocate(row_bufs(s));
  if (e != hipSuccess) *s = RowSampler();
  return e;
}

void destroy_rows(RowSampler* s) {
  release(row_bufs(s));
  *s = RowSampler();
}

static hipError_t create(Sampler* s, int V, bool chain_scratch) {
  hipError_t e = create_rows(s, V, 1);
  if (e != hipSuccess) return e;
  s->serial = test_hook("L2_SAMPLER_SERIAL"); s->chain = test_hook("L2_SAMPLER_CHAIN");
  if ((s->chain || chain_scratch) && (e = allocate(chain_bufs(s))) != hipSuccess) destroy(s);
  return e;
}
hipError_t create(Sampler* s, int V) { return create(s, V, false); }

void destroy(Sampler* s) {
  release(chain_bufs(s));
  destroy_rows(s);
  *s = Sampler();
}

hipError_t reset_rows(const RowSampler& s, int n, hipStream_t st) {
  hipError_t e;
  if ((e = hipMemsetAsync(s.rank_acc, 0, (size_t)n * s.P * sizeof(unsigned), st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(s.part_sorted, 0, (size_t)n * s.G * sizeof(double), st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(s.mxkey, 0, (size_t)n * sizeof(unsigned), st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(s.ticket, 0, (size_t)n * sizeof(unsigned), st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(s.pick, 0, (size_t)4 * n * sizeof(int), st)) != hipSuccess) return e;
  return hipMemsetAsync(s.stats, 0, (size_t)2 * n * sizeof(unsigned long long), st);
}

hipError_t read_stats(const Sampler& s, unsigned long long out[2], hipStream_t st) {
  if (!s.stats) return hipErrorInvalidValue;
  hipError_t e = hipMemcpyAsync(out, s.stats, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
  return e == hipSuccess ? hipStreamSynchronize(st) : e;
}

hipError_t running_sums(const float* x_dev, int n, double* prefix_dev, hipStream_t st) {
  Sampler s;
  hipError_t e = create(&s, n, true);
  if (e != hipSuccess) return e;
  s_launch(tile_sums_kernel, dim3(s.G), dim3(TN), 0, st, x_dev, n, s.part);
  s_launch(runs_kernel<false>, dim3(s.G), dim3(TN), 0, st, x_dev, n, s.part, (Run*)s.recs, s.cnt, s.cq, s.cm);
  e = launch_chain(chain_args(s, x_dev, s.part, false), CHAIN_DEBUG, st);
  if (e == hipSuccess) {
    s_launch(prefix_kernel, dim3(s.G), dim3(TN), 0, st, x_dev, n, s.part, s.off, s.runS, s.runBad, s.runEnd, prefix_dev);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  destroy(&s);
  return e;
}

// ---- the margin form's launches, n rows at a time --------------------------------------------------------------------------------
static void launch_max(const RowSampler& s, const float* logits, int n, hipStream_t st) {
  s_launch(scaled_max_rows_kernel, dim3(s.G, n), dim3(TN), 0, st, logits, s.V, s.params, s.mxkey);
}
static void launch_exps(const RowSampler& s, const float* logits, int n, const unsigned long long* amax, hipStream_t st) {
  s_launch(exp_rows_kernel, dim3(s.G, n), dim3(TN), 0, st, logits, s.V, s.params, s.mxkey, amax, s.probs, s.part, s.P, s.G);
}
// Descending stable order of every top-p row's sorted tiles (run_p / idx): the rank merge writes sorted / ids and adds every value to the
// sum of the 1024-element tile it lands in (part_sorted).
static void launch_rank_merge(const RowSampler& s, int n, hipStream_t st) {
  const int gs = (int)(s.P / STILE), ne = gs * STILE;
  s_launch(sort_rank_rows_kernel, dim3((ne + RT - 1) / RT, (gs + RANK_TQ - 1) / RANK_TQ, n), dim3(RT), 0, st, s.run_p, s.idx, gs, s.G, s.rank_acc,
           s.sorted, s.ids, s.part_sorted, s.P, s.params);
}

hipError_t enqueue_rows(const RowSampler& s, const float* logits, int n, int picks, const Pick& out, hipStream_t st) {
  if (n < 1 || n > s.rows) return hipErrorInvalidValue;
  if (!out.amax) launch_max(s, logits, n, st);
  launch_exps(s, logits, n, out.amax, st);
  MarginArgs m = {};
  m.exps = s.probs; m.part = s.part; m.V = s.V; m.G = s.G; m.part2 = s.part2; m.amb = s.amb; m.ticket = s.ticket;
  m.sorted = s.sorted; m.ids = s.ids; m.part_sorted = s.part_sorted; m.params = s.params; m.rng = s.rng;
  m.tokpos = out.tokpos; m.tokens_out = out.tokens_out; m.mxkey = s.mxkey; m.amax = out.amax; m.stats = s.stats; m.force_serial = s.force_serial ? 1 : 0;
  if (picks & PICK_SAMPLE) s_launch(sample_margin_rows_kernel, dim3(s.G, n), dim3(TN), 0, st, m, s.P);
  if (picks & PICK_TOPP) {
    // the descending order needs the exact probabilities: runs of the exps + their exact total, [probabilities -> sorted tiles], rank merge
    ChainArgs c = {};
    c.x = s.probs; c.V = s.V; c.G = s.G; c.part = s.part; c.recs = (const Run*)s.recs; c.cnt = s.cnt;
    c.S = s.runS; c.End = s.runEnd; c.Bad = s.runBad; c.params = s.params; c.rng = s.rng; c.mxkey = s.mxkey;
    s_launch(runs_total_rows_kernel, dim3(s.G, n), dim3(TN), 0, st, c, s.P, s.R, s.params, (Run*)s.recs, s.cnt, s.ticket, s.total);
    s_launch(sort_tile_wide_rows_kernel, dim3((unsigned)(s.P / STILE), n), dim3(WT), 0, st, s.probs, s.total, s.V, s.run_p, s.idx, s.P, s.params);
    launch_rank_merge(s, n, st);
    s_launch(topp_margin_rows_kernel, dim3(1, n), dim3(TN), 0, st, m, s.P);
  }
  return hipGetLastError();
}

// The A/B forms (one row): the straightforward one, and the exact chain behind the margin form's max, exps and rank merge.
static hipError_t enqueue_ab(const Sampler& s, const float* logits, bool topp_mode, const Pick& out, hipStream_t st) {
  const int gs = (int)(s.P / STILE);
  if (s.serial) {
    if (!topp_mode) {
      s_launch(sample_kernel, dim3(1), dim3(NT), 0, st, logits, s.V, s.params, s.probs, s.rng, out.tokpos, out.tokens_out);
      return hipGetLastError();
    }
    s_launch(softmax_kernel, dim3(1), dim3(NT), 0, st, logits, s.V, s.params, s.probs, (int*)nullptr);
    s_launch(sort_tile_kernel<false>, dim3(gs), dim3(TN), 0, st, ChainArgs(), s.probs, s.V, s.run_p, s.idx);
    launch_rank_merge(s, 1, st);
    s_launch(topp_kernel, dim3(1), dim3(NT), 0, st, s.sorted, s.ids, s.V, s.params, s.rng, out.tokpos, out.tokens_out);
    return hipGetLastError();
  }
  // temperature + exp (:481-483, :183-188), runs of the exps' running sum
  if (!out.amax) launch_max(s, logits, 1, st);
  launch_exps(s, logits, 1, out.amax, st);
  s_launch(runs_kernel<false>, dim3(s.G), dim3(TN), 0, st, s.probs, s.V, s.part, (Run*)s.recs, s.cnt, s.cq, s.cm);
  const ChainArgs exps = chain_args(s, s.probs, s.part, false);
  ChainArgs pick;
  if (!topp_mode) {
    // exact total -> probabilities -> their runs, in one launch; then sample (:368-376)
    s_launch(normalise_runs_kernel, dim3(s.G), dim3(TN), 0, st, exps, s.probs_n, (Run*)s.recs2, s.cnt2, s.cq, s.cm);
    pick = chain_args(s, s.probs_n, s.part, true);
  } else {
    // sample_topp (:378-394): exact total -> probabilities -> sorted tiles in one launch, rank merge, runs of the sorted order
    s_launch(sort_tile_kernel<true>, dim3(gs), dim3(TN), 0, st, exps, s.probs, s.V, s.run_p, s.idx);
    launch_rank_merge(s, 1, st);
    s_launch(runs_kernel<true>, dim3(s.G), dim3(TN), 0, st, s.sorted, s.V, s.part_sorted, (Run*)s.recs2, s.cnt2, s.cq, s.cm);
    pick = chain_args(s, s.sorted, s.part_sorted, true);
    pick.part_sorted = s.part_sorted;
    pick.ids = s.ids;
  }
  hipError_t e;
  if ((e = hipGetLastError()) != hipSuccess) return e;
  pick.tokpos = out.tokpos; pick.tokens_out = out.tokens_out; pick.amax = out.amax;
  return launch_chain(pick, topp_mode ? CHAIN_TOPP : CHAIN_SAMPLE, st);
}

hipError_t enqueue(const Sampler& s, const float* logits, bool topp_mode, int* tokpos, int* tokens_out, unsigned long long* amax, hipStream_t st) {
  const Pick out = {tokpos, tokens_out, amax};
  if (s.serial || s.chain) return enqueue_ab(s, logits, topp_mode, out, st);
  return enqueue_rows(s, logits, 1, topp_mode ? PICK_TOPP : PICK_SAMPLE, out, st);
}

}  // namespace l2s
