// Device-side temperature / top-p sampling (llama2.ts:348-394 and 476-493): the part of the
// reference's decode loop that sits between transformer() and the next token, kept on the GPU so that a sampled
// run needs no 128 KB logits hand-off and no host sort of 32 000 objects per token.  sampler.hip holds the
// kernels; this is the interface llama2_hip.hip uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace l2s {

enum { MAX_VOCAB = 256 * 1024 };   // one chain thread per 1024-element tile

// The buffers of the default ("margin") form for `rows` rows of a V-entry vocabulary: every phase is launched ONCE per step for rows
// 0 .. n-1, the row on a spare grid dimension, every per-row buffer at a row stride.  Row r reads logits + r V and its settings
// params[2 r] = {temperature, topp}, draws from rng[r] and counts into stats[2 r ..].  A row whose mode a phase does not serve
// (temperature 0: argmax, not the sampler's; plain sample; sample_topp with 0 < topp < 1) leaves that phase at entry, so one recording
// serves any mix of settings.  A single sequence (l2_decode_sample: Sampler below) is one row; the batched decode (batch_host.hip.h)
// holds one row per reserved sequence.  L2_SAMPLER_FORCE_SERIAL (behind L2_TEST_HOOKS) is the margin form's own branch and honoured here.
struct RowSampler {
  int V = 0, G = 0, rows = 0;    // G: tiles of 1024 elements
  size_t P = 0;                  // row stride of the per-element buffers (V padded to whole sort tiles)
  size_t R = 0;                  // row stride of the run records (G * 1025)
  float* probs = nullptr;        // (rows x P) exps of the scaled logits (the serial A/B form: -> probabilities, in place like state.logits)
  float* run_p = nullptr;        // (rows x P) sorted tiles (top-p)
  int* idx = nullptr;            // (rows x P) their ids
  float* sorted = nullptr;       // (rows x P) probabilities in descending order
  int* ids = nullptr;            // (rows x P) token ids beside them, ties by id (stable sort)
  unsigned* rank_acc = nullptr;  // (rows x P) the rank merge's per-element accumulators {groups reported : 8, elements in front : 24}, zero between tokens
  double* part = nullptr;        // (rows x G) tile sums of the exps
  double* part2 = nullptr;       // (rows x G) tile sums of the probabilities
  double* amb = nullptr;         // (rows x G) float spacings of the ambiguous quotients
  double* part_sorted = nullptr; // (rows x G) tile sums of the sorted order (accumulated by the rank merge), zero between tokens
  void* recs = nullptr;          // (rows x R) xs::Run records of the exps' running sum (top-p)
  int* cnt = nullptr;            // (rows x G) records per tile
  double* runS = nullptr;        // (rows x R) per run state when the runs do not fit in LDS: exact running sum after it
  int* runEnd = nullptr;
  int* runBad = nullptr;
  double* total = nullptr;       // (rows) exact total of the exps (top-p: runs_total_rows_kernel -> the tile sort)
  unsigned* mxkey = nullptr;     // (rows) max of the scaled logits (order-preserving key), zero between tokens
  unsigned* ticket = nullptr;    // (rows) arrivals of a launch, zero between tokens
  double* params = nullptr;      // (rows x 2) {temperature, topp}
  unsigned long long* rng = nullptr;     // (rows) xorshift* states (the reference's BigInt rng_seed)
  unsigned long long* stats = nullptr;   // (rows x 2) {tokens picked, of those by the serial loop}
  int* pick = nullptr;           // (rows x 4) the batch rows' picks: advance()'s record {token, count, step, token}; bt_pick_kernel reads
                                 // the token and puts step back to 0
  double* h_params = nullptr;    // pinned staging of params / rng / stats
  unsigned long long* h_rng = nullptr;
  unsigned long long* h_stats = nullptr;
  bool force_serial = false;     // L2_SAMPLER_FORCE_SERIAL=1: every token treated as undecided
};
// Buffers for `rows` rows of a V-entry vocabulary (V <= MAX_VOCAB); on failure nothing is held.
hipError_t create_rows(RowSampler* s, int V, int rows);
void destroy_rows(RowSampler* s);
// The scratch that must be zero between tokens (a call that ended early may have left it otherwise) and the per-row counters.
hipError_t reset_rows(const RowSampler& s, int n, hipStream_t st);

// Where the picks go.  tokens_out given (one row): the token is stored in tokens_out[step] and {token, pos, step} advanced in tokpos --
// the same protocol as argmax_advance_kernel.  tokens_out null: tokpos is the rows' pick records (RowSampler::pick).  `amax` (may be
// null; one row only): the 8 argmax keys the classifier folded max(logits) into (one per 128-byte line); usable only for
// temperature > 0; they replace the sampler's own maximum pass, and the sampler zeroes them for the next token.
struct Pick { int* tokpos; int* tokens_out; unsigned long long* amax; };
enum { PICK_SAMPLE = 1, PICK_TOPP = 2, PICK_BOTH = 3 };
// Enqueue the margin form's phases of one step for rows 0 .. n-1 after the classifier (logits: n rows of V floats, left untouched): the
// maximum pass unless out.amax supplies it, the exps, and the launches of the pickers named in `picks` -- plain sample 1 launch, top-p 4.
// Every row's token is what llama2.ts:480-493 picks from its settings and rng state.
hipError_t enqueue_rows(const RowSampler& s, const float* logits, int n, int picks, const Pick& out, hipStream_t st);

// The single sequence of l2_decode_sample: one row, and the A/B forms behind L2_TEST_HOOKS (not carried into batches) with the scratch
// the exact-chain form and the diagnostic hold beside it.
struct Sampler : RowSampler {
  bool chain = false;            // L2_SAMPLER_CHAIN=1: every running sum exact on the whole chip (round 2-3 default), kept for A/B
  bool serial = false;           // L2_SAMPLER_SERIAL=1: one lane accumulates (the straightforward form, kept for A/B)
  float* probs_n = nullptr;      // (P) probabilities
  void* recs2 = nullptr;         // (R) run records of the probabilities (in index or sorted order)
  int* cnt2 = nullptr;           // (G)
  int* off = nullptr;            // (G + 1) first run of every tile
  unsigned long long* cq = nullptr;   // (P) per element: grid composite since the start of its run
  int* cm = nullptr;
};

// Launch recorder: while one is set (thread-local), every launch of the sampler is handed to it -- host function, geometry, dynamic LDS,
// the explicit arguments packed as the kernel-argument segment lays them out -- instead of to HIP: the library's own AQL queue
// records the sampled step that way (aql_queue.h).  Returns false when the launch could not be recorded.
typedef bool (*LaunchRecorder)(void* user, const void* host_fn, dim3 grid, dim3 block, size_t lds, hipStream_t st, const void* args, size_t arg_bytes);
void set_recorder(LaunchRecorder r, void* user);
bool recorder_failed();      // since the last set_recorder

hipError_t create(Sampler* s, int V);
void destroy(Sampler* s);
// One sampled step of the single sequence: enqueue_rows at one row with the picker of the mode -- `topp_mode`: the sample_topp branch
// (0 < topp < 1, as s.params says on the device) -- or the A/B form the hooks chose.
hipError_t enqueue(const Sampler& s, const float* logits, bool topp_mode, int* tokpos, int* tokens_out, unsigned long long* amax, hipStream_t st);

// {tokens the margin form picked, of those by its serial loop} since create(); synchronous.
hipError_t read_stats(const Sampler& s, unsigned long long out[2], hipStream_t st);

// Diagnostic: running sums S_i = fl(S_{i-1} + x_i) of n <= MAX_VOCAB non-negative fp32 values, by the exact parallel
// algorithm (synchronous).
hipError_t running_sums(const float* x_dev, int n, double* prefix_dev, hipStream_t st);

}  // namespace l2s
