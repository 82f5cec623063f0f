// constrain.hip.h -- constrained picks of the mixed step (l2_step_batch_constrained; host side: batch_host.hip.h): the two launches
// that make a row's token mask and logit bias hold for everything that reads the row afterwards.
//
// bt_constrain_rows_kernel rewrites rows of the [n][V] fp32 logits buffer in place, after the classifier and before the row sampler,
// the pick and lp_rows_kernel read it:
//   x'[j] = -inf                    the row has a mask and bit j of it is clear
//   x'[j] = (float)(x[j] + bias)    j is allowed and in the row's bias list (one fp32 add)
//   x'[j] = x[j]                    otherwise: never written, so bit for bit
// Grid (column blocks of 1024, rows), 256 threads.  A row with no mask and no bias leaves at entry (block-uniform).  MASK PASS: a thread
// owns 4 consecutive logits, whose 4 bits lie in one mask word (token j: bit j & 31 of word j >> 5; one word serves 8 threads).  The
// pass stores a constant, so it loads no logit: all 4 bits clear and V % 4 == 0 (every row then starts 16-byte aligned) is one
// 16-byte store; a mixed group, or any group when V % 4 != 0 (row bases are V * 4 bytes apart), stores 4 bytes per clear bit, and an
// allowed element is not written at all.  Bits at or above V are never looked at.  BIAS PASS, same launch: the row's column block 0
// walks the row's list (<= 256 entries: one per thread; ids distinct within a row, checked by the host) and writes x + b where the id
// is allowed.  The two passes write disjoint elements -- clear bits here, set bits there -- so nothing orders them.
//
// bt_allowed_pick_kernel runs after bt_pick_kernel when some row both samples and has a mask.  The reference's sample_topp / sample
// return 0 when their loop runs out (llama2.ts:375, :393), and 0 may be a token the mask forbids: one workgroup per row tests the
// bit of the pick in the token table; if it is clear the row's pick becomes the first maximum of the (constrained) row under
// argmax_key (llama2.ts:364-366) -- always an allowed token, the others being -inf -- written to the token table and out[r][0], where
// lp_rows_kernel and the copy-back read it.  The draw has been made and the rng state stays as the sampler left it.
//
// Device tables of a call (uint32 words, one upload): [n] mask index of every row in packing order (-1: none), [n] offset of its bias
// list, [n] its length; [n_masks][W] the masks, W = ceil(V / 32); [nb] bias ids; [nb] bias values (float bits).
#pragma once
#include "kernels.hip.h"

namespace l2k {

enum { CS_COLS = 1024, CS_THREADS = 256, CS_BIAS_MAX = 256 };
static_assert(CS_COLS == 4 * CS_THREADS, "a thread owns 4 consecutive logits");
static_assert(CS_BIAS_MAX <= CS_THREADS, "column block 0 walks a row's bias list one entry per thread");

struct ConstrainArgs {
  float* logits;             // [rows][V]
  const int* mask_of;        // [rows] mask index, -1: none
  const int* bias_off;       // [rows] first entry of the row's bias list
  const int* bias_n;         // [rows] its length (0 .. CS_BIAS_MAX)
  const unsigned* masks;     // [n_masks][W]
  const int* bias_ids;
  const float* bias_vals;
  int V, W;
};

__global__ void __launch_bounds__(CS_THREADS) bt_constrain_rows_kernel(const ConstrainArgs a) {
  const int r = blockIdx.y, tid = threadIdx.x;
  const int m = a.mask_of[r];
  const int nb = blockIdx.x == 0 ? a.bias_n[r] : 0;
  if (m < 0 && nb == 0) return;
  const int V = a.V;
  float* lg = a.logits + (size_t)r * V;
  const unsigned* mw = a.masks + (size_t)(m < 0 ? 0 : m) * a.W;
  if (m >= 0) {
    const int c = blockIdx.x * CS_COLS + 4 * tid;
    if (c < V) {
      const unsigned nib = (mw[c >> 5] >> (c & 31)) & 0xfu;
      if ((V & 3) == 0 && nib == 0u) {
        *reinterpret_cast<f4*>(lg + c) = f4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c + e < V && !((nib >> e) & 1u)) lg[c + e] = -INFINITY;
      }
    }
  }
  if (tid < nb) {
    const int k = a.bias_off[r] + tid, id = a.bias_ids[k];
    if (m < 0 || ((mw[id >> 5] >> (id & 31)) & 1u)) lg[id] = lg[id] + a.bias_vals[k];
  }
}

struct AllowedPickArgs {
  const float* logits;       // [rows][V], constrained
  const double* params;      // [rows][2]: the row sampler's {temperature, topp}
  const int* mask_of;        // [rows]
  const unsigned* masks;     // [n_masks][W]
  int* tok;                  // [rows] the token table's picks
  int* out;                  // [rows][out_stride]
  int V, W, out_stride;
};

__global__ void __launch_bounds__(1024) bt_allowed_pick_kernel(const AllowedPickArgs a) {
  __shared__ unsigned long long sk[16];
  __shared__ int s_redo;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int m = a.mask_of[r];
  if (m < 0 || a.params[2 * r] == 0.0) return;             // no mask, or a greedy row: its argmax is an allowed token
  if (tid == 0) {
    const int t = a.tok[r];
    s_redo = !((a.masks[(size_t)m * a.W + (t >> 5)] >> (t & 31)) & 1u);
  }
  __syncthreads();
  if (!s_redo) return;
  const int V = a.V;
  const float* lg = a.logits + (size_t)r * V;
  unsigned long long best = 0;
  if ((V & 3) == 0) {   // rows start 16-byte aligned
    const f4* l4 = reinterpret_cast<const f4*>(lg);
    for (int c = tid; c < V / 4; c += 1024) {
      const f4 v = l4[c];
      unsigned long long k = argmax_key(v.x, 4 * c); best = k > best ? k : best;
      k = argmax_key(v.y, 4 * c + 1); best = k > best ? k : best;
      k = argmax_key(v.z, 4 * c + 2); best = k > best ? k : best;
      k = argmax_key(v.w, 4 * c + 3); best = k > best ? k : best;
    }
  } else {
    for (int i = tid; i < V; i += 1024) { const unsigned long long k = argmax_key(lg[i], i); best = k > best ? k : best; }
  }
  best = wave_max_u64(best);
  if ((tid & 63) == 0) sk[tid >> 6] = best;
  __syncthreads();
  if (tid < 64) {
    best = wave_max_u64(tid < 16 ? sk[tid] : 0ull);
    if (tid == 0) {
      const int bi = (best == 0) ? 0 : (int)~(unsigned)best;   // nothing but NaN: reduce() keeps index 0
      a.tok[r] = bi;
      a.out[(size_t)r * a.out_stride] = bi;
    }
  }
}

}  // namespace l2k
