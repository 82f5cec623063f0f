// controls.hip.h -- sampling controls of the mixed step (l2_step_batch_sampling; host side: batch_host.hip.h): the three launches that
// make a row's repetition / presence / frequency penalties, its top-k and its min-p hold on the device.
//
// bt_penalise_rows_kernel (stage A) rewrites rows of the [n][V] fp32 logits buffer in place, after the classifier and BEFORE
// bt_constrain_rows_kernel (penalise, then bias, then mask).  For every id j that occurs c_j > 0 times in the row's history:
//   y     = rep == 1 ? x[j] : (x[j] > 0 ? (float)((double)x[j] / rep) : (float)((double)x[j] * rep))
//   x'[j] = presence == 0 && frequency == 0 ? y : (float)((double)y - (presence + frequency * (double)c_j))
// every product, sum and difference rounded on its own (no fused multiply-add); an id that does not occur is never written.  Grid
// (rows), 1024 threads; a row with an empty history or neutral penalties leaves at entry.  COUNT: every history entry adds 1 to its
// id's word of the row's count table ([V] ints, zeroed once when it is allocated).  REWRITE, behind a workgroup barrier: every entry
// swaps its id's word for 0; the one entry that gets the count back (the others get 0) rewrites the logit, so each distinct id is
// rewritten exactly once however often it occurs, and the table is zero again when the launch ends: that, and nothing else, is
// what keeps it zero from call to call.
//
// bt_truncate_rows_kernel (stage B) writes all n rows of a second [n][V] buffer that only the row sampler (and the fall-through
// below) reads: a plain copy of x', or for a sampling row with top-k / min-p
//   x''[j] = x'[j]   fewer than k ids rank before j (descending value, equal values by ascending id: the upper word of argmax_key)
//                    AND (double)s_j - (double)s_max >= log(min_p), s_j = (float)((double)x'[j] / T) (sampler_serial.hip.h:50)
//   x''[j] = -inf    otherwise
// Grid (rows), 1024 threads.  The k-th rank is found exactly by a radix select over the 32-bit order-preserving key: four passes of
// 8 bits, each an LDS histogram of the ids that match the prefix found so far and a block scan from the top bin down; that leaves
// the threshold key, and how many ids of its tie group survive.  When not all of them do, the output pass numbers the group's ids
// in ascending order with a block scan per 1024 columns and a running carry.  s_max is the scaled maximum of the row (x -> x / T is
// monotone for T > 0; NaN entries stand aside); log(min_p) comes from the host.
//
// bt_survivor_pick_kernel runs after bt_pick_kernel when the truncation launch ran.  The reference's sample_topp / sample return 0
// when their loop runs out (llama2.ts:375, :393), and 0 may be a token that top-k or min-p removed: one workgroup per sampling row
// that truncates tests x''[pick] == -inf; if so the row's pick becomes the first maximum of x'' under argmax_key (llama2.ts:364-366),
// written to the token table and out[r][0].  The draw has been made and the rng state stays as the sampler left it.  A row that
// is only masked is never touched here: bt_allowed_pick_kernel keeps testing its mask bit, whatever else the call holds, so a row's
// pick does not depend on the other rows of its call.  (For a row that is masked and truncates both rules give the same token: the
// first maximum of x' survives top-k and min-p, so it is the first maximum of x'' too.)
//
// Device tables of a call (one upload, rows in packing order): [n][4] doubles {repetition, presence, frequency, log(min_p) or -inf
// for off}; [n][4] ints {first history entry, history length (0: nothing to penalise), top_k (0: off), 1 for a sampling row that
// truncates}; the history ids back to back.  The host has checked every id against V and every count before anything is launched.
//
// The kernels are templates over their workgroup size and have ONE instance each, listed at the end of this file the way
// attention_inst.hip.h lists the attention family's: llama2_hip.hip sees explicit instantiation DECLARATIONS (it launches them, it
// does not compile them), attention_inst.hip explicit instantiation DEFINITIONS, behind the attention instances.  So the main code
// object (the GEMMs, the pick and constraint kernels) stays byte for byte what it was, and in the attention family's every earlier
// kernel keeps its place.
#pragma once
#include "kernels.hip.h"

namespace l2k {

enum { SC_THREADS = 1024, SC_HIST_MAX = 65536 };

struct ControlArgs {
  float* logits;             // [rows][V]: x -> x' (penalties), then read
  float* trunc;              // [rows][V]: x''
  const double* pen;         // [rows][4]
  const int* ctl;            // [rows][4]
  const int* hist;           // history ids
  int* count;                // [rows][V], zero between launches (the penalty launch leaves it so)
  const double* params;      // [rows][2]: the row sampler's {temperature, topp}
  int V;
};

struct SurvivorPickArgs {
  const float* trunc;        // [rows][V]: x''
  const int* ctl;            // [rows][4]
  int* tok;                  // [rows] the token table's picks
  int* out;                  // [rows][out_stride]
  int V, out_stride;
};

template <int NT>
__global__ void __launch_bounds__(NT) bt_penalise_rows_kernel(const ControlArgs a) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const int hn = a.ctl[4 * r + 1];
  if (hn == 0) return;
  const int* h = a.hist + a.ctl[4 * r];
  int* cnt = a.count + (size_t)r * a.V;
  for (int i = tid; i < hn; i += NT) atomicAdd(cnt + h[i], 1);
  __threadfence();
  __syncthreads();
  const double rep = a.pen[4 * r], pres = a.pen[4 * r + 1], freq = a.pen[4 * r + 2];
  float* lg = a.logits + (size_t)r * a.V;
  for (int i = tid; i < hn; i += NT) {
    const int j = h[i];
    const int c = atomicExch(cnt + j, 0);
    if (c == 0) continue;                                   // another entry of the same id took the count
    const float x = lg[j];
    float y = x;
    if (rep != 1.0) y = x > 0.0f ? (float)((double)x / rep) : (float)__dmul_rn((double)x, rep);
    if (pres != 0.0 || freq != 0.0) y = (float)__dsub_rn((double)y, __dadd_rn(pres, __dmul_rn(freq, (double)c)));
    lg[j] = y;
  }
}

// The rank key of top-k: the value word of argmax_key (-0 as +0; NaN below -inf, except at index 0 where it is above +inf).
__device__ __forceinline__ unsigned sc_key(float v, int i) { return (unsigned)(argmax_key(v, i) >> 32); }

// Inclusive scan of one int per thread over the workgroup (every thread calls it); *total: the sum.  sw: [NT / 64] of LDS.
template <int NT>
__device__ __forceinline__ int sc_block_scan(int v, int* sw, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) sw[w] = x;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int q = 0; q < NT / 64; ++q) {
    const int t = sw[q];
    base += q < w ? t : 0;
    tot += t;
  }
  __syncthreads();                                          // sw may be written again
  *total = tot;
  return x + base;
}

template <int NT>
__global__ void __launch_bounds__(NT) bt_truncate_rows_kernel(const ControlArgs a) {
  __shared__ int s_hist[256];
  __shared__ int s_w[NT / 64];
  __shared__ unsigned s_mx[NT / 64];
  __shared__ int s_sel[3];
  const int r = blockIdx.x, tid = threadIdx.x, V = a.V;
  const float* x = a.logits + (size_t)r * V;
  float* out = a.trunc + (size_t)r * V;
  const double T = a.params[2 * r], lmp = a.pen[4 * r + 3];
  const int k0 = a.ctl[4 * r + 2];
  const bool by_k = T != 0.0 && k0 > 0 && k0 < V, by_p = T != 0.0 && lmp > -INFINITY;
  if (!by_k && !by_p) {      // a greedy row, or nothing to truncate: the copy
    if ((V & 3) == 0) {      // rows start 16-byte aligned
      const f4* x4 = reinterpret_cast<const f4*>(x);
      f4* o4 = reinterpret_cast<f4*>(out);
      for (int c = tid; c < V / 4; c += NT) o4[c] = x4[c];
    } else {
      for (int i = tid; i < V; i += NT) out[i] = x[i];
    }
    return;
  }

  // ---- top-k: the k-th largest key, and how many ids of its tie group survive
  unsigned thr = 0;
  int krem = 0, ties = 0;
  if (by_k) {
    krem = k0;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      if (tid < 256) s_hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < V; i += NT) {
        const unsigned key = sc_key(x[i], i);
        if (pass == 0 || (key >> ((shift + 8) & 31)) == thr) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
      }
      __syncthreads();
      const int hv = tid < 256 ? s_hist[255 - tid] : 0;     // thread t: bin 255 - t, so the scan runs from the top bin down
      int tot;
      const int incl = sc_block_scan<NT>(hv, s_w, &tot);        // ids in bins >= 255 - t
      if (tid < 256 && incl >= krem && incl - hv < krem) { s_sel[0] = 255 - tid; s_sel[1] = krem - (incl - hv); s_sel[2] = hv; }
      __syncthreads();
      thr = (thr << 8) | (unsigned)s_sel[0];
      krem = s_sel[1];
      ties = s_sel[2];
    }
  }

  // ---- min-p: the scaled maximum
  float smax = -INFINITY;
  if (by_p) {
    unsigned best = 0;                                      // order-preserving key of the maximum; NaN: 0, below -inf
    for (int i = tid; i < V; i += NT) {
      const float v = x[i] + 0.0f;
      const unsigned u = __float_as_uint(v);
      const unsigned o = (v != v) ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
      best = o > best ? o : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned o = (unsigned)__shfl_xor((int)best, off, 64); best = o > best ? o : best; }
    if ((tid & 63) == 0) s_mx[tid >> 6] = best;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NT / 64; ++q) best = s_mx[q] > best ? s_mx[q] : best;
    if (best != 0u) smax = (float)((double)__uint_as_float((best & 0x80000000u) ? (best & 0x7fffffffu) : ~best) / T);
  }

  // ---- the output pass; the tie group's ids are numbered in ascending order only when some of them do not survive
  const bool number = by_k && krem < ties;
  int carry = 0;
  for (int base = 0; base < V; base += NT) {
    const int i = base + tid;
    const bool in = i < V;
    const float v = in ? x[i] : 0.0f;
    bool keep = in;
    int tie = 0;
    if (by_k && in) {
      const unsigned key = sc_key(v, i);
      keep = key >= thr;
      tie = key == thr;
    }
    if (number) {
      int tot;
      const int incl = sc_block_scan<NT>(tie, s_w, &tot);
      if (tie && carry + incl > krem) keep = false;
      carry += tot;
    }
    if (by_p && keep) {
      const float s = (float)((double)v / T);
      keep = (double)s - (double)smax >= lmp;
    }
    if (in) out[i] = keep ? v : -INFINITY;
  }
}

// bt_allowed_pick_kernel's rule with another test in front (constrain.hip.h; that kernel's own text stays as it is, so that its
// instruction stream does): the first maximum of the row under argmax_key, into the token table and out[r][0].
template <int NT>
__global__ void __launch_bounds__(NT) bt_survivor_pick_kernel(const SurvivorPickArgs a) {
  __shared__ unsigned long long sk[NT / 64];
  __shared__ int s_redo;
  const int r = blockIdx.x, tid = threadIdx.x;
  if (a.ctl[4 * r + 3] == 0) return;                        // a greedy row, or one that does not truncate
  const int V = a.V;
  const float* lg = a.trunc + (size_t)r * V;
  if (tid == 0) s_redo = lg[a.tok[r]] == -INFINITY;
  __syncthreads();
  if (!s_redo) return;
  unsigned long long best = 0;
  for (int i = tid; i < V; i += NT) { const unsigned long long k = argmax_key(lg[i], i); best = k > best ? k : best; }
  best = wave_max_u64(best);
  if ((tid & 63) == 0) sk[tid >> 6] = best;
  __syncthreads();
  if (tid < 64) {
    best = wave_max_u64(tid < NT / 64 ? sk[tid] : 0ull);
    if (tid == 0) {
      const int bi = (best == 0) ? 0 : (int)~(unsigned)best;   // nothing but NaN: reduce() keeps index 0
      a.tok[r] = bi;
      a.out[(size_t)r * a.out_stride] = bi;
    }
  }
}

#ifndef L2_CONTROLS_INST
#define L2_CONTROLS_INST extern      // declarations by default
#endif
L2_CONTROLS_INST template __global__ void bt_penalise_rows_kernel<SC_THREADS>(const ControlArgs);
L2_CONTROLS_INST template __global__ void bt_truncate_rows_kernel<SC_THREADS>(const ControlArgs);
L2_CONTROLS_INST template __global__ void bt_survivor_pick_kernel<SC_THREADS>(const SurvivorPickArgs);

}  // namespace l2k
