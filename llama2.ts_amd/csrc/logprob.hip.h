// logprob.hip.h -- log-probabilities of the rows of a [rows][V] fp32 logits buffer (l2_seq_score_batch, l2_step_batch_logprobs; host
// side: batch_host.hip.h).
//
// One workgroup of 1024 threads per row, any V: 16-byte loads when V % 4 == 0 (every row then starts 16-byte aligned), scalar loads
// otherwise, as bt_argmax_body.inc reads a row.  For row r it writes
//   amax[r]    the first maximum under argmax_key (kernels.hip.h: llama2.ts:364-366, its rules for ties, +-0, +-inf and NaN) -- the
//              index bt_argmax_kernel picks from the same row;
//   lp[r]      (double)x_t - lse for the row's target t = target[r] (-1: NaN), where lse = m + log(sum_j exp((double)x_j - m)) and
//              m = max_j x_j, all in fp64.  The sum has ONE order -- per-thread strided partials, the DPP wave sum, then the 16 waves
//              in order -- so a row's results depend on its own logits and V only, never on its neighbours or the row count;
//   top_ids / top_lp [r * k ..]  for 0 < k <= LP_TOPK_MAX: the k largest argmax_keys in descending order (equal logits in ascending
//              index order; entry 0 is amax[r]) and their lps.  Pass 1 keeps each thread's largest key; the k-th largest of a wave's
//              64 lane maxima is k distinct keys of the row, so no key below it can be among the row's k largest.  Pass 2 (the one
//              that sums) inserts only keys at or above that threshold into the thread's KL-key list in registers (a compare-exchange
//              chain with constant indices) -- a handful per wave instead of ~20 per thread (V = 32 000: the unguarded chain took
//              68 us for 16 rows).  Then, with no barrier between rounds, every wave takes its own k largest out of its lanes' lists by
//              k rounds of wave_max_u64, and wave 0 takes the workgroup's k largest out of the 16 waves'.  Nothing is sorted.
// NON-FINITE ROWS.  A row holding a NaN or +inf logit, or none above -inf, has no distribution: every lp of it (target and top-k) is
// NaN, while amax and the top ids still follow the key order (NaN at index 0 first, any other NaN below -inf).  In a row without
// them, a -inf logit has lp -inf (exp(-inf) adds 0 to the sum).
#pragma once
#include "kernels.hip.h"

namespace l2k {

enum { LP_TOPK_MAX = 20 };

struct LpRowsArgs {
  const float* logits;     // [rows][V]
  const int* target;       // [rows]: the token whose lp is asked for, or -1
  double* lp;              // [rows]
  int* amax;               // [rows]
  int* top_ids;            // [rows][k]
  double* top_lp;          // [rows][k]
  int V, k;                // k <= KL
};

// KL: the per-thread list length -- 1 when no top-k is asked for (round 0 is the argmax), else LP_TOPK_MAX.
template <int KL>
__global__ void __launch_bounds__(1024) lp_rows_kernel(const LpRowsArgs a) {
  __shared__ unsigned long long cand[16 * KL];           // wave w's q-th largest key at w * KL + q
  __shared__ unsigned long long sel[KL];
  __shared__ float smx[16];
  __shared__ double ssum[16];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V;
  const float* lg = a.logits + (size_t)r * V;
  const int rounds = a.k > 1 ? a.k : 1;
  unsigned long long top[KL];
#pragma unroll
  for (int j = 0; j < KL; ++j) top[j] = 0;
  float mx = -INFINITY;
  bool bad = false;
  unsigned long long kmax = 0;
  auto take = [&](float v, int i) {
    bad = bad || !(v < INFINITY);                        // NaN or +inf
    mx = fmaxf(mx, v);
    const unsigned long long key = argmax_key(v, i);
    kmax = key > kmax ? key : kmax;
  };
  // ---- pass 1: the thread's largest key, max and the non-finite flag
  if ((V & 3) == 0) {
    const f4* l4 = reinterpret_cast<const f4*>(lg);
    for (int c = tid; c < V / 4; c += 1024) {
      const f4 v = l4[c];
      take(v.x, 4 * c); take(v.y, 4 * c + 1); take(v.z, 4 * c + 2); take(v.w, 4 * c + 3);
    }
  } else {
    for (int i = tid; i < V; i += 1024) take(lg[i], i);
  }
  mx = wave_max(bad ? INFINITY : mx);                    // a non-finite row reduces to m = +inf
  if (lane == 0) smx[wave] = mx;
  unsigned long long thr = 0;                            // the wave's rounds-th largest lane maximum (0: fewer lanes hold a key)
  {
    unsigned long long c = kmax;
    for (int q = 0; q < rounds; ++q) {
      thr = wave_max_u64(c);
      c = (c == thr) ? 0ull : c;
    }
  }
  auto insert = [&](float v, int i) {
    unsigned long long key = argmax_key(v, i);
    if (key >= thr && key > top[KL - 1]) {
#pragma unroll
      for (int j = 0; j < KL; ++j) {                     // insert, keeping top[] descending
        const unsigned long long t = top[j];
        top[j] = key > t ? key : t;
        key = key > t ? t : key;
      }
    }
  };
  __syncthreads();
  float m = -INFINITY;
  for (int w = 0; w < 16; ++w) m = fmaxf(m, smx[w]);
  const bool fin = m > -INFINITY && m < INFINITY;
  // ---- pass 2: sum_j exp(x_j - m) in fp64, in the one order (finite rows), and the thread's keys at or above the threshold
  const double md = (double)m;
  double s = 0.0;
  if ((V & 3) == 0) {
    const f4* l4 = reinterpret_cast<const f4*>(lg);
    for (int c = tid; c < V / 4; c += 1024) {
      const f4 v = l4[c];
      if (fin) { s += exp_fast((double)v.x - md); s += exp_fast((double)v.y - md); s += exp_fast((double)v.z - md); s += exp_fast((double)v.w - md); }
      insert(v.x, 4 * c); insert(v.y, 4 * c + 1); insert(v.z, 4 * c + 2); insert(v.w, 4 * c + 3);
    }
  } else {
    for (int i = tid; i < V; i += 1024) {
      const float v = lg[i];
      if (fin) s += exp_fast((double)v - md);
      insert(v, i);
    }
  }
  s = wave_sum(s);
  if (lane == 0) ssum[wave] = s;
  // ---- top-k: round q of a wave takes its largest remaining key out of the one lane list that holds it (keys are unique: they carry
  // the index); then wave 0 does the same over the 16 waves' keys, lane l holding candidates l, l + 64, ...
  for (int q = 0; q < rounds; ++q) {
    const unsigned long long h = wave_max_u64(top[0]);
    if (h != 0 && top[0] == h) {
#pragma unroll
      for (int j = 0; j + 1 < KL; ++j) top[j] = top[j + 1];
      top[KL - 1] = 0;
    }
    if (lane == 0) cand[wave * KL + q] = h;
  }
  __syncthreads();
  if (wave == 0) {
    constexpr int PER = (16 * KL + 63) / 64;
    unsigned long long cv[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) { const int i = lane + 64 * e; cv[e] = (i < 16 * KL && i % KL < rounds) ? cand[i] : 0ull; }
    for (int q = 0; q < rounds; ++q) {
      unsigned long long mk = 0;
#pragma unroll
      for (int e = 0; e < PER; ++e) mk = cv[e] > mk ? cv[e] : mk;
      const unsigned long long best = wave_max_u64(mk);
#pragma unroll
      for (int e = 0; e < PER; ++e) cv[e] = (cv[e] == best) ? 0ull : cv[e];
      if (lane == 0) sel[q] = best;
    }
  }
  __syncthreads();
  double tot = 0.0;
  for (int w = 0; w < 16; ++w) tot += ssum[w];
  const double lse = fin ? md + log(tot) : __builtin_nan("");
  if (tid == 0) {
    const unsigned long long b0 = sel[0];
    a.amax[r] = (b0 == 0) ? 0 : (int)~(unsigned)b0;      // nothing but NaN: reduce() keeps index 0
    const int t = a.target[r];
    a.lp[r] = (t < 0 || !fin) ? __builtin_nan("") : (double)lg[t] - lse;
  }
  if (tid < a.k) {
    const unsigned long long key = sel[tid];
    const int id = (key == 0) ? 0 : (int)~(unsigned)key;
    a.top_ids[(size_t)r * a.k + tid] = id;
    a.top_lp[(size_t)r * a.k + tid] = fin ? (double)lg[id] - lse : __builtin_nan("");
  }
}

}  // namespace l2k
