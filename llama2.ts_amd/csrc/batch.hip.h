// batch.hip.h -- batched greedy decode of independent sequences over one copy of the weights (kernels of its own; host side:
// batch_host.hip.h).
//
// A decode step of n sequences (n <= 64) is prefill's launch sequence with one row per SEQUENCE instead of one per prompt position:
// every GEMM streams each weight once for all n rows on the fp64 MFMA (prefill.hip.h: pf_gemm_kernel / pf_gemm3_kernel), so the
// numeric contract is prefill's (exact products, fp64 accumulation, one fp32 rounding per stored element).  What differs per row
// lives in device tables -- row t feeds token tok[t] at position pos[t] of sequence seq[t] -- read by the q / k / v epilogue (RoPE
// and the cache stores: pf_emit<MODE_QKV_ROWS>), the attention kernel (attention.hip.h: bt_attn_tile_kernel, one workgroup per
// (head, row) over that row's own cache) and the per-row pick below, so one recorded step serves every placement of the sequences.
// The step runs as a replayed hipGraph or eager launches on the context's stream, never on the library's AQL queue: every kernel
// boundary carries the usual acquire / release, and the tables the pick advances are read with plain loads by the next step.
#pragma once
#include "prefill.hip.h"

namespace l2k {

// Row r's pick (llama2.ts:364-366: first maximum, the argmax_key rules -- NaN at index 0, +-0, +-inf), then the step's bookkeeping:
// the token is fed next (tok[r]), recorded at out[r * out_stride + pos[r] - start[r]], and the row moves to the next position.
__global__ void __launch_bounds__(1024) bt_argmax_kernel(const float* logits, int V, int* tok, int* pos, const int* start, int* out, int out_stride) {
  __shared__ unsigned long long sk[16];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* lg = logits + (size_t)r * V;
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
      const int p = pos[r];
      out[(size_t)r * out_stride + (p - start[r])] = bi;
      tok[r] = bi;
      pos[r] = p + 1;
    }
  }
}

}  // namespace l2k
