// batch.hip.h -- batched greedy decode of independent sequences over one copy of the weights (kernels of its own; host side:
// batch_host.hip.h).
//
// A decode step of n sequences (n <= 64) is prefill's launch sequence with one row per SEQUENCE instead of one per prompt position:
// every GEMM streams each weight once for all n rows on the fp64 MFMA (prefill.hip.h: pf_gemm_kernel / pf_gemm3_kernel), so the
// numeric contract is prefill's (exact products, fp64 accumulation, one fp32 rounding per stored element).  What differs per row
// lives in device tables -- row t feeds token tok[t] at position pos[t] of sequence seq[t] -- read by the q / k / v epilogue (RoPE
// and the cache stores: pf_emit<MODE_QKV_ROWS>), the attention kernel (attention.hip.h: bt_attn_tile_kernel, one workgroup per
// (head, row) over that row's own cache) and the per-row pick below, so one recorded step serves every placement of the sequences.
// The sampled step (l2_decode_sample_batch) ends with the row form of the device sampler (sampler.h: BatchSampler) and bt_pick_kernel.
// The step runs as a replayed hipGraph or eager launches on the context's stream, never on the library's AQL queue: every kernel
// boundary carries the usual acquire / release, and the tables the pick advances are read with plain loads by the next step.
#pragma once
#include "prefill.hip.h"

namespace l2k {

// Row r's pick (llama2.ts:364-366: first maximum, the argmax_key rules -- NaN at index 0, +-0, +-inf), then the step's bookkeeping:
// the token is fed next (tok[r]), recorded at out[r * out_stride + pos[r] - start[r]], and the row moves to the next position.
__global__ void __launch_bounds__(1024) bt_argmax_kernel(const float* logits, int V, int* tok, int* pos, const int* start, int* out, int out_stride) {
#include "bt_argmax_body.inc"
}

// The sampled step's last launch: row r takes its argmax when its temperature params[2 r] is 0 (no draw), else the token the row
// sampler left in pick[4 r] (sampler.h: BatchSampler); every row's pick is applied exactly once, as bt_argmax_kernel does it.
__global__ void __launch_bounds__(1024) bt_pick_kernel(const float* logits, int V, const double* params, int* pick, int* tok, int* pos, const int* start,
                                                       int* out, int out_stride) {
  if (params[2 * blockIdx.x] != 0.0) {
    if (threadIdx.x == 0) {
      const int q = blockIdx.x, p = pos[q], bi = pick[4 * q];
      pick[4 * q + 2] = 0;                                     // the row sampler's advance() writes its token at step 0 again
      out[(size_t)q * out_stride + (p - start[q])] = bi;
      tok[q] = bi;
      pos[q] = p + 1;
    }
    return;
  }
#include "bt_argmax_body.inc"
}

}  // namespace l2k
