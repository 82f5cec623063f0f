// batch.hip.h -- batched greedy decode of independent sequences over one copy of the weights (kernels of its own; host side:
// batch_host.hip.h).
//
// A decode step of n sequences (n <= 64) is prefill's launch sequence with one row per SEQUENCE instead of one per prompt position:
// every GEMM streams each weight once for all n rows on the fp64 MFMA (prefill.hip.h: pf_gemm_kernel / pf_gemm3_kernel), so the
// numeric contract is prefill's (exact products, fp64 accumulation, one fp32 rounding per stored element).  What differs per row
// lives in device tables -- row t feeds token tok[t] at position pos[t] of sequence seq[t] -- read by the q / k / v epilogue (RoPE
// and the cache stores: pf_emit<MODE_QKV_ROWS>), the attention kernel (attention.hip.h: bt_attn_tile_kernel, one workgroup per
// (head, row) over that row's own cache) and the per-row pick below, so one recorded step serves every placement of the sequences.
// The sampled step (l2_decode_sample_batch) ends with the row form of the device sampler (sampler.h: RowSampler) and bt_pick_kernel.
// The step runs as a replayed hipGraph or eager launches on the context's stream, never on the library's AQL queue: every kernel
// boundary carries the usual acquire / release, and the tables the pick advances are read with plain loads by the next step.
// Packed prompts (l2_seq_prefill_batch) run prefill's launch sequence over several sequences' prompt rows at once: the same per-row
// q / k / v epilogue (also in the register-blocked GEMMs), the row-agnostic GEMMs as they are, and bp_attn_mfma_kernel below.
#pragma once
#include "prefill.hip.h"

namespace l2k {

// Row r's pick (llama2.ts:364-366: first maximum, the argmax_key rules -- NaN at index 0, +-0, +-inf), then the step's bookkeeping:
// the token is fed next (tok[r]), recorded at out[r * out_stride + pos[r] - start[r]], and the row moves to the next position.
__global__ void __launch_bounds__(1024) bt_argmax_kernel(const float* logits, int V, int* tok, int* pos, const int* start, int* out, int out_stride) {
#include "bt_argmax_body.inc"
}

// The sampled step's last launch: row r takes its argmax when its temperature params[2 r] is 0 (no draw), else the token the row
// sampler left in pick[4 r] (sampler.h: RowSampler); every row's pick is applied exactly once, as bt_argmax_kernel does it.
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

// ------------------------------------------------------------------------------------------------
// Attention of packed prompts (l2_seq_prefill_batch): the rows of one launch sequence are several sequences' prompt runs back to back,
// cut into TILES of up to 16 consecutive rows of one sequence, each starting at its run's first row or 16 rows after the previous tile.
// One workgroup per (head, tile), with pf_attn_mfma_kernel's arithmetic (prefill.hip.h) over the tile's own sequence's cache: scores on
// v_mfma_f64_16x16x4_f64, one fp32 rounding of dot x 1/sqrt(hs), causal mask by position, the reference's softmax roundings, P V in fp64
// with ONE rounding.  Every query row's result depends on its own position and keys only, so it is what the single prompt's tiling gives.
// The cache rows of the whole launch sequence were stored by the q / k / v GEMM before this launch: a row at position p sees rows
// 0 .. p of its sequence, those of earlier runs and launch sequences included.
struct BpTile { int seq, row0, pos0, nvalid; };     // sequence, first packed row, its position, valid rows (1 .. 16)
struct BpAttnArgs {
  const float* q;           // [rows][dim] rotated queries of the launch sequence
  float* xb;                // [rows][dim] out
  float* const* seq_kc;     // per sequence: cache slabs [L][S][dim]; this layer's starts seq_loff further
  float* const* seq_vc;
  size_t seq_loff;
  const BpTile* tiles;      // [gridDim.y]
  int dim, seq_len;
  double inv_sqrt_hs;
};

template <int HS>      // head_size: 64 or 128
__global__ void __launch_bounds__(256) bp_attn_mfma_kernel(const BpAttnArgs a) {
  static_assert(HS % 64 == 0, "four waves x whole 16-wide column tiles");
  constexpr int KB = HS / 16;                          // 16-column blocks of a head row
  constexpr int CT = HS / 64;                          // output column tiles per wave
  extern __shared__ __attribute__((aligned(16))) char bpa_smem[];
  const int h = blockIdx.x;
  const BpTile tl = a.tiles[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  const int P0 = tl.pos0;                              // position of the tile's query row 0
  const int T = P0 + 16;                               // keys 0 .. T-1 cover every query of the tile
  const int Tb = (T + 15) >> 4;                        // key blocks of 16
  const int ST = Tb * 16 + 4;                          // LDS row stride, floats
  float* sc = reinterpret_cast<float*>(bpa_smem);      // [16][ST]
  const int dim = a.dim;
  const unsigned slab = (unsigned)a.seq_len * (unsigned)dim * 4u;      // keys past seq_len read as zeros (and are masked)
  const auto krs = __builtin_amdgcn_make_buffer_rsrc(a.seq_kc[tl.seq] + a.seq_loff, 0, slab, 0x00020000);
  const auto vrs = __builtin_amdgcn_make_buffer_rsrc(a.seq_vc[tl.seq] + a.seq_loff, 0, slab, 0x00020000);

  // ---- Q fragments of the tile, widened once: lane (j, kq) holds q[row0 + j][h*HS + 16 b + 4 kq + e]; rows past the tile's last
  // read its last row (a tile may end the launch sequence's rows: nothing past them is read)
  double qd[KB][4];
  {
    const float* qrow = a.q + (size_t)(tl.row0 + min(j, tl.nvalid - 1)) * dim + (size_t)h * HS + 4 * kq;
#pragma unroll
    for (int b = 0; b < KB; ++b) {
      const f4 v = *reinterpret_cast<const f4*>(qrow + 16 * b);
      qd[b][0] = v.x; qd[b][1] = v.y; qd[b][2] = v.z; qd[b][3] = v.w;
    }
  }
  // ---- scores: key block kb (keys 16 kb .. 16 kb + 15) -> D[query kq + 4 r][key j]
  const unsigned kvoff = (unsigned)(((size_t)j * dim + (size_t)h * HS + 4 * kq) * 4);     // this lane's element of a 16-row block
  const unsigned blk = 16u * (unsigned)dim * 4u;                                          // bytes per key block
  const double rsq = a.inv_sqrt_hs;
  for (int kb = wave; kb < Tb; kb += 4) {
    f4 kf[KB];
#pragma unroll
    for (int b = 0; b < KB; ++b) kf[b] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(krs, kvoff, (unsigned)kb * blk + (unsigned)b * 64u, 0));
    d4 acc = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};   // two chains: a dependent MFMA does not issue back to back
#pragma unroll
    for (int b = 0; b < KB; ++b) {
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(qd[b][0], (double)kf[b].x, acc, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(qd[b][1], (double)kf[b].y, acc1, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(qd[b][2], (double)kf[b].z, acc, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(qd[b][3], (double)kf[b].w, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += acc1[r];
    const int t = kb * 16 + j;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qi = kq + 4 * r;                        // query row of the tile; its position is P0 + qi
      const float s = (float)(acc[r] * rsq);            // one rounding (llama2.ts:253 divides by sqrt(head_size))
      sc[qi * ST + t] = (t <= P0 + qi) ? s : -INFINITY;
    }
  }
  __syncthreads();
  // ---- softmax per query row (llama2.ts:181-194): wave w owns rows 4w .. 4w + 3
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    float* row = sc + (wave * 4 + rr) * ST;
    const int nk = P0 + wave * 4 + rr + 1;              // keys this query sees
    float mx = -INFINITY;
    for (int t = lane; t < nk; t += 64) mx = fmaxf(mx, row[t]);
    mx = wave_max(mx);
    double lsum = 0.0;
    for (int t = lane; t < Tb * 16; t += 64) {
      const float e = (t < nk) ? (float)exp_fast((double)row[t] - (double)mx) : 0.0f;    // stored to fp32 (:187); masked keys contribute nothing
      row[t] = e;
      lsum += (double)e;                                                                  // sum of the ROUNDED values (:190)
    }
    lsum = wave_sum(lsum);
    const double rs = rcp_fast(lsum);
    for (int t = lane; t < nk; t += 64) row[t] = (float)((double)row[t] * rs);            // quotient stored fp32 (:192)
  }
  __syncthreads();
  // ---- xb = P V: wave w owns output columns [w * 16 CT, (w + 1) * 16 CT) of the head; D[query kq + 4 r][column j]
  d4 o[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) o[c] = d4{0.0, 0.0, 0.0, 0.0};
  const unsigned vcol = (unsigned)(((size_t)h * HS + (size_t)wave * 16 * CT + j) * 4);    // this lane's column, bytes
  for (int kb = 0; kb < Tb; ++kb) {
    const f4 pf = *reinterpret_cast<const f4*>(sc + j * ST + kb * 16 + 4 * kq);          // P[query j][keys 16 kb + 4 kq .. + 3]
    float vv[CT][4];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        vv[c][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(vrs, vcol + (unsigned)c * 64u + (unsigned)(kb * 16 + 4 * kq + e) * (unsigned)dim * 4u, 0, 0));
    const double p0 = pf.x, p1 = pf.y, p2 = pf.z, p3 = pf.w;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      o[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(p0, (double)vv[c][0], o[c], 0, 0, 0);
      o[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(p1, (double)vv[c][1], o[c], 0, 0, 0);
      o[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(p2, (double)vv[c][2], o[c], 0, 0, 0);
      o[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(p3, (double)vv[c][3], o[c], 0, 0, 0);
    }
  }
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qi = kq + 4 * r;
      if (qi < tl.nvalid) a.xb[(size_t)(tl.row0 + qi) * dim + (size_t)h * HS + (size_t)wave * 16 * CT + c * 16 + j] = (float)o[c][r];   // ONE rounding of the fp64 sum
    }
}

}  // namespace l2k
