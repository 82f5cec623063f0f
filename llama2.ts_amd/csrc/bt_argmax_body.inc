// bt_argmax_body.inc -- the body of bt_argmax_kernel and bt_pick_kernel (batch.hip.h), included inside each
// kernel's braces (a function would be optimised on its own before inlining, and move the existing kernel's instruction stream).
// The including scope names `logits`, `V`, `tok`, `pos`, `start`, `out`, `out_stride`.  Not a stand-alone header.
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
