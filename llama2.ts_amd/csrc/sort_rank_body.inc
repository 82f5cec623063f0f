// sort_rank_body.inc -- the body of sort_rank_kernel and sort_rank_rows_kernel (sampler.hip), included inside each
// kernel's braces (a function would be optimised on its own before inlining, and move the existing kernel's instruction stream).
// The including scope names `run_p`, `run_id`, `GS`, `G`, `acc`, `sorted`, `ids`, `part` and the LDS arrays `lds_p`, `lpart`.  Not a stand-alone header.
  const int tid = threadIdx.x, n = GS * STILE;
  for (int j = tid; j < G; j += RT) lpart[j] = 0.0;
  const int e = blockIdx.x * RT + tid;
  const int mine = e < n ? reinterpret_cast<const int*>(run_p)[e] : -1;
  const int own = e / STILE;
  const int g0 = blockIdx.y * RANK_TQ, gt = min(RANK_TQ, GS - g0), gn = gt * STILE, groups = gridDim.y;
  {
    // one 16-byte load in flight per thread (deeper queues measured slower), every workgroup starting at another tile
    const int* src = reinterpret_cast<const int*>(run_p) + (size_t)g0 * STILE;
    const int rot = (int)(blockIdx.x % (unsigned)gt) * STILE;
    for (int j = tid * 4; j < gn; j += RT * 4) { int jj = j + rot; if (jj >= gn) jj -= gn; *reinterpret_cast<int4*>(lds_p + jj) = *reinterpret_cast<const int4*>(src + jj); }
  }
  __syncthreads();
  if (mine >= 0) {                                              // not a pad
    int lo[RANK_TQ], thr[RANK_TQ];
#pragma unroll
    for (int u = 0; u < RANK_TQ; ++u) {
      const int b = min(u, gt - 1);
      lo[u] = b * STILE;
      thr[u] = mine - (g0 + b < own ? 1 : 0);                   // earlier tile: elements >= mine come first; later tile: only > mine
    }
#pragma unroll
    for (int s = STILE / 2; s > 0; s >>= 1) {
#pragma unroll
      for (int u = 0; u < RANK_TQ; ++u) if (lds_p[lo[u] + s - 1] > thr[u]) lo[u] += s;
    }
    unsigned count = (own >= g0 && own < g0 + gt) ? (unsigned)(e - own * STILE) : 0u;   // its place in its own tile, counted once
#pragma unroll
    for (int u = 0; u < RANK_TQ; ++u) {
      const int b = min(u, gt - 1);
      int cnt = lo[u] - b * STILE;
      if (cnt == STILE - 1 && lds_p[lo[u]] > thr[u]) cnt = STILE;
      if (u < gt && g0 + b != own) count += (unsigned)cnt;
    }
    const unsigned before = groups > 1 ? atomicAdd(acc + e, count + (1u << 24)) : 0u;
    if ((int)(before >> 24) == groups - 1) {                     // every other group has reported: the rank is complete
      const int rank = (int)((before & 0xffffffu) + count);
      if (groups > 1) __hip_atomic_store(acc + e, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // past the L2, like the adds
      sorted[rank] = __int_as_float(mine);
      ids[rank] = run_id[e];
      atomicAdd(lpart + rank / TILE, (double)__int_as_float(mine));
    }
  }
  __syncthreads();
  for (int j = tid; j < G; j += RT) if (lpart[j] != 0.0) atomicAdd(part + j, lpart[j]);
