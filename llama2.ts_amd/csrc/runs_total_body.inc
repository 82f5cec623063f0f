// runs_total_body.inc -- the body of runs_total_kernel and runs_total_rows_kernel (sampler.hip), included inside each
// kernel's braces (a function would be optimised on its own before inlining, and move the existing kernel's instruction stream).
// The including scope names `a` (ChainArgs), `recs`, `cnt`, `ticket`, `total` and `sh` (ChainShared).  Not a stand-alone header.
  float v[IT];
  load_tile(a.x, a.V, blockIdx.x, v);
  Elems el;
  tile_scan(v, tile_base(a.part, blockIdx.x), sh.tile, el);
  emit_runs<false, true>(el, v, a.V, blockIdx.x, recs, cnt, nullptr, nullptr);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) sh.slot = (int)__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (sh.slot != a.G - 1) return;
  __syncthreads();
  bool in_lds;
  chain_total<true>(a, sh, &in_lds);
  if (threadIdx.x == 0) { *total = sh.val; __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
