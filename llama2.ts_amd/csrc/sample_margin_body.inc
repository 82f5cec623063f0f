// sample_margin_body.inc -- the body of sample_margin_kernel and sample_margin_rows_kernel (sampler.hip), included inside each
// kernel's braces (a function would be optimised on its own before inlining, and move the existing kernel's instruction stream).
// The including scope names `a` (MarginArgs) and `sh` (MarginShared).  Not a stand-alone header.
  const int tid = threadIdx.x, tile = blockIdx.x, n = a.V;
  const double T = tile_base(a.part, a.G);                     // tree total of the exps: the same bits in every lane of every workgroup
  const int win = mr::window(n);
  float v[IT];
  load_tile(a.exps, n, tile, v);
  double amb = 0.0;
#pragma unroll
  for (int k = 0; k < IT; ++k) v[k] = mr::quotient_checked(v[k], T, win, &amb);      // padding: e = 0 -> p = 0
  const double t = tile_total(v, sh.wsum);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) amb += __shfl_xor(amb, off, 64);
  if ((tid & 63) == 0) sh.wamb[tid >> 6] = amb;
  __syncthreads();
  if (tid == 0) {
    // write-through stores another CU's L1-bypassing loads see, drained before the ticket is taken (MI355X_MICROARCH.md, hand-off forms)
    __hip_atomic_store(a.part2 + tile, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.amb + tile, (sh.wamb[0] + sh.wamb[1]) + (sh.wamb[2] + sh.wamb[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    sh.slot[3] = (int)__hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (sh.slot[3] != a.G - 1) return;
  // ---- the last workgroup: every tile's sums are in memory
  const double own = tid < a.G ? __hip_atomic_load(a.part2 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
  const double own_amb = tid < a.G ? __hip_atomic_load(a.amb + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
  double Qn, A;
  const double incl = block_scan(own, sh.wsum, &Qn);
  block_scan(own_amb, sh.wamb, &A);
  if (tid == 0) { sh.val[1] = (double)random_f32(a.rng); __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }   // past the L2, where the adds are made
  __syncthreads();
  const double u = sh.val[1];
  const double M = mr::margin(n, Qn, A);
  auto prob = [&](int i) { return (float)((double)a.exps[i] / T); };
  int hit = -2;
  double qhit;
  if (!a.force_serial && Qn > 0.0 && Qn <= 1.7976931348623157e308) hit = decide_first(prob, n, a.G, u * Qn, M, n, incl, own, sh, &qhit);   // randValue = random_f32() * sum (:370)
  const bool serial = hit == -2;
  if (serial) {                                                // llama2.ts:189-192, :368-376 as written
    double total, sum;
    serial_sum([&](int i) { return a.exps[i]; }, n, sh, &total, false, INFINITY);
    auto p = [&](int i) { return (float)((double)a.exps[i] / total); };
    serial_sum(p, n, sh, &sum, true, INFINITY);
    hit = serial_first(p, n, u * sum, sh);
  }
  pick_done(a, hit < 0 ? 0 : hit, serial);                     // fall-through returns 0 (:375)
