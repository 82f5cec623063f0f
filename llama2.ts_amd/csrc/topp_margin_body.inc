// topp_margin_body.inc -- the body of topp_margin_kernel and topp_margin_rows_kernel (sampler.hip), included inside each
// kernel's braces (a function would be optimised on its own before inlining, and move the existing kernel's instruction stream).
// The including scope names `a` (MarginArgs) and `sh` (MarginShared).  Not a stand-alone header.
  const int tid = threadIdx.x, n = a.V;
  const double topp = a.params[1];
  const double own = tid < a.G ? a.part_sorted[tid] : 0.0;
  double Qn;
  const double incl = block_scan(own, sh.wsum, &Qn);
  if (tid == 0) sh.val[1] = (double)random_f32(a.rng);
  __syncthreads();
  if (tid < a.G) a.part_sorted[tid] = 0.0;
  const double u = sh.val[1];
  const double M = mr::margin(n, Qn, 0.0);
  auto sorted = [&](int i) { return a.sorted[i]; };
  int token = 0;
  bool serial = a.force_serial || !(Qn > 0.0 && Qn <= 1.7976931348623157e308);
  if (!serial) {
    // cumProb > topp (:385): `topp < cum_i` with an exact constant
    double qc;
    const int c = decide_first(sorted, n, a.G, topp, M, n, incl, own, sh, &qc);
    if (c == -2) serial = true;
    else if (c <= 0) token = 0;                                // never crossed (lastIdx stays 0, :383) or crossed by the first: the second loop is empty
    else {
      __syncthreads();
      double qh;
      const int hit = decide_first(sorted, n, a.G, u * qc, 2.0 * M, c, incl, own, sh, &qh);   // cumProb as the loop left it (:388), i < lastIdx only (:390)
      if (hit == -2) serial = true;
      else token = hit < 0 ? 0 : a.ids[hit];
    }
  }
  if (serial) {                                                // llama2.ts:382-393 as written
    double cum;
    const int at = serial_sum(sorted, n, sh, &cum, true, topp);
    const int last = at < 0 ? 0 : at;
    const int hit = serial_first(sorted, last, u * cum, sh);
    token = hit < 0 ? 0 : a.ids[hit];
  }
  pick_done(a, token, serial);
