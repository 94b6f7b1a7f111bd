// fw_slow_body.inc -- the body of k_slow and k_slow_cont (fw_device.hip), included once into each with FW_SLOW_CONT
// false / true.  Text, not a function template: with the body behind a call, even a forced-inline one, the compiler
// allocates k_slow's registers differently (two more SGPR spills), and the kernels of the handles that exist keep
// the code they had.  Parameters: c, wm, srow, T, sk, stt, sv, skh, tb, out, side, st, resume.
  if (__hip_atomic_load(&st->suspended, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;  // resumed later
  // list length: the ordered-path offset of the last tile plus that tile's own count
  const int64_t n = (int64_t)(srow[T - 1] - srow[0]) + srow[T + T - 1];
  const int64_t first = resume ? st->slow_resume : 0;
  if (first >= n) return;
  __shared__ int64_t ck[SLOW_CHUNK];
  __shared__ int32_t ci[SLOW_CHUNK], cp[SLOW_CHUNK], cd[SLOW_CHUNK];
  __shared__ int bad;
  SlowCtx x{c, wm, tb, out, side, st};
  unsigned long long late = 0;
  const int tid = threadIdx.x;
  const int64_t row_bound = c.assigner == FW_SESSION ? 1 : c.wpr;  // fired rows per record, at most
  int64_t b0 = first;
  for (; b0 < n; b0 += SLOW_CHUNK) {
    const int m = (int)min((int64_t)SLOW_CHUNK, n - b0);
    if (tid == 0) bad = 0;
    if (tid < m) {
      const int64_t i = b0 + tid;
      ck[tid] = sk[i];
      cp[tid] = partition_of(c, ck[tid], skh[i]);
      int64_t last;
      cd[tid] = c.assigner == FW_SESSION ? 1 : num_windows(c, stt[i], &last);  // new windows, at most
      ci[tid] = tid;
    } else {
      ck[tid] = LMAX;
      cp[tid] = INT32_MAX;
      cd[tid] = 0;
      ci[tid] = INT32_MAX;
    }
    __syncthreads();
    // bitonic sort by (partition, key, arrival index): a key's records stay in arrival order and a
    // partition's records are contiguous, so its demand on the region is one segmented sum
    for (int kk = 2; kk <= SLOW_CHUNK; kk <<= 1) {
      for (int jj = kk >> 1; jj > 0; jj >>= 1) {
        const int o = tid ^ jj;
        if (o > tid) {
          const bool up = (tid & kk) == 0;
          const int32_t pa = cp[tid], pb = cp[o];
          const int64_t a = ck[tid], b = ck[o];
          const int32_t ia = ci[tid], ib = ci[o];
          const bool gt = pa > pb || (pa == pb && (a > b || (a == b && ia > ib)));
          if (gt == up) {
            cp[tid] = pb;
            cp[o] = pa;
            ck[tid] = b;
            ck[o] = a;
            ci[tid] = ib;
            ci[o] = ia;
            const int32_t da = cd[tid];
            cd[tid] = cd[o];
            cd[o] = da;
          }
        }
        __syncthreads();
      }
    }
    // capacity: every region the chunk touches must take its new windows within the load limit,
    // and the fired-row buffer must take every row the chunk may fire; otherwise suspend here
    if (tid < m && (tid == 0 || cp[tid - 1] != cp[tid])) {
      int64_t demand = 0;
      for (int j = tid; j < m && cp[j] == cp[tid]; j++) demand += cd[j];
      const int64_t want = (int64_t)tb.live[cp[tid]] + demand;
      if (want > region_limit(c.log_r)) {
        bad = 1;
        atomicMax(&st->need_live, (int32_t)min(want, (int64_t)INT32_MAX));
      }
    }
    if (tid == 0) {
      const int64_t want = (int64_t)__hip_atomic_load(&st->out_rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) +
                           (int64_t)m * row_bound;
      if (want > out.slow_limit) {
        bad = 1;
        atomicMax((long long*)&st->need_out, (long long)want);
      }
    }
    __syncthreads();
    if (bad) break;
    if (tid < m && (tid == 0 || ck[tid - 1] != ck[tid] || cp[tid - 1] != cp[tid])) {
      for (int j = tid; j < m && ck[j] == ck[tid] && cp[j] == cp[tid]; j++) {
        const int64_t i = b0 + ci[j];
        const int64_t k = sk[i], t = stt[i], v = sv[i];
        const int64_t fo = agg_ordinal(c) ? c.slow_ord[i] : 0;
        const int32_t p = cp[j];
        bool skipped = true;
        if constexpr (FW_SLOW_CONT)  // (never sessions)
          replay_time_windows<true>(x, p, k, t, v, fo, &skipped);
        else if (c.assigner == FW_SESSION)
          replay_session(x, p, k, t, v, fo, &skipped);
        else
          replay_time_windows<false>(x, p, k, t, v, fo, &skipped);
        if (skipped && jadd(t, c.lateness) <= wm) {  // isSkippedElement && isElementLate
          if (c.side_output)
            side_one(side, st, k, t, v);
          else
            late++;
        }
      }
    }
    __syncthreads();
  }
  if (late) atomicAdd(&st->late_dropped, late);
  if (tid == 0) {
    atomicAdd(&st->slow_total, (unsigned long long)(min(b0, n) - first));
    if (b0 < n) {
      st->slow_resume = b0;
      atomicOr(&st->suspended, (int)FW_SUSP_SLOW);
    }
  }
