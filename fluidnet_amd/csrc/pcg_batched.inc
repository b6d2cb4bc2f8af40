// pcg_batched.inc -- solveLinearSystemPCGBatched: pcg.hip's solve with every batch item advancing in the SAME launches. Included
// by pcg.hip inside its unnamed namespace: the kernels here run pcg.hip's kernel bodies (d_*) with the batch item in blockIdx.y.
//
// A system is (item b, the c-th component of item b in scan order). Round c advances the c-th system of every item at once, for
// c = 0 .. max over the items of the component count - 1; an item without a c-th system (or with one of size 1) is `done` from
// the start of the round and its blocks return at once. What pcg_solve's host code decides per component -- root, size, the
// preconditioner (none below 5 cells), closed or open -- the kernels read from the item's record (PcgItemRec, device memory),
// which k_pcgb_round fills from the component table and the mg set-up completes. Item b's arrays lie b * stride floats behind
// item 0's (pcg_batched_ws); flags, div and p are the caller's tensors, b * n floats on.
// Why every item gets the bits pcg_solve gives it: the arithmetic is the d_* / mg_* device functions themselves, a cell's value
// never depends on the thread that computes it, and every reduction keeps its kRedBlocks partial sums and their order, one set per
// item (blockIdx.x is the partial's index as before). The chunk length differs (one for the batch), which no value depends on:
// the kernels of an iteration past convergence return, and the host's exit test is the device's next top-of-loop test.
// Host round trips: B "changed" words per labelling round; the counts once; the component table once; B states per chunk.

// ---- labelling: cc = [kPcgCcWords][B] int32: changed | count | border fluid | spare ----------------------------------------------
__global__ __launch_bounds__(256) void k_cc_init_b(Dom d, bool is3d, int B, const float* __restrict__ flags, int* __restrict__ label,
                                                   int* __restrict__ size_at, long long stride, int* __restrict__ cc) {
  const int b = blockIdx.y, o = blockIdx.x * 256 + threadIdx.x;
  if (o < d.sc) size_at[b * stride + o] = 0;
  d_cc_init(d, is3d, flags + (long long)b * d.sc, label + b * stride, cc + 2 * B + b);
}
__global__ __launch_bounds__(256) void k_cc_hook_b(Dom d, bool is3d, int* __restrict__ label, long long stride, int* __restrict__ cc) {
  d_cc_hook(d, is3d, label + blockIdx.y * stride, cc + blockIdx.y);
}
__global__ __launch_bounds__(256) void k_cc_compress_b(Dom d, int* __restrict__ label, long long stride) {
  d_cc_compress(d, label + blockIdx.y * stride);
}
__global__ __launch_bounds__(256) void k_cc_count_b(Dom d, int B, const int* __restrict__ label, int* __restrict__ size_at,
                                                    int* __restrict__ roots, long long stride, int* __restrict__ cc) {
  const long long off = blockIdx.y * stride;
  d_cc_count(d, label + off, size_at + off, roots + off, cc + B + blockIdx.y);
}
// comps[b][rank] = {root, size}, the roots ascending (scan order of the first cell, as read_components sorts them): a root's
// rank is the number of smaller roots
__global__ __launch_bounds__(256) void k_cc_table_b(int B, const int* __restrict__ roots, const int* __restrict__ size_at,
                                                    long long stride, const int* __restrict__ cc, int* __restrict__ comps) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int cnt = min(cc[B + b], kMaxComponents);
  if (i >= cnt) return;
  const int* rt = roots + b * stride;
  const int root = rt[i];
  int rank = 0;
  for (int j = 0; j < cnt; j++) rank += rt[j] < root ? 1 : 0;
  int* row = comps + ((long long)b * kMaxComponents + rank) * 2;
  row[0] = root; row[1] = size_at[b * stride + root];
}

// ---- a round's records ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pcgb_round(PcgBatch bt, int B, const int* __restrict__ cc, const int* __restrict__ comps, int c,
                                                   int precond) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const bool has = c < min(cc[B + b], kMaxComponents);
  const int* row = comps + ((long long)b * kMaxComponents + (has ? c : 0)) * 2;
  PcgItemRec rc{};
  rc.root = has ? row[0] : -1;
  rc.size = has ? row[1] : 0;
  rc.pc = rc.size < 5 ? 0 : precond;          // generic/tfluids.cu:1390-1393
  rc.open = 0;                                // k_mg_level0_b raises it
  rc.active = (has && rc.size != 1) ? 1 : 0;  // :1375-1383: a single cell has no valid solution, its pressure stays 0
  bt.rec[b] = rc;
}

// ---- CG: pcg.hip's bodies on the item's arrays ----------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T* item_at(T* p, long long off) { return reinterpret_cast<T*>(reinterpret_cast<float*>(p) + off); }
template <class T>
__device__ __forceinline__ const T* item_at(const T* p, long long off) { return reinterpret_cast<const T*>(reinterpret_cast<const float*>(p) + off); }

// what the vectors of a CG iteration are for the kernels: item 0's, all of one block
struct PcgVecs {
  const int* label;
  float *x, *r, *z, *s, *w;
  double *partials, *p_den, *p_rr;
};

__global__ __launch_bounds__(256) void k_pcg_setup_b(PcgBatch bt, long long n, PcgVecs v, const float* __restrict__ div) {
  const int b = blockIdx.y;
  const PcgItemRec& rc = bt.rec[b];
  if (!rc.active) return;
  const long long off = b * bt.stride;
  // z is only ever written on the component; its other cells must read as 0 in s = z and r.z
  for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n; o += (long long)gridDim.x * 256) v.z[off + o] = 0.0f;
  d_pcg_setup(n, v.label + off, rc.root, div + b * n, v.x + off, v.r + off, v.s + off, item_at(v.partials, off));
}
__global__ __launch_bounds__(256) void k_pcg_begin_b(PcgBatch bt, PcgVecs v, float tol, int max_iter) {
  const int b = blockIdx.y;
  PcgState* S = pcg_state_of(bt, b);
  if (!bt.rec[b].active) {     // no system in this round: done before it starts
    if (threadIdx.x == 0) { S->rr1 = 0.0; S->iter = 0; S->bad = 0; S->pending = 0; S->done = 1; }
    return;
  }
  d_pcg_begin(S, item_at(v.partials, b * bt.stride), tol, max_iter);
}
__global__ __launch_bounds__(256) void k_pcg_top_b(PcgBatch bt, PcgVecs v, int test) {
  d_pcg_top(pcg_state_of(bt, blockIdx.y), item_at(v.p_rr, blockIdx.y * bt.stride), test);
}
__global__ __launch_bounds__(256) void k_pcg_dot_b(PcgBatch bt, long long n, PcgVecs v) {
  const int b = blockIdx.y;
  const PcgState* S = pcg_state_of(bt, b);
  if (S->done || !bt.rec[b].pc) return;
  const long long off = b * bt.stride;
  d_pcg_dot(S, n, v.r + off, v.z + off, item_at(v.partials, off));
}
__global__ __launch_bounds__(256) void k_pcg_dir_b(PcgBatch bt, long long n, PcgVecs v) {
  const int b = blockIdx.y;
  PcgState* S = pcg_state_of(bt, b);
  if (S->done) return;
  const long long off = b * bt.stride;
  const int pc = bt.rec[b].pc;
  d_pcg_dir(S, n, item_at(v.partials, off), pc ? 1 : 0, (pc ? v.z : v.r) + off, v.s + off);
}
template <bool IS3D>
__global__ __launch_bounds__(256) void k_pcg_apply_b(PcgBatch bt, Dom d, PcgVecs v, const float* __restrict__ flags) {
  const int b = blockIdx.y;
  const PcgState* S = pcg_state_of(bt, b);
  if (S->done) return;
  const long long off = b * bt.stride;
  d_pcg_apply<IS3D>(S, d, flags + (long long)b * d.sc, v.label + off, bt.rec[b].root, v.s + off, v.w + off, item_at(v.p_den, off));
}
__global__ __launch_bounds__(256) void k_pcg_update_b(PcgBatch bt, long long n, PcgVecs v) {
  const int b = blockIdx.y;
  PcgState* S = pcg_state_of(bt, b);
  if (S->done) return;
  const long long off = b * bt.stride;
  d_pcg_update(S, n, item_at(v.p_den, off), v.s + off, v.w + off, v.x + off, v.r + off, item_at(v.p_rr, off));
}
__global__ __launch_bounds__(256) void k_pcg_sum_b(PcgBatch bt, long long n, PcgVecs v) {
  const int b = blockIdx.y;
  if (!bt.rec[b].active) return;
  const long long off = b * bt.stride;
  d_pcg_sum(n, v.x + off, item_at(v.partials, off));
}
__global__ __launch_bounds__(256) void k_pcg_sum_end_b(PcgBatch bt, PcgVecs v) {
  const int b = blockIdx.y;
  if (!bt.rec[b].active) return;
  d_pcg_sum_end(pcg_state_of(bt, b), item_at(v.partials, b * bt.stride));
}
__global__ __launch_bounds__(256) void k_pcg_write_b(PcgBatch bt, long long n, PcgVecs v, float* __restrict__ p) {
  const int b = blockIdx.y;
  const PcgItemRec& rc = bt.rec[b];
  if (!rc.active) return;
  const long long off = b * bt.stride;
  d_pcg_write(pcg_state_of(bt, b), n, v.label + off, rc.root, rc.size, v.x + off, p + b * n);
}

// ---- host code ------------------------------------------------------------------------------------------------------------------
// One call of pcg_solve_batched: the views of pcg_batched_ws, the phases label / components / round.
struct BatchedSolve {
  hipStream_t st;
  const PcgProblem& q;
  Report er;
  Dom d;
  long long n;
  int B;
  bool mg;
  PcgBatchedWs t;
  PcgBatch bt;
  PcgVecs v;
  int *label, *size_at, *roots, *cc, *comps;
  MgDev mgd{};
  std::vector<int> h_cc, h_comps;          // [kPcgCcWords][B] | [B][maxc][2]
  int maxc = 0;
  std::vector<PcgState> h_state;           // one per slot, as read back
  std::vector<float> max_res;
  std::vector<long long> iters;

  BatchedSolve(hipStream_t st, const PcgProblem& q, float* workspace, char* msg, size_t msg_len);
  dim3 grid(int blocks) const { return dim3(blocks, B); }
  PcgResult label_items();
  PcgResult read_components();
  bool active(int b, int c) const { return c < h_cc[B + b] && h_comps[((size_t)b * maxc + c) * 2 + 1] != 1; }
  bool preconditioned(int b, int c) const { return mg && h_comps[((size_t)b * maxc + c) * 2 + 1] >= 5; }
  PcgResult round(int c);
  void iteration(bool any_mg);
  PcgResult run_chunks(int c, bool any_mg);
};

BatchedSolve::BatchedSolve(hipStream_t st_, const PcgProblem& q_, float* workspace, char* msg, size_t msg_len)
    : st(st_), q(q_), er{"solveLinearSystemPCGBatched", msg, msg_len}, d(whole_dom(q_.Z, q_.Y, q_.X)), n(d.sc), B(q_.B), mg(q_.precond == 3),
      t(pcg_batched_ws(q_.B, q_.Z, q_.Y, q_.X, q_.precond == 3, q_.is3d)) {
  float* it0 = workspace + t.items.off;      // item 0's block
  const PcgWs& w = t.item;
  bt = PcgBatch{view<PcgItemRec>(workspace, t.recs), view<PcgState>(workspace, t.states), t.stride};
  label = view<int>(it0, w.label); size_at = view<int>(it0, w.size_at); roots = view<int>(it0, w.roots);
  cc = view<int>(workspace, t.cc); comps = view<int>(workspace, t.comps);
  v = PcgVecs{label, view<float>(it0, w.x), view<float>(it0, w.r), view<float>(it0, w.z), view<float>(it0, w.s), view<float>(it0, w.w),
              view<double>(it0, w.partials), view<double>(it0, w.p_den), view<double>(it0, w.p_rr)};
  if (mg) {
    // as Solve's: level 0 keeps diag in dg, its second iterate in y; its right-hand side is r (open) or w (closed), per item
    const MgLevels ml = mg_levels(q.Z, q.Y, q.X, q.is3d);
    mgd.count = ml.count; mgd.first_block_level = ml.first_block_level;
    mgd.lv[0] = MgLv{ml.lv[0], (int)ml.lv[0].n, view<float>(it0, w.dg), view<float>(it0, w.mg_invd0), view<float>(it0, w.mg_cx0),
                     view<float>(it0, w.mg_cy0), view<float>(it0, w.mg_cz0), v.r, view<float>(it0, w.y), v.z};
    for (int l = 1; l < ml.count; l++) {
      const long long o = ml.lv[l].off;
      mgd.lv[l] = MgLv{ml.lv[l], (int)ml.lv[l].n, view<float>(it0, w.mg_c_diag) + o, view<float>(it0, w.mg_c_invd) + o,
                       view<float>(it0, w.mg_c_cx) + o, view<float>(it0, w.mg_c_cy) + o, view<float>(it0, w.mg_c_cz) + o,
                       view<float>(it0, w.mg_c_r) + o, view<float>(it0, w.mg_c_za) + o, view<float>(it0, w.mg_c_zb) + o};
    }
  }
  h_cc.assign((size_t)kPcgCcWords * B, 0);
  h_state.resize(B);
  max_res.assign(B, -std::numeric_limits<float>::infinity());
  iters.assign(B, 0);
}

// every item's labels: init, then hook + compress for all items until a round changes none of them (an item that has reached
// its fixed point is not changed by further rounds)
PcgResult BatchedSolve::label_items() {
  const int gcell = cdiv(n, 256);
  HIP_TRY(hipMemsetAsync(cc, 0, sizeof(int) * kPcgCcWords * B, st), "memset");
  { TFL_TIMED("k_cc", st); k_cc_init_b<<<grid(gcell), 256, 0, st>>>(d, q.is3d, B, q.flags, label, size_at, t.stride, cc); }
  for (int round = 0;; round++) {
    HIP_TRY(hipMemsetAsync(cc, 0, sizeof(int) * B, st), "memset");
    { TFL_TIMED("k_cc", st);
      k_cc_hook_b<<<grid(gcell), 256, 0, st>>>(d, q.is3d, label, t.stride, cc);
      k_cc_compress_b<<<grid(gcell), 256, 0, st>>>(d, label, t.stride); }
    HIP_TRY(hipMemcpyAsync(h_cc.data(), cc, sizeof(int) * B, hipMemcpyDeviceToHost, st), "memcpy");
    HIP_TRY(hipStreamSynchronize(st), "sync");
    if (std::all_of(h_cc.begin(), h_cc.begin() + B, [](int c) { return c == 0; })) return PcgResult::ok;
    if (round > 100000) { snprintf(er.msg, er.len, "%s: component labelling did not converge", er.who); return PcgResult::hip_error; }
  }
}

// the items' counts, then their (root, size) rows in scan order: sorted on the device, read once
PcgResult BatchedSolve::read_components() {
  { TFL_TIMED("k_cc", st);
    k_cc_count_b<<<grid(cdiv(n, 256)), 256, 0, st>>>(d, B, label, size_at, roots, t.stride, cc);
    k_cc_table_b<<<grid(kMaxComponents / 256), 256, 0, st>>>(B, roots, size_at, t.stride, cc, comps); }
  HIP_TRY(hipMemcpyAsync(h_cc.data(), cc, sizeof(int) * kPcgCcWords * B, hipMemcpyDeviceToHost, st), "memcpy");
  HIP_TRY(hipStreamSynchronize(st), "sync");
  for (int b = 0; b < B; b++) {
    if (h_cc[2 * B + b] > 0) {   // generic/tfluids.cu:1083-1091 raises for a fluid cell on the border
      snprintf(er.msg, er.len, "solveLinearSystemPCGBatched: Non fluid cell found in a connected component or fluid cell found on the "
               "domain border (%d fluid border cells in batch item %d)", h_cc[2 * B + b], b);
      return PcgResult::bad_flags;
    }
  }
  for (int b = 0; b < B; b++) {
    if (h_cc[B + b] > kMaxComponents) {
      snprintf(er.msg, er.len, "solveLinearSystemPCGBatched: %d fluid components in batch item %d (the solver handles %d)", h_cc[B + b], b,
               kMaxComponents);
      return PcgResult::too_many_components;
    }
    maxc = std::max(maxc, h_cc[B + b]);
  }
  if (!maxc) return PcgResult::ok;
  h_comps.resize((size_t)B * maxc * 2);
  HIP_TRY(hipMemcpy2DAsync(h_comps.data(), sizeof(int) * 2 * maxc, comps, sizeof(int) * 2 * kMaxComponents, sizeof(int) * 2 * maxc, B,
                           hipMemcpyDeviceToHost, st), "memcpy components");
  HIP_TRY(hipStreamSynchronize(st), "sync");
  return PcgResult::ok;
}

// one CG iteration of every item, enqueued: the launches of Solve::iteration, B items each
void BatchedSolve::iteration(bool any_mg) {
  k_pcg_top_b<<<grid(1), 256, 0, st>>>(bt, v, 1);
  if (any_mg) { TFL_TIMED("k_pcg_precond", st); mg_vcycle_batched(st, q.is3d, B, bt, mgd, v.w, v.r, v.partials); }
  TFL_TIMED("k_pcg", st);
  if (any_mg) k_pcg_dot_b<<<grid(kRedBlocks), 256, 0, st>>>(bt, n, v);
  k_pcg_dir_b<<<grid(kRedBlocks), 256, 0, st>>>(bt, n, v);
  if (q.is3d) k_pcg_apply_b<true><<<grid(kRedBlocks), 256, 0, st>>>(bt, d, v, q.flags);
  else k_pcg_apply_b<false><<<grid(kRedBlocks), 256, 0, st>>>(bt, d, v, q.flags);
  k_pcg_update_b<<<grid(kRedBlocks), 256, 0, st>>>(bt, n, v);
}

// chunks of iterations until every item of the round has left its loop: each item's exit test is Solve::run_chunks'
PcgResult BatchedSolve::run_chunks(int c, bool any_mg) {
  const int chunk = any_mg ? 8 : 32;
  for (;;) {
    for (int it = 0; it < chunk; it++) iteration(any_mg);
    { TFL_TIMED("k_pcg", st); k_pcg_top_b<<<grid(1), 256, 0, st>>>(bt, v, 0); }     // fold the last update's residual for the host
    HIP_TRY(hipMemcpy2DAsync(h_state.data(), sizeof(PcgState), bt.S, sizeof(float) * kPcgStateFloats, sizeof(PcgState), B,
                             hipMemcpyDeviceToHost, st), "memcpy state");
    HIP_TRY(hipStreamSynchronize(st), "sync");
    bool all = true;
    for (int b = 0; b < B; b++) {
      if (!active(b, c)) continue;
      const PcgState& hs = h_state[b];
      if (hs.bad) {
        snprintf(er.msg, er.len, "solveLinearSystemPCGBatched: ERROR: r_norm_sq1 is nan! (batch item %d)", b);
        return PcgResult::nan_residual;
      }
      // the loop ends when the NEXT top-of-loop test fails
      all = all && (hs.done || !((float)hs.rr1 > q.tol * q.tol) || hs.iter > q.max_iter);
    }
    if (all) break;
  }
  for (int b = 0; b < B; b++) {
    if (!active(b, c)) continue;
    max_res[b] = std::max(max_res[b], (float)std::sqrt((float)h_state[b].rr1));
    iters[b] += h_state[b].iter;
  }
  return PcgResult::ok;
}

// round c: the c-th system of every item
PcgResult BatchedSolve::round(int c) {
  bool any = false, any_mg = false;
  for (int b = 0; b < B; b++) { any = any || active(b, c); any_mg = any_mg || (active(b, c) && preconditioned(b, c)); }
  if (!any) return PcgResult::ok;
  { TFL_TIMED("k_pcg", st);
    k_pcgb_round<<<cdiv(B, 64), 64, 0, st>>>(bt, B, cc, comps, c, q.precond);
    k_pcg_setup_b<<<grid(kRedBlocks), 256, 0, st>>>(bt, n, v, q.div);
    k_pcg_begin_b<<<grid(1), 256, 0, st>>>(bt, v, q.tol, q.max_iter); }
  if (any_mg) { TFL_TIMED("k_pcg_precond", st); mg_build_levels_batched(st, q.is3d, B, bt, d, mgd, q.flags, label); }
  PCG_TRY(run_chunks(c, any_mg));
  TFL_TIMED("k_pcg", st);
  k_pcg_sum_b<<<grid(kRedBlocks), 256, 0, st>>>(bt, n, v);
  k_pcg_sum_end_b<<<grid(1), 256, 0, st>>>(bt, v);
  k_pcg_write_b<<<grid(kRedBlocks), 256, 0, st>>>(bt, n, v, q.p);
  return PcgResult::ok;
}
