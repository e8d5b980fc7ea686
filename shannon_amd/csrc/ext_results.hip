// What reads a finished extension (struct shn_ext, ext_state.h): statistics of the walks, the accept filter, the contigs' text
// from the claims, seed keys and k1-mer weights.
#include "ext_state.h"
#include "k1dict.h"

extern "C" uint64_t shn_ext_n_walks(const shn_ext* e) { return e ? e->n_seeds : 0; }
extern "C" int shn_ext_iterations(const shn_ext* e) { return e ? e->iterations : 0; }
extern "C" uint64_t shn_ext_total_steps(const shn_ext* e) { return e ? e->total_steps : 0; }
extern "C" uint64_t shn_ext_wave_steps(const shn_ext* e) { return e ? e->wave_steps : 0; }
extern "C" uint64_t shn_ext_fresh_steps(const shn_ext* e) { return e ? e->fresh_steps : 0; }
extern "C" int shn_ext_dense_rounds(const shn_ext* e) { return e ? e->dense_rounds : 0; }

extern "C" int shn_ext_stats_range(shn_ctx* ctx, const shn_ext* e, uint64_t lo, uint64_t n, uint32_t* n_right, uint32_t* n_left, uint64_t* tot_weight) {
  if (!ctx || !e || (n && (!n_right || !n_left || !tot_weight))) return shn_fail(SHN_ERR_ARG, "shn_ext_stats_range: NULL argument");
  if (lo + n > e->n_seeds) return shn_fail(SHN_ERR_ARG, "shn_ext_stats_range: range outside the walks");
  if (!n) return SHN_OK;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  HIP_TRY(hipMemcpyAsync(n_right, e->d_nr + lo, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(n_left, e->d_nl + lo, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(tot_weight, e->d_totw + lo, n * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return SHN_OK;
}

extern "C" int shn_ext_stats(shn_ctx* ctx, const shn_ext* e, uint32_t* n_right, uint32_t* n_left, uint64_t* tot_weight) {
  if (!ctx || !e) return shn_fail(SHN_ERR_ARG, "shn_ext_stats: NULL argument");
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  if (n_right) HIP_TRY(hipMemcpyAsync(n_right, e->d_nr, e->n_seeds * 4, hipMemcpyDeviceToHost, s));
  if (n_left) HIP_TRY(hipMemcpyAsync(n_left, e->d_nl, e->n_seeds * 4, hipMemcpyDeviceToHost, s));
  if (tot_weight) HIP_TRY(hipMemcpyAsync(tot_weight, e->d_totw, e->n_seeds * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return SHN_OK;
}

// ---- the non-void walks only (a few percent of the seeds), in seed order: what the accept filter needs
__global__ void ext_live_flag_kernel(const uint32_t* __restrict__ nr, const uint32_t* __restrict__ nl, uint64_t ns, uint32_t min_steps,
                                     uint32_t* __restrict__ flag) {
  uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < ns) { const uint32_t a = nr[r]; flag[r] = (a != UNCLAIMED && (uint64_t)a + nl[r] >= min_steps) ? 1u : 0u; }
}
__global__ void ext_live_gather_kernel(const uint32_t* __restrict__ nr, const uint32_t* __restrict__ nl, const uint64_t* __restrict__ totw,
                                       const uint64_t* __restrict__ pos, uint64_t ns, uint32_t* __restrict__ o_rank,
                                       uint32_t* __restrict__ o_nr, uint32_t* __restrict__ o_nl, uint64_t* __restrict__ o_tw) {
  uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ns) return;
  uint64_t p = pos[r];
  if (pos[r + 1] == p) return;                                  // not selected by the flag pass
  o_rank[p] = (uint32_t)r; o_nr[p] = nr[r]; o_nl[p] = nl[r]; o_tw[p] = totw[r];
}

extern "C" int shn_ext_live_stats_min(shn_ctx* ctx, const shn_ext* e, uint32_t min_steps, uint64_t* n_live, uint32_t* rank, uint32_t* n_right,
                                      uint32_t* n_left, uint64_t* tot_weight);
extern "C" int shn_ext_live_stats(shn_ctx* ctx, const shn_ext* e, uint64_t* n_live, uint32_t* rank, uint32_t* n_right, uint32_t* n_left,
                                  uint64_t* tot_weight) {
  return shn_ext_live_stats_min(ctx, e, 0, n_live, rank, n_right, n_left, tot_weight);
}
// ... of the non-void walks of at least min_steps steps (the first clause of the accept filter, extension_correction.py:361, is a
// bound on the contig length k1 + steps: at BASELINE configs[2] it leaves 0.7 M of tens of millions of live walks to download)
extern "C" int shn_ext_live_stats_min(shn_ctx* ctx, const shn_ext* e, uint32_t min_steps, uint64_t* n_live, uint32_t* rank, uint32_t* n_right,
                                      uint32_t* n_left, uint64_t* tot_weight) {
  if (!ctx || !e || !n_live) return shn_fail(SHN_ERR_ARG, "shn_ext_live_stats: NULL argument");
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  const uint64_t ns = e->n_seeds;
  if (!ns) { *n_live = 0; return SHN_OK; }
  void *pf, *pp, *po;
  int rc;
  if ((rc = shn_ws(ctx)[9].get((ns + 1) * 4, &pf)) || (rc = shn_ws(ctx)[11].get((ns + 2) * 8, &pp))) return rc;
  uint32_t* flag = (uint32_t*)pf;
  uint64_t* pos = (uint64_t*)pp;
  hipLaunchKernelGGL(ext_live_flag_kernel, dim3((uint32_t)cdiv(ns, 256)), dim3(256), 0, s, e->d_nr, e->d_nl, ns, min_steps, flag);
  uint64_t total = 0;
  if ((rc = shn_device_scan_u32(ctx, flag, ns, pos, &total))) return rc;
  if (!rank) { *n_live = total; return SHN_OK; }                  // sizing call
  if (*n_live < total) return shn_fail(SHN_ERR_ARG, "shn_ext_live_stats: output arrays too small");
  *n_live = total;
  if (!total) return SHN_OK;
  if ((rc = shn_ws(ctx)[10].get(total * 20 + 64, &po))) return rc;
  uint64_t* o_tw = (uint64_t*)po;
  uint32_t* o_rank = (uint32_t*)(o_tw + total);
  uint32_t* o_nr = o_rank + total;
  uint32_t* o_nl = o_nr + total;
  hipLaunchKernelGGL(ext_live_gather_kernel, dim3((uint32_t)cdiv(ns, 256)), dim3(256), 0, s, e->d_nr, e->d_nl, e->d_totw, pos, ns, o_rank, o_nr,
                     o_nl, o_tw);
  HIP_TRY(hipMemcpyAsync(rank, o_rank, total * 4, hipMemcpyDeviceToHost, s));
  if (n_right) HIP_TRY(hipMemcpyAsync(n_right, o_nr, total * 4, hipMemcpyDeviceToHost, s));
  if (n_left) HIP_TRY(hipMemcpyAsync(n_left, o_nl, total * 4, hipMemcpyDeviceToHost, s));
  if (tot_weight) HIP_TRY(hipMemcpyAsync(tot_weight, o_tw, total * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  return SHN_OK;
}

// ---- the accept filter itself (extension_correction.py:361: len >= min_length and len * avg_weight ** 0.25 >= threshold) over the
// non-void walks, in seed order: class 1 = passes for sure, 2 = within 1e-9 (relative) of the threshold -- the caller decides those
// few with the reference's own arithmetic (math.pow); two square roots here stand for the fourth root, a few ulp from pow.
__global__ void ext_accept_flag_kernel(const uint32_t* __restrict__ nr, const uint32_t* __restrict__ nl, const uint64_t* __restrict__ totw, uint64_t ns,
                                       int k, uint32_t min_length, double thr, uint32_t* __restrict__ flag) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ns) return;
  const uint32_t a = nr[r];
  uint32_t f = 0;
  if (a != UNCLAIMED) {
    const uint64_t steps = (uint64_t)a + nl[r], len = steps + (uint64_t)k;
    if (len >= min_length) {
      const double avg = (double)totw[r] / (double)(steps + 1);
      const double lhs = (double)len * sqrt(sqrt(avg));
      f = lhs >= thr * (1.0 - 1e-9) ? 1u : 0u;
    }
  }
  flag[r] = f;
}
__global__ void ext_accept_gather_kernel(const uint32_t* __restrict__ nr, const uint32_t* __restrict__ nl, const uint64_t* __restrict__ totw,
                                         const uint64_t* __restrict__ pos, uint64_t ns, int k, double thr, uint32_t* __restrict__ o_rank,
                                         uint32_t* __restrict__ o_steps, uint64_t* __restrict__ o_tw, uint8_t* __restrict__ o_cls) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ns) return;
  const uint64_t p = pos[r];
  if (pos[r + 1] == p) return;
  const uint64_t steps = (uint64_t)nr[r] + nl[r];
  const double lhs = (double)(steps + (uint64_t)k) * sqrt(sqrt((double)totw[r] / (double)(steps + 1)));
  o_rank[p] = (uint32_t)r; o_steps[p] = (uint32_t)steps; o_tw[p] = totw[r];
  o_cls[p] = lhs >= thr * (1.0 + 1e-9) ? 1 : 2;
}
// n_out: in = room of the output arrays (0 with NULL arrays: a sizing call), out = candidates; rank / steps (= n_right + n_left) /
// tot_weight / cls per candidate, in seed order
extern "C" int shn_ext_accept(shn_ctx* ctx, const shn_ext* e, uint32_t min_length, double threshold, uint64_t* n_out, uint32_t* rank, uint32_t* steps,
                              uint64_t* tot_weight, uint8_t* cls) {
  if (!ctx || !e || !n_out) return shn_fail(SHN_ERR_ARG, "shn_ext_accept: NULL argument");
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  const uint64_t ns = e->n_seeds;
  if (!ns) { *n_out = 0; return SHN_OK; }
  void *pf, *pp, *po;
  int rc;
  if ((rc = shn_ws(ctx)[9].get((ns + 1) * 4, &pf)) || (rc = shn_ws(ctx)[11].get((ns + 2) * 8, &pp))) return rc;
  uint32_t* flag = (uint32_t*)pf;
  uint64_t* pos = (uint64_t*)pp;
  hipLaunchKernelGGL(ext_accept_flag_kernel, dim3((uint32_t)cdiv(ns, 256)), dim3(256), 0, s, e->d_nr, e->d_nl, e->d_totw, ns, e->k, min_length, threshold, flag);
  uint64_t total = 0;
  if ((rc = shn_device_scan_u32(ctx, flag, ns, pos, &total))) return rc;
  if (!rank) { *n_out = total; return SHN_OK; }
  if (*n_out < total || !steps || !tot_weight || !cls) return shn_fail(SHN_ERR_ARG, "shn_ext_accept: output arrays too small");
  *n_out = total;
  if (!total) return SHN_OK;
  if ((rc = shn_ws(ctx)[10].get(total * 17 + 64, &po))) return rc;
  uint64_t* o_tw = (uint64_t*)po;
  uint32_t* o_rank = (uint32_t*)(o_tw + total);
  uint32_t* o_steps = o_rank + total;
  uint8_t* o_cls = (uint8_t*)(o_steps + total);
  hipLaunchKernelGGL(ext_accept_gather_kernel, dim3((uint32_t)cdiv(ns, 256)), dim3(256), 0, s, e->d_nr, e->d_nl, e->d_totw, pos, ns, e->k, threshold, o_rank,
                     o_steps, o_tw, o_cls);
  HIP_TRY(hipMemcpyAsync(rank, o_rank, total * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(steps, o_steps, total * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(tot_weight, o_tw, total * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(cls, o_cls, total, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  return SHN_OK;
}

// seed string (oriented k1-mer key) and seed weight of the given walks: the global order of the walks is
// (weight descending, key ascending), which is what merges the candidates of several shards
__global__ void ext_seed_info_kernel(const uint32_t* __restrict__ ranks, uint64_t n, const uint32_t* __restrict__ order,
                                     const uint64_t* __restrict__ tkeys, const uint32_t* __restrict__ weight, int k,
                                     uint64_t* __restrict__ keys, uint32_t* __restrict__ w) {
  uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  uint32_t o = order[ranks[j]];
  keys[j] = oriented_string(tkeys, o, k);
  w[j] = weight[o >> 1];
}
extern "C" int shn_ext_seed_info(shn_ctx* ctx, const shn_ext* e, const uint32_t* ranks, uint64_t n, uint64_t* keys, uint32_t* weights) {
  if (!ctx || !e || (n && (!ranks || !keys || !weights))) return shn_fail(SHN_ERR_ARG, "shn_ext_seed_info: NULL argument");
  if (!n) return SHN_OK;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  for (uint64_t j = 0; j < n; j++) if (ranks[j] >= e->n_seeds) return shn_fail(SHN_ERR_ARG, "shn_ext_seed_info: rank out of range");
  uint32_t *dr, *dw; uint64_t* dk;
  HIP_TRY(shn_dev_malloc(&dr, n * 4)); HIP_TRY(shn_dev_malloc(&dw, n * 4)); HIP_TRY(shn_dev_malloc(&dk, n * 8));
  HIP_TRY(hipMemcpyAsync(dr, ranks, n * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(ext_seed_info_kernel, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, s, dr, n, e->d_order, e->table->d_keys, e->d_weight, e->k, dk, dw);
  HIP_TRY(hipMemcpyAsync(keys, dk, n * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(weights, dw, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  shn_dev_free(dr); shn_dev_free(dw); shn_dev_free(dk);
  return SHN_OK;
}

// Contig bases straight from the converged claims: every oriented k1-mer knows its walk and its step index
// (claim = rank << 32 | pos; pos 0 = seed, 1..nR right steps, nR+1..nR+nL left steps), so the contig of a
// selected walk is a scatter -- no walking.  (extension_correction.py:223-245: a right step appends the last
// base of the new k1-mer, a left step prepends its first base.)
__global__ void ext_select_kernel(const uint32_t* __restrict__ ranks, uint64_t n_sel, int32_t* __restrict__ sel_of_rank,
                                  unsigned long long* __restrict__ n_twice) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_sel) return;
  if (atomicCAS((int*)&sel_of_rank[ranks[t]], -1, (int)t) != -1) atomicAdd(n_twice, 1ULL);
}

__global__ void ext_emit_claims_kernel(const u64* __restrict__ claim, uint64_t n2, const int32_t* __restrict__ sel_of_rank, uint64_t ns,
                                       const uint32_t* __restrict__ nr_a, const uint32_t* __restrict__ nl_a,
                                       const uint64_t* __restrict__ tkeys, int k, const uint64_t* __restrict__ out_off,
                                       uint8_t* __restrict__ out_bases, unsigned long long* __restrict__ counters) {
  uint32_t n_wrote = 0, n_stray = 0, n_misfit = 0;
  for (uint64_t y = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; y < n2; y += (uint64_t)gridDim.x * blockDim.x) {
    const u64 c = claim[y];
    const uint32_t r = RANK(c), pos = POS(c);
    if (r == UNCLAIMED || r >= ns) continue;
    const int32_t t = sel_of_rank[r];
    if (t < 0) continue;
    const uint32_t nr = nr_a[r], nl = nl_a[r];
    if (nr == UNCLAIMED || pos > nr + nl) { n_stray++; continue; }    // claim of a void walk / beyond its recorded path
    // the caller's room for this contig is not the contig's length: nothing of it is written (a shorter room would be overrun)
    if (out_off[t + 1] - out_off[t] != (uint64_t)nr + nl + (uint64_t)k) { n_misfit++; continue; }
    uint8_t* dst = out_bases + out_off[t];
    const uint64_t str = oriented_string(tkeys, (uint32_t)y, k);
    if (pos == 0) for (int j = 0; j < k; j++) dst[nl + j] = "ACGT"[(str >> (2 * (k - 1 - j))) & 3];
    else if (pos <= nr) dst[nl + k + (pos - 1)] = "ACGT"[str & 3];
    else dst[nl - 1 - (pos - nr - 1)] = "ACGT"[(str >> (2 * (k - 1))) & 3];
    n_wrote++;
  }
  __shared__ unsigned long long blk[3];
  if (threadIdx.x < 3) blk[threadIdx.x] = 0;
  __syncthreads();
  if (n_wrote) atomicAdd(&blk[0], (unsigned long long)n_wrote);
  if (n_stray) atomicAdd(&blk[1], (unsigned long long)n_stray);
  if (n_misfit) atomicAdd(&blk[2], (unsigned long long)n_misfit);
  __syncthreads();
  // counters: 0 written, 1 stray, 2 selected twice (ext_select_kernel), 3 claims of walks whose room does not fit
  if (threadIdx.x < 2 && blk[threadIdx.x]) atomicAdd(&counters[threadIdx.x], blk[threadIdx.x]);
  if (threadIdx.x == 2 && blk[2]) atomicAdd(&counters[3], blk[2]);
}

// bases_out: the contigs' text on the host; dev_out (instead): the text stays on the device (total + 64 bytes, the tail zeroed; the
// caller frees it with shn_dev_free) -- the GPU contig stage reads it there
static int ext_emit_impl(shn_ctx* ctx, const shn_ext* e, const uint32_t* ranks, uint64_t n_sel, const uint64_t* offsets, uint8_t* bases_out, uint8_t** dev_out) {
  if (!ctx || !e || (n_sel && (!ranks || !offsets || (!bases_out && !dev_out)))) return shn_fail(SHN_ERR_ARG, "shn_ext_emit: NULL argument");
  if (dev_out) *dev_out = nullptr;
  if (!n_sel) return SHN_OK;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  TimerRegion treg(ctx, T_EXTEND);
  const uint64_t total = offsets[n_sel], ns = e->n_seeds;
  // rank -> index in the selection (built on the device: the map has one entry per walk, the selection is small);
  // expected number of k1-mers of the selected walks
  for (uint64_t t = 0; t < n_sel; t++)
    if (ranks[t] >= ns) return shn_fail(SHN_ERR_ARG, "shn_ext_emit: rank out of range");
  unsigned long long expect = 0;
  for (uint64_t t = 0; t < n_sel; t++) {
    uint64_t len = offsets[t + 1] - offsets[t];
    if (len < (uint64_t)e->k) return shn_fail(SHN_ERR_ARG, "shn_ext_emit: offsets do not fit the walk lengths");
    expect += len - e->k + 1;
  }
  int32_t* d_sel; uint64_t* d_off; uint8_t* d_out; unsigned long long* d_cnt; uint32_t* d_ranks;
  HIP_TRY(shn_dev_malloc(&d_sel, (ns + 1) * 4));
  HIP_TRY(shn_dev_malloc(&d_off, (n_sel + 1) * 8));
  HIP_TRY(shn_dev_malloc(&d_out, total + 64));
  HIP_TRY(shn_dev_malloc(&d_cnt, 32));
  HIP_TRY(shn_dev_malloc(&d_ranks, (n_sel + 1) * 4));
  HIP_TRY(hipMemsetAsync(d_sel, 0xFF, (ns + 1) * 4, s));                    // -1: not selected
  HIP_TRY(hipMemcpyAsync(d_ranks, ranks, n_sel * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_off, offsets, (n_sel + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(d_cnt, 0, 32, s));
  hipLaunchKernelGGL(ext_select_kernel, dim3((uint32_t)cdiv(n_sel, 256)), dim3(256), 0, s, d_ranks, n_sel, d_sel, d_cnt + 2);
  HIP_TRY(hipMemsetAsync(d_out, 0, total + 64, s));
  {
    TimerRegion tk(ctx, T_EXT_EMIT);
    hipLaunchKernelGGL(ext_emit_claims_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(2 * e->n, 256), 4096)), dim3(256), 0, s, e->d_claim, 2 * e->n, d_sel, ns,
                       e->d_nr, e->d_nl, e->table->d_keys, e->k, d_off, d_out, d_cnt);
  }
  unsigned long long cnt[4] = {0, 0, 0, 0};
  if (bases_out) HIP_TRY(hipMemcpyAsync(bases_out, d_out, total, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(cnt, d_cnt, 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  shn_dev_free(d_sel); shn_dev_free(d_off); shn_dev_free(d_cnt); shn_dev_free(d_ranks);
  struct FreeOut { uint8_t* p; ~FreeOut() { if (p) shn_dev_free(p); } } free_out{d_out};
  HIP_TRY(hipGetLastError());
  if (cnt[2]) return shn_fail(SHN_ERR_ARG, "shn_ext_emit: a walk is selected twice");
  if (cnt[3]) return shn_fail(SHN_ERR_ARG, "shn_ext_emit: offsets do not fit the walk lengths");
  // every base of every selected contig must have been written exactly once
  if (cnt[1] || cnt[0] != expect)
    return shn_fail(SHN_ERR_INTERNAL, "shn_ext_emit: claims do not match the recorded walks (k1-mers written " + std::to_string(cnt[0]) +
                    ", expected " + std::to_string(expect) + ", stray claims " + std::to_string(cnt[1]) + ")");
  if (dev_out) { *dev_out = d_out; free_out.p = nullptr; }
  return SHN_OK;
}
extern "C" int shn_ext_emit(shn_ctx* ctx, const shn_ext* e, const uint32_t* ranks, uint64_t n_sel, const uint64_t* offsets,
                            uint8_t* bases_out) {
  if (n_sel && !bases_out) return shn_fail(SHN_ERR_ARG, "shn_ext_emit: NULL argument");
  return ext_emit_impl(ctx, e, ranks, n_sel, offsets, bases_out, nullptr);
}
// the same with the text left on the device (shn_devtext: what shn_contig_stage_device reads; shn_devtext_segments fetches pieces)
extern "C" int shn_ext_emit_device(shn_ctx* ctx, const shn_ext* e, const uint32_t* ranks, uint64_t n_sel, const uint64_t* offsets, shn_devtext** out) {
  if (!out) return shn_fail(SHN_ERR_ARG, "shn_ext_emit_device: NULL argument");
  *out = nullptr;
  uint8_t* d = nullptr;
  int rc = ext_emit_impl(ctx, e, ranks, n_sel, offsets, nullptr, &d);
  if (rc) return rc;
  shn_devtext* t = new shn_devtext();
  t->ctx = ctx; t->d = d; t->n = n_sel ? offsets[n_sel] : 0;
  *out = t;
  return SHN_OK;
}

// weights of arbitrary k1-mer strings in the doubled input (for the `allowed` dict, :404-408)
__global__ void ext_weight_lookup_kernel(const TabIdx T,
                                         const uint32_t* __restrict__ weight, const uint8_t* __restrict__ flags, int k, int canonical,
                                         const uint64_t* __restrict__ q, uint64_t nq, uint32_t* __restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  uint64_t key = q[i];
  if (canonical) { uint64_t rc = shn_revcomp(key, k); key = rc < key ? rc : key; }
  int64_t j = shn_tab_find(T, key);
  out[i] = (j >= 0 && !(flags[j] & 2)) ? weight[j] : 0;
}

extern "C" int shn_ext_weights(shn_ctx* ctx, const shn_ext* e, const uint64_t* keys, uint64_t n, uint32_t* weights) {
  if (!ctx || !e || (n && (!keys || !weights))) return shn_fail(SHN_ERR_ARG, "shn_ext_weights: NULL argument");
  if (e->owned_table) return shn_fail(SHN_ERR_ARG, "shn_ext_weights: not available on a component shard (it holds only this rank's k1-mers)");
  if (!n) return SHN_OK;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  uint64_t* dq; uint32_t* dw;
  HIP_TRY(shn_dev_malloc(&dq, n * 8));
  HIP_TRY(shn_dev_malloc(&dw, n * 4));
  HIP_TRY(hipMemcpyAsync(dq, keys, n * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(ext_weight_lookup_kernel, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, s, shn_tab_idx(e->table),
                     e->d_weight, e->d_flags, e->k, e->table->canonical, dq, n, dw);
  HIP_TRY(hipMemcpyAsync(weights, dw, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  shn_dev_free(dq); shn_dev_free(dw);
  return SHN_OK;
}
