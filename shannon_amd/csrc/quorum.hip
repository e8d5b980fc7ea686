// --quorum: quality-aware read error correction in front of the counting (shannon.py:289-299 turns it on for FASTQ input,
// shannon.py:385-391 puts corrected_reads*.fa in the place of the read files).  Quorum itself is replaced by the rule of DESIGN.md
// 3.11; its two halves are the two calls of this file:
//   shn_quorum_table    can(w) of every high-quality window of every read of the run (count per read, the library's scan, fill),
//                       sorted by the library's radix sort and reduced to (k-mer, count) by run lengths, then the table every
//                       consumer of the library probes (shn_table_from_pairs);
//   shn_quorum_correct  one read per thread, as the abd_* map kernels: anchor, forward walk, backward walk (quorum_dev.h), the
//                       substitutions written into a copy of the read set -- the original stays as it is.
// The high-quality mask is the ingest's (shn_reads_quality_mask, ingest.hip).
#include "record_expand_dev.h"
#include "quorum_dev.h"
#include "runs.h"

int shn_reads_clone(shn_ctx* ctx, const shn_reads* src, shn_reads** out);      // core.hip
int shn_reads_refresh_bad(shn_ctx* ctx, shn_reads* r);

namespace {

constexpr int Q_BLK = 256;

__device__ __forceinline__ uint32_t q_len(const ReadSetView& S, uint64_t r) { return S.len ? S.len[r] : S.fixed_len; }

// HQ windows of every read: a window ends at base j when j and the k - 1 bases before it are all marked.  One mask word per 64 bases.
__global__ __launch_bounds__(Q_BLK) void quorum_count_kernel(ReadSetView S, const uint64_t* __restrict__ hq, int k, uint32_t* __restrict__ cnt) {
  SHN_GRID_FOR(r, S.n) {
    const uint32_t len = q_len(S, r);
    const uint64_t mb = S.word_base(r) >> 1;
    uint32_t run = 0, c = 0;
    for (uint32_t j0 = 0; j0 < len; j0 += 64) {
      const uint64_t m = hq[mb + (j0 >> 6)];
      const uint32_t nb = min(64u, len - j0);
      for (uint32_t j = 0; j < nb; j++) {
        run = ((m >> (63 - j)) & 1) ? run + 1 : 0;
        c += run >= (uint32_t)k ? 1u : 0u;
      }
    }
    cnt[r] = c;
  }
}

// the same walk with the bases: the window and its reverse complement are carried from base to base, two words per 64 bases
__global__ __launch_bounds__(Q_BLK) void quorum_fill_kernel(ReadSetView S, const uint64_t* __restrict__ hq, int k, const uint64_t* __restrict__ off,
                                                            uint64_t* __restrict__ keys) {
  const uint64_t kmask = k == 32 ? ~0ULL : ((1ULL << (2 * k)) - 1);
  SHN_GRID_FOR(r, S.n) {
    const uint32_t len = q_len(S, r);
    const uint64_t wb = S.word_base(r);
    uint64_t at = off[r];
    if (off[r + 1] == at) continue;
    QKmer x{0, 0};
    uint32_t run = 0;
    for (uint32_t j0 = 0; j0 < len; j0 += 64) {
      const uint64_t m = hq[(wb >> 1) + (j0 >> 6)];
      const uint64_t w0 = S.words[wb + (j0 >> 5)], w1 = S.words[wb + (j0 >> 5) + 1];
      const uint32_t nb = min(64u, len - j0);
      for (uint32_t j = 0; j < nb; j++) {
        const uint32_t c = (uint32_t)((j < 32 ? w0 >> (62 - 2 * j) : w1 >> (62 - 2 * (j - 32))) & 3);
        x = q_append(x, c, k, kmask);
        run = ((m >> (63 - j)) & 1) ? run + 1 : 0;
        if (run >= (uint32_t)k) keys[at++] = x.can();
      }
    }
  }
}

// One read per thread.  S: the reads as they are (read only); ow / om: the output set's words and mask, already a copy of S's.
// ctr[5]: reads with an anchor, reads changed, substitutions, stopped directions, window reverts.
// SPANS (shn_quorum_correct_spans): span[2 r], span[2 r + 1] = the [lo, hi) the walks of read r vouch for (rule 6), (0, 0) for a read
// that is too short or has no anchor.  The instantiation without it is the kernel shn_quorum_correct always ran.
template <bool SPANS>
__global__ __launch_bounds__(Q_BLK) void quorum_correct_kernel(ReadSetView S, TabIdx T, const uint32_t* __restrict__ counts, int k, uint32_t A, uint32_t W,
                                                               uint32_t E, uint64_t* __restrict__ ow, uint64_t* __restrict__ om,
                                                               unsigned long long* __restrict__ ctr, uint32_t* __restrict__ span) {
  const uint64_t kmask = k == 32 ? ~0ULL : ((1ULL << (2 * k)) - 1);
  SHN_GRID_FOR(r, S.n) {
    if (SPANS) { span[2 * r] = 0; span[2 * r + 1] = 0; }
    const uint32_t len = q_len(S, r);
    if (len < (uint32_t)k) continue;
    const uint64_t wb = S.word_base(r);
    ReadCursor<true> cur;
    cur.open(S, wb);
    // rule 2: the first window of ACGT only that the table holds A times or more
    QKmer x{0, 0};
    uint32_t run = 0, i0 = 0;
    bool found = false;
    for (uint32_t p = 0; p < len && !found; p++) {
      const uint32_t c = cur.code(p);
      if (c == 4) { run = 0; continue; }
      x = q_append(x, c, k, kmask);
      if (++run < (uint32_t)k) continue;
      const int64_t at = shn_tab_find(T, x.can());
      if (at >= 0 && counts[at] >= A) { found = true; i0 = p + 1 - (uint32_t)k; }
    }
    if (!found) continue;
    auto present = [&](const QKmer& y) { return shn_tab_find(T, y.can()) >= 0; };
    QWalkStats st{0, 0, 0};
    uint64_t* rw = ow + wb;
    uint64_t* rm = om + (wb >> 1);
    const uint32_t ef = q_walk<true>(cur, rw, rm, x, k, kmask, W, E, i0 + (uint32_t)k, len - i0 - (uint32_t)k, present, st);
    const uint32_t eb = q_walk<false>(cur, rw, rm, x, k, kmask, W, E, i0 - 1, i0, present, st);
    if (SPANS) { span[2 * r] = i0 - eb; span[2 * r + 1] = i0 + (uint32_t)k + ef; }
    atomicAdd(&ctr[0], 1ULL);
    if (st.subs) { atomicAdd(&ctr[1], 1ULL); atomicAdd(&ctr[2], (unsigned long long)st.subs); }
    if (st.stops) atomicAdd(&ctr[3], (unsigned long long)st.stops);
    if (st.reverts) atomicAdd(&ctr[4], (unsigned long long)st.reverts);
  }
}

bool mask_belongs(const shn_qmask* m, const shn_reads* r) {
  return m->owner == r && m->n_reads == r->n_reads && m->n_words == r->n_words && m->total_bases == r->total_bases && m->device == r->device;
}

}  // namespace

extern "C" int shn_quorum_table(shn_ctx* ctx, const shn_reads* const* sets, const shn_qmask* const* masks, int n_sets, int k, shn_table** out) {
  if (!ctx || !sets || !masks || !out) return shn_fail(SHN_ERR_ARG, "shn_quorum_table: NULL argument");
  *out = nullptr;
  if (k < 15 || k > 32) return shn_fail(SHN_ERR_ARG, "shn_quorum_table: k outside 15 .. 32");
  if (n_sets < 1 || n_sets > 16) return shn_fail(SHN_ERR_ARG, "shn_quorum_table: 1 .. 16 read sets");
  uint64_t n_reads = 0;
  for (int i = 0; i < n_sets; i++) {
    if (!sets[i] || !masks[i]) return shn_fail(SHN_ERR_ARG, "shn_quorum_table: NULL read set or mask");
    if (!mask_belongs(masks[i], sets[i])) return shn_fail(SHN_ERR_ARG, "shn_quorum_table: mask " + std::to_string(i) + " does not belong to its read set");
    n_reads += sets[i]->n_reads;
  }
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs B(s);
  uint32_t* d_cnt = nullptr; uint64_t* d_off = nullptr;
  HIP_TRY(B.get(&d_cnt, (n_reads + 1) * 4)); HIP_TRY(B.get(&d_off, (n_reads + 2) * 8));
  uint64_t total = 0;
  int rc;
  {
    // bytes: the masks (1 bit per base slot) and 4 B of count per read; then the scan's
    TimerRegion t(ctx, T_QUORUM_COUNT);
    uint64_t r0 = 0, bytes = 0;
    for (int i = 0; i < n_sets; i++) {
      if (sets[i]->n_reads)
        hipLaunchKernelGGL(quorum_count_kernel, dim3(shn_grid(sets[i]->n_reads, Q_BLK)), dim3(Q_BLK), 0, s, view_of(sets[i]), (const uint64_t*)masks[i]->d_hq, k, d_cnt + r0);
      r0 += sets[i]->n_reads;
      bytes += sets[i]->n_words / 2 * 8 + sets[i]->n_reads * 4;
    }
    HIP_TRY(hipGetLastError());
    if ((rc = shn_device_scan_u32(ctx, d_cnt, n_reads, d_off, &total))) return rc;
    t.bytes(bytes + n_reads * 12);
  }
  if (total >= 0xFFFFFFFFULL) return shn_fail(SHN_ERR_OVERFLOW, "shn_quorum_table: 2^32 high-quality windows or more in one call (" + std::to_string(total) + ")");
  uint64_t *d_keys = nullptr, *d_tmp = nullptr;
  HIP_TRY(B.get(&d_keys, (total + 1) * 8)); HIP_TRY(B.get(&d_tmp, (total + 1) * 8));
  if (total) {
    // bytes: words and masks once, 8 B of offset per read, 8 B per window written
    TimerRegion t(ctx, T_QUORUM_COUNT);
    uint64_t r0 = 0, bytes = 0;
    for (int i = 0; i < n_sets; i++) {
      if (sets[i]->n_reads)
        hipLaunchKernelGGL(quorum_fill_kernel, dim3(shn_grid(sets[i]->n_reads, Q_BLK)), dim3(Q_BLK), 0, s, view_of(sets[i]), (const uint64_t*)masks[i]->d_hq, k,
                           (const uint64_t*)(d_off + r0), d_keys);
      r0 += sets[i]->n_reads;
      bytes += sets[i]->n_words * 12 + sets[i]->n_reads * 8;
    }
    HIP_TRY(hipGetLastError());
    t.bytes(bytes + total * 8);
  }
  {
    // bytes: the sort reads and writes every key once per 8-bit pass; heads, scan and run lengths touch 8 + 4 + 8 B per window and
    // 8 + 4 + 4 B per distinct k-mer; the table build reads and writes the pairs once more
    TimerRegion t(ctx, T_QUORUM_TABLE);
    uint64_t* sorted = d_keys;
    if (total && (rc = shn_sort_keys(ctx, d_keys, d_tmp, total, 0, 2 * k, &sorted))) return rc;
    ShnRuns runs;                                 // (no window: no run, nothing launched)
    if ((rc = shn_sorted_runs(ctx, B, sorted, total, 0, SHN_RUNS_KEYS | SHN_RUNS_LEN, &runs))) return rc;
    const uint64_t nu = runs.n_runs;
    t.bytes(total * 16 * (uint64_t)((2 * k + 7) / 8) + total * 20 + nu * 16 + nu * 24);
    if ((rc = shn_table_from_pairs(ctx, runs.keys, runs.len, nu, k, 1, out))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  return SHN_OK;
}

// shn_quorum_correct and shn_quorum_correct_spans: one body, the kernel instantiated with or without the span output
static int quorum_correct_impl(shn_ctx* ctx, const char* who, const shn_reads* reads, const shn_table* table, int k, uint32_t anchor_count, uint32_t window,
                               uint32_t max_subs, shn_reads** out, shn_qspans** spans_out, uint64_t* stats5) {
  const std::string name(who);
  if (!ctx || !reads || !table || !out || !stats5) return shn_fail(SHN_ERR_ARG, name + ": NULL argument");
  *out = nullptr;
  if (spans_out) *spans_out = nullptr;
  if (k < 15 || k > 32) return shn_fail(SHN_ERR_ARG, name + ": k outside 15 .. 32");
  if (table->k != k || !table->canonical) return shn_fail(SHN_ERR_ARG, name + ": the table is not a canonical table of k-mers of this k");
  if (anchor_count == 0) return shn_fail(SHN_ERR_ARG, name + ": anchor_count is 0 (every window would be an anchor)");
  if (max_subs > (uint32_t)QUORUM_MAX_E)
    return shn_fail(SHN_ERR_ARG, name + ": max_subs above " + std::to_string(QUORUM_MAX_E) + ", what a walk keeps in registers for the revert");
  if (table->device != reads->device) return shn_fail(SHN_ERR_ARG, name + ": table and reads on different devices");
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs B(s);
  unsigned long long* d_ctr = nullptr;
  HIP_TRY(B.get(&d_ctr, 5 * 8));
  shn_reads* r = nullptr;
  shn_qspans* sp = nullptr;
  if (spans_out) {
    sp = new shn_qspans();
    sp->ctx = ctx; sp->device = ctx->device; sp->n_reads = reads->n_reads; sp->d_span = nullptr;
    hipError_t e = shn_hip_malloc(&sp->d_span, (reads->n_reads + 1) * 8);
    if (e != hipSuccess) { delete sp; return shn_fail(SHN_ERR_HIP, name + ": " + hipGetErrorString(e)); }
  }
  auto drop = [&]() { if (r) shn_reads_destroy(r); if (sp) shn_qspans_destroy(sp); };
  unsigned long long ctr[5] = {0, 0, 0, 0, 0};
  {
    // bytes: the copy (words and masks read and written), the walk's reads of words and masks, one probed key per base, 4 B of length
    // per read; with spans 8 B more per read
    TimerRegion t(ctx, T_QUORUM_CORRECT);
    int rc = shn_reads_clone(ctx, reads, &r);
    if (rc) { drop(); return rc; }
    hipError_t e = hipMemsetAsync(d_ctr, 0, 5 * 8, s);
    if (e == hipSuccess && reads->n_reads) {
      const dim3 grid(shn_grid(reads->n_reads, Q_BLK)), blk(Q_BLK);
      if (sp)
        hipLaunchKernelGGL(quorum_correct_kernel<true>, grid, blk, 0, s, view_of(reads), shn_tab_idx(table), (const uint32_t*)table->d_counts, k, anchor_count, window,
                           max_subs, r->d_words, r->d_mask, d_ctr, sp->d_span);
      else
        hipLaunchKernelGGL(quorum_correct_kernel<false>, grid, blk, 0, s, view_of(reads), shn_tab_idx(table), (const uint32_t*)table->d_counts, k, anchor_count, window,
                           max_subs, r->d_words, r->d_mask, d_ctr, (uint32_t*)nullptr);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(ctr, d_ctr, 5 * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);              // (ctr is this frame's: the copy ends here)
    if (e != hipSuccess) { drop(); return shn_fail(SHN_ERR_HIP, name + ": " + hipGetErrorString(e)); }
    t.bytes(reads->n_words * 12 * 3 + reads->total_bases * 8 + reads->n_reads * (sp ? 12 : 4));
  }
  int rc = shn_reads_refresh_bad(ctx, r);            // (the N that became bases are counted out)
  if (rc) { drop(); return rc; }
  for (int i = 0; i < 5; i++) stats5[i] = ctr[i];
  *out = r;
  if (spans_out) *spans_out = sp;
  return SHN_OK;
}

extern "C" int shn_quorum_correct(shn_ctx* ctx, const shn_reads* reads, const shn_table* table, int k, uint32_t anchor_count, uint32_t window,
                                  uint32_t max_subs, shn_reads** out, uint64_t* stats5) {
  return quorum_correct_impl(ctx, "shn_quorum_correct", reads, table, k, anchor_count, window, max_subs, out, nullptr, stats5);
}

extern "C" int shn_quorum_correct_spans(shn_ctx* ctx, const shn_reads* reads, const shn_table* table, int k, uint32_t anchor_count, uint32_t window,
                                        uint32_t max_subs, shn_reads** out, shn_qspans** spans_out, uint64_t* stats5) {
  if (!spans_out) return shn_fail(SHN_ERR_ARG, "shn_quorum_correct_spans: NULL argument");
  return quorum_correct_impl(ctx, "shn_quorum_correct_spans", reads, table, k, anchor_count, window, max_subs, out, spans_out, stats5);
}

// ---- tables added up: the pairs of both, every count held at 2^31 - 1, then the sum by key of shn_table_from_pairs
namespace {
constexpr uint32_t Q_COUNT_CAP = 0x7fffffffu;
__global__ __launch_bounds__(Q_BLK) void quorum_concat_kernel(const uint64_t* __restrict__ ka, const uint32_t* __restrict__ ca, uint64_t na,
                                                              const uint64_t* __restrict__ kb, const uint32_t* __restrict__ cb, uint64_t nb,
                                                              uint64_t* __restrict__ keys, uint32_t* __restrict__ cnts) {
  SHN_GRID_FOR(i, na + nb) {
    const bool first = i < na;
    const uint64_t j = first ? i : i - na;
    keys[i] = first ? ka[j] : kb[j];
    cnts[i] = min(first ? ca[j] : cb[j], Q_COUNT_CAP);
  }
}
}  // namespace

extern "C" int shn_quorum_add_tables(shn_ctx* ctx, const shn_table* a, const shn_table* b, shn_table** out) {
  if (!ctx || !a || !b || !out) return shn_fail(SHN_ERR_ARG, "shn_quorum_add_tables: NULL argument");
  *out = nullptr;
  if (a->k != b->k || !a->canonical || !b->canonical) return shn_fail(SHN_ERR_ARG, "shn_quorum_add_tables: two canonical tables of one k");
  if (a->device != b->device) return shn_fail(SHN_ERR_ARG, "shn_quorum_add_tables: tables on different devices");
  const uint64_t n = a->n + b->n;
  if (n >= 0xFFFFFFFFULL) return shn_fail(SHN_ERR_OVERFLOW, "shn_quorum_add_tables: 2^32 pairs or more");
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs B(s);
  uint64_t* d_k = nullptr; uint32_t* d_c = nullptr;
  HIP_TRY(B.get(&d_k, (n + 1) * 8)); HIP_TRY(B.get(&d_c, (n + 1) * 4));
  {
    // bytes: 12 B per pair read and written; the table build reads and writes the pairs once more
    TimerRegion t(ctx, T_QUORUM_TABLE);
    if (n) hipLaunchKernelGGL(quorum_concat_kernel, dim3(shn_grid(n, Q_BLK)), dim3(Q_BLK), 0, s, (const uint64_t*)a->d_keys, (const uint32_t*)a->d_counts, a->n,
                              (const uint64_t*)b->d_keys, (const uint32_t*)b->d_counts, b->n, d_k, d_c);
    HIP_TRY(hipGetLastError());
    t.bytes(n * 24 + n * 24);
    int rc = shn_table_from_pairs(ctx, d_k, d_c, n, a->k, 1, out);
    if (rc) return rc;
  }
  (*out)->total = a->total + b->total;
  HIP_TRY(hipStreamSynchronize(s));
  return SHN_OK;
}
