// correct --trim (rules 6 and 7): sub-reads of a resident read set as a new resident read set.
//   shn_qspans_*     the span [lo, hi) of every read, from the walks (shn_quorum_correct_spans, quorum.hip) or from the host;
//   shn_qspans_keep  rule 7: one flag per read (per pair), and the five counters of the trimming;
//   shn_reads_slice  flags -> the library's scan twice (output index of a kept read, word offset of its sub-read) -> one kernel that
//                    places lengths and offsets -> the copy: one thread per 64 bases of OUTPUT (two words of bases, one word of the
//                    mask of bases outside ACGT -- the unit pack_kernel writes), its read found by the offset search of runs.h.  A
//                    thread assembles each word from two source words, shifted by 2 (lo & 31) bits, and the mask word from two
//                    source mask words, shifted by lo & 63: 24 bytes stored side by side by neighbouring threads, whatever the
//                    reads' lengths are.
// The source is only read.  The output has the layout of shn_reads_create: every read on an even word boundary, 2 cdiv(max(len, 1),
// 64) words, zero bits behind its last base; shn_reads_refresh_bad fills d_bad / n_invalid.
#include <string.h>
#include "record_expand_dev.h"
#include "runs.h"

int shn_reads_refresh_bad(shn_ctx* ctx, shn_reads* r);      // core.hip

namespace {

constexpr int S_BLK = 256;

__device__ __forceinline__ uint32_t s_len(const ReadSetView& S, uint64_t r) { return S.len ? S.len[r] : S.fixed_len; }
// the span of read r held inside the read: lo <= hi <= len, whatever the array says
__device__ __forceinline__ void s_span(const uint32_t* __restrict__ span, uint64_t r, uint32_t len, uint32_t& lo, uint32_t& hi) {
  hi = min(span[2 * r + 1], len);
  lo = min(span[2 * r], hi);
}

// rule 7.  ctr[5]: reads kept, kept reads trimmed, bases cut from kept reads, reads whose own span is below M, pairs dropped
__global__ __launch_bounds__(S_BLK) void keep_kernel(ReadSetView A, const uint32_t* __restrict__ sa, ReadSetView B, const uint32_t* __restrict__ sb, int paired,
                                                     uint32_t M, uint32_t* __restrict__ keep, unsigned long long* __restrict__ ctr) {
  SHN_GRID_FOR(r, A.n) {
    const uint32_t la = s_len(A, r);
    uint32_t lo, hi;
    s_span(sa, r, la, lo, hi);
    const uint32_t na = hi - lo;
    uint32_t lb = 0, nb = M;
    if (paired) {
      lb = s_len(B, r);
      s_span(sb, r, lb, lo, hi);
      nb = hi - lo;
    }
    const bool ka = na >= M, kb = nb >= M, both = ka && kb;
    keep[r] = both ? 1u : 0u;
    const unsigned long long below = (ka ? 0u : 1u) + (kb ? 0u : 1u);
    if (below) atomicAdd(&ctr[3], below);
    if (both) {
      atomicAdd(&ctr[0], paired ? 2ULL : 1ULL);
      const unsigned long long cut = (unsigned long long)(la - na) + (paired ? lb - nb : 0u);
      const unsigned long long trimmed = (na < la ? 1u : 0u) + ((paired && nb < lb) ? 1u : 0u);
      if (trimmed) { atomicAdd(&ctr[1], trimmed); atomicAdd(&ctr[2], cut); }
    } else if (paired) atomicAdd(&ctr[4], 1ULL);
  }
}

// per read of the source: is it kept (flag), and the words its sub-read takes (0 for a read that is not kept)
__global__ __launch_bounds__(S_BLK) void slice_sizes_kernel(ReadSetView S, const uint32_t* __restrict__ span, const uint32_t* __restrict__ keep,
                                                            uint32_t* __restrict__ flag, uint32_t* __restrict__ nw) {
  SHN_GRID_FOR(r, S.n) {
    const bool k = keep ? keep[r] != 0 : true;
    uint32_t lo, hi;
    s_span(span, r, s_len(S, r), lo, hi);
    const uint32_t n = hi - lo;
    flag[r] = k ? 1u : 0u;
    nw[r] = k ? 2 * ((max(n, 1u) + 63) / 64) : 0u;
  }
}

// kept read r becomes read j = pos[r] of the output: its length, its word offset, and where it comes from.  tot[0]: bases of the
// output, tot[1]: its longest read
__global__ __launch_bounds__(S_BLK) void slice_place_kernel(ReadSetView S, const uint32_t* __restrict__ span, const uint32_t* __restrict__ flag,
                                                            const uint64_t* __restrict__ pos, const uint64_t* __restrict__ wpos, uint64_t n_out,
                                                            uint64_t n_words_out, uint64_t* __restrict__ woff, uint32_t* __restrict__ len,
                                                            uint32_t* __restrict__ src, unsigned long long* __restrict__ tot) {
  SHN_GRID_FOR(r, S.n) {
    if (r == 0) woff[n_out] = n_words_out;
    if (!flag[r]) continue;
    uint32_t lo, hi;
    s_span(span, r, s_len(S, r), lo, hi);
    const uint64_t j = pos[r];
    woff[j] = wpos[r];
    len[j] = hi - lo;
    src[j] = (uint32_t)r;
    atomicAdd(&tot[0], (unsigned long long)(hi - lo));
    atomicMax(&tot[1], (unsigned long long)(hi - lo));
  }
}

// 64 bits of a bit string that starts `sh` bits into word a and goes on in word b
__device__ __forceinline__ uint64_t s_funnel(uint64_t a, uint64_t b, uint32_t sh) { return sh ? (a << sh) | (b >> (64 - sh)) : a; }
// the first nb (0 .. 32) bases of a word kept, the rest zero
__device__ __forceinline__ uint64_t s_head2(uint64_t v, uint32_t nb) { return nb >= 32 ? v : nb ? v & ~(~0ULL >> (2 * nb)) : 0; }
__device__ __forceinline__ uint64_t s_head1(uint64_t v, uint32_t nb) { return nb >= 64 ? v : nb ? v & ~(~0ULL >> nb) : 0; }

// One thread per 64 bases of output: group g holds bases [b0, b0 + 64) of output read j, which are bases lo + b0 .. of source read
// src[j].  A source word or mask word is loaded only where a base of the sub-read lies in it, so nothing beyond the source read's own
// words is touched but the word right behind them (the next read's first, or the two spare words every set ends with).
__global__ __launch_bounds__(S_BLK) void slice_copy_kernel(ReadSetView S, const uint32_t* __restrict__ span, const uint64_t* __restrict__ woff,
                                                           const uint32_t* __restrict__ len, const uint32_t* __restrict__ src, uint64_t n_out,
                                                           uint64_t n_groups, uint64_t* __restrict__ ow, uint64_t* __restrict__ om) {
  SHN_GRID_FOR(g, n_groups) {
    const uint64_t j = shn_segment_of(woff, n_out, 2 * g);
    const uint32_t b0 = (uint32_t)(2 * g - woff[j]) * 32;
    const uint32_t n = len[j];
    const uint64_t r = src[j];
    uint64_t w0 = 0, w1 = 0, m = 0;
    if (b0 < n) {
      const uint32_t left = n - b0;
      const uint32_t lo = min(span[2 * r], s_len(S, r));          // (as s_span: n = hi - lo was made from the same numbers)
      const uint64_t wb = S.word_base(r);
      const uint32_t p = lo + b0;
      const uint64_t* w = S.words + wb + (p >> 5);
      const uint32_t sh = 2 * (p & 31);
      const uint64_t a = w[0], b = w[1];
      w0 = s_head2(s_funnel(a, b, sh), left);
      if (left > 32) w1 = s_head2(s_funnel(b, w[2], sh), left - 32);
      if (S.mask) {
        const uint64_t* q = S.mask + (wb >> 1) + (p >> 6);
        m = s_head1(s_funnel(q[0], q[1], p & 63), left);
      }
    }
    ow[2 * g] = w0;
    ow[2 * g + 1] = w1;
    om[g] = m;
  }
}

}  // namespace

extern "C" int shn_qspans_create(shn_ctx* ctx, const uint32_t* lo_hi, uint64_t n_reads, shn_qspans** out) {
  if (!ctx || !out || (!lo_hi && n_reads)) return shn_fail(SHN_ERR_ARG, "shn_qspans_create: NULL argument");
  *out = nullptr;
  for (uint64_t r = 0; r < n_reads; r++)
    if (lo_hi[2 * r] > lo_hi[2 * r + 1]) return shn_fail(SHN_ERR_ARG, "shn_qspans_create: read " + std::to_string(r) + " has lo > hi");
  SHN_ENTER(ctx);
  shn_qspans* sp = new shn_qspans();
  sp->ctx = ctx; sp->device = ctx->device; sp->n_reads = n_reads; sp->d_span = nullptr;
  sp->host.assign(lo_hi, lo_hi + 2 * n_reads);
  hipError_t e = shn_hip_malloc(&sp->d_span, (n_reads + 1) * 8);
  if (e == hipSuccess && n_reads) e = hipMemcpyAsync(sp->d_span, sp->host.data(), n_reads * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { shn_qspans_destroy(sp); return shn_fail(SHN_ERR_HIP, std::string("shn_qspans_create: ") + hipGetErrorString(e)); }
  *out = sp;
  return SHN_OK;
}
extern "C" void shn_qspans_destroy(shn_qspans* s) {
  if (!s) return;
  hipSetDevice(s->device);
  if (s->d_span) hipFree(s->d_span);
  delete s;
}
extern "C" uint64_t shn_qspans_count(const shn_qspans* s) { return s ? s->n_reads : 0; }
extern "C" int shn_qspans_download(shn_ctx* ctx, const shn_qspans* s, uint32_t* lo_hi_out) {
  if (!ctx || !s || (!lo_hi_out && s->n_reads)) return shn_fail(SHN_ERR_ARG, "shn_qspans_download: NULL argument");
  SHN_ENTER(ctx);
  if (s->n_reads) HIP_TRY(hipMemcpyAsync(lo_hi_out, s->d_span, s->n_reads * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return SHN_OK;
}

extern "C" void shn_qkeep_destroy(shn_qkeep* k) {
  if (!k) return;
  hipSetDevice(k->device);
  if (k->d_keep) hipFree(k->d_keep);
  delete k;
}
extern "C" uint64_t shn_qkeep_count(const shn_qkeep* k) { return k ? k->n_kept : 0; }

extern "C" int shn_qspans_keep(shn_ctx* ctx, const shn_reads* reads_a, const shn_qspans* spans_a, const shn_reads* reads_b, const shn_qspans* spans_b,
                               uint32_t min_len, shn_qkeep** out, uint64_t* stats5) {
  if (!ctx || !reads_a || !spans_a || !out || !stats5 || (reads_b != nullptr) != (spans_b != nullptr)) return shn_fail(SHN_ERR_ARG, "shn_qspans_keep: NULL argument");
  *out = nullptr;
  if (min_len == 0) return shn_fail(SHN_ERR_ARG, "shn_qspans_keep: min_len is 0");
  if (spans_a->n_reads != reads_a->n_reads || (reads_b && spans_b->n_reads != reads_b->n_reads))
    return shn_fail(SHN_ERR_ARG, "shn_qspans_keep: spans that are not of their set's read count");
  if (reads_b && reads_b->n_reads != reads_a->n_reads)
    return shn_fail(SHN_ERR_ARG, "shn_qspans_keep: " + std::to_string(reads_a->n_reads) + " reads and " + std::to_string(reads_b->n_reads) + " mates");
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  const uint64_t n = reads_a->n_reads;
  ShnDevBufs B(s);
  unsigned long long* d_ctr = nullptr;
  HIP_TRY(B.get(&d_ctr, 5 * 8));
  shn_qkeep* kp = new shn_qkeep();
  kp->ctx = ctx; kp->device = ctx->device; kp->n_reads = n; kp->n_kept = 0; kp->d_keep = nullptr;
  unsigned long long ctr[5] = {0, 0, 0, 0, 0};
  hipError_t e = shn_hip_malloc(&kp->d_keep, (n + 1) * 4);
  {
    // bytes: 8 B of span and 4 B of length per read of either set, 4 B of flag per read
    TimerRegion t(ctx, T_QUORUM_TRIM);
    if (e == hipSuccess) e = hipMemsetAsync(d_ctr, 0, 5 * 8, s);
    if (e == hipSuccess && n) {
      hipLaunchKernelGGL(keep_kernel, dim3(shn_grid(n, S_BLK)), dim3(S_BLK), 0, s, view_of(reads_a), (const uint32_t*)spans_a->d_span,
                         reads_b ? view_of(reads_b) : view_of(reads_a), (const uint32_t*)(spans_b ? spans_b->d_span : spans_a->d_span), reads_b ? 1 : 0, min_len,
                         kp->d_keep, d_ctr);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(ctr, d_ctr, 5 * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    t.bytes(n * (reads_b ? 24 : 12) + n * 4);
  }
  if (e != hipSuccess) { shn_qkeep_destroy(kp); return shn_fail(SHN_ERR_HIP, std::string("shn_qspans_keep: ") + hipGetErrorString(e)); }
  for (int i = 0; i < 5; i++) stats5[i] = ctr[i];
  kp->n_kept = reads_b ? ctr[0] / 2 : ctr[0];
  *out = kp;
  return SHN_OK;
}

extern "C" int shn_reads_slice(shn_ctx* ctx, const shn_reads* src, const shn_qspans* spans, const shn_qkeep* keep, shn_reads** out) {
  if (!ctx || !src || !spans || !out) return shn_fail(SHN_ERR_ARG, "shn_reads_slice: NULL argument");
  *out = nullptr;
  const uint64_t n = src->n_reads;
  if (spans->n_reads != n) return shn_fail(SHN_ERR_ARG, "shn_reads_slice: spans of " + std::to_string(spans->n_reads) + " reads, a set of " + std::to_string(n));
  if (keep && keep->n_reads != n) return shn_fail(SHN_ERR_ARG, "shn_reads_slice: keep flags of " + std::to_string(keep->n_reads) + " reads, a set of " + std::to_string(n));
  if (n >= 0xFFFFFFFFULL) return shn_fail(SHN_ERR_OVERFLOW, "shn_reads_slice: 2^32 reads or more");
  if (spans->device != src->device || (keep && keep->device != src->device)) return shn_fail(SHN_ERR_ARG, "shn_reads_slice: spans and reads on different devices");
  for (uint64_t r = 0; r < (uint64_t)spans->host.size() / 2; r++) {          // (spans from the host: what the host can know)
    if (spans->host[2 * r] > spans->host[2 * r + 1]) return shn_fail(SHN_ERR_ARG, "shn_reads_slice: read " + std::to_string(r) + " has lo > hi");
    if (spans->host[2 * r + 1] > src->max_len)
      return shn_fail(SHN_ERR_ARG, "shn_reads_slice: read " + std::to_string(r) + " has hi " + std::to_string(spans->host[2 * r + 1]) + " beyond the reads' length " +
                                       std::to_string(src->max_len));
  }
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs B(s);
  uint32_t *d_flag = nullptr, *d_nw = nullptr, *d_src = nullptr;
  uint64_t *d_pos = nullptr, *d_wpos = nullptr;
  unsigned long long* d_tot = nullptr;
  HIP_TRY(B.get(&d_flag, (n + 1) * 4)); HIP_TRY(B.get(&d_nw, (n + 1) * 4));
  HIP_TRY(B.get(&d_pos, (n + 2) * 8)); HIP_TRY(B.get(&d_wpos, (n + 2) * 8));
  HIP_TRY(B.get(&d_tot, 16));
  const ReadSetView S = view_of(src);
  const uint32_t* d_span = spans->d_span;
  uint64_t n_out = 0, n_words = 0;
  TimerRegion t(ctx, T_QUORUM_TRIM);
  if (n) {
    hipLaunchKernelGGL(slice_sizes_kernel, dim3(shn_grid(n, S_BLK)), dim3(S_BLK), 0, s, S, d_span, (const uint32_t*)(keep ? keep->d_keep : nullptr), d_flag, d_nw);
    HIP_TRY(hipGetLastError());
    int rc;
    if ((rc = shn_device_scan_u32(ctx, d_flag, n, d_pos, &n_out))) return rc;
    if ((rc = shn_device_scan_u32(ctx, d_nw, n, d_wpos, &n_words))) return rc;
  }
  shn_reads* r = new shn_reads();
  memset(r, 0, sizeof(*r));
  r->ctx = ctx; r->device = ctx->device; r->n_reads = n_out; r->n_words = n_words;
  auto fail = [&](hipError_t e) { shn_reads_destroy(r); return shn_fail(SHN_ERR_HIP, std::string("shn_reads_slice: ") + hipGetErrorString(e)); };
  hipError_t e;
  if ((e = shn_hip_malloc(&r->d_words, (n_words + 2) * 8)) != hipSuccess) return fail(e);
  if ((e = shn_hip_malloc(&r->d_mask, (n_words / 2 + 2) * 8)) != hipSuccess) return fail(e);
  if ((e = shn_hip_malloc(&r->d_woff, (n_out + 1) * 8)) != hipSuccess) return fail(e);
  if ((e = shn_hip_malloc(&r->d_len, (n_out + 1) * 4)) != hipSuccess) return fail(e);
  if ((e = hipMemsetAsync(r->d_words + n_words, 0, 16, s)) != hipSuccess) return fail(e);
  if ((e = hipMemsetAsync(r->d_mask + n_words / 2, 0, 16, s)) != hipSuccess) return fail(e);
  if ((e = hipMemsetAsync(r->d_woff, 0, 8, s)) != hipSuccess) return fail(e);                  // (no read kept: woff[0] = 0 is all there is)
  if ((e = hipMemsetAsync(d_tot, 0, 16, s)) != hipSuccess) return fail(e);
  unsigned long long tot[2] = {0, 0};
  if (n_out) {
    if ((e = shn_hip_malloc(&d_src, (n_out + 1) * 4)) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(slice_place_kernel, dim3(shn_grid(n, S_BLK)), dim3(S_BLK), 0, s, S, d_span, (const uint32_t*)d_flag, (const uint64_t*)d_pos,
                       (const uint64_t*)d_wpos, n_out, n_words, r->d_woff, r->d_len, d_src, d_tot);
    hipLaunchKernelGGL(slice_copy_kernel, dim3(shn_grid(n_words / 2, S_BLK)), dim3(S_BLK), 0, s, S, d_span, (const uint64_t*)r->d_woff, (const uint32_t*)r->d_len,
                       (const uint32_t*)d_src, n_out, n_words / 2, r->d_words, r->d_mask);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (d_src) hipFree(d_src);
  if (e != hipSuccess) return fail(e);
  // bytes: 8 B of span, 4 B of length and (flags) 4 B per source read in the sizing and again in the placing, 8 + 8 + 16 B of scans,
  // 16 B of offset, length and source per kept read; the copy reads and writes every output word and mask word once (a source word
  // is shared by two output words at the most) and 12 B of offset and length per 64 bases for the search's last steps
  t.bytes(n * 2 * 16 + n * 32 + n_out * 16 + n_words * 8 * 2 + n_words / 2 * 8 * 2 + n_words / 2 * 12);
  r->total_bases = tot[0];
  r->max_len = (uint32_t)tot[1];
  int rc = shn_reads_refresh_bad(ctx, r);
  if (rc) { shn_reads_destroy(r); return rc; }
  *out = r;
  return SHN_OK;
}
