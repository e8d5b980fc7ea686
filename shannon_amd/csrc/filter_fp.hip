// --filter_FP on the device: how many bases of every transcript the read pairs routed to its partition cover
// (filter_FP.py:29-55 as run_MB_SF_fn.py:272-277 runs it per partition; here all partitions in one call).  hisat + samtools
// are replaced by the rule of DESIGN.md ("filter_FP"); the kernels below state the part of it they implement.
//
//   index   all transcripts packed 2 bits a base into one text; one record per 15-mer position that lies inside a transcript,
//           key = partition << 30 | 15-mer, value = position in the text, sorted by key (shn_sort_pairs, stable: equal keys
//           stay in text order).  A partition's pairs only ever meet the 15-mers of their own partition.
//   map     one thread per route.  A mate of L >= 15 bases may carry L / 30 mismatches and holds L / 30 + 1 disjoint 15-base
//           seeds (at 0, 15, 30, ...): one of them is free of mismatches (pigeonhole), so the exact hits of the seeds name
//           every start the rule admits.  A start reached through seed s is taken up only if no earlier seed matches there
//           too (de-duplication without a candidate store); verification is XOR + popcount of 64-bit words against the text.
//           Two passes over the same enumeration: the fragment's minimum cost, then every placement that attains it is marked.
//           Nothing is stored per fragment, so nothing is capped.
//   mark    one bit per base of the text.  The word is loaded first and the atomic OR is issued only when it would set a new
//           bit: a highly expressed transcript is covered within its first few thousand fragments and every later one then
//           costs loads only.  (The rate of scattered 64-bit integer ORs on this chip is not measured anywhere in this
//           repository; the load-first form is what keeps the kernel from depending on it.)
//   count   bits set inside every transcript's range.
//   merge   (N ranks) the same count over the OR of several bitmaps: every rank marks what ITS routes cover
//           (shn_filter_fp_cover), the owner of a partition counts over all of them (shn_filter_fp_count).
//
// The thread-per-route shape trades lane divergence (mates differ in how many candidates their seeds name) for having no
// intermediate candidate lists at all; DESIGN.md gives the measured time next to the byte models below.
#include "common.h"
#include "filter_fp_dev.h"

__device__ __forceinline__ void ffp_mark(unsigned long long* __restrict__ cov, uint64_t g0, uint32_t len) {
  const uint64_t g1 = g0 + len;
  for (uint64_t w = g0 >> 6; w <= (g1 - 1) >> 6; w++) {
    const uint64_t b0 = w << 6;
    const uint32_t lo = (uint32_t)((g0 > b0 ? g0 : b0) - b0), hi = (uint32_t)((g1 < b0 + 64 ? g1 : b0 + 64) - b0);
    const unsigned long long m = (hi - lo == 64 ? ~0ULL : ((1ULL << (hi - lo)) - 1ULL)) << lo;
    if (~cov[w] & m) atomicOr(&cov[w], m);
  }
}

// MARK == false: *best becomes the smallest cost of a concordant placement of the oriented pair (x, y); MARK == true: the placements
// of cost *best are marked (the enumeration itself: ffp_each_placement, filter_fp_dev.h)
template <bool MARK>
__device__ void ffp_pairs(const FfpIndex& I, uint64_t pkey, const FfpRead& x, const FfpRead& y, uint32_t max_span, uint32_t* best,
                          unsigned long long* __restrict__ cov) {
  if (!MARK) { ffp_min_cost(I, pkey, x, y, max_span, best); return; }
  const uint32_t lx = x.L, ly = y.L;
  ffp_each_placement<true>(I, pkey, x, y, max_span, best, [&](uint32_t c, uint64_t, uint64_t u, uint64_t v) {
    if (c == *best) { ffp_mark(cov, u, lx); ffp_mark(cov, v, ly); }
  });
}

// One route a thread: fragment i = the route's read index (strand-specific) or index mod n_pairs (strand-doubled numbering);
// oriented pairs (r1[i], RC(r2[i])) and -- not strand-specific -- (r2[i], RC(r1[i])).
__global__ __launch_bounds__(FFP_BLOCK) void ffp_map_kernel(FfpIndex I, FfpSet A, FfpSet B, uint64_t n_pairs, const uint32_t* __restrict__ pid,
                                                            const uint32_t* __restrict__ ridx, uint64_t n_routes, uint32_t n_parts, int ss,
                                                            uint32_t max_span, unsigned long long* __restrict__ cov,
                                                            unsigned long long* __restrict__ n_placed) {
  const uint64_t r = (uint64_t)blockIdx.x * FFP_BLOCK + threadIdx.x;
  bool placed = false;
  if (r < n_routes) {
    const uint32_t p = pid[r];
    uint64_t i = ridx[r];
    if (!ss && i >= n_pairs) i -= n_pairs;
    if (p < n_parts && i < n_pairs) {
      const uint64_t pkey = (uint64_t)p << (2 * FFP_SEED);
      const FfpRead a = ffp_read(A, i, false), b_rc = ffp_read(B, i, true);
      uint32_t best = FFP_NONE;
      ffp_pairs<false>(I, pkey, a, b_rc, max_span, &best, cov);
      if (!ss) {
        const FfpRead b = ffp_read(B, i, false), a_rc = ffp_read(A, i, true);
        ffp_pairs<false>(I, pkey, b, a_rc, max_span, &best, cov);
        if (best != FFP_NONE) {
          ffp_pairs<true>(I, pkey, a, b_rc, max_span, &best, cov);
          ffp_pairs<true>(I, pkey, b, a_rc, max_span, &best, cov);
        }
      } else if (best != FFP_NONE) {
        ffp_pairs<true>(I, pkey, a, b_rc, max_span, &best, cov);
      }
      placed = best != FFP_NONE;
    }
  }
  const unsigned long long vote = __ballot(placed);
  if ((threadIdx.x & 63) == 0 && vote) atomicAdd(n_placed, (unsigned long long)__popcll(vote));
}

// ASCII -> 2 bits a base, one word a thread; a base outside ACGT raises *bad
__global__ void ffp_pack_text_kernel(const uint8_t* __restrict__ text, uint64_t n, uint64_t* __restrict__ tw, uint32_t* __restrict__ bad) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w * 32 >= n) return;
  uint64_t v = 0;
  bool any_bad = false;
  for (uint32_t j = 0; j < 32; j++) {
    const uint64_t g = w * 32 + j;
    uint64_t c = 0;
    if (g < n) {
      switch (text[g]) {
        case 'A': case 'a': c = 0; break;
        case 'C': case 'c': c = 1; break;
        case 'G': case 'g': c = 2; break;
        case 'T': case 't': c = 3; break;
        default: any_bad = true;
      }
    }
    v |= c << (62 - 2 * j);
  }
  tw[w] = v;
  if (any_bad) atomicOr(bad, 1u);
}

// record r = the r-th 15-mer position inside a transcript (rec_off[j] = records of the transcripts before j)
__global__ void ffp_records_kernel(const uint64_t* __restrict__ tw, const uint64_t* __restrict__ t_off, const uint64_t* __restrict__ rec_off,
                                   const uint32_t* __restrict__ t_part, uint64_t n_tr, uint64_t n_rec, uint64_t* __restrict__ keys,
                                   uint32_t* __restrict__ vals) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rec) return;
  const uint64_t lo = shn_segment_of(rec_off, n_tr, r);       // the transcript that holds record r
  const uint64_t g = t_off[lo] + (r - rec_off[lo]);
  keys[r] = ((uint64_t)t_part[lo] << (2 * FFP_SEED)) | ffp_text_seed(tw, g);
  vals[r] = (uint32_t)g;
}

// the reverse complement of every read of a set in the set's own geometry: one thread per 64-base group (two words + one mask word)
__global__ void ffp_revcomp_kernel(const uint64_t* __restrict__ words, const uint64_t* __restrict__ mask, const uint64_t* __restrict__ woff,
                                   const uint32_t* __restrict__ lens, uint64_t n_reads, uint32_t fixed_len, uint32_t wpr, uint64_t n_groups,
                                   uint64_t* __restrict__ words_rc, uint64_t* __restrict__ mask_rc) {
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n_groups) return;
  uint64_t r, g, wbase;
  uint32_t len;
  if (!woff) {
    const uint32_t gpr = wpr / 2;
    r = gid / gpr; g = gid % gpr; wbase = r * wpr; len = fixed_len;
  } else {
    r = shn_segment_of(woff, n_reads, gid * 2); wbase = woff[r]; g = (gid * 2 - wbase) / 2; len = lens[r];
  }
  const uint64_t* w = words + wbase;
  const uint64_t* m = mask ? mask + wbase / 2 : nullptr;
  uint64_t w0 = 0, w1 = 0, mo = 0;
  for (uint32_t j = 0; j < 64; j++) {
    const uint64_t p = g * 64 + j;
    uint64_t c = 0;
    if (p < len) {
      const uint32_t q = len - 1 - (uint32_t)p;
      c = 3 - ((w[q >> 5] >> (62 - 2 * (q & 31))) & 3);
      if (m && ((m[q >> 6] >> (63 - (q & 63))) & 1)) { mo |= 1ULL << (63 - j); c = 0; }
    }
    if (j < 32) w0 |= c << (62 - 2 * j); else w1 |= c << (62 - 2 * (j - 32));
  }
  words_rc[wbase + 2 * g] = w0;
  words_rc[wbase + 2 * g + 1] = w1;
  if (mask_rc) mask_rc[wbase / 2 + g] = mo;
}

__global__ void ffp_count_kernel(const unsigned long long* __restrict__ cov, const uint64_t* __restrict__ t_off, uint64_t n_tr,
                                 uint32_t* __restrict__ hits) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_tr) return;
  const uint64_t g0 = t_off[j], g1 = t_off[j + 1];
  uint32_t n = 0;
  if (g1 > g0) {
    for (uint64_t w = g0 >> 6; w <= (g1 - 1) >> 6; w++) {
      const uint64_t b0 = w << 6;
      const uint32_t lo = (uint32_t)((g0 > b0 ? g0 : b0) - b0), hi = (uint32_t)((g1 < b0 + 64 ? g1 : b0 + 64) - b0);
      const unsigned long long m = (hi - lo == 64 ? ~0ULL : ((1ULL << (hi - lo)) - 1ULL)) << lo;
      n += (uint32_t)__popcll(cov[w] & m);
    }
  }
  hits[j] = n;
}

// The OR of n_covers bitmaps and the masked count of a transcript's bits in one pass.  One wave a transcript: lane l takes the words
// first + l, first + l + 64, ... of the transcript's range and reads that word of every bitmap, so the 64 lanes of a load read 512
// consecutive bytes of one bitmap; the lanes' counts meet in a shuffle reduction.  (A thread a transcript -- ffp_count_kernel's shape
// -- would walk n_covers bitmaps with a stride of one transcript between neighbouring lanes.)  Word w of the text is word w - word0
// of every bitmap; the host has checked that every transcript lies inside the window.
__global__ __launch_bounds__(FFP_BLOCK) void ffp_merge_count_kernel(const unsigned long long* __restrict__ covers, uint32_t n_covers, uint64_t n_words,
                                                                    uint64_t word0, const uint64_t* __restrict__ t_off, uint64_t n_tr,
                                                                    uint32_t* __restrict__ hits) {
  const uint64_t j = (uint64_t)blockIdx.x * (FFP_BLOCK / 64) + (threadIdx.x >> 6);
  if (j >= n_tr) return;                                   // (the whole wave)
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t g0 = t_off[j], g1 = t_off[j + 1];
  uint32_t n = 0;
  if (g1 > g0) {
    const uint64_t last = (g1 - 1) >> 6;
    for (uint64_t w = (g0 >> 6) + lane; w <= last; w += 64) {
      const uint64_t b0 = w << 6;
      const uint32_t lo = (uint32_t)((g0 > b0 ? g0 : b0) - b0), hi = (uint32_t)((g1 < b0 + 64 ? g1 : b0 + 64) - b0);
      const unsigned long long m = (hi - lo == 64 ? ~0ULL : ((1ULL << (hi - lo)) - 1ULL)) << lo;
      unsigned long long v = 0;
      for (uint32_t c = 0; c < n_covers; c++) v |= covers[(uint64_t)c * n_words + (w - word0)];
      n += (uint32_t)__popcll(v & m);
    }
  }
  for (int off = 32; off; off >>= 1) n += __shfl_down(n, off, 64);
  if (lane == 0) hits[j] = n;
}

int ffp_set(shn_ctx* ctx, ShnDevBufs& bufs, const shn_reads* r, bool want_rc, FfpSet* out, uint64_t* rc_bytes) {
  hipStream_t s = ctx->stream;
  const bool use_mask = r->n_invalid != 0 && r->d_mask && r->d_bad;
  FfpSet S;
  S.words = r->d_words; S.mask = use_mask ? r->d_mask : nullptr; S.words_rc = nullptr; S.mask_rc = nullptr;
  S.woff = r->fixed_len ? nullptr : r->d_woff; S.len = r->fixed_len ? nullptr : r->d_len; S.bad = use_mask ? r->d_bad : nullptr;
  S.fixed_len = r->fixed_len; S.wpr = r->wpr;
  if (want_rc && r->n_words) {
    uint64_t *wrc = nullptr, *mrc = nullptr;
    HIP_TRY(bufs.get(&wrc, (r->n_words + 2) * 8));
    HIP_TRY(hipMemsetAsync(wrc + r->n_words, 0, 16, s));
    if (use_mask) {
      HIP_TRY(bufs.get(&mrc, (r->n_words / 2 + 2) * 8));
      HIP_TRY(hipMemsetAsync(mrc + r->n_words / 2, 0, 16, s));
    }
    const uint64_t n_groups = r->n_words / 2;
    hipLaunchKernelGGL(ffp_revcomp_kernel, dim3((uint32_t)cdiv(n_groups, 256)), dim3(256), 0, s, S.words, S.mask, S.woff, S.len, r->n_reads,
                       r->fixed_len, r->wpr, n_groups, wrc, mrc);
    S.words_rc = wrc; S.mask_rc = mrc;
    *rc_bytes += r->n_words * 16 + (use_mask ? r->n_words * 8 : 0);          // the set read once, its reverse complement written once
  }
  *out = S;
  return SHN_OK;
}

int ffp_record_offsets(const std::string& fn, const uint64_t* t_off, uint64_t n_tr, std::vector<uint64_t>* rec_off) {
  if (t_off[0] != 0) return shn_fail(SHN_ERR_ARG, fn + ": t_off[0] is not 0");
  rec_off->assign(n_tr + 1, 0);
  for (uint64_t j = 0; j < n_tr; j++) {
    if (t_off[j + 1] < t_off[j]) return shn_fail(SHN_ERR_ARG, fn + ": t_off not monotone");
    const uint64_t len = t_off[j + 1] - t_off[j];
    (*rec_off)[j + 1] = (*rec_off)[j] + (len >= FFP_SEED ? len - FFP_SEED + 1 : 0);
  }
  return SHN_OK;
}

// The transcripts' text packed and the sorted index of its 15-mers (the header says what the arguments are).
int ffp_index_build(const std::string& fn, shn_ctx* ctx, ShnDevBufs& bufs, int slot, const uint8_t* text, const uint64_t* t_off, const uint32_t* t_part,
                    uint64_t n_tr, uint32_t n_parts, const std::vector<uint64_t>& rec_off, FfpIndex* out, uint64_t* n_tw_out) {
  hipStream_t s = ctx->stream;
  const uint64_t total = t_off[n_tr], n_rec = rec_off[n_tr];
  const uint64_t n_tw = cdiv(total, 32);
  uint8_t* d_text = nullptr;
  uint64_t *d_tw = nullptr, *d_toff = nullptr, *d_roff = nullptr, *d_keys = nullptr, *d_keys_tmp = nullptr;
  uint32_t *d_tpart = nullptr, *d_vals = nullptr, *d_vals_tmp = nullptr, *d_flag = nullptr;
  HIP_TRY(bufs.get(&d_text, total + 1));
  HIP_TRY(bufs.get(&d_tw, (n_tw + 2) * 8));
  HIP_TRY(bufs.get(&d_toff, (n_tr + 1) * 8));
  HIP_TRY(bufs.get(&d_roff, (n_tr + 1) * 8));
  HIP_TRY(bufs.get(&d_tpart, n_tr * 4));
  HIP_TRY(bufs.get(&d_flag, 4));
  HIP_TRY(bufs.get(&d_keys, (n_rec + 1) * 8));
  HIP_TRY(bufs.get(&d_keys_tmp, (n_rec + 1) * 8));
  HIP_TRY(bufs.get(&d_vals, (n_rec + 1) * 4));
  HIP_TRY(bufs.get(&d_vals_tmp, (n_rec + 1) * 4));
  HIP_TRY(hipMemcpyAsync(d_text, text, total, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_toff, t_off, (n_tr + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_roff, rec_off.data(), (n_tr + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_tpart, t_part, n_tr * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(d_flag, 0, 4, s));
  HIP_TRY(hipMemsetAsync(d_tw + n_tw, 0, 16, s));
  {
    // (n_parts >= 1 here.  The partition field holds 0 .. n_parts, one value more than there are partitions: kept as it was, it
    // decides the number of sort passes at n_parts = 2^k)
    const int key_bits = 2 * FFP_SEED + shn_bits_for((uint64_t)n_parts + 1);
    const uint64_t passes = (uint64_t)(key_bits + 7) / 8;
    TimerRegion treg(ctx, slot);
    // bytes: the text read and written packed (1.25 B a base), a record written (12 B), every sort pass reads and writes the records
    treg.bytes(total + total / 4 + n_rec * 12 + passes * n_rec * 24);
    if (n_tw) hipLaunchKernelGGL(ffp_pack_text_kernel, dim3((uint32_t)cdiv(n_tw, 256)), dim3(256), 0, s, d_text, total, d_tw, d_flag);
    if (n_rec) {
      hipLaunchKernelGGL(ffp_records_kernel, dim3((uint32_t)cdiv(n_rec, 256)), dim3(256), 0, s, d_tw, d_toff, d_roff, d_tpart, n_tr, n_rec, d_keys, d_vals);
      int rc = shn_sort_pairs(ctx, d_keys, d_vals, d_keys_tmp, d_vals_tmp, n_rec, 0, key_bits);
      if (rc) return rc;
    }
  }
  uint32_t flag = 0;
  HIP_TRY(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (flag) return shn_fail(SHN_ERR_ARG, fn + ": a transcript holds a base outside ACGT");
  out->keys = d_keys; out->vals = d_vals; out->n_rec = n_rec; out->tw = d_tw; out->t_off = d_toff; out->n_tr = n_tr;
  *n_tw_out = n_tw;
  return SHN_OK;
}

// Both halves of the filter's device work.  hits != NULL: index, map + mark, count -- the bitmap never leaves the device
// (shn_filter_fp_hits).  cover != NULL: index, map + mark, the bitmap to the host (shn_filter_fp_cover).  fn: who is asked, for the messages.
static int ffp_run(const char* fn_, shn_ctx* ctx, const uint8_t* text, const uint64_t* t_off, const uint32_t* t_part, uint64_t n_tr, uint32_t n_parts,
                   const shn_reads* r1, const shn_reads* r2, const shn_routes* routes, const uint32_t* h_pid, const uint32_t* h_frag, uint64_t n_host,
                   int strand_specific, uint32_t max_span, uint32_t* hits, uint64_t* cover, uint64_t* stats) {
  const std::string fn(fn_);
  if (!ctx || !r1 || !r2 || !t_off || (n_tr && (!text || !t_part || (!hits && !cover))))
    return shn_fail(SHN_ERR_ARG, fn + ": NULL argument");
  if (!routes && n_host && (!h_pid || !h_frag)) return shn_fail(SHN_ERR_ARG, fn + ": routes neither on the device nor on the host");
  if (r1->n_reads != r2->n_reads) return shn_fail(SHN_ERR_ARG, fn + ": the two read sets are not mates of each other (different sizes)");
  if (n_parts >= (1u << 31)) return shn_fail(SHN_ERR_ARG, fn + ": too many partitions");
  const uint64_t n_pairs = r1->n_reads;
  const uint64_t total = t_off[n_tr];
  std::vector<uint64_t> rec_off;
  if (int rc = ffp_record_offsets(fn, t_off, n_tr, &rec_off)) return rc;
  if (total >= 0xFFFFFF00ULL) return shn_fail(SHN_ERR_OVERFLOW, fn + ": more than 2^32 transcript bases in one call");
  for (uint64_t j = 0; j < n_tr; j++)
    if (t_part[j] >= n_parts) return shn_fail(SHN_ERR_ARG, fn + ": partition of a transcript out of range");
  const uint64_t n_rec = rec_off[n_tr];
  if (!routes)
    for (uint64_t i = 0; i < n_host; i++)
      if (h_pid[i] >= n_parts || h_frag[i] >= (strand_specific ? n_pairs : 2 * n_pairs))
        return shn_fail(SHN_ERR_ARG, fn + ": a route names a partition or a fragment that does not exist");
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);

  const uint32_t *d_pid = nullptr, *d_ridx = nullptr;
  uint64_t n_routes = 0;
  if (routes) {
    int rc = shn_routes_device_arrays(routes, &d_pid, &d_ridx, &n_routes);
    if (rc) return rc;
  } else if (n_host) {
    uint32_t *p = nullptr, *f = nullptr;
    HIP_TRY(bufs.get(&p, n_host * 4));
    HIP_TRY(bufs.get(&f, n_host * 4));
    HIP_TRY(hipMemcpyAsync(p, h_pid, n_host * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(f, h_frag, n_host * 4, hipMemcpyHostToDevice, s));
    d_pid = p; d_ridx = f; n_routes = n_host;
  }
  if (stats) { stats[0] = n_routes; stats[1] = 0; }
  if (n_tr == 0) { HIP_TRY(hipStreamSynchronize(s)); return SHN_OK; }

  // ---- index
  FfpIndex I;
  uint64_t n_tw = 0;
  {
    int rc = ffp_index_build(fn, ctx, bufs, T_FFP_INDEX, text, t_off, t_part, n_tr, n_parts, rec_off, &I, &n_tw);
    if (rc) return rc;
  }
  const uint64_t* d_toff = I.t_off;
  uint32_t* d_hits = nullptr;
  unsigned long long *d_cov = nullptr, *d_placed = nullptr;

  // ---- map + mark
  const uint64_t n_cov = cdiv(total, 64) + 1;
  HIP_TRY(bufs.get(&d_cov, n_cov * 8));
  HIP_TRY(bufs.get(&d_placed, 8));
  if (hits) HIP_TRY(bufs.get(&d_hits, n_tr * 4));
  HIP_TRY(hipMemsetAsync(d_cov, 0, n_cov * 8, s));
  HIP_TRY(hipMemsetAsync(d_placed, 0, 8, s));
  if (n_routes && n_rec) {
    FfpSet A, B;
    uint64_t rc_bytes = 0;
    TimerRegion treg(ctx, T_FFP_MAP);
    int rc = ffp_set(ctx, bufs, r1, !strand_specific, &A, &rc_bytes);
    if (!rc) rc = ffp_set(ctx, bufs, r2, true, &B, &rc_bytes);
    if (rc) return rc;
    // bytes: a route (8 B) and both mates of its fragment in each orientation used (2 bits a base); the index, the text and the
    // bitmap are re-read from the caches and priced once; what the reverse complements cost is added above
    const uint64_t per_pair = n_pairs ? (r1->n_words + r2->n_words) * 8 / n_pairs : 0;
    treg.bytes(rc_bytes + n_routes * (8 + per_pair * (strand_specific ? 1 : 2)) + n_rec * 12 + n_tw * 8 + n_cov * 8);
    hipLaunchKernelGGL(ffp_map_kernel, dim3((uint32_t)cdiv(n_routes, FFP_BLOCK)), dim3(FFP_BLOCK), 0, s, I, A, B, n_pairs, d_pid, d_ridx, n_routes,
                       n_parts, strand_specific ? 1 : 0, max_span, d_cov, d_placed);
  }
  // ---- count
  if (hits) {
    TimerRegion treg(ctx, T_FFP_COUNT);
    treg.bytes(n_cov * 8 + n_tr * 20);          // the bitmap, two offsets read and a count written per transcript
    hipLaunchKernelGGL(ffp_count_kernel, dim3((uint32_t)cdiv(n_tr, 256)), dim3(256), 0, s, d_cov, d_toff, n_tr, d_hits);
  }
  unsigned long long placed = 0;
  if (hits) HIP_TRY(hipMemcpyAsync(hits, d_hits, n_tr * 4, hipMemcpyDeviceToHost, s));
  if (cover && total) HIP_TRY(hipMemcpyAsync(cover, d_cov, cdiv(total, 64) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&placed, d_placed, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  if (stats) stats[1] = placed;
  return SHN_OK;
}

extern "C" int shn_filter_fp_hits(shn_ctx* ctx, const uint8_t* text, const uint64_t* t_off, const uint32_t* t_part, uint64_t n_tr,
                                  uint32_t n_parts, const shn_reads* r1, const shn_reads* r2, const shn_routes* routes, const uint32_t* h_pid,
                                  const uint32_t* h_frag, uint64_t n_host, int strand_specific, uint32_t max_span, uint32_t* hits,
                                  uint64_t* stats) {
  if (n_tr && !hits) return shn_fail(SHN_ERR_ARG, "shn_filter_fp_hits: NULL argument");
  return ffp_run("shn_filter_fp_hits", ctx, text, t_off, t_part, n_tr, n_parts, r1, r2, routes, h_pid, h_frag, n_host, strand_specific, max_span,
                 hits, nullptr, stats);
}

// One rank's half of the filter on N ranks: what THESE routes cover, as the bitmap itself (filter_FP.py:29-55 as run_MB_SF_fn.py:272-277
// runs it; the depth file of a partition is the union of what every rank's pairs cover).
extern "C" int shn_filter_fp_cover(shn_ctx* ctx, const uint8_t* text, const uint64_t* t_off, const uint32_t* t_part, uint64_t n_tr,
                                   uint32_t n_parts, const shn_reads* r1, const shn_reads* r2, const shn_routes* routes, const uint32_t* h_pid,
                                   const uint32_t* h_frag, uint64_t n_host, int strand_specific, uint32_t max_span, uint64_t* cover,
                                   uint64_t* stats) {
  if (n_tr && !cover) return shn_fail(SHN_ERR_ARG, "shn_filter_fp_cover: NULL argument");
  return ffp_run("shn_filter_fp_cover", ctx, text, t_off, t_part, n_tr, n_parts, r1, r2, routes, h_pid, h_frag, n_host, strand_specific, max_span,
                 nullptr, cover, stats);
}

// The owner's half: the bitmaps of all ranks for a window of the text -> covered bases of every transcript inside it (the depth
// file's line count per transcript, filter_FP.py:7-13).
extern "C" int shn_filter_fp_count(shn_ctx* ctx, const uint64_t* covers, uint32_t n_covers, uint64_t n_words, uint64_t word0,
                                   const uint64_t* t_off, uint64_t n_tr, uint32_t* hits) {
  if (!ctx || !t_off || (n_tr && !hits)) return shn_fail(SHN_ERR_ARG, "shn_filter_fp_count: NULL argument");
  if (n_covers == 0) return shn_fail(SHN_ERR_ARG, "shn_filter_fp_count: no bitmap to count (n_covers is 0)");
  if (n_words && !covers) return shn_fail(SHN_ERR_ARG, "shn_filter_fp_count: NULL argument");
  if (word0 >= (1ULL << 56) || n_words >= (1ULL << 56)) return shn_fail(SHN_ERR_ARG, "shn_filter_fp_count: window out of range");
  const uint64_t lo = word0 * 64, hi = (word0 + n_words) * 64;
  for (uint64_t j = 0; j <= n_tr; j++) {
    if (j && t_off[j] < t_off[j - 1]) return shn_fail(SHN_ERR_ARG, "shn_filter_fp_count: t_off not monotone");
    if (t_off[j] < lo || t_off[j] > hi)
      return shn_fail(SHN_ERR_ARG, "shn_filter_fp_count: a transcript lies outside the window of the bitmaps (t_off " + std::to_string(t_off[j]) +
                                       ", window " + std::to_string(lo) + " .. " + std::to_string(hi) + ")");
  }
  if (n_tr == 0) return SHN_OK;
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  unsigned long long* d_cov = nullptr;
  uint64_t* d_toff = nullptr;
  uint32_t* d_hits = nullptr;
  const uint64_t cov_bytes = (uint64_t)n_covers * n_words * 8;
  HIP_TRY(bufs.get(&d_cov, cov_bytes + 8));
  HIP_TRY(bufs.get(&d_toff, (n_tr + 1) * 8));
  HIP_TRY(bufs.get(&d_hits, n_tr * 4));
  if (cov_bytes) HIP_TRY(hipMemcpyAsync(d_cov, covers, cov_bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_toff, t_off, (n_tr + 1) * 8, hipMemcpyHostToDevice, s));
  {
    TimerRegion treg(ctx, T_FFP_MERGE);
    // bytes: the words of every bitmap that lie under a transcript (a boundary word is read by both neighbours), two offsets read and
    // a count written per transcript
    treg.bytes((uint64_t)n_covers * (cdiv(t_off[n_tr] - t_off[0], 64) + n_tr) * 8 + n_tr * 20);
    hipLaunchKernelGGL(ffp_merge_count_kernel, dim3((uint32_t)cdiv(n_tr, FFP_BLOCK / 64)), dim3(FFP_BLOCK), 0, s, d_cov, n_covers, n_words, word0, d_toff,
                       n_tr, d_hits);
  }
  HIP_TRY(hipMemcpyAsync(hits, d_hits, n_tr * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  return SHN_OK;
}
