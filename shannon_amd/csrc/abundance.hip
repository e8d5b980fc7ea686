// --kallisto_cutoff on the device: how many read pairs every final transcript explains (shannon.py:309-318, 609-614,
// filter_kallisto.py:23-31 -- `kallisto index` + `kallisto quant`).  kallisto is replaced by the rule of DESIGN.md 3.10 ("abundance");
// the kernels below state the part of it they implement.  The placement of a pair is --filter_FP's (filter_fp_dev.h: the same
// index, the same enumeration), all transcripts forming one partition.  Single reads (python -m shannon_amd.quant --single, DESIGN.md
// 3.13) go the same way with a map stage of their own: no mate, no span, no histogram.
//
//   map      one thread per fragment, three passes over the same enumeration: the minimum cost; the number of placements that attain
//            it (and the span of the only one: the fragment-length histogram, integer atomics in LDS, then one global add per
//            bin and block); behind an exclusive scan of the numbers, the placements' transcript ids -- count, scan, fill, so
//            nothing is capped.  The filling thread then sorts its list, drops the repeats (two placements on one transcript)
//            and hashes what is left.
//   classes  the fragments sorted by the hash of their list (shn_sort_pairs, stable: equal hashes stay in fragment order; an
//            unmapped fragment carries the largest key and ends up behind the mapped ones); a fragment heads a class iff its LIST
//            differs from its predecessor's, element by element -- two lists with one hash give two classes, a hash that falls
//            between two runs of one list splits that list's class in two, which the EM does not notice; scan of the head flags ->
//            class_off[] / members[] / n_c[].
//   EM       the transposed CSR once (entries sorted by transcript with the same stable sort: a transcript's entries stay in class
//            order); a round is two gather passes, a wave a row: d_c = sum over the members of alpha_j / eff_j, then alpha'_j = sum
//            over the classes of j of n_c (alpha_j / eff_j) / d_c.  Every sum has ONE order: lane l adds the row's terms l, l + 64,
//            l + 128, ... in that order, starting from 0, then the 64 partial sums meet in the shuffle tree of strides 32, 16, 8, 4, 2, 1
//            (lane l takes lane l + stride).  No floating-point atomic anywhere: two runs give the same bits.
//   merge    (quant on several read files or ranks) the classes of several read sets as weighted lists: a key per
//            list -- the map stage's hash of the same list --, then `classes` with a list in a fragment's place and n_c = the sum of
//            a class's weights.  Integers only.
#include "filter_fp_dev.h"

#define ABD_MAX_SPAN 8191u     // bins of the span histogram a block keeps in LDS (32 KiB); a larger max_span is refused
#define ABD_INSERTION 32u      // a fragment's list up to this many ids is sorted by insertion, a longer one by heapsort

struct shn_abundance {
  uint64_t n_tr = 0, n_frag = 0, mapped = 0;
  std::vector<uint64_t> class_off, n_c, hist;
  std::vector<uint32_t> members;
};

// f(j, span) for every placement of fragment i whose cost is `best` (both oriented pairs unless strand-specific)
template <class F>
__device__ __forceinline__ void abd_each_best(const FfpIndex& I, const FfpSet& A, const FfpSet& B, uint64_t i, int ss, uint32_t max_span,
                                              uint32_t best, F&& f) {
  const FfpRead a = ffp_read(A, i, false), b_rc = ffp_read(B, i, true);
  ffp_each_placement<true>(I, 0, a, b_rc, max_span, &best, [&](uint32_t c, uint64_t j, uint64_t u, uint64_t v) {
    if (c == best) f(j, (uint32_t)(v + b_rc.L - u));
  });
  if (!ss) {
    const FfpRead b = ffp_read(B, i, false), a_rc = ffp_read(A, i, true);
    ffp_each_placement<true>(I, 0, b, a_rc, max_span, &best, [&](uint32_t c, uint64_t j, uint64_t u, uint64_t v) {
      if (c == best) f(j, (uint32_t)(v + a_rc.L - u));
    });
  }
}

// pass 1 + 2: best[i] = the fragment's minimum cost (FFP_NONE: unmapped), cnt[i] = placements of that cost; a fragment with exactly one
// adds 1 to the bin of its span
__global__ __launch_bounds__(FFP_BLOCK) void abd_count_kernel(FfpIndex I, FfpSet A, FfpSet B, uint64_t n_pairs, int ss, uint32_t max_span,
                                                              uint32_t* __restrict__ best_out, uint32_t* __restrict__ cnt,
                                                              unsigned long long* __restrict__ hist, unsigned long long* __restrict__ n_mapped,
                                                              uint32_t* __restrict__ too_many) {
  extern __shared__ __attribute__((aligned(16))) uint32_t abd_lh[];
  for (uint32_t k = threadIdx.x; k <= max_span; k += FFP_BLOCK) abd_lh[k] = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * FFP_BLOCK + threadIdx.x;
  bool placed = false;
  if (i < n_pairs) {
    uint32_t best = FFP_NONE;
    ffp_min_cost(I, 0, ffp_read(A, i, false), ffp_read(B, i, true), max_span, &best);
    if (!ss) ffp_min_cost(I, 0, ffp_read(B, i, false), ffp_read(A, i, true), max_span, &best);
    uint64_t n = 0;
    uint32_t span = 0;
    if (best != FFP_NONE) abd_each_best(I, A, B, i, ss, max_span, best, [&](uint64_t, uint32_t sp) { n++; span = sp; });
    if (n > 0xFFFFFFFEULL) { atomicOr(too_many, 1u); n = 0; }
    placed = n != 0;
    best_out[i] = placed ? best : FFP_NONE;
    cnt[i] = (uint32_t)n;
    if (n == 1 && span <= max_span) atomicAdd(&abd_lh[span], 1u);
  }
  const unsigned long long vote = __ballot(placed);
  if ((threadIdx.x & 63) == 0 && vote) atomicAdd(n_mapped, (unsigned long long)__popcll(vote));
  __syncthreads();
  for (uint32_t k = threadIdx.x; k <= max_span; k += FFP_BLOCK)
    if (abd_lh[k]) atomicAdd(&hist[k], (unsigned long long)abd_lh[k]);
}

__device__ __forceinline__ uint64_t abd_mix(uint64_t h, uint64_t v) {
  h ^= v + 0x9E3779B97F4A7C15ULL;
  h ^= h >> 33; h *= 0xFF51AFD7ED558CCDULL; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ULL; h ^= h >> 33;
  return h;
}

// max-heap L[0 .. n): the value at p sinks to its place
__device__ __forceinline__ void abd_sift_down(uint32_t* L, uint64_t p, uint64_t n) {
  const uint32_t v = L[p];
  for (;;) {
    uint64_t c = 2 * p + 1;
    if (c >= n) break;
    if (c + 1 < n && L[c + 1] > L[c]) c++;
    if (L[c] <= v) break;
    L[p] = L[c];
    p = c;
  }
  L[p] = v;
}

// The n >= 1 ids of a fragment's placements as they were enumerated -> sorted, repeats dropped: *nuniq of them stay at the front,
// *key = 63 bits of their hash: the tail of abd_fill_kernel, for abd_fill_single_kernel.  (abd_fill_kernel keeps its own lines:
// calling this from it compiles to 90 VGPRs instead of its 88.)
__device__ __forceinline__ void abd_finish_list(uint32_t* L, uint64_t n, uint32_t* nuniq, uint64_t* key) {
  if (n <= ABD_INSERTION) {
    for (uint64_t p = 1; p < n; p++) {
      const uint32_t v = L[p];
      uint64_t q = p;
      while (q > 0 && L[q - 1] > v) { L[q] = L[q - 1]; q--; }
      L[q] = v;
    }
  } else {
    for (uint64_t p = n / 2; p-- > 0;) abd_sift_down(L, p, n);
    for (uint64_t e = n - 1; e > 0; e--) {
      const uint32_t v = L[0]; L[0] = L[e]; L[e] = v;
      abd_sift_down(L, 0, e);
    }
  }
  uint64_t u = 1;
  for (uint64_t p = 1; p < n; p++)
    if (L[p] != L[u - 1]) L[u++] = L[p];
  uint64_t h = abd_mix(0, u);
  for (uint64_t p = 0; p < u; p++) h = abd_mix(h, L[p]);
  *nuniq = (uint32_t)u;
  *key = h >> 1;
}

// pass 3: the transcript ids of fragment i's placements into ids[off[i] .. off[i + 1]), sorted, repeats dropped: nuniq[i] of them
// stay at the front.  key[i] = 63 bits of the list's hash; an unmapped fragment: all ones.
__global__ __launch_bounds__(FFP_BLOCK) void abd_fill_kernel(FfpIndex I, FfpSet A, FfpSet B, uint64_t n_pairs, int ss, uint32_t max_span,
                                                             const uint32_t* __restrict__ best_in, const uint64_t* __restrict__ off,
                                                             uint32_t* __restrict__ ids, uint32_t* __restrict__ nuniq, uint64_t* __restrict__ key,
                                                             uint32_t* __restrict__ frag) {
  const uint64_t i = (uint64_t)blockIdx.x * FFP_BLOCK + threadIdx.x;
  if (i >= n_pairs) return;
  frag[i] = (uint32_t)i;
  const uint64_t o = off[i], n = off[i + 1] - o;
  if (n == 0) { nuniq[i] = 0; key[i] = ~0ULL; return; }
  uint32_t* L = ids + o;
  uint64_t k = 0;
  abd_each_best(I, A, B, i, ss, max_span, best_in[i], [&](uint64_t j, uint32_t) { if (k < n) L[k] = (uint32_t)j; k++; });
  // (k == n: the same enumeration as the counting pass.)  The list is a few ascending runs, one per seed and orientation (a seed's
  // hits are in text order).  Up to ABD_INSERTION ids: insertion sort; a longer list (a fragment inside a repeat that many
  // transcripts share) by heapsort in place, so that one lane never does more than n log n moves while its wave waits.
  if (n <= ABD_INSERTION) {
    for (uint64_t p = 1; p < n; p++) {
      const uint32_t v = L[p];
      uint64_t q = p;
      while (q > 0 && L[q - 1] > v) { L[q] = L[q - 1]; q--; }
      L[q] = v;
    }
  } else {
    for (uint64_t p = n / 2; p-- > 0;) abd_sift_down(L, p, n);
    for (uint64_t e = n - 1; e > 0; e--) {
      const uint32_t v = L[0]; L[0] = L[e]; L[e] = v;
      abd_sift_down(L, 0, e);
    }
  }
  uint64_t u = 1;
  for (uint64_t p = 1; p < n; p++)
    if (L[p] != L[u - 1]) L[u++] = L[p];
  uint64_t h = abd_mix(0, u);
  for (uint64_t p = 0; p < u; p++) h = abd_mix(h, L[p]);
  nuniq[i] = (uint32_t)u;
  key[i] = h >> 1;
}

// ---- single reads (DESIGN.md 3.13 rule 1): read i as itself and, unless strand-specific, as its reverse complement
// f(j) for every placement of read i whose cost is `best`
template <class F>
__device__ __forceinline__ void abd_each_best_single(const FfpIndex& I, const FfpSet& A, uint64_t i, int ss, uint32_t best, F&& f) {
  ffp_each_single<true>(I, 0, ffp_read(A, i, false), &best, [&](uint32_t c, uint64_t j, uint64_t) { if (c == best) f(j); });
  if (!ss) ffp_each_single<true>(I, 0, ffp_read(A, i, true), &best, [&](uint32_t c, uint64_t j, uint64_t) { if (c == best) f(j); });
}

// pass 1 + 2: best[i] = the read's minimum cost over its orientations (FFP_NONE: unmapped), cnt[i] = placements of that cost
__global__ __launch_bounds__(FFP_BLOCK) void abd_count_single_kernel(FfpIndex I, FfpSet A, uint64_t n_reads, int ss, uint32_t* __restrict__ best_out,
                                                                     uint32_t* __restrict__ cnt, unsigned long long* __restrict__ n_mapped,
                                                                     uint32_t* __restrict__ too_many) {
  const uint64_t i = (uint64_t)blockIdx.x * FFP_BLOCK + threadIdx.x;
  bool placed = false;
  if (i < n_reads) {
    uint32_t best = FFP_NONE;
    auto lower = [&](uint32_t c, uint64_t, uint64_t) { if (c < best) best = c; };
    ffp_each_single<false>(I, 0, ffp_read(A, i, false), &best, lower);
    if (!ss) ffp_each_single<false>(I, 0, ffp_read(A, i, true), &best, lower);
    uint64_t n = 0;
    if (best != FFP_NONE) abd_each_best_single(I, A, i, ss, best, [&](uint64_t) { n++; });
    if (n > 0xFFFFFFFEULL) { atomicOr(too_many, 1u); n = 0; }
    placed = n != 0;
    best_out[i] = placed ? best : FFP_NONE;
    cnt[i] = (uint32_t)n;
  }
  const unsigned long long vote = __ballot(placed);
  if ((threadIdx.x & 63) == 0 && vote) atomicAdd(n_mapped, (unsigned long long)__popcll(vote));
}

// pass 3, as abd_fill_kernel: the ids of read i's placements into ids[off[i] .. off[i + 1]), sorted, repeats dropped, hashed
__global__ __launch_bounds__(FFP_BLOCK) void abd_fill_single_kernel(FfpIndex I, FfpSet A, uint64_t n_reads, int ss, const uint32_t* __restrict__ best_in,
                                                                    const uint64_t* __restrict__ off, uint32_t* __restrict__ ids,
                                                                    uint32_t* __restrict__ nuniq, uint64_t* __restrict__ key, uint32_t* __restrict__ frag) {
  const uint64_t i = (uint64_t)blockIdx.x * FFP_BLOCK + threadIdx.x;
  if (i >= n_reads) return;
  frag[i] = (uint32_t)i;
  const uint64_t o = off[i], n = off[i + 1] - o;
  if (n == 0) { nuniq[i] = 0; key[i] = ~0ULL; return; }
  uint32_t* L = ids + o;
  uint64_t k = 0;
  abd_each_best_single(I, A, i, ss, best_in[i], [&](uint64_t j) { if (k < n) L[k] = (uint32_t)j; k++; });
  abd_finish_list(L, n, &nuniq[i], &key[i]);
}

// sorted position r heads a class iff its fragment's list is not its predecessor's
__global__ void abd_heads_kernel(uint64_t n_mapped, const uint32_t* __restrict__ frag, const uint64_t* __restrict__ off, const uint32_t* __restrict__ nuniq,
                                 const uint32_t* __restrict__ ids, uint32_t* __restrict__ head) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_mapped) return;
  uint32_t h = 1;
  if (r) {
    const uint32_t f = frag[r], g = frag[r - 1];
    const uint32_t n = nuniq[f];
    if (n == nuniq[g]) {
      const uint32_t *a = ids + off[f], *b = ids + off[g];
      uint32_t p = 0;
      while (p < n && a[p] == b[p]) p++;
      h = p < n;
    }
  }
  head[r] = h;
}

// class c = the head flags before its head: first[c] = sorted position of its head, size[c] = members
__global__ void abd_first_kernel(uint64_t n_mapped, uint64_t n_classes, const uint32_t* __restrict__ head, const uint64_t* __restrict__ head_scan,
                                 const uint32_t* __restrict__ frag, const uint32_t* __restrict__ nuniq, uint64_t* __restrict__ first,
                                 uint32_t* __restrict__ size) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_mapped) return;
  if (head[r]) {
    const uint64_t c = head_scan[r];
    if (c < n_classes) { first[c] = r; size[c] = nuniq[frag[r]]; }
  }
  if (r == n_mapped - 1) first[n_classes] = n_mapped;
}

__global__ void abd_members_kernel(uint64_t n_classes, const uint64_t* __restrict__ first, const uint32_t* __restrict__ frag,
                                   const uint64_t* __restrict__ off, const uint32_t* __restrict__ ids, const uint64_t* __restrict__ class_off,
                                   uint32_t* __restrict__ members, uint64_t* __restrict__ n_c) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_classes) return;
  const uint32_t* src = ids + off[frag[first[c]]];
  const uint64_t o = class_off[c], n = class_off[c + 1] - o;
  for (uint64_t p = 0; p < n; p++) members[o + p] = src[p];
  n_c[c] = first[c + 1] - first[c];
}

// class c of weighted lists (shn_abundance_merge): n_c[c] = the sum of weight[frag[r]] over its sorted positions r in [first[c], first[c + 1]),
// a wave a class: lane l adds the positions first[c] + l, + 64, ..., then the 64 sums meet in the shuffle tree.  64-bit integer adds: exact
// in any order, no atomics.
__global__ __launch_bounds__(FFP_BLOCK) void abd_weights_kernel(uint64_t n_classes, const uint64_t* __restrict__ first, const uint32_t* __restrict__ frag,
                                                                const uint64_t* __restrict__ weight, uint64_t* __restrict__ n_c) {
  const uint64_t c = (uint64_t)blockIdx.x * (FFP_BLOCK / 64) + (threadIdx.x >> 6);
  if (c >= n_classes) return;                               // (the whole wave)
  const uint32_t lane = threadIdx.x & 63;
  unsigned long long x = 0;
  for (uint64_t r = first[c] + lane, end = first[c + 1]; r < end; r += 64) x += weight[frag[r]];
  for (int off = 32; off; off >>= 1) x += __shfl_down(x, off, 64);
  if (lane == 0) n_c[c] = x;
}

// ---- classes: the fragments (pairs or single reads) whose lists the map stage left -- ids[off[i] .. off[i] + nuniq[i]) sorted, key[i]
// their hash, frag[i] = i, `mapped` of the n_frag with a list -- sorted by hash, cut where the LIST changes, written into R.  timer: the
// group the launches report under.  d_weight == NULL: n_c[c] = the fragments of class c; else (shn_abundance_merge: the "fragments" are
// weighted lists) the sum of their weight[].
static int abd_emit_classes(shn_ctx* ctx, ShnDevBufs& bufs, int timer, uint64_t n_frag, uint64_t mapped, uint64_t n_place, const uint64_t* d_off,
                            const uint32_t* d_ids, const uint32_t* d_nuniq, uint64_t* d_key, uint64_t* d_key_tmp, uint32_t* d_frag, uint32_t* d_frag_tmp,
                            const uint64_t* d_weight, shn_abundance* R) {
  hipStream_t s = ctx->stream;
  uint32_t *d_head = nullptr, *d_size = nullptr, *d_members = nullptr;
  uint64_t *d_head_scan = nullptr, *d_first = nullptr, *d_class_off = nullptr, *d_nc = nullptr;
  uint64_t n_classes = 0, n_entries = 0;
  HIP_TRY(bufs.get(&d_head, mapped * 4));
  HIP_TRY(bufs.get(&d_head_scan, (mapped + 1) * 8));
  {
    TimerRegion treg(ctx, timer);
    // bytes: 8 sort passes over (key, fragment) pairs (24 B a pair and pass), then per mapped fragment its list and its predecessor's
    // (8 B a member at the most: n_place bounds both), ids, counts, offsets (32 B) and the flag (4 B)
    treg.bytes(8 * n_frag * 24 + mapped * 36 + n_place * 8);
    int rc = shn_sort_pairs(ctx, d_key, d_frag, d_key_tmp, d_frag_tmp, n_frag, 0, 64);
    if (rc) return rc;
    hipLaunchKernelGGL(abd_heads_kernel, dim3((uint32_t)cdiv(mapped, 256)), dim3(256), 0, s, mapped, d_frag, d_off, d_nuniq, d_ids, d_head);
    // the scan of the head flags: a flag read, a number written (12 B a mapped fragment)
    treg.bytes(mapped * 12);
    rc = shn_device_scan_u32(ctx, d_head, mapped, d_head_scan, &n_classes);
    if (rc) return rc;
  }
  HIP_TRY(bufs.get(&d_first, (n_classes + 1) * 8));
  HIP_TRY(bufs.get(&d_size, n_classes * 4));
  HIP_TRY(bufs.get(&d_class_off, (n_classes + 1) * 8));
  HIP_TRY(bufs.get(&d_nc, n_classes * 8));
  {
    TimerRegion treg(ctx, timer);
    // bytes: a mapped fragment's flag (4 B); a head's number and fragment read, its count read, first and size written (28 B a
    // class); the scan of the sizes (12 B a class)
    treg.bytes(mapped * 4 + n_classes * 40);
    hipLaunchKernelGGL(abd_first_kernel, dim3((uint32_t)cdiv(mapped, 256)), dim3(256), 0, s, mapped, n_classes, d_head, d_head_scan, d_frag, d_nuniq,
                       d_first, d_size);
    int rc = shn_device_scan_u32(ctx, d_size, n_classes, d_class_off, &n_entries);
    if (rc) return rc;
  }
  HIP_TRY(bufs.get(&d_members, (n_entries + 1) * 4));
  {
    TimerRegion treg(ctx, timer);
    // bytes: per class head, fragment, three offsets read, its count written (52 B); a member read and written (8 B)
    treg.bytes(mapped * 16 + n_classes * 52 + n_entries * 8);
    hipLaunchKernelGGL(abd_members_kernel, dim3((uint32_t)cdiv(n_classes, 256)), dim3(256), 0, s, n_classes, d_first, d_frag, d_off, d_ids, d_class_off,
                       d_members, d_nc);
    if (d_weight) {
      // bytes: per list its index and weight read (12 B); per class two positions read, the sum written (24 B)
      treg.bytes(mapped * 12 + n_classes * 24);
      hipLaunchKernelGGL(abd_weights_kernel, dim3((uint32_t)cdiv(n_classes, FFP_BLOCK / 64)), dim3(FFP_BLOCK), 0, s, n_classes, d_first, d_frag, d_weight,
                         d_nc);
    }
  }
  R->class_off.resize(n_classes + 1);
  R->n_c.resize(n_classes);
  R->members.resize(n_entries);
  HIP_TRY(hipMemcpyAsync(R->class_off.data(), d_class_off, (n_classes + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(R->n_c.data(), d_nc, n_classes * 8, hipMemcpyDeviceToHost, s));
  if (n_entries) HIP_TRY(hipMemcpyAsync(R->members.data(), d_members, n_entries * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  return SHN_OK;
}

// ---- the host side of map + classes, for read pairs and for single reads
// what an entry point's count and fill launches are handed
struct AbdMap {
  hipStream_t s;
  uint32_t grid;
  FfpIndex I;
  FfpSet A, B;                          // (B: pairs only)
  uint64_t n;                           // fragments
  int ss;
  uint32_t *best, *cnt, *flag, *ids, *nuniq, *frag;
  uint64_t *off, *key;
  unsigned long long *hist, *mapped;    // (hist: n_bins of them; none: NULL)
};

// The classes of the n fragments of r1 (single reads: r2 == NULL) or (r1, r2) (mates, r1->n_reads == r2->n_reads) on the transcripts,
// under the caller's name fn: the refusals, the index over one partition, count -> scan -> fill, the classes, *out.  n_bins: the bins of
// the span histogram count() fills (0: none, the handle reports 0 bins); many / one: what the messages call the fragments; count(M) and
// fill(M) launch the entry point's two kernels on M.grid blocks of FFP_BLOCK.
template <class Count, class Fill>
static int abd_classes_run(const std::string& fn, shn_ctx* ctx, const uint8_t* text, const uint64_t* t_off, uint64_t n_tr, const shn_reads* r1,
                           const shn_reads* r2, int strand_specific, uint64_t n_bins, const char* many, const char* one, Count&& count, Fill&& fill,
                           shn_abundance** out) {
  if (n_tr >= 0xFFFFFFFFULL) return shn_fail(SHN_ERR_OVERFLOW, fn + ": too many transcripts");
  const uint64_t n_frag = r1->n_reads;
  if (n_frag >= 0xFFFFFFFEULL) return shn_fail(SHN_ERR_OVERFLOW, fn + ": too many " + many + " in one call");
  std::vector<uint64_t> rec_off;
  if (int rc = ffp_record_offsets(fn, t_off, n_tr, &rec_off)) return rc;
  const uint64_t total = t_off[n_tr], n_rec = rec_off[n_tr];
  if (total >= 0xFFFFFF00ULL) return shn_fail(SHN_ERR_OVERFLOW, fn + ": more than 2^32 transcript bases in one call");
  shn_abundance* R = new shn_abundance();
  R->n_tr = n_tr; R->n_frag = n_frag;
  R->hist.assign((size_t)n_bins, 0);
  R->class_off.assign(1, 0);
  struct Guard { shn_abundance* p; ~Guard() { delete p; } } guard{R};
  auto done = [&]() { *out = R; guard.p = nullptr; return SHN_OK; };
  if (n_rec == 0 || n_frag == 0) return done();
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);

  // ---- index (all transcripts in partition 0)
  AbdMap M{};
  M.s = s; M.n = n_frag; M.ss = strand_specific ? 1 : 0; M.grid = (uint32_t)cdiv(n_frag, FFP_BLOCK);
  uint64_t n_tw = 0;
  {
    std::vector<uint32_t> t_part(n_tr, 0);
    int rc = ffp_index_build(fn, ctx, bufs, T_ABD_INDEX, text, t_off, t_part.data(), n_tr, 1, rec_off, &M.I, &n_tw);
    if (rc) return rc;
  }

  // ---- map: minimum cost + placements per fragment (+ span histogram), scan, lists
  uint32_t* d_frag_tmp = nullptr;
  uint64_t* d_key_tmp = nullptr;
  HIP_TRY(bufs.get(&M.best, n_frag * 4));
  HIP_TRY(bufs.get(&M.cnt, n_frag * 4));
  HIP_TRY(bufs.get(&M.flag, 4));
  HIP_TRY(bufs.get(&M.off, (n_frag + 1) * 8));
  HIP_TRY(bufs.get(&M.mapped, 8));
  HIP_TRY(hipMemsetAsync(M.flag, 0, 4, s));
  HIP_TRY(hipMemsetAsync(M.mapped, 0, 8, s));
  if (n_bins) {
    HIP_TRY(bufs.get(&M.hist, n_bins * 8));
    HIP_TRY(hipMemsetAsync(M.hist, 0, n_bins * 8, s));
  }
  uint64_t rc_bytes = 0, n_place = 0;
  const uint64_t per_frag = (r1->n_words + (r2 ? r2->n_words : 0)) * 8 / n_frag * (strand_specific ? 1 : 2);
  {
    TimerRegion treg(ctx, T_ABD_MAP);
    int rc = ffp_set(ctx, bufs, r1, !strand_specific, &M.A, &rc_bytes);
    if (!rc && r2) rc = ffp_set(ctx, bufs, r2, true, &M.B, &rc_bytes);
    if (rc) return rc;
    // bytes: the read or both mates of every fragment in each orientation used (2 bits a base), minimum cost and count written (8 B);
    // the index and the text are re-read from the caches and priced once; a block's non-empty bins (at most 8 B each, not priced);
    // what the reverse complements cost is added above
    treg.bytes(rc_bytes + n_frag * (per_frag + 8) + n_rec * 12 + n_tw * 8);
    count(M);
    // the scan of the numbers: a count read, an offset written (12 B a fragment)
    treg.bytes(n_frag * 12);
    rc = shn_device_scan_u32(ctx, M.cnt, n_frag, M.off, &n_place);             // (synchronises)
    if (rc) return rc;
  }
  uint32_t flag = 0;
  unsigned long long mapped = 0;
  HIP_TRY(hipMemcpyAsync(&flag, M.flag, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&mapped, M.mapped, 8, hipMemcpyDeviceToHost, s));
  if (n_bins) HIP_TRY(hipMemcpyAsync(R->hist.data(), M.hist, n_bins * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  if (flag) return shn_fail(SHN_ERR_OVERFLOW, fn + ": " + one + " has 2^32 or more placements of its minimum cost");
  if (n_place >= 0xFFFFFFFFULL) return shn_fail(SHN_ERR_OVERFLOW, fn + ": " + std::to_string(n_place) + " placements in one call (2^32 - 1 at most)");
  R->mapped = mapped;
  if (mapped == 0) return done();
  HIP_TRY(bufs.get(&M.ids, (n_place + 1) * 4));
  HIP_TRY(bufs.get(&M.nuniq, n_frag * 4));
  HIP_TRY(bufs.get(&M.key, (n_frag + 1) * 8));
  HIP_TRY(bufs.get(&d_key_tmp, (n_frag + 1) * 8));
  HIP_TRY(bufs.get(&M.frag, (n_frag + 1) * 4));
  HIP_TRY(bufs.get(&d_frag_tmp, (n_frag + 1) * 4));
  {
    TimerRegion treg(ctx, T_ABD_MAP);
    // bytes: the reads again, cost and two offsets read (20 B), the ids written, sorted in place and read for the hash (12 B a
    // placement), count, key and fragment id written (16 B)
    treg.bytes(n_frag * (per_frag + 36) + n_place * 12 + n_rec * 12 + n_tw * 8);
    fill(M);
  }
  // ---- classes
  if (int rc = abd_emit_classes(ctx, bufs, T_ABD_CLASSES, n_frag, mapped, n_place, M.off, M.ids, M.nuniq, M.key, d_key_tmp, M.frag, d_frag_tmp, nullptr, R))
    return rc;
  return done();
}

// Classes of the read pairs of two resident sets on the final transcripts (kallisto's pseudoalignment, `kallisto quant`,
// filter_kallisto.py:29, replaced by DESIGN.md 3.10 rules 1-3).
extern "C" int shn_abundance_classes(shn_ctx* ctx, const uint8_t* text, const uint64_t* t_off, uint64_t n_tr, const shn_reads* r1, const shn_reads* r2,
                                     int strand_specific, uint32_t max_span, shn_abundance** out) {
  const std::string fn("shn_abundance_classes");
  if (!ctx || !r1 || !r2 || !t_off || !out || (n_tr && !text)) return shn_fail(SHN_ERR_ARG, fn + ": NULL argument");
  if (r1->n_reads != r2->n_reads) return shn_fail(SHN_ERR_ARG, fn + ": the two read sets are not mates of each other (different sizes)");
  if (max_span > ABD_MAX_SPAN) return shn_fail(SHN_ERR_ARG, fn + ": max_span " + std::to_string(max_span) + " above the " + std::to_string(ABD_MAX_SPAN) +
                                                                " bins the span histogram holds");
  const uint64_t n_bins = (uint64_t)max_span + 1;
  return abd_classes_run(
      fn, ctx, text, t_off, n_tr, r1, r2, strand_specific, n_bins, "read pairs", "a fragment",
      [&](const AbdMap& M) {
        hipLaunchKernelGGL(abd_count_kernel, dim3(M.grid), dim3(FFP_BLOCK), n_bins * 4, M.s, M.I, M.A, M.B, M.n, M.ss, max_span, M.best, M.cnt, M.hist, M.mapped,
                           M.flag);
      },
      [&](const AbdMap& M) {
        hipLaunchKernelGGL(abd_fill_kernel, dim3(M.grid), dim3(FFP_BLOCK), 0, M.s, M.I, M.A, M.B, M.n, M.ss, max_span, M.best, M.off, M.ids, M.nuniq, M.key,
                           M.frag);
      },
      out);
}

// Classes of the single reads of one resident set on the transcripts (`kallisto quant --single`, filter_kallisto.py:25, replaced by
// DESIGN.md 3.13 rule 1 and 3.10 rule 3).  No span, so no histogram: the handle reports 0 bins.
extern "C" int shn_abundance_classes_single(shn_ctx* ctx, const uint8_t* text, const uint64_t* t_off, uint64_t n_tr, const shn_reads* r, int strand_specific,
                                            shn_abundance** out) {
  const std::string fn("shn_abundance_classes_single");
  if (!ctx || !r || !t_off || !out || (n_tr && !text)) return shn_fail(SHN_ERR_ARG, fn + ": NULL argument");
  return abd_classes_run(
      fn, ctx, text, t_off, n_tr, r, nullptr, strand_specific, 0, "reads", "a read",
      [](const AbdMap& M) {
        hipLaunchKernelGGL(abd_count_single_kernel, dim3(M.grid), dim3(FFP_BLOCK), 0, M.s, M.I, M.A, M.n, M.ss, M.best, M.cnt, M.mapped, M.flag);
      },
      [](const AbdMap& M) {
        hipLaunchKernelGGL(abd_fill_single_kernel, dim3(M.grid), dim3(FFP_BLOCK), 0, M.s, M.I, M.A, M.n, M.ss, M.best, M.off, M.ids, M.nuniq, M.key, M.frag);
      },
      out);
}

// ---- merge: the classes of several read sets on the same transcripts, given as one CSR of weighted lists, become the
// classes of the union of the reads.  A list takes the place abd_emit_classes gives a fragment: off = class_off, ids = members.
// list i: nuniq[i] = its length, key[i] = the low hash_bits bits of the key abd_finish_list gives the same list, frag[i] = i
__global__ void abd_list_keys_kernel(uint64_t n_lists, const uint64_t* __restrict__ off, const uint32_t* __restrict__ ids, uint64_t mask,
                                     uint32_t* __restrict__ nuniq, uint64_t* __restrict__ key, uint32_t* __restrict__ frag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_lists) return;
  const uint64_t o = off[i], u = off[i + 1] - o;
  uint64_t h = abd_mix(0, u);
  for (uint64_t p = 0; p < u; p++) h = abd_mix(h, ids[o + p]);
  nuniq[i] = (uint32_t)u;
  key[i] = (h >> 1) & mask;
  frag[i] = (uint32_t)i;
}

// the refusals of shn_abundance_merge, before anything is launched; *total = the sum of the weights
static int abd_merge_check(const std::string& fn, const uint64_t* class_off, const uint32_t* members, const uint64_t* n_c, uint64_t n_lists, uint64_t m,
                           uint32_t hash_bits, uint64_t* total) {
  if (m == 0) return shn_fail(SHN_ERR_ARG, fn + ": no transcripts (m is 0)");
  if (hash_bits < 1 || hash_bits > 63) return shn_fail(SHN_ERR_ARG, fn + ": hash_bits " + std::to_string(hash_bits) + " outside 1 .. 63");
  if (!class_off || (n_lists && !n_c)) return shn_fail(SHN_ERR_ARG, fn + ": NULL argument");
  if (m >= 0xFFFFFFFFULL) return shn_fail(SHN_ERR_OVERFLOW, fn + ": too many transcripts");
  if (n_lists >= (1ULL << 32)) return shn_fail(SHN_ERR_OVERFLOW, fn + ": 2^32 or more lists (the sort carries a list's index in 32 bits)");
  if (class_off[0] != 0) return shn_fail(SHN_ERR_ARG, fn + ": class_off[0] is not 0");
  for (uint64_t c = 0; c < n_lists; c++) {
    if (class_off[c + 1] < class_off[c]) return shn_fail(SHN_ERR_ARG, fn + ": class_off not monotone");
    if (class_off[c + 1] == class_off[c]) return shn_fail(SHN_ERR_ARG, fn + ": list " + std::to_string(c) + " is empty");
  }
  const uint64_t n_entries = class_off[n_lists];
  if (n_entries >= 0xFFFFFFFFULL) return shn_fail(SHN_ERR_OVERFLOW, fn + ": too many list members");
  if (n_entries && !members) return shn_fail(SHN_ERR_ARG, fn + ": NULL argument");
  for (uint64_t c = 0; c < n_lists; c++)
    for (uint64_t e = class_off[c]; e < class_off[c + 1]; e++) {
      if (members[e] >= m) return shn_fail(SHN_ERR_ARG, fn + ": a list names transcript " + std::to_string(members[e]) + " of " + std::to_string(m));
      if (e > class_off[c] && members[e] <= members[e - 1]) return shn_fail(SHN_ERR_ARG, fn + ": list " + std::to_string(c) + " is not strictly ascending");
    }
  uint64_t sum = 0;
  for (uint64_t c = 0; c < n_lists; c++)
    if (__builtin_add_overflow(sum, n_c[c], &sum)) return shn_fail(SHN_ERR_OVERFLOW, fn + ": the weights' sum does not fit in 64 bits");
  *total = sum;
  return SHN_OK;
}

// The classes of the union of several read sets from the sets' own classes: integers only.
extern "C" int shn_abundance_merge(shn_ctx* ctx, const uint64_t* class_off, const uint32_t* members, const uint64_t* n_c, uint64_t n_lists, uint64_t m,
                                   uint32_t hash_bits, shn_abundance** out) {
  const std::string fn("shn_abundance_merge");
  uint64_t total = 0;
  if (int rc = abd_merge_check(fn, class_off, members, n_c, n_lists, m, hash_bits, &total)) return rc;
  if (!ctx || !out) return shn_fail(SHN_ERR_ARG, fn + ": NULL argument");
  shn_abundance* R = new shn_abundance();
  R->n_tr = m; R->n_frag = total; R->mapped = total;
  R->class_off.assign(1, 0);
  struct Guard { shn_abundance* p; ~Guard() { delete p; } } guard{R};
  auto done = [&]() { *out = R; guard.p = nullptr; return SHN_OK; };
  if (n_lists == 0) return done();
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  const uint64_t n_entries = class_off[n_lists];
  uint64_t *d_off = nullptr, *d_w = nullptr, *d_key = nullptr, *d_key_tmp = nullptr;
  uint32_t *d_ids = nullptr, *d_nuniq = nullptr, *d_frag = nullptr, *d_frag_tmp = nullptr;
  HIP_TRY(bufs.get(&d_off, (n_lists + 1) * 8));
  HIP_TRY(bufs.get(&d_ids, (n_entries + 1) * 4));
  HIP_TRY(bufs.get(&d_w, n_lists * 8));
  HIP_TRY(bufs.get(&d_nuniq, n_lists * 4));
  HIP_TRY(bufs.get(&d_key, (n_lists + 1) * 8));
  HIP_TRY(bufs.get(&d_key_tmp, (n_lists + 1) * 8));
  HIP_TRY(bufs.get(&d_frag, (n_lists + 1) * 4));
  HIP_TRY(bufs.get(&d_frag_tmp, (n_lists + 1) * 4));
  HIP_TRY(hipMemcpyAsync(d_off, class_off, (n_lists + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_ids, members, n_entries * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_w, n_c, n_lists * 8, hipMemcpyHostToDevice, s));
  {
    TimerRegion treg(ctx, T_ABD_MERGE);
    // bytes: per list two offsets read, length, key and index written (32 B); a member read for the hash (4 B)
    treg.bytes(n_lists * 32 + n_entries * 4);
    hipLaunchKernelGGL(abd_list_keys_kernel, dim3((uint32_t)cdiv(n_lists, 256)), dim3(256), 0, s, n_lists, d_off, d_ids, (~0ULL) >> (64 - hash_bits), d_nuniq,
                       d_key, d_frag);
  }
  if (int rc = abd_emit_classes(ctx, bufs, T_ABD_MERGE, n_lists, n_lists, n_entries, d_off, d_ids, d_nuniq, d_key, d_key_tmp, d_frag, d_frag_tmp, d_w, R))
    return rc;
  return done();
}

extern "C" int shn_abundance_sizes(const shn_abundance* a, uint64_t* sizes) {
  if (!a || !sizes) return shn_fail(SHN_ERR_ARG, "shn_abundance_sizes: NULL argument");
  sizes[0] = a->n_tr; sizes[1] = a->n_frag; sizes[2] = a->mapped; sizes[3] = a->n_c.size(); sizes[4] = a->members.size(); sizes[5] = a->hist.size();
  return SHN_OK;
}

extern "C" int shn_abundance_export(const shn_abundance* a, uint64_t* class_off, uint32_t* members, uint64_t* n_c, uint64_t* hist) {
  if (!a || !class_off || (a->hist.size() && !hist) || (a->n_c.size() && !n_c) || (a->members.size() && !members))
    return shn_fail(SHN_ERR_ARG, "shn_abundance_export: NULL argument");
  std::copy(a->class_off.begin(), a->class_off.end(), class_off);
  std::copy(a->members.begin(), a->members.end(), members);
  std::copy(a->n_c.begin(), a->n_c.end(), n_c);
  std::copy(a->hist.begin(), a->hist.end(), hist);
  return SHN_OK;
}

extern "C" void shn_abundance_destroy(shn_abundance* a) { delete a; }

// ------------------------------------------------------------------------------------------------------------------------ EM
// DESIGN.md 3.10 rule 4.  The refusals (abd_em_check) and the classes on the device with their transposition (abd_em_setup) are shared
// by shn_abundance_em -- one count vector, kernels of its own: abd_em_* -- and the batched EM of the bootstrap replicates (DESIGN.md
// 3.14 rule 2: abd_emb_*, the same loops with a slot index).  tests/golden/abundance_em_bits.json pins both to the same bits.

// the sum of a wave's partial sums in lane 0: strides 32, 16, 8, 4, 2, 1, lane l takes lane l + stride
__device__ __forceinline__ double abd_wave_sum(double x) {
  for (int off = 32; off; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

// entry e of the classes' CSR: key = its transcript, value = e; cls[e] = its class (the last c with class_off[c] <= e)
__global__ void abd_entries_kernel(uint64_t n_entries, uint64_t n_classes, const uint64_t* __restrict__ class_off, const uint32_t* __restrict__ members,
                                   uint64_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t* __restrict__ cls) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_entries) return;
  key[e] = members[e];
  val[e] = (uint32_t)e;
  cls[e] = (uint32_t)shn_segment_of(class_off, n_classes, e);
}

// the transposed CSR from the sorted entries: tr_off[j] = first sorted entry of transcript j (j = m: all), tr_cls[k] = class of the k-th
__global__ void abd_transpose_kernel(uint64_t n_entries, uint64_t m, const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
                                     const uint32_t* __restrict__ cls, uint64_t* __restrict__ tr_off, uint32_t* __restrict__ tr_cls) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_entries) tr_cls[t] = cls[val[t]];
  if (t <= m) tr_off[t] = shn_lower_bound(key, n_entries, t);
}

// the refusals every EM entry point shares, under the caller's name
static int abd_em_check(const std::string& fn, const uint64_t* class_off, const uint32_t* members, uint64_t n_classes, const double* eff, uint64_t m) {
  if (m == 0) return shn_fail(SHN_ERR_ARG, fn + ": no transcripts (m is 0)");
  if (!class_off || !eff) return shn_fail(SHN_ERR_ARG, fn + ": NULL argument");
  if (m >= 0xFFFFFFFFULL || n_classes >= 0xFFFFFFFFULL) return shn_fail(SHN_ERR_OVERFLOW, fn + ": too many transcripts or classes");
  if (class_off[0] != 0) return shn_fail(SHN_ERR_ARG, fn + ": class_off[0] is not 0");
  for (uint64_t c = 0; c < n_classes; c++)
    if (class_off[c + 1] < class_off[c]) return shn_fail(SHN_ERR_ARG, fn + ": class_off not monotone");
  const uint64_t n_entries = class_off[n_classes];
  if (n_entries >= 0xFFFFFFFFULL) return shn_fail(SHN_ERR_OVERFLOW, fn + ": too many class members");
  if (n_entries && !members) return shn_fail(SHN_ERR_ARG, fn + ": NULL argument");
  for (uint64_t e = 0; e < n_entries; e++)
    if (members[e] >= m) return shn_fail(SHN_ERR_ARG, fn + ": a class names transcript " + std::to_string(members[e]) + " of " + std::to_string(m));
  for (uint64_t j = 0; j < m; j++)
    if (!(eff[j] > 0.0)) return shn_fail(SHN_ERR_ARG, fn + ": eff of transcript " + std::to_string(j) + " is not above 0");
  return SHN_OK;
}

// the classes, their transposition and eff on the device: what every replicate shares
struct AbdEmDev {
  uint64_t n_classes = 0, n_entries = 0, m = 0;
  uint64_t *coff = nullptr, *troff = nullptr;
  uint32_t *mem = nullptr, *trcls = nullptr;
  double* eff = nullptr;
};

// timer: the slot the caller reports under, T_ABD_EM or T_ABD_EM_BATCH; then(region): what the caller launches in the same region
template <class Then>
static int abd_em_setup(shn_ctx* ctx, ShnDevBufs& bufs, int timer, const uint64_t* class_off, const uint32_t* members, uint64_t n_classes,
                        const double* eff, uint64_t m, AbdEmDev* E, Then&& then) {
  hipStream_t s = ctx->stream;
  const uint64_t n_entries = class_off[n_classes];
  E->n_classes = n_classes; E->n_entries = n_entries; E->m = m;
  uint64_t *d_key = nullptr, *d_key_tmp = nullptr;
  uint32_t *d_val = nullptr, *d_val_tmp = nullptr, *d_cls = nullptr;
  HIP_TRY(bufs.get(&E->coff, (n_classes + 1) * 8));
  HIP_TRY(bufs.get(&E->mem, (n_entries + 1) * 4));
  HIP_TRY(bufs.get(&E->eff, m * 8));
  HIP_TRY(bufs.get(&E->troff, (m + 1) * 8));
  HIP_TRY(bufs.get(&E->trcls, (n_entries + 1) * 4));
  HIP_TRY(bufs.get(&d_key, (n_entries + 1) * 8));
  HIP_TRY(bufs.get(&d_key_tmp, (n_entries + 1) * 8));
  HIP_TRY(bufs.get(&d_val, (n_entries + 1) * 4));
  HIP_TRY(bufs.get(&d_val_tmp, (n_entries + 1) * 4));
  HIP_TRY(bufs.get(&d_cls, (n_entries + 1) * 4));
  HIP_TRY(hipMemcpyAsync(E->coff, class_off, (n_classes + 1) * 8, hipMemcpyHostToDevice, s));
  if (n_entries) HIP_TRY(hipMemcpyAsync(E->mem, members, n_entries * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(E->eff, eff, m * 8, hipMemcpyHostToDevice, s));
  int key_bits = 1;
  while (key_bits < 32 && (m >> key_bits)) key_bits++;
  TimerRegion treg(ctx, timer);
  // bytes, the transposition (once for all replicates): an entry read (4 B + its class's offsets from the caches) and written as key,
  // value, class (16 B), every sort pass reads and writes the pairs (24 B), the sorted entry's class gathered and written (12 B); 8 B a
  // transcript offset
  treg.bytes(n_entries * (32 + 24 * (uint64_t)((key_bits + 7) / 8)) + (m + 1) * 8);
  if (n_entries) {
    hipLaunchKernelGGL(abd_entries_kernel, dim3((uint32_t)cdiv(n_entries, 256)), dim3(256), 0, s, n_entries, n_classes, E->coff, E->mem, d_key, d_val, d_cls);
    int rc = shn_sort_pairs(ctx, d_key, d_val, d_key_tmp, d_val_tmp, n_entries, 0, key_bits);
    if (rc) return rc;
  }
  const uint64_t n_t = n_entries > m + 1 ? n_entries : m + 1;
  hipLaunchKernelGGL(abd_transpose_kernel, dim3((uint32_t)cdiv(n_t, 256)), dim3(256), 0, s, n_entries, m, d_key, d_val, d_cls, E->troff, E->trcls);
  then(treg);
  return SHN_OK;
}

__global__ void abd_em_init_kernel(uint64_t m, const double* __restrict__ eff, double* __restrict__ alpha, double* __restrict__ w) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const double a = 1.0 / (double)m;
  alpha[j] = a;
  w[j] = a / eff[j];
}

// d_c = sum over the members of class c of w_j = alpha_j / eff_j: a wave a class
__global__ __launch_bounds__(FFP_BLOCK) void abd_em_d_kernel(uint64_t n_classes, const uint64_t* __restrict__ class_off, const uint32_t* __restrict__ members,
                                                             const double* __restrict__ w, double* __restrict__ d) {
  const uint64_t c = (uint64_t)blockIdx.x * (FFP_BLOCK / 64) + (threadIdx.x >> 6);
  if (c >= n_classes) return;                               // (the whole wave)
  const uint32_t lane = threadIdx.x & 63;
  double x = 0.0;
  for (uint64_t e = class_off[c] + lane, end = class_off[c + 1]; e < end; e += 64) x += w[members[e]];
  x = abd_wave_sum(x);
  if (lane == 0) d[c] = x;
}

// alpha'_j = sum over the classes c of transcript j of n_c w_j / d_c (a class with d_c == 0 gives nothing): a wave a transcript.
// check != 0: *moved is raised when alpha'_j > 1e-2 and |alpha'_j - alpha_j| > 1e-2 alpha'_j.  alpha and w are replaced in place: a
// wave reads and writes its own transcript's only.
__global__ __launch_bounds__(FFP_BLOCK) void abd_em_alpha_kernel(uint64_t m, const uint64_t* __restrict__ tr_off, const uint32_t* __restrict__ tr_cls,
                                                                 const double* __restrict__ n_c, const double* __restrict__ d,
                                                                 const double* __restrict__ eff, double* __restrict__ alpha, double* __restrict__ w,
                                                                 int check, uint32_t* __restrict__ moved) {
  const uint64_t j = (uint64_t)blockIdx.x * (FFP_BLOCK / 64) + (threadIdx.x >> 6);
  if (j >= m) return;                                       // (the whole wave)
  const uint32_t lane = threadIdx.x & 63;
  const double wj = w[j];
  double x = 0.0;
  for (uint64_t t = tr_off[j] + lane, end = tr_off[j + 1]; t < end; t += 64) {
    const uint32_t c = tr_cls[t];
    const double dc = d[c];
    if (dc != 0.0) x += n_c[c] * wj / dc;
  }
  x = abd_wave_sum(x);
  if (lane == 0) {
    const double old = alpha[j];
    alpha[j] = x;
    w[j] = x / eff[j];
    if (check && x > 1e-2 && fabs(x - old) > 1e-2 * x) *moved = 1u;
  }
}

// The EM of `kallisto quant` (filter_kallisto.py:29) on classes given as host arrays: DESIGN.md 3.10 rule 4.
extern "C" int shn_abundance_em(shn_ctx* ctx, const uint64_t* class_off, const uint32_t* members, const uint64_t* n_c, uint64_t n_classes,
                                const double* eff, uint64_t m, double* alpha, uint32_t* rounds) {
  const std::string fn("shn_abundance_em");
  if (int rc = abd_em_check(fn, class_off, members, n_classes, eff, m)) return rc;
  if (!ctx || !alpha || !rounds || (n_classes && !n_c)) return shn_fail(SHN_ERR_ARG, fn + ": NULL argument");
  std::vector<double> ncd(n_classes);
  for (uint64_t c = 0; c < n_classes; c++) ncd[c] = (double)n_c[c];
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  uint32_t* d_moved = nullptr;
  double *d_nc = nullptr, *d_alpha = nullptr, *d_w = nullptr, *d_d = nullptr;
  HIP_TRY(bufs.get(&d_nc, (n_classes + 1) * 8));
  HIP_TRY(bufs.get(&d_alpha, m * 8));
  HIP_TRY(bufs.get(&d_w, m * 8));
  HIP_TRY(bufs.get(&d_d, (n_classes + 1) * 8));
  HIP_TRY(bufs.get(&d_moved, 4));
  if (n_classes) HIP_TRY(hipMemcpyAsync(d_nc, ncd.data(), n_classes * 8, hipMemcpyHostToDevice, s));
  AbdEmDev E;
  int rc = abd_em_setup(ctx, bufs, T_ABD_EM, class_off, members, n_classes, eff, m, &E, [&](TimerRegion& treg) {
    treg.bytes(m * 24);                                       // alpha and w written, eff read
    hipLaunchKernelGGL(abd_em_init_kernel, dim3((uint32_t)cdiv(m, 256)), dim3(256), 0, s, m, E.eff, d_alpha, d_w);
  });
  if (rc) return rc;
  const uint64_t n_entries = E.n_entries;
  const uint32_t waves = FFP_BLOCK / 64;
  uint32_t round = 0;
  for (;;) {                                                  // a block of 50 rounds, the last of them with the test; one read of the flag
    HIP_TRY(hipMemsetAsync(d_moved, 0, 4, s));
    {
      TimerRegion treg(ctx, T_ABD_EM);
      // bytes of a round: d pass -- two offsets a class (16 B), a member and its w (12 B an entry), d written (8 B a class); alpha pass
      // -- two offsets, w, alpha, eff read, alpha and w written (56 B a transcript), class, n_c and d of an entry (20 B)
      treg.bytes(50 * (n_classes * 24 + n_entries * 32 + m * 56));
      for (int k = 0; k < 50; k++) {
        if (n_classes)
          hipLaunchKernelGGL(abd_em_d_kernel, dim3((uint32_t)cdiv(n_classes, waves)), dim3(FFP_BLOCK), 0, s, n_classes, E.coff, E.mem, d_w, d_d);
        hipLaunchKernelGGL(abd_em_alpha_kernel, dim3((uint32_t)cdiv(m, waves)), dim3(FFP_BLOCK), 0, s, m, E.troff, E.trcls, d_nc, d_d, E.eff, d_alpha, d_w,
                           k == 49 ? 1 : 0, d_moved);
      }
    }
    round += 50;
    uint32_t moved = 0;
    HIP_TRY(hipMemcpyAsync(&moved, d_moved, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    if (!moved || round >= 10000) break;
  }
  HIP_TRY(hipMemcpyAsync(alpha, d_alpha, m * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  for (uint64_t j = 0; j < m; j++)
    if (alpha[j] < 1e-8) alpha[j] = 0.0;
  *rounds = round;
  return SHN_OK;
}

// ----------------------------------------------------------------------------------------------------------------- bootstrap
// quant -b B --seed S: B resampled count vectors of the classes, and the EM above on all of them at once.
//
//   resample  replicate b makes N = sum n_c draws; draw t = Philox4x32-10 of counter (t, b, 0, 0) under the key (seed lo, seed hi), u = o0 |
//             o1 << 32, r = the high word of u * N, the class c with cum[c] <= r < cum[c + 1] (shn_segment_of on the exclusive prefix sum:
//             an empty class shares its offset with the next one, which wins -- it is never drawn).  A block takes ABD_RS_DRAWS
//             consecutive draws of one replicate.  Up to ABD_RS_LDS classes it counts them in LDS (32-bit integer atomics) and adds
//             its non-empty bins to counts[b][] (64-bit integer atomics); above that a wave combines its equal destinations (one lane
//             per distinct class adds the number of lanes that drew it) before the global add.  Integers only: the order of the adds
//             does not show.
//   EM        the transposed CSR once, as shn_abundance_em builds it; alpha, w, d and the counts as doubles laid out [slot][row] for the
//             replicates resident at once; a round is ONE d launch and ONE alpha launch over (row x live replicate), blockIdx.y = the
//             position in the list of live slots.  The loops, the shuffle tree and the expressions are those of abd_em_d_kernel /
//             abd_em_alpha_kernel, so a replicate's bits are shn_abundance_em's on its counts.  A moved flag per slot; after 50
//             rounds the host reads the flags once and strikes the replicates that are done from the list.
#define ABD_RS_DRAWS 4096u     // draws a block makes for one replicate (16 a thread)
#define ABD_RS_LDS 8192u       // classes a block counts in LDS (32 KiB of 32-bit bins)
#define ABD_EMB_SLOTS 32768u   // replicates resident at once at the most (blockIdx.y)
#define ABD_EMB_BUDGET (1ULL << 30)   // bytes of alpha, w, d and counts of the resident replicates that max_live == 0 allows

struct AbdPhilox { uint32_t c0, c1, c2, c3; };
__device__ __forceinline__ AbdPhilox abd_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return AbdPhilox{c0, c1, c2, c3};
}

// class of draw t of replicate b
__device__ __forceinline__ uint32_t abd_draw(uint64_t t, uint32_t b, uint32_t k0, uint32_t k1, uint64_t N, const uint64_t* __restrict__ cum,
                                             uint64_t n_classes) {
  const AbdPhilox o = abd_philox((uint32_t)t, b, 0u, 0u, k0, k1);
  const uint64_t u = (uint64_t)o.c0 | (uint64_t)o.c1 << 32;
  return (uint32_t)shn_segment_of(cum, n_classes, __umul64hi(u, N));
}

// work item wi = (replicate wi / chunks, draws [chunk * ABD_RS_DRAWS, ...) of it); LDS: n_classes bins when lds != 0
__global__ __launch_bounds__(FFP_BLOCK) void abd_resample_kernel(uint64_t N, uint64_t n_classes, uint64_t B, uint64_t chunks, uint32_t k0, uint32_t k1,
                                                                 const uint64_t* __restrict__ cum, int lds, unsigned long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t abd_rs[];
  for (uint64_t wi = blockIdx.x; wi < B * chunks; wi += gridDim.x) {
    const uint64_t b = wi / chunks, t0 = (wi - b * chunks) * ABD_RS_DRAWS;
    const uint64_t t1 = t0 + ABD_RS_DRAWS < N ? t0 + ABD_RS_DRAWS : N;
    unsigned long long* out = counts + b * n_classes;
    if (lds) {
      for (uint32_t c = threadIdx.x; c < n_classes; c += FFP_BLOCK) abd_rs[c] = 0;
      __syncthreads();
      for (uint64_t t = t0 + threadIdx.x; t < t1; t += FFP_BLOCK) atomicAdd(&abd_rs[abd_draw(t, (uint32_t)b, k0, k1, N, cum, n_classes)], 1u);
      __syncthreads();
      for (uint32_t c = threadIdx.x; c < n_classes; c += FFP_BLOCK)
        if (abd_rs[c]) atomicAdd(&out[c], (unsigned long long)abd_rs[c]);
      __syncthreads();
    } else {
      for (uint64_t base = t0; base < t1; base += FFP_BLOCK) {          // (the same trip count for every lane of a wave)
        const uint64_t t = base + threadIdx.x;
        const bool on = t < t1;
        const uint32_t c = on ? abd_draw(t, (uint32_t)b, k0, k1, N, cum, n_classes) : 0u;
        unsigned long long todo = __ballot(on);
        const uint32_t lane = threadIdx.x & 63;
        while (todo) {                                                  // one turn per distinct class among the wave's draws
          const int lead = __ffsll((long long)todo) - 1;
          const uint32_t cl = (uint32_t)__shfl((int)c, lead, 64);
          const unsigned long long same = __ballot(on && c == cl) & todo;
          if (lane == (uint32_t)lead) atomicAdd(&out[cl], (unsigned long long)__popcll(same));
          todo &= ~same;
        }
      }
    }
  }
}

// the counts of rule 1 into d_counts[B][n_classes] (device); N = sum n_c < 2^32, B < 2^32 (the callers refuse anything else)
static int abd_resample_run(shn_ctx* ctx, ShnDevBufs& bufs, const uint64_t* n_c, uint64_t n_classes, uint64_t N, uint64_t B, uint64_t seed,
                            unsigned long long* d_counts) {
  hipStream_t s = ctx->stream;
  if (B * n_classes) HIP_TRY(hipMemsetAsync(d_counts, 0, B * n_classes * 8, s));
  if (N == 0 || n_classes == 0) return SHN_OK;
  std::vector<uint64_t> cum(n_classes + 1, 0);
  for (uint64_t c = 0; c < n_classes; c++) cum[c + 1] = cum[c] + n_c[c];
  uint64_t* d_cum = nullptr;
  HIP_TRY(bufs.get(&d_cum, (n_classes + 1) * 8));
  HIP_TRY(hipMemcpyAsync(d_cum, cum.data(), (n_classes + 1) * 8, hipMemcpyHostToDevice, s));
  const uint64_t chunks = cdiv(N, ABD_RS_DRAWS);
  const int lds = n_classes <= ABD_RS_LDS;
  {
    TimerRegion treg(ctx, T_ABD_RESAMPLE);
    // bytes: the draws come from registers; the prefix sum is searched in the caches and priced once; a bin of every replicate is
    // zeroed and, at the least, added to once (16 B)
    treg.bytes((n_classes + 1) * 8 + B * n_classes * 16);
    hipLaunchKernelGGL(abd_resample_kernel, dim3(shn_grid(B * chunks, 1)), dim3(FFP_BLOCK), lds ? n_classes * 4 : 0, s, N, n_classes, B, chunks,
                       (uint32_t)seed, (uint32_t)(seed >> 32), d_cum, lds, d_counts);
  }
  HIP_TRY(hipStreamSynchronize(s));                                     // (cum is a host vector)
  HIP_TRY(hipGetLastError());
  return SHN_OK;
}

// N = sum n_c, refused at 2^32 (and B at 2^32): before anything is launched
static int abd_resample_check(const std::string& fn, const uint64_t* n_c, uint64_t n_classes, uint64_t B, uint64_t* N) {
  if (B == 0) return shn_fail(SHN_ERR_ARG, fn + ": no replicates (B is 0)");
  if (B >= (1ULL << 32)) return shn_fail(SHN_ERR_OVERFLOW, fn + ": 2^32 or more replicates");
  if (n_classes >= 0xFFFFFFFFULL) return shn_fail(SHN_ERR_OVERFLOW, fn + ": too many classes");
  uint64_t n = 0;
  for (uint64_t c = 0; c < n_classes; c++) {
    if (n_c[c] >= (1ULL << 32) || n + n_c[c] >= (1ULL << 32)) return shn_fail(SHN_ERR_OVERFLOW, fn + ": 2^32 or more fragments in the classes");
    n += n_c[c];
  }
  *N = n;
  return SHN_OK;
}

extern "C" int shn_abundance_resample(shn_ctx* ctx, const uint64_t* n_c, uint64_t n_classes, uint64_t B, uint64_t seed, uint64_t* counts_out) {
  const std::string fn("shn_abundance_resample");
  if (!ctx || (n_classes && (!n_c || !counts_out))) return shn_fail(SHN_ERR_ARG, fn + ": NULL argument");
  uint64_t N = 0;
  if (int rc = abd_resample_check(fn, n_c, n_classes, B, &N)) return rc;
  if (n_classes == 0) return SHN_OK;
  if (N == 0) { std::fill(counts_out, counts_out + B * n_classes, 0ULL); return SHN_OK; }
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  unsigned long long* d_counts = nullptr;
  HIP_TRY(bufs.get(&d_counts, B * n_classes * 8));
  if (int rc = abd_resample_run(ctx, bufs, n_c, n_classes, N, B, seed, d_counts)) return rc;
  HIP_TRY(hipMemcpyAsync(counts_out, d_counts, B * n_classes * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  return SHN_OK;
}

// ---- the batched EM
// slot s < n_slots: the counts of replicate b0 + s as doubles, alpha = 1 / m, w = alpha / eff
__global__ void abd_emb_init_kernel(uint64_t n_slots, uint64_t m, uint64_t n_classes, const unsigned long long* __restrict__ counts,
                                    const double* __restrict__ eff, double* __restrict__ ncd, double* __restrict__ alpha, double* __restrict__ w) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_slots * n_classes) ncd[i] = (double)counts[i];
  if (i < n_slots * m) {
    const double a = 1.0 / (double)m;
    alpha[i] = a;
    w[i] = a / eff[i % m];
  }
}

// abd_em_d_kernel for the slot live[blockIdx.y]
__global__ __launch_bounds__(FFP_BLOCK) void abd_emb_d_kernel(uint64_t n_classes, uint64_t m, const uint64_t* __restrict__ class_off,
                                                              const uint32_t* __restrict__ members, const uint32_t* __restrict__ live,
                                                              const double* __restrict__ w_all, double* __restrict__ d_all) {
  const uint64_t c = (uint64_t)blockIdx.x * (FFP_BLOCK / 64) + (threadIdx.x >> 6);
  if (c >= n_classes) return;                               // (the whole wave)
  const uint64_t slot = live[blockIdx.y];
  const double* __restrict__ w = w_all + slot * m;
  const uint32_t lane = threadIdx.x & 63;
  double x = 0.0;
  for (uint64_t e = class_off[c] + lane, end = class_off[c + 1]; e < end; e += 64) x += w[members[e]];
  x = abd_wave_sum(x);
  if (lane == 0) d_all[slot * n_classes + c] = x;
}

// abd_em_alpha_kernel for the slot live[blockIdx.y]; check != 0: moved[slot] is raised
__global__ __launch_bounds__(FFP_BLOCK) void abd_emb_alpha_kernel(uint64_t m, uint64_t n_classes, const uint64_t* __restrict__ tr_off,
                                                                  const uint32_t* __restrict__ tr_cls, const uint32_t* __restrict__ live,
                                                                  const double* __restrict__ ncd_all, const double* __restrict__ d_all,
                                                                  const double* __restrict__ eff, double* __restrict__ alpha_all,
                                                                  double* __restrict__ w_all, int check, uint32_t* __restrict__ moved) {
  const uint64_t j = (uint64_t)blockIdx.x * (FFP_BLOCK / 64) + (threadIdx.x >> 6);
  if (j >= m) return;                                       // (the whole wave)
  const uint64_t slot = live[blockIdx.y];
  const double* __restrict__ n_c = ncd_all + slot * n_classes;
  const double* __restrict__ d = d_all + slot * n_classes;
  double* __restrict__ alpha = alpha_all + slot * m;
  double* __restrict__ w = w_all + slot * m;
  const uint32_t lane = threadIdx.x & 63;
  const double wj = w[j];
  double x = 0.0;
  for (uint64_t t = tr_off[j] + lane, end = tr_off[j + 1]; t < end; t += 64) {
    const uint32_t c = tr_cls[t];
    const double dc = d[c];
    if (dc != 0.0) x += n_c[c] * wj / dc;
  }
  x = abd_wave_sum(x);
  if (lane == 0) {
    const double old = alpha[j];
    alpha[j] = x;
    w[j] = x / eff[j];
    if (check && x > 1e-2 && fabs(x - old) > 1e-2 * x) moved[slot] = 1u;
  }
}

// rule 4 for the B count vectors d_counts[B][n_classes] (device) -> alpha_out[B][m], rounds_out[B] (host)
static int abd_em_batch_run(shn_ctx* ctx, ShnDevBufs& bufs, const AbdEmDev& E, const unsigned long long* d_counts, uint64_t B, uint64_t max_live,
                            double* alpha_out, uint32_t* rounds_out) {
  hipStream_t s = ctx->stream;
  const uint64_t m = E.m, n_classes = E.n_classes, n_entries = E.n_entries;
  const uint64_t per_slot = (2 * m + 2 * n_classes) * 8;
  uint64_t L = ABD_EMB_BUDGET / per_slot;
  if (L < 1) L = 1;
  if (L > ABD_EMB_SLOTS) L = ABD_EMB_SLOTS;
  if (max_live && max_live < L) L = max_live;
  if (B < L) L = B;
  double *d_ncd = nullptr, *d_alpha = nullptr, *d_w = nullptr, *d_d = nullptr;
  uint32_t *d_live = nullptr, *d_moved = nullptr;
  HIP_TRY(bufs.get(&d_ncd, (L * n_classes + 1) * 8));
  HIP_TRY(bufs.get(&d_d, (L * n_classes + 1) * 8));
  HIP_TRY(bufs.get(&d_alpha, L * m * 8));
  HIP_TRY(bufs.get(&d_w, L * m * 8));
  HIP_TRY(bufs.get(&d_live, L * 4));
  HIP_TRY(bufs.get(&d_moved, L * 4));
  const uint32_t waves = FFP_BLOCK / 64;
  std::vector<uint32_t> live, moved(L);
  for (uint64_t b0 = 0; b0 < B; b0 += L) {
    const uint64_t n_slots = B - b0 < L ? B - b0 : L;
    live.resize(n_slots);
    for (uint64_t k = 0; k < n_slots; k++) live[k] = (uint32_t)k;
    HIP_TRY(hipMemcpyAsync(d_live, live.data(), n_slots * 4, hipMemcpyHostToDevice, s));
    {
      TimerRegion treg(ctx, T_ABD_EM_BATCH);
      // bytes: a count read and written as a double (16 B a class and replicate), alpha and w written, eff read (24 B a transcript)
      treg.bytes(n_slots * (n_classes * 16 + m * 24));
      const uint64_t n_i = n_slots * (n_classes > m ? n_classes : m);
      hipLaunchKernelGGL(abd_emb_init_kernel, dim3((uint32_t)cdiv(n_i, 256)), dim3(256), 0, s, n_slots, m, n_classes, d_counts + b0 * n_classes, E.eff,
                         d_ncd, d_alpha, d_w);
    }
    uint32_t round = 0;
    while (!live.empty()) {                                   // a block of 50 rounds of the live replicates, the last with the test; one read of the flags
      const uint32_t n_live = (uint32_t)live.size();
      HIP_TRY(hipMemsetAsync(d_moved, 0, n_slots * 4, s));
      {
        TimerRegion treg(ctx, T_ABD_EM_BATCH);
        // bytes of a round and live replicate: as shn_abundance_em prices a round (the members and offsets are shared, and re-read
        // from the caches by every replicate's waves: priced per replicate all the same)
        treg.bytes(50 * (uint64_t)n_live * (n_classes * 24 + n_entries * 32 + m * 56));
        for (int k = 0; k < 50; k++) {
          if (n_classes)
            hipLaunchKernelGGL(abd_emb_d_kernel, dim3((uint32_t)cdiv(n_classes, waves), n_live), dim3(FFP_BLOCK), 0, s, n_classes, m, E.coff, E.mem, d_live,
                               d_w, d_d);
          hipLaunchKernelGGL(abd_emb_alpha_kernel, dim3((uint32_t)cdiv(m, waves), n_live), dim3(FFP_BLOCK), 0, s, m, n_classes, E.troff, E.trcls, d_live,
                             d_ncd, d_d, E.eff, d_alpha, d_w, k == 49 ? 1 : 0, d_moved);
        }
      }
      round += 50;
      HIP_TRY(hipMemcpyAsync(moved.data(), d_moved, n_slots * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      HIP_TRY(hipGetLastError());
      size_t keep = 0;
      for (uint32_t slot : live) {
        if (moved[slot] && round < 10000) live[keep++] = slot;
        else rounds_out[b0 + slot] = round;
      }
      if (keep != live.size()) {
        live.resize(keep);
        if (keep) HIP_TRY(hipMemcpyAsync(d_live, live.data(), keep * 4, hipMemcpyHostToDevice, s));
      }
    }
    HIP_TRY(hipMemcpyAsync(alpha_out + b0 * m, d_alpha, n_slots * m * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
  }
  for (uint64_t i = 0; i < B * m; i++)
    if (alpha_out[i] < 1e-8) alpha_out[i] = 0.0;
  return SHN_OK;
}

// shn_abundance_em for B count vectors at once: DESIGN.md 3.14 rule 2
extern "C" int shn_abundance_em_batch(shn_ctx* ctx, const uint64_t* class_off, const uint32_t* members, const uint64_t* n_c, uint64_t n_classes,
                                      const double* eff, uint64_t m, uint64_t B, uint64_t max_live, double* alpha_out, uint32_t* rounds_out) {
  const std::string fn("shn_abundance_em_batch");
  if (int rc = abd_em_check(fn, class_off, members, n_classes, eff, m)) return rc;
  if (!ctx || !alpha_out || !rounds_out || (n_classes && !n_c)) return shn_fail(SHN_ERR_ARG, fn + ": NULL argument");
  if (B == 0) return shn_fail(SHN_ERR_ARG, fn + ": no replicates (B is 0)");
  if (B >= (1ULL << 32)) return shn_fail(SHN_ERR_OVERFLOW, fn + ": 2^32 or more replicates");
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  AbdEmDev E;
  if (int rc = abd_em_setup(ctx, bufs, T_ABD_EM_BATCH, class_off, members, n_classes, eff, m, &E, [](TimerRegion&) {})) return rc;
  unsigned long long* d_counts = nullptr;
  HIP_TRY(bufs.get(&d_counts, (B * n_classes + 1) * 8));
  if (n_classes) HIP_TRY(hipMemcpyAsync(d_counts, n_c, B * n_classes * 8, hipMemcpyHostToDevice, s));
  return abd_em_batch_run(ctx, bufs, E, d_counts, B, max_live, alpha_out, rounds_out);
}

// resample, then the batched EM, the counts staying on the device: DESIGN.md 3.14
extern "C" int shn_abundance_bootstrap(shn_ctx* ctx, const uint64_t* class_off, const uint32_t* members, const uint64_t* n_c, uint64_t n_classes,
                                       const double* eff, uint64_t m, uint64_t B, uint64_t seed, uint64_t max_live, double* alpha_out,
                                       uint32_t* rounds_out, uint64_t* counts_out) {
  const std::string fn("shn_abundance_bootstrap");
  if (int rc = abd_em_check(fn, class_off, members, n_classes, eff, m)) return rc;
  if (!ctx || !alpha_out || !rounds_out || (n_classes && !n_c)) return shn_fail(SHN_ERR_ARG, fn + ": NULL argument");
  uint64_t N = 0;
  if (int rc = abd_resample_check(fn, n_c, n_classes, B, &N)) return rc;
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  AbdEmDev E;
  if (int rc = abd_em_setup(ctx, bufs, T_ABD_EM_BATCH, class_off, members, n_classes, eff, m, &E, [](TimerRegion&) {})) return rc;
  unsigned long long* d_counts = nullptr;
  HIP_TRY(bufs.get(&d_counts, (B * n_classes + 1) * 8));
  if (int rc = abd_resample_run(ctx, bufs, n_c, n_classes, N, B, seed, d_counts)) return rc;
  if (counts_out && n_classes) HIP_TRY(hipMemcpyAsync(counts_out, d_counts, B * n_classes * 8, hipMemcpyDeviceToHost, s));
  return abd_em_batch_run(ctx, bufs, E, d_counts, B, max_live, alpha_out, rounds_out);
}
