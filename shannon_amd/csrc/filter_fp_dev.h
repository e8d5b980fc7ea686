// What the mapping of read pairs onto transcripts shares between --filter_FP (filter_fp.hip) and --kallisto_cutoff (abundance.hip):
// the views of a read set and of the transcripts' index, the placement of a mate (seeds, verification) and the enumeration of
// every concordant placement of an oriented pair (DESIGN.md "filter_FP", rules 2-5).  What a caller does with a placement is its own.
#pragma once
#include "common.h"
#include "runs.h"

#define FFP_SEED SHN_FILTER_FP_SEED
#define FFP_NONE 0xFFFFFFFFu
#define FFP_BLOCK 256
#define FFP_YSEEDS 9

struct shn_routes;
int shn_routes_device_arrays(const shn_routes* r, const uint32_t** pid, const uint32_t** ridx, uint64_t* n);   // route.hip

// a read set as the mapping sees it: the set as packed by shn_reads_create / shn_reads_ingest and its reverse complement in the
// same geometry (every read in its own words, so RC(read i) lies where read i lies)
struct FfpSet {
  const uint64_t *words, *mask, *words_rc, *mask_rc, *woff;
  const uint32_t* len;
  const uint8_t* bad;          // NULL: no read of the set holds a non-ACGT base
  uint32_t fixed_len, wpr;
};
struct FfpRead { const uint64_t* w; const uint64_t* m; uint32_t L; bool bad; };

struct FfpIndex {
  const uint64_t* keys; const uint32_t* vals; uint64_t n_rec;
  const uint64_t* tw;          // the text, 32 bases a word, first base in the top bits; two zero words behind the end
  const uint64_t* t_off; uint64_t n_tr;
};

__device__ __forceinline__ FfpRead ffp_read(const FfpSet& S, uint64_t i, bool rc) {
  FfpRead r;
  const uint64_t wb = S.woff ? S.woff[i] : i * (uint64_t)S.wpr;
  r.L = S.len ? S.len[i] : S.fixed_len;
  r.w = (rc ? S.words_rc : S.words) + wb;
  r.bad = S.bad != nullptr && S.bad[i] != 0;
  r.m = r.bad ? (rc ? S.mask_rc : S.mask) + wb / 2 : nullptr;
  return r;
}

// 32 bases of the text from base g on (the words behind the text's end are zero)
__device__ __forceinline__ uint64_t ffp_text32(const uint64_t* __restrict__ tw, uint64_t g) {
  const uint64_t wi = g >> 5;
  const uint32_t sh = (uint32_t)(g & 31) * 2;
  uint64_t v = tw[wi] << sh;
  if (sh) v |= tw[wi + 1] >> (64 - sh);
  return v;
}
__device__ __forceinline__ uint64_t ffp_text_seed(const uint64_t* __restrict__ tw, uint64_t g) {
  return ffp_text32(tw, g) >> (64 - 2 * FFP_SEED);
}

// bit i of a 32-bit word -> bit 2 i (the N mask of 32 bases onto the low bits of their 2-bit fields)
__device__ __forceinline__ uint64_t ffp_spread(uint32_t n) {
  uint64_t x = n;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFULL;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFULL;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0FULL;
  x = (x | (x << 2)) & 0x3333333333333333ULL;
  x = (x | (x << 1)) & 0x5555555555555555ULL;
  return x;
}

// Hamming distance between the read and the text at u (a non-ACGT base of the read is a mismatch); gives up above thr
__device__ __forceinline__ uint32_t ffp_hamming(const FfpRead& x, const uint64_t* __restrict__ tw, uint64_t u, uint32_t thr) {
  uint32_t mm = 0;
  const uint32_t nw = (x.L + 31) >> 5;
  for (uint32_t k = 0; k < nw; k++) {
    uint64_t d = x.w[k] ^ ffp_text32(tw, u + 32ull * k);
    d = (d | (d >> 1)) & 0x5555555555555555ULL;
    if (x.bad) {
      const uint64_t m = x.m[k >> 1];
      d |= ffp_spread((k & 1) ? (uint32_t)m : (uint32_t)(m >> 32));
    }
    const uint32_t rem = x.L - 32 * k;
    if (rem < 32) d &= ~0ULL << (64 - 2 * rem);
    mm += (uint32_t)__popcll(d);
    if (mm > thr) return mm;
  }
  return mm;
}

__device__ __forceinline__ bool ffp_seed_of(const FfpRead& x, uint32_t s, uint64_t* seed) {
  if (x.bad && shn_extract_mask(x.m, s * FFP_SEED, FFP_SEED)) return false;
  *seed = shn_extract(x.w, s * FFP_SEED, FFP_SEED);
  return true;
}

// does a seed before s match the text exactly when the read starts at u?  (then that seed has named this start already)
__device__ __forceinline__ bool ffp_named_before(const FfpRead& x, const uint64_t* __restrict__ tw, uint64_t u, uint32_t s) {
  for (uint32_t e = 0; e < s; e++) {
    uint64_t seed;
    if (ffp_seed_of(x, e, &seed) && ffp_text_seed(tw, u + (uint64_t)e * FFP_SEED) == seed) return true;
  }
  return false;
}

// Every concordant placement of the oriented pair (x, y) in the partition whose key prefix is pkey: x at u, y at v on the same
// transcript j, u <= v, u + |x| <= v + |y|, v + |y| - u <= max_span, each mate within its mismatch bound; f(cost, j, u, v) is
// called for each of them whose first mate alone does not already cost more than *best (EXACT == false: not already as much --
// the pass that looks for the minimum, f may lower *best as it goes).
template <bool EXACT, class F>
__device__ __forceinline__ void ffp_each_placement(const FfpIndex& I, uint64_t pkey, const FfpRead& x, const FfpRead& y, uint32_t max_span,
                                                   const uint32_t* best, F&& f) {
  if (x.L < FFP_SEED || y.L < FFP_SEED) return;
  const uint32_t thrx = x.L / 30, thry = y.L / 30;
  uint32_t ylo[FFP_YSEEDS];                              // first index record of the second mate's seeds (reads up to 269 bases: all of them)
  bool have_y = false;
  for (uint32_t s = 0; s <= thrx; s++) {
    uint64_t seed;
    if (!ffp_seed_of(x, s, &seed)) continue;
    const uint64_t key = pkey | seed;
    for (uint64_t r = shn_lower_bound(I.keys, I.n_rec, key); r < I.n_rec && I.keys[r] == key; r++) {
      const uint64_t g = I.vals[r];
      const uint64_t j = shn_segment_of(I.t_off, I.n_tr, g);               // (an empty transcript holds no base)
      const uint64_t a = I.t_off[j], b = I.t_off[j + 1];
      if (g < a + (uint64_t)s * FFP_SEED) continue;
      const uint64_t u = g - (uint64_t)s * FFP_SEED;
      if (u + x.L > b || ffp_named_before(x, I.tw, u, s)) continue;
      const uint32_t cx = ffp_hamming(x, I.tw, u, thrx);
      if (cx > thrx || (EXACT ? cx > *best : cx >= *best)) continue;
      if (!have_y) {                                     // (the first verified first mate: where the second mate's seeds start in the index)
        for (uint32_t t = 0; t <= thry && t < FFP_YSEEDS; t++) {
          uint64_t seed_y;
          ylo[t] = ffp_seed_of(y, t, &seed_y) ? (uint32_t)shn_lower_bound(I.keys, I.n_rec, pkey | seed_y) : FFP_NONE;
        }
        have_y = true;
      }
      for (uint32_t t = 0; t <= thry; t++) {
        uint64_t seed_y;
        if (!ffp_seed_of(y, t, &seed_y)) continue;
        const uint64_t key_y = pkey | seed_y;
        for (uint64_t q = t < FFP_YSEEDS ? ylo[t] : shn_lower_bound(I.keys, I.n_rec, key_y); q < I.n_rec && I.keys[q] == key_y; q++) {
          const uint64_t gy = I.vals[q];
          if (gy < a + (uint64_t)t * FFP_SEED || gy >= b) continue;                 // (another transcript, or y would start before this one)
          const uint64_t v = gy - (uint64_t)t * FFP_SEED;
          if (v + y.L > b || v < u || u + x.L > v + y.L || v + y.L - u > max_span) continue;
          if (ffp_named_before(y, I.tw, v, t)) continue;
          const uint32_t cy = ffp_hamming(y, I.tw, v, thry);
          if (cy > thry) continue;
          f(cx + cy, j, u, v);
        }
      }
    }
  }
}

// the fragment's minimum cost over one oriented pair (FFP_NONE stays when nothing is concordant)
__device__ __forceinline__ void ffp_min_cost(const FfpIndex& I, uint64_t pkey, const FfpRead& x, const FfpRead& y, uint32_t max_span, uint32_t* best) {
  ffp_each_placement<false>(I, pkey, x, y, max_span, best, [&](uint32_t c, uint64_t, uint64_t, uint64_t) { if (c < *best) *best = c; });
}

// Every placement of the single read x in the partition whose key prefix is pkey (DESIGN.md 3.13 rule 1): x at u on transcript j,
// u + |x| <= len_j, at most |x| / 30 mismatches.  The first |x| / 30 + 1 seeds find every one of them (they do not overlap and lie
// inside the read: one of them is free of mismatches); a start is named by the first seed that matches there.  f(cost, j, u) is
// called for each placement that does not cost more than *best (EXACT == false: not as much -- the pass that looks for the
// minimum, f may lower *best as it goes).
template <bool EXACT, class F>
__device__ __forceinline__ void ffp_each_single(const FfpIndex& I, uint64_t pkey, const FfpRead& x, const uint32_t* best, F&& f) {
  if (x.L < FFP_SEED) return;
  const uint32_t thr = x.L / 30;
  for (uint32_t s = 0; s <= thr; s++) {
    uint64_t seed;
    if (!ffp_seed_of(x, s, &seed)) continue;
    const uint64_t key = pkey | seed;
    for (uint64_t r = shn_lower_bound(I.keys, I.n_rec, key); r < I.n_rec && I.keys[r] == key; r++) {
      const uint64_t g = I.vals[r];
      const uint64_t j = shn_segment_of(I.t_off, I.n_tr, g);               // (an empty transcript holds no base)
      const uint64_t a = I.t_off[j], b = I.t_off[j + 1];
      if (g < a + (uint64_t)s * FFP_SEED) continue;
      const uint64_t u = g - (uint64_t)s * FFP_SEED;
      if (u + x.L > b || ffp_named_before(x, I.tw, u, s)) continue;
      const uint32_t lim = *best < thr ? *best : thr;                       // (the count gives up above both bounds)
      const uint32_t c = ffp_hamming(x, I.tw, u, lim);
      if (c > lim || (!EXACT && c >= *best)) continue;
      f(c, j, u - a);
    }
  }
}

// ---- host side (filter_fp.hip): what both callers prepare the same way
// the device view of a resident read set; want_rc: its reverse complement written beside it (rc_bytes += what that read and wrote)
int ffp_set(shn_ctx* ctx, ShnDevBufs& bufs, const shn_reads* r, bool want_rc, FfpSet* out, uint64_t* rc_bytes);
// t_off (host, n_tr + 1) checked -- [0] == 0, monotone: SHN_ERR_ARG in fn's name -- and rec_off[j] = 15-mer records of the
// transcripts before j (n_tr + 1).  Host work alone: both callers run it with their other argument checks, before the device is touched.
int ffp_record_offsets(const std::string& fn, const uint64_t* t_off, uint64_t n_tr, std::vector<uint64_t>* rec_off);
// the transcripts' text packed 2 bits a base and the sorted index of its 15-mers, timed under `slot`; rec_off: ffp_record_offsets'.
// Synchronises; a base outside ACGT fails the call.  *n_tw = words of the packed text.
int ffp_index_build(const std::string& fn, shn_ctx* ctx, ShnDevBufs& bufs, int slot, const uint8_t* text, const uint64_t* t_off, const uint32_t* t_part,
                    uint64_t n_tr, uint32_t n_parts, const std::vector<uint64_t>& rec_off, FfpIndex* out, uint64_t* n_tw);
