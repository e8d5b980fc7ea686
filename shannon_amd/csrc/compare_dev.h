// The part of the comparison against a reference transcriptome (compare.hip) that is arithmetic alone: the
// maximum-segment summary of a stretch of a diagonal, how 32 bases fold into one and how two neighbours combine; and, for the
// chained form, the trim count, the join of two blocks and the links a chain is made of.  Host and device compile it alike, so a
// stand-alone host program can run it under a sanitizer.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CMP_HD __host__ __device__ __forceinline__
#else
#define CMP_HD inline
#endif

#define CMP_MATCH 1                 // score of a matching base
#define CMP_MISMATCH (-2)           // of any other pair of bases (a base outside ACGT matches nothing)

// A stretch of `len` positions of one diagonal.  Scores are sums of CMP_MATCH / CMP_MISMATCH.
//   tot        the whole stretch
//   ps, pl     the best prefix (the empty one counts): greatest score, then the longest
//   ss, sl     the best suffix, likewise
//   bs, bl, b0 the best segment: greatest score, then the longest, then the smallest start b0 (relative to the stretch);
//              bl == 0: the empty segment, score 0 (a named diagonal never ends with it: it holds 16 matches in a row)
struct CmpSum {
  int32_t tot; uint32_t len;
  int32_t ps; uint32_t pl;
  int32_t ss; uint32_t sl;
  int32_t bs; uint32_t bl, b0;
};

CMP_HD CmpSum cmp_empty() { return CmpSum{0, 0, 0, 0, 0, 0, 0, 0, 0}; }

// is segment (s, l, at) better than (bs, bl, b0)?  Equal keys: no -- the left operand of a combine stays.
CMP_HD bool cmp_better(int32_t s, uint32_t l, uint32_t at, int32_t bs, uint32_t bl, uint32_t b0) {
  return s > bs || (s == bs && (l > bl || (l == bl && at < b0)));
}

// A followed by B.  Associative; the tie rules survive: of two prefixes (suffixes) of equal score the one that reaches into the
// other operand is the longer one, and the segment across the seam is the longest best suffix of A and the longest best prefix of
// B, which of all segments across the seam of that score is the longest and, of those, starts first.
CMP_HD CmpSum cmp_combine(const CmpSum& A, const CmpSum& B) {
  CmpSum R;
  R.tot = A.tot + B.tot;
  R.len = A.len + B.len;
  if (A.tot + B.ps >= A.ps) { R.ps = A.tot + B.ps; R.pl = A.len + B.pl; } else { R.ps = A.ps; R.pl = A.pl; }
  if (A.ss + B.tot >= B.ss) { R.ss = A.ss + B.tot; R.sl = A.sl + B.len; } else { R.ss = B.ss; R.sl = B.sl; }
  R.bs = A.bs; R.bl = A.bl; R.b0 = A.b0;
  const int32_t xs = A.ss + B.ps;
  const uint32_t xl = A.sl + B.pl, x0 = A.len - A.sl;
  if (cmp_better(xs, xl, x0, R.bs, R.bl, R.b0)) { R.bs = xs; R.bl = xl; R.b0 = x0; }
  if (cmp_better(B.bs, B.bl, A.len + B.b0, R.bs, R.bl, R.b0)) { R.bs = B.bs; R.bl = B.bl; R.b0 = A.len + B.b0; }
  return R;
}

// `n` <= 32 positions: bit 62 - 2 j of `diff` is set where position j does not match (the low bit of base j's 2-bit field, first
// base in the top bits).  One position after the other: what cmp_combine gives with a one-position right operand.
CMP_HD CmpSum cmp_fold32(uint64_t diff, uint32_t n) {
  CmpSum R = cmp_empty();
  for (uint32_t j = 0; j < n; j++) {
    const int32_t v = ((diff >> (62 - 2 * j)) & 1) ? CMP_MISMATCH : CMP_MATCH;
    R.tot += v;
    R.len++;
    if (R.tot >= R.ps) { R.ps = R.tot; R.pl = R.len; }
    if (R.ss + v >= 0) { R.ss += v; R.sl++; } else { R.ss = 0; R.sl = 0; }
    if (R.ss > R.bs || (R.ss == R.bs && R.sl > R.bl)) { R.bs = R.ss; R.bl = R.sl; R.b0 = R.len - R.sl; }
  }
  return R;
}

// matches and mismatches of a segment of `len` positions and score s = matches - 2 mismatches
CMP_HD uint32_t cmp_mismatches(int32_t s, uint32_t len) { return (uint32_t)((int32_t)len - s) / 3u; }

// ---- the chained form ("Chained rows"): a pair's diagonals joined into one multi-block row

// 64 bits of a packed text from base g on (first base in the top bits) and 32 mask bits (bit 31 = base g); both texts carry two
// zero words behind their ends, so the word behind the last one may be read.  (ffp_text32, cmp_mask32 and ffp_spread once more,
// for both compilers: those three are __device__ alone and the kernels that use them stay as they are.)
CMP_HD uint64_t cmp_words32(const uint64_t* w, uint64_t g) {
  const uint64_t wi = g >> 5;
  const uint32_t sh = (uint32_t)(g & 31) * 2;
  uint64_t v = w[wi] << sh;
  if (sh) v |= w[wi + 1] >> (64 - sh);
  return v;
}
CMP_HD uint32_t cmp_nmask32(const uint64_t* nm, uint64_t g) {
  const uint64_t wi = g >> 6;
  const uint32_t sh = (uint32_t)(g & 63);
  uint64_t v = nm[wi] << sh;
  if (sh) v |= nm[wi + 1] >> (64 - sh);
  return (uint32_t)(v >> 32);
}
// bit i of a 32-bit word -> bit 2 i
CMP_HD uint64_t cmp_spread32(uint32_t n) {
  uint64_t x = n;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFULL;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFULL;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0FULL;
  x = (x | (x << 2)) & 0x3333333333333333ULL;
  x = (x | (x << 1)) & 0x5555555555555555ULL;
  return x;
}

// Trim count: the matches (rule 3: both ACGT and equal) among the v positions of a diagonal that start at base gq of the packed
// queries and base gt of the packed oriented targets.  The score's XOR / pair-fold / mask-OR, 32 positions a step, a popcount of
// the mismatches; the last step keeps its first v - k positions only.
CMP_HD uint32_t cmp_trim_matches(const uint64_t* qw, const uint64_t* qnm, const uint64_t* tw, const uint64_t* tnm, uint64_t gq, uint64_t gt,
                                 uint32_t v) {
  uint32_t mis = 0;
  for (uint32_t k = 0; k < v; k += 32) {
    const uint32_t n = v - k < 32 ? v - k : 32;
    uint64_t diff = cmp_words32(qw, gq + k) ^ cmp_words32(tw, gt + k);
    diff = (diff | (diff >> 1)) & 0x5555555555555555ULL;
    diff |= cmp_spread32(cmp_nmask32(qnm, gq + k) | cmp_nmask32(tnm, gt + k));
    diff &= ~0ULL << (64 - 2 * n);
    mis += (uint32_t)__builtin_popcountll(diff);
  }
  return v - mis;
}

#define CMP_NONE 0xFFFFFFFFu

// a block: the best segment of one diagonal d -- query [q0, q0 + len), oriented target [q0 + d, q0 + d + len), score s
struct CmpBlock { int32_t d; uint32_t q0, len; int32_t s; };

// A chain that ends in some block: its value (S, M, R = sums of score and matches over its blocks, every block after the first
// trimmed against its predecessor; the number of blocks), the last block's predecessor (CMP_NONE: it is the first) and how the last
// block entered: without its first v positions, m matches in what is left.  S == INT32_MIN: no chain.
struct CmpLink { int32_t S; uint32_t M, R, pred, v, m; };

CMP_HD CmpLink cmp_link_none() { return CmpLink{INT32_MIN, 0, 0, CMP_NONE, 0, 0}; }
CMP_HD CmpLink cmp_link_alone(const CmpBlock& B) {
  const uint32_t m = B.len - cmp_mismatches(B.s, B.len);
  return CmpLink{B.s, m, 1, CMP_NONE, 0, m};
}
// the value of x greater than that of y: S, then M, then the fewer blocks
CMP_HD bool cmp_value_greater(const CmpLink& x, const CmpLink& y) {
  return x.S > y.S || (x.S == y.S && (x.M > y.M || (x.M == y.M && x.R < y.R)));
}
// x before y: the greater value, then the smaller predecessor -- a total order on the links into one block, so a reduction gives
// the same link whatever its shape
CMP_HD bool cmp_link_before(const CmpLink& x, const CmpLink& y) {
  return cmp_value_greater(x, y) || (x.S == y.S && x.M == y.M && x.R == y.R && x.pred < y.pred);
}
// may B follow A?  *v: the positions B loses at its start
CMP_HD bool cmp_joins(const CmpBlock& A, const CmpBlock& B, uint32_t* v) {
  const int64_t qe = (int64_t)A.q0 + A.len, dq = qe - (int64_t)B.q0, dt = qe + A.d - ((int64_t)B.q0 + B.d);
  const int64_t o = dq > dt ? dq : dt, w = o > 0 ? o : 0;
  *v = (uint32_t)w;
  return A.d != B.d && w < (int64_t)B.len;
}
// the best chain into A (at index a), then B without its first v positions, of which mt match
CMP_HD CmpLink cmp_link_after(const CmpLink& into_a, uint32_t a, const CmpBlock& B, uint32_t v, uint32_t mt) {
  const uint32_t mm_b = cmp_mismatches(B.s, B.len), m = B.len - mm_b - mt, mm = mm_b - (v - mt);
  return CmpLink{into_a.S + (int32_t)m - 2 * (int32_t)mm, into_a.M + m, into_a.R + 1, a, v, m};
}
