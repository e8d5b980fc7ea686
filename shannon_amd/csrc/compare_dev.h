// The part of the comparison against a reference transcriptome (compare.hip) that is arithmetic alone: the
// maximum-segment summary of a stretch of a diagonal, how 32 bases fold into one and how two neighbours combine.  Host and
// device compile it alike, so a stand-alone host program can run it under a sanitizer.
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
