// --compare on the device: every reference transcript against every reconstructed transcript (shannon.py:620-622 starts
// run_MB_SF_fn.py --compare, whose parallel_blat_python.py run -- run_MB_SF_fn.py:299 -- writes reconstr_per.txt).  BLAT is replaced
// by the rule of DESIGN.md 3.12; this file makes its rows, shannon_amd/compare.py the reference's analysis of them.
//
//   index   queries and targets packed 2 bits a base beside a mask of the bases outside ACGT; the reverse complement of every
//           target packed once behind the targets (the oriented targets: m of them, 2 m unless strand-specific).  One record per
//           16-mer position inside an oriented target, key = the 16-mer (bit 32 set where it holds a base outside ACGT: no query
//           looks there), value = position in the oriented text, sorted by key (shn_sort_pairs; stable, so by position in a run).
//   seeds   a thread per query position: binary search of its 16-mer, a candidate for every hit whose neighbour one base earlier
//           on the same diagonal does not match (the start of a run of 16-mer hits -- ffp_named_before's idea); count, scan, fill, so
//           nothing is capped.  Candidate = query << .. | (target * 2 + orientation) << 21 | diagonal + 2^20, sorted by the whole
//           key (shn_sort_keys) and made unique: (query, target) pairs in row order, inside a pair + before -, then by diagonal.
//   score   a wave per candidate diagonal, a lane per 32 bases (XOR of the words, OR of the masks), the lanes' summaries combined
//           in order through shuffles, a carry across passes of 2,048 bases (compare_dev.h holds the summary).
//   rows    the first candidate of a pair walks the pair's candidates for the best; pairs of 30 matches or more are counted,
//           scanned and filled into the row arrays.
//   chain   (shn_compare_chains, in place of rows) every scored diagonal of a (query, target, orientation) is a block; one stable
//           sort puts a group's blocks in the order (qEnd, diagonal); a wave per group chains them -- per block the lanes stride over
//           its possible predecessors, trim it against each (compare_dev.h: the join and the trim count) and reduce to the best
//           link through shuffles; the pair's better orientation is picked, rows and blocks are counted, scanned and a thread per
//           row walks its chain back and writes the row and its blocks.
#include "common.h"
#include "filter_fp_dev.h"
#include "compare_dev.h"
#include "runs.h"
#include <algorithm>

namespace {

constexpr int CMP_BLK = 256;
constexpr int CMP_SEED = SHN_COMPARE_SEED;
constexpr int CMP_DBITS = 21;                       // a diagonal + 2^20 (sequences are shorter than 2^20 bases)
constexpr uint64_t CMP_DBIAS = 1ULL << 20;
constexpr uint64_t CMP_BAD_KEY = 1ULL << 32;

// sequences one after the other: w 32 bases a word (first base in the top bits), nm 64 mask bits a word (1 = outside ACGT, the
// base itself packed as A), both with two zero words behind the end; off[n_seq + 1] on the device
struct CmpText { const uint64_t* w; const uint64_t* nm; const uint64_t* off; uint64_t n_seq, total; };

// 32 mask bits from base g on (bit 31 = base g)
__device__ __forceinline__ uint32_t cmp_mask32(const uint64_t* __restrict__ nm, uint64_t g) {
  const uint64_t wi = g >> 6;
  const uint32_t sh = (uint32_t)(g & 63);
  uint64_t v = nm[wi] << sh;
  if (sh) v |= nm[wi + 1] >> (64 - sh);
  return (uint32_t)(v >> 32);
}
// base g as a code 0..3, 4 outside ACGT
__device__ __forceinline__ uint32_t cmp_base(const CmpText& X, uint64_t g) {
  if ((X.nm[g >> 6] >> (63 - (g & 63))) & 1) return 4;
  return (uint32_t)(X.w[g >> 5] >> (62 - 2 * (g & 31))) & 3;
}

// ASCII -> packed, a thread per 64 bases (two words, one mask word).  Bases [0, total) are the text as it is; [total, n_out) --
// n_out is total or 2 total -- the reverse complement of every sequence, RC(sequence j) lying where j lies, `total` further on.
__global__ __launch_bounds__(CMP_BLK) void cmp_pack_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ off, uint64_t n_seq,
                                                           uint64_t total, uint64_t n_out, uint64_t* __restrict__ w, uint64_t* __restrict__ nm) {
  SHN_GRID_FOR(grp, (n_out + 63) / 64) {
    uint64_t w0 = 0, w1 = 0, m = 0, j = 0;
    bool have = false;
    for (uint32_t e = 0; e < 64; e++) {
      const uint64_t g = grp * 64 + e;
      if (g >= n_out) break;
      uint8_t ch;
      if (g < total) ch = text[g];
      else {
        const uint64_t h = g - total;
        if (!have || h >= off[j + 1]) { j = shn_segment_of(off, n_seq, h); have = true; }
        ch = text[off[j + 1] - 1 - (h - off[j])];
      }
      uint64_t c = 0;
      bool bad = false;
      switch (ch) {
        case 'A': case 'a': c = 0; break;
        case 'C': case 'c': c = 1; break;
        case 'G': case 'g': c = 2; break;
        case 'T': case 't': c = 3; break;
        default: bad = true;
      }
      if (bad) m |= 1ULL << (63 - e);
      else {
        if (g >= total) c = 3 - c;
        if (e < 32) w0 |= c << (62 - 2 * e); else w1 |= c << (62 - 2 * (e - 32));
      }
    }
    w[2 * grp] = w0;
    w[2 * grp + 1] = w1;
    nm[grp] = m;
  }
}

// record r = the r-th 16-mer position inside an oriented target (rec_off[t] = records of the oriented targets before t)
__global__ __launch_bounds__(CMP_BLK) void cmp_records_kernel(CmpText T, const uint64_t* __restrict__ rec_off, uint64_t n_rec, uint64_t* __restrict__ keys,
                                                              uint32_t* __restrict__ vals) {
  SHN_GRID_FOR(r, n_rec) {
    const uint64_t t = shn_segment_of(rec_off, T.n_seq, r);
    const uint64_t g = T.off[t] + (r - rec_off[t]);
    keys[r] = (cmp_mask32(T.nm, g) >> (32 - CMP_SEED)) ? CMP_BAD_KEY : ffp_text32(T.w, g) >> (64 - 2 * CMP_SEED);
    vals[r] = (uint32_t)g;
  }
}

// A thread per query base g.  FILL == false: cnt[g] = its candidates; FILL == true: they are written from pos[g] on.
// m: targets (oriented target t is target t, forward, below m and target t - m, reverse complement, from m on).
template <bool FILL>
__global__ __launch_bounds__(CMP_BLK) void cmp_seed_kernel(CmpText Q, CmpText T, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                           uint64_t n_rec, uint64_t m, int i_shift, uint32_t* __restrict__ cnt,
                                                           const uint64_t* __restrict__ pos, uint64_t* __restrict__ out) {
  SHN_GRID_FOR(g, Q.total) {
    uint32_t c = 0;
    const uint64_t i = shn_segment_of(Q.off, Q.n_seq, g);
    const uint64_t a = g - Q.off[i];
    if (g + CMP_SEED <= Q.off[i + 1] && (cmp_mask32(Q.nm, g) >> (32 - CMP_SEED)) == 0) {
      const uint64_t seed = ffp_text32(Q.w, g) >> (64 - 2 * CMP_SEED);
      const uint32_t before = a ? cmp_base(Q, g - 1) : 4u;
      for (uint64_t r = shn_lower_bound(keys, n_rec, seed); r < n_rec && keys[r] == seed; r++) {
        const uint64_t h = vals[r];
        const uint64_t t = shn_segment_of(T.off, T.n_seq, h);
        const uint64_t b = h - T.off[t];
        if (before < 4 && b && cmp_base(T, h - 1) == before) continue;      // (the hit one base earlier names this diagonal)
        if (FILL) {
          const uint64_t o = t >= m ? 1 : 0, j = o ? t - m : t;
          out[pos[g] + c] = (i << i_shift) | ((j * 2 + o) << CMP_DBITS) | (b + CMP_DBIAS - a);
        }
        c++;
      }
    }
    if (!FILL) cnt[g] = c;
  }
}

struct CmpCand { uint64_t i, j, t; uint32_t o; int64_t d; };
__device__ __forceinline__ CmpCand cmp_decode(uint64_t key, int i_shift, uint64_t m) {
  CmpCand c;
  c.i = key >> i_shift;
  const uint64_t jo = (key >> CMP_DBITS) & ((1ULL << (i_shift - CMP_DBITS)) - 1);
  c.j = jo >> 1; c.o = (uint32_t)(jo & 1);
  c.t = c.o ? m + c.j : c.j;
  c.d = (int64_t)(key & ((1ULL << CMP_DBITS) - 1)) - (int64_t)CMP_DBIAS;
  return c;
}

__device__ __forceinline__ CmpSum cmp_shfl_down(const CmpSum& x, int off) {
  CmpSum y;
  y.tot = __shfl_down(x.tot, off, 64); y.len = __shfl_down(x.len, off, 64);
  y.ps = __shfl_down(x.ps, off, 64); y.pl = __shfl_down(x.pl, off, 64);
  y.ss = __shfl_down(x.ss, off, 64); y.sl = __shfl_down(x.sl, off, 64);
  y.bs = __shfl_down(x.bs, off, 64); y.bl = __shfl_down(x.bl, off, 64); y.b0 = __shfl_down(x.b0, off, 64);
  return y;
}

// One wave a candidate: the positions where both sequences exist are a0 .. a1 of the query; lane l of pass p takes the 32 of them
// from a0 + 32 (64 p + l) on.  After the strides 1, 2, .. 32 lane 0 holds the 64 summaries combined in order (lane l combines
// itself, on the left, with lane l + stride: what it then holds covers l .. l + 2 stride - 1; lanes near the end pick up
// their own value instead, which lane 0 never sees).
__global__ __launch_bounds__(CMP_BLK) void cmp_score_kernel(CmpText Q, CmpText T, const uint64_t* __restrict__ cand, uint64_t n_cand, uint64_t m, int i_shift,
                                                            int32_t* __restrict__ out_s, uint32_t* __restrict__ out_len, uint32_t* __restrict__ out_q0) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t n_waves = (uint64_t)gridDim.x * (CMP_BLK / 64);
  for (uint64_t c = (uint64_t)blockIdx.x * (CMP_BLK / 64) + (threadIdx.x >> 6); c < n_cand; c += n_waves) {
    const CmpCand k = cmp_decode(cand[c], i_shift, m);
    const uint64_t qo = Q.off[k.i], to = T.off[k.t];
    const int64_t Lq = (int64_t)(Q.off[k.i + 1] - qo), Lt = (int64_t)(T.off[k.t + 1] - to);
    const int64_t a0 = k.d < 0 ? -k.d : 0, a1 = Lq < Lt - k.d ? Lq : Lt - k.d;
    const uint64_t n = a1 > a0 ? (uint64_t)(a1 - a0) : 0;
    CmpSum carry = cmp_empty();
    for (uint64_t base = 0; base < n; base += 2048) {
      const uint64_t s = base + 32ull * lane;
      CmpSum x = cmp_empty();
      if (s < n) {
        const uint32_t len = (uint32_t)(n - s < 32 ? n - s : 32);
        const uint64_t gq = qo + (uint64_t)a0 + s, gt = to + (uint64_t)(a0 + k.d) + s;
        uint64_t diff = ffp_text32(Q.w, gq) ^ ffp_text32(T.w, gt);
        diff = (diff | (diff >> 1)) & 0x5555555555555555ULL;
        diff |= ffp_spread(cmp_mask32(Q.nm, gq) | cmp_mask32(T.nm, gt));
        x = cmp_fold32(diff, len);
      }
      for (int off = 1; off < 64; off <<= 1) x = cmp_combine(x, cmp_shfl_down(x, off));
      carry = cmp_combine(carry, x);                        // (lane 0's is the diagonal's)
    }
    if (lane == 0) { out_s[c] = carry.bs; out_len[c] = carry.bl; out_q0[c] = (uint32_t)a0 + carry.b0; }
  }
}

// The first candidate of a (query, target) pair walks the pair's candidates -- they are in the order + before -, then by diagonal
// -- for the greatest score, then the most matches (of equal scores the longer segment holds more); the first of equals stays.
__global__ void cmp_pairs_kernel(const uint64_t* __restrict__ cand, uint64_t n_cand, const int32_t* __restrict__ s, const uint32_t* __restrict__ len,
                                 uint32_t min_matches, uint32_t* __restrict__ keep, uint32_t* __restrict__ best) {
  SHN_GRID_FOR(c, n_cand) {
    const uint64_t pair = cand[c] >> (CMP_DBITS + 1);
    uint32_t k = 0;
    if (c == 0 || (cand[c - 1] >> (CMP_DBITS + 1)) != pair) {
      uint64_t at = c;
      for (uint64_t e = c + 1; e < n_cand && (cand[e] >> (CMP_DBITS + 1)) == pair; e++)
        if (s[e] > s[at] || (s[e] == s[at] && len[e] > len[at])) at = e;
      best[c] = (uint32_t)at;
      k = len[at] - cmp_mismatches(s[at], len[at]) >= min_matches ? 1u : 0u;
    }
    keep[c] = k;
  }
}

// rows[f * n_rows + r], f = i, j, strand (0 +, 1 -), matches, mismatches, qStart, qEnd, tStart (on the target's forward strand)
__global__ void cmp_rows_kernel(CmpText T, const uint64_t* __restrict__ cand, uint64_t n_cand, uint64_t m, int i_shift, const int32_t* __restrict__ s,
                                const uint32_t* __restrict__ len, const uint32_t* __restrict__ q0, const uint32_t* __restrict__ keep,
                                const uint32_t* __restrict__ best, const uint64_t* __restrict__ pos, uint64_t n_rows, uint32_t* __restrict__ rows) {
  SHN_GRID_FOR(c, n_cand) {
    if (!keep[c]) continue;
    const uint32_t e = best[c];
    const CmpCand k = cmp_decode(cand[e], i_shift, m);
    const uint32_t mm = cmp_mismatches(s[e], len[e]);
    const int64_t Lt = (int64_t)(T.off[k.t + 1] - T.off[k.t]);
    const int64_t b0 = (int64_t)q0[e] + k.d;
    const uint64_t r = pos[c];
    rows[r] = (uint32_t)k.i;
    rows[n_rows + r] = (uint32_t)k.j;
    rows[2 * n_rows + r] = k.o;
    rows[3 * n_rows + r] = len[e] - mm;
    rows[4 * n_rows + r] = mm;
    rows[5 * n_rows + r] = q0[e];
    rows[6 * n_rows + r] = q0[e] + len[e];
    rows[7 * n_rows + r] = (uint32_t)(k.o ? Lt - (b0 + (int64_t)len[e]) : b0);
  }
}

// ---- the chained form: a pair's diagonals joined into one multi-block row ("Chained rows")
constexpr int CMP_QBITS = 20;                       // a qEnd (sequences are shorter than 2^20 bases)

// block order: key = (query, 2 target + orientation, qEnd), value = the candidate; the candidates come sorted by diagonal inside
// an oriented pair, which a stable sort by this key keeps as the tie
__global__ void cmp_chain_keys_kernel(const uint64_t* __restrict__ cand, const uint32_t* __restrict__ len, const uint32_t* __restrict__ q0, uint64_t n_cand,
                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  SHN_GRID_FOR(c, n_cand) {
    keys[c] = ((cand[c] >> CMP_DBITS) << CMP_QBITS) | (uint64_t)(q0[c] + len[c]);
    vals[c] = (uint32_t)c;
  }
}
// block p of the order = candidate perm[p]; head[p]: the first block of its (query, target, orientation)
__global__ void cmp_blocks_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ perm, uint64_t n_cand, const uint64_t* __restrict__ cand,
                                  const int32_t* __restrict__ s, const uint32_t* __restrict__ len, const uint32_t* __restrict__ q0, CmpBlock* __restrict__ blk,
                                  uint32_t* __restrict__ head) {
  SHN_GRID_FOR(p, n_cand) {
    const uint32_t c = perm[p];
    CmpBlock b;
    b.d = (int32_t)((int64_t)(cand[c] & ((1ULL << CMP_DBITS) - 1)) - (int64_t)CMP_DBIAS);
    b.q0 = q0[c]; b.len = len[c]; b.s = s[c];
    blk[p] = b;
    head[p] = (p == 0 || (keys[p] >> CMP_QBITS) != (keys[p - 1] >> CMP_QBITS)) ? 1u : 0u;
  }
}
struct CmpGroup { uint64_t i, j, t; uint32_t o; };
__device__ __forceinline__ CmpGroup cmp_group_of(uint64_t key, int jo_bits, uint64_t m) {
  CmpGroup g;
  const uint64_t k = key >> CMP_QBITS, jo = k & ((1ULL << jo_bits) - 1);
  g.i = k >> jo_bits; g.j = jo >> 1; g.o = (uint32_t)(jo & 1);
  g.t = g.o ? m + g.j : g.j;
  return g;
}
__device__ __forceinline__ CmpLink cmp_shfl_down(const CmpLink& x, int off) {
  CmpLink y;
  y.S = __shfl_down(x.S, off, 64); y.M = __shfl_down(x.M, off, 64); y.R = __shfl_down(x.R, off, 64);
  y.pred = __shfl_down(x.pred, off, 64); y.v = __shfl_down(x.v, off, 64); y.m = __shfl_down(x.m, off, 64);
  return y;
}

// One wave a (query, target, orientation) group: its blocks b0 .. b1 - 1 one after the other; for block b the lanes stride over
// the blocks in front of it (lane l takes b0 + l, b0 + l + 64, ..), each forms the overlap v, the trimmed block and the value of
// the best chain into a followed by it (cmp_link_after), keeps its best, and the wave reduces through __shfl_down at strides
// 1, 2, .. 32 under cmp_link_before -- a total order, so lane 0 ends with the greatest value and of equals the smallest
// predecessor.  Lane 0 writes st[b]; the lanes read it in later rounds, so a fence stands between the rounds (st is neither
// const nor restrict).  A group of one block is a copy.  top[g]: the best chain of the group, its pred field naming its LAST
// block (the first of equals: the smallest index).  A group of r blocks takes about r^2 / 64 steps of its wave.
__global__ __launch_bounds__(CMP_BLK) void cmp_chain_kernel(CmpText Q, CmpText T, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ gstart,
                                                            uint64_t n_groups, uint64_t m, int jo_bits, const CmpBlock* __restrict__ blk, CmpLink* st,
                                                            CmpLink* __restrict__ top) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t n_waves = (uint64_t)gridDim.x * (CMP_BLK / 64);
  for (uint64_t g = (uint64_t)blockIdx.x * (CMP_BLK / 64) + (threadIdx.x >> 6); g < n_groups; g += n_waves) {
    const uint32_t b0 = gstart[g], b1 = gstart[g + 1];
    const CmpGroup G = cmp_group_of(keys[b0], jo_bits, m);
    const uint64_t qo = Q.off[G.i], to = T.off[G.t];
    CmpLink best = cmp_link_none();
    for (uint32_t b = b0; b < b1; b++) {
      const CmpBlock B = blk[b];
      CmpLink x = cmp_link_none();
      if (b > b0) {
        for (uint32_t a = b0 + lane; a < b; a += 64) {
          uint32_t v;
          if (!cmp_joins(blk[a], B, &v)) continue;
          const uint32_t mt = v ? cmp_trim_matches(Q.w, Q.nm, T.w, T.nm, qo + B.q0, to + (uint64_t)((int64_t)B.q0 + B.d), v) : 0u;
          const CmpLink y = cmp_link_after(st[a], a, B, v, mt);
          if (cmp_link_before(y, x)) x = y;
        }
        for (int off = 1; off < 64; off <<= 1) {
          const CmpLink y = cmp_shfl_down(x, off);
          if (cmp_link_before(y, x)) x = y;
        }
      }
      if (lane == 0) {
        const CmpLink own = cmp_link_alone(B);
        if (!cmp_value_greater(x, own)) x = own;              // (their block counts differ: never equal)
        st[b] = x;
        if (cmp_value_greater(x, best)) { best = x; best.pred = b; }
      }
      if (b + 1 < b1) __threadfence();
    }
    if (lane == 0) top[g] = best;
  }
}

// The first group of a (query, target) pair picks the pair's orientation: the greater value, '+' of equals.  keep: the chain
// holds min_matches matches or more; nblk: its blocks (0 where no row is written).
__global__ void cmp_chain_pick_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ gstart, uint64_t n_groups, const CmpLink* __restrict__ top,
                                      uint32_t min_matches, uint32_t* __restrict__ keep, uint32_t* __restrict__ nblk, uint32_t* __restrict__ win) {
  SHN_GRID_FOR(g, n_groups) {
    const uint64_t pair = keys[gstart[g]] >> (CMP_QBITS + 1);
    uint32_t k = 0, nb = 0;
    if (g == 0 || (keys[gstart[g - 1]] >> (CMP_QBITS + 1)) != pair) {
      uint64_t w = g;
      if (g + 1 < n_groups && (keys[gstart[g + 1]] >> (CMP_QBITS + 1)) == pair && cmp_value_greater(top[g + 1], top[g])) w = g + 1;
      win[g] = (uint32_t)w;
      if (top[w].M >= min_matches) { k = 1; nb = top[w].R; }
    }
    keep[g] = k;
    nblk[g] = nb;
  }
}

// A thread per row: walks the winning chain back from its last block and writes the blocks in chain order.
// rows[f * n_rows + r]: the eight columns of cmp_rows_kernel (matches and mismatches summed over the blocks, qStart of the first
// block, qEnd of the last, tStart of the whole on the forward strand); gaps[f * n_rows + r], f = qNumInsert, qBaseInsert,
// tNumInsert, tBaseInsert, blockCount; blocks[f * n_blocks + k], f = size, qStart, tStart (forward strand)
__global__ void cmp_chain_rows_kernel(CmpText T, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ gstart, uint64_t n_groups, uint64_t m, int jo_bits,
                                      const CmpBlock* __restrict__ blk, const CmpLink* __restrict__ st, const CmpLink* __restrict__ top,
                                      const uint32_t* __restrict__ keep, const uint32_t* __restrict__ win, const uint64_t* __restrict__ rpos,
                                      const uint64_t* __restrict__ bpos, uint64_t n_rows, uint64_t n_blocks, uint32_t* __restrict__ rows,
                                      uint32_t* __restrict__ gaps, uint32_t* __restrict__ blocks) {
  SHN_GRID_FOR(g, n_groups) {
    if (!keep[g]) continue;
    const uint32_t w = win[g];
    const CmpLink C = top[w];
    const CmpGroup G = cmp_group_of(keys[gstart[w]], jo_bits, m);
    const int64_t Lt = (int64_t)(T.off[G.t + 1] - T.off[G.t]);
    const uint64_t r = rpos[g], bp = bpos[g];
    uint32_t e = C.pred, k = C.R, qn = 0, qb = 0, tn = 0, tb = 0, q_first = 0;
    const uint32_t q_end = blk[e].q0 + blk[e].len;
    const int64_t t_end = (int64_t)q_end + blk[e].d;
    int64_t t_first = 0;
    while (k) {
      k--;
      const CmpBlock B = blk[e];
      const CmpLink L = st[e];
      const uint32_t size = B.len - L.v, qs = B.q0 + L.v;
      const int64_t ts = (int64_t)qs + B.d;
      blocks[bp + k] = size;
      blocks[n_blocks + bp + k] = qs;
      blocks[2 * n_blocks + bp + k] = (uint32_t)(G.o ? Lt - (ts + (int64_t)size) : ts);
      if (L.pred == CMP_NONE) { q_first = qs; t_first = ts; break; }
      const CmpBlock A = blk[L.pred];
      const int64_t qg = (int64_t)qs - ((int64_t)A.q0 + A.len), tg = ts - ((int64_t)A.q0 + A.len + A.d);
      if (qg > 0) { qn++; qb += (uint32_t)qg; }
      if (tg > 0) { tn++; tb += (uint32_t)tg; }
      e = L.pred;
    }
    rows[r] = (uint32_t)G.i;
    rows[n_rows + r] = (uint32_t)G.j;
    rows[2 * n_rows + r] = G.o;
    rows[3 * n_rows + r] = C.M;
    rows[4 * n_rows + r] = (uint32_t)((int32_t)C.M - C.S) / 2u;
    rows[5 * n_rows + r] = q_first;
    rows[6 * n_rows + r] = q_end;
    rows[7 * n_rows + r] = (uint32_t)(G.o ? Lt - t_end : t_first);
    gaps[r] = qn; gaps[n_rows + r] = qb; gaps[2 * n_rows + r] = tn; gaps[3 * n_rows + r] = tb; gaps[4 * n_rows + r] = C.R;
  }
}


int check_offsets(const char* what, const uint64_t* off, uint64_t n) {
  if (off[0] != 0) return shn_fail(SHN_ERR_ARG, std::string("shn_compare_rows: ") + what + "_off[0] is not 0");
  for (uint64_t j = 0; j < n; j++) {
    if (off[j + 1] < off[j]) return shn_fail(SHN_ERR_ARG, std::string("shn_compare_rows: ") + what + "_off not monotone");
    if (off[j + 1] - off[j] >= CMP_DBIAS)
      return shn_fail(SHN_ERR_OVERFLOW, std::string("shn_compare_rows: a sequence of 2^20 bases or more (") + what + " " + std::to_string(j) + ")");
  }
  return SHN_OK;
}

// upload + pack; *out views the packed text (rc: the reverse complements behind it, their offsets appended to off)
int pack_text(shn_ctx* ctx, ShnDevBufs& B, const uint8_t* text, const uint64_t* off, uint64_t n_seq, bool rc, CmpText* out) {
  hipStream_t s = ctx->stream;
  const uint64_t total = off[n_seq], n_out = rc ? 2 * total : total, n_o = rc ? 2 * n_seq : n_seq;
  std::vector<uint64_t> o(n_o + 1);
  for (uint64_t j = 0; j <= n_seq; j++) o[j] = off[j];
  if (rc) for (uint64_t j = 1; j <= n_seq; j++) o[n_seq + j] = total + off[j];
  uint8_t* d_text = nullptr;
  uint64_t *d_w = nullptr, *d_nm = nullptr, *d_off = nullptr;
  const uint64_t n_grp = cdiv(n_out, 64);
  HIP_TRY(B.get(&d_text, total + 1));
  HIP_TRY(B.get(&d_w, (2 * n_grp + 2) * 8));
  HIP_TRY(B.get(&d_nm, (n_grp + 2) * 8));
  HIP_TRY(B.get(&d_off, (n_o + 1) * 8));
  if (total) HIP_TRY(hipMemcpyAsync(d_text, text, total, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_off, o.data(), (n_o + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));                          // (o is this frame's)
  HIP_TRY(hipMemsetAsync(d_w + 2 * n_grp, 0, 16, s));
  HIP_TRY(hipMemsetAsync(d_nm + n_grp, 0, 16, s));
  if (n_out) hipLaunchKernelGGL(cmp_pack_kernel, dim3(shn_grid(n_grp, CMP_BLK)), dim3(CMP_BLK), 0, s, (const uint8_t*)d_text, (const uint64_t*)d_off, n_seq, total, n_out, d_w, d_nm);
  HIP_TRY(hipGetLastError());
  out->w = d_w; out->nm = d_nm; out->off = d_off; out->n_seq = n_o; out->total = n_out;
  return SHN_OK;
}

}  // namespace

struct shn_cmprows {
  uint64_t n_rows = 0, n_hits = 0, n_cand = 0, n_rec = 0;
  std::vector<uint32_t> rows;          // 8 columns of n_rows
  // shn_compare_chains alone
  bool chained = false;
  uint64_t n_blocks = 0, n_groups = 0;
  std::vector<uint32_t> gaps;          // 5 columns of n_rows: qNumInsert, qBaseInsert, tNumInsert, tBaseInsert, blockCount
  std::vector<uint32_t> blocks;        // 3 columns of n_blocks: size, qStart, tStart; a row's blocks lie together, rows in order
};

namespace {

// The chained rows from the scored candidates: block order (one stable sort), groups, the chain kernel, the pair's orientation,
// two scans and the rows with their blocks.
int chain_rows(shn_ctx* ctx, ShnDevBufs& B, const CmpText& Q, const CmpText& T, const uint64_t* d_ucand, uint64_t n_cand, uint64_t n_t, int i_shift, int i_bits,
               const int32_t* d_s, const uint32_t* d_len, const uint32_t* d_q0, uint32_t min_matches, shn_cmprows* R) {
  hipStream_t s = ctx->stream;
  int rc;
  const int jo_bits = i_shift - CMP_DBITS, key_bits = CMP_QBITS + jo_bits + i_bits;
  uint64_t *d_keys = nullptr, *d_keys_tmp = nullptr, *d_rpos = nullptr, *d_bpos = nullptr;
  uint32_t *d_perm = nullptr, *d_perm_tmp = nullptr, *d_head = nullptr, *d_keep = nullptr, *d_nblk = nullptr, *d_win = nullptr;
  uint32_t *d_rows = nullptr, *d_gaps = nullptr, *d_blocks = nullptr;
  CmpBlock* d_blk = nullptr;
  CmpLink *d_st = nullptr, *d_top = nullptr;
  uint64_t n_rows = 0, n_blocks = 0;
  HIP_TRY(B.get(&d_keys, (n_cand + 1) * 8)); HIP_TRY(B.get(&d_keys_tmp, (n_cand + 1) * 8));
  HIP_TRY(B.get(&d_perm, (n_cand + 1) * 4)); HIP_TRY(B.get(&d_perm_tmp, (n_cand + 1) * 4));
  HIP_TRY(B.get(&d_head, (n_cand + 1) * 4));
  HIP_TRY(B.get(&d_blk, n_cand * sizeof(CmpBlock))); HIP_TRY(B.get(&d_st, n_cand * sizeof(CmpLink)));
  TimerRegion treg(ctx, T_CMP_CHAIN);
  hipLaunchKernelGGL(cmp_chain_keys_kernel, dim3(shn_grid(n_cand, CMP_BLK)), dim3(CMP_BLK), 0, s, d_ucand, d_len, d_q0, n_cand, d_keys, d_perm);
  if ((rc = shn_sort_pairs(ctx, d_keys, d_perm, d_keys_tmp, d_perm_tmp, n_cand, 0, key_bits))) return rc;
  hipLaunchKernelGGL(cmp_blocks_kernel, dim3(shn_grid(n_cand, CMP_BLK)), dim3(CMP_BLK), 0, s, (const uint64_t*)d_keys, (const uint32_t*)d_perm, n_cand, d_ucand, d_s, d_len, d_q0,
                     d_blk, d_head);
  ShnRuns groups;                               // a group = the blocks of one (query, target, orientation)
  if ((rc = shn_runs_from_heads(ctx, B, d_head, n_cand, nullptr, SHN_RUNS_START, &groups))) return rc;
  const uint64_t n_groups = groups.n_runs;
  const uint32_t* d_gstart = groups.start;
  HIP_TRY(B.get(&d_top, n_groups * sizeof(CmpLink)));
  HIP_TRY(B.get(&d_keep, (n_groups + 1) * 4)); HIP_TRY(B.get(&d_nblk, (n_groups + 1) * 4)); HIP_TRY(B.get(&d_win, n_groups * 4));
  HIP_TRY(B.get(&d_rpos, (n_groups + 2) * 8)); HIP_TRY(B.get(&d_bpos, (n_groups + 2) * 8));
  hipLaunchKernelGGL(cmp_chain_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(n_groups, CMP_BLK / 64), 1u << 20)), dim3(CMP_BLK), 0, s, Q, T, (const uint64_t*)d_keys,
                     d_gstart, n_groups, n_t, jo_bits, (const CmpBlock*)d_blk, d_st, d_top);
  hipLaunchKernelGGL(cmp_chain_pick_kernel, dim3(shn_grid(n_groups, CMP_BLK)), dim3(CMP_BLK), 0, s, (const uint64_t*)d_keys, d_gstart, n_groups,
                     (const CmpLink*)d_top, min_matches, d_keep, d_nblk, d_win);
  HIP_TRY(hipGetLastError());
  if ((rc = shn_device_scan_u32(ctx, d_keep, n_groups, d_rpos, &n_rows))) return rc;
  if ((rc = shn_device_scan_u32(ctx, d_nblk, n_groups, d_bpos, &n_blocks))) return rc;
  // bytes: per candidate its key, length and start read and the sort pair written (16 + 12 B), the sort's passes (24 B a pass), the
  // pair, key and three results read and the block and its head flag written, scanned and read (36 + 20 + 20 B), a block read and
  // its link written by the chain kernel (16 + 24 B; the blocks in front of it and the trimmed stretches of the packed texts come
  // from the caches); per group its start, best chain, three flags and two scans (4 + 24 + 12 + 40 B); per row 13 values and per
  // block 3 written with the block and link they are made of (52 B, 12 + 40 B)
  treg.bytes(n_cand * (28 + 76 + 40) + (uint64_t)((key_bits + 7) / 8) * n_cand * 24 + n_groups * 80 + n_rows * 52 + n_blocks * 52);
  R->n_rows = n_rows; R->n_blocks = n_blocks; R->n_groups = n_groups;
  R->rows.resize(n_rows * 8); R->gaps.resize(n_rows * 5); R->blocks.resize(n_blocks * 3);
  if (n_rows) {
    HIP_TRY(B.get(&d_rows, n_rows * 8 * 4)); HIP_TRY(B.get(&d_gaps, n_rows * 5 * 4)); HIP_TRY(B.get(&d_blocks, n_blocks * 3 * 4));
    hipLaunchKernelGGL(cmp_chain_rows_kernel, dim3(shn_grid(n_groups, CMP_BLK)), dim3(CMP_BLK), 0, s, T, (const uint64_t*)d_keys, d_gstart, n_groups, n_t, jo_bits,
                       (const CmpBlock*)d_blk, (const CmpLink*)d_st, (const CmpLink*)d_top, (const uint32_t*)d_keep, (const uint32_t*)d_win, (const uint64_t*)d_rpos,
                       (const uint64_t*)d_bpos, n_rows, n_blocks, d_rows, d_gaps, d_blocks);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(R->rows.data(), d_rows, n_rows * 8 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(R->gaps.data(), d_gaps, n_rows * 5 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(R->blocks.data(), d_blocks, n_blocks * 3 * 4, hipMemcpyDeviceToHost, s));
  }
  return SHN_OK;
}


// shn_compare_rows (chain == false) and shn_compare_chains: one path up to the scored candidates
int compare_rows(shn_ctx* ctx, const uint8_t* q_text, const uint64_t* q_off, uint64_t n_q, const uint8_t* t_text, const uint64_t* t_off, uint64_t n_t,
                 int strand_specific, uint32_t min_matches, bool chain, shn_cmprows** out) {
  if (!ctx || !q_off || !t_off || !out) return shn_fail(SHN_ERR_ARG, "shn_compare_rows: NULL argument");
  *out = nullptr;
  int rc;
  if ((rc = check_offsets("q", q_off, n_q)) || (rc = check_offsets("t", t_off, n_t))) return rc;
  if ((q_off[n_q] && !q_text) || (t_off[n_t] && !t_text)) return shn_fail(SHN_ERR_ARG, "shn_compare_rows: NULL text");
  const uint64_t n_o = strand_specific ? n_t : 2 * n_t;
  if (t_off[n_t] >= 0x7FFFFF00ULL) return shn_fail(SHN_ERR_OVERFLOW, "shn_compare_rows: 2^31 target bases or more in one call");
  const int t_bits = shn_bits_for(2 * n_t), i_bits = shn_bits_for(n_q), i_shift = CMP_DBITS + t_bits;
  if (i_shift + i_bits > 64) return shn_fail(SHN_ERR_OVERFLOW, "shn_compare_rows: queries times targets do not fit the 64-bit candidate key");
  std::vector<uint64_t> rec_off(n_o + 1, 0);
  for (uint64_t t = 0; t < n_o; t++) {
    const uint64_t j = t < n_t ? t : t - n_t, len = t_off[j + 1] - t_off[j];
    rec_off[t + 1] = rec_off[t] + (len >= CMP_SEED ? len - CMP_SEED + 1 : 0);
  }
  const uint64_t n_rec = rec_off[n_o];
  shn_cmprows* R = new shn_cmprows();
  R->n_rec = n_rec;
  R->chained = chain;
  *out = R;
  if (n_q == 0 || q_off[n_q] < CMP_SEED || n_rec == 0) return SHN_OK;
  struct Guard { shn_cmprows** o; bool ok = false; ~Guard() { if (!ok) { delete *o; *o = nullptr; } } } guard{out};
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs B(s);

  // ---- index
  CmpText Q, T;
  uint64_t *d_roff = nullptr, *d_keys = nullptr, *d_keys_tmp = nullptr;
  uint32_t *d_vals = nullptr, *d_vals_tmp = nullptr;
  HIP_TRY(B.get(&d_roff, (n_o + 1) * 8));
  HIP_TRY(B.get(&d_keys, (n_rec + 1) * 8)); HIP_TRY(B.get(&d_keys_tmp, (n_rec + 1) * 8));
  HIP_TRY(B.get(&d_vals, (n_rec + 1) * 4)); HIP_TRY(B.get(&d_vals_tmp, (n_rec + 1) * 4));
  HIP_TRY(hipMemcpyAsync(d_roff, rec_off.data(), (n_o + 1) * 8, hipMemcpyHostToDevice, s));
  {
    TimerRegion treg(ctx, T_CMP_INDEX);
    if ((rc = pack_text(ctx, B, q_text, q_off, n_q, false, &Q)) || (rc = pack_text(ctx, B, t_text, t_off, n_t, !strand_specific, &T))) return rc;
    // bytes: both texts read (1 B a base; the targets twice with their reverse complements) and written packed (2 + 1 bits a base),
    // a record written (12 B), every one of the sort's five 8-bit passes reads and writes the records
    treg.bytes(Q.total + T.total + (Q.total + T.total) * 3 / 8 + n_rec * 12 + 5 * n_rec * 24);
    hipLaunchKernelGGL(cmp_records_kernel, dim3(shn_grid(n_rec, CMP_BLK)), dim3(CMP_BLK), 0, s, T, (const uint64_t*)d_roff, n_rec, d_keys, d_vals);
    if ((rc = shn_sort_pairs(ctx, d_keys, d_vals, d_keys_tmp, d_vals_tmp, n_rec, 0, 2 * CMP_SEED + 1))) return rc;
  }

  // ---- seeds: candidates counted, scanned, filled, sorted, made unique
  uint32_t* d_cnt = nullptr;
  uint64_t *d_pos = nullptr, *d_cand = nullptr, *d_cand_tmp = nullptr;
  const uint64_t* d_ucand = nullptr;
  uint64_t n_hits = 0, n_cand = 0;
  HIP_TRY(B.get(&d_cnt, (Q.total + 1) * 4)); HIP_TRY(B.get(&d_pos, (Q.total + 2) * 8));
  {
    TimerRegion treg(ctx, T_CMP_SEEDS);
    hipLaunchKernelGGL(cmp_seed_kernel<false>, dim3(shn_grid(Q.total, CMP_BLK)), dim3(CMP_BLK), 0, s, Q, T, (const uint64_t*)d_keys, (const uint32_t*)d_vals, n_rec, n_t, i_shift,
                       d_cnt, (const uint64_t*)nullptr, (uint64_t*)nullptr);
    if ((rc = shn_device_scan_u32(ctx, d_cnt, Q.total, d_pos, &n_hits))) return rc;
    if (n_hits >= 0xFFFFFFFEULL) return shn_fail(SHN_ERR_OVERFLOW, "shn_compare_rows: 2^32 seed hits or more in one call (" + std::to_string(n_hits) + ")");
    HIP_TRY(B.get(&d_cand, (n_hits + 1) * 8)); HIP_TRY(B.get(&d_cand_tmp, (n_hits + 1) * 8));
    // bytes: per query base its words and mask (3 bits, twice: count and fill), 4 B of count, 8 B of offset written and read; the
    // index (12 B a record) and the targets' packed text are re-read from the caches and priced once; 8 B per hit written; the
    // sort reads and writes them once per 8-bit pass; heads, scan and compaction touch 8 + 4 + 8 + 8 B per hit
    const uint64_t passes = (uint64_t)(i_shift + i_bits + 7) / 8;
    treg.bytes(Q.total * 3 / 4 + Q.total * 20 + n_rec * 12 + T.total * 3 / 8 + n_hits * 8 + passes * n_hits * 16 + n_hits * 28);
    if (n_hits) {
      hipLaunchKernelGGL(cmp_seed_kernel<true>, dim3(shn_grid(Q.total, CMP_BLK)), dim3(CMP_BLK), 0, s, Q, T, (const uint64_t*)d_keys, (const uint32_t*)d_vals, n_rec, n_t, i_shift,
                         (uint32_t*)nullptr, (const uint64_t*)d_pos, d_cand);
      uint64_t* sorted = nullptr;
      if ((rc = shn_sort_keys(ctx, d_cand, d_cand_tmp, n_hits, 0, i_shift + i_bits, &sorted))) return rc;
      ShnRuns runs;
      if ((rc = shn_sorted_runs(ctx, B, sorted, n_hits, 0, SHN_RUNS_KEYS, &runs))) return rc;
      n_cand = runs.n_runs; d_ucand = runs.keys;
    }
  }
  R->n_hits = n_hits; R->n_cand = n_cand;
  if (n_cand == 0) { HIP_TRY(hipStreamSynchronize(s)); guard.ok = true; return SHN_OK; }

  // ---- score
  int32_t* d_s = nullptr;
  uint32_t *d_len = nullptr, *d_q0 = nullptr, *d_keep = nullptr, *d_best = nullptr, *d_rows = nullptr;
  uint64_t* d_rpos = nullptr;
  HIP_TRY(B.get(&d_s, n_cand * 4)); HIP_TRY(B.get(&d_len, n_cand * 4)); HIP_TRY(B.get(&d_q0, n_cand * 4));
  if (!chain) { HIP_TRY(B.get(&d_keep, (n_cand + 1) * 4)); HIP_TRY(B.get(&d_best, n_cand * 4)); HIP_TRY(B.get(&d_rpos, (n_cand + 2) * 8)); }
  {
    TimerRegion treg(ctx, T_CMP_SCORE);
    // bytes: a candidate read (8 B), four offsets (32 B), three results written (12 B); the diagonals' bases come from the packed
    // texts, which are re-read from the caches and priced once
    treg.bytes(n_cand * 52 + (Q.total + T.total) * 3 / 8);
    hipLaunchKernelGGL(cmp_score_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(n_cand, CMP_BLK / 64), 1u << 20)), dim3(CMP_BLK), 0, s, Q, T, d_ucand, n_cand,
                       n_t, i_shift, d_s, d_len, d_q0);
    HIP_TRY(hipGetLastError());
  }

  // ---- chained rows
  if (chain) {
    if ((rc = chain_rows(ctx, B, Q, T, d_ucand, n_cand, n_t, i_shift, i_bits, d_s, d_len, d_q0, min_matches, R))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    guard.ok = true;
    return SHN_OK;
  }

  // ---- rows
  uint64_t n_rows = 0;
  {
    TimerRegion treg(ctx, T_CMP_ROWS);
    hipLaunchKernelGGL(cmp_pairs_kernel, dim3(shn_grid(n_cand, CMP_BLK)), dim3(CMP_BLK), 0, s, d_ucand, n_cand, (const int32_t*)d_s, (const uint32_t*)d_len, min_matches,
                       d_keep, d_best);
    if ((rc = shn_device_scan_u32(ctx, d_keep, n_cand, d_rpos, &n_rows))) return rc;
    // bytes: per candidate its key, score and length read (16 B), the flag written, scanned and read (4 + 4 + 8 + 4 + 8 B), the
    // winner's index (4 B); per row 8 values written and what it reads of its winner (32 + 36 B)
    treg.bytes(n_cand * 48 + n_rows * 68);
    if (n_rows) {
      HIP_TRY(B.get(&d_rows, n_rows * 8 * 4));
      hipLaunchKernelGGL(cmp_rows_kernel, dim3(shn_grid(n_cand, CMP_BLK)), dim3(CMP_BLK), 0, s, T, d_ucand, n_cand, n_t, i_shift, (const int32_t*)d_s,
                         (const uint32_t*)d_len, (const uint32_t*)d_q0, (const uint32_t*)d_keep, (const uint32_t*)d_best, (const uint64_t*)d_rpos, n_rows, d_rows);
      HIP_TRY(hipGetLastError());
    }
  }
  R->n_rows = n_rows;
  R->rows.resize(n_rows * 8);
  if (n_rows) HIP_TRY(hipMemcpyAsync(R->rows.data(), d_rows, n_rows * 8 * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  guard.ok = true;
  return SHN_OK;
}

}  // namespace

extern "C" int shn_compare_rows(shn_ctx* ctx, const uint8_t* q_text, const uint64_t* q_off, uint64_t n_q, const uint8_t* t_text, const uint64_t* t_off,
                                uint64_t n_t, int strand_specific, uint32_t min_matches, shn_cmprows** out) {
  return compare_rows(ctx, q_text, q_off, n_q, t_text, t_off, n_t, strand_specific, min_matches, false, out);
}

extern "C" int shn_compare_chains(shn_ctx* ctx, const uint8_t* q_text, const uint64_t* q_off, uint64_t n_q, const uint8_t* t_text, const uint64_t* t_off,
                                  uint64_t n_t, int strand_specific, uint32_t min_matches, shn_cmprows** out) {
  return compare_rows(ctx, q_text, q_off, n_q, t_text, t_off, n_t, strand_specific, min_matches, true, out);
}

extern "C" int shn_cmprows_chain_sizes(const shn_cmprows* r, uint64_t* sizes3) {
  if (!r || !sizes3) return shn_fail(SHN_ERR_ARG, "shn_cmprows_chain_sizes: NULL argument");
  if (!r->chained) return shn_fail(SHN_ERR_ARG, "shn_cmprows_chain_sizes: the rows are shn_compare_rows', not shn_compare_chains'");
  uint64_t multi = 0;
  for (uint64_t k = 0; k < r->n_rows; k++) multi += r->gaps[4 * r->n_rows + k] > 1 ? 1 : 0;
  sizes3[0] = r->n_blocks; sizes3[1] = r->n_groups; sizes3[2] = multi;
  return SHN_OK;
}

extern "C" int shn_cmprows_chain_export(const shn_cmprows* r, uint32_t* gaps_out, uint64_t* block_off_out, uint32_t* blocks_out) {
  if (!r || !block_off_out || (r->n_rows && (!gaps_out || !blocks_out))) return shn_fail(SHN_ERR_ARG, "shn_cmprows_chain_export: NULL argument");
  if (!r->chained) return shn_fail(SHN_ERR_ARG, "shn_cmprows_chain_export: the rows are shn_compare_rows', not shn_compare_chains'");
  std::copy(r->gaps.begin(), r->gaps.end(), gaps_out);
  std::copy(r->blocks.begin(), r->blocks.end(), blocks_out);
  block_off_out[0] = 0;
  for (uint64_t k = 0; k < r->n_rows; k++) block_off_out[k + 1] = block_off_out[k] + r->gaps[4 * r->n_rows + k];
  return SHN_OK;
}

extern "C" int shn_cmprows_sizes(const shn_cmprows* r, uint64_t* sizes4) {
  if (!r || !sizes4) return shn_fail(SHN_ERR_ARG, "shn_cmprows_sizes: NULL argument");
  sizes4[0] = r->n_rows; sizes4[1] = r->n_cand; sizes4[2] = r->n_hits; sizes4[3] = r->n_rec;
  return SHN_OK;
}

extern "C" int shn_cmprows_export(const shn_cmprows* r, uint32_t* rows_out) {
  if (!r || (r->n_rows && !rows_out)) return shn_fail(SHN_ERR_ARG, "shn_cmprows_export: NULL argument");
  std::copy(r->rows.begin(), r->rows.end(), rows_out);
  return SHN_OK;
}

extern "C" void shn_cmprows_destroy(shn_cmprows* r) { delete r; }
