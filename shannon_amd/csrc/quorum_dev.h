// --quorum: what the kernels of quorum.hip share -- a k-mer carried together with its reverse complement, and the
// walk of one direction of one read.  Plain C++ behind one qualifier, as record_expand.h (whose ReadSetView / ReadCursor read the
// packed bases from whole 64-bit words).
#pragma once
#include "record_expand.h"

constexpr int QUORUM_MAX_E = 4;      // substitutions a walk keeps in registers for the revert: the largest E a call may ask for

// a k-mer x (2k bits, first base in the high bits) and RC(x); can(x) is the smaller of the two
struct QKmer {
  uint64_t fw, rc;
  SHN_XHD uint64_t can() const { return fw < rc ? fw : rc; }
};
// x[1:] + c
SHN_XHD QKmer q_append(const QKmer& x, uint32_t c, int k, uint64_t kmask) {
  return QKmer{((x.fw << 2) | c) & kmask, (x.rc >> 2) | ((uint64_t)(3 - c) << (2 * (k - 1)))};
}
// c + x[:-1]
SHN_XHD QKmer q_prepend(const QKmer& x, uint32_t c, int k, uint64_t kmask) {
  return QKmer{(x.fw >> 2) | ((uint64_t)c << (2 * (k - 1))), ((x.rc << 2) | (3 - c)) & kmask};
}
template <bool FWD> SHN_XHD QKmer q_step(const QKmer& x, uint32_t c, int k, uint64_t kmask) {
  return FWD ? q_append(x, c, k, kmask) : q_prepend(x, c, k, kmask);
}

// base p of a read of the OUTPUT set (words at ow, mask at om: the read's own words, nobody else's) becomes `code` (4: the base
// outside ACGT it was -- packed as 0 with its mask bit set, as the pack kernel leaves it)
SHN_XHD void q_put(uint64_t* ow, uint64_t* om, uint32_t p, uint32_t code) {
  const uint32_t sh = 62 - 2 * (p & 31);
  const uint64_t w = ow[p >> 5] & ~(3ULL << sh);
  ow[p >> 5] = w | ((uint64_t)(code & 3) << sh);
  const uint64_t bit = 1ULL << (63 - (p & 63));
  const uint64_t m = om[p >> 6];
  om[p >> 6] = code == 4 ? (m | bit) : (m & ~bit);
}

struct QWalkStats { uint32_t subs, stops, reverts; };

// Rules 3 / 4: one direction from the anchor k-mer x.  Step d (0 .. n_steps - 1) looks at base p = p0 + d (FWD) or p0 - d; the
// bases it reads are the read's own (`cur`: the working copy differs from them only behind the walk), what it substitutes goes to
// the output read (ow / om).  present(QKmer) is the table probe.  The last QUORUM_MAX_E substitutions (step, original code) are
// held in hd / ho, newest first: every substitution within the window of a step is among them, because a walk that finds E <=
// QUORUM_MAX_E of them there ends.
// Returns the steps the walk vouches for (rule 6): n_steps at the read's end, d at a stop, the smallest step among
// the substitutions it set back at a window revert.  A caller that drops the value pays nothing for it.
template <bool FWD, class Cursor, class Present>
SHN_XHD uint32_t q_walk(Cursor& cur, uint64_t* ow, uint64_t* om, QKmer x, int k, uint64_t kmask, uint32_t W, uint32_t E, uint32_t p0, uint32_t n_steps,
                    Present&& present, QWalkStats& st) {
  uint32_t hd[QUORUM_MAX_E], ho[QUORUM_MAX_E], nh = 0;
#pragma unroll
  for (int i = 0; i < QUORUM_MAX_E; i++) { hd[i] = 0; ho[i] = 0; }
  for (uint32_t d = 0; d < n_steps; d++) {
    const uint32_t p = FWD ? p0 + d : p0 - d;
    const uint32_t r = cur.code(p);
    if (r < 4) {
      const QKmer y = q_step<FWD>(x, r, k, kmask);
      if (present(y)) { x = y; continue; }
    }
    uint32_t S = 0;
#pragma unroll
    for (uint32_t c = 0; c < 4; c++)
      if (c != r && present(q_step<FWD>(x, c, k, kmask))) S |= 1u << c;
    if ((S & (S - 1)) != 0) {                                    // two candidates or more: the next base of the read decides, or nothing does
      uint32_t S2 = 0;
      if (d + 1 < n_steps) {
        const uint32_t nx = cur.code(FWD ? p + 1 : p - 1);
        if (nx < 4) {
#pragma unroll
          for (uint32_t c = 0; c < 4; c++)
            if (((S >> c) & 1) && present(q_step<FWD>(q_step<FWD>(x, c, k, kmask), nx, k, kmask))) S2 |= 1u << c;
        }
      }
      S = (S2 && (S2 & (S2 - 1)) == 0) ? S2 : 0;
    }
    if (!S) { st.stops++; return d; }
    const uint32_t c = S & 1 ? 0u : S & 2 ? 1u : S & 4 ? 2u : 3u;
    // substitutions of this direction inside the window: steps d' with d - W < d' < d
    uint32_t in_window = 0;
#pragma unroll
    for (int i = 0; i < QUORUM_MAX_E; i++) in_window += ((uint32_t)i < nh && (uint64_t)hd[i] + W > d) ? 1u : 0u;
    if (in_window >= E) {
      uint32_t first = d;
#pragma unroll
      for (int i = 0; i < QUORUM_MAX_E; i++)
        if ((uint32_t)i < nh && (uint64_t)hd[i] + W > d) {
          q_put(ow, om, FWD ? p0 + hd[i] : p0 - hd[i], ho[i]); st.subs--;
          first = hd[i] < first ? hd[i] : first;
        }
      st.reverts++; st.stops++;
      return first;
    }
    q_put(ow, om, p, c);
#pragma unroll
    for (int i = QUORUM_MAX_E - 1; i > 0; i--) { hd[i] = hd[i - 1]; ho[i] = ho[i - 1]; }
    hd[0] = d; ho[0] = r;
    nh = nh < (uint32_t)QUORUM_MAX_E ? nh + 1 : nh;
    st.subs++;
    x = q_step<FWD>(x, c, k, kmask);
  }
  return n_steps;
}
