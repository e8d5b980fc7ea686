// The chained form's arithmetic of the comparison against a reference transcriptome (shannon_amd/csrc/compare_dev.h) on the host,
// for a run under sanitizers.  Random texts with a few N, packed as compare.hip packs them (2 bits a base, a mask bit a base, two
// zero words behind the end), each sequence at a random place of its text, so every word alignment of either comes up.
//   trim count   random blocks, every v in 0 .. len: cmp_trim_matches against a loop over the letters
//   chain step   groups of 1 .. 200 random blocks in the rule's order (half of them pieces of the query planted in the target, so
//                real chains form): per block the wave's work as cmp_chain_kernel does it -- lane l takes the predecessors l, l + 64,
//                .., keeps its best under cmp_link_before, the 64 lanes reduce through the shuffle tree (lane l takes lane
//                l + stride's value where that is before its own; a lane past the end picks up its own, as __shfl_down does), lane 0
//                decides against the block alone -- held against a plain quadratic loop over the predecessors in order.
// Exit code 0: no difference.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/probes/compare_chain_check.cpp -o /tmp/compare_chain_check && /tmp/compare_chain_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>
#include "../../shannon_amd/csrc/compare_dev.h"

struct Packed { std::vector<uint64_t> w, nm; };
static Packed pack(const std::string& s) {
  Packed P;
  const size_t grp = (s.size() + 63) / 64;
  P.w.assign(2 * grp + 2, 0);
  P.nm.assign(grp + 2, 0);
  for (size_t g = 0; g < s.size(); g++) {
    uint64_t c = 0;
    switch (s[g]) { case 'A': c = 0; break; case 'C': c = 1; break; case 'G': c = 2; break; case 'T': c = 3; break; default: P.nm[g >> 6] |= 1ULL << (63 - (g & 63)); }
    P.w[g >> 5] |= c << (62 - 2 * (g & 31));
  }
  return P;
}
static bool same(const CmpLink& a, const CmpLink& b) { return a.S == b.S && a.M == b.M && a.R == b.R && a.pred == b.pred && a.v == b.v && a.m == b.m; }

int main() {
  std::mt19937_64 rng(7);
  long bad = 0, n_trims = 0, n_groups = 0, n_links = 0, n_joined = 0;
  for (int it = 0; it < 400; it++) {
    const int r = it < 8 ? 1 + it : (it % 9 == 0 ? 180 + (int)(rng() % 21) : 1 + (int)(rng() % 140));
    const size_t Lq = 200 + rng() % 1800, Lt = 200 + rng() % 1800, pq = rng() % 70, pt = rng() % 70;
    std::string q(Lq, 'A'), t(Lt, 'A');
    for (auto& c : q) c = "ACGT"[rng() % 4];
    for (auto& c : t) c = "ACGT"[rng() % 4];
    // blocks: q0, len, d with both ends inside; half of them planted (the target made equal to the query there, a few substitutions)
    std::vector<CmpBlock> blk;
    for (int k = 0; k < r; k++) {
      const uint32_t len = 1 + (uint32_t)(rng() % (k % 5 == 0 ? 150 : 40));
      if (len > Lq || len > Lt) continue;
      const uint32_t q0 = (uint32_t)(rng() % (Lq - len + 1)), t0 = (uint32_t)(rng() % (Lt - len + 1));
      if (k % 2) for (uint32_t x = 0; x < len; x++) if (rng() % 20) t[t0 + x] = q[q0 + x];
      blk.push_back(CmpBlock{(int32_t)t0 - (int32_t)q0, q0, len, 0});
    }
    for (int k = 0; k < 6; k++) { q[rng() % Lq] = 'N'; t[rng() % Lt] = 'N'; }
    const std::string qtext = std::string(pq, 'C') + q + "GG", ttext = std::string(pt, 'T') + t + "A";
    const Packed Q = pack(qtext), T = pack(ttext);
    auto matches = [&](const CmpBlock& B, uint32_t from, uint32_t to) {
      uint32_t m = 0;
      for (uint32_t x = from; x < to; x++) { const char a = q[B.q0 + x], b = t[(int64_t)B.q0 + B.d + x]; m += (a == b && a != 'N') ? 1 : 0; }
      return m;
    };
    for (auto& B : blk) { const uint32_t m = matches(B, 0, B.len); B.s = (int32_t)m - 2 * (int32_t)(B.len - m); }
    std::sort(blk.begin(), blk.end(), [](const CmpBlock& a, const CmpBlock& b) { return a.q0 + a.len != b.q0 + b.len ? a.q0 + a.len < b.q0 + b.len : a.d < b.d; });
    // ---- trim count: every v of a few blocks
    for (size_t k = 0; k < blk.size() && k < 12; k++) {
      const CmpBlock& B = blk[k];
      for (uint32_t v = 0; v <= B.len; v++) {
        const uint32_t got = cmp_trim_matches(Q.w.data(), Q.nm.data(), T.w.data(), T.nm.data(), pq + B.q0, pt + (uint64_t)((int64_t)B.q0 + B.d), v);
        n_trims++;
        if (got != matches(B, 0, v)) { bad++; if (bad < 10) printf("trim: len %u v %u got %u want %u\n", B.len, v, got, matches(B, 0, v)); }
      }
    }
    // ---- chain step
    const uint32_t n = (uint32_t)blk.size();
    std::vector<CmpLink> st(n), ref(n);
    for (uint32_t b = 0; b < n; b++) {
      const CmpBlock& B = blk[b];
      auto link = [&](const std::vector<CmpLink>& state, uint32_t a, CmpLink* y) {
        uint32_t v;
        if (!cmp_joins(blk[a], B, &v)) return false;
        const uint32_t mt = v ? cmp_trim_matches(Q.w.data(), Q.nm.data(), T.w.data(), T.nm.data(), pq + B.q0, pt + (uint64_t)((int64_t)B.q0 + B.d), v) : 0u;
        *y = cmp_link_after(state[a], a, B, v, mt);
        return true;
      };
      // the wave
      CmpLink x[64];
      for (uint32_t l = 0; l < 64; l++) {
        x[l] = cmp_link_none();
        for (uint32_t a = l; a < b; a += 64) { CmpLink y; if (link(st, a, &y) && cmp_link_before(y, x[l])) x[l] = y; }
      }
      for (int off = 1; off < 64; off <<= 1) {
        CmpLink y[64];
        for (int l = 0; l < 64; l++) { const CmpLink o = l + off < 64 ? x[l + off] : x[l]; y[l] = cmp_link_before(o, x[l]) ? o : x[l]; }
        for (int l = 0; l < 64; l++) x[l] = y[l];
      }
      const CmpLink own = cmp_link_alone(B);
      st[b] = cmp_value_greater(x[0], own) ? x[0] : own;
      // the plain loop: predecessors in order, a later one only with a strictly greater value; the joins and the trimmed blocks from
      // the letters
      CmpLink best = own;
      const uint32_t m_all = matches(B, 0, B.len);
      if (own.M != m_all || own.S != (int32_t)m_all - 2 * (int32_t)(B.len - m_all)) { bad++; printf("alone\n"); }
      for (uint32_t a = 0; a < b; a++) {
        const CmpBlock& A = blk[a];
        const int64_t qe = (int64_t)A.q0 + A.len, te = qe + A.d, v = std::max<int64_t>(0, std::max(qe - (int64_t)B.q0, te - ((int64_t)B.q0 + B.d)));
        if (A.d == B.d || v >= (int64_t)B.len) continue;
        const uint32_t m = matches(B, (uint32_t)v, B.len), mm = B.len - (uint32_t)v - m;
        const CmpLink y{ref[a].S + (int32_t)m - 2 * (int32_t)mm, ref[a].M + m, ref[a].R + 1, a, (uint32_t)v, m};
        n_links++;
        if (y.S > best.S || (y.S == best.S && (y.M > best.M || (y.M == best.M && y.R < best.R)))) best = y;
      }
      ref[b] = best;
      n_joined += best.pred != CMP_NONE;
      if (!same(st[b], ref[b])) { bad++; if (bad < 10) printf("chain: group of %u, block %u: got %d %u %u %u want %d %u %u %u\n", n, b, st[b].S, st[b].M, st[b].R, st[b].pred, ref[b].S, ref[b].M, ref[b].R, ref[b].pred); }
    }
    n_groups++;
  }
  printf("groups %ld links %ld joined blocks %ld trims %ld bad %ld\n", n_groups, n_links, n_joined, n_trims, bad);
  return bad != 0;
}
