// The score arithmetic of the comparison against a reference transcriptome (shannon_amd/csrc/compare_dev.h) on the host, for a run
// under sanitizers: random diagonals through cmp_fold32 per 32 positions, the wave's shuffle tree (lane l combines itself with
// lane l + stride; a lane past the end picks up its own value, as __shfl_down does) and the carry across passes of 2,048
// positions, held against every start and every end.  Exit code 0: no difference.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/probes/compare_dev_check.cpp -o /tmp/compare_dev_check && /tmp/compare_dev_check
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <random>
#include "../../shannon_amd/csrc/compare_dev.h"
int main() {
  std::mt19937_64 rng(1);
  long bad = 0, n_cases = 0;
  for (int it = 0; it < 3000; it++) {
    int n = it < 200 ? it : (int)(rng() % 5000) + 1;
    double pm = (it % 5) * 0.08 + 0.01;
    std::vector<int> mis(n);
    for (auto& x : mis) x = (rng() % 10000) < pm * 10000;
    if (it % 7 == 0) for (int i = 0; i < n; i++) mis[i] = (i % 3 == 2);     // M M X pattern: many ties
    // device-shaped evaluation
    CmpSum carry = cmp_empty();
    for (int base = 0; base < n; base += 2048) {
      CmpSum x[64];
      for (int l = 0; l < 64; l++) {
        int s = base + 32 * l;
        x[l] = cmp_empty();
        if (s < n) {
          int len = n - s < 32 ? n - s : 32;
          uint64_t d = 0;
          for (int j = 0; j < len; j++) if (mis[s + j]) d |= 1ULL << (62 - 2 * j);
          x[l] = cmp_fold32(d, len);
        }
      }
      for (int off = 1; off < 64; off <<= 1) {
        CmpSum y[64];
        for (int l = 0; l < 64; l++) y[l] = cmp_combine(x[l], l + off < 64 ? x[l + off] : x[l]);
        for (int l = 0; l < 64; l++) x[l] = y[l];
      }
      carry = cmp_combine(carry, x[0]);
    }
    // brute force
    std::vector<long> P(n + 1, 0);
    for (int i = 0; i < n; i++) P[i + 1] = P[i] + (mis[i] ? -2 : 1);
    long bs = 0, bl = 0, b0 = 0; bool have = false;
    if (n <= 1500 || it % 10 == 0)
    {
      for (int s = 0; s < n; s++) for (int e = s + 1; e <= n; e++) {
        long v = P[e] - P[s], l = e - s;
        if (!have || v > bs || (v == bs && (l > bl || (l == bl && s < b0)))) { bs = v; bl = l; b0 = s; have = true; }
      }
      n_cases++;
      if (have && bs > 0 && (carry.bs != bs || carry.bl != bl || carry.b0 != b0)) { bad++; if (bad < 10) printf("n %d: got %d %u %u want %ld %ld %ld\n", n, carry.bs, carry.bl, carry.b0, bs, bl, b0); }
      if (carry.tot != P[n] || carry.len != (uint32_t)n) { bad++; printf("tot\n"); }
    }
  }
  printf("cases %ld bad %ld\n", n_cases, bad);
  return bad != 0;
}
