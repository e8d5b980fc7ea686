// The two searches and the bit count of shannon_amd/csrc/runs.h on the host, for a run under sanitizers: shn_segment_of and
// shn_lower_bound against a linear scan on offset arrays with empty segments at the front, in the middle and at the end, n = 1, and
// g up to the last offset minus 1 (and past it); shn_bits_for at 0, 1 and around every power of two against the three loops it
// replaced.  Every array is a heap block of exactly the elements the search may read -- n offsets, not n + 1 -- so a read of
// off[n] or keys[n] is a heap overflow.  Exit code 0: no difference.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/probes/runs_host_check.cpp -o /tmp/runs_host_check && /tmp/runs_host_check
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>
#include "../../shannon_amd/csrc/runs.h"

static long bad = 0, n_checks = 0;
static void miss(const char* what, uint64_t n, uint64_t at, uint64_t got, uint64_t want) {
  if (bad++ < 10) printf("%s: n %llu at %llu: %llu, expected %llu\n", what, (unsigned long long)n, (unsigned long long)at, (unsigned long long)got, (unsigned long long)want);
}

// lens: the segments' lengths; searched: off[0 .. n), its n entries and no more
static void check_offsets(const std::vector<uint64_t>& lens, uint64_t base) {
  const uint64_t n = lens.size();
  std::vector<uint64_t> full(n + 1, base);
  for (uint64_t j = 0; j < n; j++) full[j + 1] = full[j] + lens[j];
  std::unique_ptr<uint64_t[]> off(new uint64_t[n]);
  for (uint64_t j = 0; j < n; j++) off[j] = full[j];
  for (uint64_t g = base; g <= full[n] + 2; g++) {                  // (g >= off[n]: the last segment with off[j] <= g, as the callers' strided loops may ask)
    uint64_t want = 0;
    for (uint64_t j = 0; j < n; j++) if (full[j] <= g) want = j;
    const uint64_t got = shn_segment_of(off.get(), n, g);
    n_checks++;
    if (got != want) miss("segment_of", n, g, got, want);
    if (g < full[n] && !(full[got] <= g && g < full[got + 1])) miss("segment_of (g outside the segment)", n, g, got, want);
  }
  // the offsets themselves as sorted keys (ties where segments are empty): the lower bound of every value around them
  for (uint64_t key = base ? base - 1 : 0; key <= full[n] + 1; key++) {
    uint64_t want = n;
    for (uint64_t j = n; j-- > 0;) if (full[j] >= key) want = j;
    const uint64_t got = shn_lower_bound(off.get(), n, key);
    n_checks++;
    if (got != want) miss("lower_bound", n, key, got, want);
  }
}

int main() {
  check_offsets({5}, 0);                                             // n = 1
  check_offsets({1}, 0);
  check_offsets({0, 0, 4, 3}, 0);                                    // empty segments at the front
  check_offsets({4, 0, 0, 0, 3, 0, 2}, 0);                           // ... in the middle
  check_offsets({4, 3, 0, 0}, 0);                                    // ... at the end
  check_offsets({0, 0, 1, 0, 0}, 0);
  check_offsets({0, 5, 0}, 7);                                       // offsets that do not start at 0 (a window of a larger array)
  std::mt19937_64 rng(7);
  for (int it = 0; it < 2000; it++) {
    std::vector<uint64_t> lens(1 + rng() % 70);
    for (auto& l : lens) l = (rng() % 3) ? rng() % 9 : 0;
    if (lens.size() > 1 || lens[0]) check_offsets(lens, rng() % 5);
  }
  { // nothing to search: no key is read
    std::unique_ptr<uint64_t[]> none(new uint64_t[0]);
    n_checks++;
    if (shn_lower_bound(none.get(), 0, 5) != 0) { bad++; printf("lower_bound of no keys\n"); }
  }
  // shn_bits_for against the loops of the call sites it replaced
  auto compare_bits = [](uint64_t n) { int b = 1; while (b < 63 && (n - 1) >> b) b++; return b; };                      // n >= 1
  auto probe_bits = [](uint64_t n) { int b = 1; while ((1ULL << b) < n) b++; return b; };                             // n < 2^63
  auto filter_bits = [](uint64_t n) { int b = 30; while (b < 62 && (n >> (b - 30))) b++; return b - 30; };            // 1 <= n < 2^31
  std::vector<uint64_t> ns = {0, 1, 2, 3};
  for (int e = 2; e < 64; e++) { ns.push_back((1ULL << e) - 1); ns.push_back(1ULL << e); ns.push_back((1ULL << e) + 1); }
  ns.push_back(~0ULL);
  for (uint64_t n : ns) {
    const int got = shn_bits_for(n);
    n_checks++;
    const bool holds = got >= 1 && got <= 63 && (got == 63 || n <= (1ULL << got)) && (got == 1 || n > (1ULL << (got - 1)));
    if (!holds) miss("bits_for (the smallest b >= 1 with n <= 2^b)", n, n, got, 0);
    if (n >= 1 && got != compare_bits(n)) miss("bits_for against compare's loop", n, n, got, compare_bits(n));
    if (n >= 1 && n <= (1ULL << 62) && got != probe_bits(n)) miss("bits_for against the probe's loop", n, n, got, probe_bits(n));
    if (n >= 1 && n < (1ULL << 31) && shn_bits_for(n + 1) != filter_bits(n)) miss("bits_for(n + 1) against the filter's loop", n, n, shn_bits_for(n + 1), filter_bits(n));
  }
  const uint32_t grids[][3] = {{0, 256, 1}, {1, 256, 1}, {256, 256, 1}, {257, 256, 2}, {0xFFFFFFFFu, 256, 1u << 20}};
  for (auto& g : grids) { n_checks++; if (shn_grid(g[0], g[1]) != g[2]) { bad++; printf("grid(%u, %u) = %u\n", g[0], g[1], shn_grid(g[0], g[1])); } }
  printf("checks %ld bad %ld\n", n_checks, bad);
  return bad != 0;
}
