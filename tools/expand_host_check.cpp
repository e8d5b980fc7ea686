// The per-thread half of shn_reads_collect and of the --inDisk formatters (shannon_amd/csrc/record_expand.h: length functions,
// record search, expand_chunk, the three record types) run on the CPU against a plain per-record writer -- a program of its own,
// so that it can run under sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/expand_host_check.cpp -o expand_host_check
//   c++ -std=c++17 -O1 tools/expand_host_check.cpp -o expand_host_check
//   ./expand_host_check
// Offsets come from the header's length functions and a prefix sum; expand_chunk is called for every 16-byte chunk, in blocks of
// 256 whose first and last record are found as the kernel finds them.  Every array has exactly the size the calls allocate (the
// output: its bytes rounded up to 16, nothing more; the packed sets without their two spare words), so a read or write one element
// out of bounds is a sanitizer report.  Exit status 0 and "expand_host_check: OK" when every case holds.
#include "../shannon_amd/csrc/record_expand.h"
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static uint32_t g_x = 12345;
static uint32_t rnd(uint32_t n) { g_x = g_x * 1664525u + 1013904223u; return (g_x >> 8) % n; }

// ---- a packed read set as shn_reads_create lays it out: 2 bits a base MSB-first, every read on an even word; a mask bit per base
struct HostSet {
  std::vector<std::string> reads;               // over ACGTN
  std::vector<uint64_t> words, mask, woff;
  std::vector<uint32_t> len;
  uint32_t fixed_len = 0, wpr = 0;
  bool has_n = false;
  ReadSetView view() const {
    ReadSetView v;
    v.words = words.data(); v.mask = has_n ? mask.data() : nullptr;
    v.woff = fixed_len ? nullptr : woff.data(); v.len = fixed_len ? nullptr : len.data();
    v.n = reads.size(); v.fixed_len = fixed_len; v.wpr = wpr;
    return v;
  }
};
static uint64_t cdiv(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

static HostSet pack(const std::vector<std::string>& reads, uint32_t fixed_len) {
  HostSet S;
  S.reads = reads; S.fixed_len = fixed_len; S.wpr = fixed_len ? (uint32_t)(2 * cdiv(fixed_len, 64)) : 0;
  uint64_t w = 0;
  for (const std::string& r : reads) { S.woff.push_back(w); S.len.push_back((uint32_t)r.size()); w += fixed_len ? S.wpr : 2 * cdiv(r.size() ? r.size() : 1, 64); }
  S.woff.push_back(w);
  S.words.assign(w, 0); S.mask.assign(w / 2, 0);
  for (size_t r = 0; r < reads.size(); r++)
    for (size_t p = 0; p < reads[r].size(); p++) {
      const char* at = strchr("ACGT", reads[r][p]);
      if (at) S.words[S.woff[r] + p / 32] |= (uint64_t)(at - "ACGT") << (62 - 2 * (p % 32));
      else { S.mask[S.woff[r] / 2 + p / 64] |= 1ULL << (63 - p % 64); S.has_n = true; }
    }
  return S;
}

static std::string random_read(uint32_t len, const std::vector<uint32_t>& n_at = {}) {
  std::string s(len, 'A');
  for (uint32_t p = 0; p < len; p++) s[p] = "ACGT"[rnd(4)];
  for (uint32_t p : n_at) if (p < len) s[p] = 'N';
  return s;
}
static HostSet fixed_set(uint32_t n, uint32_t L, bool with_n) {
  std::vector<std::string> reads;
  for (uint32_t i = 0; i < n; i++) reads.push_back(random_read(L, with_n && i % 3 == 0 ? std::vector<uint32_t>{0, 31, 32, 63, 64, L - 1} : std::vector<uint32_t>{}));
  return pack(reads, L);
}
// empty reads first, last and three in a row; an N at bases 0, 31, 32, 63, 64 and the last base
static HostSet ragged_set(bool with_n) {
  const uint32_t lens[] = {0, 5, 0, 0, 0, 33, 64, 0, 1, 100, 65, 31, 250, 32, 129, 0, 63, 16, 0};
  std::vector<std::string> reads;
  for (int rep = 0; rep < 3; rep++)
    for (uint32_t L : lens) reads.push_back(random_read(L, with_n && L ? std::vector<uint32_t>{0, 31, 32, 63, 64, L - 1} : std::vector<uint32_t>{}));
  return pack(reads, 0);
}

static std::string revcomp(const std::string& s) {
  std::string r(s.rbegin(), s.rend());
  for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
  return r;
}

// ---- passes 2 and 3 as the calls run them over records [r0, r1) of `lens`; `rec` is the launch's record type, laid out for r0
template <class R>
static std::string expand(const R& rec, const std::vector<uint32_t>& lens, uint64_t r0, uint64_t r1, uint64_t cap) {
  const uint64_t n = r1 - r0;
  std::vector<uint64_t> all(lens.size() + 1, 0);
  for (size_t i = 0; i < lens.size(); i++) all[i + 1] = all[i] + lens[i];
  const std::vector<uint64_t> off(all.begin() + r0, all.begin() + r1 + 1);          // exactly n + 1 offsets; off[0] != 0 where r0 != 0
  const uint64_t base = off[0], total = std::min(off[n] - base, cap);
  if (total == 0) return std::string();                                           // (the calls launch nothing)
  const uint64_t room = cdiv(total, SHN_XCHUNK) * SHN_XCHUNK, per_block = (uint64_t)SHN_XBLK * SHN_XCHUNK;
  uint8_t* out = (uint8_t*)aligned_alloc(16, room);
  memset(out, 0xAB, room);
  const uint64_t grid = 2;                                                        // a grid of two blocks: a thread keeps its copy of the kernel argument from round to round
  std::vector<R> threads(grid * SHN_XBLK, rec);
  for (uint64_t blk = 0, b0 = 0; b0 < total; blk++, b0 += per_block) {
    const uint64_t first = record_of(off.data(), 0, n, base + b0), last = record_of(off.data(), 0, n, base + std::min(b0 + per_block, total) - 1);
    for (uint64_t t = 0; t < (uint64_t)SHN_XBLK; t++) {
      const uint64_t pos0 = b0 + t * SHN_XCHUNK;
      if (pos0 < total) expand_chunk(threads[(blk % grid) * SHN_XBLK + t], n, off.data(), first, last, total, pos0, out);
    }
  }
  for (uint64_t p = total; p < room; p++) CHECK(out[p] == 0xAB);                  // nothing at or behind the total
  std::string text((const char*)out, total);
  free(out);
  return text;
}
static void same(const std::string& got, const std::string& want, uint64_t cap, const char* what) {
  const std::string w = want.substr(0, std::min<uint64_t>(cap, want.size()));
  if (got != w) { fprintf(stderr, "FAILED %s: %zu bytes, expected %zu (cap %llu)\n", what, got.size(), w.size(), (unsigned long long)cap); failures++; }
}
// the whole output, and with a capacity of 0, 1 and 4,096 bytes less than it
template <class R>
static void check_caps(const R& rec, const std::vector<uint32_t>& lens, uint64_t r0, uint64_t r1, const std::string& want, const char* what) {
  for (uint64_t cut : {0ull, 1ull, 4096ull})
    if (cut <= want.size()) { const uint64_t cap = want.size() - cut; same(expand(rec, lens, r0, r1, cap), want, cap, what); }
  same(expand(rec, lens, r0, r1, ~0ULL), want, ~0ULL, what);
}

// ---- shn_reads_collect
static void check_collect(const HostSet& a, const HostSet& b, const std::vector<uint32_t>& sel, std::vector<uint8_t> flags, const char* what,
                          uint64_t expect_total = ~0ULL) {
  if (flags.empty()) flags.assign(sel.size(), 0);                                 // (all of set a)
  const ReadSetView A = a.view(), B = b.view();
  std::vector<uint32_t> lens(sel.size());
  std::string want;
  for (size_t i = 0; i < sel.size(); i++) {
    lens[i] = code_len(A, B, sel.data(), flags.data(), i);
    const std::string& r = (flags[i] ? b : a).reads[sel[i]];
    CHECK(lens[i] == r.size());
    for (char c : r) want += (char)(c == 'N' ? 4 : strchr("ACGT", c) - "ACGT");
  }
  if (expect_total != ~0ULL) CHECK(want.size() == expect_total);
  if (A.mask || B.mask) check_caps(CodeRec<true>{A, B, sel.data(), flags.data()}, lens, 0, sel.size(), want, what);
  else check_caps(CodeRec<false>{A, B, sel.data(), flags.data()}, lens, 0, sel.size(), want, what);
}

// ---- shn_reads_fasta: the table of include/shannon_hip.h, row by row
static void check_fasta(const HostSet& a, const HostSet& b, int ss, int mate, const std::vector<uint32_t>& ridx, uint64_t e0, const char* what) {
  const ReadSetView A = a.view(), B = mate ? b.view() : A;
  const ReadPick pick{a.reads.size(), ss, mate};
  const uint64_t N = a.reads.size(), n = ridx.size();
  std::vector<uint32_t> lens(n);
  std::vector<std::string> recs;
  for (uint64_t i = 0; i < n; i++) {
    bool ok;
    lens[i] = fasta_len(A, B, pick, ridx.data(), e0, i, &ok);
    const uint64_t d = ridx[i];
    std::string seq;
    if (ss) seq = mate == 2 ? revcomp(b.reads[d]) : a.reads[d];
    else if (mate == 0) seq = d < N ? a.reads[d] : revcomp(a.reads[d - N]);
    else if (mate == 1) seq = d < N ? a.reads[d] : revcomp(b.reads[d - N]);
    else seq = d < N ? revcomp(a.reads[d]) : b.reads[d - N];
    recs.push_back(">" + std::to_string(e0 + i) + (mate ? "_" + std::to_string(mate) : "") + "\n" + seq + "\n");
    CHECK(ok && lens[i] == recs.back().size());
  }
  // all records in one launch, and as the file drivers launch them: from any first record (off[0] != 0) on
  for (uint64_t r0 = 0; r0 < n; r0 += (r0 < 4 ? 1 : 17)) {
    std::string want;
    for (uint64_t i = r0; i < n; i++) want += recs[i];
    if (A.mask || B.mask) check_caps(FastaRec<true>{A, B, pick, ridx.data() + r0, e0 + r0}, lens, r0, n, want, what);
    else check_caps(FastaRec<false>{A, B, pick, ridx.data() + r0, e0 + r0}, lens, r0, n, want, what);
  }
}
static std::vector<uint32_t> routes(uint32_t n, uint32_t below) {
  std::vector<uint32_t> r(n);
  for (uint32_t& d : r) d = rnd(below);
  return r;
}

// ---- shn_k1mers_dict_text: every window of every contig, launches from any first window
static void check_dict(uint32_t k1) {
  const uint32_t clen[] = {k1, 0, k1 - 1, k1 + 40, k1 + 1, 3, 2 * k1, k1 + 330};  // (the last one: more than two blocks of text, a thread's contig carries on)
  std::string text;
  std::vector<uint64_t> coff(1, 0), woff(1, 0);
  for (uint32_t L : clen) { text += random_read(L); coff.push_back(text.size()); woff.push_back(woff.back() + (L >= k1 ? L - k1 + 1 : 0)); }
  const uint64_t n = woff.back(), big[] = {0, 9, 10, 99, 100, 999999999, 1000000000, 4294967295u};
  std::vector<uint32_t> weights(n), lens(n);
  std::vector<std::string> recs;
  for (uint64_t c = 0, i = 0; c + 1 < coff.size(); c++)
    for (uint64_t p = coff[c]; p + k1 <= coff[c + 1]; p++, i++) {
      weights[i] = (uint32_t)(i % 3 ? rnd(5000) : big[rnd(8)]);
      lens[i] = dict_len(weights.data(), k1, i);
      recs.push_back(text.substr(p, k1) + "\t" + std::to_string(weights[i]) + "\n");
      CHECK(lens[i] == recs.back().size());
    }
  CHECK(recs.size() == n);
  for (uint64_t r0 = 0; r0 < n; r0++)
    for (uint64_t r1 : {n, std::min(n, r0 + 1 + rnd(40))}) {
      std::string want;
      for (uint64_t i = r0; i < r1; i++) want += recs[i];
      DictRec R;
      R.text = (const uint8_t*)text.data(); R.coff = coff.data(); R.woff = woff.data(); R.n_strings = coff.size() - 1;
      R.weights = weights.data() + r0; R.w0 = r0; R.k1 = k1; R.c = ~0ULL; R.tpos = R.dlo = R.dhi = 0; R.dig = 0;
      if (r0 < 48 || r0 % 7 == 0) check_caps(R, lens, r0, r1, want, "k1mer.dict");
      else same(expand(R, lens, r0, r1, ~0ULL), want, ~0ULL, "k1mer.dict");
    }
}

int main() {
  const std::vector<uint8_t> zeros;
  // fixed-length sets: collect and all six rows of the table, a fixed set beside a ragged one of as many reads
  for (uint32_t L : {1u, 15u, 16u, 17u, 31u, 32u, 33u, 63u, 64u, 65u, 100u, 250u})
    for (bool with_n : {false, true}) {
      const HostSet a = fixed_set(57, L, with_n), b = fixed_set(57, L == 100 ? 80 : L, false), rg = ragged_set(true);
      CHECK(rg.reads.size() == 57);
      std::vector<uint32_t> every(57);
      for (uint32_t i = 0; i < 57; i++) every[i] = i;
      check_collect(a, a, every, zeros, "collect, a fixed set");
      for (int ss = 0; ss < 2; ss++)
        for (int mate = 0; mate < 3; mate++) {
          const std::vector<uint32_t> r = routes(90, ss ? 57 : 114);
          check_fasta(a, b, ss, mate, r, 7, "fasta, fixed sets");
          if (L == 33 || L == 100) { check_fasta(a, rg, ss, mate, r, 95, "fasta, a fixed set beside a ragged one"); check_fasta(rg, a, ss, mate, r, 995, "fasta, ragged beside fixed"); }
        }
    }
  // ragged sets, empty reads among them
  for (bool with_n : {false, true}) {
    const HostSet rg = ragged_set(with_n), fx = fixed_set(40, 80, !with_n);
    const uint32_t n = (uint32_t)rg.reads.size();
    std::vector<uint32_t> every(n), empties, rep(300);
    for (uint32_t i = 0; i < n; i++) { every[i] = i; if (rg.reads[i].empty()) empties.push_back(i); }
    for (uint32_t& d : rep) d = rnd(n);
    check_collect(rg, rg, every, zeros, "collect, every read of a ragged set");
    check_collect(rg, rg, rep, zeros, "collect, a selection with repeats");
    check_collect(rg, rg, empties, zeros, "collect, empty reads only", 0);
    check_collect(rg, rg, {n - 1}, zeros, "collect, the last read (empty)", 0);
    check_collect(rg, rg, {0, 1}, zeros, "collect, an empty read in front");
    for (int ss = 0; ss < 2; ss++)
      for (int mate = 0; mate < 3; mate++) {
        check_fasta(rg, rg, ss, mate, routes(120, ss ? n : 2 * n), 0, "fasta, ragged sets");
        check_fasta(rg, rg, ss, mate, empties, 3, "fasta, empty reads only");
      }
    // two sets of different geometry in one collect, repeats; outputs of exactly 4,096 and 4,097 codes
    std::vector<uint32_t> sel(500);
    std::vector<uint8_t> flags(500);
    for (int i = 0; i < 500; i++) { flags[i] = (uint8_t)rnd(2); sel[i] = rnd(flags[i] ? 40 : n); }
    check_collect(rg, fx, sel, flags, "collect, two sets");
    std::vector<uint32_t> s51(51);
    for (uint32_t& d : s51) d = rnd(40);
    std::vector<uint8_t> f51(51, 1);
    s51.push_back(6); f51.push_back(0);                                           // 51 x 80 + 16 (read 6 of the ragged set: 64 bases, cut below)
    HostSet cut = rg;
    cut.reads[6] = cut.reads[6].substr(0, 16); cut = pack(cut.reads, 0);
    check_collect(cut, fx, s51, f51, "collect, 4,096 codes", 4096);
    s51.push_back(8); f51.push_back(0);                                           // + read 8: one base
    check_collect(cut, fx, s51, f51, "collect, 4,097 codes", 4097);
  }
  // names of 1 to 20 digits, across every power of ten
  {
    const HostSet a = fixed_set(9, 17, true);
    uint64_t p10 = 1;
    for (int d = 1; d <= 20; d++) {
      const uint64_t e0 = d == 1 ? 0 : p10 - 3;
      check_fasta(a, a, 0, d % 3, routes(8, 18), e0, "fasta, names");
      if (d < 20) p10 *= 10;
    }
    check_fasta(a, a, 1, 2, routes(8, 9), ~0ULL - 8, "fasta, the last names");
  }
  for (uint32_t k1 : {21u, 26u, 32u}) check_dict(k1);
  if (failures) { fprintf(stderr, "expand_host_check: %d check(s) failed\n", failures); return 1; }
  printf("expand_host_check: OK\n");
  return 0;
}
