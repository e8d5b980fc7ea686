// What the extension and the component labelling share about a k1-mer table: the weights and flags of its k1-mers
// (ext_prepare_kernel) and the one-line dictionary their neighbour look-ups go through (k1dict.hip builds it).
#pragma once
#include "common.h"

__device__ __forceinline__ uint64_t oriented_string(const uint64_t* __restrict__ tkeys, uint32_t o, int k) {
  uint64_t key = tkeys[o >> 1];
  return (o & 1) ? shn_revcomp(key, k) : key;
}

// ---- the dictionary of the adjacency build: one 128-byte line per bucket -- ten keys (80 bytes), their ten id words (40 bytes),
// the number of keys that hashed here (4 bytes) -- so that a look-up, hit or miss, is ONE fetch.  HBM serves 128 bytes per request
// whatever is asked for (profiles/r03_fetch_calibration.txt), and the build makes 5.8 G look-ups at configs[2] of which 70 % miss:
// through the count table (bucket offsets -> bisection of a ~90-key bucket) a look-up was ~5 fetches, with a Bloom filter and a
// separator record per bucket in front (round 2) 1 for most misses and 3 for a hit -- 1.5 TB per launch, the kernel sat at the
// HBM limit.  Five keys per line on average: a bucket overflows with probability 1.4 %; what does not fit is found through the
// count table (the line's count says that there is more).  id word = table index | palindrome << 31; low-complexity k1-mers are
// not entered (load_kmers drops them, extension_correction.py:202-221).  An empty slot holds key 0 = AAA...A, which is
// low-complexity and therefore never a valid answer.
#define FD_SLOTS 10
#define FD_PER_LINE 4         // keys per line on average: a line overflows with probability 0.3 % (5: 1.4 %)
#define FD_HOPS 4             // what does not fit its line goes into the next ones
#define FD_PAL 0x80000000u
// (the hash of the count table's buckets, so that the build -- which goes through the table in bucket order -- fills the lines
// front to back: its atomics stay in the L2 and the lines stream out once; with a hash of its own the build was 724 M random
// read-modify-writes, 70 ms)
// (tables of layout 1 -- buckets of minimizers: a bucket's keys spread over the bucket's own stretch of lines, so the build still
// streams, and since a k1-mer's eight neighbours mostly share its minimizer, their look-ups mostly fall into the stretch the block
// is working through -- lines the L2 already holds)
__device__ __forceinline__ uint64_t fd_bucket(const TabIdx& T, uint64_t key, uint64_t n_lines) {
  const uint64_t h = shn_mix64(key);
  if (!T.layout) return __umul64hi(h, n_lines);
  // (buckets of minimizers differ in size by orders of magnitude: a bucket's lines are its share of the table -- one line per
  // FD_PER_LINE keys, from where its keys begin -- and the key picks one of them)
  const uint32_t b = shn_tab_bucket(T, key);
  const uint64_t lo = T.boff[b], hi = T.boff[b + 1];
  return lo / FD_PER_LINE + b + __umul64hi(h, (hi - lo) / FD_PER_LINE + 1);
}
// the same with the key's bucket known (layout 1)
__device__ __forceinline__ uint64_t fd_line_in_bucket(const TabIdx& T, uint32_t b, uint64_t key) {
  const uint64_t lo = T.boff[b], hi = T.boff[b + 1];
  return lo / FD_PER_LINE + b + __umul64hi(shn_mix64(key), (hi - lo) / FD_PER_LINE + 1);
}
// One look-up by the eight lanes g0 .. g0+7 of a wavefront (p = lane - g0; all eight pass the same key): lane p holds bytes
// 16 p .. 16 p + 15 of the line -- one coalesced 128-byte request.  Returns the id word or 0xFFFFFFFF, the same in all eight lanes.
__device__ __forceinline__ uint64_t shfl_u64(uint64_t x, int src) {
  return ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(x >> 32), src, 64) << 32) | (uint64_t)(uint32_t)__shfl((int)(uint32_t)x, src, 64);
}
__device__ __forceinline__ uint32_t fd_match(ulonglong2 v, const unsigned long long* __restrict__ lines, uint64_t line, uint64_t key, int p, int g0,
                                             const TabIdx& T, const uint8_t* __restrict__ flags) {
  for (int hop = 0;; hop++) {
    const bool ok = p < 5 && key != 0;
    const unsigned long long m0 = (__ballot(ok && v.x == key) >> g0) & 0xFFULL, m1 = (__ballot(ok && v.y == key) >> g0) & 0xFFULL;
    if (m0 | m1) {
      const int slot = m0 ? 2 * (__ffsll((long long)m0) - 1) : 2 * (__ffsll((long long)m1) - 1) + 1;
      // id words: bytes 80 .. 119 = words 20 .. 29: lane 5 + slot / 4, its word slot % 4
      const uint32_t w = (slot & 2) ? ((slot & 1) ? (uint32_t)(v.y >> 32) : (uint32_t)v.y) : ((slot & 1) ? (uint32_t)(v.x >> 32) : (uint32_t)v.x);
      return (uint32_t)__shfl((int)w, g0 + 5 + (slot >> 2), 64);
    }
    const uint32_t cnt = (uint32_t)__shfl((int)(uint32_t)(v.y >> 0), g0 + 7, 64) ;   // word 30 = low half of lane 7's second word
    if (cnt <= FD_SLOTS || key == 0) return 0xFFFFFFFFu;
    if (hop == FD_HOPS - 1) break;
    line++;                                                          // (the line overflowed, 0.3 % of them do: the next one -- one more fetch of the eight lanes)
    v = ((const ulonglong2*)(lines + line * 16))[p];
  }
  const int64_t j = shn_tab_find(T, key);                           // (FD_HOPS full lines in a row)
  if (j < 0) return 0xFFFFFFFFu;
  const uint8_t fj = flags[j];
  return (fj & 2) ? 0xFFFFFFFFu : ((uint32_t)j | ((fj & 1) ? FD_PAL : 0u));
}

// weight (count, x2 for palindromes) and flags (bit0 palindrome, bit1 low complexity) of every k1-mer of a table that has some, on stream s
void ext_prepare_launch(hipStream_t s, const shn_table* t, uint32_t* d_weight, uint8_t* d_flags);
// the dictionary of the records / labelling kernels (see fd_build_kernel).  room: memory of at least fine_dict_lines(n) * 128 bytes
// to build it in (shn_extend: the claims and their snapshot are not in use yet -- the dictionary is 23 GB at 907 M k1-mers, and a
// block of its own on top of the records put the steady state of the K = 31 slice over the device: every step then paid for
// hipMalloc again); NULL: a block of its own, which the caller frees after the stream has drained
int build_fine_dict(shn_ctx* ctx, const shn_table* t, const uint8_t* d_flags, unsigned long long** lines_out, uint64_t* n_lines_out,
                    void* room = nullptr);
uint64_t fine_dict_lines(const shn_table* t);
