// Contig extension / k1-mer error correction on gfx950 (rows a3-a4): replaces the sequential
// heaviest-first greedy walk of extension_correction.py:334-354 (load_kmers :202-221, extend
// :223-245, argmax :159-166).
//
// The reference processes seeds one by one in (weight desc, k1-mer asc) order with a global
// `traversed` set.  Here every seed is a walk with priority = its rank in that order and all
// walks run in parallel as a fixpoint iteration:  walk r treats a k1-mer as traversed iff it was
// claimed (previous iteration) by a walk of smaller rank, or is on its own trail.  The sequential
// result is the unique fixpoint (walk 0 is right after one iteration, walk r once every walk < r
// it touches is right), so iterating until no walk changes reproduces the reference exactly.
//
// The iteration is change-driven (a worklist): claims persist in one array; after a round every k1-mer whose
// owner changed marks as dirty the walks whose view it changes -- the walks standing next to it (owners of its 8
// neighbours) and the walk seeded on it, and only those for which it BECAME available (old owner < walk < new
// owner).  Only dirty walks run in the next round, after their old claims have been released; the round count
// stays the dependency depth of the data, but a round costs the affected walks, not all of them.  A consistent
// state (no dirty walk) is the unique fixpoint = the sequential result.
// Memos: after every round the path of each walk that ran alive is rebuilt from the claims into a memo slot, and
// every k1-mer remembers the (walk, step) it was written under (hint).  A wavefront re-checks 64 memo steps per
// memory round trip -- of its own memo, or of the memo of whatever walk last owned the k1-mer it reached, in either
// direction -- and walks sequentially only in between.  Memos are hints: every entry is validated against the
// hint of its k1-mer, and a changed decision is re-made against the live claims.
// Short walks run one per thread; one that turns out long hands over to a wavefront in the same round.
// shn_extend_sharded: walks never leave their connected component of the k1-mer graph, so the components (GPU
// union-find, components.hip) can be dealt to several ranks.  What reads a finished extension is in ext_results.hip.
//
// Oriented k1-mers: the count table stores canonical keys; oriented id o = 2*i + s is the string
// key_i (s=0) or its reverse complement (s=1; unused for palindromes).  Both strands are walked,
// as in the reference's strand-doubled input.
#include "ext_state.h"
#include "k1dict.h"
#include <cstring>
#include <vector>
#include <time.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>

// the thread walkers run in workgroups of ONE wavefront: a workgroup keeps its place on the CU (8 per CU at 256 threads) until its
// last wavefront has ended, and a walk kernel's wavefronts end at very different times (each runs as long as its longest walk) --
// measured with 256-thread workgroups: 1,750 of 8,192 wavefront slots in use on average over a bulk round
#define WBLK 64
#define NOHINT_WORD 0xFFFFFFFFu   // = NOHINT (defined with the memo machinery below)
#define LONG_WALK 8           // dirty walks at least this long (last run or memo) get a wavefront
#define MEMO_MIN 1            // walks at least this long get a memo slot
#define PROMOTE_STEPS 16      // a thread walker that gets this far hands over to a wavefront

// The driver and its kernels share one block of 64-bit counters (workspace slot 13, zeroed when a call starts).  A kernel is
// handed the block, or the word of it where its own counts begin.
enum {
  CNT_STEPS = 1,              // steps of the thread walkers, all rounds
  CNT_PLAN = 2,               // ext_plan_kernel: the round's four counts (PLAN_*)
  CNT_CHANGED = 6,            // ext_mark_kernel: k1-mers whose owner changed in the round
  CNT_SPARE = 7,              // (cleared with CNT_CHANGED)
  CNT_POOL = 10,              // memo pool: the next free word
  CNT_HANDED = 13,            // walks the thread walker handed over in the round (the length of promo_list)
  CNT_TRIPS = 15,             // wavefront trips of the thread walker (the SHN_DEBUG log reads it)
  CNT_FRESH_STEPS = 16,       // ... of CNT_STEPS, the ones made in the first round of a block
  CNT_ROBSAT = 21,            // SHN_EXT_XTIME: the round's claim holders that were robbed while they sat out (ROBSAT_*)
  CNT_HELD = 24,              // claims the round's dirty walks hold, by their records
  CNT_LOG = 26,               // claim logs: the next free chunk
  CNT_DBG = 32,               // WalkArgs::dbg (DBG_*)
  CNT_AUDIT = 48,             // what an audit found (AUDIT_*)
  CNT_WAVE_STEPS = 64,        // steps of the wavefront walker, all rounds, spread over 64 words
  CNT_WORDS = 256
};
enum { PLAN_LONG = 0, PLAN_NOMEMO = 1, PLAN_SHORT = 2, PLAN_DIRTY = 3 };   // long walks, claim holders without a current memo or log, short walks, dirty walks
enum { ROBSAT_WALKS = 0, ROBSAT_LONGEST = 1, ROBSAT_STEPS = 2 };
enum {
  DBG_OWN = 0, DBG_FOREIGN = 1,             // wave steps confirmed from an own / a foreign memo
  DBG_WHY = 0,                              // + i: how often memo_follow ended with WHY(i), i = 2 .. 7
  DBG_BROKE_FIRST = 8, DBG_BROKE_LATER = 9, // memo chunks that broke at their first step / later
  DBG_MOST_SEQ = 10, DBG_LONGEST_WAVE = 11, // maxima of the round: a wavefront walk's sequential steps (with its WHY counts), its steps
  DBG_LONGEST_THREAD = 12                   // the longest thread walk of the launch: steps << 32 | ticks of 10 ns
};
enum { AUDIT_NODES = 0, AUDIT_WALKS = 1,    // the fixpoint audit: k1-mers / walks that disagree with the greedy rule
       AUDIT_BAD = 0, AUDIT_LOWEST = 1 };   // SHN_EXT_AUDIT: walks that are not at their fixpoint, the lowest such rank

__global__ void ext_digest_kernel(const uint32_t* __restrict__ w, uint64_t n_words, uint64_t salt, unsigned long long* __restrict__ out) {
  unsigned long long acc = 0;
  uint32_t cur = 0xFFFFFFFFu;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ch = (uint32_t)((i * EXT_DIG_CHUNKS) / n_words);
    if (ch != cur) { if (cur != 0xFFFFFFFFu && acc) atomicAdd(&out[cur], acc); cur = ch; acc = 0; }
    acc += shn_mix64((i * 0x9E3779B97F4A7C15ULL) ^ ((uint64_t)w[i] << 1) ^ salt);
  }
  if (cur != 0xFFFFFFFFu && acc) atomicAdd(&out[cur], acc);
}

// The records of both orientations of every canonical k1-mer from 8 look-ups instead of 16: the right candidates of the reverse-
// complement orientation are the reverse complements of the forward orientation's left candidates (rc(s)[1:] + b = rc(comp(b) +
// s[:-1])) and vice versa -- the same table entry j, the other orientation (the same one if entry j is its own reverse
// complement).  Eight lanes per canonical k1-mer: they make its eight look-ups together, one after the other (every look-up one
// 128-byte request of the eight lanes, all eight requests in flight before the first is looked at), and then write the two
// records -- 128 contiguous bytes -- 16 bytes each.
struct __attribute__((aligned(16))) Quad { uint32_t a, b, c, d; };
__global__ void ext_records_kernel(const TabIdx T, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ weight, uint64_t n, int k, int canonical,
                                   Rec* __restrict__ rec, const unsigned long long* __restrict__ lines, uint64_t n_lines) {
  const uint64_t* __restrict__ tkeys = T.keys;
  const uint64_t total = n * 8;
  const uint64_t rounded = (total + 63) & ~63ULL;                       // whole wavefronts take part in the ballots and shuffles
  const uint64_t mask = (k == 32) ? ~0ULL : ((1ULL << (2 * k)) - 1);
  const int lane = threadIdx.x & 63, g0 = lane & ~7, p = lane & 7;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool in = gid < total;
  uint64_t i = in ? gid >> 3 : 0;
  uint8_t f = (gid < rounded && in) ? flags[i] : (uint8_t)2;
  uint64_t str = gid < rounded ? tkeys[i] : 0ULL;
  uint32_t wt = (gid < rounded && in && (p == 2 || p == 6)) ? weight[i] : 0u;
  for (; gid < rounded;) {
    const bool dead0 = (f & 2) != 0;                                    // forward orientation
    const bool dead1 = dead0 || (f & 1) || !canonical;                  // reverse-complement orientation (absent for palindromes)
    // look-up q: q = 0..3 append base q, q = 4..7 prepend base q - 4; lane q prepares it (key, strand, line), the group shares
    uint64_t mykey; uint32_t mystrand = 0;
    {
      const uint64_t b = (uint64_t)(p & 3);
      mykey = p < 4 ? (((str << 2) | b) & mask) : ((str >> 2) | (b << (2 * (k - 1))));
      if (canonical) { const uint64_t rc = shn_revcomp(mykey, k); if (rc < mykey) { mykey = rc; mystrand = 1; } }
      if (dead0) mykey = 0;                                             // (no look-up is needed: key 0 is never found)
    }
    uint64_t myline;
    if (T.layout) {
      // The minimizers of the eight neighbours from the k1-mer's own m-mers: the four successors share its m-mers 1 .. w - 1, the
      // four predecessors its m-mers 0 .. w - 2, and each adds one m-mer of its own (its last / first).  The eight lanes split the
      // k1-mer's w m-mers between them (a minimizer is the same on both strands, so the stored orientation serves); a look-up made
      // from scratch costs w order values per neighbour, and the kernel was bound by exactly that arithmetic.
      const int m = T.m, w = k - m + 1;
      const uint32_t mmask = m == 16 ? 0xFFFFFFFFu : ((1u << (2 * m)) - 1u);
      uint32_t smin = 0xFFFFFFFFu, pmin = 0xFFFFFFFFu;                  // over m-mers 1 .. w - 1 / 0 .. w - 2
      for (int pos = p; pos < w; pos += 8) {
        const uint32_t f = (uint32_t)(str >> (2 * (k - m - pos))) & mmask;
        uint32_t c = f;
        if (canonical) { const uint32_t r = shn_revcomp32(f, m); c = r < f ? r : f; }
        const uint32_t o = shn_sk_order(c);
        if (pos >= 1) smin = o < smin ? o : smin;
        if (pos <= w - 2) pmin = o < pmin ? o : pmin;
      }
#pragma unroll
      for (int d = 1; d < 8; d <<= 1) {
        const uint32_t a = (uint32_t)__shfl_xor((int)smin, d, 64), b2 = (uint32_t)__shfl_xor((int)pmin, d, 64);
        smin = a < smin ? a : smin; pmin = b2 < pmin ? b2 : pmin;
      }
      const uint32_t nb = (uint32_t)(p & 3);
      const uint32_t f = p < 4 ? ((((uint32_t)str & (mmask >> 2)) << 2) | nb)                          // the successor's last m-mer
                               : ((nb << (2 * (m - 1))) | ((uint32_t)(str >> (2 * (k - m + 1))) & (mmask >> 2)));   // the predecessor's first
      uint32_t c = f;
      if (canonical) { const uint32_t r = shn_revcomp32(f, m); c = r < f ? r : f; }
      uint32_t o = shn_sk_order(c);
      const uint32_t shared = p < 4 ? smin : pmin;
      o = shared < o ? shared : o;
      myline = fd_line_in_bucket(T, shn_sk_bucket(o, T.bits), mykey);
    } else myline = fd_bucket(T, mykey, n_lines);
    const uint32_t strands = (uint32_t)((__ballot(mystrand != 0) >> g0) & 0xFFULL);
    uint64_t key[8];
    ulonglong2 v[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
      key[q] = shfl_u64(mykey, g0 + q);
      v[q] = ((const ulonglong2*)(lines + shfl_u64(myline, g0 + q) * 16))[p];
    }
    uint32_t r8[8], d8[8];                                              // the candidate (oriented id), its other orientation
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const uint32_t w = fd_match(v[q], lines, shfl_u64(myline, g0 + q), key[q], p, g0, T, flags);
      if (w == 0xFFFFFFFFu) { r8[q] = d8[q] = 0xFFFFFFFFu; continue; }
      const uint32_t j = w & ~FD_PAL;
      const uint32_t st = (strands >> q) & 1u;
      r8[q] = 2 * j + st;
      d8[q] = (w & FD_PAL) ? r8[q] : 2 * j + (1 - st);
    }
    if (in) {
      // lane p writes bytes 16 p .. of the pair of records (forward, reverse complement)
      Quad out;
      const Quad none = Quad{~0u, ~0u, ~0u, ~0u};
      switch (p) {
        case 0: out = Quad{r8[0], r8[1], r8[2], r8[3]}; break;           // forward: right row = the append candidates
        case 1: out = Quad{r8[4], r8[5], r8[6], r8[7]}; break;           //          left row = the prepend candidates
        case 4: out = dead1 ? none : Quad{d8[7], d8[6], d8[5], d8[4]}; break;   // reverse complement: right row = the prepend candidates' other orientations, mirrored (base b <-> 3 - b)
        case 5: out = dead1 ? none : Quad{d8[3], d8[2], d8[1], d8[0]}; break;   //                     left row = the append candidates' ...
        case 2: case 6: out = Quad{wt, NOHINT_WORD, 0xFFFFFFFFu, 0u}; break;
        default: out = Quad{0u, 0u, 0u, 0u}; break;
      }
      ((Quad*)(rec + 2 * i))[p] = out;
    }
    gid += stride; in = gid < total; i = in ? gid >> 3 : 0;
    if (gid < rounded) { str = tkeys[i]; f = in ? flags[i] : (uint8_t)2; wt = (in && (p == 2 || p == 6)) ? weight[i] : 0u; }
  }
}

// The seeds (oriented k1-mers of weight >= min_weight; low-complexity ones and the second orientation of a palindrome left out) in
// two passes without a shared cursor: the count pass leaves one count per block, a scan turns them into bases, the write pass
// recomputes and writes -- in table order, whatever the scheduling.  (One atomic per block on ONE address was 17 ms per pass at
// 1.4 M blocks.)  One thread per canonical k1-mer, both orientations.
__global__ __launch_bounds__(1024) void ext_seed_kernel(const uint64_t* __restrict__ tkeys, const uint32_t* __restrict__ weight,
                                const uint8_t* __restrict__ flags, uint64_t n, int k, int canonical, uint32_t min_weight,
                                uint32_t* __restrict__ block_count, const uint64_t* __restrict__ block_base,
                                uint64_t* __restrict__ skeys, uint32_t* __restrict__ svals) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool s0 = false, s1 = false;
  if (i < n) {
    const uint8_t f = flags[i];
    s0 = !(f & 2) && weight[i] >= min_weight;
    s1 = s0 && !(f & 1) && canonical;
  }
  __shared__ uint32_t wcnt[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned long long m0 = __ballot(s0), m1 = __ballot(s1), below = (1ULL << lane) - 1ULL;
  if (lane == 0) wcnt[wid] = (uint32_t)(__popcll(m0) + __popcll(m1));
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); w++) { const uint32_t c = wcnt[w]; if (w < wid) before += c; total += c; }
  if (!skeys) { if (threadIdx.x == 0) block_count[blockIdx.x] = total; return; }
  if (!s0) return;
  uint64_t p = block_base[blockIdx.x] + before + (uint32_t)(__popcll(m0 & below) + __popcll(m1 & below));
  const uint64_t key = tkeys[i];
  skeys[p] = key; svals[p] = (uint32_t)(2 * i);
  if (s1) { skeys[p + 1] = shn_revcomp(key, k); svals[p + 1] = (uint32_t)(2 * i + 1); }
}

__global__ void ext_weightkey_kernel(const uint32_t* __restrict__ svals, const uint32_t* __restrict__ weight, uint64_t ns,
                                     uint64_t* __restrict__ wkeys) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  wkeys[i] = (uint64_t)(0xFFFFFFFFu - weight[svals[i] >> 1]);   // ascending sort => weight descending
}

// entry b of a row, b known only at run time: picked with compares (an indexed access makes the compiler keep the row in
// scratch memory)
__device__ __forceinline__ int32_t adj_get(const Adj4& a, int b) { return b == 0 ? a.v[0] : b == 1 ? a.v[1] : b == 2 ? a.v[2] : a.v[3]; }
#define CHUNK_SHIFT 4          // 16 oriented k1-mers = one 128-byte line of claims per flag

struct WalkArgs {
  const uint32_t* order; RowView adjR; RowView adjL; WordView weight;   // weight: by ORIENTED id (views of the record array)
  u64* claim;            // live claims: clean walks' + this round's (dirty walks released theirs before the round)
  const u64* claim_old;  // snapshot taken before the round
  uint32_t* nr_out; uint32_t* nl_out; uint64_t* totw_out;
  // memo: the path of the walk's last live run, rebuilt from the claims after every round it ran alive
  // (ext_memo_plan_kernel + the scatter in ext_mark_kernel).  Hints only -- every use is validated.
  const uint32_t* pool; const uint64_t* moff; const uint32_t* mR; const uint32_t* mL; const uint8_t* mvalid;
  WordView hint;         // per k1-mer: where it was last written into a memo (pool index << 2 | kind), NOHINT if never
  unsigned long long* steps_counter;
  unsigned long long* fresh_steps_counter;   // ... of them in the first round of a rank block (ext_walk_kernel<true>: its own line in bench.py's kernel table)
  unsigned long long* wave_steps_counter;
  unsigned long long* dbg;     // debug counters (DBG_*), NULL: off
  // a thread walker that turns out long hands its walk over to a wavefront (same round): where it stands
  uint32_t* promo_list; unsigned long long* promo_count; uint32_t* res_cur; uint32_t* res_info;   // info = dir << 31 | steps so far
  uint32_t promote_steps;
  uint8_t* chunk;        // per 2^CHUNK_SHIFT oriented k1-mers: "a claim in here was written this round" (the mark pass visits only those)
  uint8_t* robbed;       // per walk: a claim of its record is not (or no longer) its own -- see note_claim
  // claim logs (round 6): in a bulk round -- no memos are made there -- the thread walker writes the k1-mers it claims into a chain of
  // 8-word chunks of its own ([0] = the chunk before, [1..7] = k1-mers; the seed is not logged: it is order[r]); a walk that re-runs
  // later gives back what it still holds through its log (ext_release_memo_kernel) instead of the begin pass streaming every claim
  uint32_t* logpool; uint32_t* log_head; uint8_t* log_cnt; unsigned long long* log_cursor; uint64_t log_cap;   // pool of log_cap chunks; per walk: last chunk (NONE32: no log, LOG_LOST: the pool ran out) and its entries
};
#define LOG_WORDS 8u
#define LOG_PER (LOG_WORDS - 1u)
#define LOG_SLAB 64u           // chunks a wavefront reserves with one global atomic
#define LOG_LOST 0xFEFEFEFEu        // (the byte pattern of hipMemset(0xFE): "no log" is what the arrays start as)

// Claim `node` as step `pos` of walk r: atomic min on rank:pos.  Returns what stood there before; the caller hands it to note_claim
// -- one step later in the thread walkers, where the answer has long arrived behind the loads of the next step (memory operations
// of a wavefront return in issue order), so the atomic's round trip is on nobody's critical path.
__device__ __forceinline__ u64 claim_node(const WalkArgs& A, uint32_t node, uint32_t r, uint32_t pos) {
  const u64 old = __hip_atomic_fetch_min(&A.claim[node], CLAIM(r, pos), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (A.chunk) A.chunk[node >> CHUNK_SHIFT] = 1;
  return old;
}
// What a claim found: a lower rank (it got there between this walk's look and its claim: the walk's record holds a k1-mer it does
// not own) or a higher one (robbed: THAT walk's record is stale, if it ran this round -- one that sat out is found by the mark
// pass through the snapshot).  Either way the walk has to run again: ext_verify_kernel reads the flags.  (Until round 3 the mark
// pass counted the k1-mers every walk owned, one random atomic per claimed k1-mer, and the verify kernel compared the count with
// the record.)
__device__ __forceinline__ void note_claim(const WalkArgs& A, u64 old, uint32_t r) {
  const uint32_t x = RANK(old);
  if (x != UNCLAIMED && x != r) A.robbed[x < r ? r : x] = 1;
}

// One greedy decision (extension_correction.py:223-237): among the candidates that exist and are not
// traversed pick the heaviest, ties in BASES order A,G,C,T (codes 0,2,1,3; strict >).  Traversed = claimed
// live by a rank <= r (lower ranks of this round, or this walk's own trail), or claimed in the pre-round
// snapshot by a lower rank.
__device__ __forceinline__ int decide(const Adj4& cand, uint32_t r, const u64* claim, const u64* __restrict__ claim_old,
                                      const WordView weight, uint32_t dummy, uint32_t& bw) {
  u64 cl[4], co[4];
  uint32_t w[4];
#pragma unroll
  for (int b = 0; b < 4; b++) {
    uint32_t idx = cand.v[b] < 0 ? dummy : (uint32_t)cand.v[b];
    cl[b] = __hip_atomic_load(&claim[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    co[b] = claim_old[idx];
    w[b] = weight[idx];
  }
  int best = -1;
  bw = 0;
#define CONSIDER(b) if (cand.v[b] >= 0 && RANK(cl[b]) > r && RANK(co[b]) >= r && (best < 0 || w[b] > bw)) { best = b; bw = w[b]; }
  CONSIDER(0) CONSIDER(2) CONSIDER(1) CONSIDER(3)
#undef CONSIDER
  return best;
}

// the greedy choice of walk r standing at step p, from the claims alone (for walk r a k1-mer is traversed iff a lower rank
// owns it or r owns it at a step <= p); used by the precise marks of ext_mark_kernel and by the fixpoint audit
__device__ __forceinline__ int audit_decide(const Adj4& cd, uint32_t r, uint32_t p, const u64* __restrict__ claim,
                                            const WordView weight) {
  int best = -1;
  uint32_t bw = 0;
#pragma unroll
  for (int bi = 0; bi < 4; bi++) {
    const int b = bi == 0 ? 0 : bi == 1 ? 2 : bi == 2 ? 1 : 3;          // BASES order A,G,C,T
    if (cd.v[b] < 0) continue;
    const u64 c = claim[cd.v[b]];
    const bool avail = RANK(c) > r || (RANK(c) == r && POS(c) > p);
    const uint32_t w = weight[(uint32_t)cd.v[b]];
    if (avail && (best < 0 || w > bw)) { best = b; bw = w; }
  }
  return best;
}


// ---- short walks: one thread per walk, one memory round trip per step (candidate rows prefetched).
// FRESH: the first round of a block that has just opened -- none of its walks has run before, so the snapshot holds nothing but
// the claims of final walks, which the live claims hold too: the snapshot is not read (a quarter of a step's memory accesses,
// in the rounds that make most of the steps).
template <bool FRESH>
__global__ __launch_bounds__(WBLK) void ext_walk_kernel(WalkArgs A, uint64_t n_walks, const uint32_t* __restrict__ list,
                                                        const u64* __restrict__ snap) {
  __shared__ unsigned long long blk_steps;
  __shared__ uint32_t blk_promo[WBLK], n_promo, promo_base;      // walks handed over: one global atomic per block
  __shared__ uint32_t slab_next, slab_end;                        // claim logs: the wavefront's reserve of chunks
  if (threadIdx.x == 0) { blk_steps = 0; n_promo = 0; slab_next = 0; slab_end = 0; }
  __syncthreads();
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t mysteps = 0;
  // a chunk for every lane that asks in this trip (the lanes of the wavefront that are in the loop right now): one LDS update by
  // the first of them, one global atomic per LOG_SLAB chunks
  auto log_chunk = [&](bool need) -> uint32_t {
    const unsigned long long m = __ballot(need);
    uint32_t got = NONE32;
    if (m) {
      const int leader = __ffsll((long long)m) - 1;
      const uint32_t cnt = (uint32_t)__popcll(m);
      uint32_t base = 0;
      if ((int)threadIdx.x == leader) {
        uint32_t nx = *(volatile uint32_t*)&slab_next, en = *(volatile uint32_t*)&slab_end;
        if (nx + cnt > en) {
          const unsigned long long g = atomicAdd(A.log_cursor, (unsigned long long)LOG_SLAB);
          if (g + LOG_SLAB <= A.log_cap) { nx = (uint32_t)g; en = nx + LOG_SLAB; } else { nx = NONE32 - 2 * LOG_SLAB; en = nx; }     // (the pool ran out: nobody gets a chunk)
        }
        base = nx + cnt <= en ? nx : NONE32;
        *(volatile uint32_t*)&slab_next = nx + (base == NONE32 ? 0u : cnt); *(volatile uint32_t*)&slab_end = en;
      }
      base = (uint32_t)__shfl((int)base, leader, 64);
      if (need && base != NONE32) got = base + (uint32_t)__popcll(m & ((1ULL << threadIdx.x) - 1ULL));
    }
    return got;
  };
  const bool logging = A.logpool != nullptr;
  uint32_t lg_chunk = NONE32, lg_k = LOG_PER;                     // the walk's last chunk and the entries it holds (LOG_PER: full, or none yet)
  bool lg_lost = false;
  if (t < n_walks) {
    const uint32_t r = list[t];
    const uint32_t o = A.order[r];
    const unsigned long long t_begin = A.dbg ? __builtin_amdgcn_s_memrealtime() : 0ULL;      // (100 MHz)
    uint32_t nr = 0, nl = 0;
    uint64_t tot = 0;
    bool promoted = false;
    // snap: the pre-round snapshot; A.claim: live claims of this round
    bool isvoid = (!FRESH && RANK(snap[o]) < r) || RANK(__hip_atomic_load(&A.claim[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < r;
    if (!isvoid) {
      u64 seen = claim_node(A, o, r, 0);             // what the last claim found; looked at one step later
      uint32_t pos = 0, pend = NONE32;
      tot = A.weight[o];
      bool gave_up = false;
      // (unrolled: a copy of the step loop per direction, each with its rows' base in registers of its own.  Left to itself the
      // compiler keeps one copy and picks the base per step: 72 / 80 VGPRs and 10 spilled SGPRs against 70 / 78 and none)
#pragma unroll
      for (int dir = 0; dir < 2; dir++) {
        const RowView adj = dir == 0 ? A.adjR : A.adjL;
        uint32_t steps = 0;
        Adj4 cand = adj[o];
        while (true) {
          u64 cl[4], cf[4];
          uint32_t w[4];
          Adj4 nxt[4];
#pragma unroll
          for (int b = 0; b < 4; b++) {
            uint32_t idx = cand.v[b] < 0 ? o : (uint32_t)cand.v[b];
            cl[b] = __hip_atomic_load(&A.claim[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            cf[b] = FRESH ? UNCLAIMED64 : snap[idx];
            w[b] = A.weight[idx];
            nxt[b] = adj[idx];
          }
          // the walk's own seed (one line, in the L2 from the second step on): once a lower rank has taken it this walk is void in
          // the end -- 98.6 % of the walks of BASELINE configs[2] are -- and whatever it goes on to claim is wasted; it stops, is
          // flagged like any robbed walk and looks again next round
          const u64 cseed = __hip_atomic_load(&A.claim[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          // the claim of the step just taken goes out BEHIND the loads of this step: vector memory operations of a wavefront
          // return in issue order (one counter for loads, stores and atomics), so a claim issued in front of the loads would put
          // the latency of a memory-side atomic on every step of the walk -- and a bulk round lasts as long as its longest walk
          u64 found = UNCLAIMED64;
          if (pend != NONE32) {
            found = claim_node(A, pend, r, pos);
            pend = NONE32;
          }
          int best = -1;
          uint32_t bw = 0;
#define CONSIDER(b) if (cand.v[b] >= 0 && RANK(cl[b]) > r && RANK(cf[b]) >= r && (best < 0 || w[b] > bw)) { best = b; bw = w[b]; }
          CONSIDER(0) CONSIDER(2) CONSIDER(1) CONSIDER(3)
#undef CONSIDER
          // (what the claim BEFORE this step's found: it was issued in front of this step's loads, which have just been used)
          note_claim(A, seen, r);
          seen = found;
          if (RANK(cseed) < r) { A.robbed[r] = 1; gave_up = true; break; }
          if (best < 0) break;
          // (selected with compares, not indexed: a run-time index puts the rows into scratch memory -- 96 bytes per lane of private
          // memory traffic on every step)
          uint32_t nbest = (uint32_t)(best == 0 ? cand.v[0] : best == 1 ? cand.v[1] : best == 2 ? cand.v[2] : cand.v[3]);
          pos++;
          pend = nbest;                            // claimed at the top of the next trip (or below, when the walk stops here)
          steps++;
          tot += bw;
          if (logging) {                           // the k1-mer goes into the walk's log (whoever gets this far claims it)
            const bool need = lg_k == LOG_PER && !lg_lost;
            const uint32_t nc = log_chunk(need);
            if (need) {
              if (nc == NONE32) lg_lost = true;
              else { A.logpool[(uint64_t)nc * LOG_WORDS] = lg_chunk; lg_chunk = nc; lg_k = 0; }
            }
            if (!lg_lost) { A.logpool[(uint64_t)lg_chunk * LOG_WORDS + 1 + lg_k] = nbest; lg_k++; }
          }
          if (pos >= A.promote_steps) {            // long after all: a wavefront takes over from here (memos, 64 steps a trip)
            note_claim(A, seen, r);
            seen = claim_node(A, nbest, r, pos);
            pend = NONE32;
            A.res_cur[r] = nbest;
            A.res_info[r] = ((uint32_t)dir << 31) | pos;
            blk_promo[atomicAdd(&n_promo, 1u)] = r;
            promoted = true;
            break;
          }
#pragma unroll
          for (int q = 0; q < 4; q++) cand.v[q] = best == 0 ? nxt[0].v[q] : best == 1 ? nxt[1].v[q] : best == 2 ? nxt[2].v[q] : nxt[3].v[q];   // (word by word: a select between structs goes through memory)
        }
        if (pend != NONE32) {                        // the last step of this direction
          note_claim(A, seen, r);
          seen = claim_node(A, pend, r, pos);
          pend = NONE32;
        }
        if (dir == 0) nr = steps; else nl = steps;
        if (promoted || gave_up) break;
      }
      note_claim(A, seen, r);
    }
    A.nr_out[r] = isvoid ? UNCLAIMED : nr;
    A.nl_out[r] = nl;
    A.totw_out[r] = tot;
    if (logging) { A.log_head[r] = lg_lost ? LOG_LOST : lg_chunk; A.log_cnt[r] = (uint8_t)(lg_chunk == NONE32 ? 0u : lg_k); }      // (a walk that took no step: NONE32 -- its seed is all it holds)
    mysteps = nr + nl;
    // debug: the longest walk of the launch and how long it took (steps << 32 | ticks of 10 ns): a bulk round cannot end before it
    if (A.dbg && mysteps >= 64) atomicMax(&A.dbg[DBG_LONGEST_THREAD], ((unsigned long long)mysteps << 32) | ((__builtin_amdgcn_s_memrealtime() - t_begin) & 0xFFFFFFFFULL));
  }
  if (mysteps) atomicAdd(&blk_steps, (unsigned long long)mysteps);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (blk_steps) { atomicAdd(A.steps_counter, blk_steps); if (FRESH) atomicAdd(A.fresh_steps_counter, blk_steps); }
    promo_base = n_promo ? (uint32_t)atomicAdd(A.promo_count, (unsigned long long)n_promo) : 0u;
  }
  __syncthreads();
  if (threadIdx.x < n_promo) A.promo_list[promo_base + threadIdx.x] = blk_promo[threadIdx.x];
}

// ---- long walks: one wavefront per dirty walk.  A memo (the path of some walk's last live run, own or foreign)
// is re-checked 64 steps per memory round trip; the walk is sequential only from the first changed decision
// until it meets a memo again -- its own, or the one of the walk whose territory it is taking over.
// Memo entries are hints: an entry counts only if the k1-mer's hint says it sits at exactly that position of
// that memo (so the validated entries of a chunk are pairwise distinct), and a changed decision is re-made
// sequentially against the live claims, never taken from the speculative lane.
__device__ __forceinline__ bool is_term_any(bool term, bool at_mark) { return term && at_mark; }
// Memo slots are never rewritten: a walk that runs again gets a new slot, so a hint always leads to an intact old path.
//   slot = [MARK][nR | HI][seed][R_1 .. R_nR][MARK][L_1 .. L_nL][MARK]       (HI = top bit; k1-mer ids are < 2^31)
// Every word with the top bit set ends a segment: marks, the header, and the NONE32 holes of steps that were robbed.
#define MEMO_MARK 0xFFFFFFFEu
#define MEMO_HI 0x80000000u
#define NOHINT 0xFFFFFFFFu
#define HINT_R 0u
#define HINT_L 1u
#define HINT_SEED 2u
struct MemoCursor { int64_t i; int32_t step; bool term; };
// i = pool index of the next expected step, step = +1 / -1 (a memo can be followed against the direction its walk
// took), term = the segment ends where that walk ended (then "stop" is the expected decision at its mark)

// `node` was just reached going in direction dir; its hint says where it sits in some memo: follow that memo
struct WhyStat { uint32_t c2 = 0, c4 = 0, c5 = 0, c7 = 0; };      // (named fields, not an array: an array whose address is passed on lives in scratch)
__device__ __forceinline__ bool memo_follow(const WalkArgs& A, uint32_t hh, uint32_t node, int dir, MemoCursor& mc, WhyStat* why = nullptr) {
#define WHY(i) do { if (A.dbg && threadIdx.x == 0) atomicAdd(&A.dbg[DBG_WHY + i], 1ULL); if (why) why->c##i++; } while (0)
  if (hh == NOHINT) { WHY(2); return false; }                     // never written into a memo
  const int64_t idx = (int64_t)(hh >> 2);
  const uint32_t kind = hh & 3u;
  if (A.pool[idx] != node) { WHY(4); return false; }              // (cannot happen while slots are not recycled)
  if (kind == HINT_SEED) {                                          // the walk's part of my direction, forwards
    const uint32_t nR = A.pool[idx - 1] & ~MEMO_HI;
    mc.i = dir == 0 ? idx + 1 : idx + 2 + (int64_t)nR; mc.step = 1; mc.term = true;
  } else if ((kind == HINT_R) == (dir == 0)) { mc.i = idx + 1; mc.step = 1; mc.term = true; }
  else { mc.i = idx - 1; mc.step = -1; mc.term = false; WHY(5); }    // back along that walk's path (its seed included)
  WHY(7);
#undef WHY
  return true;
}

// RESUME: the walks of the list were started by the thread kernel this round (promo_list); go on where they stand.
template <bool RESUME>
__global__ __launch_bounds__(64) void ext_walk_long_kernel(WalkArgs A, const uint32_t* __restrict__ long_list, uint64_t n_walks,
                                                           const unsigned long long* __restrict__ list_count) {
  const unsigned long long n_list = RESUME ? *list_count : (unsigned long long)gridDim.x;
  for (unsigned long long li = blockIdx.x; li < n_list; li += gridDim.x) {
  const uint32_t r = long_list[li];
  const int lane = threadIdx.x;
  const uint32_t o = A.order[r];
  uint32_t ns = 0, nr_new = 0;
  uint64_t tot;
  int dir0 = 0;
  uint32_t cur0 = o;
  u64 seen = UNCLAIMED64;                     // per lane: what its last claim found, looked at when it claims again (note_claim)
  if (RESUME) {
    const uint32_t info = A.res_info[r];
    dir0 = (int)(info >> 31);
    ns = info & 0x7FFFFFFFu;
    cur0 = A.res_cur[r];
    nr_new = dir0 ? A.nr_out[r] : 0;
    tot = A.totw_out[r];
  } else {
    const bool isvoid = RANK(A.claim_old[o]) < r || RANK(__hip_atomic_load(&A.claim[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < r;
    if (isvoid) {                                 // seed currently traversed; the memo stays for later
      if (lane == 0) { A.nr_out[r] = UNCLAIMED; A.nl_out[r] = 0; A.totw_out[r] = 0; }
      continue;
    }
    tot = A.weight[o];
    if (lane == 0) seen = claim_node(A, o, r, 0);
  }
  const uint32_t ns_start = ns;
  uint32_t nseq = 0;                          // sequential steps (debug statistics)
  WhyStat why;
  for (int dir = dir0; dir < 2; dir++) {
    const RowView adj = dir == 0 ? A.adjR : A.adjL;
    uint32_t cur = (RESUME && dir == dir0) ? cur0 : o;
    MemoCursor mc;
    // own memo first (its steps of this direction), else whatever memo the k1-mer was last written into
    bool following;
    if (RESUME && dir == dir0) following = memo_follow(A, A.hint[cur], cur, dir, mc);
    else {
      const uint32_t own = A.mvalid[r] ? (uint32_t)(((A.moff[r] + 2) << 2) | HINT_SEED) : NOHINT;
      following = memo_follow(A, own, o, dir, mc) || memo_follow(A, A.hint[o], o, dir, mc);
    }
    uint32_t cool = 0;                        // sequential steps to take before trusting a memo again
    Adj4 cand = {{-1, -1, -1, -1}};           // row of `cur` while walking sequentially
    bool have_cand = false;
    while (true) {
      if (following) {
        // 64 memo steps per trip.  A word with the top bit set (mark, header, hole) ends the segment; going backwards
        // the segment also ends after the memo walk's seed (the word before a seed is its header).
        const int64_t pi = mc.i + (int64_t)lane * mc.step;  // pool index of this lane's step
        const uint32_t mine = A.pool[pi];
        const u64 stopm = __ballot((mine & MEMO_HI) != 0);
        const uint32_t nchunk = stopm ? (uint32_t)(__ffsll((long long)stopm) - 1) : 64u;   // steps before the first stop word
        const bool at_mark = nchunk < 64u && __shfl(mine, (int)nchunk, 64) == MEMO_MARK;
        const bool is_term = mc.term && at_mark && (uint32_t)lane == nchunk;    // the memo walk stopped here: would I?
        const bool checked = (uint32_t)lane < nchunk || is_term;
        bool ok = false;
        if (checked) {
          const uint32_t before = lane == 0 ? cur : A.pool[pi - mc.step];
          // an entry counts only if its k1-mer's hint points at exactly this pool word (validated entries are distinct)
          bool valid = is_term || (A.hint[mine] >> 2) == (uint32_t)pi;
          if (valid) {
            Adj4 cd = adj[before];
            uint32_t bw;
            int b = decide(cd, r, A.claim, A.claim_old, A.weight, o, bw);
            uint32_t chosen = b < 0 ? NONE32 : (uint32_t)adj_get(cd, b);
            ok = chosen == (is_term ? NONE32 : mine);
          }
        }
        const u64 bad = __ballot(checked && !ok);
        const uint32_t m = bad ? (uint32_t)(__ffsll((long long)bad) - 1) : 64u;
        const uint32_t conf = min(m, nchunk);               // confirmed memo steps: lanes [0, conf)
        uint64_t myw = 0;
        if ((uint32_t)lane < conf) {
          note_claim(A, seen, r);
          seen = claim_node(A, mine, r, ns + lane + 1);
          myw = A.weight[mine];
        }
        for (int off = 32; off > 0; off >>= 1) myw += __shfl_xor(myw, off, 64);
        tot += myw;
        if (conf > 0) cur = __shfl(mine, (int)conf - 1, 64);
        if (A.dbg && lane == 0 && conf) atomicAdd(&A.dbg[DBG_FOREIGN], (unsigned long long)conf);
        ns += conf;
        mc.i += (int64_t)conf * mc.step;
        if (m == 64u) {
          if (nchunk < 64u) {
            if (is_term_any(mc.term, at_mark)) break;      // the terminal lane agreed: the walk ends where the memo's walk ended
            following = false;                // the segment just runs out (hole, or followed backwards): go on from its last k1-mer
            have_cand = false;
          }
          continue;
        }
        following = false;                    // decision m changed (or its entry is not trustworthy): go on sequentially
        have_cand = false;
        if (A.dbg && lane == 0) atomicAdd(&A.dbg[conf == 0 ? DBG_BROKE_FIRST : DBG_BROKE_LATER], 1ULL);
        if (conf == 0) cool = 2;
        continue;
      }
      // sequential step from `cur`: lanes 0..3 each fetch one candidate (claims, weight, hint and its own row, one
      // memory round trip), the decision is made by everybody from the shuffled weights
      if (!have_cand) cand = adj[cur];
      const int myc = lane == 0 ? cand.v[0] : lane == 1 ? cand.v[1] : lane == 2 ? cand.v[2] : lane == 3 ? cand.v[3] : -1;
      uint32_t hmy = NOHINT;
      uint32_t wmy = 0;
      Adj4 row = {{-1, -1, -1, -1}};
      bool avail = false;
      if (myc >= 0) {
        u64 cl = __hip_atomic_load(&A.claim[myc], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        u64 co = A.claim_old[myc];
        hmy = A.hint[myc];
        wmy = A.weight[(uint32_t)myc];
        row = adj[myc];
        avail = RANK(cl) > r && RANK(co) >= r;
      }
      const uint32_t am = (uint32_t)(__ballot(avail) & 0xFull);
      if (!am) break;
      const uint32_t w0 = __shfl(wmy, 0, 64), w1 = __shfl(wmy, 1, 64), w2 = __shfl(wmy, 2, 64), w3 = __shfl(wmy, 3, 64);
      int best = -1;
      uint32_t bw = 0;
#define CONSIDER(b, wb) if ((am >> b) & 1u) { if (best < 0 || wb > bw) { best = b; bw = wb; } }
      CONSIDER(0, w0) CONSIDER(2, w2) CONSIDER(1, w1) CONSIDER(3, w3)
#undef CONSIDER
      const uint32_t taken = (uint32_t)__shfl(myc, best, 64);
      const uint32_t hh = (uint32_t)__shfl((int)hmy, best, 64);
      cand.v[0] = __shfl(row.v[0], best, 64); cand.v[1] = __shfl(row.v[1], best, 64);
      cand.v[2] = __shfl(row.v[2], best, 64); cand.v[3] = __shfl(row.v[3], best, 64);
      have_cand = true;
      if (lane == 0) { note_claim(A, seen, r); seen = claim_node(A, taken, r, ns + 1); }
      tot += bw;
      ns++;
      nseq++;
      cur = taken;
      if (cool) cool--;
      else following = memo_follow(A, hh, taken, dir, mc, &why);
    }
    if (dir == 0) nr_new = ns;
  }
  note_claim(A, seen, r);
  if (A.dbg && lane == 0) {
    atomicMax(&A.dbg[DBG_MOST_SEQ], ((unsigned long long)nseq << 48) | ((unsigned long long)min(why.c2, 4095u) << 36) |
                              ((unsigned long long)min(why.c4, 4095u) << 12) | (unsigned long long)min(why.c7, 4095u));
    atomicMax(&A.dbg[DBG_LONGEST_WAVE], (unsigned long long)(ns - ns_start));
  }
  if (lane == 0) {
    A.nr_out[r] = nr_new;
    A.nl_out[r] = ns - nr_new;
    A.totw_out[r] = tot;
    const uint32_t mine = ns - ns_start;
    if (mine) atomicAdd(&A.wave_steps_counter[blockIdx.x & 63], (unsigned long long)mine);   // 64 slots: no single hot address
  }
  }
}

// ---- fixpoint audit, after the last block settles (always on; one pass over the claims, no walking): the claims are
// the fixpoint iff every claimed k1-mer is what its walk's greedy rule picks at the step before it, every walk ends
// where its rule finds nothing, and every walk owns exactly its recorded steps.  For walk r at step p a k1-mer is
// traversed if a lower rank owns it or r owns it at a step <= p.  A walk that fails is made dirty and the rounds go
// on with every block reopened -- the rounds' change tracking is an optimisation, this is the definition.
__global__ void ext_audit_nodes_kernel(const u64* __restrict__ claim, uint64_t n2, const RowView adjR, const RowView adjL,
                                       const WordView weight, const uint32_t* __restrict__ order,
                                       const uint32_t* __restrict__ nr_a, const uint32_t* __restrict__ nl_a, uint64_t ns,
                                       uint32_t* __restrict__ owned, uint8_t* __restrict__ dirty, unsigned long long* __restrict__ counters) {
  for (uint64_t y = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; y < n2; y += (uint64_t)gridDim.x * blockDim.x) {
    const u64 c = claim[y];
    const uint32_t r = RANK(c), p = POS(c);
    if (r == UNCLAIMED) continue;
    if (r >= ns) { atomicAdd(&counters[AUDIT_NODES], 1ULL); continue; }
    atomicAdd(&owned[r], 1u);
    const uint32_t nr = nr_a[r], nl = nl_a[r];
    bool bad = false;
    if (nr == UNCLAIMED || p > nr + nl) bad = true;                     // claim of a void walk / beyond its record
    else {
      if (p == 0) bad = order[r] != (uint32_t)y;
      else {
        // the step before: position p-1 going right, and the seed again for the first step to the left
        const bool right = p <= nr;
        const u64 want = CLAIM(r, p == nr + 1 ? 0u : p - 1);
        const Adj4 back = right ? adjL[y] : adjR[y];
        int32_t x = -1;
#pragma unroll
        for (int q = 0; q < 4; q++) if (back.v[q] >= 0 && claim[back.v[q]] == want) x = back.v[q];
        if (x < 0) bad = true;
        else {
          const Adj4 cd = right ? adjR[x] : adjL[x];
          const int b = audit_decide(cd, r, p - 1, claim, weight);
          bad = b < 0 || adj_get(cd, b) != (int32_t)y;
        }
      }
      if (!bad && p == nr) bad = audit_decide(adjR[y], r, nr, claim, weight) >= 0;                      // right end
      if (!bad && (nl ? p == nr + nl : p == 0)) bad = audit_decide(adjL[y], r, nr + nl, claim, weight) >= 0;   // left end
    }
    if (bad) { dirty[r] = 1; atomicAdd(&counters[AUDIT_NODES], 1ULL); }
  }
}

__global__ void ext_audit_walks_kernel(const u64* __restrict__ claim, const uint32_t* __restrict__ order, const uint32_t* __restrict__ nr_a,
                                       const uint32_t* __restrict__ nl_a, uint64_t ns, const uint32_t* __restrict__ owned,
                                       uint8_t* __restrict__ dirty, unsigned long long* __restrict__ counters) {
  uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ns) return;
  const u64 cs = claim[order[r]];
  const uint32_t nr = nr_a[r];
  const bool bad = nr == UNCLAIMED ? !(RANK(cs) < r && owned[r] == 0) : (cs != CLAIM((uint32_t)r, 0) || owned[r] != nr + nl_a[r] + 1u);
  if (bad) { dirty[r] = 1; atomicAdd(&counters[AUDIT_WALKS], 1ULL); }
}

// ---- audit (SHN_EXT_AUDIT=1, tests and stress runs): re-derive every walk from the converged claims alone, one thread
// per walk.  For walk r a k1-mer is traversed if a lower rank owns it or r owns it at a position already passed; the
// greedy choice at every step must be the k1-mer r owns at the next position, and the walk must end where its
// recorded counts say.  counters: AUDIT_BAD walks that disagree, AUDIT_LOWEST the lowest such rank
__global__ void ext_audit_kernel(WalkArgs A, uint64_t ns, unsigned long long* __restrict__ counters) {
  uint64_t r64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r64 >= ns) return;
  const uint32_t r = (uint32_t)r64;
  const uint32_t o = A.order[r];
  const u64 cs = A.claim[o];
  const uint32_t nr = A.nr_out[r], nl = A.nl_out[r];
  bool bad = false;
  if (nr == UNCLAIMED) bad = !(RANK(cs) < r);
  else if (cs != CLAIM(r, 0)) bad = true;
  else {
    uint32_t pos = 0;
    uint64_t tot = A.weight[o];
    for (int dir = 0; dir < 2 && !bad; dir++) {
      const RowView adj = dir == 0 ? A.adjR : A.adjL;
      const uint32_t end = dir == 0 ? nr : nr + nl;
      uint32_t cur = o;
      while (true) {
        Adj4 cd = adj[cur];
        int best = -1;
        uint32_t bw = 0;
#pragma unroll
        for (int bi = 0; bi < 4; bi++) {
          const int b = bi == 0 ? 0 : bi == 1 ? 2 : bi == 2 ? 1 : 3;
          if (cd.v[b] < 0) continue;
          const u64 c = A.claim[cd.v[b]];
          const bool avail = RANK(c) > r || (RANK(c) == r && POS(c) > pos);
          const uint32_t w = A.weight[(uint32_t)cd.v[b]];
          if (avail && (best < 0 || w > bw)) { best = b; bw = w; }
        }
        if (best < 0) { if (pos != end) bad = true; break; }
        if (pos == end) { bad = true; break; }                // the recorded walk stopped, the rule goes on
        const uint32_t nx = (uint32_t)adj_get(cd, best);
        if (A.claim[nx] != CLAIM(r, pos + 1)) { bad = true; break; }
        pos++; tot += bw; cur = nx;
      }
    }
    if (!bad && tot != A.totw_out[r]) bad = true;
  }
  if (bad) { atomicAdd(&counters[AUDIT_BAD], 1ULL); atomicMin(&counters[AUDIT_LOWEST], (unsigned long long)r); }
}

// classify the dirty walks of the open block: long ones (memo or recorded length) go to the wavefront kernel,
// the others to the thread kernel.  counters: PLAN_LONG, PLAN_NOMEMO (dirty walks that hold claims and have no current memo), PLAN_SHORT,
// PLAN_DIRTY
__global__ __launch_bounds__(1024) void ext_plan_kernel(uint32_t* nr, uint32_t* nl, uint64_t ns, uint32_t frozen,
                                const uint8_t* __restrict__ mvalid, const uint32_t* __restrict__ mR, const uint32_t* __restrict__ mL,
                                const uint8_t* __restrict__ dirty, uint32_t* __restrict__ long_list, uint32_t* __restrict__ short_list,
                                unsigned long long* __restrict__ counters, uint32_t long_walk, uint8_t* __restrict__ coarse,
                                const u64* __restrict__ fresh_claim, const uint32_t* __restrict__ order, uint64_t* __restrict__ totw,
                                uint8_t* __restrict__ robsat, unsigned long long* __restrict__ n_robsat, const uint32_t* __restrict__ log_head,
                                unsigned long long* __restrict__ rel_steps) {
  // ns here = current rank limit (walks >= limit have not started yet); walks < frozen are final and never run
  uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + frozen;
  const bool isd_all = r < ns && dirty[r];
  // coarse[i]: one of the 64 walks frozen + 64 i .. is dirty (the begin pass asks it before dirty[]: 1/64 of the bytes, they stay
  // in the L2 while the claims stream past)
  { const unsigned long long anyd = __ballot(isd_all); if ((threadIdx.x & 63) == 0) coarse[(r - frozen) >> 6] = anyd ? 1 : 0; }
  // fresh_claim != NULL: the first round of a block that has just opened -- every claim there is belongs to a final walk, so a walk
  // whose seed is claimed (by a lower rank: final walks are all lower) is void for good: its record is written here and it is on
  // no list.  At BASELINE configs[2] 98.6 % of the walks are void, most of them through walks of EARLIER blocks: the walk kernel of
  // the second and third block then runs over the survivors, packed -- not one live walk among 63 lanes that look at their seed and
  // idle until the wavefront's longest walk ends.
  bool isd = isd_all;
  if (isd && fresh_claim && RANK(fresh_claim[order[r]]) < r) { nr[r] = UNCLAIMED; nl[r] = 0; totw[r] = 0; isd = false; }
  bool lg = false;
  if (isd) {
    uint32_t a = nr[r];
    uint32_t len = a == UNCLAIMED ? 0 : a + nl[r];
    if (mvalid[r]) len = max(len, mR[r] + mL[r]);
    lg = len >= long_walk;
  }
  // one atomic per block of 1024 and list (one per wavefront on three single addresses was 39 us per launch)
  __shared__ uint32_t wl[16], wsh[16];
  __shared__ unsigned long long bl, bs, bd, bh;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned long long below = (1ULL << lane) - 1ULL;
  const unsigned long long lm = __ballot(isd && lg), sm = __ballot(isd && !lg);
  if (lane == 0) { wl[wid] = (uint32_t)__popcll(lm); wsh[wid] = (uint32_t)__popcll(sm); }
  if (threadIdx.x == 0) { bd = 0; bh = 0; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tl = 0, ts = 0;
    const int nw = (int)(blockDim.x >> 6);
    for (int w = 0; w < nw; w++) { tl += wl[w]; ts += wsh[w]; }
    bl = tl ? atomicAdd(&counters[PLAN_LONG], (unsigned long long)tl) : 0ULL;
    bs = ts ? atomicAdd(&counters[PLAN_SHORT], (unsigned long long)ts) : 0ULL;
  }
  {                                                                // dirty walks, the ones found void above included (they "ran")
    const unsigned long long dm = __ballot(isd_all);
    if (lane == 0 && dm) atomicAdd(&bd, (unsigned long long)__popcll(dm));
    // ... of them the ones that hold claims (a record of a live walk): with none, the round's begin pass has nothing to release
    // (counted: the holders WITHOUT a current memo -- with none of those, the dirty walks release their claims themselves, from
    // their memos: ext_release_memo_kernel)
    // (... nor a claim log: a walk that last ran in a bulk round gives its claims back through the log it wrote there)
    const bool holds = isd_all && nr[r] != UNCLAIMED;
    const bool has_log = holds && mvalid[r] != 2 && log_head && log_head[r] != LOG_LOST;      // (NONE32: it took no step -- its seed is all it holds)
    const unsigned long long hm = __ballot(holds && mvalid[r] != 2 && !has_log);
    if (lane == 0 && hm) atomicAdd(&bh, (unsigned long long)__popcll(hm));
    if (rel_steps && __ballot(holds)) {                           // the claims a targeted release would have to visit (most wavefronts hold no dirty walk at all)
      unsigned long long st = holds ? (unsigned long long)nr[r] + nl[r] + 1ULL : 0ULL;
      for (int o = 32; o > 0; o >>= 1) st += __shfl_down(st, o, 64);
      if (lane == 0 && st) atomicAdd(rel_steps, st);
    }
    if (robsat) {      // (development, SHN_EXT_XTIME: of those, the walks that were robbed while they sat out -- their chain of claims has a gap)
      const unsigned long long rm = __ballot(isd_all && nr[r] != UNCLAIMED && mvalid[r] != 2 && robsat[r]);
      if (lane == 0 && rm) atomicAdd(n_robsat + ROBSAT_WALKS, (unsigned long long)__popcll(rm));
      if (isd_all && nr[r] != UNCLAIMED && mvalid[r] != 2) { const unsigned long long len = (unsigned long long)nr[r] + nl[r]; atomicMax(n_robsat + ROBSAT_LONGEST, len); atomicAdd(n_robsat + ROBSAT_STEPS, len); }
      if (isd_all) robsat[r] = 0;                                    // (it runs now: what it holds afterwards is a fresh chain)
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && bd) atomicAdd(&counters[PLAN_DIRTY], bd);
  if (threadIdx.x == 0 && bh) atomicAdd(&counters[PLAN_NOMEMO], bh);
  __syncthreads();
  uint32_t ol = 0, os = 0;
  for (int w = 0; w < wid; w++) { ol += wl[w]; os += wsh[w]; }
  if (isd && lg) long_list[bl + ol + __popcll(lm & below)] = (uint32_t)r;
  if (isd && !lg) short_list[bs + os + __popcll(sm & below)] = (uint32_t)r;
}

// after the walkers: every walk that ran alive and is long enough gets a NEW memo slot for its new path (filled from
// the claims by ext_mark_kernel); old slots stay as they are -- the hints of k1-mers the walk no longer owns still lead
// to an intact path.  When the pool is full, no more memos are made (they only save time).
__global__ void ext_memo_plan_kernel(uint8_t* __restrict__ ran, uint8_t* __restrict__ dirty,
                                     const uint32_t* __restrict__ nr, const uint32_t* __restrict__ nl, const uint32_t* __restrict__ order,
                                     uint32_t frozen, uint32_t limit, uint64_t* __restrict__ moff, uint32_t* __restrict__ mR,
                                     uint32_t* __restrict__ mL, uint8_t* __restrict__ mvalid, uint8_t* __restrict__ fill,
                                     uint32_t* __restrict__ pool, unsigned long long* __restrict__ cursor, uint64_t pool_cap, uint32_t memo_min,
                                     uint32_t* __restrict__ log_head = nullptr) {
  uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + frozen;
  if (r >= limit) return;
  const uint8_t did_run = dirty[r];              // end-of-round bookkeeping: who ran, clean slate for the marks
  ran[r] = did_run;
  dirty[r] = 0;
  // (a walk that ran in a round without logging -- a round that makes memos -- holds other claims than its log says; one that took
  // no step holds its seed and nothing else: the empty log says so -- such a walk gets no memo slot either)
  if (log_head && did_run && memo_min != 0xFFFFFFFFu) log_head[r] = (nr[r] != UNCLAIMED && nr[r] + nl[r] == 0) ? NONE32 : LOG_LOST;
  uint8_t f = 0;
  if (did_run && nr[r] != UNCLAIMED) {
    const uint32_t R = nr[r], L = nl[r];
    if (R + L >= memo_min) {
      const uint64_t cap = (uint64_t)R + L + 5;
      const unsigned long long off = atomicAdd(cursor, (unsigned long long)cap);
      if (off + cap + 64 <= pool_cap) {
        pool[off] = MEMO_MARK; pool[off + 1] = R | MEMO_HI; pool[off + 2] = order[r];
        pool[off + 3 + R] = MEMO_MARK; pool[off + 4 + R + L] = MEMO_MARK;
        moff[r] = off; mR[r] = R; mL[r] = L; mvalid[r] = 2; f = 1;     // 2: the memo holds exactly the walk's claims (until it runs again)
      }
    }
  }
  if (did_run && !f && mvalid[r]) mvalid[r] = 1;     // ran without a new slot (a bulk round, a full pool, void now): the old memo is a hint only
  fill[r] = f;
}

// The release of a round that re-runs few walks, all of which have a current memo (the path of their last run, written from the
// claims by the mark pass of the round they ran in; they have not run since): a wavefront per dirty walk goes through its memo and
// gives back what the walk still owns.  The begin pass below streams all 11.6 GB of claims of BASELINE configs[2] to find those
// few thousand k1-mers -- 2.7 ms a round, half of the rounds of a step re-run fewer than 10,000 walks.
__global__ __launch_bounds__(64) void ext_release_memo_kernel(const uint32_t* __restrict__ long_list, uint64_t n_long, const uint32_t* __restrict__ short_list,
                                                              uint64_t n_short, const uint32_t* __restrict__ nr, const uint64_t* __restrict__ moff,
                                                              const uint32_t* __restrict__ mR, const uint32_t* __restrict__ mL, const uint32_t* __restrict__ pool,
                                                              u64* claim, uint8_t* __restrict__ chunk, const uint8_t* __restrict__ mvalid = nullptr,
                                                              const uint32_t* __restrict__ order = nullptr, const uint32_t* __restrict__ logpool = nullptr,
                                                              const uint32_t* __restrict__ log_head = nullptr, const uint8_t* __restrict__ log_cnt = nullptr) {
  const uint64_t idx = blockIdx.x;
  if (idx >= n_long + n_short) return;
  const uint32_t r = idx < n_long ? long_list[idx] : short_list[idx - n_long];
  if (nr[r] == UNCLAIMED) return;                                        // void: it holds nothing
  if (mvalid && mvalid[r] != 2) {
    // no current memo: the walk last ran in a bulk round and wrote a claim log there -- its seed, then the chunks from the last one
    // back; a k1-mer of the log that is no longer the walk's (a lower rank took it) stays as it is
    auto give_back = [&](uint32_t node) {
      const u64 c = __hip_atomic_load(&claim[node], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (RANK(c) == r && atomicCAS(&claim[node], c, UNCLAIMED64) == c && chunk) chunk[node >> CHUNK_SHIFT] = 1;
    };
    if (threadIdx.x == 0) give_back(order[r]);
    uint32_t ch = log_head[r], cnt = log_cnt[r];
    while (ch != NONE32 && ch != LOG_LOST) {
      const uint32_t* c = logpool + (uint64_t)ch * LOG_WORDS;
      if (threadIdx.x >= 1 && threadIdx.x <= cnt) give_back(c[threadIdx.x]);
      ch = c[0];
      cnt = LOG_PER;
    }
    return;
  }
  const uint64_t off = moff[r];
  const uint32_t R = mR[r], L = mL[r];
  for (uint32_t j = threadIdx.x; j <= R + L; j += 64) {
    const uint32_t node = pool[off + (j <= R ? 2 : 3) + j];
    if (node & 0x80000000u) continue;                                    // a step that was robbed before the memo was written
    if (atomicCAS(&claim[node], CLAIM(r, j), UNCLAIMED64) == CLAIM(r, j) && chunk) chunk[node >> CHUNK_SHIFT] = 1;
  }
}

// start of a round: snapshot the claims, drop the claims of the walks that are about to re-run, clear the round's counters
// (copy == 0: the snapshot is already the claims -- ext_mark_kernel brought it up to date where the last round changed something)
__global__ void ext_round_begin_kernel(u64* __restrict__ claim, u64* __restrict__ snap, uint64_t n2, const uint8_t* __restrict__ dirty,
                                       uint64_t ns, unsigned long long* __restrict__ d_cnt, int copy, uint8_t* __restrict__ chunk,
                                       uint32_t frozen, uint32_t limit, const uint8_t* __restrict__ coarse) {
  // four claims per thread, as two 16-byte loads (n2 is padded to a multiple of 4 by the allocation; the claims are 16-byte aligned):
  // with one 8-byte load per thread the pass ran at 3 TB/s
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) { d_cnt[CNT_CHANGED] = 0; d_cnt[CNT_SPARE] = 0; d_cnt[CNT_HANDED] = 0; }
  const uint64_t o0 = t * 4;
  if (o0 >= n2) return;
  ulonglong2 c01 = ((const ulonglong2*)(claim + o0))[0], c23 = ((const ulonglong2*)(claim + o0))[1];
  if (copy) { ((ulonglong2*)(snap + o0))[0] = c01; ((ulonglong2*)(snap + o0))[1] = c23; }
  // (only walks of the open block can be dirty: the flag of a final walk's k1-mer -- most claimed k1-mers in the later blocks --
  // is not looked up: a random byte read per claimed k1-mer otherwise)
  u64 c[4] = {c01.x, c01.y, c23.x, c23.y};
  bool any = false;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint32_t rk = RANK(c[q]);
    if (o0 + q < n2 && rk >= frozen && rk < limit && rk < ns && coarse[(rk - frozen) >> 6] && dirty[rk]) { c[q] = UNCLAIMED64; any = true; }
  }
  if (any) {
    ((ulonglong2*)(claim + o0))[0] = ulonglong2{c[0], c[1]}; ((ulonglong2*)(claim + o0))[1] = ulonglong2{c[2], c[3]};
    if (chunk) chunk[o0 >> CHUNK_SHIFT] = 1;
  }
}

// after a round: every k1-mer whose owner changed dirties the walks that looked at it; the k1-mers of the walks
// that got a memo slot are written into it (memo + hint)
__global__ void ext_mark_kernel(const u64* __restrict__ claim, u64* claim_old, uint64_t n2, Rec* __restrict__ rec,
                                uint8_t* __restrict__ dirty, const uint8_t* __restrict__ ran,
                                unsigned long long* __restrict__ n_changed, uint32_t frozen, uint32_t limit,
                                const uint8_t* __restrict__ fill /* NULL: no walk got a memo slot this round */, const uint64_t* __restrict__ moff, const uint32_t* __restrict__ mR,
                                uint32_t* __restrict__ pool,
                                const uint32_t* __restrict__ nr_a, const uint32_t* __restrict__ nl_a, int precise,
                                const uint8_t* __restrict__ chunk, uint8_t* __restrict__ robsat = nullptr) {
  const RowView adjR = rows_R(rec), adjL = rows_L(rec);
  const WordView weight = words_weight(rec);
  // grid-stride: the change counter costs one atomic per block (one per wavefront on a single address was the
  // most expensive thing in this kernel).  A wavefront takes 64 k1-mers at a time and, in rounds that re-run few walks
  // (chunk != NULL), looks only at the 128-byte lines of claims (16 k1-mers, one flag) a claim was written in this round
  // (claim_node and the release of the begin pass flag them): where nothing was written nothing changed, and every k1-mer of a
  // walk that ran was written.  The k1-mers of a walk are scattered over the table, so the flags have to be this fine: with a flag
  // per 64 k1-mers a round of 500 k short walks read 3 GB of claims and snapshot for its 3 M written k1-mers.
  uint32_t my_changed = 0;
  const uint64_t n_groups = (n2 + 63) >> 6;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  // the part every written k1-mer goes through; true: its owner changed to a higher rank (or nobody) -- the walks around it have to be looked at (mark_around)
  auto mark_node = [&](const uint64_t y, uint32_t& a_out) -> bool {
    const u64 oy = claim_old[y];
    const uint32_t a = RANK(oy);
    const u64 cy = claim[y];
    const uint32_t b = RANK(cy);
    // precise marks read the snapshot only at y itself: bring it up to date here, and the next round's begin pass has nothing
    // to copy (8 of the 32 bytes the two passes move per k1-mer and round)
    if (precise && oy != cy) claim_old[y] = cy;
    // (only walks of the open block can have run; a walk that got a slot ran.  In a bulk round nobody gets one, and a claimed
    // k1-mer whose owner did not change costs nothing beyond the two streams)
    if (fill && b >= frozen && b < limit && fill[b]) {            // slot layout: see MemoCursor
      const uint32_t pos = POS(cy), R = mR[b];
      const uint64_t idx = moff[b] + (pos <= R ? 2 : 3) + pos;
      if (pos) pool[idx] = (uint32_t)y;
      rec[y].hint = (uint32_t)(idx << 2) | (pos == 0 ? HINT_SEED : pos <= R ? HINT_R : HINT_L);
    }
    if (a == b) return false;
    my_changed++;
    // Who has to look again?  Walk x treats y as traversed iff its owner's rank is below x, and removing a
    // candidate it did not choose never changes a greedy choice -- so only walks for which y BECAME available
    // (a < x < b) are affected: the walks that stood next to y (owners of its 8 neighbours) and the walk seeded
    // on y (void while y belonged to a lower rank).  The old owner re-runs if it was robbed while it sat out this
    // round (one that ran this round gave y up knowingly; one that lost it during its run is caught by the verify
    // kernel); the new owner ran this round.  Walks below `frozen` are final, walks at or above `limit` have not
    // started (they all run when their phase opens).
#define MARK(x) if ((x) >= frozen && (x) < limit) dirty[x] = 1
    if (a != UNCLAIMED && !ran[a]) { MARK(a); if (robsat && a >= frozen && a < limit) robsat[a] = 1; }
    a_out = a;
    return b >= a;
  };
  auto mark_around = [&](const uint64_t y, const uint32_t a) {
    const uint32_t b = RANK(claim[y]);
#define MARKX(x) if (a < (x) && (x) < b) MARK(x)
    const uint32_t sr = rec[y].seed_rank;                        // (the same line as the two rows)
    MARKX(sr);
    Adj4 L = adjL[y], R = adjR[y];
#pragma unroll
    for (int q = 0; q < 8; q++) {
      int32_t nb = q < 4 ? L.v[q] : R.v[q - 4];
      if (nb < 0) continue;
      const u64 cz = claim[nb];
      const uint32_t z = RANK(cz);
      if (!precise) { uint32_t x = RANK(claim_old[nb]); MARKX(x); MARKX(z); continue; }
      // Precise: y became available to the walk z that stands next to it (a < z < b).  z has to look again only if its greedy
      // choice at nb, re-made from the final claims, is not the step it recorded there -- the same test the fixpoint audit
      // applies to every k1-mer, here applied where something changed.  (A former owner of nb either re-ran or was robbed
      // while it sat out and is marked at nb itself.)
      if (!(a < z && z < b) || z < frozen || z >= limit || dirty[z]) continue;
      const uint32_t pos = POS(cz), nrz = nr_a[z], nlz = nl_a[z];
      if (nrz == UNCLAIMED || pos > nrz + nlz) { dirty[z] = 1; continue; }
      const bool dirR = q < 4;                                   // y is a right candidate of nb (nb is a left neighbour of y)
      if (dirR ? pos > nrz : (pos != 0 && pos <= nrz)) continue;  // z left nb in the other direction: it never looked at y from here
      const uint32_t thr = dirR ? pos : (pos == 0 ? nrz : pos);   // own steps up to here count as traversed
      const bool has_next = dirR ? pos < nrz : (pos == 0 ? nlz > 0 : pos < nrz + nlz);
      const uint32_t next_pos = dirR ? pos + 1 : (pos == 0 ? nrz + 1 : pos + 1);
      const Adj4 cd = dirR ? adjR[nb] : adjL[nb];
      const int bsel = audit_decide(cd, z, thr, claim, weight);
      const bool same = has_next ? (bsel >= 0 && claim[adj_get(cd, bsel)] == CLAIM(z, next_pos)) : bsel < 0;
      if (!same) dirty[z] = 1;
    }
#undef MARKX
#undef MARK
  };
  if (!chunk) {
    for (uint64_t ch = wave; ch < n_groups; ch += n_waves) {
      const uint64_t y = (ch << 6) + lane;
      uint32_t a;
      if (y < n2 && mark_node(y, a)) mark_around(y, a);
    }
  } else {
    // 64 groups of 64 k1-mers per trip: every lane fetches the four line flags of one group, the wavefront then visits the groups
    // that have one set.  (Putting the k1-mers whose surroundings have to be looked at on a list for a second launch, 64 to a
    // wavefront, was slower: 235 against 210 ms per step -- the pass is bound by its random accesses, not by their latency.)
    static_assert(CHUNK_SHIFT == 4, "four line flags per group of 64 k1-mers");
    const uint64_t n_super = (n_groups + 63) >> 6;
    for (uint64_t sg = wave; sg < n_super; sg += n_waves) {
      const uint64_t g = (sg << 6) + lane;
      const uint32_t fl = g < n_groups ? *(const uint32_t*)(chunk + g * 4) : 0u;
      unsigned long long todo = __ballot(fl != 0);
      while (todo) {
        const int j = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t flj = (uint32_t)__shfl((int)fl, j, 64);
        const uint64_t y = ((((sg << 6) + (uint64_t)j)) << 6) + lane;
        uint32_t a = 0;
        if (y < n2 && ((flj >> (8 * (lane >> 4))) & 0xFFu) && mark_node(y, a)) mark_around(y, a);
      }
    }
  }
  __shared__ unsigned long long blk_changed;
  if (threadIdx.x == 0) blk_changed = 0;
  __syncthreads();
  if (my_changed) atomicAdd(&blk_changed, (unsigned long long)my_changed);
  __syncthreads();
  if (threadIdx.x == 0 && blk_changed) atomicAdd(n_changed, blk_changed);
}

// A walk that ran this round must own exactly the k1-mers on the path it recorded; if a lower rank took one of them during the
// round (before or after the walk claimed it: note_claim saw either) its record is stale: run it again.
__global__ void ext_verify_kernel(const uint8_t* __restrict__ ran, uint8_t* __restrict__ robbed, uint64_t ns, uint8_t* __restrict__ dirty) {
  uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ns) return;
  if (robbed[r]) { robbed[r] = 0; if (ran[r]) dirty[r] = 1; }
}

__global__ void ext_seed_rank_kernel(const uint32_t* __restrict__ order, uint64_t ns, Rec* __restrict__ rec) {
  uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < ns) rec[order[r]].seed_rank = (uint32_t)r;
}

extern "C" void shn_ext_destroy(shn_ext* e) {
  if (!e) return;
  hipSetDevice(e->device);
  void* ptrs[] = {e->d_weight, e->d_flags, e->d_rec, e->d_order, e->d_claim, e->d_nr, e->d_nl, e->d_totw};
  for (void* p : ptrs) if (p) shn_dev_free(p);
  if (e->owned_table) shn_table_destroy(e->owned_table);
  delete e;
}

// Pipelining hook: called from inside shn_extend, on the calling thread, whenever the walks of a rank block are final
// (lo <= rank < hi; their claims never change again), so that the caller can take their contigs and start the contig stage
// while the later blocks are still iterating.  status 0 = a block, 1 = the last block, -1 = the fixpoint audit reopened
// the blocks: everything handed over so far is void.  The shn_ext passed is valid for shn_ext_stats_range / shn_ext_emit /
// shn_ext_seed_info during the call-back.
typedef void (*shn_block_cb)(void* user, shn_ext* e, uint64_t lo, uint64_t hi, int status);
static thread_local shn_block_cb g_block_cb = nullptr;
static thread_local void* g_block_user = nullptr;
extern "C" void shn_ext_set_block_callback(shn_block_cb cb, void* user) { g_block_cb = cb; g_block_user = user; }

// checksum of one array into e->dig[stage] (added to what is there: a stage may be made of several arrays)
static int ext_digest(shn_ctx* ctx, shn_ext* e, int stage, const void* d, uint64_t bytes, uint64_t salt) {
  if (!bytes) return SHN_OK;
  hipStream_t s = ctx->stream;
  unsigned long long* d_out = nullptr;
  HIP_TRY(hipMalloc(&d_out, EXT_DIG_CHUNKS * 8));
  hipError_t er = hipMemsetAsync(d_out, 0, EXT_DIG_CHUNKS * 8, s);
  uint64_t h[EXT_DIG_CHUNKS];
  if (er == hipSuccess) {
    hipLaunchKernelGGL(ext_digest_kernel, dim3(1024), dim3(256), 0, s, (const uint32_t*)d, bytes / 4, salt, d_out);
    er = hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, s);
  }
  if (er == hipSuccess) er = hipStreamSynchronize(s);
  (void)hipFree(d_out);
  if (er != hipSuccess) return shn_fail(SHN_ERR_HIP, std::string("ext_digest: ") + hipGetErrorString(er));
  for (int i = 0; i < EXT_DIG_CHUNKS; i++) e->dig[stage][i] += h[i];
  e->has_dig = 1;
  return SHN_OK;
}
extern "C" int shn_ext_digests(const shn_ext* e, uint64_t* out) {
  if (!e || !out) return shn_fail(SHN_ERR_ARG, "shn_ext_digests: NULL argument");
  if (!e->has_dig) return shn_fail(SHN_ERR_ARG, "shn_ext_digests: the extension was not made with SHN_EXT_DIGEST=1");
  memcpy(out, e->dig, sizeof e->dig);
  return SHN_OK;
}

extern "C" int shn_extend(shn_ctx* ctx, const shn_table* t, uint32_t min_weight, int max_iterations, shn_ext** out) {
  return shn_extend_sharded(ctx, t, min_weight, max_iterations, 1, 0, out);
}

// ---- the driver of shn_extend_sharded: what is read once (ExtPlan, ExtSchedule), the state of a call (ExtRun), and the phases
// in the order they run.

// The words the driver reads a round's counts into: pinned (a pageable destination costs a staging copy kernel per round), one
// block per host thread, allocated once and kept.
struct ExtPlan {
  unsigned long long n_long, n_nomemo, n_short, n_dirty;   // the round's plan: CNT_PLAN, in PLAN_* order
  unsigned long long audit[2];                             // CNT_AUDIT (AUDIT_*)
  unsigned long long pool0;                                // what the memo pool's cursor starts at
  unsigned long long held;                                 // CNT_HELD
};
static_assert(sizeof(ExtPlan) == 64, "eight words");
static thread_local ExtPlan* g_ext_plan = nullptr;

// The switches of a call, read once (README.md has the table).
struct ExtSchedule {
  uint64_t pool_cap;                        // words of the memo pool
  unsigned long long lim0, grow, tail_div;  // rank blocks: the first one, the factor between them, the last ones = ns / tail_div walks (0: off)
  int precise_marks;                        // 0: the conservative rule (every walk standing next to a freed k1-mer)
  uint32_t long_walk, memo_min, promote_steps;
  unsigned long long bulk_min, dense_min;
  bool memo_release;                        // rounds whose dirty walks all have a current memo release through it (ext_release_memo_kernel)
  unsigned long long memo_release_max;
  bool prepass;                             // a block's first round settles the walks whose seed an earlier block holds (ext_plan_kernel)
  bool logs; uint64_t log_cap;              // claim logs and the chunks of their pool
  unsigned long long targeted_max;          // ... a round gives back at most this many claims through memos / logs
  uint64_t fault_round;                     // (tests: lose every mark of this round)
  bool debug, xtime, digest, audit, audit_fatal;
};
static ExtSchedule ext_schedule(uint64_t n, uint64_t ns) {
  ExtSchedule c;
  // memo slots are never recycled within a call (a word per step ever walked by a memo-bearing walk); pool
  // indices live in 30 bits of a hint
  c.pool_cap = std::min<uint64_t>(24 * n + (1ULL << 20), (1ULL << 30) - 1);
  c.pool_cap = shn_env_u64("SHN_EXT_POOL_WORDS", c.pool_cap, 256, c.pool_cap);   // (tests: a full pool only costs time)
  // Rank phases: a walk depends only on lower ranks, so the fixpoint is reached block by block -- first the
  // heaviest seeds (where the long, mutually dependent walks live), then geometrically larger blocks that see
  // final lower ranks and settle in a few rounds.
  // (many seeds -- BASELINE configs[2]: 186 M over 20,000 genes -- interfere locally: fewer, larger blocks; every round costs two
  // passes over all claims whatever it re-runs.  tools/ext_blocks_probe.py: 51 rounds / 2.27 s -> 32 rounds / 2.15 s)
  const bool many = ns >= (1ULL << 24);
  c.lim0 = shn_env_u64("SHN_EXT_LIMIT0", std::max<unsigned long long>(ns / (many ? 8 : 32), 4096));
  c.grow = shn_env_u64("SHN_EXT_GROW", 4);
  c.tail_div = shn_env_u64("SHN_EXT_TAIL", many ? 0 : 8);
  c.precise_marks = (int)shn_env_u64("SHN_EXT_PRECISE", 1);
  c.long_walk = (uint32_t)shn_env_u64("SHN_EXT_LONG_WALK", LONG_WALK);
  c.memo_min = (uint32_t)shn_env_u64("SHN_EXT_MEMO_MIN", MEMO_MIN);
  c.promote_steps = (uint32_t)shn_env_u64("SHN_EXT_PROMOTE", PROMOTE_STEPS);
  // Bulk rounds: with hundreds of thousands of dirty walks the GPU is throughput-bound, not latency-bound, and one thread
  // per walk (one memory round trip per step, every lane busy) beats a wavefront per walk by an order of magnitude; memos
  // (which serve the latency-bound re-runs of a few long walks) are not made in such a round.  The expected number of
  // dirty walks is the block size when a block opens, else the count of the round before.
  c.bulk_min = shn_env_u64("SHN_EXT_BULK", 262144);
  c.dense_min = shn_env_u64("SHN_EXT_DENSE", 4ULL << 20);   // (BASELINE configs[2]: 262144 -> 954 ms, 2 M or 16 M -> 900 ms per extension)
  c.memo_release = shn_env_u64("SHN_EXT_MEMO_RELEASE", 1) != 0;
  c.memo_release_max = shn_env_u64("SHN_EXT_MEMO_RELEASE_MAX", 65536);
  c.prepass = shn_env_u64("SHN_EXT_PREPASS", 1) != 0;
  // Claim logs (round 6; SHN_EXT_LOGS=0: off).  The begin pass streams every claim (11.6 GB at BASELINE configs[2], 2.7 ms) to find
  // those of the walks that re-run; 22 of a step's 25 rounds re-run walks that hold fewer than ten million claims between them, and
  // what kept them on the stream was a handful of claim holders per round WITHOUT a memo: walks that last ran in a bulk round (no
  // memos there: rebuilding them from the claims is a scattered store per claim).  Their chains are intact but thousands of steps
  // long -- following one from its seed is two dependent round trips a step (SHN_EXT_XTIME=1 says how many and how long).  So the
  // bulk walker writes the k1-mers it claims into a log of its own as it goes (a 4-byte store per step into a 32-byte chunk; a
  // wavefront reserves 64 chunks with one atomic), and a round whose claim holders all have a current memo or a log, and few
  // enough claims to give back, releases through those (ext_release_memo_kernel) instead of the stream.
  c.logs = shn_env_u64("SHN_EXT_LOGS", 1) != 0 && ns > 0;
  c.targeted_max = shn_env_u64("SHN_EXT_TARGETED_MAX", 12ULL << 20);
  c.log_cap = c.logs ? std::min<uint64_t>(2 * n / 4 + (1u << 16), 0x7FFFFFF0ULL) : 0;
  if (c.logs) c.log_cap = shn_env_u64("SHN_EXT_LOG_CHUNKS", c.log_cap, LOG_SLAB, c.log_cap);   // (tests: a pool that runs out -- the walks' logs are void and their rounds fall back to the begin pass)
  c.fault_round = shn_env_u64("SHN_EXT_FAULT", 0);
  c.debug = shn_env_set("SHN_DEBUG");
  c.xtime = shn_env_set("SHN_EXT_XTIME");
  c.digest = shn_env_flag("SHN_EXT_DIGEST", false);
  c.audit = shn_env_set("SHN_EXT_AUDIT");
  c.audit_fatal = shn_env_u64("SHN_EXT_AUDIT", 0) > 1;
  return c;
}

// Everything a call holds until it returns; the destructor gives it back, on every way out.
struct ExtRun {
  shn_ctx* ctx; const shn_table* t; hipStream_t s;
  uint64_t n, ns = 0;
  int max_iterations;
  shn_ext* e = nullptr;                     // under construction: destroyed with the run unless the caller has taken it
  ShnDevBufs bufs;                          // the seed pass's block counts and bases, robsat, chunk, coarse, logpool
  hipStream_t aux = nullptr;                // the wavefront walkers run beside the thread walkers
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  ExtSchedule sch;
  ExtPlan* plan = nullptr;
  unsigned long long* d_cnt = nullptr;      // the counter block (CNT_*)
  // scratch of the rounds: claim snapshot, memo pool, per-walk plan arrays
  u64 *claim = nullptr, *snap = nullptr;
  uint32_t* pool = nullptr;
  uint64_t* moff = nullptr;
  uint32_t *mR, *mL, *long_list, *short_list, *promo_list, *res_cur, *res_info, *owned;
  uint32_t* log_head;                       // claim logs: a walk's last chunk (LOG_LOST: none)
  uint8_t *mvalid, *fill, *dirty, *ran, *robbed;
  uint8_t* log_cnt;                         // claim logs: entries of a walk's last chunk
  uint8_t* robsat = nullptr;                // (development, SHN_EXT_XTIME: walks robbed while they sat out, until they run again)
  uint8_t* chunk = nullptr;                 // see ext_mark_kernel
  uint64_t n_chunks = 0;
  uint8_t* coarse = nullptr;                // see ext_plan_kernel
  uint32_t* logpool = nullptr;
  uint32_t g2n = 0;
  // the loop
  int it = 0, repairs = 0, n_begin_skipped = 0;
  bool converged = false;
  bool snap_current = false;                // the snapshot equals the claims (after a round with precise marks)
  bool fresh_block = true;                  // the open block has not run a round yet (and no repair has reopened earlier blocks)
  uint32_t frozen = 0, limit = 0;           // walks below frozen are final, walks at or above limit have not started
  unsigned long long expect_dirty = 0;
  // the SHN_DEBUG log: the round before
  double dbg_t_prev = 0;
  unsigned long long dbg_st_prev[2] = {0, 0};

  ExtRun(shn_ctx* c, const shn_table* tab, int max_it) : ctx(c), t(tab), s(c->stream), n(tab->n), max_iterations(max_it), bufs(c->stream) {}
  void close_aux() {
    if (aux) { hipStreamSynchronize(aux); hipStreamDestroy(aux); aux = nullptr; }
    if (ev_fork) { hipEventDestroy(ev_fork); ev_fork = nullptr; }
    if (ev_join) { hipEventDestroy(ev_join); ev_join = nullptr; }
  }
  ~ExtRun() { close_aux(); if (e) shn_ext_destroy(e); }
};
// what kind of round this one is: decided as its phases run, printed by the XTIME log
struct ExtRound { bool bulk, dense, was_fresh, snap_was_current, memo_release_done; };

// 1. the extension's own arrays; weights, flags and records of the table's k1-mers
static int ext_build_records(ExtRun& R, uint32_t min_weight) {
  shn_ctx* ctx = R.ctx; const shn_table* t = R.t; hipStream_t s = R.s; const uint64_t n = R.n;
  shn_ext* e = R.e = new shn_ext();
  memset(e, 0, sizeof(*e));
  e->ctx = ctx; e->device = ctx->device; e->k = t->k; e->n = t->n; e->min_weight = min_weight; e->table = t;
  HIP_TRY(shn_dev_malloc(&e->d_weight, (n + 1) * 4));
  HIP_TRY(shn_dev_malloc(&e->d_flags, n + 1));
  HIP_TRY(shn_dev_malloc(&e->d_rec, (2 * n + 1) * sizeof(Rec)));
  // claims and snapshot in one block ((+4: the begin pass reads four claims per thread); the dictionary of the records kernel is
  // built in it first, see build_fine_dict)
  const uint64_t claim_words = (2 * n + 4 + 31) & ~31ULL;
  { u64* both = nullptr;
    HIP_TRY(shn_dev_malloc(&both, std::max<uint64_t>(2 * claim_words * 8, fine_dict_lines(t) * 128)));
    e->d_claim = both; e->d_claim2 = both + claim_words; }
  if (n) {
    TimerRegion t1(ctx, T_EXT_PREP);
    ext_prepare_launch(s, t, e->d_weight, e->d_flags);
    {
      unsigned long long* lines = nullptr;
      uint64_t n_lines = 0;
      { int rca = build_fine_dict(ctx, t, e->d_flags, &lines, &n_lines, e->d_claim); if (rca) return rca; }
      // (the kernel strides over the k1-mers its grid does not cover: above 2^22 blocks -- 134 M k1-mers -- or, in tests, SHN_EXT_ADJ_BLOCKS)
      const uint64_t full_grid = std::min<uint64_t>(cdiv(n * 8, 256), 1u << 22);
      const uint64_t adj_blocks = shn_env_u64("SHN_EXT_ADJ_BLOCKS", full_grid, 1, full_grid);
      { TimerRegion ta(ctx, T_EXT_ADJ);                  // (one launch: bench.py's roofline entry for this kernel)
        hipLaunchKernelGGL(ext_records_kernel, dim3((uint32_t)adj_blocks), dim3(256), 0, s, shn_tab_idx(t),
                           e->d_flags, e->d_weight, n, t->k, t->canonical, e->d_rec, (const unsigned long long*)lines, n_lines); }
      (void)lines;                                       // (lives in the claims' block: overwritten when the claims are initialised below)
    }
    HIP_TRY(hipGetLastError());
  }
  return SHN_OK;
}

// 2. the seeds: counted, gathered, sorted by string then (stable) by weight descending; the walks' records and the claims start empty
static int ext_order_seeds(ExtRun& R) {
  shn_ctx* ctx = R.ctx; const shn_table* t = R.t; hipStream_t s = R.s; shn_ext* e = R.e; const uint64_t n = R.n;
  void *pk, *pv, *pk2, *pv2, *pc;
  int rc;
  if ((rc = shn_ws(ctx)[13].get(CNT_WORDS * 8, &pc))) return rc;
  R.d_cnt = (unsigned long long*)pc;
  // the seeds are counted first: the sort buffers are sized for them, not for every oriented k1-mer (at 20,000 genes 13 % of
  // the table are seeds -- 30 GB less)
  HIP_TRY(hipMemsetAsync(R.d_cnt, 0, CNT_WORDS * 8, s));
  const uint64_t n_sblk = cdiv(n, 1024);
  uint32_t* d_bcnt = nullptr; uint64_t* d_bbase = nullptr;
  HIP_TRY(R.bufs.get(&d_bcnt, (n_sblk + 1) * 4));
  HIP_TRY(R.bufs.get(&d_bbase, (n_sblk + 2) * 8));
  if (n) hipLaunchKernelGGL(ext_seed_kernel, dim3((uint32_t)n_sblk), dim3(1024), 0, s, t->d_keys, e->d_weight, e->d_flags, n,
                            t->k, t->canonical, e->min_weight, d_bcnt, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr);
  uint64_t ns = 0;
  if (n && (rc = shn_device_scan_u32(ctx, d_bcnt, n_sblk, d_bbase, &ns))) return rc;
  if ((rc = shn_ws(ctx)[9].get((ns + 2) * 8, &pk)) || (rc = shn_ws(ctx)[10].get((ns + 2) * 4, &pv)) ||
      (rc = shn_ws(ctx)[11].get((ns + 2) * 8, &pk2)) || (rc = shn_ws(ctx)[12].get((ns + 2) * 4, &pv2))) return rc;
  uint64_t* skeys = (uint64_t*)pk; uint32_t* svals = (uint32_t*)pv;
  if (n) hipLaunchKernelGGL(ext_seed_kernel, dim3((uint32_t)n_sblk), dim3(1024), 0, s, t->d_keys, e->d_weight, e->d_flags, n,
                            t->k, t->canonical, e->min_weight, d_bcnt, (const uint64_t*)d_bbase, skeys, svals);
  R.ns = e->n_seeds = ns;
  {
    TimerRegion t2(ctx, T_EXT_SORT);
    if ((rc = shn_sort_pairs(ctx, skeys, svals, (uint64_t*)pk2, (uint32_t*)pv2, ns, 0, 2 * t->k))) return rc;
    if (ns) {
      hipLaunchKernelGGL(ext_weightkey_kernel, dim3((uint32_t)cdiv(ns, 256)), dim3(256), 0, s, svals, e->d_weight, ns, skeys);
      if ((rc = shn_sort_pairs(ctx, skeys, svals, (uint64_t*)pk2, (uint32_t*)pv2, ns, 0, 32))) return rc;
    }
  }
  HIP_TRY(shn_dev_malloc(&e->d_order, (ns + 1) * 4));
  HIP_TRY(shn_dev_malloc(&e->d_nr, (ns + 1) * 4));
  HIP_TRY(shn_dev_malloc(&e->d_nl, (ns + 1) * 4));
  HIP_TRY(shn_dev_malloc(&e->d_totw, (ns + 1) * 8));
  HIP_TRY(hipMemcpyAsync(e->d_order, svals, ns * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemsetAsync(e->d_nr, 0xFF, (ns + 1) * 4, s));
  HIP_TRY(hipMemsetAsync(e->d_nl, 0, (ns + 1) * 4, s));
  HIP_TRY(hipMemsetAsync(e->d_totw, 0, (ns + 1) * 8, s));
  HIP_TRY(hipMemsetAsync(e->d_claim, 0xFF, (2 * n + 4) * 8, s));
  return SHN_OK;
}

// the rank of the walk seeded on it into the record of every seed (hints and seed ranks live in the records: ext_records_kernel
// wrote "none" into both)
static void ext_seed_ranks(ExtRun& R) {
  if (R.ns) hipLaunchKernelGGL(ext_seed_rank_kernel, dim3((uint32_t)cdiv(R.ns, 256)), dim3(256), 0, R.s, R.e->d_order, (uint64_t)R.ns, R.e->d_rec);
}

// 3. the scratch of the rounds -- memo pool, per-walk plan arrays, flags, claim logs -- and the first block
static int ext_setup_rounds(ExtRun& R) {
  shn_ctx* ctx = R.ctx; const shn_table* t = R.t; hipStream_t s = R.s; shn_ext* e = R.e; const uint64_t n = R.n, ns = R.ns;
  const ExtSchedule& sch = R.sch = ext_schedule(n, ns);
  void *ppool, *pplan;
  int rc;
  if ((rc = shn_ws(ctx)[27].get(sch.pool_cap * 4, &ppool)) ||
      (rc = shn_ws(ctx)[28].get((ns + 1) * (8 + 4 * 10 + 1 + 1 + 1 + 1 + 1 + 1) + 64, &pplan))) return rc;
  R.claim = e->d_claim; R.snap = e->d_claim2;
  R.pool = (uint32_t*)ppool;
  R.moff = (uint64_t*)pplan;
  uint32_t* mcap = (uint32_t*)(R.moff + ns + 1);
  R.mR = mcap + ns + 1;
  R.mL = R.mR + ns + 1;
  R.long_list = R.mL + ns + 1;
  R.short_list = R.long_list + ns + 1;
  R.promo_list = R.short_list + ns + 1;
  R.res_cur = R.promo_list + ns + 1;
  R.res_info = R.res_cur + ns + 1;
  R.owned = R.res_info + ns + 1;
  R.log_head = R.owned + ns + 1;
  R.mvalid = (uint8_t*)(R.log_head + ns + 1);
  R.fill = R.mvalid + ns + 1;
  R.dirty = R.fill + ns + 1;
  R.ran = R.dirty + ns + 1;
  R.robbed = R.ran + ns + 1;
  R.log_cnt = R.robbed + ns + 1;
  HIP_TRY(hipMemsetAsync(R.robbed, 0, ns + 1, s));
  HIP_TRY(hipMemsetAsync(R.log_head, 0xFE, (ns + 1) * 4, s));
  if (sch.xtime) { HIP_TRY(R.bufs.get(&R.robsat, ns + 1)); HIP_TRY(hipMemsetAsync(R.robsat, 0, ns + 1, s)); }
  HIP_TRY(hipMemsetAsync(R.mvalid, 0, 2 * (ns + 1), s));
  HIP_TRY(hipMemsetAsync(R.pool, 0xFF, sch.pool_cap * 4, s));            // NONE32: "no entry"
  ext_seed_ranks(R);
  if (sch.digest) {
    int rd;
    if ((rd = ext_digest(ctx, e, 0, t->d_keys, n * 8, 1)) || (rd = ext_digest(ctx, e, 1, t->d_counts, n * 4, 2)) ||
        (rd = ext_digest(ctx, e, 2, t->d_bucket_off, (t->n_buckets + 1) * 8, 3)) || (rd = ext_digest(ctx, e, 3, e->d_weight, n * 4, 4)) ||
        (rd = ext_digest(ctx, e, 3, e->d_flags, n & ~3ULL, 5)) || (rd = ext_digest(ctx, e, 4, e->d_rec, 2 * n * sizeof(Rec), 6)) ||
        (rd = ext_digest(ctx, e, 5, e->d_order, ns * 4, 7))) return rd;
  }
  HIP_TRY(hipStreamCreateWithFlags(&R.aux, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&R.ev_fork, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&R.ev_join, hipEventDisableTiming));
  if (!g_ext_plan) HIP_TRY(hipHostMalloc((void**)&g_ext_plan, sizeof(ExtPlan)));
  R.plan = g_ext_plan;
  R.converged = ns == 0;
  R.n_chunks = ((2 * n) >> CHUNK_SHIFT) + 16;
  HIP_TRY(R.bufs.get(&R.chunk, R.n_chunks));
  HIP_TRY(hipMemsetAsync(R.chunk, 0, R.n_chunks, s));
  HIP_TRY(R.bufs.get(&R.coarse, (size_t)ns / 64 + 64));
  R.g2n = (uint32_t)cdiv(2 * n, 256);
  R.frozen = 0; R.limit = (uint32_t)std::min<unsigned long long>(ns, sch.lim0);
  HIP_TRY(hipMemsetAsync(R.dirty, 0, 2 * (ns + 1), s));               // dirty + ran
  HIP_TRY(hipMemsetAsync(R.dirty, 1, R.limit, s));
  HIP_TRY(hipMemsetAsync(R.owned, 0, (ns + 1) * 4, s));
  R.plan->pool0 = 64;                                                 // memo pool cursor: 64 words of NONE32 padding in front
  HIP_TRY(hipMemcpyAsync(R.d_cnt + CNT_POOL, &R.plan->pool0, 8, hipMemcpyHostToDevice, s));   // (from the pinned block, on the context's stream like everything else here)
  if (sch.logs) { HIP_TRY(R.bufs.get(&R.logpool, sch.log_cap * LOG_WORDS * 4)); HIP_TRY(hipMemsetAsync(R.d_cnt + CNT_LOG, 0, 8, s)); }
  R.expect_dirty = R.limit;
  return SHN_OK;
}

// 4a. classify the dirty walks of the open block; a block without dirty walks is consistent = final
static int ext_plan_round(ExtRun& R, bool bulk) {
  hipStream_t s = R.s; shn_ext* e = R.e; const ExtSchedule& sch = R.sch; unsigned long long* d_cnt = R.d_cnt;
  HIP_TRY(hipMemsetAsync(d_cnt + CNT_PLAN, 0, 32, s));
  HIP_TRY(hipMemsetAsync(d_cnt + CNT_HELD, 0, 8, s));
  if (R.limit > R.frozen)
    hipLaunchKernelGGL(ext_plan_kernel, dim3((uint32_t)cdiv(R.limit - R.frozen, 1024)), dim3(1024), 0, s, e->d_nr, e->d_nl, (uint64_t)R.limit, R.frozen,
                       R.mvalid, R.mR, R.mL, R.dirty, R.long_list, R.short_list, d_cnt + CNT_PLAN, bulk ? 0xFFFFFFFFu : sch.long_walk, R.coarse,
                       (R.fresh_block && R.frozen > 0 && sch.prepass) ? (const u64*)R.claim : (const u64*)nullptr, e->d_order, e->d_totw,
                       R.robsat, d_cnt + CNT_ROBSAT,
                       sch.logs ? (const uint32_t*)R.log_head : (const uint32_t*)nullptr, d_cnt + CNT_HELD);
  HIP_TRY(hipMemcpyAsync(&R.plan->n_long, d_cnt + CNT_PLAN, 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&R.plan->held, d_cnt + CNT_HELD, 8, hipMemcpyDeviceToHost, s));      // the claims the dirty walks hold (by their records)
  HIP_TRY(hipStreamSynchronize(s));
  R.expect_dirty = R.plan->n_dirty;
  return SHN_OK;
}

// 4b. every block is settled: audit the claims (see ext_audit_nodes_kernel); a walk that is not at its fixpoint
// re-runs with all blocks open.  Never seen to fire in testing except by fault injection (SHN_EXT_FAULT).
// Leaves R.converged set, or R.repairs counted up (more than 16: the caller gives up).
static int ext_audit_fixpoint(ExtRun& R) {
  hipStream_t s = R.s; shn_ext* e = R.e; ExtPlan* plan = R.plan; unsigned long long* d_cnt = R.d_cnt; const uint64_t n = R.n, ns = R.ns;
  TimerRegion ta(R.ctx, T_EXT_AUDIT);
  HIP_TRY(hipMemsetAsync(R.owned, 0, (ns + 1) * 4, s));
  HIP_TRY(hipMemsetAsync(d_cnt + CNT_AUDIT, 0, 16, s));
  hipLaunchKernelGGL(ext_audit_nodes_kernel, dim3(std::min<uint32_t>(R.g2n, 4096u)), dim3(256), 0, s, R.claim, 2 * n, rows_R(e->d_rec),
                     rows_L(e->d_rec), words_weight(e->d_rec), e->d_order, e->d_nr, e->d_nl, (uint64_t)ns, R.owned, R.dirty, d_cnt + CNT_AUDIT);
  hipLaunchKernelGGL(ext_audit_walks_kernel, dim3((uint32_t)cdiv(ns, 256)), dim3(256), 0, s, R.claim, e->d_order, e->d_nr, e->d_nl, (uint64_t)ns,
                     R.owned, R.dirty, d_cnt + CNT_AUDIT);
  HIP_TRY(hipMemcpyAsync(plan->audit, d_cnt + CNT_AUDIT, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (plan->audit[AUDIT_NODES] == 0 && plan->audit[AUDIT_WALKS] == 0) {
    R.converged = true;
    if (g_block_cb) g_block_cb(g_block_user, e, R.frozen, ns, 1);
    return SHN_OK;
  }
  if (g_block_cb) g_block_cb(g_block_user, e, 0, 0, -1);
  fprintf(stderr, "[shn_extend] fixpoint audit after %d rounds: %llu k1-mers / %llu walks disagree with the greedy rule; reopening all blocks\n",
          R.it, plan->audit[AUDIT_NODES], plan->audit[AUDIT_WALKS]);
  if (++R.repairs > 16) return SHN_OK;
  R.fresh_block = false;
  R.frozen = 0;
  R.expect_dirty = plan->audit[AUDIT_NODES] + plan->audit[AUDIT_WALKS];
  HIP_TRY(hipMemsetAsync(R.ran, 0, ns + 1, s));
  HIP_TRY(hipMemsetAsync(R.owned, 0, (ns + 1) * 4, s));
  return SHN_OK;
}

// 4b'. the open block is final: hand it to the call-back and open the next one
static int ext_open_next_block(ExtRun& R) {
  const ExtSchedule& sch = R.sch; const uint64_t ns = R.ns;
  if (g_block_cb && R.repairs == 0) g_block_cb(g_block_user, R.e, R.frozen, R.limit, 0);
  R.frozen = R.limit;
  // geometric blocks up to half of the walks, then blocks of ns / tail_div: the light half of the seed order settles in
  // a few cheap rounds per block, and what a block call-back receives early can be worked on beside the later blocks
  if (sch.tail_div && ((unsigned long long)R.frozen + ns / 16) * 2 >= ns) R.limit = (uint32_t)std::min<unsigned long long>(ns, (unsigned long long)R.frozen + std::max<unsigned long long>(1, ns / sch.tail_div));
  else R.limit = (uint32_t)std::min<unsigned long long>(ns, (unsigned long long)R.limit * sch.grow);
  HIP_TRY(hipMemsetAsync(R.ran, 0, R.frozen, R.s));       // frozen walks never run again
  HIP_TRY(hipMemsetAsync(R.dirty + R.frozen, 1, R.limit - R.frozen, R.s));
  R.expect_dirty = R.limit - R.frozen;
  R.fresh_block = R.repairs == 0;
  return SHN_OK;
}

// 4c. snapshot, then release the claims of the walks that re-run this round
// (a block that has just opened holds no claims yet: with the snapshot up to date there is nothing to release and nothing to copy)
// (... and so does a round none of whose dirty walks holds a claim -- void walks looking at their seed again: n_nomemo)
static int ext_release_claims(ExtRun& R, ExtRound& rd) {
  hipStream_t s = R.s; shn_ext* e = R.e; const ExtSchedule& sch = R.sch; const ExtPlan* plan = R.plan; unsigned long long* d_cnt = R.d_cnt;
  const bool memo_release = !R.fresh_block && !rd.dense && sch.memo_release && plan->n_nomemo == 0 &&
                            (sch.logs ? plan->held <= sch.targeted_max : plan->n_long + plan->n_short <= sch.memo_release_max);
  rd.snap_was_current = R.snap_current;
  rd.memo_release_done = !R.fresh_block && memo_release && sch.precise_marks && R.snap_current;
  if ((R.fresh_block || memo_release) && sch.precise_marks && R.snap_current) {
    HIP_TRY(hipMemsetAsync(d_cnt + CNT_CHANGED, 0, 16, s)); HIP_TRY(hipMemsetAsync(d_cnt + CNT_HANDED, 0, 8, s));
    if (!R.fresh_block) {
      R.n_begin_skipped++;
      if (plan->n_long + plan->n_short)
        hipLaunchKernelGGL(ext_release_memo_kernel, dim3((uint32_t)(plan->n_long + plan->n_short)), dim3(64), 0, s, R.long_list, (uint64_t)plan->n_long, R.short_list, (uint64_t)plan->n_short,
                           e->d_nr, R.moff, R.mR, R.mL, R.pool, R.claim, R.chunk, (const uint8_t*)R.mvalid, (const uint32_t*)e->d_order, (const uint32_t*)R.logpool,
                           (const uint32_t*)R.log_head, (const uint8_t*)R.log_cnt);
    }
  }
  else {
    TimerRegion tb(R.ctx, T_EXT_BEGIN);
    hipLaunchKernelGGL(ext_round_begin_kernel, dim3((uint32_t)cdiv(cdiv(2 * R.n, 4), 256)), dim3(256), 0, s, R.claim, R.snap, 2 * R.n, R.dirty, (uint64_t)R.ns, d_cnt,
                       (!sch.precise_marks || !R.snap_current) ? 1 : 0, rd.dense ? (uint8_t*)nullptr : R.chunk, R.frozen, R.limit, R.coarse);
  }
  R.snap_current = true;
  return SHN_OK;
}

// 4d. the walkers: a wavefront per long walk on the second stream, a thread per short walk beside them; in a round that is not
// a bulk round the thread walker hands the walks that turn out long to a second launch of the wavefront walker
static int ext_launch_walkers(ExtRun& R, const ExtRound& rd) {
  shn_ctx* ctx = R.ctx; hipStream_t s = R.s, aux = R.aux; shn_ext* e = R.e; const ExtSchedule& sch = R.sch; const ExtPlan* plan = R.plan;
  unsigned long long* d_cnt = R.d_cnt; const uint64_t ns = R.ns;
  WalkArgs A;
  A.order = e->d_order; A.adjR = rows_R(e->d_rec); A.adjL = rows_L(e->d_rec); A.weight = words_weight(e->d_rec);
  A.claim = R.claim; A.claim_old = R.snap;
  A.nr_out = e->d_nr; A.nl_out = e->d_nl; A.totw_out = e->d_totw;
  A.pool = R.pool; A.moff = R.moff; A.mR = R.mR; A.mL = R.mL; A.mvalid = R.mvalid; A.hint = words_hint(e->d_rec);
  A.promote_steps = rd.bulk ? 0xFFFFFFFFu : sch.promote_steps;   // (in a bulk round a thread walker walks to the end itself)
  A.promo_list = R.promo_list; A.promo_count = d_cnt + CNT_HANDED; A.res_cur = R.res_cur; A.res_info = R.res_info;
  A.chunk = rd.dense ? nullptr : R.chunk;         // (dense rounds write nearly everywhere: their mark pass is dense, the walkers do not flag)
  A.robbed = R.robbed;
  A.logpool = (sch.logs && rd.bulk) ? R.logpool : nullptr; A.log_head = R.log_head; A.log_cnt = R.log_cnt; A.log_cursor = d_cnt + CNT_LOG; A.log_cap = sch.log_cap;
  A.steps_counter = d_cnt + CNT_STEPS; A.fresh_steps_counter = d_cnt + CNT_FRESH_STEPS; A.wave_steps_counter = d_cnt + CNT_WAVE_STEPS;
  A.dbg = (sch.debug || sch.xtime) ? d_cnt + CNT_DBG : nullptr;
  // long (wave per walk) and short (thread per walk) kernels are independent: overlap them on two streams
  if (plan->n_long) {
    HIP_TRY(hipEventRecord(R.ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(aux, R.ev_fork, 0));
    { TimerRegion tk(ctx, T_EXT_WALK_WAVE, aux);
      hipLaunchKernelGGL(ext_walk_long_kernel<false>, dim3((uint32_t)plan->n_long), dim3(64), 0, aux, A, R.long_list, (uint64_t)ns, (const unsigned long long*)nullptr); }
    HIP_TRY(hipEventRecord(R.ev_join, aux));
  }
  double x_t0 = 0;
  if (sch.xtime) {   // (development: time of every thread-walker launch)
     HIP_TRY(hipStreamSynchronize(s)); timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); x_t0 = ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }
  if (plan->n_short) {
    TimerRegion tk(ctx, rd.was_fresh ? T_EXT_WALK_FRESH : T_EXT_WALK_THREAD);
    if (rd.was_fresh) hipLaunchKernelGGL(ext_walk_kernel<true>, dim3((uint32_t)cdiv(plan->n_short, WBLK)), dim3(WBLK), 0, s, A, (uint64_t)plan->n_short, R.short_list, R.snap);
    else hipLaunchKernelGGL(ext_walk_kernel<false>, dim3((uint32_t)cdiv(plan->n_short, WBLK)), dim3(WBLK), 0, s, A, (uint64_t)plan->n_short, R.short_list, R.snap);
  }
  if (x_t0 > 0) {
    HIP_TRY(hipStreamSynchronize(s)); timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
    unsigned long long st = 0, lw = 0; HIP_TRY(hipMemcpyAsync(&st, d_cnt + CNT_STEPS, 8, hipMemcpyDeviceToHost, s));
    if (A.dbg) { HIP_TRY(hipMemcpyAsync(&lw, d_cnt + CNT_DBG + DBG_LONGEST_THREAD, 8, hipMemcpyDeviceToHost, s)); HIP_TRY(hipMemsetAsync(d_cnt + CNT_DBG + DBG_LONGEST_THREAD, 0, 8, s)); }
    HIP_TRY(hipStreamSynchronize(s));
    unsigned long long nrs[3] = {0, 0, 0}; HIP_TRY(hipMemcpyAsync(nrs, d_cnt + CNT_ROBSAT, 24, hipMemcpyDeviceToHost, s)); HIP_TRY(hipMemsetAsync(d_cnt + CNT_ROBSAT, 0, 24, s)); HIP_TRY(hipStreamSynchronize(s));
    fprintf(stderr, "[shn_extend] XTIME round %d [%u,%u): of the claim holders without a memo %llu were robbed while they sat out; their walks: longest %llu steps, %llu steps in all\n", R.it + 1, R.frozen, R.limit, nrs[ROBSAT_WALKS], nrs[ROBSAT_LONGEST], nrs[ROBSAT_STEPS]);
    fprintf(stderr, "[shn_extend] XTIME round %d: release %s (claims to give back by the records: %llu; bulk %d dense %d fresh %d snapshot current %d)\n", R.it + 1,
            rd.was_fresh ? "none (a new block)" : rd.memo_release_done ? "through memos / logs" : "the begin pass", plan->held, (int)rd.bulk, (int)rd.dense, (int)rd.was_fresh, (int)rd.snap_was_current);
    fprintf(stderr, "[shn_extend] XTIME round %d: %llu dirty walks, %llu of them hold claims without a current memo (rounds released through memos so far: %d); thread walker %llu walks, %.2f ms, steps so far %llu; longest walk %llu steps in %.2f ms (%.2f us per step)\n", R.it + 1, plan->n_dirty, plan->n_nomemo, R.n_begin_skipped, plan->n_short,
            ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6 - x_t0, st, lw >> 32, (double)(lw & 0xFFFFFFFFULL) * 1e-5, (lw >> 32) ? (double)(lw & 0xFFFFFFFFULL) * 1e-2 / (double)(lw >> 32) : 0.0);
  }
  if (plan->n_short && !rd.bulk) {             // walks the thread kernel handed over (the count stays on the device)
    TimerRegion tk(ctx, T_EXT_WALK_WAVE);
    hipLaunchKernelGGL(ext_walk_long_kernel<true>, dim3((uint32_t)std::min<unsigned long long>(plan->n_short, 8192ULL)), dim3(64), 0, s, A, R.promo_list,
                       (uint64_t)ns, (const unsigned long long*)(d_cnt + CNT_HANDED));
  }
  if (plan->n_long) HIP_TRY(hipStreamWaitEvent(s, R.ev_join, 0));
  return SHN_OK;
}

// 4e. who has to run next round?  walks whose view changed (mark) + walks that lost a claim race (verify);
// the walks that ran get their memo rebuilt from the claims
static int ext_mark_and_verify(ExtRun& R, const ExtRound& rd) {
  hipStream_t s = R.s; shn_ext* e = R.e; const ExtSchedule& sch = R.sch; unsigned long long* d_cnt = R.d_cnt; const uint64_t n = R.n, ns = R.ns;
  // A block's first round when it is a bulk round: no walk of the block held a claim before it, so every change is
  // "nobody -> a walk of the block" -- nothing the mark pass would mark (a k1-mer only BECOMES available to somebody when a lower
  // rank gives it up), no memo slots to fill; what is left of the pass is bringing the snapshot up to date, which the next begin
  // pass does while it streams the claims anyway (copy = 1): the pass is skipped (3 x 25 ms at BASELINE configs[2]).
  const bool skip_mark = rd.was_fresh && rd.bulk && sch.precise_marks;
  R.fresh_block = false;
  if (rd.dense) e->dense_rounds++;
  hipLaunchKernelGGL(ext_memo_plan_kernel, dim3((uint32_t)cdiv(R.limit - R.frozen, 256)), dim3(256), 0, s, R.ran, R.dirty, e->d_nr, e->d_nl, e->d_order, R.frozen, R.limit,
                     R.moff, R.mR, R.mL, R.mvalid, R.fill, R.pool, d_cnt + CNT_POOL, sch.pool_cap, rd.bulk ? 0xFFFFFFFFu : sch.memo_min, sch.logs ? R.log_head : (uint32_t*)nullptr);
  if (skip_mark) { R.snap_current = false; if (!rd.dense) HIP_TRY(hipMemsetAsync(R.chunk, 0, R.n_chunks, s)); }
  else
  { TimerRegion tk(R.ctx, T_EXT_MARK);
    hipLaunchKernelGGL(ext_mark_kernel, dim3(std::min<uint32_t>(R.g2n, 4096u)), dim3(256), 0, s, R.claim, R.snap, 2 * n, e->d_rec,
                       R.dirty, R.ran, d_cnt + CNT_CHANGED, R.frozen, R.limit, rd.bulk ? (const uint8_t*)nullptr : (const uint8_t*)R.fill, R.moff, R.mR, R.pool, e->d_nr, e->d_nl, sch.precise_marks,
                       rd.dense ? (const uint8_t*)nullptr : R.chunk, R.robsat);
    if (!rd.dense) HIP_TRY(hipMemsetAsync(R.chunk, 0, R.n_chunks, s)); }
  hipLaunchKernelGGL(ext_verify_kernel, dim3((uint32_t)cdiv(ns, 256)), dim3(256), 0, s, R.ran, R.robbed, (uint64_t)ns, R.dirty);
  if ((uint64_t)(R.it + 1) == sch.fault_round) HIP_TRY(hipMemsetAsync(R.dirty, 0, ns + 1, s));   // (tests: lose every mark of this round)
  R.it++;
  return SHN_OK;
}

// 4f. SHN_DEBUG: a line per round
static int ext_log_round(ExtRun& R) {
  hipStream_t s = R.s; const ExtPlan* plan = R.plan; unsigned long long* d_cnt = R.d_cnt;
  unsigned long long chg = 0, cur = 0, mx[2] = {0, 0}, st_tr[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&st_tr[0], d_cnt + CNT_STEPS, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&st_tr[1], d_cnt + CNT_TRIPS, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&chg, d_cnt + CNT_CHANGED, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&cur, d_cnt + CNT_POOL, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(mx, d_cnt + CNT_DBG + DBG_MOST_SEQ, 16, hipMemcpyDeviceToHost, s));        // DBG_MOST_SEQ, DBG_LONGEST_WAVE
  HIP_TRY(hipMemsetAsync(d_cnt + CNT_DBG + DBG_MOST_SEQ, 0, 16, s));
  HIP_TRY(hipStreamSynchronize(s));
  timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
  double tn = ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
  unsigned long long* st_prev = R.dbg_st_prev;
  fprintf(stderr, "[shn_extend] round %d [%u,%u): dirty=%llu long=%llu short=%llu changed_kmers=%llu pool=%.1f%% longest wavefront walk: %llu steps, most sequential: %llu (no hint %llu, owner without memo %llu, memo moved on %llu, followed %llu)  thread steps %llu in %llu wavefront trips (lanes busy %.3f)  %.2f ms\n", R.it, R.frozen, R.limit,
          plan->n_dirty, plan->n_long, plan->n_short, chg, 100.0 * (double)cur / (double)R.sch.pool_cap, mx[1], mx[0] >> 48, (mx[0] >> 36) & 4095, (mx[0] >> 24) & 4095, (mx[0] >> 12) & 4095, mx[0] & 4095,
          st_tr[0] - st_prev[0], st_tr[1] - st_prev[1], (double)(st_tr[0] - st_prev[0]) / (64.0 * (double)std::max<unsigned long long>(1, st_tr[1] - st_prev[1])), R.it == 1 ? 0.0 : tn - R.dbg_t_prev);
  st_prev[0] = st_tr[0]; st_prev[1] = st_tr[1];
  R.dbg_t_prev = tn;
  return SHN_OK;
}

// 4. the rounds: until no walk of the last block is dirty and the audit agrees
static int ext_iterate(ExtRun& R) {
  const ExtSchedule& sch = R.sch;
  int rc;
  while (!R.converged && R.it < R.max_iterations) {
    ExtRound rd;
    rd.bulk = sch.bulk_min && R.expect_dirty >= sch.bulk_min;
    // dense: the begin / mark passes stream all claims (rounds that write nearly everywhere); else they follow the 128-byte-line
    // flags the walkers and the release leave behind.  A bulk round of a few hundred thousand walks writes a few million
    // k1-mers: far fewer lines than the 23 GB of claims and snapshot the dense passes read.
    rd.dense = rd.bulk && R.expect_dirty >= sch.dense_min;
    if ((rc = ext_plan_round(R, rd.bulk))) return rc;
    if (R.plan->n_dirty == 0) {
      if (R.limit < R.ns) { if ((rc = ext_open_next_block(R))) return rc; continue; }
      if ((rc = ext_audit_fixpoint(R))) return rc;
      if (R.converged || R.repairs > 16) break;
      continue;
    }
    TimerRegion t3(R.ctx, T_EXT_WALK);
    rd.was_fresh = R.fresh_block;
    if ((rc = ext_release_claims(R, rd)) || (rc = ext_launch_walkers(R, rd)) || (rc = ext_mark_and_verify(R, rd))) return rc;
    if (sch.debug && (rc = ext_log_round(R))) return rc;
  }
  return SHN_OK;
}

// 5. SHN_EXT_AUDIT (tests and stress runs): every walk again from the converged claims alone (ext_audit_kernel)
static int ext_rewalk_audit(ExtRun& R) {
  hipStream_t s = R.s; shn_ext* e = R.e; ExtPlan* plan = R.plan; unsigned long long* d_cnt = R.d_cnt; const uint64_t ns = R.ns;
  WalkArgs A;
  memset(&A, 0, sizeof(A));
  A.order = e->d_order; A.adjR = rows_R(e->d_rec); A.adjL = rows_L(e->d_rec); A.weight = words_weight(e->d_rec);
  A.claim = R.claim; A.nr_out = e->d_nr; A.nl_out = e->d_nl; A.totw_out = e->d_totw;
  plan->audit[AUDIT_BAD] = 0; plan->audit[AUDIT_LOWEST] = ~0ULL;
  HIP_TRY(hipMemcpyAsync(d_cnt + CNT_AUDIT, plan->audit, 16, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(ext_audit_kernel, dim3((uint32_t)cdiv(ns, 64)), dim3(64), 0, s, A, (uint64_t)ns, d_cnt + CNT_AUDIT);
  HIP_TRY(hipMemcpyAsync(plan->audit, d_cnt + CNT_AUDIT, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (plan->audit[AUDIT_BAD]) {
    fprintf(stderr, "[shn_extend] AUDIT: %llu walks are not at their fixpoint, lowest rank %llu of %llu (rounds %d)\n", plan->audit[AUDIT_BAD], plan->audit[AUDIT_LOWEST],
            (unsigned long long)ns, R.it);
    if (R.sch.audit_fatal) return shn_fail(SHN_ERR_INTERNAL, "shn_extend: audit failed");
  }
  return SHN_OK;
}

// 6. the last two stage checksums, the step totals; what only the rounds needed goes back
static int ext_finish(ExtRun& R) {
  shn_ctx* ctx = R.ctx; hipStream_t s = R.s; shn_ext* e = R.e; unsigned long long* d_cnt = R.d_cnt; const uint64_t n = R.n, ns = R.ns;
  if (R.sch.digest) {
    int rd;
    if ((rd = ext_digest(ctx, e, 6, R.claim, 2 * n * 8, 8)) || (rd = ext_digest(ctx, e, 7, e->d_nr, ns * 4, 9)) || (rd = ext_digest(ctx, e, 7, e->d_nl, ns * 4, 10)) ||
        (rd = ext_digest(ctx, e, 7, e->d_totw, ns * 8, 11))) return rd;
  }
  // what is left to do with the result (stats, emit, seed info, weights) reads the claims, the walk records and the table: the
  // records and the snapshot (most of the state) go back to the allocator now
  HIP_TRY(hipStreamSynchronize(s));
  shn_dev_free(e->d_rec); e->d_rec = nullptr;
  e->d_claim2 = nullptr;                                   // (not used any more; its memory goes back with the claims')
  unsigned long long steps = 0, wsteps = 0, fsteps = 0, wslots[64];
  HIP_TRY(hipMemcpyAsync(&steps, d_cnt + CNT_STEPS, 8, hipMemcpyDeviceToHost, s));          // thread-kernel steps
  HIP_TRY(hipMemcpyAsync(&fsteps, d_cnt + CNT_FRESH_STEPS, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(wslots, d_cnt + CNT_WAVE_STEPS, 64 * 8, hipMemcpyDeviceToHost, s));    // wavefront-kernel steps
  HIP_TRY(hipStreamSynchronize(s));
  for (int i = 0; i < 64; i++) wsteps += wslots[i];
  steps += wsteps;
  if (R.sch.debug) {
    unsigned long long dbg[10];
    HIP_TRY(hipMemcpyAsync(dbg, d_cnt + CNT_DBG, 80, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    fprintf(stderr, "[shn_extend] converged after %d rounds; steps: %llu total, %llu in the wave kernel (%llu from own memos, %llu from foreign memos)\n",
            R.it, steps, wsteps, dbg[DBG_OWN], dbg[DBG_FOREIGN]);
    fprintf(stderr, "[shn_extend] memo_follow: no hint %llu, owner without memo %llu, memo moved on %llu, followed backwards %llu, nothing left %llu, followed %llu; "
            "chunks broken at the first step %llu, later %llu\n", dbg[DBG_WHY + 2], dbg[DBG_WHY + 3], dbg[DBG_WHY + 4], dbg[DBG_WHY + 5], dbg[DBG_WHY + 6], dbg[DBG_WHY + 7],
            dbg[DBG_BROKE_FIRST], dbg[DBG_BROKE_LATER]);
  }
  e->total_steps = steps;
  e->wave_steps = wsteps;
  e->fresh_steps = fsteps;
  HIP_TRY(hipGetLastError());
  return SHN_OK;
}

extern "C" int shn_extend_sharded(shn_ctx* ctx, const shn_table* t, uint32_t min_weight, int max_iterations, int world, int rank,
                                  shn_ext** out) {
  if (!ctx || !t || !out) return shn_fail(SHN_ERR_ARG, "shn_extend: NULL argument");
  if (world < 1 || world > 255 || rank < 0 || rank >= world) return shn_fail(SHN_ERR_ARG, "shn_extend_sharded: bad world/rank");
  if (2 * t->n >= 0x7FFFFFFFULL) return shn_fail(SHN_ERR_ARG, "shn_extend: table too large for 31-bit oriented ids");
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  shn_use_stream(ctx->stream);
  if (world > 1 && t->n) {
    shn_table* sub = nullptr;
    int rcs;
    { TimerRegion treg(ctx, T_EXTEND); rcs = component_shard(ctx, t, world, rank, &sub); }
    if (rcs) return rcs;
    rcs = shn_extend_sharded(ctx, sub, min_weight, max_iterations, 1, 0, out);
    if (rcs) { shn_table_destroy(sub); return rcs; }
    (*out)->owned_table = sub;
    return SHN_OK;
  }
  TimerRegion treg(ctx, T_EXTEND);
  ExtRun R(ctx, t, max_iterations <= 0 ? 100000 : max_iterations);
  int rc;
  if ((rc = ext_build_records(R, min_weight)) || (rc = ext_order_seeds(R)) || (rc = ext_setup_rounds(R)) || (rc = ext_iterate(R))) return rc;
  R.close_aux();
  if (R.converged && R.ns && R.sch.audit && (rc = ext_rewalk_audit(R))) return rc;
  R.e->iterations = R.it;
  if (!R.converged) return shn_fail(SHN_ERR_INTERNAL, "shn_extend: walk fixpoint did not converge");
  if ((rc = ext_finish(R))) return rc;
  *out = R.e;
  R.e = nullptr;
  return SHN_OK;
}

// Test hook (tests/test_ext_setup_gpu.py): phases 1 and 2 of the driver above and the seed ranks, unchanged, for world = 1 -- no
// scratch of the rounds, no walk -- and what they left on the device as host arrays.  Every output may be NULL.  Not part of the path.
extern "C" int shn_debug_ext_setup(shn_ctx* ctx, const shn_table* t, uint32_t min_weight, uint32_t* weight_out /* n */, uint8_t* flags_out /* n */,
                                   int32_t* rows_out /* 2n x 8: R[0..3], L[0..3] */, uint32_t* rec_weight_out /* 2n */, uint32_t* seed_rank_out /* 2n */,
                                   uint64_t* n_seeds_out, uint32_t* order_out /* room for 2n, n_seeds written */) {
  if (!ctx || !t) return shn_fail(SHN_ERR_ARG, "shn_debug_ext_setup: NULL argument");
  if (2 * t->n >= 0x7FFFFFFFULL) return shn_fail(SHN_ERR_ARG, "shn_debug_ext_setup: table too large for 31-bit oriented ids");
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  ExtRun R(ctx, t, 1);
  int rc;
  if ((rc = ext_build_records(R, min_weight)) || (rc = ext_order_seeds(R))) return rc;
  ext_seed_ranks(R);
  HIP_TRY(hipGetLastError());
  const uint64_t n = R.n, ns = R.ns;
  hipStream_t s = R.s;
  const shn_ext* e = R.e;
  std::vector<Rec> rec((rows_out || rec_weight_out || seed_rank_out) ? 2 * n : 0);
  if (n && weight_out) HIP_TRY(hipMemcpyAsync(weight_out, e->d_weight, n * 4, hipMemcpyDeviceToHost, s));
  if (n && flags_out) HIP_TRY(hipMemcpyAsync(flags_out, e->d_flags, n, hipMemcpyDeviceToHost, s));
  if (!rec.empty()) HIP_TRY(hipMemcpyAsync(rec.data(), e->d_rec, rec.size() * sizeof(Rec), hipMemcpyDeviceToHost, s));
  if (ns && order_out) HIP_TRY(hipMemcpyAsync(order_out, e->d_order, ns * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (uint64_t o = 0; o < rec.size(); o++) {
    if (rows_out) for (int b = 0; b < 4; b++) { rows_out[8 * o + b] = rec[o].R.v[b]; rows_out[8 * o + 4 + b] = rec[o].L.v[b]; }
    if (rec_weight_out) rec_weight_out[o] = rec[o].weight;
    if (seed_rank_out) seed_rank_out[o] = rec[o].seed_rank;
  }
  if (n_seeds_out) *n_seeds_out = ns;
  return SHN_OK;                                   // (the run gives the extension under construction back)
}
