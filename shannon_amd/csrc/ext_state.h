// The state of a contig extension (extend.hip makes it, ext_results.hip reads it): the record of an oriented k1-mer, the claim
// words, struct shn_ext.
#pragma once
#include "common.h"

#define UNCLAIMED 0xFFFFFFFFu
#define NONE32 0xFFFFFFFFu
#define UNCLAIMED64 0xFFFFFFFFFFFFFFFFULL
typedef unsigned long long u64;
#define CLAIM(rank, pos) (((u64)(rank) << 32) | (u64)(uint32_t)(pos))
#define RANK(c) ((uint32_t)((c) >> 32))
#define POS(c) ((uint32_t)(c))

struct Adj4 { int32_t v[4]; };
// Everything about an oriented k1-mer that does not change while the walks iterate, in ONE 64-byte line: both adjacency rows, its
// weight, and the two words the mark pass keeps per k1-mer (memo hint, rank of the walk seeded on it).  A walk step used to touch
// four arrays per candidate (claims, snapshot, weights, rows); the rows and the weight of a candidate -- and whatever the mark
// pass needs around a changed k1-mer -- now come with one sector.  The bulk rounds are bound by the NUMBER of random 64-byte
// sectors the chip serves (~30 G/s measured, at any lane occupancy), so sectors per step is what the layout is chosen for.
// The claims and their snapshot stay compact arrays of their own: the begin / mark / audit / emit passes stream them.
struct __attribute__((aligned(64))) Rec {
  Adj4 R;                // oriented id reached by appending base b, or -1
  Adj4 L;                // ... by prepending base b
  uint32_t weight;       // weight of the string in the doubled input
  uint32_t hint;         // where this k1-mer was last written into a memo (pool index << 2 | kind), NOHINT if never
  uint32_t seed_rank;    // rank of the walk seeded on it, 0xFFFFFFFF if it is not a seed
  uint32_t pad[5];
};
static_assert(sizeof(Rec) == 64, "one line per oriented k1-mer");
// rows of one direction / the weights / the hints, indexed by oriented id (strided views of the record array)
struct RowView { const char* p; __device__ __forceinline__ Adj4 operator[](uint32_t i) const { return *(const Adj4*)(p + ((uint64_t)i << 6)); } };
struct WordView { const char* p; __device__ __forceinline__ uint32_t operator[](uint32_t i) const { return *(const uint32_t*)(p + ((uint64_t)i << 6)); } };
__host__ __device__ __forceinline__ RowView rows_R(const Rec* r) { return RowView{(const char*)r}; }
__host__ __device__ __forceinline__ RowView rows_L(const Rec* r) { return RowView{(const char*)r + 16}; }
__host__ __device__ __forceinline__ WordView words_weight(const Rec* r) { return WordView{(const char*)r + 32}; }
__host__ __device__ __forceinline__ WordView words_hint(const Rec* r) { return WordView{(const char*)r + 36}; }

// ---- stage checksums (SHN_EXT_DIGEST=1; tests/test_stress_gpu.py, tools/stress_digest.py): two runs on the same input must agree
// stage by stage; the first stage that differs -- and the 1/64 of its array where -- localises a run-to-run difference.
// Stages: 0 table keys, 1 table counts, 2 bucket offsets, 3 weights + flags, 4 records (adjacency rows, weight, seed rank; before the
// first round), 5 seed order, 6 converged claims, 7 walk records (n_right, n_left, total weight).
#define EXT_DIG_STAGES 8
#define EXT_DIG_CHUNKS 64
struct shn_ext {
  shn_ctx* ctx;
  int device;
  int k;
  uint64_t n;            // canonical entries
  uint64_t n_seeds;
  int iterations;
  uint32_t min_weight;
  const shn_table* table;
  shn_table* owned_table; // sharded: the k1-mers of this rank's components (table points at it)
  uint32_t* d_weight;    // [n] weight of the string in the doubled input (count, x2 for palindromes)
  uint8_t* d_flags;      // [n] bit0 palindrome, bit1 low complexity
  Rec* d_rec;            // [2n] per oriented k1-mer: adjacency rows, weight, memo hint, seed rank (see Rec)
  uint32_t* d_order;     // [n_seeds] oriented id of the seed with rank r
  u64* d_claim;          // [2n] converged claims: (rank of the owning walk) << 32 | (1 + step index on its path)
  u64* d_claim2;         // [2n] scratch (the second half of the block d_claim starts: freed with it)
  uint64_t total_steps;  // walk steps executed over all iterations (for the bench's byte model)
  uint64_t wave_steps;   // ... of which by the wavefront kernel
  uint64_t fresh_steps;  // ... of which by the thread walker in the first round of a rank block
  int dense_rounds;      // rounds whose begin / mark passes streamed all claims
  uint32_t* d_nr;        // [n_seeds] right steps (UNCLAIMED = void walk)
  uint32_t* d_nl;        // [n_seeds]
  uint64_t* d_totw;      // [n_seeds] sum of weights incl. the seed
  uint64_t dig[EXT_DIG_STAGES][EXT_DIG_CHUNKS];   // SHN_EXT_DIGEST=1: checksums of the stages' arrays (shn_ext_digests)
  int has_dig;
};

// components.hip: the table of the k1-mers of the components that rank `rank` of `world` walks (see component_shard there)
int component_shard(shn_ctx* ctx, const shn_table* t, int world, int rank, shn_table** out);
