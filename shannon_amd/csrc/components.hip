// Connected components of the k1-mer graph, and the tables of whole components the ranks of a multi-GPU job walk: on a replicated
// table (component_shard, behind shn_extend_sharded) and on owner shards (shn_cc_*).
#include "ext_state.h"
#include "k1dict.h"
#include "runs.h"
#include <cstring>
#include <vector>
#include <algorithm>

// ---- connected components of the k1-mer graph (vertices = canonical k1-mers, edges = the adjacency rows).
// A walk never leaves its component, so the components can be extended independently -- on different GPUs.
// Lock-free union-find: roots only ever link to smaller ids (no cycles), finds halve paths as they go.
__device__ __forceinline__ uint32_t cc_find(uint32_t* lab, uint32_t x) {
  uint32_t cur = x;
  while (true) {
    uint32_t p = __hip_atomic_load(&lab[cur], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == cur) return cur;
    uint32_t gp = __hip_atomic_load(&lab[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gp != p) __hip_atomic_store(&lab[cur], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cur = p;
  }
}
__global__ void cc_init_kernel(uint32_t* __restrict__ lab, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) lab[i] = (uint32_t)i;
}
__device__ __forceinline__ void cc_unite(uint32_t* lab, uint32_t u, uint32_t v) {
  while (true) {
    const uint32_t ru = cc_find(lab, u), rv = cc_find(lab, v);
    if (ru == rv) return;
    const uint32_t hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
    if (atomicCAS(&lab[hi], hi, lo) == hi) return;
  }
}
// Every edge of the k1-mer graph straight from the table, no adjacency rows in between: one thread per (canonical k1-mer, which),
// which = 0..7: the eight neighbours of its forward orientation (append / prepend a base: the other orientation has the same
// ones), which = 8..15: its siblings.  contig_connections joins contigs that share a K-mer (extension_correction.py:372-390):
// besides adjacent k1-mers those are k1-mers with the same K-suffix (x.m, x'.m) or the same K-prefix (m.y, m.y') -- not adjacent,
// and only joined through a common neighbour if that neighbour exists and is not low-complexity (a transcript's last K-mer before
// a poly-A tail is the typical exception).  So the labelling also unites every k1-mer with its (up to six) siblings.
// Look-ups as in the records kernel: eight lanes per canonical k1-mer, through the one-line dictionary.
__global__ void cc_edges_kernel(const TabIdx T, const uint8_t* __restrict__ flags,
                                uint64_t n, int k, int canonical, uint32_t* lab, const unsigned long long* __restrict__ lines, uint64_t n_lines) {
  const uint64_t* __restrict__ tkeys = T.keys;
  const uint64_t mask = (k == 32) ? ~0ULL : ((1ULL << (2 * k)) - 1);
  const uint64_t total = n * 8, rounded = (total + 63) & ~63ULL;
  const int lane = threadIdx.x & 63, g0 = lane & ~7, p = lane & 7;
  SHN_GRID_FOR(gid, rounded) {
    const bool in = gid < total;
    const uint64_t i = in ? gid >> 3 : 0;
    const bool dead = !in || (flags[i] & 2);
    const uint64_t str = tkeys[i];
#pragma unroll
    for (int half = 0; half < 2; half++) {
      uint64_t mykey;
      {
        const uint64_t b = (uint64_t)(p & 3);
        bool skip = dead;
        if (half == 0) mykey = (p & 4) ? ((str >> 2) | (b << (2 * (k - 1)))) : (((str << 2) | b) & mask);
        else if (p & 4) { skip |= (str & 3) == b; mykey = (str & ~3ULL) | b; }
        else { const int sh = 2 * (k - 1); skip |= ((str >> sh) & 3) == b; mykey = (str & ~(3ULL << sh)) | (b << sh); }
        if (canonical) { const uint64_t rc = shn_revcomp(mykey, k); if (rc < mykey) mykey = rc; }
        // (every edge is seen from both of its ends -- the neighbour and sibling relations are symmetric, and so is "both not
        // low-complexity" -- so an end asks only for the larger keys: half the look-ups; what is not asked goes to line 0, which the
        // caches hold)
        if (skip || mykey <= str) mykey = 0;
      }
      const uint64_t myline = mykey ? fd_bucket(T, mykey, n_lines) : 0ULL;
      uint64_t key[8];
      ulonglong2 v[8];
#pragma unroll
      for (int q = 0; q < 8; q++) {
        key[q] = shfl_u64(mykey, g0 + q);
        v[q] = ((const ulonglong2*)(lines + shfl_u64(myline, g0 + q) * 16))[p];
      }
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const uint32_t w = fd_match(v[q], lines, shfl_u64(myline, g0 + q), key[q], p, g0, T, flags);
        // (lane q of the group does the union: eight independent ones side by side)
        if (w != 0xFFFFFFFFu && p == q && (uint64_t)(w & ~FD_PAL) != i) cc_unite(lab, (uint32_t)i, w & ~FD_PAL);
      }
    }
  }
}
// Every k1-mer gets its root.  The find here must NOT compress: a compressing find of one thread stores an ancestor into lab[j]
// (correct inside the union-find, where any ancestor will do) -- and when that store lands after thread j has written j's root, j
// keeps a label that is not a root.  Found in round 5 when the labelling asked every edge from one end only: the trees were deeper
// at this point, 70 % of the runs left 1-40 k1-mers of a 227 k table with an ancestor for a label (a k1-mer then went to another
// rank than its component).  With every edge united twice the trees are all but flat here and the window almost never opened --
// almost.  Without stores other than the roots themselves, every value a find can read is an ancestor and the roots do not move.
__device__ __forceinline__ uint32_t cc_find_readonly(const uint32_t* lab, uint32_t x) {
  uint32_t cur = x;
  while (true) {
    const uint32_t p = __hip_atomic_load(&lab[cur], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == cur) return cur;
    cur = p;
  }
}
__global__ void cc_flatten_kernel(uint32_t* lab, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const uint32_t r = cc_find_readonly(lab, (uint32_t)i); __hip_atomic_store(&lab[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
}
// size estimate of the components from every 64th k1-mer (a full count would hammer a handful of addresses)
__global__ void cc_sample_kernel(const uint32_t* __restrict__ lab, uint64_t n, uint32_t* __restrict__ size_s) {
  uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 64;
  if (i < n) atomicAdd(&size_s[lab[i]], 1u);
}
// owner of every root by hash; roots of big components are listed for the host to balance
__global__ void cc_owner_kernel(const uint32_t* __restrict__ lab, const uint32_t* __restrict__ size_s, uint64_t n, uint32_t world,
                                uint8_t* __restrict__ owner_root, uint32_t* __restrict__ big_root, uint32_t* __restrict__ big_size,
                                unsigned long long* __restrict__ n_big, uint32_t big_cap) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (lab[i] != (uint32_t)i) { owner_root[i] = 0xFF; return; }
  owner_root[i] = (uint8_t)(shn_mix64((uint64_t)i ^ 0x5851F42D4C957F2DULL) % world);
  if (size_s[i] >= 16) {
    unsigned long long p = atomicAdd(n_big, 1ULL);
    if (p < big_cap) { big_root[p] = (uint32_t)i; big_size[p] = size_s[i]; }
  }
}
__global__ void cc_assign_kernel(const uint32_t* __restrict__ big_root, const uint8_t* __restrict__ big_owner, uint32_t n_big,
                                 uint8_t* __restrict__ owner_root) {
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n_big) owner_root[big_root[j]] = big_owner[j];
}

// ---- component shard of a k1-mer table: the walks of a connected component of the k1-mer graph touch no other
// component, so a rank that is given whole components needs only their k1-mers.  Labels the components (lock-free
// union-find over the adjacency rows), gives every component to one rank (the big ones balanced by sampled size,
// the rest by hash -- the same on every rank) and compacts this rank's k1-mers into a table of their own (same
// bucket grid, so lookups work unchanged).  Everything after that is the unsharded algorithm on the small table.
__global__ void shard_select_kernel(const uint32_t* __restrict__ lab, const uint8_t* __restrict__ owner_root, uint64_t n, uint32_t my_rank,
                                    uint32_t* __restrict__ sel) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) sel[i] = owner_root[lab[i]] == my_rank ? 1u : 0u;
}
__global__ void shard_compact_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ sel,
                                     const uint64_t* __restrict__ pos, uint64_t n, uint64_t* __restrict__ okeys, uint32_t* __restrict__ ocounts) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && sel[i]) { okeys[pos[i]] = keys[i]; ocounts[pos[i]] = counts[i]; }
}
__global__ void shard_offsets_kernel(const uint64_t* __restrict__ boff, uint64_t n_buckets, const uint64_t* __restrict__ pos,
                                     uint64_t* __restrict__ oboff) {
  uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b <= n_buckets) oboff[b] = pos[boff[b]];        // pos has n+1 entries: pos[n] = number of selected k1-mers
}

int component_shard(shn_ctx* ctx, const shn_table* t, int world, int rank, shn_table** out) {
  hipStream_t s = ctx->stream; shn_use_stream(s);
  const uint64_t n = t->n;
  uint32_t* d_weight = nullptr; uint8_t* d_flags = nullptr;
  unsigned long long* lines = nullptr;
  uint64_t n_lines = 0;
  shn_table* sub = nullptr;
  auto cleanup = [&]() { if (d_weight) shn_dev_free(d_weight); if (d_flags) shn_dev_free(d_flags); if (lines) shn_dev_free(lines); };
#define TRYS(x) do { hipError_t _e = (x); if (_e != hipSuccess) { cleanup(); if (sub) shn_table_destroy(sub); \
      return shn_fail(SHN_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(_e)); } } while (0)
  TRYS(shn_dev_malloc(&d_weight, (n + 1) * 4));
  TRYS(shn_dev_malloc(&d_flags, n + 1));
  ext_prepare_launch(s, t, d_weight, d_flags);
  { int rca = build_fine_dict(ctx, t, d_flags, &lines, &n_lines); if (rca) { cleanup(); return rca; } }
  void *pl, *po, *pz, *pb, *pc, *pp;
  const uint32_t big_cap = 1u << 16;
  enum { CS_N_BIG = 20 };                                    // word of the counter block (workspace slot 13) that counts the large components
  int rc;
  if ((rc = shn_ws(ctx)[14].get((n + 1) * 4, &pl)) || (rc = shn_ws(ctx)[15].get(n + 1, &po)) || (rc = shn_ws(ctx)[16].get((n + 1) * 4, &pz)) ||
      (rc = shn_ws(ctx)[17].get((size_t)big_cap * 9 + 64, &pb)) || (rc = shn_ws(ctx)[13].get(2048, &pc)) || (rc = shn_ws(ctx)[9].get((2 * n + 2) * 8, &pp))) { cleanup(); return rc; }
  uint32_t* d_lab = (uint32_t*)pl; uint8_t* d_owner_root = (uint8_t*)po;
  uint32_t* d_size = (uint32_t*)pz;
  uint32_t* d_big_root = (uint32_t*)pb; uint32_t* d_big_size = d_big_root + big_cap; uint8_t* d_big_owner = (uint8_t*)(d_big_size + big_cap);
  unsigned long long* d_cnt = (unsigned long long*)pc;
  uint64_t* d_pos = (uint64_t*)pp;
  TRYS(hipMemsetAsync(d_cnt, 0, 2048, s));
  hipLaunchKernelGGL(cc_init_kernel, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, s, d_lab, n);
  { TimerRegion t1(ctx, T_EXT_PREP);
    hipLaunchKernelGGL(cc_edges_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(n * 8, 256), 1u << 22)), dim3(256), 0, s, shn_tab_idx(t),
                       d_flags, n, t->k, t->canonical, d_lab, (const unsigned long long*)lines, n_lines); }
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, s, d_lab, n);
  TRYS(hipMemsetAsync(d_size, 0, (n + 1) * 4, s));
  hipLaunchKernelGGL(cc_sample_kernel, dim3((uint32_t)cdiv(cdiv(n, 64), 256)), dim3(256), 0, s, d_lab, n, d_size);
  hipLaunchKernelGGL(cc_owner_kernel, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, s, d_lab, d_size, n, (uint32_t)world, d_owner_root,
                     d_big_root, d_big_size, d_cnt + CS_N_BIG, big_cap);
  unsigned long long nb = 0;
  TRYS(hipMemcpyAsync(&nb, d_cnt + CS_N_BIG, 8, hipMemcpyDeviceToHost, s));
  TRYS(hipStreamSynchronize(s));
  // more large components than the list holds: which ones got recorded depends on the arrival order of the atomics, i.e. could
  // differ from rank to rank -- every root then keeps its hash owner (the same on every rank), no balancing
  if (nb > big_cap) nb = 0;
  if (nb) {
    std::vector<uint32_t> br(nb), bs(nb);
    TRYS(hipMemcpyAsync(br.data(), d_big_root, nb * 4, hipMemcpyDeviceToHost, s));
    TRYS(hipMemcpyAsync(bs.data(), d_big_size, nb * 4, hipMemcpyDeviceToHost, s));
    TRYS(hipStreamSynchronize(s));
    std::vector<uint32_t> ord(nb);
    for (uint32_t j = 0; j < nb; j++) ord[j] = j;
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return bs[a] != bs[b] ? bs[a] > bs[b] : br[a] < br[b]; });
    std::vector<uint64_t> load(world, 0);
    std::vector<uint8_t> bo(nb);
    for (uint32_t j : ord) {                                  // largest first onto the least loaded rank
      int best = 0;
      for (int w = 1; w < world; w++) if (load[w] < load[best]) best = w;
      bo[j] = (uint8_t)best;
      load[best] += bs[j];
    }
    TRYS(hipMemcpyAsync(d_big_owner, bo.data(), nb, hipMemcpyHostToDevice, s));       // (bo lives until the synchronisation at the end of this function)
    hipLaunchKernelGGL(cc_assign_kernel, dim3((uint32_t)cdiv(nb, 256)), dim3(256), 0, s, d_big_root, d_big_owner, (uint32_t)nb, d_owner_root);
  }
  // this rank's k1-mers, in table order (bucket by bucket, ascending inside a bucket)
  uint32_t* d_sel = d_size;                                   // (the sampled sizes are done with)
  hipLaunchKernelGGL(shard_select_kernel, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, s, d_lab, d_owner_root, n, (uint32_t)rank, d_sel);
  uint64_t n_sub = 0;
  if ((rc = shn_device_scan_u32(ctx, d_sel, n, d_pos, &n_sub))) { cleanup(); return rc; }
  sub = new shn_table();
  memset(sub, 0, sizeof(*sub));
  sub->ctx = t->ctx; sub->device = t->device; sub->k = t->k; sub->canonical = t->canonical; sub->n = n_sub; sub->total = 0;
  sub->bits = t->bits; sub->n_buckets = t->n_buckets; sub->layout = t->layout; sub->sk_m = t->sk_m;
  TRYS(shn_dev_malloc(&sub->d_keys, (n_sub + 1) * 8));
  TRYS(shn_dev_malloc(&sub->d_counts, (n_sub + 1) * 4));
  TRYS(shn_dev_malloc(&sub->d_bucket_off, (t->n_buckets + 1) * 8));
  hipLaunchKernelGGL(shard_compact_kernel, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, s, t->d_keys, t->d_counts, d_sel, d_pos, n, sub->d_keys, sub->d_counts);
  hipLaunchKernelGGL(shard_offsets_kernel, dim3((uint32_t)cdiv(t->n_buckets + 1, 256)), dim3(256), 0, s, t->d_bucket_off, t->n_buckets, d_pos, sub->d_bucket_off);
  TRYS(hipStreamSynchronize(s));
  TRYS(hipGetLastError());
#undef TRYS
  cleanup();
  *out = sub;
  return SHN_OK;
}

// ---- Component labelling on OWNER SHARDS (the N-rank path without a replicated table: BASELINE configs[4]) ----
// component_shard above wants the whole table on every rank.  Here every rank holds only the k1-mers whose minimizer it owns
// (shn_table_shard_mode 1: most edges of the k1-mer graph stay inside a shard):
//   1. shn_cc_create:   the local components -- the union-find of cc_edges_kernel over the shard (an edge whose other end is not in
//                       the shard is simply not found);
//   2. shn_cc_queries:  every neighbour / sibling key of a local k1-mer that a HIGHER rank owns, with the local root of the asker
//                       (an edge is seen from both ends; the lower rank asks, so it is recorded once) -> all-to-all by owner;
//   3. shn_cc_answer:   the owner looks the keys up: present and not low-complexity = an edge between two local components of two
//                       ranks, as a pair of global ids (rank's base + local root);
//   4. shn_cc_solve:    the edges of all ranks (gathered) -> the components of the component graph, the same on every rank: sorted
//                       distinct ids + the smallest id of the component of each;
//   5. shn_cc_labels / shn_cc_owners / shn_cc_shard: a global label and an owner rank for every local k1-mer, and the shard's pairs
//                       grouped by owner -> all-to-all -> a table of whole components per rank, walked by the unsharded shn_extend
//                       (ids and records are those of the rank's own table: the 31-bit id limit applies to a rank, not to the job).
// The edge rule is cc_edges_kernel's, so the components are those of component_shard on the whole table (tests/test_cc_shards_gpu.py
// against scipy's connected components of the same graph).
struct shn_cc {
  shn_ctx* ctx; const shn_table* t; int world, rank, device;
  uint8_t* d_flags; uint32_t* d_lab;
  unsigned long long* d_cnt;          // 64 totals + 64 bases
  uint32_t* d_bc; uint64_t* d_pos;    // per (rank, block): how many entries the block has for the rank, and where they go (see cc_query_kernel)
  uint32_t q_grid;
  uint64_t per_rank[64];
};
#define CC_GRID 2048                  // blocks of the passes that group entries by rank (count pass and write pass have the same shape)

// key number `which` = 8 * half + p of the k1-mer str (see cc_edges_kernel): half 0 = its eight neighbours, half 1 = its siblings
__device__ __forceinline__ uint64_t cc_which_key(uint64_t str, int p, int half, int k, uint64_t mask, int canonical, bool* skip) {
  const uint64_t b = (uint64_t)(p & 3);
  uint64_t key;
  *skip = false;
  if (half == 0) key = (p & 4) ? ((str >> 2) | (b << (2 * (k - 1)))) : (((str << 2) | b) & mask);
  else if (p & 4) { *skip = (str & 3) == b; key = (str & ~3ULL) | b; }
  else { const int sh = 2 * (k - 1); *skip = ((str >> sh) & 3) == b; key = (str & ~(3ULL << sh)) | (b << sh); }
  if (canonical) { const uint64_t rc = shn_revcomp(key, k); if (rc < key) key = rc; }
  return key;
}

// WRITE = false: how many queries this block has for every rank (block_count[rank * blocks + block]; the totals into `total`);
// true: the queries, grouped by rank -- pos = the exclusive scan of block_count, an LDS cursor per rank inside the block.  The two
// passes have the same launch shape.  (One HBM cursor per rank, wave-aggregated, took 292 ms for 64 M queries: every wavefront of
// the launch on the same three addresses.)
template <bool WRITE>
__global__ void cc_query_kernel(const uint64_t* __restrict__ tkeys, const uint8_t* __restrict__ flags, uint64_t n, int k, int canonical,
                                int world, int rank, const uint32_t* __restrict__ lab, unsigned long long* __restrict__ total,
                                uint32_t* __restrict__ block_count, const uint64_t* __restrict__ pos,
                                uint64_t* __restrict__ qk, uint32_t* __restrict__ ql) {
  __shared__ uint32_t lh[64];
  __shared__ uint64_t lbase[64];
  if (threadIdx.x < 64) {
    lh[threadIdx.x] = 0;
    if (WRITE) lbase[threadIdx.x] = (int)threadIdx.x < world ? pos[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] : 0;
  }
  __syncthreads();
  const uint64_t mask = (k == 32) ? ~0ULL : ((1ULL << (2 * k)) - 1);
  const uint64_t total_items = n * 8;
  const int m = k < SHN_OWNER_M ? k : SHN_OWNER_M, w = k - m + 1;
  const uint32_t mmask = m == 16 ? 0xFFFFFFFFu : ((1u << (2 * m)) - 1u);
  SHN_GRID_FOR(gid, total_items) {
    const uint64_t i = gid >> 3;
    const int p = (int)(gid & 7);
    if (flags[i] & 2) continue;                                         // (the eight lanes of a k1-mer leave together)
    const uint64_t str = tkeys[i];
    // The minimizers of the sixteen keys from the k1-mer's own m-mers (as ext_records_kernel does for the neighbours): a successor
    // and a sibling with another last base share its m-mers 1 .. w - 1 resp. 0 .. w - 2 and have one m-mer of their own, a
    // predecessor and a sibling with another first base likewise -- 14 + 16 order values per k1-mer instead of 16 x 14 (the
    // two passes of this kernel took 0.4 s of the labelling's 0.9 s at 724 M k1-mers with the minimizers made from scratch).
    uint32_t smin = 0xFFFFFFFFu, pmin = 0xFFFFFFFFu;                    // over the k1-mer's m-mers 1 .. w - 1 / 0 .. w - 2
    for (int pos = p; pos < w; pos += 8) {
      const uint32_t fm = (uint32_t)(str >> (2 * (k - m - pos))) & mmask;
      uint32_t c = fm;
      if (canonical) { const uint32_t r = shn_revcomp32(fm, m); c = r < fm ? r : fm; }
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
    const uint32_t first_m = (uint32_t)(str >> (2 * (k - m))) & mmask, last_m = (uint32_t)str & mmask;
#pragma unroll
    for (int half = 0; half < 2; half++) {
      bool skip;
      const uint64_t key = cc_which_key(str, p, half, k, mask, canonical, &skip);
      if (skip) continue;
      // the key's own m-mer and which of the k1-mer's it shares
      uint32_t fm, shared;
      if (half == 0) {
        if (p & 4) { fm = (nb << (2 * (m - 1))) | (first_m >> 2); shared = pmin; }            // predecessor: new first m-mer + m-mers 0 .. w - 2
        else { fm = ((last_m & (mmask >> 2)) << 2) | nb; shared = smin; }                       // successor: m-mers 1 .. w - 1 + new last m-mer
      } else {
        if (p & 4) { fm = (last_m & ~3u) | nb; shared = pmin; }                                 // another last base: m-mers 0 .. w - 2 + its last m-mer
        else { fm = (first_m & (mmask >> 2)) | (nb << (2 * (m - 1))); shared = smin; }          // another first base: its first m-mer + m-mers 1 .. w - 1
      }
      uint32_t c = fm;
      if (canonical) { const uint32_t r = shn_revcomp32(fm, m); c = r < fm ? r : fm; }
      uint32_t o = shn_sk_order(c);
      o = shared < o ? shared : o;
      const int dest = (int)shn_owner_of_order(o, world);
      if (dest <= rank) continue;
      const uint32_t at = atomicAdd(&lh[dest], 1u);
      if (WRITE) { const uint64_t d = lbase[dest] + at; qk[d] = key; ql[d] = lab[i]; }
    }
  }
  if (!WRITE) {
    __syncthreads();
    if ((int)threadIdx.x < world) {
      block_count[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = lh[threadIdx.x];
      if (lh[threadIdx.x]) atomicAdd(&total[threadIdx.x], (unsigned long long)lh[threadIdx.x]);
    }
  }
}

// the queries received (grouped by asking rank: group s begins at src_off[s]) against this shard
__global__ void cc_answer_kernel(const TabIdx T, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ lab,
                                 const uint64_t* __restrict__ qk, const uint32_t* __restrict__ ql, uint64_t nq,
                                 const unsigned long long* __restrict__ src_off, const unsigned long long* __restrict__ base, int world, int rank,
                                 uint64_t* __restrict__ edges, unsigned long long* __restrict__ n_edges) {
  const int lane = threadIdx.x & 63;
  const uint64_t rounded = (nq + 63) & ~63ULL;
  SHN_GRID_FOR(q, rounded) {
    int64_t j = -1;
    if (q < nq) { j = shn_tab_find(T, qk[q]); if (j >= 0 && (flags[j] & 2)) j = -1; }
    const unsigned long long m = __ballot(j >= 0);
    if (!m) continue;
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long at = 0;
    if (lane == leader) at = atomicAdd(n_edges, (unsigned long long)__popcll(m));
    at = shfl_u64(at, leader);
    if (j >= 0) {
      int src = 0;
      while (src + 1 < world && q >= src_off[src + 1]) src++;
      const uint64_t d = at + __popcll(m & ((1ULL << lane) - 1));
      edges[2 * d] = base[rank] + lab[j];
      edges[2 * d + 1] = base[src] + ql[q];
    }
  }
}

extern "C" void shn_cc_destroy(shn_cc* c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->d_flags) shn_dev_free(c->d_flags);
  if (c->d_lab) shn_dev_free(c->d_lab);
  if (c->d_cnt) shn_dev_free(c->d_cnt);
  if (c->d_bc) shn_dev_free(c->d_bc);
  if (c->d_pos) shn_dev_free(c->d_pos);
  delete c;
}

// the local components of the shard `t` of rank `rank` of `world` (t must outlive the object) + the number of queries per rank
extern "C" int shn_cc_create(shn_ctx* ctx, const shn_table* t, int world, int rank, shn_cc** out) {
  if (!ctx || !t || !out || world < 1 || world > 64 || rank < 0 || rank >= world) return shn_fail(SHN_ERR_ARG, "shn_cc_create: bad argument");
  if (t->n >= 0x7FFFFFFFULL) return shn_fail(SHN_ERR_ARG, "shn_cc_create: a shard holds at most 2^31 - 1 k1-mers (use more ranks)");
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  const uint64_t n = t->n;
  shn_cc* c = new shn_cc();
  memset(c, 0, sizeof(*c));
  c->ctx = ctx; c->t = t; c->world = world; c->rank = rank; c->device = ctx->device;
  uint32_t* d_weight = nullptr;
  unsigned long long* lines = nullptr;
  uint64_t n_lines = 0;
  auto fail = [&](int rc) { if (d_weight) shn_dev_free(d_weight); if (lines) shn_dev_free(lines); shn_cc_destroy(c); return rc; };
#define TRYC(x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail(shn_fail(SHN_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(_e))); } while (0)
  TRYC(shn_dev_malloc(&d_weight, (n + 1) * 4));
  TRYC(shn_dev_malloc(&c->d_flags, n + 1));
  TRYC(shn_dev_malloc(&c->d_lab, (n + 1) * 4));
  TRYC(shn_dev_malloc(&c->d_cnt, 128 * 8));
  TRYC(shn_dev_malloc(&c->d_bc, (size_t)64 * CC_GRID * 4));
  TRYC(shn_dev_malloc(&c->d_pos, ((size_t)64 * CC_GRID + 2) * 8));
  TRYC(hipMemsetAsync(c->d_cnt, 0, 128 * 8, s));
  c->q_grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, cdiv(n * 8, 256)), CC_GRID);
  if (n) {
    ext_prepare_launch(s, t, d_weight, c->d_flags);
    { int rc = build_fine_dict(ctx, t, c->d_flags, &lines, &n_lines); if (rc) return fail(rc); }
    hipLaunchKernelGGL(cc_init_kernel, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, s, c->d_lab, n);
    hipLaunchKernelGGL(cc_edges_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(n * 8, 256), 1u << 22)), dim3(256), 0, s, shn_tab_idx(t),
                       c->d_flags, n, t->k, t->canonical, c->d_lab, (const unsigned long long*)lines, n_lines);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, s, c->d_lab, n);
    hipLaunchKernelGGL((cc_query_kernel<false>), dim3(c->q_grid), dim3(256), 0, s, t->d_keys, c->d_flags, n, t->k, t->canonical, world, rank, c->d_lab,
                       c->d_cnt, c->d_bc, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr);
    { int rc = shn_device_scan_u32(ctx, c->d_bc, (uint64_t)world * c->q_grid, c->d_pos, nullptr); if (rc) return fail(rc); }
  }
  unsigned long long h[64];
  TRYC(hipMemcpyAsync(h, c->d_cnt, 64 * 8, hipMemcpyDeviceToHost, s));
  TRYC(hipStreamSynchronize(s));
  TRYC(hipGetLastError());
  for (int r = 0; r < 64; r++) c->per_rank[r] = r < world ? h[r] : 0;
  shn_dev_free(d_weight); d_weight = nullptr;
  if (lines) { shn_dev_free(lines); lines = nullptr; }
#undef TRYC
  *out = c;
  return SHN_OK;
}

extern "C" int shn_cc_query_counts(const shn_cc* c, uint64_t* per_rank) {
  if (!c || !per_rank) return shn_fail(SHN_ERR_ARG, "shn_cc_query_counts: bad argument");
  for (int r = 0; r < c->world; r++) per_rank[r] = c->per_rank[r];
  return SHN_OK;
}

// the queries, grouped by destination rank in rank order (per_rank[r] entries each): key (8 bytes) and the asker's local root (4 bytes)
extern "C" int shn_cc_queries(shn_cc* c, void* dev_keys_out, void* dev_labs_out) {
  if (!c) return shn_fail(SHN_ERR_ARG, "shn_cc_queries: bad argument");
  shn_ctx* ctx = c->ctx;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  unsigned long long a = 0;
  for (int r = 0; r < 64; r++) a += c->per_rank[r];
  if (!a) return SHN_OK;
  if (!dev_keys_out || !dev_labs_out) return shn_fail(SHN_ERR_ARG, "shn_cc_queries: NULL output");
  const uint64_t n = c->t->n;
  hipLaunchKernelGGL((cc_query_kernel<true>), dim3(c->q_grid), dim3(256), 0, s, c->t->d_keys, c->d_flags, n, c->t->k, c->t->canonical, c->world, c->rank,
                     c->d_lab, c->d_cnt, c->d_bc, (const uint64_t*)c->d_pos, (uint64_t*)dev_keys_out, (uint32_t*)dev_labs_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return SHN_OK;
}

// recv_per_rank[s]: queries received from rank s (grouped in rank order); base[r]: first global id of rank r (the ranks' shard sizes,
// summed); dev_edges_out: room for 2 ids per query.  n_edges: how many of the queries named a k1-mer of this shard.
extern "C" int shn_cc_answer(shn_cc* c, const void* dev_keys, const void* dev_labs, const uint64_t* recv_per_rank, const uint64_t* base,
                             void* dev_edges_out, uint64_t* n_edges) {
  if (!c || !recv_per_rank || !base || !n_edges) return shn_fail(SHN_ERR_ARG, "shn_cc_answer: bad argument");
  shn_ctx* ctx = c->ctx;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  unsigned long long h[128], a = 0;
  for (int r = 0; r < 64; r++) { h[r] = a; if (r < c->world) a += recv_per_rank[r]; h[64 + r] = r < c->world ? base[r] : 0; }
  *n_edges = 0;
  if (!a) return SHN_OK;
  if (!dev_keys || !dev_labs || !dev_edges_out) return shn_fail(SHN_ERR_ARG, "shn_cc_answer: NULL buffer");
  unsigned long long* d_ne = nullptr;
  HIP_TRY(shn_dev_malloc(&d_ne, 8));
  hipError_t e = hipMemcpyAsync(c->d_cnt, h, 128 * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(d_ne, 0, 8, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(cc_answer_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(a, 256), 1u << 20)), dim3(256), 0, s, shn_tab_idx(c->t), c->d_flags, c->d_lab,
                       (const uint64_t*)dev_keys, (const uint32_t*)dev_labs, (uint64_t)a, c->d_cnt, c->d_cnt + 64, c->world, c->rank,
                       (uint64_t*)dev_edges_out, d_ne);
    e = hipGetLastError();
  }
  unsigned long long ne = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&ne, d_ne, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  shn_dev_free(d_ne);
  if (e != hipSuccess) return shn_fail(SHN_ERR_HIP, std::string("shn_cc_answer: ") + hipGetErrorString(e));
  *n_edges = ne;
  return SHN_OK;
}

// ---- the component graph (nodes = local components that have an edge to another rank), the same computation on every rank
__global__ void ccs_iota_kernel(uint32_t* __restrict__ v, uint64_t n) {
  SHN_GRID_FOR(i, n) v[i] = (uint32_t)i;
}
// first, pos: the runs of the sorted ids (runs.h); a run is a node, its number the run index
__global__ void ccs_number_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ first,
                                  const uint64_t* __restrict__ pos, uint64_t n, uint32_t* __restrict__ node_of_end, uint64_t* __restrict__ nodes,
                                  uint32_t* __restrict__ lab) {
  SHN_GRID_FOR(i, n) {
    const uint32_t id = (uint32_t)shn_run_index(first, pos, i);
    node_of_end[vals[i]] = id;
    if (first[i]) { nodes[id] = keys[i]; lab[id] = id; }
  }
}
__global__ void ccs_unite_kernel(const uint32_t* __restrict__ node_of_end, uint64_t n_edges, uint32_t* lab) {
  SHN_GRID_FOR(e, n_edges)
    cc_unite(lab, node_of_end[2 * e], node_of_end[2 * e + 1]);
}
__global__ void ccs_label_kernel(uint32_t* lab, const uint64_t* __restrict__ nodes, uint64_t n_nodes, uint64_t* __restrict__ label_out) {
  SHN_GRID_FOR(i, n_nodes)
    label_out[i] = nodes[cc_find(lab, (uint32_t)i)];
}

// dev_edges: n_edges pairs of global ids (not modified).  dev_nodes_out / dev_labels_out: room for 2 n_edges ids each: the distinct
// ids, ascending, and for each the smallest id of its component (roots only ever link to smaller node numbers, node numbers follow
// the ids: the answer does not depend on the order of the edges).
// id_limit: every id is below it (0: unknown) -- the sort goes over its bits only.
extern "C" int shn_cc_solve(shn_ctx* ctx, const void* dev_edges, uint64_t n_edges, uint64_t id_limit, void* dev_nodes_out, void* dev_labels_out, uint64_t* n_nodes) {
  if (!ctx || !n_nodes) return shn_fail(SHN_ERR_ARG, "shn_cc_solve: bad argument");
  *n_nodes = 0;
  if (!n_edges) return SHN_OK;
  if (!dev_edges || !dev_nodes_out || !dev_labels_out) return shn_fail(SHN_ERR_ARG, "shn_cc_solve: NULL buffer");
  const uint64_t m = 2 * n_edges;
  if (m >= 0xFFFFFFF0ULL) return shn_fail(SHN_ERR_ARG, "shn_cc_solve: more than 2^31 edges between the shards");
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  ShnDevBufs bufs(s);
  uint64_t *k0, *k1; uint32_t *v0, *v1, *node_of_end, *lab;
  auto no = [](hipError_t e) { return e != hipSuccess; };
  if (no(bufs.get(&k0, m * 8)) || no(bufs.get(&k1, m * 8)) || no(bufs.get(&v0, m * 4)) || no(bufs.get(&v1, m * 4)) ||
      no(bufs.get(&node_of_end, m * 4)) || no(bufs.get(&lab, m * 4)))
    return shn_fail(SHN_ERR_HIP, "shn_cc_solve: out of device memory");
  const uint32_t grid = (uint32_t)std::min<uint64_t>(cdiv(m, 256), 1u << 20);
  HIP_TRY(hipMemcpyAsync(k0, dev_edges, m * 8, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(ccs_iota_kernel, dim3(grid), dim3(256), 0, s, v0, m);
  int bit_hi = 64;
  if (id_limit) { bit_hi = 8; while (bit_hi < 64 && (id_limit >> bit_hi)) bit_hi += 8; }
  int rc = shn_sort_pairs(ctx, k0, v0, k1, v1, m, 0, bit_hi);
  if (rc) return rc;
  ShnRuns runs;
  if ((rc = shn_sorted_runs(ctx, bufs, k0, m, 0, 0, &runs))) return rc;
  const uint64_t nn = runs.n_runs;
  hipLaunchKernelGGL(ccs_number_kernel, dim3(grid), dim3(256), 0, s, k0, v0, runs.head, runs.pos, m, node_of_end, (uint64_t*)dev_nodes_out, lab);
  hipLaunchKernelGGL(ccs_unite_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(n_edges, 256), 1u << 20)), dim3(256), 0, s, node_of_end, n_edges, lab);
  hipLaunchKernelGGL(ccs_label_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(nn, 256), 1u << 20)), dim3(256), 0, s, lab, (const uint64_t*)dev_nodes_out, nn,
                     (uint64_t*)dev_labels_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  *n_nodes = nn;
  return SHN_OK;
}

__device__ __forceinline__ int64_t ccs_search(const uint64_t* __restrict__ a, uint64_t n, uint64_t key) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; const uint64_t v = a[mid]; if (v == key) return (int64_t)mid; if (v < key) lo = mid + 1; else hi = mid; }
  return -1;
}
__global__ void ccs_glabel_kernel(const uint32_t* __restrict__ lab, uint64_t n, uint64_t base_me, const uint64_t* __restrict__ nodes,
                                  const uint64_t* __restrict__ labels, uint64_t n_nodes, uint64_t* __restrict__ out) {
  SHN_GRID_FOR(i, n) {
    const uint64_t g = base_me + lab[i];
    const int64_t j = ccs_search(nodes, n_nodes, g);
    out[i] = j >= 0 ? labels[j] : g;
  }
}
// the global label of every k1-mer of the shard (table order): the solved label of its local component if that has an edge to
// another rank, its own global id otherwise
extern "C" int shn_cc_labels(shn_cc* c, uint64_t base_me, const void* dev_nodes, const void* dev_labels, uint64_t n_nodes, void* dev_glabel_out) {
  if (!c) return shn_fail(SHN_ERR_ARG, "shn_cc_labels: bad argument");
  const uint64_t n = c->t->n;
  if (!n) return SHN_OK;
  if (!dev_glabel_out || (n_nodes && (!dev_nodes || !dev_labels))) return shn_fail(SHN_ERR_ARG, "shn_cc_labels: NULL buffer");
  shn_ctx* ctx = c->ctx;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  hipLaunchKernelGGL(ccs_glabel_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(n, 256), 1u << 20)), dim3(256), 0, s, c->d_lab, n, base_me,
                     (const uint64_t*)dev_nodes, (const uint64_t*)dev_labels, n_nodes, (uint64_t*)dev_glabel_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return SHN_OK;
}

__global__ void ccs_owner_kernel(const uint64_t* __restrict__ glabel, uint64_t n, const uint64_t* __restrict__ big, const uint8_t* __restrict__ big_owner,
                                 uint64_t n_big, uint32_t world, uint8_t* __restrict__ owner) {
  SHN_GRID_FOR(i, n) {
    const uint64_t g = glabel[i];
    const int64_t j = ccs_search(big, n_big, g);
    owner[i] = j >= 0 ? big_owner[j] : (uint8_t)(shn_mix64(g ^ 0x5851F42D4C957F2DULL) % world);
  }
}
// owner rank of every k1-mer of the shard: its component's -- by the hash of the label, except for the components listed (dev_big:
// n_big labels ascending, dev_big_owner: their ranks), which the caller has balanced by size
extern "C" int shn_cc_owners(shn_cc* c, const void* dev_glabel, const void* dev_big, const void* dev_big_owner, uint64_t n_big, void* dev_owner_out) {
  if (!c) return shn_fail(SHN_ERR_ARG, "shn_cc_owners: bad argument");
  const uint64_t n = c->t->n;
  if (!n) return SHN_OK;
  if (!dev_glabel || !dev_owner_out || (n_big && (!dev_big || !dev_big_owner))) return shn_fail(SHN_ERR_ARG, "shn_cc_owners: NULL buffer");
  shn_ctx* ctx = c->ctx;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  hipLaunchKernelGGL(ccs_owner_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(n, 256), 1u << 20)), dim3(256), 0, s, (const uint64_t*)dev_glabel, n,
                     (const uint64_t*)dev_big, (const uint8_t*)dev_big_owner, n_big, (uint32_t)c->world, (uint8_t*)dev_owner_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return SHN_OK;
}

template <bool WRITE>
__global__ void ccs_shard_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts, const uint8_t* __restrict__ owner, uint64_t n,
                                 int world, unsigned long long* __restrict__ total, uint32_t* __restrict__ block_count, const uint64_t* __restrict__ pos,
                                 uint64_t* __restrict__ ok, uint32_t* __restrict__ oc) {
  __shared__ uint32_t lh[64];
  __shared__ uint64_t lbase[64];
  if (threadIdx.x < 64) {
    lh[threadIdx.x] = 0;
    if (WRITE) lbase[threadIdx.x] = (int)threadIdx.x < world ? pos[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] : 0;
  }
  __syncthreads();
  SHN_GRID_FOR(i, n) {
    const int o = (int)owner[i];
    const uint32_t at = atomicAdd(&lh[o], 1u);
    if (WRITE) { const uint64_t d = lbase[o] + at; ok[d] = keys[i]; oc[d] = counts[i]; }
  }
  if (!WRITE) {
    __syncthreads();
    if ((int)threadIdx.x < world) {
      block_count[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = lh[threadIdx.x];
      if (lh[threadIdx.x]) atomicAdd(&total[threadIdx.x], (unsigned long long)lh[threadIdx.x]);
    }
  }
}
// the shard's (key, count) pairs grouped by owner rank (per_rank[r] pairs each, rank order) -- what the all-to-all sends
extern "C" int shn_cc_shard(shn_cc* c, const void* dev_owner, uint64_t* per_rank, void* dev_keys_out, void* dev_counts_out) {
  if (!c || !per_rank) return shn_fail(SHN_ERR_ARG, "shn_cc_shard: bad argument");
  const uint64_t n = c->t->n;
  for (int r = 0; r < c->world; r++) per_rank[r] = 0;
  if (!n) return SHN_OK;
  if (!dev_owner || !dev_keys_out || !dev_counts_out) return shn_fail(SHN_ERR_ARG, "shn_cc_shard: NULL buffer");
  shn_ctx* ctx = c->ctx;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream; shn_use_stream(s);
  const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, cdiv(n, 256)), CC_GRID);
  HIP_TRY(hipMemsetAsync(c->d_cnt, 0, 64 * 8, s));
  hipLaunchKernelGGL((ccs_shard_kernel<false>), dim3(grid), dim3(256), 0, s, c->t->d_keys, c->t->d_counts, (const uint8_t*)dev_owner, n, c->world, c->d_cnt,
                     c->d_bc, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr);
  int rc = shn_device_scan_u32(ctx, c->d_bc, (uint64_t)c->world * grid, c->d_pos, nullptr);
  if (rc) return rc;
  unsigned long long h[64];
  HIP_TRY(hipMemcpyAsync(h, c->d_cnt, 64 * 8, hipMemcpyDeviceToHost, s));
  hipLaunchKernelGGL((ccs_shard_kernel<true>), dim3(grid), dim3(256), 0, s, c->t->d_keys, c->t->d_counts, (const uint8_t*)dev_owner, n, c->world, c->d_cnt,
                     c->d_bc, (const uint64_t*)c->d_pos, (uint64_t*)dev_keys_out, (uint32_t*)dev_counts_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  for (int r = 0; r < c->world; r++) per_rank[r] = h[r];
  return SHN_OK;
}
