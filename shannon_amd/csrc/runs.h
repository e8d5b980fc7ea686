// What a stage does right after the library's sort, once: the runs of equal keys of a sorted array, the search of an offset array
// for the segment that holds an element, and the grid-stride loop with its grid size.
//
//   shn_sorted_runs      head[i] = (i == 0 || keys[i] >> shift != keys[i - 1] >> shift), then shn_runs_from_heads
//   shn_runs_from_heads  pos = the exclusive scan of head (shn_device_scan_u32, whose host total n_runs is the ONE synchronisation),
//                        then one scatter kernel for what `want` names -- keys[r] = the first key of run r, start[r] = its first
//                        element with the sentinel start[n_runs] = n -- and, for the lengths, one more kernel over n_runs.  Nothing
//                        wanted: head and pos alone, no kernel behind the scan (run of element i: shn_run_index).
// The buffers come from the caller's ShnDevBufs and live as long as it does; the work runs on ctx->stream inside whatever
// TimerRegion the caller has open, and the byte model stays the caller's.  n == 0: n_runs = 0, nothing is launched, pos[0] = 0 and
// (where wanted) start[0] = 0 still hold.  n >= 2^32: SHN_ERR_OVERFLOW (starts and lengths are 32 bits wide).
//
// The searches, shn_run_index, SHN_GRID_FOR, shn_grid and shn_bits_for are plain C++ behind the qualifier of record_expand.h: hipcc
// compiles them into the kernels, any C++ compiler into tools/probes/runs_host_check.cpp, which runs the searches under sanitizers
// on arrays of exactly their sizes.
//
// Copies of the offset search that stay where they are, on purpose: core.hip (pack_kernel), kpaths_gpu.hip, post_gpu.hip,
// record_expand.h (record_of: a search between two bounds), contig_gpu.hip (a strided variant) and seeds.hip (the lower bound); so
// does everything in count*.hip, extend.hip and contig_gpu.hip.  Those kernels are on the benchmarked step and their register
// counts have been fought over: they change only with a measurement of their own.
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#ifndef SHN_XHD
#ifdef __HIPCC__
#define SHN_XHD __host__ __device__ __forceinline__
#else
#define SHN_XHD inline
#endif
#endif

// segment that holds element g: the largest j in [0, n) with off[j] <= g (n >= 1, off[0] <= g; an empty segment holds nothing: it
// shares its offset with the next one, which wins).  off[n] is never read.
SHN_XHD uint64_t shn_segment_of(const uint64_t* off, uint64_t n, uint64_t g) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] <= g) lo = mid; else hi = mid; }
  return lo;
}
// the first i in [0, n] with keys[i] >= key (n: every key is smaller)
SHN_XHD uint64_t shn_lower_bound(const uint64_t* keys, uint64_t n, uint64_t key) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}
// run of element i (head, pos: ShnRuns'): pos[i] counts the heads before i, so a head names its own run and any other element the
// run of the last head before it
SHN_XHD uint64_t shn_run_index(const uint32_t* head, const uint64_t* pos, uint64_t i) { return pos[i] - (head[i] ? 0 : 1); }

#define SHN_GRID_FOR(i, n) for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (uint64_t)gridDim.x * blockDim.x)
// blocks of a SHN_GRID_FOR launch over n elements: one at the least, 2^20 at the most
static inline uint32_t shn_grid(uint64_t n, uint32_t block) {
  const uint64_t b = (n + block - 1) / block;
  return (uint32_t)(b < 1 ? 1 : b > (1u << 20) ? (1u << 20) : b);
}
// bits that hold 0 .. n - 1: the smallest b >= 1 with n <= 2^b (n <= 1: 1; 63 at the most)
static inline int shn_bits_for(uint64_t n) {
  int b = 1;
  while (b < 63 && ((n ? n - 1 : 0) >> b)) b++;
  return b;
}

#ifdef __HIPCC__
#include "common.h"

enum { SHN_RUNS_KEYS = 1, SHN_RUNS_START = 2, SHN_RUNS_LEN = 4 };      // (the lengths are made from the starts: LEN gives both)
struct ShnRuns {
  uint64_t n_runs = 0;
  const uint32_t* head = nullptr;     // n flags (shn_runs_from_heads: the caller's own)
  const uint64_t* pos = nullptr;      // n + 1: the exclusive scan of head, pos[n] = n_runs
  const uint64_t* keys = nullptr;     // SHN_RUNS_KEYS: n_runs, the first key of every run, whole (not shifted)
  const uint32_t* start = nullptr;    // SHN_RUNS_START: n_runs + 1, start[n_runs] = n
  const uint32_t* len = nullptr;      // SHN_RUNS_LEN: n_runs
};
int shn_runs_from_heads(shn_ctx* ctx, ShnDevBufs& bufs, const uint32_t* d_head, uint64_t n, const uint64_t* d_keys /* NULL: no SHN_RUNS_KEYS */,
                        int want, ShnRuns* out);
int shn_sorted_runs(shn_ctx* ctx, ShnDevBufs& bufs, const uint64_t* d_keys, uint64_t n, int shift, int want, ShnRuns* out);
#endif
