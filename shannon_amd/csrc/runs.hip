// The runs of equal keys of a sorted array (runs.h says what the two calls give and what they cost).
#include "runs.h"

namespace {

constexpr int RUNS_BLK = 256;

__global__ void runs_heads_kernel(const uint64_t* __restrict__ keys, uint64_t n, int shift, uint32_t* __restrict__ head) {
  SHN_GRID_FOR(i, n) head[i] = (i == 0 || (keys[i] >> shift) != (keys[i - 1] >> shift)) ? 1u : 0u;
}
// rkeys / start: nullptr where not wanted; element 0 writes the sentinel
__global__ void runs_scatter_kernel(const uint32_t* __restrict__ head, const uint64_t* __restrict__ pos, const uint64_t* __restrict__ keys, uint64_t n,
                                    uint64_t n_runs, uint64_t* __restrict__ rkeys, uint32_t* __restrict__ start) {
  SHN_GRID_FOR(i, n) {
    if (head[i]) {
      const uint64_t r = pos[i];
      if (rkeys) rkeys[r] = keys[i];
      if (start) start[r] = (uint32_t)i;
    }
    if (i == 0 && start) start[n_runs] = (uint32_t)n;
  }
}
__global__ void runs_len_kernel(const uint32_t* __restrict__ start, uint64_t n_runs, uint32_t* __restrict__ len) {
  SHN_GRID_FOR(r, n_runs) len[r] = start[r + 1] - start[r];
}

}  // namespace

int shn_runs_from_heads(shn_ctx* ctx, ShnDevBufs& bufs, const uint32_t* d_head, uint64_t n, const uint64_t* d_keys, int want, ShnRuns* out) {
  if (n >> 32) return shn_fail(SHN_ERR_OVERFLOW, "shn_runs_from_heads: 2^32 elements or more (" + std::to_string(n) + ")");
  if ((want & SHN_RUNS_KEYS) && n && !d_keys) return shn_fail(SHN_ERR_INTERNAL, "shn_runs_from_heads: the runs' keys wanted of no keys");
  if (want & SHN_RUNS_LEN) want |= SHN_RUNS_START;
  hipStream_t s = ctx->stream;
  uint64_t* d_pos = nullptr; uint64_t* d_rkeys = nullptr; uint32_t *d_start = nullptr, *d_len = nullptr;
  uint64_t n_runs = 0;
  HIP_TRY(bufs.get(&d_pos, (n + 2) * 8));
  if (n) {
    int rc = shn_device_scan_u32(ctx, d_head, n, d_pos, &n_runs);
    if (rc) return rc;
  } else HIP_TRY(hipMemsetAsync(d_pos, 0, 8, s));
  if (want & SHN_RUNS_KEYS) HIP_TRY(bufs.get(&d_rkeys, (n_runs + 1) * 8));
  if (want & SHN_RUNS_START) HIP_TRY(bufs.get(&d_start, (n_runs + 1) * 4));
  if (want & SHN_RUNS_LEN) HIP_TRY(bufs.get(&d_len, (n_runs + 1) * 4));
  if (n) {
    if (want & (SHN_RUNS_KEYS | SHN_RUNS_START))
      hipLaunchKernelGGL(runs_scatter_kernel, dim3(shn_grid(n, RUNS_BLK)), dim3(RUNS_BLK), 0, s, d_head, (const uint64_t*)d_pos, d_keys, n, n_runs, d_rkeys, d_start);
    if (want & SHN_RUNS_LEN)
      hipLaunchKernelGGL(runs_len_kernel, dim3(shn_grid(n_runs, RUNS_BLK)), dim3(RUNS_BLK), 0, s, (const uint32_t*)d_start, n_runs, d_len);
    HIP_TRY(hipGetLastError());
  } else if (d_start) HIP_TRY(hipMemsetAsync(d_start, 0, 4, s));
  out->n_runs = n_runs; out->head = d_head; out->pos = d_pos; out->keys = d_rkeys; out->start = d_start; out->len = d_len;
  return SHN_OK;
}

int shn_sorted_runs(shn_ctx* ctx, ShnDevBufs& bufs, const uint64_t* d_keys, uint64_t n, int shift, int want, ShnRuns* out) {
  if (n >> 32) return shn_fail(SHN_ERR_OVERFLOW, "shn_sorted_runs: 2^32 keys or more (" + std::to_string(n) + ")");
  if (shift < 0 || shift > 63) return shn_fail(SHN_ERR_INTERNAL, "shn_sorted_runs: shift outside 0 .. 63");
  uint32_t* d_head = nullptr;
  HIP_TRY(bufs.get(&d_head, (n + 1) * 4));
  if (n) hipLaunchKernelGGL(runs_heads_kernel, dim3(shn_grid(n, RUNS_BLK)), dim3(RUNS_BLK), 0, ctx->stream, d_keys, n, shift, d_head);
  return shn_runs_from_heads(ctx, bufs, d_head, n, d_keys, want, out);
}
