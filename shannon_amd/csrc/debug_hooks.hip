// Test hooks of the shared device primitives (tests/test_primitives_gpu.py): the radix sort (sort.hip), the scan (count.hip), the runs
// of a sorted array (runs.hip) and the three bucket searches of common.h, each called unchanged on host arrays staged into buffers of the caching allocator on the
// context's stream.  Not part of the path.
#include "common.h"
#include "runs.h"

static bool bad_range(int bit_lo, int bit_hi) { return bit_lo < 0 || bit_hi < 0 || bit_lo > 64 || bit_hi > 64; }

extern "C" int shn_debug_sort_pairs(shn_ctx* ctx, const uint64_t* keys, const uint32_t* vals, uint64_t n, int bit_lo, int bit_hi,
                                    uint64_t* keys_out, uint32_t* vals_out) {
  if (!ctx || (n && (!keys || !vals || !keys_out || !vals_out))) return shn_fail(SHN_ERR_ARG, "shn_debug_sort_pairs: NULL argument");
  if (bad_range(bit_lo, bit_hi)) return shn_fail(SHN_ERR_ARG, "shn_debug_sort_pairs: bit range outside [0, 64]");
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);                          // (the sort's histogram lies in a stage workspace)
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  uint64_t *dk = nullptr, *dk2 = nullptr; uint32_t *dv = nullptr, *dv2 = nullptr;
  HIP_TRY(bufs.get(&dk, (n + 1) * 8)); HIP_TRY(bufs.get(&dk2, (n + 1) * 8));
  HIP_TRY(bufs.get(&dv, (n + 1) * 4)); HIP_TRY(bufs.get(&dv2, (n + 1) * 4));
  if (n) {
    HIP_TRY(hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(dv, vals, n * 4, hipMemcpyHostToDevice, s));
  }
  int rc = shn_sort_pairs(ctx, dk, dv, dk2, dv2, n, bit_lo, bit_hi);
  if (rc) return rc;
  if (n) {
    HIP_TRY(hipMemcpyAsync(keys_out, dk, n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(vals_out, dv, n * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return SHN_OK;
}

extern "C" int shn_debug_sort_keys(shn_ctx* ctx, const uint64_t* keys, uint64_t n, int bit_lo, int bit_hi, uint64_t* keys_out) {
  if (!ctx || (n && (!keys || !keys_out))) return shn_fail(SHN_ERR_ARG, "shn_debug_sort_keys: NULL argument");
  if (bad_range(bit_lo, bit_hi)) return shn_fail(SHN_ERR_ARG, "shn_debug_sort_keys: bit range outside [0, 64]");
  SHN_ENTER(ctx);
  shn_stage_begin(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  uint64_t *dk = nullptr, *dk2 = nullptr, *sorted = nullptr;
  HIP_TRY(bufs.get(&dk, (n + 1) * 8)); HIP_TRY(bufs.get(&dk2, (n + 1) * 8));
  if (n) HIP_TRY(hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, s));
  int rc = shn_sort_keys(ctx, dk, dk2, n, bit_lo, bit_hi, &sorted);
  if (rc) return rc;
  if (sorted != dk && sorted != dk2) return shn_fail(SHN_ERR_INTERNAL, "shn_debug_sort_keys: *sorted names neither buffer");
  if (n) HIP_TRY(hipMemcpyAsync(keys_out, sorted, n * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return SHN_OK;
}

extern "C" int shn_debug_scan_u32(shn_ctx* ctx, const uint32_t* in, uint64_t n, uint64_t* out /* n + 1 */, uint64_t* total /* may be NULL */) {
  if (!ctx || !out || (n && !in)) return shn_fail(SHN_ERR_ARG, "shn_debug_scan_u32: NULL argument");
  if (n >= 0xFFFFFFFFULL) return shn_fail(SHN_ERR_ARG, "shn_debug_scan_u32: n too large");
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  uint32_t* di = nullptr; uint64_t* dout = nullptr;
  HIP_TRY(bufs.get(&di, (n + 1) * 4)); HIP_TRY(bufs.get(&dout, (n + 2) * 8));
  if (n) HIP_TRY(hipMemcpyAsync(di, in, n * 4, hipMemcpyHostToDevice, s));
  int rc = shn_device_scan_u32(ctx, di, n, dout, total);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, dout, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return SHN_OK;
}

// everything shn_sorted_runs gives, of keys the caller has sorted by (key >> shift): keys_out / len_out take n_runs (n at the most),
// start_out n_runs + 1, pos_out n + 1 elements
extern "C" int shn_debug_sorted_runs(shn_ctx* ctx, const uint64_t* keys, uint64_t n, int shift, uint64_t* keys_out, uint32_t* start_out, uint32_t* len_out,
                                     uint64_t* pos_out, uint64_t* n_runs_out) {
  if (!ctx || !start_out || !pos_out || !n_runs_out || (n && (!keys || !keys_out || !len_out))) return shn_fail(SHN_ERR_ARG, "shn_debug_sorted_runs: NULL argument");
  if (shift < 0 || shift > 63) return shn_fail(SHN_ERR_ARG, "shn_debug_sorted_runs: shift outside 0 .. 63");
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  uint64_t* dk = nullptr;
  HIP_TRY(bufs.get(&dk, (n + 1) * 8));
  if (n) HIP_TRY(hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, s));
  ShnRuns r;
  int rc = shn_sorted_runs(ctx, bufs, dk, n, shift, SHN_RUNS_KEYS | SHN_RUNS_START | SHN_RUNS_LEN, &r);
  if (rc) return rc;
  if (r.n_runs > n) return shn_fail(SHN_ERR_INTERNAL, "shn_debug_sorted_runs: more runs than keys");
  if (r.n_runs) {
    HIP_TRY(hipMemcpyAsync(keys_out, r.keys, r.n_runs * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(len_out, r.len, r.n_runs * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipMemcpyAsync(start_out, r.start, (r.n_runs + 1) * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(pos_out, r.pos, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n_runs_out = r.n_runs;
  return SHN_OK;
}

// one thread per query: the index of the key in the table's key array (the order of shn_table_download) or -1
__global__ void debug_find_kernel(TabIdx T, const uint64_t* __restrict__ q, uint64_t n, int variant, int64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = q[i];
  out[i] = variant == 0 ? shn_table_find(T.keys, T.boff, T.bits, key)
         : variant == 1 ? shn_table_find_k(T.keys, T.boff, T.bits, key, 2 * T.k)
                        : shn_tab_find(T, key);
}

extern "C" int shn_debug_table_find(shn_ctx* ctx, const shn_table* t, const uint64_t* keys, uint64_t n, int variant, int64_t* idx_out) {
  if (!ctx || !t || (n && (!keys || !idx_out))) return shn_fail(SHN_ERR_ARG, "shn_debug_table_find: NULL argument");
  if (variant < 0 || variant > 2) return shn_fail(SHN_ERR_ARG, "shn_debug_table_find: variant 0 (shn_table_find), 1 (shn_table_find_k) or 2 (shn_tab_find)");
  if (t->layout != 0 && variant != 2) return shn_fail(SHN_ERR_ARG, "shn_debug_table_find: a table of layout 1 is searched by shn_tab_find alone");
  if (n >= 0xFFFFFFFFULL) return shn_fail(SHN_ERR_ARG, "shn_debug_table_find: n too large");
  if (!n) return SHN_OK;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  uint64_t* dq = nullptr; int64_t* di = nullptr;
  HIP_TRY(bufs.get(&dq, n * 8)); HIP_TRY(bufs.get(&di, n * 8));
  HIP_TRY(hipMemcpyAsync(dq, keys, n * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(debug_find_kernel, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, s, shn_tab_idx(t), (const uint64_t*)dq, n, variant, di);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(idx_out, di, n * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return SHN_OK;
}

extern "C" int shn_debug_table_view(shn_ctx* ctx, const shn_table* t, int* bits, int* layout, uint64_t* bucket_off /* 2^bits + 1, may be NULL */) {
  if (!ctx || !t) return shn_fail(SHN_ERR_ARG, "shn_debug_table_view: NULL argument");
  SHN_ENTER(ctx);
  if (bits) *bits = t->bits;
  if (layout) *layout = t->layout;
  if (bucket_off) {
    HIP_TRY(hipMemcpyAsync(bucket_off, t->d_bucket_off, (t->n_buckets + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  return SHN_OK;
}
