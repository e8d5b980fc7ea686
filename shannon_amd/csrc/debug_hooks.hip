// Test hooks of the shared device primitives (tests/test_primitives_gpu.py): the radix sort (sort.hip), the scan (count.hip) and the
// three bucket searches of common.h, each called unchanged on host arrays staged into buffers of the caching allocator on the
// context's stream.  Not part of the path.
#include "common.h"

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
