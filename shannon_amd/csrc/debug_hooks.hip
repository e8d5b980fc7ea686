// Test hooks of the shared device primitives (tests/test_primitives_gpu.py): the radix sort (sort.hip), the scan (count.hip), the runs
// of a sorted array (runs.hip) and the three bucket searches of common.h, each called unchanged on host arrays staged into buffers of the caching allocator on the
// context's stream; and of the one-line dictionary of the extension set-up (k1dict.hip, tests/test_ext_setup_gpu.py).  Not part of the path.
#include "common.h"
#include "runs.h"
#include "k1dict.h"
#include <vector>

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

// ---- the one-line dictionary (k1dict.h).  Eight lanes per query, as in ext_records_kernel: the group fetches the key's home line,
// 16 bytes a lane, and matches it with fd_match; a partial last group of eight runs as a whole wavefront of key 0.
__global__ void debug_fd_query_kernel(const TabIdx T, const uint8_t* __restrict__ flags, const uint64_t* __restrict__ q, uint64_t n,
                                      const unsigned long long* __restrict__ lines, uint64_t n_lines, uint32_t* __restrict__ id_out,
                                      uint64_t* __restrict__ home_out) {
  const uint64_t total = n * 8, rounded = (total + 63) & ~63ULL;
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= rounded) return;                                          // (whole wavefronts)
  const int lane = threadIdx.x & 63, g0 = lane & ~7, p = lane & 7;
  const bool in = gid < total;
  const uint64_t key = in ? q[gid >> 3] : 0ULL;
  const uint64_t line = fd_bucket(T, key, n_lines);
  const ulonglong2 v = ((const ulonglong2*)(lines + line * 16))[p];
  const uint32_t w = fd_match(v, lines, line, key, p, g0, T, flags);
  if (in && p == 0) { id_out[gid >> 3] = w; home_out[gid >> 3] = line; }
}
__global__ void debug_fd_home_kernel(const TabIdx T, uint64_t n, uint64_t n_lines, uint64_t* __restrict__ home_out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) home_out[i] = fd_bucket(T, T.keys[i], n_lines);
}

extern "C" int shn_debug_fine_dict(shn_ctx* ctx, const shn_table* t, const uint64_t* queries, uint64_t n, uint32_t* id_out, uint64_t* home_line_out,
                                   uint64_t* stats_out /* [4] */) {
  if (!ctx || !t || (n && !queries)) return shn_fail(SHN_ERR_ARG, "shn_debug_fine_dict: NULL argument");
  if (n >= (1ULL << 31) || t->n >= 0x7FFFFFFFULL) return shn_fail(SHN_ERR_ARG, "shn_debug_fine_dict: too many queries or k1-mers");
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  const uint64_t nt = t->n;
  ShnDevBufs bufs(s);
  uint32_t *d_weight = nullptr, *d_id = nullptr; uint8_t* d_flags = nullptr; uint64_t *d_q = nullptr, *d_home = nullptr, *d_thome = nullptr;
  HIP_TRY(bufs.get(&d_weight, (nt + 1) * 4)); HIP_TRY(bufs.get(&d_flags, nt + 1));
  HIP_TRY(bufs.get(&d_q, (n + 1) * 8)); HIP_TRY(bufs.get(&d_id, (n + 1) * 4)); HIP_TRY(bufs.get(&d_home, (n + 1) * 8));
  HIP_TRY(bufs.get(&d_thome, (nt + 1) * 8));
  if (nt) ext_prepare_launch(s, t, d_weight, d_flags);
  unsigned long long* lines = nullptr;
  uint64_t n_lines = 0;
  { const int rc = build_fine_dict(ctx, t, d_flags, &lines, &n_lines, nullptr); if (rc) return rc; }
  // (from here on every way out drains the stream and frees the dictionary)
  const uint64_t all_lines = n_lines + FD_HOPS;
  std::vector<unsigned long long> h_lines(stats_out ? all_lines * 16 : 0);
  std::vector<uint64_t> h_thome(stats_out ? nt : 0);
  std::vector<uint8_t> h_flags(stats_out ? nt : 0);
  hipError_t e = hipSuccess;
  if (n) {
    e = hipMemcpyAsync(d_q, queries, n * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(debug_fd_query_kernel, dim3((uint32_t)cdiv(n * 8, 256)), dim3(256), 0, s, shn_tab_idx(t), (const uint8_t*)d_flags, (const uint64_t*)d_q, n,
                         (const unsigned long long*)lines, n_lines, d_id, d_home);
      e = hipGetLastError();
    }
    if (e == hipSuccess && id_out) e = hipMemcpyAsync(id_out, d_id, n * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && home_line_out) e = hipMemcpyAsync(home_line_out, d_home, n * 8, hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess && stats_out) {
    if (nt) {
      hipLaunchKernelGGL(debug_fd_home_kernel, dim3((uint32_t)cdiv(nt, 256)), dim3(256), 0, s, shn_tab_idx(t), nt, n_lines, d_thome);
      e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(h_thome.data(), d_thome, nt * 8, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipMemcpyAsync(h_flags.data(), d_flags, nt, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_lines.data(), lines, all_lines * 128, hipMemcpyDeviceToHost, s);
  }
  const hipError_t e2 = hipStreamSynchronize(s);
  shn_dev_free(lines);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) return shn_fail(SHN_ERR_HIP, std::string("shn_debug_fine_dict: ") + hipGetErrorString(e));
  if (stats_out) {
    // hashed lines; lines whose count word says "more than fits"; table keys stored in another line than their own; table keys that are
    // not low-complexity and stored in no line (found through the table)
    std::vector<uint64_t> stored(nt, ~0ULL);
    uint64_t over = 0, bad_id = 0;
    for (uint64_t l = 0; l < all_lines; l++) {
      const uint32_t* w = (const uint32_t*)(h_lines.data() + l * 16);
      const uint32_t cnt = w[30];
      if (cnt > FD_SLOTS) over++;
      for (uint32_t sl = 0; sl < (cnt < FD_SLOTS ? cnt : FD_SLOTS); sl++) {
        const uint64_t j = w[20 + sl] & ~FD_PAL;
        if (j >= nt || stored[j] != ~0ULL) bad_id++; else stored[j] = l;
      }
    }
    if (bad_id) return shn_fail(SHN_ERR_INTERNAL, "shn_debug_fine_dict: a line holds an id word outside the table, or a k1-mer twice");
    uint64_t away = 0, nowhere = 0;
    for (uint64_t j = 0; j < nt; j++) {
      if (stored[j] == ~0ULL) { if (!(h_flags[j] & 2)) nowhere++; }
      else if (stored[j] != h_thome[j]) away++;
    }
    stats_out[0] = n_lines; stats_out[1] = over; stats_out[2] = away; stats_out[3] = nowhere;
  }
  return SHN_OK;
}
