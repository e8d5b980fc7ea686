// shn_reads_collect: reads of resident sets (2 bits a base in HBM, + 1 bit a base where a set holds bases outside ACGT) as base
// codes one after the other -- what a partition's owner gets from the ranks that hold its reads (distributed.GpuOps.collect).
// Any set: fixed-length (slots of wpr words) or ragged (d_woff / d_len), two sets of different geometry in one call.
// The three passes of record_expand.h with CodeRec as the record: a record is a selected read, a byte of it a base code.
#include "record_expand_dev.h"

namespace {

constexpr uint32_t LEN_GRID = 256;   // blocks of the length pass at the most (grid-stride beyond)
constexpr uint32_t EXP_GRID = 1024;  // blocks of the expansion at the most: 16 waves per CU

__global__ __launch_bounds__(SHN_XBLK) void collect_lens_kernel(ReadSetView A, ReadSetView B, const uint32_t* __restrict__ sel, const uint8_t* __restrict__ flags,
                                                                uint64_t n, uint32_t* __restrict__ lens) {
  for (uint64_t i = (uint64_t)blockIdx.x * SHN_XBLK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SHN_XBLK) lens[i] = code_len(A, B, sel, flags, i);
}

}  // namespace

extern "C" int shn_reads_collect(shn_ctx* ctx, const shn_reads* a, const shn_reads* b, const uint32_t* sel, const uint8_t* flags, uint64_t n,
                                 uint32_t* lens_out, uint8_t* codes_out, uint64_t codes_cap, uint64_t* total_out) {
  if (!ctx || !a || !total_out || (n && (!sel || !flags))) return shn_fail(SHN_ERR_ARG, "shn_reads_collect: NULL argument");
  // ---- everything the host can check, before anything is launched
  bool uses_a = false, uses_b = false;
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t f = flags[i];
    if (f & ~1u) return shn_fail(SHN_ERR_ARG, "shn_reads_collect: flags other than bit 0 (reads travel as stored)");
    if ((f & 1) && !b) return shn_fail(SHN_ERR_ARG, "shn_reads_collect: a read of set b, and b is NULL");
    const shn_reads* r = (f & 1) ? b : a;
    if (sel[i] >= r->n_reads) return shn_fail(SHN_ERR_ARG, "shn_reads_collect: read index out of range");
    if (f & 1) uses_b = true; else uses_a = true;
  }
  const bool ragged = (uses_a && !a->fixed_len) || (uses_b && !b->fixed_len);
  uint64_t host_total = 0, bound = 0;           // the total where the host knows it; what it is at the most
  if (!ragged)
    for (uint64_t i = 0; i < n; i++) host_total += (flags[i] & 1) ? b->fixed_len : a->fixed_len;
  bound = ragged ? n * (uint64_t)std::max(uses_a ? a->max_len : 0u, uses_b ? b->max_len : 0u) : host_total;
  if (codes_out && !ragged && codes_cap < host_total) return shn_fail(SHN_ERR_ARG, "shn_reads_collect: codes_cap is below the total");
  *total_out = 0;
  if (n == 0) return SHN_OK;
  if (!ragged && !lens_out && !codes_out) { *total_out = host_total; return SHN_OK; }       // (a sizing call the host answers)
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  uint32_t *d_sel = nullptr, *d_lens = nullptr; uint8_t* d_flags = nullptr; uint64_t* d_off = nullptr;
  HIP_TRY(bufs.get(&d_sel, n * 4)); HIP_TRY(bufs.get(&d_flags, n)); HIP_TRY(bufs.get(&d_lens, n * 4)); HIP_TRY(bufs.get(&d_off, (n + 1) * 8));
  HIP_TRY(hipMemcpyAsync(d_sel, sel, n * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_flags, flags, n, hipMemcpyHostToDevice, s));
  const ReadSetView A = view_of(a), B = b ? view_of(b) : A;
  hipLaunchKernelGGL(collect_lens_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(n, SHN_XBLK), LEN_GRID)), dim3(SHN_XBLK), 0, s, A, B, (const uint32_t*)d_sel,
                     (const uint8_t*)d_flags, n, d_lens);
  int rc = shn_device_scan_u32(ctx, d_lens, n, d_off, nullptr);                              // (no synchronisation: the total comes back with the rest)
  if (rc) return rc;
  if (lens_out) HIP_TRY(hipMemcpyAsync(lens_out, d_lens, n * 4, hipMemcpyDeviceToHost, s));
  const bool use_mask = (uses_a && A.mask) || (uses_b && B.mask);
  uint64_t total = 0, dl = 0;
  rc = shn_expand_all(ctx, bufs, d_off, n, bound, codes_out, codes_cap, [&](uint8_t* d_codes, uint64_t room) {
    TimerRegion t(ctx, T_READS_COLLECT);
    if (use_mask) launch_expand(s, CodeRec<true>{A, B, d_sel, d_flags}, n, d_off, d_codes, room, EXP_GRID);
    else launch_expand(s, CodeRec<false>{A, B, d_sel, d_flags}, n, d_off, d_codes, room, EXP_GRID);
  }, &total, &dl);
  if (rc) return rc;
  *total_out = total;
  // byte model of the expansion: 2 bits read per base (+ 1 with a mask), 4 B of selection per read, 1 B written per base (said here:
  // the bases of ragged reads are counted on the device)
  if (dl && ctx->timing) __atomic_fetch_add(&ctx->abytes[T_READS_COLLECT], total / 4 + (use_mask ? total / 8 : 0) + n * 4 + total, __ATOMIC_RELAXED);
  if (codes_out && total > codes_cap) return shn_fail(SHN_ERR_ARG, "shn_reads_collect: codes_cap is below the total");
  return SHN_OK;
}
