// shn_reads_collect: reads of resident sets (2 bits a base in HBM, + 1 bit a base where a set holds bases outside ACGT) as base
// codes one after the other -- what a partition's owner gets from the ranks that hold its reads (distributed.GpuOps.collect).
// Any set: fixed-length (slots of wpr words) or ragged (d_woff / d_len), two sets of different geometry in one call.
//   1. lengths     one thread per selected read;
//   2. offsets     the library's exclusive scan (shn_device_scan_u32);
//   3. expansion   one thread per ALIGNED 16-byte chunk of the output: it finds the read its first byte belongs to by a search in the
//                  offsets (the block's first and last chunk search all of them, the threads between search what lies between the
//                  two), then walks: whole 64-bit words of d_words / d_mask, kept in a register while the chunk stays inside them,
//                  one 16-byte store.  The work of a 250-base read spreads over 16 lanes, a 30-base read shares a lane with its
//                  neighbours: no lane waits for a long read.
#include "common.h"
#include <algorithm>

namespace {

struct CollectSet {
  const uint64_t* words;
  const uint64_t* mask;      // nullptr: the set holds no base outside ACGT
  const uint64_t* woff;      // ragged: word offset of every read
  const uint32_t* len;       // ragged: length of every read (nullptr: fixed_len)
  uint32_t fixed_len, wpr;
};

constexpr int CBLK = 256;            // threads per block
constexpr int CCHUNK = 16;           // output bytes (= bases) per thread
constexpr uint32_t LEN_GRID = 256;   // blocks of the length pass at the most (grid-stride beyond)
constexpr uint32_t EXP_GRID = 1024;  // blocks of the expansion at the most: 16 waves per CU

__global__ __launch_bounds__(CBLK) void collect_lens_kernel(CollectSet A, CollectSet B, const uint32_t* __restrict__ sel, const uint8_t* __restrict__ flags,
                                                            uint64_t n, uint32_t* __restrict__ lens) {
  for (uint64_t i = (uint64_t)blockIdx.x * CBLK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * CBLK) {
    const bool second = flags[i] & 1;
    const uint32_t* len = second ? B.len : A.len;
    lens[i] = len ? len[sel[i]] : (second ? B.fixed_len : A.fixed_len);
  }
}

// largest i in [lo, hi) with off[i] <= pos (off[lo] <= pos is the caller's)
__device__ __forceinline__ uint64_t read_of(const uint64_t* __restrict__ off, uint64_t lo, uint64_t hi, uint64_t pos) {
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

// `total` = min(off[n], capacity of out): nothing is written at or behind it
template <bool MASK>
__global__ __launch_bounds__(CBLK) void collect_expand_kernel(CollectSet A, CollectSet B, const uint32_t* __restrict__ sel, const uint8_t* __restrict__ flags,
                                                              uint64_t n, const uint64_t* __restrict__ off, uint8_t* __restrict__ out, uint64_t cap) {
  __shared__ uint64_t s_first, s_last;
  const uint64_t total = min(off[n], cap);
  const uint64_t per_block = (uint64_t)CBLK * CCHUNK;
  const uint64_t n_blocks = (total + per_block - 1) / per_block;
  for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {        // (the trip count is the block's: the barriers below are uniform)
    const uint64_t b0 = blk * per_block;
    if (threadIdx.x < 2) {
      const uint64_t r = read_of(off, 0, n, threadIdx.x ? min(b0 + per_block, total) - 1 : b0);
      if (threadIdx.x) s_last = r; else s_first = r;
    }
    __syncthreads();
    const uint64_t pos0 = b0 + (uint64_t)threadIdx.x * CCHUNK;
    if (pos0 < total) {
      // the read that holds byte pos0: off[i] <= pos0 < off[i + 1] (reads without bases lie below it or are stepped over further down)
      uint64_t i = read_of(off, s_first, s_last + 1, pos0);
      uint64_t start = 0, end = off[i];
      const uint64_t *words = nullptr, *mask = nullptr;
      uint64_t wbase = 0, cw = ~0ULL, cm = ~0ULL, w = 0, m = 0;
      auto enter = [&]() {                      // read i becomes the current one
        start = end; end = off[i + 1];
        const CollectSet& S = (flags[i] & 1) ? B : A;
        const uint64_t r = sel[i];
        words = S.words; mask = S.mask;
        wbase = S.len ? S.woff[r] : r * S.wpr;
        cw = cm = ~0ULL;
      };
      enter();
      const uint32_t cnt = (uint32_t)min((uint64_t)CCHUNK, total - pos0);
      uint64_t lo = 0, hi = 0;
      for (uint32_t j = 0; j < cnt; j++) {
        const uint64_t pos = pos0 + j;
        while (pos >= end) { i++; enter(); }    // (pos < total <= off[n]: i stays below n)
        const uint32_t p = (uint32_t)(pos - start);
        const uint64_t wi = wbase + (p >> 5);
        if (wi != cw) { cw = wi; w = words[wi]; }
        uint64_t code = (w >> (62 - 2 * (p & 31))) & 3;
        if (MASK) {
          if (mask) {
            const uint64_t mi = (wbase >> 1) + (p >> 6);
            if (mi != cm) { cm = mi; m = mask[mi]; }
            if ((m >> (63 - (p & 63))) & 1) code = 4;
          }
        }
        if (j < 8) lo |= code << (8 * j); else hi |= code << (8 * (j - 8));
      }
      if (cnt == CCHUNK) *reinterpret_cast<ulonglong2*>(out + pos0) = make_ulonglong2(lo, hi);
      else for (uint32_t j = 0; j < cnt; j++) out[pos0 + j] = (uint8_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xff);      // (the last chunk of the output)
    }
    __syncthreads();                            // s_first / s_last are written again in the next round
  }
}

CollectSet view_of(const shn_reads* r) {
  CollectSet v;
  v.words = r->d_words;
  v.mask = (r->n_invalid != 0 && r->d_mask) ? r->d_mask : nullptr;
  v.woff = r->d_woff; v.len = r->fixed_len ? nullptr : r->d_len;
  v.fixed_len = r->fixed_len; v.wpr = r->wpr;
  return v;
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
  const uint64_t dl = codes_out ? std::min(codes_cap, bound) : 0;                            // bytes of codes that come back
  ShnDevBufs bufs(s);
  uint32_t *d_sel = nullptr, *d_lens = nullptr; uint8_t *d_flags = nullptr, *d_codes = nullptr; uint64_t* d_off = nullptr;
  HIP_TRY(bufs.get(&d_sel, n * 4)); HIP_TRY(bufs.get(&d_flags, n)); HIP_TRY(bufs.get(&d_lens, n * 4)); HIP_TRY(bufs.get(&d_off, (n + 1) * 8));
  if (dl) HIP_TRY(bufs.get(&d_codes, cdiv(dl, CCHUNK) * CCHUNK));
  HIP_TRY(hipMemcpyAsync(d_sel, sel, n * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_flags, flags, n, hipMemcpyHostToDevice, s));
  const CollectSet A = view_of(a), B = b ? view_of(b) : A;
  hipLaunchKernelGGL(collect_lens_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(n, CBLK), LEN_GRID)), dim3(CBLK), 0, s, A, B, (const uint32_t*)d_sel,
                     (const uint8_t*)d_flags, n, d_lens);
  int rc = shn_device_scan_u32(ctx, d_lens, n, d_off, nullptr);                              // (no synchronisation: the total comes back with the rest)
  if (rc) return rc;
  const bool use_mask = (uses_a && A.mask) || (uses_b && B.mask);
  if (dl) {
    TimerRegion t(ctx, T_READS_COLLECT);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(cdiv(dl, (uint64_t)CBLK * CCHUNK), EXP_GRID);
    if (use_mask) hipLaunchKernelGGL(collect_expand_kernel<true>, dim3(grid), dim3(CBLK), 0, s, A, B, (const uint32_t*)d_sel, (const uint8_t*)d_flags, n,
                                     (const uint64_t*)d_off, d_codes, dl);
    else hipLaunchKernelGGL(collect_expand_kernel<false>, dim3(grid), dim3(CBLK), 0, s, A, B, (const uint32_t*)d_sel, (const uint8_t*)d_flags, n,
                            (const uint64_t*)d_off, d_codes, dl);
  }
  HIP_TRY(hipGetLastError());
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, d_off + n, 8, hipMemcpyDeviceToHost, s));
  if (lens_out) HIP_TRY(hipMemcpyAsync(lens_out, d_lens, n * 4, hipMemcpyDeviceToHost, s));
  if (dl) HIP_TRY(hipMemcpyAsync(codes_out, d_codes, dl, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *total_out = total;
  // byte model of the expansion: 2 bits read per base (+ 1 with a mask), 4 B of selection per read, 1 B written per base (said here:
  // the bases of ragged reads are counted on the device)
  if (dl && ctx->timing) __atomic_fetch_add(&ctx->abytes[T_READS_COLLECT], total / 4 + (use_mask ? total / 8 : 0) + n * 4 + total, __ATOMIC_RELAXED);
  // (with a ragged set the total is the device's: known only now; the kernel stopped at codes_cap)
  if (codes_out && total > codes_cap) return shn_fail(SHN_ERR_ARG, "shn_reads_collect: codes_cap is below the total");
  return SHN_OK;
}
