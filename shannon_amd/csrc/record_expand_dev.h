// The HIP half of record_expand.h: the expansion kernel, its launch, and the call that expands everything and brings it back.
#pragma once
#include "common.h"
#include "record_expand.h"
#include <algorithm>

static inline ReadSetView view_of(const shn_reads* r) {
  ReadSetView v;
  v.words = r->d_words;
  v.mask = (r->n_invalid != 0 && r->d_mask) ? r->d_mask : nullptr;
  v.woff = r->d_woff; v.len = r->fixed_len ? nullptr : r->d_len;
  v.n = r->n_reads;
  v.fixed_len = r->fixed_len; v.wpr = r->wpr;
  return v;
}

// records 0 .. n - 1 of `rec` (byte offsets off[0 .. n]; the output starts at off[0]) into out; nothing is written at or behind
// min(off[n] - off[0], cap)
template <class R>
__global__ __launch_bounds__(SHN_XBLK) void records_expand_kernel(R rec, uint64_t n, const uint64_t* __restrict__ off, uint8_t* __restrict__ out, uint64_t cap) {
  __shared__ uint64_t s_first, s_last;
  const uint64_t base = off[0];
  const uint64_t total = min(off[n] - base, cap);
  const uint64_t per_block = (uint64_t)SHN_XBLK * SHN_XCHUNK;
  const uint64_t n_blocks = (total + per_block - 1) / per_block;
  for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {        // (the trip count is the block's: the barriers below are uniform)
    const uint64_t b0 = blk * per_block;
    if (threadIdx.x < 2) {
      const uint64_t r = record_of(off, 0, n, base + (threadIdx.x ? min(b0 + per_block, total) - 1 : b0));
      if (threadIdx.x) s_last = r; else s_first = r;
    }
    __syncthreads();
    const uint64_t pos0 = b0 + (uint64_t)threadIdx.x * SHN_XCHUNK;
    if (pos0 < total) expand_chunk(rec, n, off, s_first, s_last, total, pos0, out);
    __syncthreads();                            // s_first / s_last are written again in the next round
  }
}

// max_grid: blocks at the most (grid-stride beyond)
template <class R>
void launch_expand(hipStream_t s, const R& rec, uint64_t n, const uint64_t* d_off, uint8_t* d_out, uint64_t cap, uint32_t max_grid) {
  const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(cdiv(cap, (uint64_t)SHN_XBLK * SHN_XCHUNK), 1), max_grid);
  hipLaunchKernelGGL(records_expand_kernel<R>, dim3(grid), dim3(SHN_XBLK), 0, s, rec, n, d_off, d_out, cap);
}

// Pass 3 over all n records (offsets d_off[0 .. n] with d_off[0] = 0, queued on the context's stream) and the way back, behind ONE
// synchronisation: *total = all bytes of the records, *dl = min(cap, bound) bytes of them in `out` (out == NULL: a sizing call, *dl =
// 0, nothing is launched).  bound: what the total is at the most; expand(d_out, dl) launches into a buffer of dl bytes rounded up
// to 16.  Copies the caller queued before come back with the rest.  The total is the device's: the caller learns only now whether
// it exceeds cap -- the kernel stopped there.
template <class Expand>
int shn_expand_all(shn_ctx* ctx, ShnDevBufs& bufs, const uint64_t* d_off, uint64_t n, uint64_t bound, uint8_t* out, uint64_t cap, Expand&& expand,
                   uint64_t* total, uint64_t* dl_out) {
  hipStream_t s = ctx->stream;
  const uint64_t dl = out ? std::min(cap, bound) : 0;
  uint8_t* d_out = nullptr;
  if (dl) {
    HIP_TRY(bufs.get(&d_out, cdiv(dl, SHN_XCHUNK) * SHN_XCHUNK));
    expand(d_out, dl);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(total, d_off + n, 8, hipMemcpyDeviceToHost, s));
  if (dl) HIP_TRY(hipMemcpyAsync(out, d_out, dl, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *dl_out = dl;
  return SHN_OK;
}
