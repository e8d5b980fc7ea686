// The weights and flags of a table's k1-mers and the one-line dictionary of their keys (k1dict.h): made here for the extension
// (extend.hip) and for both component labellings (components.hip).
#include "k1dict.h"

__global__ void ext_prepare_kernel(const uint64_t* __restrict__ tkeys, const uint32_t* __restrict__ tcounts, uint64_t n, int k,
                                   int canonical, uint32_t* __restrict__ weight, uint8_t* __restrict__ flags) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t key = tkeys[i];
  uint64_t c = tcounts[i];
  uint8_t f = 0;
  if (canonical && shn_revcomp(key, k) == key) { f |= 1; c *= 2; }
  // lowComplexity (extension_correction.py:142-149): the most frequent base occurs >= k-2 times
  uint64_t lanes = (k == 32) ? 0x5555555555555555ULL : ((1ULL << (2 * k)) - 1) & 0x5555555555555555ULL;
  int mx = 0;
  for (uint64_t v = 0; v < 4; v++) {
    uint64_t pat = v * 0x5555555555555555ULL;
    uint64_t t = ~(key ^ pat);
    int cnt = __popcll((t & (t >> 1)) & lanes);
    mx = cnt > mx ? cnt : mx;
  }
  if (mx >= k - 2) f |= 2;
  weight[i] = (uint32_t)(c > 0xFFFFFFFFULL ? 0xFFFFFFFFULL : c);
  flags[i] = f;
}
void ext_prepare_launch(hipStream_t s, const shn_table* t, uint32_t* d_weight, uint8_t* d_flags) {
  hipLaunchKernelGGL(ext_prepare_kernel, dim3((uint32_t)cdiv(t->n, 256)), dim3(256), 0, s, t->d_keys, t->d_counts, t->n, t->k, t->canonical, d_weight, d_flags);
}

__global__ void fd_build_kernel(const TabIdx T, const uint8_t* __restrict__ flags, uint64_t n,
                                unsigned long long* __restrict__ lines, uint64_t n_lines) {
  const uint64_t* __restrict__ tkeys = T.keys;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t f = flags[i];
  if (f & 2) return;
  const uint64_t key = tkeys[i];
  // (a full line sends the entry on to the next one -- the count word tallies the attempts, so a look-up that finds more than
  // FD_SLOTS there goes on as well; the dictionary ends in FD_HOPS spare lines)
  unsigned long long* line = lines + fd_bucket(T, key, n_lines) * 16;
  for (int hop = 0; hop < FD_HOPS; hop++, line += 16) {
    const uint32_t slot = atomicAdd((uint32_t*)line + 30, 1u);
    if (slot < FD_SLOTS) { line[slot] = key; ((uint32_t*)line)[20 + slot] = (uint32_t)i | ((f & 1) ? FD_PAL : 0u); break; }
  }
}

uint64_t fine_dict_lines(const shn_table* t) { return t->n / FD_PER_LINE + 1 + (t->layout ? t->n_buckets + 1 : 0) + FD_HOPS; }
int build_fine_dict(shn_ctx* ctx, const shn_table* t, const uint8_t* d_flags, unsigned long long** lines_out, uint64_t* n_lines_out,
                    void* room) {
  hipStream_t s = ctx->stream; shn_use_stream(s);
  const uint64_t n = t->n;
  const uint64_t n_lines = fine_dict_lines(t);
  unsigned long long* lines = (unsigned long long*)room;
  hipError_t e = lines ? hipSuccess : shn_dev_malloc(&lines, n_lines * 128);
  if (e == hipSuccess) e = hipMemsetAsync(lines, 0, n_lines * 128, s);
  if (e != hipSuccess) { if (lines && !room) shn_dev_free(lines); return shn_fail(SHN_ERR_HIP, std::string("build_fine_dict: ") + hipGetErrorString(e)); }
  if (n) hipLaunchKernelGGL(fd_build_kernel, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, s, shn_tab_idx(t), d_flags, n, lines, n_lines - FD_HOPS);
  *lines_out = lines; *n_lines_out = n_lines - FD_HOPS;          // (the look-ups hash into all but the spare lines at the end)
  return SHN_OK;
}
