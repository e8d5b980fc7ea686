// --inDisk: a partition's reads*.fasta and k1mer.dict as the reference writes them (kmers_for_component.py:351, 396-397, 452-477),
// formatted on the device from what is resident there -- the packed read sets + the routes (shn_reads_fasta), the partition
// contigs' text + one weight per window (shn_k1mers_dict_text) -- and written to files in chunks (shn_*_file).
// Both formatters have the three passes of shn_reads_collect (reads_collect.hip):
//   1. lengths     one thread per record (the decimal digits of a name / a weight in closed form);
//   2. offsets     the library's exclusive scan (shn_device_scan_u32);
//   3. expansion   one thread per ALIGNED 16-byte chunk of the output: it finds the record its first byte belongs to by a search in
//                  the offsets (the block's first and last chunk search all of them, the threads between search what lies between
//                  the two), then walks header, bases and newline -- a read's bases from whole 64-bit words of d_words / d_mask,
//                  kept in a register while the chunk stays inside them; base p of a reverse complement is 3 - code(len - 1 - p)
//                  -- and issues one 16-byte store.
#include "common.h"
#include "graph_dev.h"
#include "chunk_writer.h"
#include <algorithm>

namespace {

constexpr int TBLK = 256;            // threads per block
constexpr int TCHUNK = 16;           // output bytes per thread
constexpr uint32_t LEN_GRID = 1024;  // blocks of a length pass at the most (grid-stride beyond)
constexpr uint32_t EXP_GRID = 2048;  // blocks of an expansion at the most: 256 CUs x 8

struct TextSet {
  const uint64_t* words;
  const uint64_t* mask;      // nullptr: the set holds no base outside ACGT
  const uint64_t* woff;      // ragged: word offset of every read
  const uint32_t* len;       // ragged: length of every read (nullptr: fixed_len)
  uint64_t n;
  uint32_t fixed_len, wpr;
};

// which read a route entry names (include/shannon_hip.h, the table at shn_reads_fasta; kfc.ReadStore.mate1 / mate2)
struct ReadPick {
  uint64_t n_a;              // N: reads of set a
  int ss, mate;
  __device__ __forceinline__ bool operator()(const TextSet& A, const TextSet& B, uint64_t d, bool& second, uint64_t& r, bool& rc) const {
    if (ss) { second = mate == 2; r = d; rc = second; }
    else {
      const bool up = d >= n_a;
      r = up ? d - n_a : d;
      if (mate == 0) { second = false; rc = up; }
      else if (mate == 1) { second = up; rc = up; }
      else { second = up; rc = !up; }
    }
    return r < (second ? B.n : A.n);
  }
};

__device__ __forceinline__ uint32_t dec_digits(uint64_t v) {
  uint32_t d = 1;
  while (v >= 10) { v /= 10; d++; }
  return d;
}
// a number as decimal digits, four bits each: digit k from the right in lo (k < 16) / hi
__device__ __forceinline__ void dec_set(uint64_t v, uint64_t& lo, uint64_t& hi, uint32_t& dig) {
  lo = hi = 0; dig = 0;
  do {
    const uint64_t q = v / 10, d = v - q * 10;
    if (dig < 16) lo |= d << (4 * dig); else hi |= d << (4 * (dig - 16));
    dig++; v = q;
  } while (v);
}
__device__ __forceinline__ uint8_t dec_char(uint64_t lo, uint64_t hi, uint32_t k) {
  return (uint8_t)('0' + ((k < 16 ? lo >> (4 * k) : hi >> (4 * (k - 16))) & 15));
}

// ---- records of reads*.fasta: '>' name [_1 | _2] '\n' bases '\n'
__global__ __launch_bounds__(TBLK) void fasta_lens_kernel(TextSet A, TextSet B, ReadPick pick, const uint32_t* __restrict__ ridx, uint64_t n, uint64_t e0,
                                                          uint32_t* __restrict__ lens, uint32_t* __restrict__ err) {
  for (uint64_t i = (uint64_t)blockIdx.x * TBLK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TBLK) {
    bool second, rc; uint64_t r;
    uint32_t len = 0;
    if (pick(A, B, ridx[i], second, r, rc)) {
      const uint32_t* lp = second ? B.len : A.len;
      len = lp ? lp[r] : (second ? B.fixed_len : A.fixed_len);
    } else {
      atomicOr(err, 1u);                        // a route outside the read sets: an empty sequence here, SHN_ERR_ARG from the call
    }
    lens[i] = 1 + dec_digits(e0 + i) + (pick.mate ? 2 : 0) + 1 + len + 1;
  }
}

template <bool MASK>
struct FastaRec {
  TextSet A, B;
  ReadPick pick;
  const uint32_t* ridx;
  uint64_t e0;
  // the current record
  const uint64_t *words, *mask;
  uint64_t wbase, cw, cm, w, m, dlo, dhi;
  uint32_t len, H, dig;
  bool rc;
  __device__ __forceinline__ void enter(uint64_t i, uint32_t reclen) {
    bool second; uint64_t r;
    const bool ok = pick(A, B, ridx[i], second, r, rc);
    const TextSet& S = second ? B : A;
    words = S.words; mask = S.mask;
    wbase = !ok ? 0 : S.len ? S.woff[r] : r * S.wpr;
    dec_set(e0 + i, dlo, dhi, dig);
    H = 1 + dig + (pick.mate ? 2 : 0) + 1;
    len = reclen - H - 1;                       // (0 for a route outside the sets: nothing of them is read)
    cw = cm = ~0ULL;
  }
  __device__ __forceinline__ uint8_t at(uint32_t q) {
    if (q < H) {
      if (q == 0) return '>';
      if (q <= dig) return dec_char(dlo, dhi, dig - q);
      if (q == H - 1) return '\n';
      return q == dig + 1 ? '_' : (uint8_t)('0' + pick.mate);
    }
    const uint32_t p = q - H;
    if (p >= len) return '\n';
    const uint32_t sp = rc ? len - 1 - p : p;
    const uint64_t wi = wbase + (sp >> 5);
    if (wi != cw) { cw = wi; w = words[wi]; }
    uint32_t code = (uint32_t)(w >> (62 - 2 * (sp & 31))) & 3;
    if (rc) code = 3 - code;
    if (MASK) {
      if (mask) {
        const uint64_t mi = (wbase >> 1) + (sp >> 6);
        if (mi != cm) { cm = mi; m = mask[mi]; }
        if ((m >> (63 - (sp & 63))) & 1) return 'N';
      }
    }
    return (uint8_t)(0x54474341u >> (8 * code));          // "ACGT"
  }
};

// ---- records of k1mer.dict: k1mer '\t' weight '\n', every window of every contig in order
__global__ __launch_bounds__(TBLK) void dict_lens_kernel(const uint32_t* __restrict__ weights, uint64_t n, uint32_t k1, uint32_t* __restrict__ lens) {
  for (uint64_t i = (uint64_t)blockIdx.x * TBLK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TBLK)
    lens[i] = k1 + 1 + dec_digits(weights[i]) + 1;
}

struct DictRec {
  const uint8_t* text;       // the contigs one after the other
  const uint64_t* coff;      // n_strings + 1 offsets into text
  const uint64_t* woff;      // n_strings + 1: windows in front of every contig
  uint64_t n_strings;
  const uint32_t* weights;   // of the records of this launch
  uint64_t w0;               // window index of this launch's record 0
  uint32_t k1;
  uint64_t c;                // contig of the current record (~0: none yet)
  uint64_t tpos, dlo, dhi;
  uint32_t dig;
  __device__ __forceinline__ void enter(uint64_t i, uint32_t) {
    const uint64_t wi = w0 + i;
    if (c == ~0ULL) {                           // the last contig with woff[c] <= wi (contigs without a window share their offset with the next)
      uint64_t lo = 0, hi = n_strings;
      while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (woff[mid] <= wi) lo = mid; else hi = mid; }
      c = lo;
    } else {
      while (woff[c + 1] <= wi) c++;            // (wi < woff[n_strings]: c stays below n_strings)
    }
    tpos = coff[c] + (wi - woff[c]);
    dec_set(weights[i], dlo, dhi, dig);
  }
  __device__ __forceinline__ uint8_t at(uint32_t q) {
    if (q < k1) return text[tpos + q];
    if (q == k1) return '\t';
    if (q <= k1 + dig) return dec_char(dlo, dhi, k1 + dig - q);
    return '\n';
  }
};

// largest i in [lo, hi) with off[i] <= pos (off[lo] <= pos is the caller's)
__device__ __forceinline__ uint64_t record_of(const uint64_t* __restrict__ off, uint64_t lo, uint64_t hi, uint64_t pos) {
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

// records 0 .. n - 1 of `rec` (byte offsets off[0 .. n]; the output starts at off[0]) into out; nothing is written at or behind
// min(off[n] - off[0], cap).  Every record holds at least one byte.
template <class R>
__global__ __launch_bounds__(TBLK) void text_expand_kernel(R rec, uint64_t n, const uint64_t* __restrict__ off, uint8_t* __restrict__ out, uint64_t cap) {
  __shared__ uint64_t s_first, s_last;
  const uint64_t base = off[0];
  const uint64_t total = min(off[n] - base, cap);
  const uint64_t per_block = (uint64_t)TBLK * TCHUNK;
  const uint64_t n_blocks = (total + per_block - 1) / per_block;
  for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {        // (the trip count is the block's: the barriers below are uniform)
    const uint64_t b0 = blk * per_block;
    if (threadIdx.x < 2) {
      const uint64_t r = record_of(off, 0, n, base + (threadIdx.x ? min(b0 + per_block, total) - 1 : b0));
      if (threadIdx.x) s_last = r; else s_first = r;
    }
    __syncthreads();
    const uint64_t pos0 = b0 + (uint64_t)threadIdx.x * TCHUNK;
    if (pos0 < total) {
      // the record that holds byte pos0: off[i] <= base + pos0 < off[i + 1]
      uint64_t i = record_of(off, s_first, s_last + 1, base + pos0);
      uint64_t start = off[i] - base, end = off[i + 1] - base;
      rec.enter(i, (uint32_t)(end - start));
      const uint32_t cnt = (uint32_t)min((uint64_t)TCHUNK, total - pos0);
      uint64_t lo = 0, hi = 0;
      for (uint32_t j = 0; j < cnt; j++) {
        const uint64_t pos = pos0 + j;
        while (pos >= end) {                    // (pos < total <= off[n] - base: i stays below n)
          i++; start = end; end = off[i + 1] - base;
          rec.enter(i, (uint32_t)(end - start));
        }
        const uint64_t ch = rec.at((uint32_t)(pos - start));
        if (j < 8) lo |= ch << (8 * j); else hi |= ch << (8 * (j - 8));
      }
      if (cnt == TCHUNK) *reinterpret_cast<ulonglong2*>(out + pos0) = make_ulonglong2(lo, hi);
      else for (uint32_t j = 0; j < cnt; j++) out[pos0 + j] = (uint8_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xff);      // (the last chunk of the output)
    }
    __syncthreads();                            // s_first / s_last are written again in the next round
  }
}

template <class R>
void launch_expand(hipStream_t s, const R& rec, uint64_t n, const uint64_t* d_off, uint8_t* d_out, uint64_t cap) {
  const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(cdiv(cap, (uint64_t)TBLK * TCHUNK), 1), EXP_GRID);
  hipLaunchKernelGGL(text_expand_kernel<R>, dim3(grid), dim3(TBLK), 0, s, rec, n, d_off, d_out, cap);
}

TextSet view_of(const shn_reads* r) {
  TextSet v;
  v.words = r->d_words;
  v.mask = (r->n_invalid != 0 && r->d_mask) ? r->d_mask : nullptr;
  v.woff = r->d_woff; v.len = r->fixed_len ? nullptr : r->d_len;
  v.n = r->n_reads;
  v.fixed_len = r->fixed_len; v.wpr = r->wpr;
  return v;
}

// sum of the decimal digit counts of e0, e0 + 1, ..., e0 + n - 1 (one round per digit count)
uint64_t digits_sum(uint64_t e0, uint64_t n) {
  uint64_t sum = 0, lo = e0, left = n;
  while (left) {
    uint32_t d = 1;
    uint64_t next = 10;                          // the first number of d + 1 digits (d < 20)
    while (d < 20 && lo >= next) { d++; if (d < 20) next *= 10; }
    const uint64_t take = d < 20 ? std::min(left, next - lo) : left;
    sum += take * d;
    left -= take; lo += take;
  }
  return sum;
}

// ---- the FASTA formatter's call, checked and laid out once: one launch per call, or per chunk of a file
struct FastaJob {
  shn_ctx* ctx = nullptr;
  TextSet A, B;
  ReadPick pick;
  const uint32_t* d_ridx = nullptr;              // entries [lo, lo + n) of the routes, where they lie
  uint64_t n = 0, e0 = 0;
  bool use_mask = false;
  uint32_t* d_lens = nullptr;
  uint64_t* d_off = nullptr;                     // n + 1
  uint32_t* d_err = nullptr;
};

int fasta_check(const char* who, shn_ctx* ctx, const shn_reads* a, const shn_reads* b, const shn_routes* routes, uint64_t lo, uint64_t n, int mode, int mate,
                uint64_t e0, FastaJob* J) {
  const std::string w(who);
  if (!ctx || !a || !routes) return shn_fail(SHN_ERR_ARG, w + ": NULL argument");
  if (mode != SHN_READS_DOUBLED && mode != SHN_READS_STRAND_SPECIFIC) return shn_fail(SHN_ERR_ARG, w + ": unknown mode");
  if (mate < 0 || mate > 2) return shn_fail(SHN_ERR_ARG, w + ": unknown mate (0 single-end, 1, 2)");
  if (mate != 0 && !b) return shn_fail(SHN_ERR_ARG, w + ": a mate of a pair, and b is NULL");
  if (mate != 0 && b->n_reads != a->n_reads) return shn_fail(SHN_ERR_ARG, w + ": the two sets of a pair hold different numbers of reads");
  const uint64_t have = shn_routes_size(routes);
  if (lo > have || n > have - lo) return shn_fail(SHN_ERR_ARG, w + ": lo + n lies beyond the routes");
  if (e0 + n < e0) return shn_fail(SHN_ERR_ARG, w + ": e0 + n overflows");
  J->ctx = ctx;
  J->A = view_of(a); J->B = (mate != 0) ? view_of(b) : J->A;
  J->pick.n_a = a->n_reads; J->pick.ss = mode == SHN_READS_STRAND_SPECIFIC; J->pick.mate = mate;
  J->n = n; J->e0 = e0;
  J->use_mask = J->A.mask || (mate != 0 && J->B.mask);
  if (n) { int rc = shn_routes_device_slice(routes, lo, n, &J->d_ridx); if (rc) return rc; }
  return SHN_OK;
}

// passes 1 and 2 (nothing waits for them)
int fasta_plan(FastaJob* J, ShnDevBufs& bufs) {
  hipStream_t s = J->ctx->stream;
  HIP_TRY(bufs.get(&J->d_lens, J->n * 4)); HIP_TRY(bufs.get(&J->d_off, (J->n + 1) * 8)); HIP_TRY(bufs.get(&J->d_err, 4));
  HIP_TRY(hipMemsetAsync(J->d_err, 0, 4, s));
  hipLaunchKernelGGL(fasta_lens_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(J->n, TBLK), LEN_GRID)), dim3(TBLK), 0, s, J->A, J->B, J->pick, J->d_ridx, J->n,
                     J->e0, J->d_lens, J->d_err);
  return shn_device_scan_u32(J->ctx, J->d_lens, J->n, J->d_off, nullptr);
}

// pass 3 over records [r0, r1) into d_out (room for `cap` bytes rounded up to 16)
void fasta_expand(const FastaJob& J, uint64_t r0, uint64_t r1, uint8_t* d_out, uint64_t cap) {
  TimerRegion t(J.ctx, T_READS_FASTA);
  hipStream_t s = J.ctx->stream;
  if (J.use_mask) {
    FastaRec<true> R; R.A = J.A; R.B = J.B; R.pick = J.pick; R.ridx = J.d_ridx + r0; R.e0 = J.e0 + r0;
    launch_expand(s, R, r1 - r0, J.d_off + r0, d_out, cap);
  } else {
    FastaRec<false> R; R.A = J.A; R.B = J.B; R.pick = J.pick; R.ridx = J.d_ridx + r0; R.e0 = J.e0 + r0;
    launch_expand(s, R, r1 - r0, J.d_off + r0, d_out, cap);
  }
}
// byte model of the expansion of `nrec` records named from `e` on, `bytes` bytes of text: 2 bits read per base (+ 1 with a mask),
// 4 B of route per record, the bytes written (said once the bytes are known: the bases of ragged reads are counted on the device)
void fasta_model(const FastaJob& J, uint64_t e, uint64_t nrec, uint64_t bytes) {
  if (!J.ctx->timing) return;
  const uint64_t head = nrec * (3 + (J.pick.mate ? 2 : 0)) + digits_sum(e, nrec);
  const uint64_t bases = bytes > head ? bytes - head : 0;
  __atomic_fetch_add(&J.ctx->abytes[T_READS_FASTA], bases / 4 + (J.use_mask ? bases / 8 : 0) + nrec * 4 + bytes, __ATOMIC_RELAXED);
}

// ---- the dictionary formatter's call
struct DictJob {
  shn_ctx* ctx = nullptr;
  uint64_t n_strings = 0, n_windows = 0, text_bytes = 0;
  uint32_t k1 = 0;
  std::vector<uint64_t> coff, woff;              // relative to the first contig's first byte
  uint8_t* d_text = nullptr;
  uint64_t *d_coff = nullptr, *d_woff = nullptr, *d_off = nullptr;
  uint32_t *d_weights = nullptr, *d_lens = nullptr;
};

int dict_check(const char* who, shn_ctx* ctx, const uint8_t* text, const uint64_t* off, uint64_t n_strings, int k1, const uint32_t* weights, DictJob* J) {
  const std::string w(who);
  if (!ctx || (n_strings && (!text || !off))) return shn_fail(SHN_ERR_ARG, w + ": NULL argument");
  if (k1 < 1 || k1 > 4096) return shn_fail(SHN_ERR_ARG, w + ": k1 out of range");
  J->ctx = ctx; J->n_strings = n_strings; J->k1 = (uint32_t)k1;
  J->coff.assign(n_strings + 1, 0); J->woff.assign(n_strings + 1, 0);
  for (uint64_t c = 0; c < n_strings; c++) {
    if (off[c + 1] < off[c]) return shn_fail(SHN_ERR_ARG, w + ": offsets not monotone");
    const uint64_t len = off[c + 1] - off[c];
    J->coff[c + 1] = off[c + 1] - off[0];
    J->woff[c + 1] = J->woff[c] + (len >= (uint64_t)k1 ? len - k1 + 1 : 0);
  }
  J->n_windows = J->woff[n_strings]; J->text_bytes = J->coff[n_strings];
  if (J->n_windows && !weights) return shn_fail(SHN_ERR_ARG, w + ": weights is NULL");
  return SHN_OK;
}

// uploads + passes 1 and 2 (n_windows != 0)
int dict_plan(DictJob* J, ShnDevBufs& bufs, const uint8_t* text, const uint64_t* off, const uint32_t* weights) {
  hipStream_t s = J->ctx->stream;
  const uint64_t n = J->n_windows, ns = J->n_strings;
  HIP_TRY(bufs.get(&J->d_text, J->text_bytes)); HIP_TRY(bufs.get(&J->d_coff, (ns + 1) * 8)); HIP_TRY(bufs.get(&J->d_woff, (ns + 1) * 8));
  HIP_TRY(bufs.get(&J->d_weights, n * 4)); HIP_TRY(bufs.get(&J->d_lens, n * 4)); HIP_TRY(bufs.get(&J->d_off, (n + 1) * 8));
  HIP_TRY(hipMemcpyAsync(J->d_text, text + off[0], J->text_bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(J->d_coff, J->coff.data(), (ns + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(J->d_woff, J->woff.data(), (ns + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(J->d_weights, weights, n * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(dict_lens_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(n, TBLK), LEN_GRID)), dim3(TBLK), 0, s, (const uint32_t*)J->d_weights, n, J->k1,
                     J->d_lens);
  return shn_device_scan_u32(J->ctx, J->d_lens, n, J->d_off, nullptr);
}

// pass 3 over windows [r0, r1); byte model: the contig text under them once (the k1-mer bytes are a copy of it), 4 B of weight per
// window, the bytes written
void dict_expand(const DictJob& J, uint64_t r0, uint64_t r1, uint8_t* d_out, uint64_t cap, uint64_t bytes) {
  TimerRegion t(J.ctx, T_K1MERS_DICT);
  DictRec R;
  R.text = J.d_text; R.coff = J.d_coff; R.woff = J.d_woff; R.n_strings = J.n_strings; R.weights = J.d_weights + r0; R.w0 = r0; R.k1 = J.k1; R.c = ~0ULL;
  launch_expand(J.ctx->stream, R, r1 - r0, J.d_off + r0, d_out, cap);
  t.bytes((r1 - r0) + J.k1 - 1 + (r1 - r0) * 4 + bytes);
}

// ---- staging of the file drivers: two pinned buffers, kept from call to call (one file at a time per process)
std::mutex g_stage_mu;
ShnPinned g_stage[2];

uint64_t stage_bytes() { return shn_env_u64("SHN_INDISK_STAGE_BYTES", 32ull << 20, 4096, 1ull << 30); }

}  // namespace

extern "C" int shn_reads_fasta(shn_ctx* ctx, const shn_reads* a, const shn_reads* b, const shn_routes* routes, uint64_t lo, uint64_t n, int mode, int mate,
                               uint64_t e0, uint8_t* out, uint64_t cap, uint64_t* total_out) {
  if (!total_out) return shn_fail(SHN_ERR_ARG, "shn_reads_fasta: NULL argument");
  // ---- everything the host can check, before anything is launched
  FastaJob J;
  int rc = fasta_check("shn_reads_fasta", ctx, a, b, routes, lo, n, mode, mate, e0, &J);
  if (rc) return rc;
  *total_out = 0;
  if (n == 0) return SHN_OK;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  if ((rc = fasta_plan(&J, bufs))) return rc;
  // what the text is at the most: the host knows the reads' longest length, the device their sum
  const uint64_t bound = n * (26ull + std::max(a->max_len, mate ? b->max_len : 0u));
  const uint64_t dl = out ? std::min(cap, bound) : 0;                      // bytes of text that come back
  uint8_t* d_text = nullptr;
  if (dl) {
    HIP_TRY(bufs.get(&d_text, cdiv(dl, TCHUNK) * TCHUNK));
    fasta_expand(J, 0, n, d_text, dl);
  }
  HIP_TRY(hipGetLastError());
  uint64_t total = 0; uint32_t err = 0;
  HIP_TRY(hipMemcpyAsync(&total, J.d_off + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&err, J.d_err, 4, hipMemcpyDeviceToHost, s));
  if (dl) HIP_TRY(hipMemcpyAsync(out, d_text, dl, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *total_out = total;
  if (dl) fasta_model(J, e0, n, std::min(total, dl));
  if (err) return shn_fail(SHN_ERR_ARG, "shn_reads_fasta: a route names a read outside the read sets");
  // (the total is the device's: known only now; the kernel stopped at cap)
  if (out && total > cap) return shn_fail(SHN_ERR_ARG, "shn_reads_fasta: cap is below the total");
  return SHN_OK;
}

extern "C" int shn_reads_fasta_file(shn_ctx* ctx, const shn_reads* a, const shn_reads* b, const shn_routes* routes, uint64_t lo, uint64_t n, int mode,
                                    int mate, uint64_t e0, const char* path, uint64_t* bytes_out) {
  if (!path) return shn_fail(SHN_ERR_ARG, "shn_reads_fasta_file: NULL argument");
  FastaJob J;
  int rc = fasta_check("shn_reads_fasta_file", ctx, a, b, routes, lo, n, mode, mate, e0, &J);
  if (rc) return rc;
  if (bytes_out) *bytes_out = 0;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  std::vector<uint64_t> off(n + 1, 0);
  if (n) {
    if ((rc = fasta_plan(&J, bufs))) return rc;
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(off.data(), J.d_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&err, J.d_err, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err) return shn_fail(SHN_ERR_ARG, "shn_reads_fasta_file: a route names a read outside the read sets");
  }
  const uint64_t stage = stage_bytes();
  const uint64_t room = cdiv(std::max(stage, shn_longest_record(off.data(), n)), TCHUNK) * TCHUNK;
  std::lock_guard<std::mutex> lk(g_stage_mu);
  uint8_t* pin[2] = {nullptr, nullptr};
  uint8_t* d_stage = nullptr;
  if (n) {
    for (int i = 0; i < 2; i++) { void* p; if ((rc = g_stage[i].get(room, &p))) return rc; pin[i] = (uint8_t*)p; }
    HIP_TRY(bufs.get(&d_stage, room));
  }
  std::string msg;
  auto fill = [&](uint64_t r0, uint64_t r1, int slot, const uint8_t** data) -> int {
    const uint64_t bytes = off[r1] - off[r0];
    fasta_expand(J, r0, r1, d_stage, bytes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(pin[slot], d_stage, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    fasta_model(J, e0 + r0, r1 - r0, bytes);
    *data = pin[slot];
    return 0;
  };
  rc = shn_write_records_chunked(path, off.data(), n, stage, fill, &msg, bytes_out);
  if (rc == -1) return shn_fail(SHN_ERR_IO, "shn_reads_fasta_file: " + msg);
  return rc;
}

extern "C" int shn_k1mers_dict_text(shn_ctx* ctx, const uint8_t* text, const uint64_t* off, uint64_t n_strings, int k1, const uint32_t* weights, uint8_t* out,
                                    uint64_t cap, uint64_t* total_out) {
  if (!total_out) return shn_fail(SHN_ERR_ARG, "shn_k1mers_dict_text: NULL argument");
  DictJob J;
  int rc = dict_check("shn_k1mers_dict_text", ctx, text, off, n_strings, k1, weights, &J);
  if (rc) return rc;
  *total_out = 0;
  const uint64_t n = J.n_windows;
  if (n == 0) return SHN_OK;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  if ((rc = dict_plan(&J, bufs, text, off, weights))) return rc;
  const uint64_t bound = n * ((uint64_t)k1 + 12);                          // a weight has ten digits at the most
  const uint64_t dl = out ? std::min(cap, bound) : 0;
  uint8_t* d_text = nullptr;
  if (dl) {
    HIP_TRY(bufs.get(&d_text, cdiv(dl, TCHUNK) * TCHUNK));
    dict_expand(J, 0, n, d_text, dl, dl);
  }
  HIP_TRY(hipGetLastError());
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, J.d_off + n, 8, hipMemcpyDeviceToHost, s));
  if (dl) HIP_TRY(hipMemcpyAsync(out, d_text, dl, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *total_out = total;
  if (out && total > cap) return shn_fail(SHN_ERR_ARG, "shn_k1mers_dict_text: cap is below the total");
  return SHN_OK;
}

extern "C" int shn_k1mers_dict_file(shn_ctx* ctx, const uint8_t* text, const uint64_t* off, uint64_t n_strings, int k1, const uint32_t* weights,
                                    const char* path, uint64_t* bytes_out) {
  if (!path) return shn_fail(SHN_ERR_ARG, "shn_k1mers_dict_file: NULL argument");
  DictJob J;
  int rc = dict_check("shn_k1mers_dict_file", ctx, text, off, n_strings, k1, weights, &J);
  if (rc) return rc;
  if (bytes_out) *bytes_out = 0;
  SHN_ENTER(ctx);
  hipStream_t s = ctx->stream;
  ShnDevBufs bufs(s);
  const uint64_t n = J.n_windows;
  std::vector<uint64_t> roff(n + 1, 0);
  if (n) {
    if ((rc = dict_plan(&J, bufs, text, off, weights))) return rc;
    HIP_TRY(hipMemcpyAsync(roff.data(), J.d_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  const uint64_t stage = stage_bytes();
  const uint64_t room = cdiv(std::max(stage, shn_longest_record(roff.data(), n)), TCHUNK) * TCHUNK;
  std::lock_guard<std::mutex> lk(g_stage_mu);
  uint8_t* pin[2] = {nullptr, nullptr};
  uint8_t* d_stage = nullptr;
  if (n) {
    for (int i = 0; i < 2; i++) { void* p; if ((rc = g_stage[i].get(room, &p))) return rc; pin[i] = (uint8_t*)p; }
    HIP_TRY(bufs.get(&d_stage, room));
  }
  std::string msg;
  auto fill = [&](uint64_t r0, uint64_t r1, int slot, const uint8_t** data) -> int {
    const uint64_t bytes = roff[r1] - roff[r0];
    dict_expand(J, r0, r1, d_stage, bytes, bytes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(pin[slot], d_stage, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *data = pin[slot];
    return 0;
  };
  rc = shn_write_records_chunked(path, roff.data(), n, stage, fill, &msg, bytes_out);
  if (rc == -1) return shn_fail(SHN_ERR_IO, "shn_k1mers_dict_file: " + msg);
  return rc;
}
