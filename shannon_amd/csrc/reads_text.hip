// --inDisk: a partition's reads*.fasta and k1mer.dict as the reference writes them (kmers_for_component.py:351, 396-397, 452-477),
// formatted on the device from what is resident there -- the packed read sets + the routes (shn_reads_fasta), the partition
// contigs' text + one weight per window (shn_k1mers_dict_text) -- and written to files in chunks (shn_*_file).
// Both formatters are the three passes of record_expand.h, with FastaRec / DictRec as the record: header, bases and newline of a
// read (base p of a reverse complement is 3 - code(len - 1 - p)), k1-mer, tab, weight and newline of a window.
#include "record_expand_dev.h"
#include "graph_dev.h"
#include "chunk_writer.h"

namespace {

constexpr uint32_t LEN_GRID = 1024;  // blocks of a length pass at the most (grid-stride beyond)
constexpr uint32_t EXP_GRID = 2048;  // blocks of an expansion at the most: 256 CUs x 8

__global__ __launch_bounds__(SHN_XBLK) void fasta_lens_kernel(ReadSetView A, ReadSetView B, ReadPick pick, const uint32_t* __restrict__ ridx, uint64_t n, uint64_t e0,
                                                              uint32_t* __restrict__ lens, uint32_t* __restrict__ err) {
  for (uint64_t i = (uint64_t)blockIdx.x * SHN_XBLK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SHN_XBLK) {
    bool ok;
    lens[i] = fasta_len(A, B, pick, ridx, e0, i, &ok);
    if (!ok) atomicOr(err, 1u);
  }
}

__global__ __launch_bounds__(SHN_XBLK) void dict_lens_kernel(const uint32_t* __restrict__ weights, uint64_t n, uint32_t k1, uint32_t* __restrict__ lens) {
  for (uint64_t i = (uint64_t)blockIdx.x * SHN_XBLK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SHN_XBLK) lens[i] = dict_len(weights, k1, i);
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
  ReadSetView A, B;
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
  hipLaunchKernelGGL(fasta_lens_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(J->n, SHN_XBLK), LEN_GRID)), dim3(SHN_XBLK), 0, s, J->A, J->B, J->pick, J->d_ridx, J->n,
                     J->e0, J->d_lens, J->d_err);
  return shn_device_scan_u32(J->ctx, J->d_lens, J->n, J->d_off, nullptr);
}

// pass 3 over records [r0, r1) into d_out (room for `cap` bytes rounded up to 16)
void fasta_expand(const FastaJob& J, uint64_t r0, uint64_t r1, uint8_t* d_out, uint64_t cap) {
  TimerRegion t(J.ctx, T_READS_FASTA);
  hipStream_t s = J.ctx->stream;
  if (J.use_mask) launch_expand(s, FastaRec<true>{J.A, J.B, J.pick, J.d_ridx + r0, J.e0 + r0}, r1 - r0, J.d_off + r0, d_out, cap, EXP_GRID);
  else launch_expand(s, FastaRec<false>{J.A, J.B, J.pick, J.d_ridx + r0, J.e0 + r0}, r1 - r0, J.d_off + r0, d_out, cap, EXP_GRID);
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
  hipLaunchKernelGGL(dict_lens_kernel, dim3((uint32_t)std::min<uint64_t>(cdiv(n, SHN_XBLK), LEN_GRID)), dim3(SHN_XBLK), 0, s, (const uint32_t*)J->d_weights, n, J->k1,
                     J->d_lens);
  return shn_device_scan_u32(J->ctx, J->d_lens, n, J->d_off, nullptr);
}

// pass 3 over windows [r0, r1); byte model: the contig text under them once (the k1-mer bytes are a copy of it), 4 B of weight per
// window, the bytes written
void dict_expand(const DictJob& J, uint64_t r0, uint64_t r1, uint8_t* d_out, uint64_t cap, uint64_t bytes) {
  TimerRegion t(J.ctx, T_K1MERS_DICT);
  DictRec R;
  R.text = J.d_text; R.coff = J.d_coff; R.woff = J.d_woff; R.n_strings = J.n_strings; R.weights = J.d_weights + r0; R.w0 = r0; R.k1 = J.k1; R.c = ~0ULL;
  launch_expand(J.ctx->stream, R, r1 - r0, J.d_off + r0, d_out, cap, EXP_GRID);
  t.bytes((r1 - r0) + J.k1 - 1 + (r1 - r0) * 4 + bytes);
}

// ---- staging of the file drivers: two pinned buffers, kept from call to call (one file at a time per process)
std::mutex g_stage_mu;
ShnPinned g_stage[2];

uint64_t stage_bytes() { return shn_env_u64("SHN_INDISK_STAGE_BYTES", 32ull << 20, 4096, 1ull << 30); }

// Pass 3 chunk by chunk into a file: records 0 .. n - 1 with the byte offsets off[0 .. n] (on the host), chunks of at most
// SHN_INDISK_STAGE_BYTES that end on a record boundary; expand(r0, r1, d_out, bytes) launches records [r0, r1) into d_out.  Chunk
// c + 1 is formatted and copied into one of the two pinned buffers while the writer thread writes chunk c (chunk_writer.h).
template <class Expand>
int expand_to_file(const char* who, shn_ctx* ctx, ShnDevBufs& bufs, const std::vector<uint64_t>& off, const char* path, Expand&& expand, uint64_t* bytes_out) {
  hipStream_t s = ctx->stream;
  const uint64_t n = off.size() - 1;
  const uint64_t stage = stage_bytes();
  const uint64_t room = cdiv(std::max(stage, shn_longest_record(off.data(), n)), SHN_XCHUNK) * SHN_XCHUNK;
  std::lock_guard<std::mutex> lk(g_stage_mu);
  uint8_t* pin[2] = {nullptr, nullptr};
  uint8_t* d_stage = nullptr;
  if (n) {
    for (int i = 0; i < 2; i++) { void* p; int rc = g_stage[i].get(room, &p); if (rc) return rc; pin[i] = (uint8_t*)p; }
    HIP_TRY(bufs.get(&d_stage, room));
  }
  std::string msg;
  auto fill = [&](uint64_t r0, uint64_t r1, int slot, const uint8_t** data) -> int {
    const uint64_t bytes = off[r1] - off[r0];
    expand(r0, r1, d_stage, bytes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(pin[slot], d_stage, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *data = pin[slot];
    return 0;
  };
  const int rc = shn_write_records_chunked(path, off.data(), n, stage, fill, &msg, bytes_out);
  if (rc == -1) return shn_fail(SHN_ERR_IO, std::string(who) + ": " + msg);
  return rc;
}

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
  ShnDevBufs bufs(ctx->stream);
  if ((rc = fasta_plan(&J, bufs))) return rc;
  uint32_t err = 0;
  HIP_TRY(hipMemcpyAsync(&err, J.d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
  // what the text is at the most: the host knows the reads' longest length, the device their sum
  const uint64_t bound = n * (26ull + std::max(a->max_len, mate ? b->max_len : 0u));
  uint64_t total = 0, dl = 0;
  rc = shn_expand_all(ctx, bufs, J.d_off, n, bound, out, cap, [&](uint8_t* d_text, uint64_t room) { fasta_expand(J, 0, n, d_text, room); }, &total, &dl);
  if (rc) return rc;
  *total_out = total;
  if (dl) fasta_model(J, e0, n, std::min(total, dl));
  if (err) return shn_fail(SHN_ERR_ARG, "shn_reads_fasta: a route names a read outside the read sets");
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
  return expand_to_file("shn_reads_fasta_file", ctx, bufs, off, path, [&](uint64_t r0, uint64_t r1, uint8_t* d_out, uint64_t bytes) {
    fasta_expand(J, r0, r1, d_out, bytes);
    fasta_model(J, e0 + r0, r1 - r0, bytes);
  }, bytes_out);
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
  ShnDevBufs bufs(ctx->stream);
  if ((rc = dict_plan(&J, bufs, text, off, weights))) return rc;
  const uint64_t bound = n * ((uint64_t)k1 + 12);                          // a weight has ten digits at the most
  uint64_t total = 0, dl = 0;
  rc = shn_expand_all(ctx, bufs, J.d_off, n, bound, out, cap, [&](uint8_t* d_text, uint64_t room) { dict_expand(J, 0, n, d_text, room, room); }, &total, &dl);
  if (rc) return rc;
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
  return expand_to_file("shn_k1mers_dict_file", ctx, bufs, roff, path,
                        [&](uint64_t r0, uint64_t r1, uint8_t* d_out, uint64_t bytes) { dict_expand(J, r0, r1, d_out, bytes, bytes); }, bytes_out);
}
