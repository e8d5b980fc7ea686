// The reads of one partition of the graph stage.  Host code only, included by mbgraph_host.hip alone (hence the unnamed namespace):
// how an entry point names the reads (ReadSource), the choice between the four ways of taking them in (choose_intake), the store
// the graph surgery reads them from with those four intake forms (PartitionReads), and the buffers of that store that are kept
// from call to call (ReadBuffers, ScratchLease).  The host-thread budget and the thread fan-out both sides use are here too.
#pragma once
#include "common.h"
#include "flatmap.h"
#include "graph_dev.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <sys/mman.h>
#include <thread>

namespace {
static inline int base_code(char c) {
  switch (c) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return -1; }
}
static inline bool all_acgt(const char* d, uint64_t n) {
  bool bad = false;
  for (uint64_t j = 0; j < n; j++) bad |= !(d[j] == 'A' || d[j] == 'C' || d[j] == 'G' || d[j] == 'T');     // (no early exit: it vectorises)
  return !bad;
}

// the stage's one clock and its one lap printer: "[mbgraph] <what> <seconds> s  <details>" (tools/sum_laps.py sums these by <what>)
static double tnow() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
__attribute__((format(printf, 4, 5))) static void lap_line(bool on, const char* what, double seconds, const char* fmt, ...) {
  if (!on) return;
  char details[256];
  va_list ap; va_start(ap, fmt); vsnprintf(details, sizeof details, fmt, ap); va_end(ap);
  fprintf(stderr, "[mbgraph] %-22s %8.3f s%s%s\n", what, seconds, details[0] ? "  " : "", details);
}

// several partitions run on host threads at once; every thread has a context / stream of its own (shn_thread_ctx, core.hip), the
// calls its GPU sections make use per-call or per-context buffers only, so the sections overlap on the device
// Host-thread budget shared by the partitions of a process.  The multi-threaded phases of a partition (read decode, duplicate
// search, numbering, path classification) take as many tokens as they start threads; with 64 partitions beginning at once and up
// to 32 threads each the cores were oversubscribed five-fold and every phase ran ten times slower than alone -- the largest
// partition, which bounds the stage, included.  Partitions are started largest first, so the large ones get their threads first.
struct ThreadBudget {
  std::mutex mu; std::condition_variable cv; int avail, total;
  ThreadBudget() { const int hw = shn_host_cpus(); avail = (int)shn_env_u64("SHN_GRAPH_HOST_THREADS", (uint64_t)std::max(4, hw), 1, 1u << 20); total = avail; }
  // large requests (the large partitions, which bound the stage) never wait -- they may overdraw the budget; small ones wait for it
  void acquire(int n) { n = std::min(n, total); std::unique_lock<std::mutex> lk(mu); if (n < 8) cv.wait(lk, [&] { return avail >= n; }); avail -= n; }
  void release(int n) { n = std::min(n, total); { std::lock_guard<std::mutex> lk(mu); avail += n; } cv.notify_all(); }
  // as many of the n wanted as are free right now (at least 1: the caller's own thread), without waiting and without overdrawing:
  // for phases that are worth spreading only when the machine is otherwise idle (the last, largest partition of a stage)
  // (the partitions that are running right now each keep a core busy themselves: `others`)
  int take_free(int n, int others) { std::lock_guard<std::mutex> lk(mu); const int got = std::max(1, std::min(n, avail - others)); avail -= got; return got; }
};
static std::atomic<int> g_partitions_running{0};      // partitions inside mbgraph_run right now
static std::atomic<int> g_host_intakes{0};            // of them, inside a host intake form (HostIntakeSlot)
static ThreadBudget g_host_threads;
struct BudgetGuard {
  int n; double waited;
  explicit BudgetGuard(int k) : n(k) { const double t0 = tnow(); g_host_threads.acquire(n); waited = tnow() - t0; }
  ~BudgetGuard() { g_host_threads.release(n); }
};
// the threads that are free right now for a phase that wants `want` (want <= 1: the caller's alone, nothing taken), given back at the end
struct FreeThreads {
  unsigned n, taken;
  explicit FreeThreads(unsigned want) : n(want > 1 ? (unsigned)g_host_threads.take_free((int)want, g_partitions_running.load() - 1) : 1u), taken(want > 1 ? n : 0u) {}
  ~FreeThreads() { if (taken) g_host_threads.release((int)taken); }
};

// fn(t) for every t in [0, nt): t = 0 on the calling thread, the others on threads of their own, all joined before the return
template <class F> static void run_on_threads(unsigned nt, F&& fn) {
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nt; t++) th.emplace_back([&fn, t] { fn(t); });
  fn(0u);
  for (auto& x : th) x.join();
}
// fn(lo, hi) over [0, n) cut into nt consecutive ranges of whole multiples of `align` (the last one ends at n)
template <class F> static void run_on_threads(unsigned nt, size_t n, F&& fn, size_t align = 1) {
  const size_t units = (n + align - 1) / align;
  nt = std::max(1u, nt);
  run_on_threads(nt, [&](unsigned t) { fn(std::min(n, units * t / nt * align), std::min(n, units * (t + 1) / nt * align)); });
}

// read string living in the interner arena (or in the lazily decoded text)
struct RStr {
  const char* p; size_t n;
  size_t size() const { return n; }
  const char& operator[](size_t i) const { return p[i]; }
  int compare(size_t pos, size_t len, const std::string& o) const {
    size_t m = std::min(len, n - pos);
    int c = memcmp(p + pos, o.data(), std::min(m, o.size()));
    if (c) return c;
    return m < o.size() ? -1 : (m > o.size() ? 1 : 0);
  }
};

// eight 2-bit codes (one per byte, all < 4) -> their letters: 'A' + 2 b0 + 6 b1 + 11 (b0 & b1) = A, C, G, T (no carry leaves a byte)
static inline uint64_t codes8_to_ascii(uint64_t x) {
  const uint64_t b0 = x & 0x0101010101010101ULL, b1 = (x >> 1) & 0x0101010101010101ULL;
  return 0x4141414141414141ULL + 2 * b0 + 6 * b1 + 11 * (b0 & b1);
}
static void decode_read(char* s, const uint8_t* p, uint64_t n, int enc, bool rc) {
  if (enc == SHN_ENC_CODES) {
    // eight bases at a time where all eight are ACGT (a byte >= 4 anywhere in the word: the word goes base by base)
    uint64_t i = 0;
    if (!rc) {
      for (; i + 8 <= n; i += 8) {
        uint64_t x; memcpy(&x, p + i, 8);
        if (x & 0xFCFCFCFCFCFCFCFCULL) { for (uint64_t j = i; j < i + 8; j++) s[j] = p[j] < 4 ? "ACGT"[p[j]] : 'N'; continue; }
        x = codes8_to_ascii(x); memcpy(s + i, &x, 8);
      }
      for (; i < n; i++) s[i] = p[i] < 4 ? "ACGT"[p[i]] : 'N';
    } else {
      for (; i + 8 <= n; i += 8) {
        uint64_t x; memcpy(&x, p + n - 8 - i, 8);
        if (x & 0xFCFCFCFCFCFCFCFCULL) { for (uint64_t j = i; j < i + 8; j++) { const uint8_t c = p[n - 1 - j]; s[j] = c < 4 ? "TGCA"[c] : 'N'; } continue; }
        x = codes8_to_ascii(__builtin_bswap64(0x0303030303030303ULL - x)); memcpy(s + i, &x, 8);
      }
      for (; i < n; i++) { uint8_t c = p[n - 1 - i]; s[i] = c < 4 ? "TGCA"[c] : 'N'; }
    }
  } else {
    auto up = [](uint8_t c) -> char { return (c >= 'a' && c <= 'z') ? (char)(c - 32) : (char)c; };
    if (!rc) for (uint64_t i = 0; i < n; i++) s[i] = up(p[i]);
    else for (uint64_t i = 0; i < n; i++) {
      char c = up(p[n - 1 - i]);
      s[i] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
    }
  }
}

// ---- how the caller names the reads of the partition
// r1 / r2 + offsets: text or codes (enc), n_reads of them (pairs if paired); rc1 / rc2 (optional, one byte per read): 1 = take the
// reverse complement of that read.  src_a / src_b (optional): the resident packed read sets of the run the reads are rows of, with
// didx / d_didx = the routed doubled read indices on the host / on the device (shn_route_reads' numbering: SE d < N -> R[d],
// d >= N -> RC(R[d-N]); PE d < N -> (R1[d], RC(R1[d])), d >= N -> (RC(R2[d-N]), R2[d-N])).  host_a / host_b (optional): the same
// sets as host code matrices [reads of the set][read length]; r1 / r2 are then not needed.
struct ReadSource {
  const uint8_t *r1 = nullptr, *r2 = nullptr, *rc1 = nullptr, *rc2 = nullptr;
  const uint64_t *r1_off = nullptr, *r2_off = nullptr;
  int enc = SHN_ENC_ASCII, paired = 0;
  uint64_t n_reads = 0;
  const shn_reads *src_a = nullptr, *src_b = nullptr;
  const uint32_t *didx = nullptr, *d_didx = nullptr;
  const uint8_t *host_a = nullptr, *host_b = nullptr;
  std::vector<uint32_t> didx_fetched;
  int nm() const { return paired ? 2 : 1; }                         // read slots per routed read: slot j = read i * nm + mate (0 / 1)
  // slot j as the caller gave it: its bytes (r1 / r2), their number, and whether the read is their reverse complement
  const uint8_t* slot(uint64_t j, uint64_t& n, bool& rc) const {
    const uint64_t i = j / nm();
    const bool second = j % nm();
    const uint64_t* off = second ? r2_off : r1_off;
    n = off[i + 1] - off[i]; rc = second ? rc2 && rc2[i] : rc1 && rc1[i];
    return (second ? r2 : r1) + off[i];
  }
  uint64_t read_len() const { return !n_reads ? 0 : host_a ? src_a->fixed_len : (uint64_t)(r1_off[1] - r1_off[0]); }   // of the first read
  // the routed list may be given by its place on the device only: a form that wants it on the host fetches it first
  int need_didx(shn_ctx* ctx) {
    if (didx || !d_didx || !n_reads) return 0;
    didx_fetched.resize(n_reads);
    hipError_t e_ = hipSetDevice(ctx->device);
    if (e_ == hipSuccess) e_ = hipMemcpy(didx_fetched.data(), d_didx, n_reads * 4, hipMemcpyDeviceToHost);
    if (e_ != hipSuccess) return shn_fail(SHN_ERR_HIP, std::string("shn_mbgraph_run_routes: ") + hipGetErrorString(e_));
    didx = didx_fetched.data();
    return 0;
  }
  // origin of slot j in the resident input, for the device gather of the distinct reads
  void origin_of(uint64_t j, uint32_t& row, uint8_t& flag) const {
    const uint64_t N_in = src_a->n_reads, i = j / nm();
    const int mate = (int)(j % nm());
    const uint64_t d = didx[i];
    const bool second = d >= N_in;
    row = (uint32_t)(second ? d - N_in : d);
    if (!paired) flag = second ? 2 : 0;
    else if (mate == 0) flag = second ? (1 | 2) : 0;              // R1[d] / RC(R2[d-N])
    else flag = second ? 1 : 2;                                     // RC(R1[d]) / R2[d-N]
  }
};

// ---- the four ways of taking the reads in, and the one place that picks among them (the only reader of the five switches below)
enum class IntakeForm {
  DeviceAttrs,       // distinct reads found on the device, their attributes left there (graph_dev.h), text decoded lazily from the rows
  DeviceDedup,       // distinct reads found on the device, attributes and text in host arrays
  HostParallel,      // host decode + hash, duplicates found and reads numbered on several threads
  HostSequential,    // host decode + hash, one read after the other through the interner
};
struct IntakePlan {
  IntakeForm form;
  bool resident;     // the reads are known as rows of the resident sets: the device copy of the distinct reads is gathered from those
  bool lazy;         // DeviceDedup: the text is decoded from the host matrices when asked for (DeviceAttrs: always)
  unsigned threads;  // the host forms' decode (and numbering) threads
};
// a partition's place among the host intakes running in this process: taken (counted and numbered in one step) by choose_intake
// when it picks a host form, left by the driver when the reads are loaded
struct HostIntakeSlot {
  int n = 0;
  int enter() { return n = ++g_host_intakes; }
  void leave() { if (n) { --g_host_intakes; n = 0; } }
  ~HostIntakeSlot() { leave(); }
};
static IntakePlan choose_intake(const ReadSource& s, shn_ctx* ctx, int K, uint64_t cutoff, HostIntakeSlot& slot) {
  IntakePlan p{IntakeForm::HostSequential, false, false, 1};
  const uint64_t used = std::min<uint64_t>(s.n_reads, cutoff + 1), nh = used * s.nm();
  p.resident = ctx && s.src_a && (s.didx || s.d_didx) && s.src_a->fixed_len && (!s.paired || (s.src_b && s.src_b->fixed_len == s.src_a->fixed_len)) &&
               s.n_reads && s.read_len() == s.src_a->fixed_len && (s.host_a || !shn_env_set("SHN_GRAPH_RESIDENT_READS"));
  // the distinct reads found on the device: with the host matrices always, with gathered rows for large sets
  const char* bulk_set = shn_env_str("SHN_GRAPH_BULK_MIN");
  const uint64_t bulk_min = bulk_set ? strtoull(bulk_set, nullptr, 10) : 1u << 17;     // reads from which the duplicates are found in parallel (tests lower it)
  const bool dev_dedup = p.resident && (s.host_a || (shn_env_flag("SHN_GRAPH_DEVICE_DEDUP", true) && s.enc == SHN_ENC_CODES && nh >= bulk_min));
  p.lazy = s.host_a && shn_env_flag("SHN_GRAPH_LAZY_TEXT", true) && s.src_a && s.src_a->n_invalid == 0 && (!s.paired || (s.src_b && s.src_b->n_invalid == 0));
  // the fast form of the rows mode (graph_dev.h): the duplicate search leaves its arrays on the device, the host gets rows + strands
  // (for the lazily decoded text) and nothing else per read.  SHN_GRAPH_DEV_ATTRS=0: the host-array form.
  if (dev_dedup && p.lazy && K <= 31 && shn_env_flag("SHN_GRAPH_DEV_ATTRS", true)) { p.form = IntakeForm::DeviceAttrs; return p; }
  if (dev_dedup) { p.form = IntakeForm::DeviceDedup; return p; }
  // (8 ranks share a node's cores; partitions running at the same time in this process share this rank's part)
  // The partitions of a run differ in size by an order of magnitude and the largest ones are started first (pipeline.py): the
  // stage ends when the largest partition does, so its read set gets threads in proportion to its size (one per 256 Ki
  // reads, at most 32 and at most a quarter of the cores), whatever else is running; small sets share what is left.
  const unsigned hwc = (unsigned)shn_host_cpus();
  const int active = slot.enter();
  unsigned nt = std::min<unsigned>(32, std::max<unsigned>(1, hwc / 8 / (unsigned)std::max(1, active / 2)));
  nt = std::max<unsigned>(nt, (unsigned)std::min<uint64_t>(std::min<uint64_t>(32, std::max(1u, hwc / 2)), nh >> 18));
  if (bulk_set) nt = std::max(nt, 4u);
  if (nh < bulk_min) nt = used < 4096 ? 1 : std::min<unsigned>(nt, (unsigned)(used / 2048));   // small sets: a few threads for the decode only
  p.threads = nt;
  if (nt > 1 && nh >= bulk_min) p.form = IntakeForm::HostParallel;
  return p;
}

// the buffer of the lazily decoded read text: NOT a vector -- it is written piecemeal (a few per cent of the reads are ever
// decoded), and a vector's resize zero-filled all of it: 0.1 s for the 354 MB of the largest partition whenever it got a
// scratch object that had served a smaller one (the spread of the graph stage from step to step)
struct LazyTextBuffer {
  char* raw = nullptr; size_t cap = 0;
  // (moved, never copied: ReadBuffers goes to a lease and back as a whole)
  LazyTextBuffer& operator=(LazyTextBuffer&& o) noexcept { std::swap(raw, o.raw); std::swap(cap, o.cap); return *this; }
  ~LazyTextBuffer() { free(raw); }
  char* room(size_t bytes) {
    if (bytes > cap) { free(raw); raw = (char*)malloc(bytes + bytes / 8); cap = raw ? bytes + bytes / 8 : 0; }
    return raw;
  }
};

// transparent huge pages for the large scratch buffers (THP in madvise mode)
static void huge_pages(const void* p, size_t bytes) {
  if (bytes < (8u << 20)) return;
  const uintptr_t a = ((uintptr_t)p + 4095) & ~(uintptr_t)4095, e = ((uintptr_t)p + bytes) & ~(uintptr_t)4095;
  if (e > a) madvise((void*)a, e - a, MADV_HUGEPAGE);
}

// Scratch kept between calls (at the read cap these buffers are 100s of MB, and fresh pages cost more than the work done
// in them): decode buffers and the read arena.  (also the per-read arrays of the graph: a partition at the read cap touches
// ~1.5 GB here, and with 64 partitions starting at once the page faults of fresh memory were most of the largest partition's
// "load reads".)  This is the list of what is kept, written once: a ScratchLease moves the whole object into PartitionReads
// and back, so a per-read array added here is leased with the others.
struct ReadBuffers {
  // work arrays of the intake forms (left as the last call left them: every form sizes what it uses)
  std::vector<uint64_t> doff, hashes; std::vector<char> text; std::vector<uint32_t> first, cnt, last; std::vector<int32_t> idmap; std::vector<uint8_t> role;
  // per distinct read
  std::vector<double> rcc;              // copies
  std::vector<int> rmate, rmp;          // rmp: 0 None, 1, 2
  std::vector<int> rfirst, rlast;       // first / last node of the read's (last) path: all find_mate_pairs reads of Read.nodes
  std::vector<char> rhas;
  StringInterner rindex;                // (sized by forget_reads when a lease hands the buffers over)
  std::vector<uint32_t> origin_row;     // row in its resident set, and
  std::vector<uint8_t> origin_flag;     // bit 0: set b, bit 1: reverse complement
  LazyTextBuffer lazy_text;
  size_t room() const { return std::max(std::max(text.capacity(), rindex.arena.capacity()), lazy_text.cap); }
  // no reads, capacity kept (origin_*: empty until a form fills them)
  void forget_reads() {
    rindex.reset(1 << 16);
    rcc.clear(); rmate.clear(); rmp.clear(); rfirst.clear(); rlast.clear(); rhas.clear(); origin_row.clear(); origin_flag.clear();
  }
};

struct PartitionReads : ReadBuffers {
  bool laps = false;                        // print the time of every phase (SHN_DEBUG / SHN_GRAPH_LAPS)
  const shn_reads *src_a = nullptr, *src_b = nullptr;      // the resident input read sets the partition's reads are rows of
  // Lazy read text (reads named by rows of the host code matrices, shn_mbgraph_run_rows): nearly every read is settled on the
  // device (distinct reads, bridging seeds, the in-node test of known_paths); the text of a read is decoded from its row the first
  // time host code asks for it -- bridging hits, reads that run past their node: a few per cent of the reads.  Host code that reads
  // text from several threads calls ensure_all_text() first.
  const uint8_t *lz_a = nullptr, *lz_b = nullptr;      // the host code matrices
  uint32_t lz_L = 0;                                   // the read length
  char* lz_buf = nullptr;                              // the text (ReadBuffers::lazy_text), a read decoded where its bit is set in
  mutable std::vector<uint64_t> lz_done;
  // device-resident read attributes (graph_dev.h): copies, mates, roles, known-path states stay on the device; the host vectors
  // rcc / rmate / rmp / rfirst / rlast / rhas are then EMPTY until need_host_attrs() fetches them for a host form that wants them
  shn_dedup* dd = nullptr;
  bool dev_attrs = false;
  size_t n_rd_dev = 0;
  int acgt_known = -1;        // set while the reads are loaded (a scan of the arena is 10s of ms at the read cap); -1 = scan
  ~PartitionReads() { if (dd) shn_dedup_destroy(dd); }
  size_t n_rd() const { return dev_attrs || dd ? n_rd_dev : rindex.size(); }
  size_t len(int r) const { return lz_buf ? (size_t)lz_L : rindex.len(r); }
  const uint8_t* lazy_row(int r) const { return ((origin_flag[r] & 1) ? lz_b : lz_a) + (uint64_t)origin_row[r] * lz_L; }
  void decode_lazy(int r) const {
    decode_read(lz_buf + (size_t)r * lz_L, lazy_row(r), lz_L, SHN_ENC_CODES, (origin_flag[r] & 2) != 0);
    // (several threads may ask for text at once -- the X-nodes of a bridging pass: two of them decoding one read write the same
    // bytes; the bit is set after the text, with release / acquire order)
    __atomic_fetch_or(&lz_done[(size_t)r >> 6], 1ULL << (r & 63), __ATOMIC_RELEASE);
  }
  bool lz_has(size_t r) const { return (__atomic_load_n(&lz_done[r >> 6], __ATOMIC_ACQUIRE) >> (r & 63)) & 1; }
  void ensure_all_text() const {
    if (!lz_buf) return;
    const size_t n = n_rd();
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(std::max(1, shn_host_cpus() / 2), n >> 16));
    // (whole 64-read words per thread: the done bits are not shared)
    run_on_threads(nt, n, [&](size_t lo, size_t hi) { for (size_t r = lo; r < hi; r++) if (!lz_has(r)) decode_lazy((int)r); }, 64);
  }
  RStr rstr(int r) const {
    if (!lz_buf) return RStr{rindex.data(r), rindex.len(r)};
    if (!lz_has((size_t)r)) decode_lazy(r);
    return RStr{lz_buf + (size_t)r * lz_L, lz_L};
  }
  // the text of read r is about to be asked for: its cache lines (or, not yet decoded, the lines of its row) on their way
  void prefetch_read(int r) const {
    if (!lz_buf) { __builtin_prefetch(rindex.data(r)); return; }
    const char* t = lz_has((size_t)r) ? lz_buf + (size_t)r * lz_L : (const char*)lazy_row(r);
    __builtin_prefetch(t); __builtin_prefetch(t + 64);
  }
  bool text_all_acgt() {
    if (acgt_known < 0) acgt_known = all_acgt(rindex.arena.data(), rindex.arena.size());
    return acgt_known == 1;
  }
  int need_host_attrs() {
    if (!dev_attrs) return 0;
    const size_t nd = n_rd_dev;
    std::vector<uint32_t> c(nd); std::vector<int32_t> m(nd); std::vector<uint8_t> ro(nd);
    int rc = shn_dedup_attrs(dd, c.data(), m.data(), ro.data());
    if (rc) return rc;
    rcc.resize(nd); rmate.resize(nd); rmp.resize(nd); rfirst.assign(nd, -1); rlast.assign(nd, -1); rhas.assign(nd, 0);
    for (size_t i = 0; i < nd; i++) { rcc[i] = (double)c[i]; rmate[i] = m[i]; rmp[i] = ro[i]; }
    dev_attrs = false;
    return 0;
  }
  int add_read(const char* b, size_t n, uint64_t h) {
    bool is_new = false;
    int r = rindex.intern_hashed(b, n, h, &is_new);
    if (!is_new) { rcc[r] += 1.0; return r; }
    rcc.push_back(1.0); rmate.push_back(-1); rmp.push_back(0); rfirst.push_back(-1); rlast.push_back(-1); rhas.push_back(0);
    return r;
  }

  // ---- intake: the first `used` routed reads of `s` (the read cap is the caller's), by the plan choose_intake made for them
  int load(shn_ctx* ctx, ReadSource& s, uint64_t used, const IntakePlan& plan) {
    if (plan.resident) { src_a = s.src_a; src_b = s.paired ? s.src_b : nullptr; }
    switch (plan.form) {
      case IntakeForm::DeviceAttrs: return load_device_attrs(ctx, s, used);
      case IntakeForm::DeviceDedup: return load_device_dedup(ctx, s, used, plan);
      default: return load_host(ctx, s, used, plan);
    }
  }
  int lazy_text_from(const ReadSource& s, uint64_t nd) {
    lz_a = s.host_a; lz_b = s.host_b; lz_L = (uint32_t)s.read_len(); lz_buf = lazy_text.room(nd * lz_L + 1);
    if (!lz_buf) return shn_fail(SHN_ERR_NOMEM, "shn_mbgraph_run: out of host memory for the reads' text");
    lz_done.assign((nd + 63) / 64, 0);
    return 0;
  }
  int load_device_attrs(shn_ctx* ctx, const ReadSource& s, uint64_t used) {
    const double t_dec = tnow();
    int rc = shn_reads_dedup_dev(ctx, s.src_a, s.paired ? s.src_b : nullptr, s.didx, s.d_didx, used, s.paired, &dd);
    if (rc) return rc;
    const uint64_t nd = dd->n_distinct;
    n_rd_dev = nd; dev_attrs = true;
    lap_line(laps, "  distinct reads (GPU)", tnow() - t_dec, "used=%llu distinct=%llu (attributes stay on the device)", (unsigned long long)used, (unsigned long long)nd);
    if ((rc = lazy_text_from(s, nd))) return rc;
    origin_row.resize(nd); origin_flag.resize(nd);
    if ((rc = shn_dedup_origin(dd, origin_row.data(), origin_flag.data()))) return rc;
    acgt_known = 1;
    lap_line(laps, "  + rows of the distinct", tnow() - t_dec, "%s", "");
    return 0;
  }
  int load_device_dedup(shn_ctx* ctx, ReadSource& s, uint64_t used, const IntakePlan& plan) {
    int rc = s.need_didx(ctx);
    if (rc) return rc;
    const uint64_t nh = used * s.nm(), Lr = s.read_len();
    const double t_dec = tnow();
    std::vector<uint32_t>& slot = first; std::vector<int32_t>& mate = idmap;
    slot.resize(nh); cnt.resize(nh); mate.resize(nh); role.resize(nh);
    uint64_t nd = 0;
    rc = shn_reads_dedup(ctx, s.src_a, s.paired ? s.src_b : nullptr, s.didx, used, s.paired, &nd, slot.data(), cnt.data(), mate.data(), role.data());
    if (rc) return rc;
    lap_line(laps, "  distinct reads (GPU)", tnow() - t_dec, "used=%llu distinct=%llu", (unsigned long long)used, (unsigned long long)nd);
    StringInterner& R = rindex;
    R.hashes.assign(nd, 0);
    const bool lazy = plan.lazy;
    if (lazy && (rc = lazy_text_from(s, nd))) return rc;
    R.off.resize(nd + 1);
    if (!lazy) { if (R.arena.capacity() < nd * Lr) { R.arena.reserve(nd * Lr); huge_pages(R.arena.data(), nd * Lr); } R.arena.resize(nd * Lr); }
    rcc.resize(nd); rmate.resize(nd); rmp.resize(nd); rfirst.assign(nd, -1); rlast.assign(nd, -1); rhas.assign(nd, 0);
    origin_row.resize(nd); origin_flag.resize(nd);
    const unsigned hwc = (unsigned)shn_host_cpus();
    const unsigned nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(32, std::max(1u, hwc / 2)), nd >> 15));
    BudgetGuard budget((int)nt);
    std::atomic<int> non_acgt{0};
    char* arena = lazy ? nullptr : &R.arena[0];
    R.off[0] = 0;
    run_on_threads(nt, nd, [&](size_t lo, size_t hi) {
      bool bad = false;
      for (uint64_t id = lo; id < hi; id++) {
        const uint64_t j = slot[id];
        uint32_t row; uint8_t fl;
        s.origin_of(j, row, fl);
        origin_row[id] = row; origin_flag[id] = fl;
        rcc[id] = (double)cnt[id]; rmate[id] = mate[id]; rmp[id] = role[id];
        if (lazy) continue;
        uint64_t n_; bool rc_ = (fl & 2) != 0;
        const uint8_t* p = s.host_a ? ((fl & 1) ? s.host_b : s.host_a) + (uint64_t)row * Lr : s.slot(j, n_, rc_);
        char* d = arena + id * Lr;
        decode_read(d, p, Lr, s.host_a ? SHN_ENC_CODES : s.enc, rc_);
        bad |= !all_acgt(d, Lr);
        R.off[id + 1] = (id + 1) * Lr;
      }
      if (bad) non_acgt.store(1);
    });
    if (non_acgt.load()) return shn_fail(SHN_ERR_ARG, "shn_mbgraph_run: a routed read holds a base outside ACGT (the packed rows cannot tell such reads apart)");
    acgt_known = 1;
    R.bulk_loaded = true;
    lap_line(laps, "  + text of the distinct", tnow() - t_dec, "nt=%u (waited %.3f s for threads)", nt, budget.waited);
    return 0;
  }
  // the two host forms: decode + hash on several host threads (independent per read), then the reads are numbered in file order
  int load_host(shn_ctx* ctx, ReadSource& s, uint64_t used, const IntakePlan& plan) {
    const int nm = s.nm();
    const uint64_t nh = used * nm;
    doff.resize((size_t)nh + 1);
    doff[0] = 0;
    for (uint64_t j = 0; j < nh; j++) { uint64_t n; bool rc_; s.slot(j, n, rc_); doff[j + 1] = doff[j] + n; }
    rindex.arena.reserve(doff.back());
    if (nh < (1u << 17)) rindex.reserve(nh);          // (large sets are numbered in bulk and never use the interner's probe table)
    rcc.reserve(nh); rmate.reserve(nh); rmp.reserve(nh); rfirst.reserve(nh); rlast.reserve(nh); rhas.reserve(nh);
    int rc = s.need_didx(ctx);
    if (rc) return rc;
    if (text.size() < doff.back() + 1) { text.clear(); text.reserve(doff.back() + 1); huge_pages(text.data(), text.capacity()); text.resize(doff.back() + 1); }
    if (hashes.capacity() < (size_t)nh) { hashes.clear(); hashes.reserve((size_t)nh); huge_pages(hashes.data(), hashes.capacity() * 8); }
    hashes.resize((size_t)nh);
    huge_pages(rindex.arena.data(), rindex.arena.capacity());
    const double t_dec = tnow();
    const unsigned nt = plan.threads;
    BudgetGuard budget((int)nt);                          // held until the reads are numbered
    std::atomic<int> non_acgt{0};
    run_on_threads(nt, (size_t)used, [&](size_t lo, size_t hi) {
      bool bad = false;
      for (uint64_t j = lo * nm; j < hi * nm; j++) {
        uint64_t n; bool rc_;
        const uint8_t* p = s.slot(j, n, rc_);
        char* d = text.data() + doff[j];
        decode_read(d, p, n, s.enc, rc_);
        bad |= !all_acgt(d, n);
        hashes[j] = StringInterner::hash(d, n);
      }
      if (bad) non_acgt.store(1);
    });
    acgt_known = non_acgt.load() ? 0 : 1;
    lap_line(laps, "  offsets+decode+hash", tnow() - t_dec, "used=%llu nt=%u (waited %.3f s for threads)", (unsigned long long)used, nt, budget.waited);
    if (plan.form == IntakeForm::HostParallel) number_in_parallel(s, used, nt, plan.resident, t_dec);
    else number_one_by_one(s, used, plan.resident);
    return 0;
  }
  // Large read sets, all on `nt` host threads: (1) the duplicates -- every thread owns the strings whose hash falls into
  // its shard (private open-addressing table: string -> index of its first occurrence, with its number of occurrences
  // and its last occurrence); (2) ids in file order of first occurrence = a prefix sum over the "first occurrence"
  // flags, the strings copied to their place in the arena in parallel; (3) every read's id; (4) mates: interning one
  // pair after the other leaves every read with the role and mate of its LAST occurrence.  Same ids, counts and mates
  // as reading one read at a time (test_native_graph_stage_parallel_read_dedup).
  void number_in_parallel(const ReadSource& s, uint64_t used, unsigned nt, bool resident, double t_dec) {
    const uint64_t nh = used * s.nm();
    first.resize(nh); cnt.resize(nh); last.resize(nh);
    run_on_threads(nt, [&](unsigned t) {
      size_t cap = 1024;                                      // shards of a hash are even: 2.5x the mean share is ample
      while (cap < (nh / nt + 1) * 5 / 2) cap <<= 1;
      std::vector<uint32_t> tab(cap, 0xFFFFFFFFu);
      uint64_t used_slots = 0;
      for (uint64_t j = 0; j < nh; j++) {
        const uint64_t h = hashes[j];
        if (((h >> 40) % nt) != t) continue;
        if (used_slots * 10 > cap * 8) {                       // (a pathological hash distribution: grow and re-insert)
          std::vector<uint32_t> old;
          old.swap(tab);
          cap <<= 1;
          tab.assign(cap, 0xFFFFFFFFu);
          for (uint32_t q : old) if (q != 0xFFFFFFFFu) { size_t sl = (size_t)hashes[q] & (cap - 1); while (tab[sl] != 0xFFFFFFFFu) sl = (sl + 1) & (cap - 1); tab[sl] = q; }
        }
        const size_t m = cap - 1;
        const char* p = text.data() + doff[j];
        const uint64_t n = doff[j + 1] - doff[j];
        size_t sl = (size_t)h & m;
        while (true) {
          const uint32_t q = tab[sl];
          if (q == 0xFFFFFFFFu) { tab[sl] = (uint32_t)j; first[j] = (uint32_t)j; cnt[j] = 1; last[j] = (uint32_t)j; used_slots++; break; }
          if (hashes[q] == h && doff[q + 1] - doff[q] == n && memcmp(text.data() + doff[q], p, n) == 0) { first[j] = q; cnt[q]++; last[q] = (uint32_t)j; break; }
          sl = (sl + 1) & m;
        }
      }
    });
    lap_line(laps, "  + duplicates found", tnow() - t_dec, "used=%llu", (unsigned long long)used);
    idmap.resize(nh);
    StringInterner& R = rindex;
    // (2) chunk c of the reads: how many first occurrences, how many bytes
    std::vector<uint64_t> nf(nt + 1, 0), nbytes(nt + 1, 0);
    auto lo_of = [&](unsigned c) { return nh * c / nt; };
    run_on_threads(nt, [&](unsigned c) {
      uint64_t f = 0, by = 0;
      for (uint64_t j = lo_of(c); j < lo_of(c + 1); j++) if (first[j] == (uint32_t)j) { f++; by += doff[j + 1] - doff[j]; }
      nf[c + 1] = f; nbytes[c + 1] = by;
    });
    for (unsigned c = 0; c < nt; c++) { nf[c + 1] += nf[c]; nbytes[c + 1] += nbytes[c]; }
    const uint64_t nd = nf[nt];
    R.hashes.resize(nd);
    R.off.resize(nd + 1);
    R.off[0] = 0;
    R.arena.resize(nbytes[nt]);
    rcc.resize(nd); rmate.resize(nd, -1); rmp.resize(nd, 0); rfirst.resize(nd, -1); rlast.resize(nd, -1); rhas.resize(nd, 0);
    if (resident) { origin_row.resize(nd); origin_flag.resize(nd); }
    char* arena = &R.arena[0];
    run_on_threads(nt, [&](unsigned c) {
      uint64_t id = nf[c], at = nbytes[c];
      for (uint64_t j = lo_of(c); j < lo_of(c + 1); j++) {
        if (first[j] != (uint32_t)j) continue;
        const uint64_t n = doff[j + 1] - doff[j];
        memcpy(arena + at, text.data() + doff[j], n);
        at += n;
        R.hashes[id] = hashes[j];
        R.off[id + 1] = at;
        rcc[id] = (double)cnt[j];
        idmap[j] = (int32_t)id;
        if (resident) s.origin_of(j, origin_row[id], origin_flag[id]);
        id++;
      }
    });
    run_on_threads(nt, [&](unsigned c) {                                  // (3) (a first occurrence precedes its duplicates, all are numbered by now)
      for (uint64_t j = lo_of(c); j < lo_of(c + 1); j++) if (first[j] != (uint32_t)j) idmap[j] = idmap[first[j]];
    });
    if (s.paired)
      run_on_threads(nt, [&](unsigned c) {                                // (4)
        for (uint64_t j = lo_of(c); j < lo_of(c + 1); j++) {
          if (first[j] != (uint32_t)j) continue;
          const uint32_t l = last[j];
          const int32_t id = idmap[j];
          rmp[id] = (l & 1) ? 2 : 1;
          rmate[id] = idmap[l ^ 1u];
        }
      });
    R.bulk_loaded = true;                 // (its probe table was bypassed: no interning by string after this)
    lap_line(laps, "  + numbered in order", tnow() - t_dec, "used=%llu", (unsigned long long)used);
  }
  void number_one_by_one(const ReadSource& s, uint64_t used, bool resident) {
    int a = -1;                                                         // the read before: the first mate when j is a second one
    for (uint64_t j = 0; j < used * s.nm(); j++) {
      const int r = add_read(text.data() + doff[j], doff[j + 1] - doff[j], hashes[j]);
      if (resident && (size_t)r == origin_row.size()) { uint32_t row; uint8_t fl; s.origin_of(j, row, fl); origin_row.push_back(row); origin_flag.push_back(fl); }
      if (s.paired && (j & 1)) { rmp[a] = 1; rmp[r] = 2; rmate[a] = r; rmate[r] = a; }
      a = r;
    }
  }
};

// A partition's ReadBuffers for the length of one call.  A free list, not thread_local: Python's partition workers are
// short-lived.  The list keeps one object per partition thread; a call takes the smallest one that is large enough for
// `need_text` bytes of read text, else the largest, and hands it back with the reads forgotten and the capacity kept.
class ScratchLease {
  struct Pool { std::mutex mu; std::vector<ReadBuffers*> free; };
  static Pool& pool() { static Pool p; return p; }
  PartitionReads& reads; ReadBuffers* held = nullptr;
 public:
  ScratchLease(PartitionReads& r, size_t need_text) : reads(r) {
    Pool& P = pool();
    { std::lock_guard<std::mutex> lk(P.mu);
      int pick = -1;
      for (size_t i = 0; i < P.free.size(); i++) {
        const size_t c = P.free[i]->room();
        if (pick < 0) { pick = (int)i; continue; }
        const size_t pc = P.free[pick]->room();
        if (pc >= need_text ? (c >= need_text && c < pc) : c > pc) pick = (int)i;
      }
      if (pick >= 0) { held = P.free[pick]; P.free.erase(P.free.begin() + pick); } }
    if (!held) held = new ReadBuffers();
    static_cast<ReadBuffers&>(reads) = std::move(*held);
    reads.forget_reads();
  }
  ScratchLease(const ScratchLease&) = delete;
  ~ScratchLease() {
    *held = std::move(static_cast<ReadBuffers&>(reads));
    std::vector<int32_t>().swap(held->rindex.table);       // (the interner's probe table is not kept: 0.5 MB and more per object)
    Pool& P = pool();
    std::lock_guard<std::mutex> lk(P.mu);
    if (P.free.size() < 192) P.free.push_back(held); else delete held;
  }
};

}  // namespace
