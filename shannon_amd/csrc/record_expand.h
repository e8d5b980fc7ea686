// Records of any lengths written one after the other: the per-thread half of shn_reads_collect (reads_collect.hip: reads as base
// codes) and of the --inDisk formatters (reads_text.hip: reads*.fasta, k1mer.dict).  All three run the same three passes:
//   1. lengths     one thread per record (code_len / fasta_len / dict_len below);
//   2. offsets     the library's exclusive scan (shn_device_scan_u32);
//   3. expansion   one thread per ALIGNED 16-byte chunk of the output (expand_chunk): it finds the record its first byte belongs to
//                  by a search in the offsets (the block's first and last chunk search all of them, the threads between search what
//                  lies between the two: record_expand_dev.h), then walks the records' bytes -- a read's bases from whole 64-bit
//                  words of d_words / d_mask, kept in a register while the chunk stays inside them (ReadCursor) -- and issues one
//                  16-byte store.  The work of a 250-base read spreads over 16 lanes, a 30-base read shares a lane with its
//                  neighbours: no lane waits for a long record.
// Plain C++ behind one qualifier: hipcc compiles it into the kernels, any C++ compiler into tools/expand_host_check.cpp, which runs
// every chunk under sanitizers with arrays of exactly the sizes the calls allocate.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SHN_XHD __host__ __device__ __forceinline__
#else
#define SHN_XHD inline
#endif

constexpr int SHN_XBLK = 256;        // threads per block of every pass
constexpr int SHN_XCHUNK = 16;       // output bytes per thread of the expansion

// a resident read set as the kernels see it (view_of(const shn_reads*): record_expand_dev.h)
struct ReadSetView {
  const uint64_t* words;
  const uint64_t* mask;      // nullptr: the set holds no base outside ACGT
  const uint64_t* woff;      // ragged: word offset of every read
  const uint32_t* len;       // ragged: length of every read (nullptr: fixed_len)
  uint64_t n;
  uint32_t fixed_len, wpr;
  SHN_XHD uint64_t word_base(uint64_t r) const { return len ? woff[r] : r * wpr; }
};

// the bases of one packed read: 0..3, or 4 where the set's mask says "outside ACGT" (MASK: some set of the call has a mask).  At
// most one load per 64-bit word while the positions asked for stay inside it.  A reverse complement is the caller's: base p of it
// is code(len - 1 - p), and 3 - that unless it is 4.
template <bool MASK>
struct ReadCursor {
  const uint64_t *words, *mask;
  uint64_t wbase, cw, cm, w, m;
  SHN_XHD void open(const ReadSetView& S, uint64_t word_base) { words = S.words; mask = S.mask; wbase = word_base; cw = cm = ~0ULL; w = m = 0; }
  SHN_XHD uint32_t code(uint32_t p) {
    const uint64_t wi = wbase + (p >> 5);
    if (wi != cw) { cw = wi; w = words[wi]; }
    if (MASK) {
      if (mask) {
        const uint64_t mi = (wbase >> 1) + (p >> 6);
        if (mi != cm) { cm = mi; m = mask[mi]; }
        if ((m >> (63 - (p & 63))) & 1) return 4;
      }
    }
    return (uint32_t)(w >> (62 - 2 * (p & 31))) & 3;
  }
};

// length of read r of set A or (second) B -- field by field: a reference chosen between two kernel arguments costs scratch
SHN_XHD uint32_t read_len(const ReadSetView& A, const ReadSetView& B, bool second, uint64_t r) {
  const uint32_t* len = second ? B.len : A.len;
  return len ? len[r] : (second ? B.fixed_len : A.fixed_len);
}

// largest i in [lo, hi) with off[i] <= pos (off[lo] <= pos is the caller's)
SHN_XHD uint64_t record_of(const uint64_t* off, uint64_t lo, uint64_t hi, uint64_t pos) {
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

struct alignas(16) Chunk16 { uint64_t lo, hi; };

// One thread of the expansion: bytes [pos0, pos0 + 16) of the output (pos0 a multiple of 16, below `total`) of records 0 .. n - 1
// of `rec`, whose byte offsets are off[0 .. n]; the output starts at off[0].  `total` = min(off[n] - off[0], capacity of out):
// nothing is written at or behind it.  [first, last] holds the record of byte pos0 (the block's first and last record).  Records
// without a byte are allowed: the search leaves them below the record it returns, the walk steps over them.
// R: enter(i, reclen) makes record i the current one, at(q) is its byte q.
template <class R>
SHN_XHD void expand_chunk(R& rec, uint64_t n, const uint64_t* off, uint64_t first, uint64_t last, uint64_t total, uint64_t pos0, uint8_t* out) {
  (void)n;                                      // (pos < total <= off[n] - off[0] below: i stays below n)
  const uint64_t base = off[0];
  uint64_t i = record_of(off, first, last + 1, base + pos0);                 // off[i] <= base + pos0 < off[i + 1]
  uint64_t start = off[i] - base, end = off[i + 1] - base;
  rec.enter(i, (uint32_t)(end - start));
  const uint32_t cnt = total - pos0 < (uint64_t)SHN_XCHUNK ? (uint32_t)(total - pos0) : (uint32_t)SHN_XCHUNK;
  uint64_t lo = 0, hi = 0;
  for (uint32_t j = 0; j < cnt; j++) {
    const uint64_t pos = pos0 + j;
    while (pos >= end) {
      i++; start = end; end = off[i + 1] - base;
      rec.enter(i, (uint32_t)(end - start));
    }
    const uint64_t ch = rec.at((uint32_t)(pos - start));
    if (j < 8) lo |= ch << (8 * j); else hi |= ch << (8 * (j - 8));
  }
  if (cnt == SHN_XCHUNK) *reinterpret_cast<Chunk16*>(out + pos0) = Chunk16{lo, hi};
  else for (uint32_t j = 0; j < cnt; j++) out[pos0 + j] = (uint8_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xff);      // (the last chunk of the output)
}

// ---- shn_reads_collect: read sel[i] of set a (flags[i] = 0) or b (1) as base codes
SHN_XHD uint32_t code_len(const ReadSetView& A, const ReadSetView& B, const uint32_t* sel, const uint8_t* flags, uint64_t i) {
  return read_len(A, B, flags[i] & 1, sel[i]);
}
template <bool MASK>
struct CodeRec {
  ReadSetView A, B;
  const uint32_t* sel;
  const uint8_t* flags;
  ReadCursor<MASK> cur;
  SHN_XHD void enter(uint64_t i, uint32_t) {
    const ReadSetView& S = (flags[i] & 1) ? B : A;
    cur.open(S, S.word_base(sel[i]));
  }
  SHN_XHD uint8_t at(uint32_t q) { return (uint8_t)cur.code(q); }
};

// ---- decimal numbers
SHN_XHD uint32_t dec_digits(uint64_t v) {
  uint32_t d = 1;
  while (v >= 10) { v /= 10; d++; }
  return d;
}
// a number as decimal digits, four bits each: digit k from the right in lo (k < 16) / hi
SHN_XHD void dec_set(uint64_t v, uint64_t& lo, uint64_t& hi, uint32_t& dig) {
  lo = hi = 0; dig = 0;
  do {
    const uint64_t q = v / 10, d = v - q * 10;
    if (dig < 16) lo |= d << (4 * dig); else hi |= d << (4 * (dig - 16));
    dig++; v = q;
  } while (v);
}
SHN_XHD uint8_t dec_char(uint64_t lo, uint64_t hi, uint32_t k) {
  return (uint8_t)('0' + ((k < 16 ? lo >> (4 * k) : hi >> (4 * (k - 16))) & 15));
}

// ---- records of reads*.fasta: '>' name [_1 | _2] '\n' bases '\n'
// which read a route entry names (include/shannon_hip.h, the table at shn_reads_fasta; kfc.ReadStore.mate1 / mate2)
struct ReadPick {
  uint64_t n_a;              // N: reads of set a
  int ss, mate;
  SHN_XHD bool operator()(const ReadSetView& A, const ReadSetView& B, uint64_t d, bool& second, uint64_t& r, bool& rc) const {
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
// *ok = false for a route outside the read sets: an empty sequence here, SHN_ERR_ARG from the call
SHN_XHD uint32_t fasta_len(const ReadSetView& A, const ReadSetView& B, const ReadPick& pick, const uint32_t* ridx, uint64_t e0, uint64_t i, bool* ok) {
  bool second, rc; uint64_t r;
  *ok = pick(A, B, ridx[i], second, r, rc);
  const uint32_t len = *ok ? read_len(A, B, second, r) : 0;
  return 1 + dec_digits(e0 + i) + (pick.mate ? 2 : 0) + 1 + len + 1;
}
template <bool MASK>
struct FastaRec {
  ReadSetView A, B;
  ReadPick pick;
  const uint32_t* ridx;
  uint64_t e0;
  // the current record
  ReadCursor<MASK> cur;
  uint64_t dlo, dhi;
  uint32_t len, H, dig;
  bool rc;
  SHN_XHD void enter(uint64_t i, uint32_t reclen) {
    bool second; uint64_t r;
    const bool ok = pick(A, B, ridx[i], second, r, rc);
    const ReadSetView& S = second ? B : A;
    cur.open(S, ok ? S.word_base(r) : 0);
    dec_set(e0 + i, dlo, dhi, dig);
    H = 1 + dig + (pick.mate ? 2 : 0) + 1;
    len = reclen - H - 1;                       // (0 for a route outside the sets: nothing of them is read)
  }
  SHN_XHD uint8_t at(uint32_t q) {
    if (q < H) {
      if (q == 0) return '>';
      if (q <= dig) return dec_char(dlo, dhi, dig - q);
      if (q == H - 1) return '\n';
      return q == dig + 1 ? '_' : (uint8_t)('0' + pick.mate);
    }
    const uint32_t p = q - H;
    if (p >= len) return '\n';
    const uint32_t code = cur.code(rc ? len - 1 - p : p);
    if (code == 4) return 'N';
    return (uint8_t)(0x54474341u >> (8 * (rc ? 3 - code : code)));          // "ACGT"
  }
};

// ---- records of k1mer.dict: k1mer '\t' weight '\n', every window of every contig in order
SHN_XHD uint32_t dict_len(const uint32_t* weights, uint32_t k1, uint64_t i) { return k1 + 1 + dec_digits(weights[i]) + 1; }
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
  SHN_XHD void enter(uint64_t i, uint32_t) {
    const uint64_t wi = w0 + i;
    if (c == ~0ULL) c = record_of(woff, 0, n_strings, wi);      // the last contig with woff[c] <= wi (contigs without a window share their offset with the next)
    else while (woff[c + 1] <= wi) c++;                         // (wi < woff[n_strings]: c stays below n_strings)
    tpos = coff[c] + (wi - woff[c]);
    dec_set(weights[i], dlo, dhi, dig);
  }
  SHN_XHD uint8_t at(uint32_t q) {
    if (q < k1) return text[tpos + q];
    if (q == k1) return '\t';
    if (q <= k1 + dig) return dec_char(dlo, dhi, k1 + dig - q);
    return '\n';
  }
};
