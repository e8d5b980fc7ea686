// The host side of the --inDisk file drivers (shannon_amd/csrc/chunk_writer.h: writer thread, two staging buffers, chunk
// bookkeeping) with the device formatter replaced by a CPU loop -- a program of its own, so that it can run under sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/indisk_host_check.cpp -o indisk_host_check
//   ./indisk_host_check <scratch directory>
// Exit status 0 and "indisk_host_check: OK" when every case holds.
#include "../shannon_amd/csrc/chunk_writer.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static std::string slurp(const std::string& path) {
  std::string s;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return s;
  char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
  fclose(f);
  return s;
}

// records ">i\n" + (len[i] letters) + "\n": the whole text and its offsets
static void make_records(const std::vector<uint32_t>& len, uint64_t base, std::string* text, std::vector<uint64_t>* off) {
  text->clear(); off->assign(1, base);
  for (size_t i = 0; i < len.size(); i++) {
    *text += ">" + std::to_string(i) + "\n";
    for (uint32_t j = 0; j < len[i]; j++) *text += "ACGT"[(i + j) & 3];
    *text += "\n";
    off->push_back(base + text->size());
  }
}

// one run of the driver over the records; returns its code, the file's bytes in *got
static int run(const std::string& path, const std::string& text, const std::vector<uint64_t>& off, uint64_t stage, std::string* msg, uint64_t* written,
               uint64_t* n_chunks, int fail_at_chunk = -1) {
  const uint64_t n = off.size() - 1;
  const uint64_t room = std::max(stage, shn_longest_record(off.data(), n));
  std::vector<uint8_t> buf[2] = {std::vector<uint8_t>(room), std::vector<uint8_t>(room)};     // exactly the room the contract promises
  uint64_t chunks = 0, next = 0;
  auto fill = [&](uint64_t r0, uint64_t r1, int slot, const uint8_t** data) -> int {
    CHECK(r0 == next && r1 > r0 && r1 <= n);                                        // chunks follow one another, none is empty
    CHECK(off[r1] - off[r0] <= room);
    CHECK(r1 == r0 + 1 || off[r1] - off[r0] <= stage);                              // only a single record may exceed the stage size
    CHECK(r1 == n || off[r1 + 1] - off[r0] > stage);                                // ... and a chunk takes every record that fits
    CHECK(slot == (int)(chunks & 1));
    if ((int)chunks == fail_at_chunk) return -77;
    memcpy(buf[slot].data(), text.data() + (off[r0] - off[0]), off[r1] - off[r0]);  // the "formatter"
    *data = buf[slot].data();
    next = r1; chunks++;
    return 0;
  };
  const int rc = shn_write_records_chunked(path.c_str(), off.data(), n, stage, fill, msg, written);
  *n_chunks = chunks;
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]); return 2; }
  const std::string dir = argv[1], path = dir + "/indisk_host_check.out";
  std::string text, msg;
  std::vector<uint64_t> off;
  uint64_t written = 0, chunks = 0;

  // 1,001 records of lengths 0 .. 130 at stage sizes around the record and chunk edges; offsets that do not start at 0
  std::vector<uint32_t> len;
  uint32_t x = 12345;
  for (int i = 0; i < 1001; i++) { x = x * 1664525u + 1013904223u; len.push_back((x >> 16) % 131); }
  for (uint64_t base : {0ull, 1000003ull}) {
    make_records(len, base, &text, &off);
    for (uint64_t stage : {1ull, 2ull, 3ull, 64ull, 133ull, 134ull, 4096ull, (unsigned long long)text.size() - 1, (unsigned long long)text.size(),
                           (unsigned long long)text.size() + 1, 1ull << 20}) {
      msg.clear();
      const int rc = run(path, text, off, stage, &msg, &written, &chunks);
      CHECK(rc == 0 && msg.empty());
      CHECK(written == text.size());
      CHECK(slurp(path) == text);
      if (stage >= text.size()) CHECK(chunks == 1);
      if (stage == 1) CHECK(chunks == len.size());
    }
  }
  // no record: an empty file, no chunk
  make_records({}, 0, &text, &off);
  CHECK(run(path, text, off, 4096, &msg, &written, &chunks) == 0 && written == 0 && chunks == 0 && slurp(path).empty());
  // one record, longer than the stage size
  make_records({5000}, 0, &text, &off);
  CHECK(run(path, text, off, 4096, &msg, &written, &chunks) == 0 && chunks == 1 && slurp(path) == text);
  // a path inside a directory that does not exist: -1, the message holds the path and strerror(ENOENT); the formatter is never called
  make_records(len, 0, &text, &off);
  const std::string nowhere = dir + "/no_such_directory/reads.fasta";
  msg.clear();
  CHECK(run(nowhere, text, off, 4096, &msg, &written, &chunks) == -1 && chunks == 0 && written == 0);
  CHECK(msg.find(nowhere) != std::string::npos && msg.find(strerror(ENOENT)) != std::string::npos);
  // a device that takes no byte: -1, path + strerror(ENOSPC); the run ends early and nothing is tried again
  if (access("/dev/full", W_OK) == 0) {
    msg.clear();
    CHECK(run("/dev/full", text, off, 4096, &msg, &written, &chunks) == -1 && written == 0);
    CHECK(msg.find("/dev/full") != std::string::npos && msg.find(strerror(ENOSPC)) != std::string::npos);
    CHECK(chunks <= 3);
  }
  // the formatter fails at its third chunk: its code comes back, the two chunks before it are in the file (the partial file is left)
  msg.clear();
  CHECK(run(path, text, off, 4096, &msg, &written, &chunks, 2) == -77 && chunks == 2);
  const std::string part = slurp(path);
  CHECK(part.size() == written && part.size() > 0 && part.size() <= 2 * 4096 && text.compare(0, part.size(), part) == 0);
  unlink(path.c_str());
  if (failures) { fprintf(stderr, "indisk_host_check: %d check(s) failed\n", failures); return 1; }
  printf("indisk_host_check: OK\n");
  return 0;
}
