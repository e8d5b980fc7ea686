// Host side of the --inDisk file drivers (reads_text.hip): records of known byte offsets written to a file chunk by chunk.  A chunk
// ends on a record boundary; while the caller fills chunk c + 1 (on the device: format + copy into the other staging buffer), a
// host thread writes chunk c.  A failed open / write ends the file where it is (the partial file stays, nothing is retried) and
// comes back as errno.  Plain C++, no HIP: tools/indisk_host_check.cpp builds this header with a CPU formatter into a program of
// its own and runs it under the address + undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>
#include <errno.h>
#include <fcntl.h>
#include <unistd.h>
#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>

struct ShnChunkWriter {
  int fd = -1;
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  const uint8_t* ptr[2] = {nullptr, nullptr};
  uint64_t len[2] = {0, 0};
  bool full[2] = {false, false};
  bool closing = false;
  int err = 0;               // errno of the first failed write
  uint64_t written = 0;
  int next = 0;              // the slot the writer takes next (the producer fills 0, 1, 0, 1, ...)

  int start(const char* path) {                      // 0 or errno
    fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) return errno ? errno : EIO;
    th = std::thread([this] { run(); });
    return 0;
  }
  void run() {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return full[next] || closing; });
      if (!full[next]) return;                       // closing, and every chunk handed over is written
      const uint8_t* p = ptr[next];
      const uint64_t n = len[next];
      const bool skip = err != 0;                    // after a failure the chunks still in flight are dropped
      lk.unlock();
      int e = 0;
      uint64_t done = 0;
      while (!skip && done < n) {
        const ssize_t w = ::write(fd, p + done, (size_t)(n - done));
        if (w < 0) { if (errno == EINTR) continue; e = errno ? errno : EIO; break; }
        done += (uint64_t)w;
      }
      lk.lock();
      written += done;
      if (e && !err) err = e;
      full[next] = false;
      next ^= 1;
      cv.notify_all();
    }
  }
  // the producer: waits until buffer `slot` is the writer's no more; the writer's errno so far (0: go on)
  int acquire(int slot) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !full[slot]; });
    return err;
  }
  void submit(int slot, const uint8_t* p, uint64_t n) {
    { std::lock_guard<std::mutex> lk(mu); ptr[slot] = p; len[slot] = n; full[slot] = true; }
    cv.notify_all();
  }
  int finish() {                                     // 0 or the errno of the first failure
    { std::lock_guard<std::mutex> lk(mu); closing = true; }
    cv.notify_all();
    if (th.joinable()) th.join();
    int e = err;
    if (fd >= 0 && ::close(fd) != 0 && !e) e = errno ? errno : EIO;
    fd = -1;
    return e;
  }
  ~ShnChunkWriter() { if (th.joinable() || fd >= 0) (void)finish(); }
};

// the longest record of off[0 .. n]
static inline uint64_t shn_longest_record(const uint64_t* off, uint64_t n) {
  uint64_t mx = 0;
  for (uint64_t i = 0; i < n; i++) mx = std::max(mx, off[i + 1] - off[i]);
  return mx;
}

// Records 0 .. n - 1 (byte offsets off[0 .. n], ascending; off[0] need not be 0) into `path`, in chunks of at most `stage` bytes
// that end on a record boundary -- a record longer than `stage` is a chunk of its own, so the caller's two buffers hold
// max(stage, shn_longest_record).  fill(r0, r1, slot, &data) formats records [r0, r1) into buffer `slot`, sets data to it and
// returns 0, or its own error code, which ends the file and is handed on.  Returns 0, fill's code, or -1 for a failed open /
// write / close: *msg then holds the path and strerror(errno).  *written: the bytes that reached the file.
template <class Fill>
int shn_write_records_chunked(const char* path, const uint64_t* off, uint64_t n, uint64_t stage, Fill fill, std::string* msg, uint64_t* written) {
  ShnChunkWriter w;
  int e = w.start(path);
  if (e) {
    *msg = std::string("cannot open ") + path + ": " + strerror(e);
    if (written) *written = 0;
    return -1;
  }
  int rc = 0, slot = 0;
  uint64_t r0 = 0;
  while (r0 < n) {
    // the last record boundary within `stage` bytes of off[r0]; at least one record
    const uint64_t* p = std::upper_bound(off + r0 + 1, off + n + 1, off[r0] + stage);
    uint64_t r1 = (uint64_t)(p - off) - 1;
    if (r1 <= r0) r1 = r0 + 1;
    if (w.acquire(slot)) break;                      // (the write of an earlier chunk failed: finish() says how)
    const uint8_t* data = nullptr;
    rc = fill(r0, r1, slot, &data);
    if (rc) break;
    w.submit(slot, data, off[r1] - off[r0]);
    slot ^= 1;
    r0 = r1;
  }
  e = w.finish();
  if (written) *written = w.written;
  if (rc) return rc;
  if (e) {
    *msg = std::string("cannot write ") + path + ": " + strerror(e);
    return -1;
  }
  return 0;
}
