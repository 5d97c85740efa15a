// dev_mem.h -- who owns device memory in the host layer.  Host only: the
// *.cpp translation units include it; no .hip file and no header a .hip file
// includes does.
//
// Before a DevBuf is destroyed (or reserve() is asked to replace its block
// without a drain stream) the caller has made the block's device current and
// drained every stream whose queued work may still touch the block: the
// destructor only frees.  A plan does this once in its *_free function, in
// the order device, streams, gather gate, buffers, events, streams; a one-shot
// entry declares its StreamScope after its buffers, so the stream is
// synchronised and destroyed before they are freed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <utility>
#include <vector>

namespace amr {

// Move-only owner of one hipMalloc block.
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept { swap(o); }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      (void)reset();
      swap(o);
    }
    return *this;
  }
  ~DevBuf() { (void)reset(); }

  // owner of a block the caller got from hipMalloc (`bytes` of it)
  static DevBuf adopt(void* p, int64_t bytes) {
    DevBuf b;
    b.p_ = p;
    b.bytes_ = p ? bytes : 0;
    return b;
  }
  // gives the block up without freeing it (a process-lifetime table): the buffer is empty after
  void* detach() {
    void* p = p_;
    p_ = nullptr;
    bytes_ = 0;
    return p;
  }

  void* get() const { return p_; }
  template <class T>
  T* as() const { return static_cast<T*>(p_); }
  int64_t bytes() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }
  void swap(DevBuf& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(bytes_, o.bytes_);
  }

  // frees the block now (see the top for what the caller has done first)
  hipError_t reset() {
    const hipError_t e = p_ ? hipFree(p_) : hipSuccess;
    p_ = nullptr;
    bytes_ = 0;
    return e;
  }

  // At least `need` bytes: nothing when the block already holds them; else
  // `drain` (when non-null and a block exists) is synchronised -- queued work
  // may still read the old block --, the old block freed and exactly `need`
  // bytes allocated (no rounding, no doubling: reported totals are sums of
  // bytes()).  The old contents are not kept.  On failure the buffer is empty.
  hipError_t reserve(int64_t need, hipStream_t drain) {
    if (p_ && bytes_ >= need) return hipSuccess;
    if (p_ && drain) {
      const hipError_t e = hipStreamSynchronize(drain);
      if (e != hipSuccess) return e;
    }
    hipError_t e = reset();
    if (e != hipSuccess) return e;
    e = hipMalloc(&p_, (size_t)need);
    if (e != hipSuccess) {
      p_ = nullptr;
      return e;
    }
    bytes_ = need;
    return hipSuccess;
  }

 private:
  void* p_ = nullptr;
  int64_t bytes_ = 0;
};

// All-or-nothing reserve of a group that is only usable whole (a host entry's
// output staging): nothing when every member already holds its bytes; else
// every member is allocated anew into temporaries and the group committed by
// swap only when all succeeded -- on failure each member is exactly as it was.
// `drain` as in DevBuf::reserve, before the replaced blocks are freed.
struct DevWant {
  DevBuf& buf;
  int64_t bytes;
};
inline hipError_t reserve_all(std::initializer_list<DevWant> wants, hipStream_t drain) {
  bool have = true, any = false;
  for (const DevWant& w : wants) {
    have = have && w.buf && w.buf.bytes() >= w.bytes;
    any = any || w.buf;
  }
  if (have) return hipSuccess;
  std::vector<DevBuf> fresh(wants.size());
  size_t i = 0;
  for (const DevWant& w : wants) {
    const hipError_t e = fresh[i++].reserve(w.bytes, nullptr);
    if (e != hipSuccess) return e;
  }
  if (any && drain) {
    const hipError_t e = hipStreamSynchronize(drain);
    if (e != hipSuccess) return e;
  }
  i = 0;
  for (const DevWant& w : wants) w.buf.swap(fresh[i++]);
  return hipSuccess;   // `fresh` now holds the replaced blocks and frees them
}

// A one-shot entry's own stream: synchronised and destroyed when the scope ends.
class StreamScope {
 public:
  StreamScope() = default;
  StreamScope(const StreamScope&) = delete;
  StreamScope& operator=(const StreamScope&) = delete;
  ~StreamScope() {
    if (!st_) return;
    (void)hipStreamSynchronize(st_);
    (void)hipStreamDestroy(st_);
  }
  static hipError_t create(StreamScope& s) { return hipStreamCreateWithFlags(&s.st_, hipStreamNonBlocking); }
  hipStream_t get() const { return st_; }

 private:
  hipStream_t st_ = nullptr;
};

}  // namespace amr
