// call_block.hpp -- the blocks of one call, for the files of entry points: ONE device block and (optionally) ONE pinned
// image from the allocation cache (devmem.cpp), carved at 256-byte offsets, and the queue that keeps the blocks of an
// enqueue-only call until the work on its stream is over.  Not part of any sampler translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kdehip_internal.hpp"

namespace kdehip {

constexpr int kMaxDevices = 64;  // devices the per-device bookkeeping (allocation cache, queue, profile sums) has slots for

inline size_t align256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

// Offsets of the pieces of a block, in the order they are taken; every piece starts at a multiple of 256.
struct Carve {
  size_t at = 0;
  size_t take(size_t bytes) { const size_t o = at; at = align256(at + bytes); return o; }
  size_t mark() const { return at; }  // where the next piece starts = the bytes taken so far
};

// ---- the deferred-release queue (devmem.cpp) -------------------------------------------------------------------------
// Runs when the entry is released, on whichever thread reaps it, with the entry's device current.
using ReleaseHook = void (*)(void *ctx, hipStream_t stream);
// (the device is current) Releases every entry of `device` whose event has fired, wherever it sits in the queue.  limit > 0:
// a caller with more than `limit` entries in flight on ITS OWN stream `mine` then waits for the oldest of those -- outside
// the lock, and never for another stream's entry.
void reap_deferred(int device, hipStream_t mine = nullptr, size_t limit = 0);
// (the device is current) Parks a device and a pinned block (either may be null) behind an event recorded on `stream` now;
// `hook` runs before they go back to the caches.  If the event cannot be created or recorded the stream is synchronised and
// everything is released at once (KDEHIP_ERR_HIP).
int defer_release(int device, hipStream_t stream, void *d, size_t dbytes, void *h, size_t hbytes, ReleaseHook hook = nullptr,
                  void *ctx = nullptr);
// Keeps a device and a pinned block (either may be null) until kdehip_clear_cache: the blocks of a call that was captured into
// a graph, whose nodes use them at every replay.  No event, no stream operation.
int keep_until_clear(int device, void *d, size_t dbytes, void *h, size_t hbytes);
// Waits for and releases everything parked for `device` (which is current), or for every device (-1: kdehip_clear_cache).
void drain_deferred(int device = -1);

// The device block and the pinned image of one call.  It remembers the (at most two) streams that work on the blocks was
// enqueued to: if the call returns while it is still armed -- an error after a launch -- the destructor synchronises them
// before the blocks go back to the cache.  A blocking call ends with wait(), an enqueue-only call with defer().
// The device the blocks were allocated on must be current when the object dies.
class CallBlock {
 public:
  CallBlock() = default;
  CallBlock(const CallBlock &) = delete;
  CallBlock &operator=(const CallBlock &) = delete;
  ~CallBlock() {
    (void)wait();
    if (d_) cached_free(d_, dbytes_);
    if (h_) cached_host_free(h_, hbytes_);
  }
  hipError_t alloc(size_t dbytes, size_t hbytes = 0) {  // hbytes == 0: no pinned image
    dbytes_ = dbytes;
    hbytes_ = hbytes;
    const hipError_t e = cached_malloc(&d_, dbytes);
    return e != hipSuccess || !hbytes ? e : cached_host_malloc(&h_, hbytes);
  }
  unsigned char *dev() const { return static_cast<unsigned char *>(d_); }
  unsigned char *host() const { return static_cast<unsigned char *>(h_); }
  size_t dev_bytes() const { return dbytes_; }
  // work that uses the blocks is about to be enqueued to `st`
  void touch(hipStream_t st) {
    last_ = st;
    for (int k = 0; k < n_; ++k) if (st_[k] == st) return;
    if (n_ < 2) st_[n_++] = st;
    else { (void)hipStreamSynchronize(st_[0]); st_[0] = st; }  // (no caller has a third)
  }
  hipStream_t stream() const { return last_; }  // the stream touched last
  // the first `bytes` of the pinned image go up in one copy
  hipError_t upload(size_t bytes, hipStream_t st) {
    touch(st);
    return hipMemcpyAsync(d_, h_, bytes, hipMemcpyHostToDevice, st);
  }
  // [offset, offset + bytes) of the device block comes back to the same place of the pinned image
  hipError_t download(size_t offset, size_t bytes, hipStream_t st) {
    touch(st);
    return hipMemcpyAsync(host() + offset, dev() + offset, bytes, hipMemcpyDeviceToHost, st);
  }
  // synchronises the streams and disarms
  hipError_t wait() {
    hipError_t e = hipSuccess;
    for (int k = 0; k < n_; ++k) {
      const hipError_t se = hipStreamSynchronize(st_[k]);
      if (e == hipSuccess) e = se;
    }
    n_ = 0;
    return e;
  }
  // an enqueue-only call: both blocks go to the queue, behind an event on the stream touched last (work on the other
  // stream, if any, must be ordered before it), and the object is disarmed
  int defer(int device, ReleaseHook hook = nullptr, void *ctx = nullptr) {
    const hipStream_t st = stream();
    void *d = d_, *h = h_;
    d_ = h_ = nullptr;
    n_ = 0;
    return defer_release(device, st, d, dbytes_, h, hbytes_, hook, ctx);
  }
  // a call captured into a graph: both blocks are kept until kdehip_clear_cache, and the object is disarmed
  int keep(int device) {
    void *d = d_, *h = h_;
    d_ = h_ = nullptr;
    n_ = 0;
    return keep_until_clear(device, d, dbytes_, h, hbytes_);
  }

 private:
  void *d_ = nullptr, *h_ = nullptr;
  size_t dbytes_ = 0, hbytes_ = 0;
  hipStream_t st_[2] = {nullptr, nullptr}, last_ = nullptr;
  int n_ = 0;
};

}  // namespace kdehip
