// Owners of what the library holds from the HIP runtime: device buffers, pinned host blocks, events, fences (an event
// plus "was it ever recorded") and streams.  Plain C++ over the runtime API: a holder releases because of its type.
// All of them are move-only (std::vector<Slot> is resized), their destructors ignore HIP's return codes, and every
// creation / release counts in live_resources (jxlh_live_resources, jxl_hip_dev.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace jxlh_host {

enum LiveKind { kLiveBuffers = 0, kLivePinned = 1, kLiveEvents = 2, kLiveStreams = 3 };
inline std::atomic<uint64_t> live_resources[4];  // process-wide, relaxed
inline void live_count(LiveKind k, int d) { live_resources[k].fetch_add((uint64_t)(int64_t)d, std::memory_order_relaxed); }

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;  // elements
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p = std::exchange(o.p, nullptr);
      n = std::exchange(o.n, 0);
    }
    return *this;
  }
  ~DevBuf() { (void)reset(); }
  // the buffer is empty afterwards, whatever hipFree says
  hipError_t reset() {
    if (!p) return hipSuccess;
    live_count(kLiveBuffers, -1);
    n = 0;
    return hipFree(std::exchange(p, nullptr));
  }
  // takes over an allocation of m elements made with hipMalloc (what it held is freed)
  void adopt(T* q, size_t m) {
    (void)reset();
    if (q) live_count(kLiveBuffers, 1);
    p = q;
    n = q ? m : 0;
  }
  // exactly m elements, contents undefined (what it held is freed)
  hipError_t alloc(size_t m) {
    (void)reset();
    void* q = nullptr;
    if (hipError_t e = hipMalloc(&q, m * sizeof(T))) return e;
    adopt(static_cast<T*>(q), m);
    return hipSuccess;
  }
  // grow-only: at least m elements, contents undefined when it grew.  *what names the call that failed.
  hipError_t ensure(size_t m, const char** what) {
    if (n >= m && p) return hipSuccess;
    *what = "hipFree(b.p)";
    if (hipError_t e = reset()) return e;
    *what = "hipMalloc(reinterpret_cast<void**>(&b.p), n * sizeof(T))";
    return m ? alloc(m) : hipSuccess;
  }
};

// a block of pinned host memory (hipHostMalloc)
template <class T>
struct Pinned {
  T* p = nullptr;
  size_t n = 0;  // elements
  Pinned() = default;
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
  Pinned(Pinned&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
  Pinned& operator=(Pinned&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p = std::exchange(o.p, nullptr);
      n = std::exchange(o.n, 0);
    }
    return *this;
  }
  ~Pinned() { (void)reset(); }
  hipError_t reset() {
    if (!p) return hipSuccess;
    live_count(kLivePinned, -1);
    n = 0;
    return hipHostFree(std::exchange(p, nullptr));
  }
  hipError_t alloc(size_t m) {  // the block must be empty
    void* q = nullptr;
    if (hipError_t e = hipHostMalloc(&q, m * sizeof(T), hipHostMallocDefault)) return e;
    live_count(kLivePinned, 1);
    p = static_cast<T*>(q);
    n = m;
    return hipSuccess;
  }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
  Event& operator=(Event&& o) noexcept {
    if (this != &o) {
      reset();
      e = std::exchange(o.e, nullptr);
    }
    return *this;
  }
  ~Event() { reset(); }
  operator hipEvent_t() const { return e; }
  void reset() {
    if (!e) return;
    live_count(kLiveEvents, -1);
    (void)hipEventDestroy(std::exchange(e, nullptr));
  }
  // a timing event (hipEventCreate) or an ordering-only one (hipEventDisableTiming); no-op when it exists
  hipError_t create(bool timing = false) {
    if (e) return hipSuccess;
    const hipError_t r = timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (r == hipSuccess) live_count(kLiveEvents, 1);
    else e = nullptr;
    return r;
  }
};

// An ordering-only event and whether it has been recorded: a wait on a fence nothing was recorded on is no wait.
struct Fence {
  Event ev;
  bool recorded = false;
  hipError_t record(hipStream_t s) {  // creates the event on first use
    if (hipError_t r = ev.create()) return r;
    if (hipError_t r = hipEventRecord(ev, s)) return r;
    recorded = true;
    return hipSuccess;
  }
  hipError_t wait(hipStream_t s) const { return recorded ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
  hipError_t sync() const { return recorded ? hipEventSynchronize(ev) : hipSuccess; }
  void clear() { recorded = false; }  // forgets the record, keeps the event
};

struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
  Stream& operator=(Stream&& o) noexcept {
    if (this != &o) {
      reset();
      s = std::exchange(o.s, nullptr);
    }
    return *this;
  }
  ~Stream() { reset(); }
  operator hipStream_t() const { return s; }
  void reset() {
    if (!s) return;
    live_count(kLiveStreams, -1);
    (void)hipStreamDestroy(std::exchange(s, nullptr));
  }
  // non-blocking with a priority, or (n_mask_words > 0) with a CU mask; the stream must be empty
  hipError_t create(int priority, const uint32_t* cu_mask = nullptr, uint32_t n_mask_words = 0) {
    const hipError_t r = n_mask_words ? hipExtStreamCreateWithCUMask(&s, n_mask_words, cu_mask)
                                      : hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority);
    if (r == hipSuccess) live_count(kLiveStreams, 1);
    else s = nullptr;
    return r;
  }
};

}  // namespace jxlh_host
