// The owners of the library's HIP resources (jxl_rs_amd/csrc/device_owned.h) without a device: this program defines
// counting stand-ins for the HIP calls the header uses -- the executable's own definitions win at link time -- and
// checks that every resource is released exactly once, by its owner's type, and that the live-resource counters agree
// with the stand-ins' own tallies.  Host only.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "../../jxl_rs_amd/csrc/device_owned.h"

using namespace jxlh_host;

namespace {
int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      failures++;                                                      \
      std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);     \
    }                                                                  \
  } while (0)

// what the stand-ins hand out and have not taken back, per kind (LiveKind), and what was asked of them
std::set<void*> live[4];
int bad_releases = 0;  // a release of something not live (a second release, a handle never handed out)
int timing_events = 0, ordering_events = 0, records = 0, stream_waits = 0, event_syncs = 0;
int masked_streams = 0, priority_streams = 0;
hipError_t free_result = hipSuccess, malloc_result = hipSuccess;

void* hand_out(LiveKind k, size_t bytes) {
  void* p = std::malloc(bytes ? bytes : 1);
  live[k].insert(p);
  return p;
}
void take_back(LiveKind k, void* p) {
  if (live[k].erase(p)) std::free(p);
  else bad_releases++;
}
bool balanced() {
  bool ok = bad_releases == 0;
  for (int k = 0; k < 4; k++) ok = ok && live[k].empty() && live_resources[k].load() == 0;
  return ok;
}
bool counters_match() {
  for (int k = 0; k < 4; k++)
    if (live_resources[k].load() != live[k].size()) return false;
  return bad_releases == 0;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
  if (malloc_result != hipSuccess) return malloc_result;
  *p = hand_out(kLiveBuffers, bytes);
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  take_back(kLiveBuffers, p);  // (the runtime's hipFree has let go of the memory when it reports a late error, too)
  return free_result;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) {
  *p = hand_out(kLivePinned, bytes);
  return hipSuccess;
}
hipError_t hipHostFree(void* p) {
  take_back(kLivePinned, p);
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) {
  timing_events++;
  *e = static_cast<hipEvent_t>(hand_out(kLiveEvents, 1));
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  if (flags != hipEventDisableTiming) return hipErrorInvalidValue;
  ordering_events++;
  *e = static_cast<hipEvent_t>(hand_out(kLiveEvents, 1));
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  take_back(kLiveEvents, e);
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {
  if (!live[kLiveEvents].count(e)) return hipErrorInvalidHandle;
  records++;
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
  if (!live[kLiveEvents].count(e)) return hipErrorInvalidHandle;
  event_syncs++;
  return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t e, unsigned int) {
  if (!live[kLiveEvents].count(e)) return hipErrorInvalidHandle;
  stream_waits++;
  return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int flags, int) {
  if (flags != hipStreamNonBlocking) return hipErrorInvalidValue;
  priority_streams++;
  *s = static_cast<hipStream_t>(hand_out(kLiveStreams, 1));
  return hipSuccess;
}
hipError_t hipExtStreamCreateWithCUMask(hipStream_t* s, uint32_t n, const uint32_t* mask) {
  if (!n || !mask) return hipErrorInvalidValue;
  masked_streams++;
  *s = static_cast<hipStream_t>(hand_out(kLiveStreams, 1));
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  take_back(kLiveStreams, s);
  return hipSuccess;
}
}  // extern "C"

namespace {

// the members of the context's Slot (jxlh_ctx.h, which a host compiler cannot include: it carries device code)
struct Slot {
  Stream stream;
  Event done;
  Fence copied;
  bool used = false;
  DevBuf<uint8_t> stage8;
};

void check_devbuf() {
  {
    DevBuf<float> a, b;
    CHECK(a.alloc(100) == hipSuccess && a.p && a.n == 100);
    CHECK(b.alloc(7) == hipSuccess);
    CHECK(live[kLiveBuffers].size() == 2 && counters_match());
    float* const was_a = a.p;
    DevBuf<float> c(std::move(a));  // move construction: the source is empty, nothing is released
    CHECK(!a.p && a.n == 0 && c.p == was_a && c.n == 100 && live[kLiveBuffers].size() == 2 && counters_match());
    b = std::move(c);  // move assignment: the target's old buffer goes, once
    CHECK(!c.p && c.n == 0 && b.p == was_a && b.n == 100 && live[kLiveBuffers].size() == 1 && counters_match());
    CHECK(b.reset() == hipSuccess && !b.p && b.n == 0 && live[kLiveBuffers].empty());
    CHECK(b.reset() == hipSuccess && counters_match());  // reset() twice is harmless
    // adopt over a held buffer frees the old one
    CHECK(b.alloc(3) == hipSuccess);
    void* raw = nullptr;
    CHECK(hipMalloc(&raw, 64) == hipSuccess);
    b.adopt(static_cast<float*>(raw), 16);
    CHECK(b.p == raw && b.n == 16 && live[kLiveBuffers].size() == 1 && counters_match());
  }
  CHECK(balanced());
  {  // ensure: grows, never shrinks
    DevBuf<int> b;
    const char* what = "";
    CHECK(b.ensure(0, &what) == hipSuccess && !b.p && b.n == 0);
    CHECK(b.ensure(10, &what) == hipSuccess && b.p && b.n == 10);
    int* const was = b.p;
    CHECK(b.ensure(4, &what) == hipSuccess && b.p == was && b.n == 10);
    CHECK(b.ensure(10, &what) == hipSuccess && b.p == was && b.n == 10);
    CHECK(b.ensure(11, &what) == hipSuccess && b.n == 11 && live[kLiveBuffers].size() == 1 && counters_match());
    // a hipFree that reports an error leaves an EMPTY buffer behind (not a pointer to freed memory), names the call,
    // and the next ensure starts from nothing
    free_result = hipErrorInvalidValue;
    CHECK(b.ensure(20, &what) == hipErrorInvalidValue && !b.p && b.n == 0 && std::string(what) == "hipFree(b.p)");
    free_result = hipSuccess;
    CHECK(live[kLiveBuffers].empty() && counters_match());
    CHECK(b.ensure(20, &what) == hipSuccess && b.n == 20);
    // an allocation that fails: empty as well
    malloc_result = hipErrorOutOfMemory;
    CHECK(b.ensure(30, &what) == hipErrorOutOfMemory && !b.p && b.n == 0 && std::string(what).rfind("hipMalloc(", 0) == 0);
    malloc_result = hipSuccess;
    CHECK(counters_match());
  }
  CHECK(balanced());
}

void check_pinned() {
  {
    Pinned<int> a, b;
    CHECK(a.alloc(1) == hipSuccess && a.p && a.n == 1);
    *a.p = 5;
    Pinned<int> c(std::move(a));
    CHECK(!a.p && a.n == 0 && c.n == 1 && *c.p == 5 && live[kLivePinned].size() == 1 && counters_match());
    CHECK(b.alloc(12) == hipSuccess && live[kLivePinned].size() == 2);
    b = std::move(c);
    CHECK(!c.p && b.n == 1 && *b.p == 5 && live[kLivePinned].size() == 1 && counters_match());
    CHECK(b.reset() == hipSuccess && b.reset() == hipSuccess && !b.p && b.n == 0);
  }
  CHECK(balanced());
}

void check_events_and_fences() {
  {
    Event t, o;
    CHECK(!t && t.create(true) == hipSuccess && t && timing_events == 1 && ordering_events == 0);
    CHECK(o.create() == hipSuccess && ordering_events == 1);
    const hipEvent_t was = o;
    CHECK(o.create() == hipSuccess && o == was && ordering_events == 1);  // exists: kept
    Event m(std::move(t));
    CHECK(!t && m && live[kLiveEvents].size() == 2 && counters_match());
    o = std::move(m);
    CHECK(!m && o && o != was && live[kLiveEvents].size() == 1 && counters_match());
    o.reset();
    o.reset();
    CHECK(!o && live[kLiveEvents].empty() && counters_match());
  }
  CHECK(balanced());
  {
    Fence f;
    const hipStream_t s = nullptr;
    // nothing recorded: wait and sync issue nothing, and no event exists yet
    CHECK(f.wait(s) == hipSuccess && f.sync() == hipSuccess && stream_waits == 0 && event_syncs == 0);
    CHECK(!f.ev && live[kLiveEvents].empty());
    const int created = ordering_events;
    CHECK(f.record(s) == hipSuccess && f.recorded && f.ev && ordering_events == created + 1 && records == 1);
    const hipEvent_t was = f.ev;
    CHECK(f.wait(s) == hipSuccess && stream_waits == 1 && f.sync() == hipSuccess && event_syncs == 1);
    f.clear();  // forgets the record, keeps the event
    CHECK(!f.recorded && f.ev == was && f.wait(s) == hipSuccess && f.sync() == hipSuccess && stream_waits == 1 && event_syncs == 1);
    CHECK(f.record(s) == hipSuccess && f.ev == was && ordering_events == created + 1 && records == 2);
    Fence g(std::move(f));  // the record moves with the event
    CHECK(!f.ev && g.recorded && g.ev == was && g.wait(s) == hipSuccess && stream_waits == 2 && counters_match());
  }
  CHECK(balanced());
}

void check_streams_and_slots() {
  {
    Stream a, b;
    const uint32_t mask[2] = {0xffffffffu, 0xffu};
    CHECK(a.create(0) == hipSuccess && a && priority_streams == 1 && masked_streams == 0);
    CHECK(b.create(0, mask, 2) == hipSuccess && masked_streams == 1 && live[kLiveStreams].size() == 2 && counters_match());
    const hipStream_t was = b;
    a = std::move(b);
    CHECK(!b && a == was && live[kLiveStreams].size() == 1 && counters_match());
    Stream c(std::move(a));
    CHECK(!a && c == was && live[kLiveStreams].size() == 1);
    c.reset();
    c.reset();
    CHECK(!c && live[kLiveStreams].empty());
  }
  CHECK(balanced());
  {  // a vector of slots resized up (its elements move) and down (the dropped ones release)
    auto fill = [](std::vector<Slot>& v, size_t from) {
      for (size_t i = from; i < v.size(); i++) {
        CHECK(v[i].stream.create(0) == hipSuccess && v[i].done.create() == hipSuccess);
        CHECK(v[i].copied.record(v[i].stream) == hipSuccess && v[i].stage8.alloc(100 + i) == hipSuccess);
      }
    };
    std::vector<Slot> v(3);
    fill(v, 0);
    const uint8_t* const stage0 = v[0].stage8.p;
    v.resize(40);
    fill(v, 3);
    CHECK(v[0].stage8.p == stage0 && v[0].copied.recorded && v[2].stage8.n == 102);
    CHECK(live[kLiveStreams].size() == 40 && live[kLiveEvents].size() == 80 && live[kLiveBuffers].size() == 40 && counters_match());
    v.resize(2);
    CHECK(live[kLiveStreams].size() == 2 && live[kLiveEvents].size() == 4 && live[kLiveBuffers].size() == 2 && counters_match());
    v.resize(5);
    CHECK(!v[4].stream && !v[4].stage8.p && counters_match());
  }
  CHECK(balanced());
}

}  // namespace

int main() {
  check_devbuf();
  check_pinned();
  check_events_and_fences();
  check_streams_and_slots();
  if (failures) {
    std::printf("device owners: %d FAILED checks\n", failures);
    return 1;
  }
  std::printf("device owners: ok\n");
  return 0;
}
