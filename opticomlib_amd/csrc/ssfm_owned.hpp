// Owners for what a plan holds on the device and in page-locked memory (ssfm_host.hip).  Host code only.
// None can be copied (streams and events can be moved), each frees what it holds in its destructor and converts to the plain handle, so that a launch
// or a HIP call takes it as it took the raw pointer.  Nothing here synchronises: a caller that frees a block which queued work may still read drains that work first (PlanT::grow).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <utility>

namespace ssfm {

// A device block that only grows.  `reserve` leaves a block that is large enough alone; otherwise the old block is freed BEFORE the new one is made (the
// two never coexist, as in the idiom this replaces) and the contents are lost.  hipFree waits for the whole device: nothing here calls it on an empty owner.
template <typename E> class DeviceBuffer {
  public:
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete; DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { free(); }
    // at least `bytes`; a new block is `bytes + slack` long
    hipError_t reserve(size_t bytes, size_t slack = 0) {
        if (p_ && cap_ >= bytes) return hipSuccess;
        free();
        const hipError_t e = hipMalloc(&p_, bytes + slack);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        cap_ = bytes + slack;
        return hipSuccess;
    }
    void free() { if (p_) (void)hipFree(p_); p_ = nullptr; cap_ = 0; }
    E* get() const { return p_; }
    operator E*() const { return p_; }
    size_t capacity() const { return cap_; }       // bytes
  private:
    E* p_ = nullptr; size_t cap_ = 0;
};

// The same in page-locked host memory.
template <typename E> class PinnedBuffer {
  public:
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer&) = delete; PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer() { if (p_) (void)hipHostFree(p_); }
    hipError_t reserve(size_t bytes) {
        if (p_ && cap_ >= bytes) return hipSuccess;
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr; cap_ = 0;
        const hipError_t e = hipHostMalloc(&p_, bytes, hipHostMallocDefault);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        cap_ = bytes;
        return hipSuccess;
    }
    operator E*() const { return p_; }
    E* operator->() const { return p_; }
  private:
    E* p_ = nullptr; size_t cap_ = 0;
};

// A stream / an event.  `out()` is where a hipStreamCreate* / hipEventCreate* call puts a new one; Stream::release() gives the handle up without destroying
// it (a plan's good pair of lane streams goes to the process's pool).
class Stream {
  public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream& operator=(Stream&& o) noexcept { std::swap(s_, o.s_); return *this; }
    Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
    ~Stream() { reset(); }
    void reset(hipStream_t s = nullptr) { if (s_) (void)hipStreamDestroy(s_); s_ = s; }
    hipStream_t* out() { reset(); return &s_; }
    hipStream_t release() { hipStream_t s = s_; s_ = nullptr; return s; }
    operator hipStream_t() const { return s_; }
  private:
    hipStream_t s_ = nullptr;
};

class Event {
  public:
    Event() = default;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(e_, o.e_); return *this; }
    Event(const Event&) = delete; Event& operator=(const Event&) = delete;
    ~Event() { reset(); }
    void reset(hipEvent_t e = nullptr) { if (e_) (void)hipEventDestroy(e_); e_ = e; }
    hipEvent_t* out() { reset(); return &e_; }
    operator hipEvent_t() const { return e_; }
  private:
    hipEvent_t e_ = nullptr;
};

}  // namespace ssfm
