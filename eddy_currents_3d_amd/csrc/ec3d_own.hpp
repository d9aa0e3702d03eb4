// ec3d_own.hpp — the owners of everything the library takes from the HIP runtime: device buffers, pinned host
// buffers, events, streams.  Move-only, empty when default-constructed, released in the destructor; they convert
// implicitly to the raw pointer / handle, so launches and copies read as they would with one.  alloc / create release
// what was held, return the runtime's status and set no error text: the caller decides whether a failure is an error
// (EC3D_HIP, MHIP) or a fallback (the placement searches, ec3d_spare_pair).  Nothing outside this header calls the
// runtime's allocation, creation, free or destroy functions.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <utility>

// status of an acquisition into h: a failed one leaves the owner empty, whatever the runtime wrote there
template <class H> inline hipError_t ec3d_acquired(hipError_t e, H &h)
{
    if (e != hipSuccess) h = nullptr;
    return e;
}

// `count` elements of device memory
template <class T> class DevBuf {
    T *p_ = nullptr;

  public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.release()) {}
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p_ = o.release(); } return *this; }
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t count) { reset(); return ec3d_acquired(hipMalloc(&p_, count * sizeof(T)), p_); }
    // fine-grained memory: coherent across devices while kernels run
    hipError_t alloc_fine(size_t count)
    {
        reset();
        return ec3d_acquired(hipExtMallocWithFlags((void **)&p_, count * sizeof(T), hipDeviceMallocFinegrained), p_);
    }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
    T *release() { return std::exchange(p_, nullptr); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    void swap(DevBuf &o) noexcept { std::swap(p_, o.p_); }
};
static_assert(!std::is_copy_constructible<DevBuf<double>>::value, "a device buffer has one owner");

// `count` elements of pinned host memory
template <class T> class PinnedBuf {
    T *p_ = nullptr;

  public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&o) noexcept : p_(o.release()) {}
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { if (this != &o) { reset(); p_ = o.release(); } return *this; }
    ~PinnedBuf() { reset(); }
    hipError_t alloc(size_t count) { reset(); return ec3d_acquired(hipHostMalloc(&p_, count * sizeof(T), hipHostMallocDefault), p_); }
    void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; }
    T *release() { return std::exchange(p_, nullptr); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    void swap(PinnedBuf &o) noexcept { std::swap(p_, o.p_); }
};
static_assert(!std::is_copy_constructible<PinnedBuf<double>>::value, "a pinned buffer has one owner");

class Event {
    hipEvent_t e_ = nullptr;

  public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); e_ = std::exchange(o.e_, nullptr); } return *this; }
    ~Event() { reset(); }
    hipError_t create() { reset(); return ec3d_acquired(hipEventCreate(&e_), e_); } // a timing event
    hipError_t create(unsigned flags) { reset(); return ec3d_acquired(hipEventCreateWithFlags(&e_, flags), e_); }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    hipEvent_t get() const { return e_; }
    operator hipEvent_t() const { return e_; }
};
static_assert(!std::is_copy_constructible<Event>::value, "an event has one owner");

class Stream {
    hipStream_t s_ = nullptr;

  public:
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    Stream(Stream &&o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { reset(); s_ = std::exchange(o.s_, nullptr); } return *this; }
    ~Stream() { reset(); }
    hipError_t create(unsigned flags) { reset(); return ec3d_acquired(hipStreamCreateWithFlags(&s_, flags), s_); }
    hipError_t create(unsigned flags, int priority)
    {
        reset();
        return ec3d_acquired(hipStreamCreateWithPriority(&s_, flags, priority), s_);
    }
    void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
    hipStream_t get() const { return s_; }
    operator hipStream_t() const { return s_; }
};
static_assert(!std::is_copy_constructible<Stream>::value, "a stream has one owner");
