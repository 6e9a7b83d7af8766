// hip_own.hpp -- move-only owners of the HIP resources a handle holds: what a handle creates it releases when it dies, on every
// exit path, without a hand-written list.  An owner converts to the raw handle, so call sites read as they would with one.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <iterator>
#include <type_traits>
#include <utility>

namespace mi {

template <class H, class Release>
class HipOwner {
  public:
    HipOwner() = default;
    HipOwner(HipOwner&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    HipOwner& operator=(HipOwner&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    ~HipOwner() { reset(); }
    void reset() {  // (the release cannot be acted upon where an owner dies: its error is dropped)
        if (h_)
            Release{}(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
    operator H() const { return h_; }
    H* put() {  // for the creating call (hipStreamCreate..., hipEventCreate..., hipHostMalloc): releases what it held
        reset();
        return &h_;
    }

  private:
    H h_ = nullptr;
};

struct DevRelease {
    void operator()(void* p) const { (void)hipFree(p); }
};
struct PinnedRelease {
    void operator()(void* p) const { (void)hipHostFree(p); }
};
struct StreamRelease {
    void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};
struct EventRelease {
    void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};

template <class T>
using DevBuf = HipOwner<T*, DevRelease>;  // hipMalloc'ed
template <class T>
using PinnedBuf = HipOwner<T*, PinnedRelease>;  // hipHostMalloc'ed
using Stream = HipOwner<hipStream_t, StreamRelease>;
using Event = HipOwner<hipEvent_t, EventRelease>;

template <class O>
constexpr bool kMoveOnly = std::is_nothrow_move_constructible<O>::value && std::is_nothrow_move_assignable<O>::value &&
                           !std::is_copy_constructible<O>::value && !std::is_copy_assignable<O>::value;
static_assert(kMoveOnly<DevBuf<float>> && kMoveOnly<PinnedBuf<char>> && kMoveOnly<Stream> && kMoveOnly<Event>, "one owner per resource");

// `count` elements of device memory (none, and an empty owner, for count == 0)
template <class T>
hipError_t dalloc(DevBuf<T>& b, size_t count) {
    T** p = b.put();
    if (count == 0)
        return hipSuccess;
    return hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
}

// ... all zero
template <class T>
hipError_t dalloc_zero(DevBuf<T>& b, size_t count) {
    const hipError_t e = dalloc(b, count);
    return (e != hipSuccess || count == 0) ? e : hipMemset(b, 0, count * sizeof(T));
}

// ... holding the elements of a host array or vector (in `room` elements, where more are wanted than are uploaded)
template <class T, class Src>
hipError_t dalloc_copy(DevBuf<T>& b, const Src& src, size_t room = 0) {
    const size_t count = std::size(src);
    const hipError_t e = dalloc(b, room > count ? room : count);
    return (e != hipSuccess || count == 0) ? e : hipMemcpy(b, std::data(src), count * sizeof(T), hipMemcpyHostToDevice);
}

}  // namespace mi
