// carma_devbuf.h -- memory of the host layer: the four allocation entry points (device, pinned host) and the owners over them.
// DevMem owns an untyped device buffer (a scoped local of an entry point, or a member of a handle); DevBuf<T> / PinnedBuf<T>
// own a typed one and read as a T* wherever one is expected.  Every handle and every sampler state holds its memory through
// these: deleting the handle releases it, and nothing under csrc/ frees by hand.  Host C++ only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <utility>

// Device allocations of the library go through these two.  CARMA_DEBUG_GUARD=1 (read once; a test switch, off by default)
// gives every allocation a virtual-memory mapping of its own whose END is the end of the buffer, with unmapped address space
// behind it: a kernel that reads or writes past a buffer faults instead of getting away with it (round 4: a read of two
// doubles past the parameter batch had lived in the lane-group kernels for two rounds, caught only when a batch happened to
// end on a page boundary).  tests/test_gpu_parity.py runs a cross-section of the entry points in that mode.
hipError_t carma_dev_malloc(void** p, size_t n);
hipError_t carma_dev_free(void* p);
// Pinned host memory (hipHostMalloc, hipHostMallocDefault): the staging blocks of the contexts
hipError_t carma_pinned_malloc(void** p, size_t n);
hipError_t carma_pinned_free(void* p);

namespace carma {

// Owns at most one allocation of Malloc; move-only, released by the destructor.  A scoped DevMem is declared BEFORE
// the host vectors that are copied to or from it, so that it is released after them -- and after the synchronisation that
// ends the copies.  A request of 0 bytes is passed on as 0 bytes (hipMalloc then hands back a null pointer, the guard mode a
// minimal mapping); no entry point asks for none today: every size is a product of counts its argument checks hold >= 1.
template <hipError_t (*Malloc)(void**, size_t), hipError_t (*Free)(void*)>
class OwnedMem {
public:
    OwnedMem() = default;
    OwnedMem(const OwnedMem&) = delete;
    OwnedMem& operator=(const OwnedMem&) = delete;
    OwnedMem(OwnedMem&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    OwnedMem& operator=(OwnedMem&& o) noexcept
    {
        if (this != &o) {
            release();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~OwnedMem() { release(); }
    // exactly `bytes`, in place of what it held; empty after a failure
    hipError_t alloc(size_t bytes)
    {
        release();
        const hipError_t e = Malloc(&p_, bytes);
        if (e == hipSuccess)
            cap_ = bytes;
        else
            p_ = nullptr;
        return e;
    }
    // room for `bytes`, grown with a quarter to spare and by 4 KiB at least (the per-call buffers of a handle)
    hipError_t need(size_t bytes) { return bytes <= cap_ ? hipSuccess : alloc(std::max(bytes + bytes / 4, (size_t)4096)); }
    void release()
    {
        if (p_) (void)Free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p_); }
    size_t capacity() const { return cap_; }

private:
    void* p_ = nullptr;
    size_t cap_ = 0;
};
using DevMem = OwnedMem<carma_dev_malloc, carma_dev_free>;
using PinnedMem = OwnedMem<carma_pinned_malloc, carma_pinned_free>;

// An owner of `count` elements of T: Mem with the element type attached.  It converts to T*, so a member of this type is read
// like the raw pointer it replaces (s->d_chol + k, if (!s->d_send), hipMemcpy(s->d_lp, ...)); where a template deduces its
// argument from it (hipLaunchKernelGGL), pass get().
template <class T, class Mem>
class TypedBuf : Mem {
public:
    hipError_t alloc(size_t count) { return Mem::alloc(sizeof(T) * count); }   // exactly; empty after a failure
    using Mem::release;
    T* get() const { return Mem::template as<T>(); }
    operator T*() const { return get(); }
};
template <class T>
using DevBuf = TypedBuf<T, DevMem>;
template <class T>
using PinnedBuf = TypedBuf<T, PinnedMem>;

}  // namespace carma
