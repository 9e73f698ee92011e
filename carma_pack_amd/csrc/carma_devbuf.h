// carma_devbuf.h -- device memory of the host layer: the two allocation entry points, and DevMem, the one owner of a device
// buffer (a scoped local of an entry point, or a member of a handle).  Host C++ only.
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
template <class T>
static inline hipError_t dev_malloc(T** p, size_t n)          // (typed front end: dev_malloc(&d_x, bytes))
{
    return carma_dev_malloc(reinterpret_cast<void**>(p), n);
}
static inline hipError_t dev_free(void* p) { return carma_dev_free(p); }

namespace carma {

// Owns at most one allocation of carma_dev_malloc; move-only, released by the destructor.  A scoped DevMem is declared BEFORE
// the host vectors that are copied to or from it, so that it is released after them -- and after the synchronisation that
// ends the copies.  A request of 0 bytes is passed on as 0 bytes (hipMalloc then hands back a null pointer, the guard mode a
// minimal mapping); no entry point asks for none today: every size is a product of counts its argument checks hold >= 1.
class DevMem {
public:
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    DevMem(DevMem&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevMem& operator=(DevMem&& o) noexcept
    {
        if (this != &o) {
            release();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~DevMem() { release(); }
    // exactly `bytes`, in place of what it held; empty after a failure
    hipError_t alloc(size_t bytes)
    {
        release();
        const hipError_t e = carma_dev_malloc(&p_, bytes);
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
        if (p_) (void)carma_dev_free(p_);
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

}  // namespace carma
