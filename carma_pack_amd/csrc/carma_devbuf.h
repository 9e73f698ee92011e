// carma_devbuf.h -- memory of the host layer: the four allocation entry points (device, pinned host) and the owners over them.
// DevMem owns an untyped device buffer (a scoped local of an entry point, or a member of a handle); DevBuf<T> / PinnedBuf<T>
// own a typed one and read as a T* wherever one is expected.  Every handle and every sampler state holds its memory through
// these: deleting the handle releases it, and nothing under csrc/ frees by hand.  Behind the owners: to_device, and WaveBatch /
// wave_batch_run, the buffers and the body of a log-density call planned in waves (carma_mlogdensity_batch,
// carma_bandset_logdensity_batch).  Host C++ only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/carma_mi355.h"
#include "carma_mseries_plan.h"

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

// A host vector into a fresh device buffer of its size (min_bytes at least), with a blocking copy: the create calls
template <class T>
inline hipError_t to_device(DevMem& b, const std::vector<T>& v, size_t min_bytes = 0)
{
    hipError_t e = b.alloc(std::max(sizeof(T) * v.size(), min_bytes));
    if (e == hipSuccess && !v.empty()) e = hipMemcpy(b.as<void>(), v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
    return e;
}

void set_error(const char* fmt, ...);        // (carma_host.h)
int hip_fail(hipError_t e, const char* what);

// The per-call state of a log-density call whose launch is PLANNED IN WAVES (carma_mseries_plan.h): B parameter vectors of
// `width` doubles, each on one of S series or objects, a wave on one of them.  Grown on demand and kept between calls.
struct WaveBatch {
    DevMem d_theta, d_out, d_wave, d_eidx;   // parameter vectors [cap_B][width], results [cap_B], plan [cap_W] + [cap_W][64]
    PinnedBuf<char> h_stage;                 // pinned: the same four, in this order
    long cap_B = 0, cap_W = 0;
    MlogdensPlan plan;                       // workspace of the launch plan

    hipError_t ensure(long B, long W, int width)
    {
        if (B <= cap_B && W <= cap_W) return hipSuccess;
        const long nB = std::max(std::max(B, cap_B), 1024L), nW = std::max(std::max(W, cap_W), 64L);
        for (DevMem* b : {&d_theta, &d_out, &d_wave, &d_eidx}) b->release();
        h_stage.release();
        cap_B = cap_W = 0;
        hipError_t e = d_theta.alloc(sizeof(double) * (size_t)nB * width);
        if (e == hipSuccess) e = d_out.alloc(sizeof(double) * (size_t)nB);
        if (e == hipSuccess) e = d_wave.alloc(sizeof(int) * (size_t)nW);
        if (e == hipSuccess) e = d_eidx.alloc(sizeof(int) * (size_t)nW * 64);
        if (e == hipSuccess) e = h_stage.alloc(sizeof(double) * (size_t)nB * (width + 1) + sizeof(int) * (size_t)nW * 65);
        if (e != hipSuccess) return e;
        cap_B = nB;
        cap_W = nW;
        return hipSuccess;
    }
};

// A planned-wave call behind its argument check (B >= 1, no null pointers): theta = [B][width], evaluation i on index[i] in
// [0, S) -- the error names it `noun`[i] and its range `count` -- len = [S] the lengths and cls = [S] the cadence classes the
// plan sorts by; out = [B].  enqueue(d_theta, d_wave, d_eidx, W, w_plain, d_out, st) launches the plan's W waves, the first
// w_plain of them of class 0, and returns a hipError_t.  The stream is synchronised before the return whatever happened: the
// enqueued copies read and write the pinned block.
template <class Enqueue>
int wave_batch_run(WaveBatch& wb, const char* who, int device, hipStream_t st, const double* theta, int width, const int* index,
                   int B, int S, const char* noun, const char* count, const int* len, const char* cls, double* out, Enqueue enqueue)
{
    // the waves are counted first, they size the staging block
    const long bad = mlogdens_plan_count(index, B, S, len, cls, wb.plan);
    if (bad >= 0) {
        set_error("%s: %s[%ld] = %d out of range (%s = %d)", who, noun, bad, index[bad], count, S);
        return CARMA_EINVAL;
    }
    const long W = wb.plan.W;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    e = wb.ensure(B, W, width);
    if (e != hipSuccess) return hip_fail(e, (std::string(who) + ": buffers").c_str());
    double* h_th = reinterpret_cast<double*>(wb.h_stage.get());
    double* h_out = h_th + (size_t)wb.cap_B * width;
    int* h_wave = reinterpret_cast<int*>(h_out + wb.cap_B);
    int* h_eidx = h_wave + wb.cap_W;
    std::memcpy(h_th, theta, sizeof(double) * (size_t)B * width);
    mlogdens_plan_fill(wb.plan, h_wave, h_eidx);              // straight into the pinned block
    double *d_theta = wb.d_theta.as<double>(), *d_out = wb.d_out.as<double>();
    int *d_wave = wb.d_wave.as<int>(), *d_eidx = wb.d_eidx.as<int>();
    e = hipMemcpyAsync(d_theta, h_th, sizeof(double) * (size_t)B * width, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_wave, h_wave, sizeof(int) * (size_t)W, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_eidx, h_eidx, sizeof(int) * (size_t)W * 64, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
        e = enqueue(d_theta, d_wave, d_eidx, W, wb.plan.w_plain, d_out, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_out, d_out, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, who);
    std::memcpy(out, h_out, sizeof(double) * (size_t)B);
    return CARMA_OK;
}

}  // namespace carma
