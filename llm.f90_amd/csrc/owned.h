// Owners of what the shim allocates or creates (llmk.hip): device buffers, pinned host buffers, events and streams.  Host code only.
// Each is move-only, releases in its destructor and is EMPTY (null) after a failed alloc / create, a reset() or a move out of it; nothing
// converts a raw pointer or handle into an owner.  An owner reads as the pointer or handle it holds, so kernel arguments, copies and
// pointer arithmetic are written as with the raw thing.  A field that points into another owner's allocation stays a raw pointer.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdlib.h>
#include <memory>
#include <type_traits>

namespace llmk {

// Every device allocation of the shim goes through here.  LLMK_POISON=1 (a test aid: tests/test_tp70_gpu.py and
// tests/host_tools/gpu_job.sh poison) fills the fresh allocation with 0xFF bytes -- NaN as f32 or f16, -1 as an integer --
// BEFORE the shim's own initialisation: a kernel that reads memory the shim never wrote then yields NaN every time,
// whatever the allocator happened to hand out (a fresh process usually sees zero pages, a long-lived one does not).
template <class T>
hipError_t dev_alloc(T** p, size_t bytes) {
    static const bool poison = getenv("LLMK_POISON") && getenv("LLMK_POISON")[0] == '1';
    hipError_t e = hipMalloc((void**)p, bytes);
    // (the fill must be COMPLETE when this returns: the shim's own initialisation often goes to the ctx's non-blocking stream, which the
    // null stream does not order -- round 6's first poison run: the self-test's mismatch counter read 0xFFFFFFFF on three ranks.  And it
    // must not wait for the DEVICE: with two ranks in one process a rank's kernel may be spinning for its peer, whose host thread is
    // in here -- the second poison run.  So: a stream of its own for the calling thread, and a wait for that stream alone)
    if (e == hipSuccess && poison) {
        static thread_local hipStream_t ps = nullptr;
        if (!ps) e = hipStreamCreateWithFlags(&ps, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMemsetAsync(*p, 0xFF, bytes, ps);
        if (e == hipSuccess) e = hipStreamSynchronize(ps);
    }
    return e;
}

// (the move-only part of every owner: a unique_ptr whose deleter is the runtime's release call)
template <class T, hipError_t (*Release)(T*)>
struct Releaser {
    void operator()(T* p) const { Release(p); }
};
template <class T, hipError_t (*Release)(T*)>
using Held = std::unique_ptr<T, Releaser<T, Release>>;

// n elements of device memory (bytes: DevBuf<char>)
template <class T>
class DevBuf {
public:
    // (hipFree waits for the device: a caller with work in flight on the buffer synchronises its stream first, and says so)
    void reset() { p_.reset(); }
    // frees what it held; uninitialised (or poisoned) memory
    hipError_t alloc(size_t n) {
        reset();
        T* p = nullptr;
        return take(dev_alloc(&p, n * sizeof(T)), p, n);
    }
    // fine-grained memory, which peers' stores and this device's system-scope polls meet in (the tensor-parallel inbox); never poisoned
    hipError_t alloc_finegrained(size_t n) {
        reset();
        T* p = nullptr;
        return take(hipExtMallocWithFlags((void**)&p, n * sizeof(T), hipDeviceMallocFinegrained), p, n);
    }
    // The one grow-only path: room for n elements, what it holds is NOT carried over.  A buffer that is large enough is left alone;
    // otherwise `st` -- the stream whose work may still use the old block -- is drained before that block is freed.  *grew says which.
    hipError_t reserve(size_t n, hipStream_t st, bool* grew = nullptr) {
        if (grew) *grew = n > size();
        if (n <= size()) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(st);
        return e == hipSuccess ? alloc(n) : e;
    }
    hipError_t zero(hipStream_t st) { return hipMemsetAsync(get(), 0, size() * sizeof(T), st); }      // ENQUEUED
    size_t size() const { return p_ ? n_ : 0; }
    T* get() const { return p_.get(); }
    operator T*() const { return get(); }

private:
    hipError_t take(hipError_t e, T* p, size_t n) {
        p_.reset(p);
        n_ = n;
        if (e != hipSuccess) reset();      // (allocated, but its poison fill failed)
        return e;
    }
    static hipError_t release(T* p) { return hipFree(p); }
    Held<T, release> p_;
    size_t n_ = 0;
};

// n elements of pinned host memory; a mapped one also carries the address the device reads and writes it at
template <class T>
class PinnedBuf {
public:
    void reset() { p_.reset(); }
    hipError_t alloc(size_t n) { return alloc_flags(n, hipHostMallocDefault); }
    hipError_t alloc_mapped(size_t n) {
        hipError_t e = alloc_flags(n, hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&dev_, get(), 0);
        if (e != hipSuccess) reset();
        return e;
    }
    size_t size() const { return p_ ? n_ : 0; }
    T* get() const { return p_.get(); }
    T* dev() const { return p_ ? dev_ : nullptr; }      // null unless mapped
    operator T*() const { return get(); }
    T* operator->() const { return get(); }

private:
    hipError_t alloc_flags(size_t n, unsigned flags) {
        reset();
        T* p = nullptr;
        const hipError_t e = hipHostMalloc((void**)&p, n * sizeof(T), flags);
        if (e == hipSuccess) p_.reset(p);
        n_ = n;
        dev_ = nullptr;
        return e;
    }
    static hipError_t release(T* p) { return hipHostFree(p); }
    Held<T, release> p_;
    T* dev_ = nullptr;
    size_t n_ = 0;
};

// An event or a stream, created with the flags its site asks for
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
class Handle {
public:
    void reset() { h_.reset(); }
    hipError_t create(unsigned flags = 0) {      // (0: hipEventDefault, an event that can be timed)
        reset();
        H h = nullptr;
        const hipError_t e = Create(&h, flags);
        if (e == hipSuccess) h_.reset(h);
        return e;
    }
    operator H() const { return h_.get(); }

private:
    Held<std::remove_pointer_t<H>, Destroy> h_;
};
using Event = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

}  // namespace llmk
