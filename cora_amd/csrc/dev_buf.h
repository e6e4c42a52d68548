// dev_buf.h - the one owner of a hipMalloc allocation in libcorahip.so: plan tables, context caches, per-call buffers.
// Host code only, and nothing of HIP beyond the runtime API header, so a plain host compiler builds it
// (tools/dev_buf_test.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <vector>

// Move-only.  Converts to T * by itself, so launch lines and `if (p->d_x)` tests read as they do for a raw pointer; a
// kernel template that deduces its pointer parameter needs .get().
template <class T>
struct dev_buf {
    dev_buf() = default;
    dev_buf(const dev_buf &) = delete;
    dev_buf &operator=(const dev_buf &) = delete;
    dev_buf(dev_buf &&o) noexcept : p(o.p) { o.p = nullptr; }
    dev_buf &operator=(dev_buf &&o) noexcept {
        if (this != &o) {
            (void)reset();
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    // hipFree waits for the device, so freeing on an error return behind queued launches that still use the buffer is safe
    ~dev_buf() { (void)reset(); }

    // releases what is held, then allocates count elements; empty on failure
    hipError_t alloc(size_t count) {
        (void)reset();
        const hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    // alloc of max(1, h.size()) elements + a copy of h on stream s, waited for (h may go away); empty on failure
    hipError_t upload(const std::vector<T> &h, hipStream_t s) {
        hipError_t e = alloc(h.empty() ? 1 : h.size());
        if (e == hipSuccess && !h.empty()) {
            e = hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) (void)reset();
        }
        return e;
    }
    // frees what is held (the status of hipFree; success when empty); may be called again
    hipError_t reset() {
        T *q = p;
        p = nullptr;
        return q ? hipFree(q) : hipSuccess;
    }
    T *get() const { return p; }
    operator T *() const { return p; }

private:
    T *p = nullptr;
};
