// mvhdp_scratch.h — the one place call-scoped device memory is owned: an array of T on the device that hipFree()s itself on scope
// exit, with the byte counts of its allocation, copies and memset derived from T.  Buffers that live as long as a handle or a group
// are not its business; one whose ownership passes to the handle on success is release()d into it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

template <class T> struct DevArray {
    T* p = nullptr;
    size_t n = 0;
    DevArray() = default;
    DevArray(const DevArray&) = delete;
    DevArray& operator=(const DevArray&) = delete;
    ~DevArray() { if (p) hipFree(p); }
    hipError_t alloc(size_t count)
    {
        if (p) { hipFree(p); p = nullptr; }
        n = 0;
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, count ? count * sizeof(T) : 1);
        if (e != hipSuccess) return e;
        p = (T*)q; n = count;
        return hipSuccess;
    }
    hipError_t upload(const T* src, size_t count, hipStream_t s)
    {
        return count > n ? hipErrorInvalidValue : hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s);
    }
    hipError_t download(T* dst, size_t count, hipStream_t s) const
    {
        return count > n ? hipErrorInvalidValue : hipMemcpyAsync(dst, p, count * sizeof(T), hipMemcpyDeviceToHost, s);
    }
    hipError_t fill(int byte, hipStream_t s) { return hipMemsetAsync(p, byte, n * sizeof(T), s); }
    operator T*() const { return p; }
    T* get() const { return p; }
    size_t size() const { return n; }
    T* release() { T* q = p; p = nullptr; n = 0; return q; }
};
