// A test-side stand-in for <hip/hip_runtime.h>: only what mvtopicmodel_amd/csrc/mvhdp_scratch.h and parts A and B of mvhdp_side.h use,
// on host memory, with a log of every call (tests/native/scratch_probe.cpp, tests/native/side_probe.cpp).  One translation unit includes it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

typedef enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 } hipError_t;
typedef enum { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 } hipMemcpyKind;
typedef struct ihipStream_t* hipStream_t;
typedef struct ihipEvent_t { float stamp; }* hipEvent_t;

struct HipStub {
    int fail_event_create_at = 0;          // the n-th hipEventCreate from now on (1: the next) returns hipErrorOutOfMemory; 0: none fails
    int events_created = 0, events_destroyed = 0, events_recorded = 0, events_timed = 0;
    float clock = 0.0f;                    // a record stamps its event with the clock and moves it on by one "millisecond"
    bool dry = false;                      // counter-based pointers that nothing dereferences: large counts cost nothing
    int fail_malloc_at = 0;                // the n-th hipMalloc from now on (1: the next) returns hipErrorOutOfMemory; 0: none fails
    std::set<void*> live;
    std::vector<size_t> malloc_bytes, copy_bytes, set_bytes;
    std::vector<hipMemcpyKind> copy_kind;
    std::vector<void*> freed;
    uintptr_t next_dry = 0x1000;
    void reset() { *this = HipStub(); }
};
inline HipStub g_hip;

inline hipError_t hipMalloc(void** p, size_t bytes)
{
    g_hip.malloc_bytes.push_back(bytes);
    if (g_hip.fail_malloc_at > 0 && --g_hip.fail_malloc_at == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    if (g_hip.dry) { *p = (void*)g_hip.next_dry; g_hip.next_dry += 0x1000; }
    else *p = malloc(bytes);               // exactly the bytes asked for: AddressSanitizer sees a copy or a memset that runs past them
    g_hip.live.insert(*p);
    return hipSuccess;
}
inline hipError_t hipFree(void* p)
{
    g_hip.freed.push_back(p);
    if (!g_hip.live.erase(p)) return hipErrorInvalidValue;
    if (!g_hip.dry) free(p);
    return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t)
{
    g_hip.copy_bytes.push_back(bytes); g_hip.copy_kind.push_back(kind);
    if (!g_hip.dry && bytes) memcpy(dst, src, bytes);
    return hipSuccess;
}
inline hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t)
{
    g_hip.set_bytes.push_back(bytes);
    if (!g_hip.dry && bytes) memset(dst, value, bytes);
    return hipSuccess;
}
// events: each its own allocation, so AddressSanitizer reports one that is never destroyed, destroyed twice or used afterwards
inline hipError_t hipEventCreate(hipEvent_t* e)
{
    if (g_hip.fail_event_create_at > 0 && --g_hip.fail_event_create_at == 0) return hipErrorOutOfMemory;   // *e is left as it was
    *e = new ihipEvent_t{-1.0f};
    g_hip.events_created++;
    return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e)
{
    if (!e) return hipErrorInvalidValue;
    delete e;
    g_hip.events_destroyed++;
    return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    if (!e) return hipErrorInvalidValue;
    e->stamp = g_hip.clock;
    g_hip.clock += 1.0f;
    g_hip.events_recorded++;
    return hipSuccess;
}
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b)
{
    if (!a || !b || a->stamp < 0.0f || b->stamp < 0.0f) return hipErrorInvalidValue;
    *ms = b->stamp - a->stamp;
    g_hip.events_timed++;
    return hipSuccess;
}
