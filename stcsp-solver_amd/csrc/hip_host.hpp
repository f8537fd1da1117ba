// hip_host.hpp -- host-side HIP plumbing of engine.hip and automaton.hip: a growable device buffer, HIPCHK, timing events.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "stcsp_engine.h"

namespace stcsp {

// what a buffer for `count` elements grows to: a quarter of slack, so that a slowly growing automaton does not reallocate every call
inline size_t grown(size_t count) { return count + count / 4 + 256; }

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count) {
        release();
        n = count;
        return hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T));
    }
    hipError_t upload(const std::vector<T> &v) {
        hipError_t e = alloc(v.size());
        if (e != hipSuccess) return e;
        if (!v.empty()) e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    // room for count + tail elements; a buffer that is too small grows to grown(count) + tail (the contents are lost)
    hipError_t reserve(size_t count, size_t tail = 0) { return n < count + tail ? alloc(grown(count) + tail) : hipSuccess; }
    // ... without the slack: the power-of-two tables, the per-variable arrays, the control blocks
    hipError_t reserve_exact(size_t count) { return n < count ? alloc(count) : hipSuccess; }
    // ... for the tables a byte budget bounds: false, with the buffer released and the error drained, when there is no room
    bool reserve_or_release(size_t count) {
        if (n >= count || alloc(count) == hipSuccess) return true;
        (void)hipGetLastError();
        release();
        return false;
    }
};

// reserve(count, tail) for several buffers of one size: the first error
template <typename... Bufs>
hipError_t reserve_all(size_t count, size_t tail, Bufs &...bufs) {
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? bufs.reserve(count, tail) : e), ...);
    return e;
}

// reserve_or_release(count) for every (buffer, count) pair, or for none: false with every buffer of the list released, those
// behind the one that failed too. ok: none has failed so far (true from outside)
template <typename T, typename... Rest>
bool reserve_or_release_all(bool ok, DevBuf<T> &buf, size_t count, Rest &&...rest) {
    ok = ok && buf.reserve_or_release(count);
    if constexpr (sizeof...(rest) > 0) ok = reserve_or_release_all(ok, rest...);
    if (!ok) buf.release();
    return ok;
}

// hipEvent_t's created on first use and destroyed with their owner
struct DevEvents {
    hipEvent_t ev[8] = {};
    ~DevEvents() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t ready(int count) {  // the first `count` (at most 8) events exist
        hipError_t e = hipSuccess;
        for (int i = 0; i < count && e == hipSuccess; i++)
            if (!ev[i]) e = hipEventCreate(&ev[i]);
        return e;
    }
    hipEvent_t operator[](int i) const { return ev[i]; }
    hipError_t mark(int k, hipStream_t stream) { return hipEventRecord(ev[k], stream); }
    // after the synchronise: *into[i] += the seconds from mark first + i to mark first + i + 1
    hipError_t add_spans(int first, std::initializer_list<double *> into) {
        hipError_t e = hipSuccess;
        for (double *seconds : into) {
            float ms = 0;
            if ((e = hipEventElapsedTime(&ms, ev[first], ev[first + 1])) != hipSuccess) break;
            *seconds += ms * 1e-3;
            first++;
        }
        return e;
    }
};

}  // namespace stcsp

// for the members of a struct with `int fail(int code, const char *fmt, ...)`
#define HIPCHK(call)                                                                                        \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess) return fail(STCSP_E_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)
