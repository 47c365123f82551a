// hs_host.hpp -- the host-side helpers every translation unit of libhs_hip.so shares: the formatted `fail`, the HIP-check macro,
// the tracked device allocation and the upload of a (possibly absent) host column.  Templates over the handle type: hs_engine,
// hs_lb and hs_graph all have `error`; the first two also `allocs`, which their destroy functions free.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/hs_engine.h"

namespace {

// the last error of a call without a handle.  One store per translation unit, on purpose: hs_last_global_error(),
// hs_lb_last_error(NULL) and hs_graph_last_error(NULL) are read independently
thread_local std::string g_last_error;

inline int vfail(std::string *handle_error, int code, const char *fmt, va_list ap) {
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    if (handle_error) *handle_error = buf;
    g_last_error = buf;
    return code;
}
template <typename H>
int fail(H *h, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int rc = vfail(h ? &h->error : nullptr, code, fmt, ap);
    va_end(ap);
    return rc;
}
inline int fail(std::nullptr_t, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int rc = vfail(nullptr, code, fmt, ap);
    va_end(ap);
    return rc;
}

#define HS_HIP(h, expr)                                                                                \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(h, HS_E_HIP, "%s: %s", #expr, hipGetErrorString(e_));        \
    } while (0)

template <typename T, typename H>
int dev_alloc(H *h, T **p, size_t count) {
    void *q = nullptr;
    const size_t bytes = count * sizeof(T) ? count * sizeof(T) : sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(h, HS_E_HIP, "hipMalloc(%zu B): %s", count * sizeof(T), hipGetErrorString(e));
    h->allocs.push_back(q);
    *p = (T *)q;
    // debug: HS_POISON_ALLOC=<byte> fills every device allocation with that byte -- nothing may depend on what hipMalloc hands out
    // (memory of an engine destroyed earlier in the process): tests/test_gpu_sharded.py::test_nothing_depends_on_what_the_allocator_hands_out
    static const char *poison = getenv("HS_POISON_ALLOC");
    if (poison && *poison) (void)hipMemset(q, (int)strtol(poison, nullptr, 0) & 0xff, bytes);
    return HS_OK;
}

// a host column on the device; an absent one (src == nullptr) as n copies of its default
template <typename T, typename H>
int upload(H *h, const T **dst, const T *src, size_t n, T dflt) {
    T *d = nullptr;
    int rc = dev_alloc(h, &d, n);
    if (rc) return rc;
    std::vector<T> tmp;
    if (!src) { tmp.assign(n, dflt); src = tmp.data(); }
    hipError_t e = hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(h, HS_E_HIP, "hipMemcpy H2D: %s", hipGetErrorString(e));
    *dst = d;
    return HS_OK;
}

}  // namespace
