// What the host side of every handle family shares (host only, header-only): the error text of a handle, the HIP-call check, the
// grid.y limit, the default feature profile, the grow-on-demand device scratch and the pack-and-upload-once table image.
// A family's handle is any struct with a `std::string err`.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/wavernn_amd.h"

// h->err = the formatted message, cut at 399 characters (h may be null); returns `code`.
template <class H>
__attribute__((format(printf, 3, 4))) int wrnn_failf(H *h, int code, const char *fmt, ...) {
    char buf[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return code;
}

// Leaves the calling entry with WRNN_ERR_HIP and "<the call as written>: <HIP's text>" when a HIP call fails.
#define WRNN_TRY(h, expr)                                                                                      \
    do {                                                                                                       \
        hipError_t e__ = (expr);                                                                               \
        if (e__ != hipSuccess) return wrnn_failf((h), WRNN_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

template <class H>
const char *wrnn_last_error_of(const H *h) {
    return h ? h->err.c_str() : "null handle";
}

constexpr int WRNN_MAX_GRID_Y = 65535;   // the batch of a call is grid.y (or grid.z) of its kernels

// The features of wavernn/utils/dsp.py: reflect padding, |X|, no pre-emphasis, direct normalisation, fmax = sample_rate / 2.
inline const wrnn_mel_features WRNN_DEFAULT_MEL_FEATURES = {(uint32_t)sizeof(wrnn_mel_features), WRNN_MEL_PAD_REFLECT, 1, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};

inline size_t wrnn_up256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// Device scratch of a handle, grown on demand and kept at its high-water mark.  The calls on one handle share it, so the caller orders
// those calls (one stream at a time).
struct WrnnScratch {
    char *p = nullptr;
    size_t cap = 0;   // bytes; 0 until an allocation succeeded

    // Growing is the one wait: an earlier call on `s` may still read the old buffer, so the stream is synchronised before the free.
    hipError_t reserve(size_t bytes, hipStream_t s) {
        if (bytes <= cap) return hipSuccess;
        hipError_t e;
        if (p) {
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
            if ((e = hipFree(p)) != hipSuccess) return e;
            p = nullptr;
            cap = 0;
        }
        if ((e = hipMalloc((void **)&p, bytes)) != hipSuccess) {
            p = nullptr;
            return e;
        }
        cap = bytes;
        return hipSuccess;
    }
    // The destroy path: the caller has set the device.
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// The host tables of a handle as one image of 256-byte aligned regions, uploaded once.
struct WrnnImage {
    std::vector<char> bytes;

    // the offset of a new zeroed region
    size_t take(size_t n) {
        const size_t o = bytes.size();
        bytes.resize(o + wrnn_up256(n), 0);
        return o;
    }
    // a region holding a copy of `n` bytes
    size_t put(const void *src, size_t n) {
        const size_t o = take(n);
        memcpy(bytes.data() + o, src, n);
        return o;
    }
    template <class T>
    T *at(size_t o) {
        return (T *)(bytes.data() + o);
    }
    // one allocation and one synchronous copy; nothing is left allocated on failure
    hipError_t upload(void **dev) const {
        void *d = nullptr;
        hipError_t e = hipMalloc(&d, bytes.size());
        if (e != hipSuccess) return e;
        e = hipMemcpy(d, bytes.data(), bytes.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return e;
        }
        *dev = d;
        return hipSuccess;
    }
};
