// apd_host.h — the host scaffolding the five device contexts of libapd_hip.so share (apd_ctx,
// apd_fusion_ctx, apd_eval_ctx, apd_prep_ctx, apd_seg_ctx): owned device buffers, the context base,
// the HIP status check, the opening of every *_create. Host code over the HIP runtime, for the .hip
// translation units only (the host twins *_host.cpp link no device library).
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/apd_hip.h"

// A device allocation and its owner: freed with the buffer (the context's device current, which every
// *_destroy sees to before it deletes the context). p != nullptr exactly when bytes > 0.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            if (p) (void)hipFree(p);
            p = o.p, bytes = o.bytes;
            o.p = nullptr, o.bytes = 0;
        }
        return *this;
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

// What every context starts with. held: the bytes of its DevBufs, kept by grow() and release().
// alloc_lib: the library named in grow()'s message ("<lib>: device allocation of N bytes failed");
// nullptr words it as the engine does ("hipMalloc(N) failed").
struct DevCtx {
    explicit DevCtx(const char *lib) : alloc_lib(lib) {}
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    size_t held = 0;
    const char *const alloc_lib;
};

#define HIP_OK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
            return APD_EDEVICE;                                                                    \
        }                                                                                          \
    } while (0)

inline void release(DevCtx *ctx, DevBuf &b) {
    ctx->held -= b.bytes;
    b = DevBuf();
}

// b emptied, then allocated anew. A failure leaves b empty and no error behind in the runtime:
// hipGetLastError() returns the last error of any runtime call, so the launch checks of the next,
// valid call would otherwise report this one's.
inline hipError_t reallocate(DevCtx *ctx, DevBuf &b, size_t bytes) {
    release(ctx, b);
    const hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        (void)hipGetLastError();
        return e;
    }
    b.bytes = bytes;
    ctx->held += bytes;
    return hipSuccess;
}

// b holds at least `bytes` afterwards (zero asks for 16; a buffer that is large enough is kept), or
// APD_ENOMEM with b empty
inline int grow(DevCtx *ctx, DevBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return APD_OK;
    if (reallocate(ctx, b, bytes) != hipSuccess) {
        const std::string n = std::to_string(bytes);
        ctx->err = ctx->alloc_lib ? std::string(ctx->alloc_lib) + ": device allocation of " + n + " bytes failed"
                                  : "hipMalloc(" + n + ") failed";
        return APD_ENOMEM;
    }
    return APD_OK;
}

// milliseconds from e0 to e1 (both recorded and complete)
inline int event_ms(DevCtx *ctx, hipEvent_t e0, hipEvent_t e1, double &ms) {
    float f = 0.0f;
    HIP_OK(ctx, hipEventElapsedTime(&f, e0, e1));
    ms = (double)f;
    return APD_OK;
}

// The opening of every *_create: the device index checked, the device made current, a context made
// and its non-blocking stream created. nullptr (and nothing left behind) when a step fails; *why says
// which, for the engine's messages.
enum OpenStep { OPEN_OK = 0, OPEN_NO_DEVICE, OPEN_BAD_INDEX, OPEN_SET_DEVICE, OPEN_STREAM };

template <class Ctx>
inline Ctx *open_ctx(int device, OpenStep *why = nullptr) {
    OpenStep w = OPEN_OK;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) w = OPEN_NO_DEVICE;
    else if (device < 0 || device >= n) w = OPEN_BAD_INDEX;
    else if (hipSetDevice(device) != hipSuccess) w = OPEN_SET_DEVICE;
    Ctx *ctx = nullptr;
    if (w == OPEN_OK) {
        ctx = new Ctx();
        ctx->device = device;
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
            delete ctx;
            ctx = nullptr;
            w = OPEN_STREAM;
        }
    }
    if (why) *why = w;
    return ctx;
}
