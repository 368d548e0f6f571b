// What every file of the C ABI needs: the error text, the HIP status macros,
// device buffers, events, a device with a stream.
#pragma once

#include <hip/hip_runtime.h>

#include "setup_core.hpp"

struct adx_params {
    adx::EnergyParams P;
};

namespace adx {

// sets the calling thread's adx_last_error text (api_base.cpp) and returns s
adx_status fail(adx_status s, const char *fmt, ...);
inline adx_status fail(const SetupError &e) { return fail(e.status, "%s", e.text.c_str()); }

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(ADX_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));         \
    } while (0)

// the same, with out-of-memory as ADX_ENOMEM and the sticky error cleared
#define MEM_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ == hipErrorOutOfMemory) {                                                   \
            (void)hipGetLastError();                                                       \
            return fail(ADX_ENOMEM, "%s: out of device memory", #expr);                    \
        }                                                                                  \
        if (e_ != hipSuccess)                                                              \
            return fail(ADX_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));         \
    } while (0)

constexpr int PICK_MAX_STEPS = 1 << 30;   // the longest record or trajectory of the pick / autocorrelation calls

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count) {
        reset();
        n = count;
        return hipMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(count, 1) * sizeof(T));
    }
    hipError_t upload(const T *src, size_t count, hipStream_t s) {
        hipError_t e = alloc(count);
        if (e != hipSuccess) return e;
        return hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s);
    }
};

// the events of one call: created on demand, destroyed with the guard
struct Events {
    std::vector<hipEvent_t> v;
    ~Events() {
        for (auto e : v)
            if (e) (void)hipEventDestroy(e);
    }
    adx_status create(size_t n) {
        v.assign(n, nullptr);
        for (auto &e : v) HIP_TRY(hipEventCreate(&e));
        return ADX_OK;
    }
    hipEvent_t operator[](size_t k) const { return v[k]; }
};

// n characters to base codes on the device; returns once they are there
inline adx_status upload_codes(const char *seqs, size_t n, DevBuf<uint8_t> &dseq, hipStream_t stream) {
    std::vector<uint8_t> codes(n);
    for (size_t k = 0; k < n; k++) codes[k] = static_cast<uint8_t>(base_code(seqs[k]));
    hipError_t e = dseq.upload(codes.data(), n, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);   // codes is this call's local
    if (e != hipSuccess)   // the text of the calls this replaces
        return fail(ADX_EHIP, "dseq.upload(codes.data(), codes.size(), pb.stream) failed: %s", hipGetErrorString(e));
    return ADX_OK;
}

// A gfx950 device and a non-blocking stream on it
struct DeviceStream {
    int device = 0;
    hipStream_t stream = nullptr;
    ~DeviceStream() {
        if (stream) (void)hipStreamDestroy(stream);
    }
    adx_status open(int dev) {
        device = dev;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            return fail(ADX_ENODEV, "no HIP device visible (the engine requires a gfx950 GPU)");
        if (device < 0 || device >= ndev) return fail(ADX_ENODEV, "device %d not present (%d visible)", device, ndev);
        HIP_TRY(hipSetDevice(device));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(ADX_ENODEV, "device %d is %s, the kernels are built for gfx950", device, prop.gcnArchName);
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return ADX_OK;
    }
};

}  // namespace adx
