// What the host translation units of the C ABI share below the handle: the error text of the calling thread, the HIP error check and a
// scoped device buffer for the vio_stage_* entry points (abi_stage.hip, stage_linalg.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "../../include/vio_abi.h"

extern thread_local std::string g_err;   // last failure of the calling thread (vio_last_error); defined in vio_abi.hip

#define HIPCHK(x)                                                                                        \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess) { g_err = std::string(#x) + ": " + hipGetErrorString(e_); return VIO_EDEVICE; } \
    } while (0)

// `count` elements of T in HBM for the duration of a scope.  Every member returns the hipError_t of its one HIP call, for HIPCHK.
template <class T> struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t count) { return hipMalloc((void **)&p, count * sizeof(T)); }
    hipError_t upload(const T *src, size_t count, size_t first = 0) { return hipMemcpy(p + first, src, count * sizeof(T), hipMemcpyHostToDevice); }
    hipError_t download(T *dst, size_t count, size_t first = 0) const { return hipMemcpy(dst, p + first, count * sizeof(T), hipMemcpyDeviceToHost); }
    operator T *() const { return p; }
};
