// capi_internal.h — shared by the translation units that implement the C ABI (not installed, not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include "host/owned_buf.h"

// records the message for slam_last_error() and returns `code`
extern "C" int slam_internal_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// slam_error_stats into a DEVICE buffer of `pad` doubles on the handle's device (entries past the batch are zero), complete when the
// call returns (the handle's stream is synchronised): the send buffer of slam_multi_error_stats' RCCL gather
struct slam_handle;
extern "C" int slam_internal_error_stats_dev(slam_handle* h, double* d_out, long long pad);

// (The runtime's "last error" is sticky and per thread: a launcher that ends in hipGetLastError() would report an error some OTHER library
// of the process left behind - PyTorch creating a stream right before slam_init did exactly that in a test.  It is cleared before every
// call; our own calls are all checked through their return values.)
#define HIP_TRY(expr)                                                                                            \
    do {                                                                                                         \
        (void)hipGetLastError();                                                                                 \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) return slam_internal_fail(SLAM_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(e_)); \
    } while (0)

#define TRY(expr)                       \
    do {                                \
        const int rc_ = (expr);         \
        if (rc_ != SLAM_OK) return rc_; \
    } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Allocation policies of slam_host::Buf: the only places the library allocates or frees device and pinned host memory.  A failed
// allocation leaves nothing behind in the runtime's sticky last error.
inline hipError_t alloc_result(hipError_t e) { if (e != hipSuccess) (void)hipGetLastError(); return e; }
struct DeviceAlloc {
    static hipError_t alloc(void** p, size_t bytes) { return alloc_result(hipMalloc(p, bytes)); }
    static void release(void* p) { (void)hipFree(p); }
};
template <unsigned Flags> struct PinnedAlloc {
    static hipError_t alloc(void** p, size_t bytes) { return alloc_result(hipHostMalloc(p, bytes, Flags)); }
    static void release(void* p) { (void)hipHostFree(p); }
};
template <class T> using DevBuf = slam_host::Buf<T, DeviceAlloc>;
template <class T> using PinnedBuf = slam_host::Buf<T, PinnedAlloc<hipHostMallocNonCoherent>>;   // CPU-cached: fast to fill
template <class T> using PinnedDefaultBuf = slam_host::Buf<T, PinnedAlloc<hipHostMallocDefault>>;
