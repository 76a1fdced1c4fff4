// Shared by the C-ABI translation units (ltm_capi.hip, vqf_capi.hip): error reporting and device buffers.
#pragma once
#include "knobs.h"
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <initializer_list>

#include "../../include/infv_ltm.h"
#include "vqf_internal.h"

namespace infv {

// Records the message returned by infv_ltm_last_error() (thread-local) and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return ::infv::fail(INFV_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// frame-token element types (tok_code): the codes the entry points accept (bytes per element: token_bytes, vqf_internal.h)
inline bool token_dtype_known(int dtype) {
    return dtype == INFV_TOKENS_F32 || dtype == INFV_TOKENS_BF16 || dtype == INFV_TOKENS_F16 || dtype == INFV_TOKENS_F8E4M3;
}
// fp8 tokens are read in 4- and 16-byte vectors from wherever `k` / `frames` starts: the address must be 16-byte aligned
inline bool token_ptr_ok(tok_code tok, const void* p) { return tok != INFV_TOKENS_F8E4M3 || (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

struct DeviceBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    ~DeviceBuf() { if (p) (void)hipFree(p); }
    hipError_t reserve(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; bytes = 0; if (e != hipSuccess) return e; }
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// Workspace growth: every listed buffer ends up with at least its size (0: left alone).  If any of them must grow, the device is
// synchronised once, before the first is freed -- work in flight may still read the old allocation.  No host allocation: this runs
// on the launch-bound per-chunk path.  *grew (optional): whether a buffer was reallocated, i.e. lost its contents.
struct BufNeed { DeviceBuf& buf; size_t bytes; };
inline hipError_t reserve_all(std::initializer_list<BufNeed> needs, bool* grew = nullptr) {
    bool grow = false;
    for (const BufNeed& n : needs) grow = grow || n.bytes > n.buf.bytes;
    if (grew) *grew = grow;
    if (!grow) return hipSuccess;
    hipError_t e = hipDeviceSynchronize();
    for (const BufNeed& n : needs)
        if (e == hipSuccess) e = n.buf.reserve(n.bytes);
    return e;
}

template <class T>
hipError_t upload(DeviceBuf& buf, const T* host, size_t n) {
    hipError_t e = buf.reserve((n ? n : 1) * sizeof(T));
    if (e != hipSuccess || n == 0) return e;
    return hipMemcpy(buf.p, host, n * sizeof(T), hipMemcpyHostToDevice);
}

}  // namespace infv
