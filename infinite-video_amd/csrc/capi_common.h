// Shared by the C-ABI translation units (the ltm_* host units, vqf_capi.hip, vqf_video.hip, vqf_vc.hip): error reporting and device buffers.
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
// Sets of buffers (a ring, the rotating workspace sets) go in through add_each: a fixed-capacity list on the stack.
struct BufList {
    static constexpr int kCap = 48;
    DeviceBuf* buf[kCap]; size_t bytes[kCap]; int n = 0;
    BufList() {}
    BufList& add(DeviceBuf& b, size_t need) { if (n < kCap) { buf[n] = &b; bytes[n] = need; } ++n; return *this; }   // (past kCap: reserve_all fails)
    template <int K> BufList& add_each(DeviceBuf (&bs)[K], size_t need, int count = K) { for (int i = 0; i < count; ++i) add(bs[i], need); return *this; }
};
inline hipError_t reserve_all(const BufList& l, bool* grew = nullptr) {
    if (l.n > BufList::kCap) return hipErrorInvalidValue;
    bool grow = false;
    for (int i = 0; i < l.n; ++i) grow = grow || l.bytes[i] > l.buf[i]->bytes;
    if (grew) *grew = grow;
    if (!grow) return hipSuccess;
    hipError_t e = hipDeviceSynchronize();
    for (int i = 0; i < l.n && e == hipSuccess; ++i) e = l.buf[i]->reserve(l.bytes[i]);
    return e;
}
inline hipError_t reserve_all(std::initializer_list<BufNeed> needs, bool* grew = nullptr) {
    BufList l;
    for (const BufNeed& n : needs) l.add(n.buf, n.bytes);
    return reserve_all(l, grew);
}

// An event of a fused call that knows whether THIS call has recorded it: a wait for a record of an earlier call would order
// nothing that stream order does not already (wait_on is then a no-op; wait_always is the plain wait).  clear() at the start of a call.
struct CallEvent {
    hipEvent_t ev = nullptr; bool recorded = false;
    CallEvent() = default;
    CallEvent(const CallEvent&) = delete;
    CallEvent& operator=(const CallEvent&) = delete;
    ~CallEvent() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t create() { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
    hipError_t record(hipStream_t s) { recorded = true; return hipEventRecord(ev, s); }
    hipError_t wait_on(hipStream_t s) const { return recorded ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
    hipError_t wait_always(hipStream_t s) const { return hipStreamWaitEvent(s, ev, 0); }
    void clear() { recorded = false; }
};

template <class T>
hipError_t upload(DeviceBuf& buf, const T* host, size_t n) {
    hipError_t e = buf.reserve((n ? n : 1) * sizeof(T));
    if (e != hipSuccess || n == 0) return e;
    return hipMemcpy(buf.p, host, n * sizeof(T), hipMemcpyHostToDevice);
}

}  // namespace infv
