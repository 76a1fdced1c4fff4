// Environment knobs of libinfv_ltm.so.
//
// The shipped library reads five documented options from the environment (all parity-tested; see README.md):
//   INFV_PROJ_X6, INFV_VPROJ_SPLIT, INFV_VQF_FP32, INFV_VQF_FUSE, INFV_VQF_SPLIT_CACHE_GB   -> plain getenv at their call sites.
// Everything else -- timing experiments that produce garbage (INFV_SKIP, INFV_S_FLAGS), in-kernel stamps, fault
// injection, occupancy pads, stream priorities and the A/B selectors of variants that are not the default -- goes through
// exp_env(), which only looks at the environment in the experiments build (-DINFV_EXPERIMENTS:
// libinfv_ltm_exp.so, what tools/ and the variant / fault-injection tests load through INFV_LTM_LIBRARY=exp).  In the
// shipped library exp_env() is a constant nullptr: no hidden work-skipping or tuning switch can change what it runs.
// A variant that was measured and rejected is deleted, selector and code together, rather than kept behind a knob: its
// measurements stay in profiles/ and docs/NOTEBOOK.md (so went round 5's call-long role S, resident GEMM and mailbox exchange,
// round 6's LDS-DMA loader of role S, the CU-mask experiment and the sub-batch schedule sweeps).
#pragma once
#include <cstdlib>

namespace infv {
inline const char* exp_env(const char* name) {
#ifdef INFV_EXPERIMENTS
    return std::getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}
// An integer / on-off knob of the experiments build with its shipped value (the call site keeps the caching `static`):
//   static const int sub_env = exp_int("INFV_SUB_BATCH", 0);
inline long exp_long(const char* name, long dflt) { const char* e = exp_env(name); return e ? std::atol(e) : dflt; }
inline int exp_int(const char* name, int dflt) { const char* e = exp_env(name); return e ? std::atoi(e) : dflt; }
inline bool exp_set(const char* name) { return exp_env(name) != nullptr; }
// a frame-token element type as the library carries it: one of the infv_token_dtype codes or INFV_TOKENS_F8E4M3 (infv_ltm.h).  A plain
// integer, not the enum: code 4 is declared beside the enum, outside the enumerators' range.
typedef int tok_code;
}  // namespace infv

// ---- launch census: every kernel launch of the library goes through INFV_LAUNCH (same argument order as hipLaunchKernelGGL); it
// counts them on the host (one relaxed atomic add per launch) so that a benchmark can state "launches per chunk" of a path without
// a profiler (infv_ltm_launch_count, include/infv_ltm.h).  tests/test_host_cpu.py checks that no source launches a kernel any other
// way (no raw <<< >>>, no hipLaunchKernelGGL, no hipModuleLaunchKernel).
#include <hip/hip_runtime.h>
#include <atomic>
namespace infv { extern std::atomic<long long> g_kernel_launches; }
#define INFV_LAUNCH(kernelName, numBlocks, numThreads, memPerBlock, streamId, ...)                                \
    do {                                                                                                          \
        ::infv::g_kernel_launches.fetch_add(1, std::memory_order_relaxed);                                        \
        (kernelName)<<<(numBlocks), (numThreads), (memPerBlock), (streamId)>>>(__VA_ARGS__);                      \
    } while (0)

// In-kernel stamp read-outs of the experiments build: a zeroed device buffer of `words` 64-bit stamps if the knob is set (else
// dev stays null and the kernel writes none); read() is true on every `every`-th call, after it has synchronised `stream` and
// copied the stamps to `host`.  The prints themselves stay with their launchers (tools/stamps*.sh parse them).
namespace infv {
struct StampBuf {
    long long* dev = nullptr; int words; int calls = 0;
    StampBuf(const char* knob, int words_) : words(words_) {
        if (exp_set(knob) && hipMalloc(&dev, words * sizeof(long long)) == hipSuccess) (void)hipMemset(dev, 0, words * sizeof(long long));
    }
    bool read(int every, hipStream_t stream, long long* host) {
        if (!dev || (++calls % every) != 0) return false;
        (void)hipStreamSynchronize(stream);
        (void)hipMemcpy(host, dev, words * sizeof(long long), hipMemcpyDeviceToHost);
        return true;
    }
};
}  // namespace infv
