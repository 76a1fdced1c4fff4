// Host-side check of what infv_ltm_source_weights refuses before any device work, under the address and undefined-behaviour
// sanitizers: a stand-alone program (its own main, no GPU, not loaded into Python).  Build and run
// (tests/test_source_weights_cpu.py does):
//
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined -I include \
//         tools/sources_host_check.cpp infinite-video_amd/csrc/ltm_sources.hip -o sources_host_check && ./sources_host_check
//
// Only ltm_sources.hip is linked: the two symbols it takes from ltm_capi.hip (the error text, the launch counter) are stood in
// for below.  The handle is a real infv_ltm_s with plans that have no device memory behind them, so every call made here must
// return before it touches the device -- which is what the header promises of these refusals.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../infinite-video_amd/csrc/ltm_handle.h"

namespace infv {
thread_local char g_err[512] = "";
std::atomic<long long> g_kernel_launches{0};
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace infv

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s  [%s]\n", __LINE__, #cond, infv::g_err); ++failures; } } while (0)

int main() {
    infv_ltm_s* h = new infv_ltm_s();
    std::memset(&h->cfg, 0, sizeof(h->cfg));
    h->N = 64; h->H = 12; h->L = 2; h->maxQ = 32; h->dh = 64; h->d = 768; h->dm = 768; h->P = 32; h->S = 512; h->maxC = 32;
    h->cfg.sticky = 1;
    h->plans[8] = new infv::Plan();                       // a sparse plan for T = 8 (its tables are never reached)
    h->plans[8]->T = 8; h->plans[8]->n_bins = 128;
    h->plans[16] = new infv::Plan();                      // a dense plan for T = 16
    h->plans[16]->T = 16; h->plans[16]->dense.on = true;
    h->plans[32] = new infv::Plan();                      // a general-psi plan for T = 32
    h->plans[32]->T = 32; h->plans[32]->dense.on = true; h->plans[32]->dense.psi_on = true;

    alignas(16) static float W[8];
    static int32_t bins[4];
    static float mass[4], attn[4];
    infv_ltm_sources_desc ok = {3, 8, 1, 1, 0, 24};
    auto call5 = [&](infv_ltm_sources_desc d, const int32_t* b, float* w, const float* m, float* a) {
        return infv_ltm_source_weights(h, &d, b, w, m, a, nullptr, nullptr);
    };
    auto call = [&](infv_ltm_sources_desc d) { return call5(d, bins, W, nullptr, nullptr); };
    auto with = [&](auto edit) { infv_ltm_sources_desc d = ok; edit(d); return d; };

    EXPECT(infv_ltm_source_weights(nullptr, &ok, bins, W, nullptr, nullptr, nullptr, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_ltm_source_weights(h, nullptr, bins, W, nullptr, nullptr, nullptr, nullptr) == INFV_ERR_INVALID);
    EXPECT(call5(ok, bins, nullptr, nullptr, nullptr) == INFV_ERR_INVALID);                                            // null W
    EXPECT(call(with([](auto& d) { d.n_chunks = 0; })) == INFV_ERR_INVALID);
    EXPECT(call(with([](auto& d) { d.n_chunks = -3; })) == INFV_ERR_INVALID);
    EXPECT(call(with([](auto& d) { d.T = 0; })) == INFV_ERR_INVALID);
    EXPECT(call(with([](auto& d) { d.frames_per_source = 0; })) == INFV_ERR_INVALID);
    EXPECT(call(with([](auto& d) { d.frames_per_source = 3; })) == INFV_ERR_INVALID);             // 3 does not divide 8
    EXPECT(call(with([](auto& d) { d.frames_per_source = 16; })) == INFV_ERR_INVALID);            // nor does 16
    EXPECT(call(with([](auto& d) { d.col_begin = -1; })) == INFV_ERR_INVALID);
    EXPECT(call(with([](auto& d) { d.col_begin = (int64_t)1 << 62; d.ld = (int64_t)1 << 62; })) == INFV_ERR_INVALID);   // no overflow on the way
    EXPECT(call(with([](auto& d) { d.ld = 20; })) == INFV_ERR_INVALID);                           // below 3 * 8
    EXPECT(call(with([](auto& d) { d.ld = 26; })) == INFV_ERR_INVALID);                           // no multiple of 4
    EXPECT(call(with([](auto& d) { d.col_begin = 4; })) == INFV_ERR_INVALID);                     // 4 + 24 > 24
    EXPECT(call5(ok, bins, W + 1, nullptr, nullptr) == INFV_ERR_INVALID);                                              // W off a 16-byte boundary
    EXPECT(call5(ok, nullptr, W, nullptr, nullptr) == INFV_ERR_INVALID);                                                  // sticky, no bins
    EXPECT(call5(ok, bins, W, mass, nullptr) == INFV_ERR_INVALID);                                   // mass_all without attn_all
    EXPECT(call5(ok, bins, W, nullptr, attn) == INFV_ERR_INVALID);                                   // ... and the other way round
    EXPECT(call(with([](auto& d) { d.T = 4; d.ld = 12; })) == INFV_ERR_STATE);                    // no plan for T = 4
    EXPECT(std::strstr(infv::g_err, "no plan") != nullptr);
    EXPECT(call(with([](auto& d) { d.T = 16; d.ld = 48; })) == INFV_ERR_UNSUPPORTED);             // dense
    EXPECT(call(with([](auto& d) { d.T = 32; d.ld = 96; })) == INFV_ERR_UNSUPPORTED);             // general psi
    h->N = 528;
    EXPECT(call(ok) == INFV_ERR_UNSUPPORTED);                                                       // num_basis above 512
    h->N = 64;
    h->cfg.sticky = 0;
    EXPECT(call(ok) == INFV_ERR_INVALID);                                                           // bins on a handle that is not sticky
    EXPECT(infv::g_kernel_launches.load() == 0);
    for (int i = 0; i < 8; ++i) EXPECT(W[i] == 0.f);
    delete h;
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("sources host check: ok\n");
    return 0;
}
