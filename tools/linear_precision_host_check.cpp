// Host-side check of infv_vqf_set_linear_precision (and of the argument validation of infv_vqf_linear) under the address and
// undefined-behaviour sanitizers: a stand-alone program (its own main, no GPU, not loaded into Python).  Build and run:
//
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/linear_precision_host_check.cpp infinite-video_amd/csrc/*.hip -o linear_precision_host_check && ./linear_precision_host_check
//
// A development aid in the manner of token_dtype_host_check.cpp, tied to the handle's internals: zeroed bytes stand in for the
// handle struct, which works only while the setter checks the handle for null alone, finds an all-zero plane cache empty (nothing
// to drop: no device call) and writes nothing but the mode field, whose fp32 code is 0; formally that is undefined behaviour on
// this non-trivial struct.  If the handle gains a validity check, give this program a real handle.
// Checked: a null handle is refused whatever the mode; on the dummy handle modes 0, 1 and 2 are taken and every other value is
// refused and changes nothing; back on mode 0 the storage is all zeros again; infv_vqf_linear refuses bad arguments before it
// reads the handle's state.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "infv_ltm.h"
#include "infv_vqf.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    const int known[] = {0, 1, 2};
    const int unknown[] = {3, 7, -1, 16, 255, -2147483647 - 1, 2147483647};
    for (int m : known) EXPECT(infv_vqf_set_linear_precision(nullptr, m) == INFV_ERR_INVALID);
    for (int m : unknown) EXPECT(infv_vqf_set_linear_precision(nullptr, m) == INFV_ERR_INVALID);
    EXPECT(std::strstr(infv_ltm_last_error(), "null") != nullptr);
    const size_t kDummy = 1u << 20;                     // far larger than the handle
    void* a = std::calloc(1, kDummy);
    void* a0 = std::malloc(kDummy);
    if (!a || !a0) return 2;
    infv_vqf_handle h = static_cast<infv_vqf_handle>(a);
    for (int m : known) {
        EXPECT(infv_vqf_set_linear_precision(h, m) == INFV_OK);
        std::memcpy(a0, a, kDummy);
        for (int bad : unknown) {
            EXPECT(infv_vqf_set_linear_precision(h, bad) == INFV_ERR_INVALID);
            EXPECT(std::strstr(infv_ltm_last_error(), "unknown mode") != nullptr);
        }
        EXPECT(std::memcmp(a0, a, kDummy) == 0);        // a refusal changes nothing
        // the setting is kept: in modes 1 and 2 every other entry point still refuses, before it reads anything else of the handle
        alignas(16) static float buf[64];
        infv_linear kv{buf, buf};
        if (m != 0) {
            EXPECT(infv_vqf_short_attention(h, buf, 64, buf, &kv, &kv, nullptr, buf, nullptr) == INFV_ERR_UNSUPPORTED);
            EXPECT(std::strstr(infv_ltm_last_error(), "infv_vqf_set_linear_precision") != nullptr);
            EXPECT(infv_vqf_vc_embed(h, reinterpret_cast<const infv_vqf_vc_front*>(buf), 0, reinterpret_cast<const int32_t*>(buf), nullptr, nullptr)
                   == INFV_ERR_UNSUPPORTED);
            EXPECT(std::memcmp(a0, a, kDummy) == 0);    // ... before any workspace change
        }
    }
    // the setter writes the mode field and nothing else: back on fp32 the storage is all zeros again
    EXPECT(infv_vqf_set_linear_precision(h, 0) == INFV_OK);
    std::memset(a0, 0, kDummy);
    EXPECT(std::memcmp(a0, a, kDummy) == 0);
    // infv_vqf_linear: every refusal comes before the handle's state is read or a launch is tried
    alignas(16) static float x[64 * 64];
    infv_linear lin[5] = {{x, x}, {x, x}, {x, x}, {x, x}, {x, x}};
    infv_layernorm half_ln{x, nullptr};
    EXPECT(infv_vqf_linear(nullptr, x, 1, 64, lin, 1, 64, 0, nullptr, 1, nullptr, x, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_linear(h, nullptr, 1, 64, lin, 1, 64, 0, nullptr, 1, nullptr, x, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_linear(h, x, 0, 64, lin, 1, 64, 0, nullptr, 1, nullptr, x, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_linear(h, x, 1, 64, lin, 0, 64, 0, nullptr, 1, nullptr, x, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_linear(h, x, 1, 64, lin, 5, 64, 0, nullptr, 1, nullptr, x, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_linear(h, x, 1, 96, lin, 1, 64, 0, nullptr, 1, nullptr, x, nullptr) == INFV_ERR_UNSUPPORTED);
    EXPECT(infv_vqf_linear(h, x, 1, 64, lin, 1, 32, 0, nullptr, 1, nullptr, x, nullptr) == INFV_ERR_UNSUPPORTED);
    EXPECT(infv_vqf_linear(h, x, 1, 4160, lin, 1, 64, 0, nullptr, 1, nullptr, x, nullptr) == INFV_ERR_UNSUPPORTED);
    EXPECT(infv_vqf_linear(h, x, 1, 64, lin, 3, 2048, 0, nullptr, 1, nullptr, x, nullptr) == INFV_ERR_UNSUPPORTED);
    EXPECT(infv_vqf_linear(h, x, 1, 64, lin, 1, 64, 2, nullptr, 1, nullptr, x, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_linear(h, x, 1, 64, lin, 1, 64, 0, x, 0, nullptr, x, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_linear(h, x, 1, 64, lin, 1, 64, 0, nullptr, 1, &half_ln, x, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_linear(h, x + 1, 1, 64, lin, 1, 64, 0, nullptr, 1, nullptr, x, nullptr) == INFV_ERR_INVALID);
    EXPECT(std::strstr(infv_ltm_last_error(), "16-byte") != nullptr);
    lin[0].w = nullptr;
    EXPECT(infv_vqf_linear(h, x, 1, 64, lin, 1, 64, 0, nullptr, 1, nullptr, x, nullptr) == INFV_ERR_INVALID);
    EXPECT(std::memcmp(a0, a, kDummy) == 0);
    std::free(a); std::free(a0);
    std::printf(failures ? "linear precision host check: %d FAILED\n" : "linear precision host check: ok\n", failures);
    return failures ? 1 : 0;
}
