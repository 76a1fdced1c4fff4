// Host-side check of infv_vqf_set_attention_precision and of the argument validation of infv_vqf_frame_cross_attention under the
// address and undefined-behaviour sanitizers: a stand-alone program (its own main, no GPU, not loaded into Python).  Build and run:
//
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/attention_precision_host_check.cpp infinite-video_amd/csrc/*.hip -o attention_precision_host_check && ./attention_precision_host_check
//
// A development aid in the manner of linear_precision_host_check.cpp, with its caveat: zeroed bytes stand in for the handle struct,
// which works only while the setter checks the handle for null alone, finds an all-zero plane cache empty (nothing to drop: no
// device call) and writes nothing but the mode field, whose default code is 0; formally that is undefined behaviour on this
// non-trivial struct.  The zeroed config reads as n_query 0 and enc_width 0, so only calls that are refused, or that have no frame,
// are made.
// Checked: a null handle is refused whatever the mode; on the dummy handle modes 0 and 1 are taken and every other value is refused
// and changes nothing; in mode 1 the other entry points refuse, naming the setter, before any workspace change; it is independent
// of the linear precision; back on mode 0 the storage is all zeros again; infv_vqf_frame_cross_attention refuses bad arguments
// before any launch or memory change, in both modes.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "infv_ltm.h"
#include "infv_vqf.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    const int known[] = {0, 1};
    const int unknown[] = {2, 3, 7, -1, 255, -2147483647 - 1, 2147483647};
    for (int m : known) EXPECT(infv_vqf_set_attention_precision(nullptr, m) == INFV_ERR_INVALID);
    for (int m : unknown) EXPECT(infv_vqf_set_attention_precision(nullptr, m) == INFV_ERR_INVALID);
    EXPECT(std::strstr(infv_ltm_last_error(), "null") != nullptr);
    const size_t kDummy = 1u << 20;                     // far larger than the handle
    void* a = std::calloc(1, kDummy);
    void* a0 = std::malloc(kDummy);
    if (!a || !a0) return 2;
    infv_vqf_handle h = static_cast<infv_vqf_handle>(a);
    alignas(16) static float buf[64 * 64];
    infv_linear kv{buf, buf}, no_w{nullptr, buf};
    infv_vqf_vision_ln half_ln{buf, nullptr, 1e-5f}, ln{buf, buf, 1e-5f};
    for (int m : known) {
        EXPECT(infv_vqf_set_attention_precision(h, m) == INFV_OK);
        std::memcpy(a0, a, kDummy);
        for (int bad : unknown) {
            EXPECT(infv_vqf_set_attention_precision(h, bad) == INFV_ERR_INVALID);
            EXPECT(std::strstr(infv_ltm_last_error(), "unknown mode") != nullptr);
        }
        EXPECT(std::memcmp(a0, a, kDummy) == 0);        // a refusal changes nothing
        if (m != 0) {                                   // the setting is kept: every other entry point refuses, naming the setter
            EXPECT(infv_vqf_short_attention(h, buf, 64, buf, &kv, &kv, nullptr, buf, nullptr) == INFV_ERR_UNSUPPORTED);
            EXPECT(std::strstr(infv_ltm_last_error(), "infv_vqf_set_attention_precision") != nullptr);
            EXPECT(infv_vqf_vc_embed(h, reinterpret_cast<const infv_vqf_vc_front*>(buf), 0, reinterpret_cast<const int32_t*>(buf), nullptr, nullptr)
                   == INFV_ERR_UNSUPPORTED);
            // with a linear precision set as well, the refusal names that setter, as before; the two settings do not touch each other
            EXPECT(infv_vqf_set_linear_precision(h, 2) == INFV_OK);
            EXPECT(infv_vqf_short_attention(h, buf, 64, buf, &kv, &kv, nullptr, buf, nullptr) == INFV_ERR_UNSUPPORTED);
            EXPECT(std::strstr(infv_ltm_last_error(), "infv_vqf_set_linear_precision") != nullptr);
            EXPECT(infv_vqf_set_linear_precision(h, 0) == INFV_OK);
            EXPECT(std::memcmp(a0, a, kDummy) == 0);    // ... before any workspace change
        }
        // infv_vqf_frame_cross_attention: every refusal comes before a launch or a memory change
        EXPECT(infv_vqf_frame_cross_attention(nullptr, 1, buf, 0, 64, nullptr, buf, &kv, &kv, buf, nullptr) == INFV_ERR_INVALID);
        EXPECT(infv_vqf_frame_cross_attention(h, 1, buf, 0, 64, nullptr, buf, nullptr, &kv, buf, nullptr) == INFV_ERR_INVALID);
        EXPECT(infv_vqf_frame_cross_attention(h, 1, buf, 0, 64, nullptr, buf, &kv, &no_w, buf, nullptr) == INFV_ERR_INVALID);
        EXPECT(infv_vqf_frame_cross_attention(h, -1, buf, 0, 64, nullptr, buf, &kv, &kv, buf, nullptr) == INFV_ERR_INVALID);
        EXPECT(infv_vqf_frame_cross_attention(h, 1, buf, 2, 64, nullptr, buf, &kv, &kv, buf, nullptr) == INFV_ERR_INVALID);
        EXPECT(infv_vqf_frame_cross_attention(h, 1, buf, 9, 64, nullptr, buf, &kv, &kv, buf, nullptr) == INFV_ERR_INVALID);
        EXPECT(infv_vqf_frame_cross_attention(h, 1, nullptr, 0, 64, nullptr, buf, &kv, &kv, buf, nullptr) == INFV_ERR_INVALID);
        EXPECT(infv_vqf_frame_cross_attention(h, 1, buf, 0, 64, nullptr, nullptr, &kv, &kv, buf, nullptr) == INFV_ERR_INVALID);
        EXPECT(infv_vqf_frame_cross_attention(h, 1, buf, 0, 64, nullptr, buf, &kv, &kv, nullptr, nullptr) == INFV_ERR_INVALID);
        EXPECT(infv_vqf_frame_cross_attention(h, 1, buf + 1, 0, 64, nullptr, buf, &kv, &kv, buf, nullptr) == INFV_ERR_INVALID);
        EXPECT(std::strstr(infv_ltm_last_error(), "16-byte") != nullptr);
        EXPECT(infv_vqf_frame_cross_attention(h, 1, buf, 0, 64, nullptr, buf + 2, &kv, &kv, buf, nullptr) == INFV_ERR_INVALID);
        EXPECT(infv_vqf_frame_cross_attention(h, 1, buf, 0, 0, nullptr, buf, &kv, &kv, buf, nullptr) == INFV_ERR_INVALID);
        EXPECT(infv_vqf_frame_cross_attention(h, 1, buf, 0, 64, &half_ln, buf, &kv, &kv, buf, nullptr) == INFV_ERR_INVALID);
        EXPECT(infv_vqf_frame_cross_attention(h, 1, buf, 4, 64, &ln, buf, &kv, &kv, buf, nullptr) == INFV_ERR_UNSUPPORTED);
        if (m == 1) {
            EXPECT(infv_vqf_frame_cross_attention(h, 1, buf, 0, 513, nullptr, buf, &kv, &kv, buf, nullptr) == INFV_ERR_UNSUPPORTED);
            EXPECT(std::strstr(infv_ltm_last_error(), "infv_vqf_set_attention_precision") != nullptr);
        }
        EXPECT(infv_vqf_frame_cross_attention(h, 0, nullptr, 0, 64, nullptr, nullptr, &kv, &kv, nullptr, nullptr) == INFV_OK);   // no frame: nothing to do
        EXPECT(std::memcmp(a0, a, kDummy) == 0);
    }
    // the setter writes the mode field and nothing else: back on the default the storage is all zeros again
    EXPECT(infv_vqf_set_attention_precision(h, 0) == INFV_OK);
    std::memset(a0, 0, kDummy);
    EXPECT(std::memcmp(a0, a, kDummy) == 0);
    std::free(a); std::free(a0);
    std::printf(failures ? "attention precision host check: %d FAILED\n" : "attention precision host check: ok\n", failures);
    return failures ? 1 : 0;
}
