// Host-side check of the token-dtype validation of infv_ltm_set_token_dtype / infv_vqf_set_token_dtype under the address and
// undefined-behaviour sanitizers: a stand-alone program (its own main, no GPU, not loaded into Python).  Build and run:
//
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/token_dtype_host_check.cpp infinite-video_amd/csrc/*.hip -o token_dtype_host_check && ./token_dtype_host_check
//
// A development aid, tied to the handles' internals: it stands zeroed bytes in for both handle structs, which works only while
// the setters check the handle for null alone and write nothing but the dtype field (whose fp32 code is 0); formally that is
// undefined behaviour on these non-trivial structs.  If a handle gains a validity check, give this program real handles.
// Null handles are refused whatever the code; on a dummy handle (zeroed storage standing in for the handle: the setters touch
// nothing but the dtype field) the known codes 0, 1, 3 and 4 (fp8 e4m3) are taken and every other code is refused and leaves the setting alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "infv_ltm.h"
#include "infv_vqf.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    const int known[] = {INFV_TOKENS_F32, INFV_TOKENS_BF16, INFV_TOKENS_F16, INFV_TOKENS_F8E4M3};
    const int unknown[] = {2, -1, 5, 7, 16, 255, -2147483647 - 1, 2147483647};
    for (int c : known) { EXPECT(infv_ltm_set_token_dtype(nullptr, c) == INFV_ERR_INVALID); EXPECT(infv_vqf_set_token_dtype(nullptr, c) == INFV_ERR_INVALID); }
    for (int c : unknown) { EXPECT(infv_ltm_set_token_dtype(nullptr, c) == INFV_ERR_INVALID); EXPECT(infv_vqf_set_token_dtype(nullptr, c) == INFV_ERR_INVALID); }
    EXPECT(std::strstr(infv_ltm_last_error(), "null") != nullptr);
    const size_t kDummy = 1u << 20;                     // far larger than either handle
    void* a = std::calloc(1, kDummy);
    void* b = std::calloc(1, kDummy);
    void* a0 = std::malloc(kDummy);
    void* b0 = std::malloc(kDummy);
    if (!a || !b || !a0 || !b0) return 2;
    infv_ltm_handle hl = static_cast<infv_ltm_handle>(a);
    infv_vqf_handle hv = static_cast<infv_vqf_handle>(b);
    for (int c : known) {
        EXPECT(infv_ltm_set_token_dtype(hl, c) == INFV_OK);
        EXPECT(infv_vqf_set_token_dtype(hv, c) == INFV_OK);
        std::memcpy(a0, a, kDummy); std::memcpy(b0, b, kDummy);
        for (int bad : unknown) {
            EXPECT(infv_ltm_set_token_dtype(hl, bad) == INFV_ERR_INVALID);
            EXPECT(std::strstr(infv_ltm_last_error(), "unknown") != nullptr);
            EXPECT(infv_vqf_set_token_dtype(hv, bad) == INFV_ERR_INVALID);
            EXPECT(std::strstr(infv_ltm_last_error(), "unknown") != nullptr);
        }
        EXPECT(std::memcmp(a0, a, kDummy) == 0 && std::memcmp(b0, b, kDummy) == 0);      // a refusal changes nothing
    }
    // the setters write the dtype field and nothing else: back on fp32 the storage is all zeros again
    EXPECT(infv_ltm_set_token_dtype(hl, INFV_TOKENS_F32) == INFV_OK && infv_vqf_set_token_dtype(hv, INFV_TOKENS_F32) == INFV_OK);
    std::memset(a0, 0, kDummy);
    EXPECT(std::memcmp(a0, a, kDummy) == 0 && std::memcmp(a0, b, kDummy) == 0);
    // code 4 wants 16-byte aligned tokens: infv_vqf_token_pass refuses a pointer 1, 2, 4 or 8 bytes off before any launch, and a lo plane
    alignas(16) static unsigned char tok[64];
    alignas(16) static unsigned char plane[64];
    for (int off : {1, 2, 4, 8}) {
        EXPECT(infv_vqf_token_pass(tok + off, INFV_TOKENS_F8E4M3, 1, 64, 64, 4, plane, nullptr, plane, nullptr, nullptr, nullptr) == INFV_ERR_INVALID);
        EXPECT(std::strstr(infv_ltm_last_error(), "16-byte") != nullptr);
    }
    EXPECT(infv_vqf_token_pass(tok, INFV_TOKENS_F8E4M3, 1, 64, 64, 4, plane, plane, plane, nullptr, nullptr, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_token_pass(tok, 5, 1, 64, 64, 4, plane, nullptr, plane, nullptr, nullptr, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_layernorm_tokens(tok, INFV_TOKENS_F8E4M3, 1, 64, nullptr, nullptr, 1e-12f, nullptr, nullptr) == INFV_ERR_UNSUPPORTED);
    std::free(a); std::free(b); std::free(a0); std::free(b0);
    std::printf(failures ? "token dtype host check: %d FAILED\n" : "token dtype host check: ok\n", failures);
    return failures ? 1 : 0;
}
