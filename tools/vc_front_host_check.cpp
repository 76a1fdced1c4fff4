// Host-side check of the argument validation of infv_vqf_vc_encode_img, infv_vqf_vc_embed and infv_vqf_layernorm_tokens under the
// address and undefined-behaviour sanitizers: a stand-alone program (its own main, no GPU, not loaded into Python).  Build and run:
//
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/vc_front_host_check.cpp infinite-video_amd/csrc/*.hip -o vc_front_host_check && ./vc_front_host_check
//
// A development aid in the style of tools/token_dtype_host_check.cpp: zeroed bytes stand in for the Q-former handle, which works
// only while every refusal exercised here is decided before the handle is written and from its config alone (all zeros: no query
// tokens, no cross layer); formally that is undefined behaviour on the non-trivial struct.  Every call below must be refused --
// null handle, reserved != 0, gamma without beta, the embedding layer beside hidden_in, ids below 0 or at vocab, a text longer than
// the position table, a negative text_len, and through the streams form cu[0] != 0, a decreasing cu or fcu, frame_src outside [0, F),
// a stream whose chunk count differs from its block's, reserved != 0 -- and none may touch the handle, the tables (their pointers are never dereferenced) or
// the device.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "infv_ltm.h"
#include "infv_vqf.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #cond, infv_ltm_last_error()); ++failures; } } while (0)
static bool said(const char* what) { return std::strstr(infv_ltm_last_error(), what) != nullptr; }

int main() {
    const size_t kDummy = 1u << 20;                     // far larger than the handle
    void* a = std::calloc(1, kDummy);
    void* a0 = std::calloc(1, kDummy);
    if (!a || !a0) return 2;
    infv_vqf_handle h = static_cast<infv_vqf_handle>(a);
    const float* tab = reinterpret_cast<const float*>(0x1000);          // never dereferenced: every call is refused first
    const int vocab = 50, max_pos = 32;
    int32_t* ids = static_cast<int32_t*>(std::malloc(5 * sizeof(int32_t)));   // exactly sum(text_len) entries: a read past them is caught
    int32_t* text_len = static_cast<int32_t*>(std::malloc(2 * sizeof(int32_t)));
    if (!ids || !text_len) return 2;
    const int32_t good[5] = {0, 49, 7, 7, 23};
    std::memcpy(ids, good, sizeof(good));
    text_len[0] = 2; text_len[1] = 3;
    float* out = reinterpret_cast<float*>(0x1000);

    infv_vqf_vc_front f{};
    f.emb.word = tab; f.emb.pos = tab; f.emb.ln.gamma = tab; f.emb.ln.beta = tab; f.emb.query_tokens = tab;
    f.emb.vocab = vocab; f.emb.max_pos = max_pos; f.input_ids = ids;

    // ---- infv_vqf_vc_embed
    EXPECT(infv_vqf_vc_embed(nullptr, &f, 2, text_len, out, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_vc_embed(h, nullptr, 2, text_len, out, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_vc_embed(h, &f, 2, nullptr, out, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_vc_embed(h, &f, -1, text_len, out, nullptr) == INFV_ERR_INVALID);
    { infv_vqf_vc_front g = f; g.reserved = 1; EXPECT(infv_vqf_vc_embed(h, &g, 2, text_len, out, nullptr) == INFV_ERR_INVALID && said("reserved")); }
    { infv_vqf_vc_front g = f; g.emb.word = nullptr; EXPECT(infv_vqf_vc_embed(h, &g, 2, text_len, out, nullptr) == INFV_ERR_INVALID); }
    { infv_vqf_vc_front g = f; g.emb.pos = nullptr; EXPECT(infv_vqf_vc_embed(h, &g, 2, text_len, out, nullptr) == INFV_ERR_INVALID); }
    { infv_vqf_vc_front g = f; g.input_ids = nullptr; EXPECT(infv_vqf_vc_embed(h, &g, 2, text_len, out, nullptr) == INFV_ERR_INVALID && said("input_ids")); }
    const int32_t bad_ids[] = {-1, vocab, -2147483647 - 1, 2147483647};
    for (int32_t bad : bad_ids)
        for (int at = 0; at < 5; ++at) {
            std::memcpy(ids, good, sizeof(good));
            ids[at] = bad;
            EXPECT(infv_vqf_vc_embed(h, &f, 2, text_len, out, nullptr) == INFV_ERR_INVALID);
            EXPECT(said(at < 2 ? "video 0" : "video 1") && said("input id"));
        }
    std::memcpy(ids, good, sizeof(good));
    { infv_vqf_vc_front g = f; g.emb.max_pos = 2; EXPECT(infv_vqf_vc_embed(h, &g, 2, text_len, out, nullptr) == INFV_ERR_INVALID && said("video 1 has 3 text tokens")); }
    text_len[1] = -3;
    EXPECT(infv_vqf_vc_embed(h, &f, 2, text_len, out, nullptr) == INFV_ERR_INVALID && said("negative"));
    text_len[1] = 3;

    // ---- infv_vqf_layernorm_tokens
    EXPECT(infv_vqf_layernorm_tokens(tab, 2, 4, 64, tab, tab, 1e-12f, out, nullptr) == INFV_ERR_INVALID && said("unknown"));
    EXPECT(infv_vqf_layernorm_tokens(nullptr, 0, 4, 64, tab, tab, 1e-12f, out, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_layernorm_tokens(tab, 0, 4, 64, tab, nullptr, 1e-12f, out, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_layernorm_tokens(tab, 0, -1, 64, tab, tab, 1e-12f, out, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_layernorm_tokens(tab, 0, 4, 96, tab, tab, 1e-12f, out, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_vqf_layernorm_tokens(tab, 0, 4, 8192, tab, tab, 1e-12f, out, nullptr) == INFV_ERR_UNSUPPORTED);
    EXPECT(infv_vqf_layernorm_tokens(reinterpret_cast<const char*>(tab) + 4, 3, 4, 64, tab, tab, 1e-12f, out, nullptr) == INFV_ERR_INVALID && said("16-byte"));

    // ---- infv_vqf_vc_encode_img (two videos of one chunk; one layer without cross-attention; videos: frame_src NULL)
    infv_vqf_vc_layer layer{};
    infv_vqf_vc_weights w{};
    w.n_layers = 1; w.layers = &layer;
    const int32_t cu[3] = {0, 1, 2};
    auto img = [&](infv_vqf_handle hh, const infv_vqf_vc_front* fr, const float* hidden_in, int code, const void* frames, const int32_t* src) {
        return infv_vqf_vc_encode_img(hh, nullptr, 2, cu, frames, code, 0, nullptr, src, 16, &w, fr, hidden_in, text_len, nullptr, 1, nullptr,
                                      nullptr, nullptr, nullptr);
    };
    EXPECT(img(nullptr, &f, nullptr, 0, tab, nullptr) == INFV_ERR_INVALID);
    EXPECT(img(h, &f, nullptr, -1, tab, nullptr) == INFV_ERR_INVALID);
    EXPECT(img(h, &f, nullptr, 2, tab, nullptr) == INFV_ERR_INVALID && said("unknown"));
    { infv_vqf_vc_front g = f; g.reserved = -5; EXPECT(img(h, &g, nullptr, 0, tab, nullptr) == INFV_ERR_INVALID && said("reserved")); }
    { infv_vqf_vc_front g = f; g.vision_ln.gamma = tab; EXPECT(img(h, &g, nullptr, 0, tab, nullptr) == INFV_ERR_INVALID && said("gamma without")); }
    { infv_vqf_vc_front g = f; g.vision_ln.gamma = tab; g.vision_ln.beta = tab;
      EXPECT(img(h, &g, nullptr, 0, reinterpret_cast<const char*>(tab) + 8, nullptr) == INFV_ERR_INVALID && said("16-byte")); }
    EXPECT(img(h, &f, tab, 0, tab, nullptr) == INFV_ERR_INVALID && said("both given"));
    ids[4] = vocab;
    EXPECT(img(h, &f, nullptr, 0, tab, nullptr) == INFV_ERR_INVALID && said("video 1") && said("position 2"));
    ids[4] = good[4];
    { infv_vqf_vc_front g = f; g.emb.max_pos = 1; EXPECT(img(h, &g, nullptr, 0, tab, nullptr) == INFV_ERR_INVALID && said("position table")); }
    text_len[0] = -1;
    EXPECT(img(h, &f, nullptr, 0, tab, nullptr) == INFV_ERR_INVALID && said("negative"));
    text_len[0] = 2;
    const int32_t src[2] = {0, 0};
    EXPECT(img(h, &f, nullptr, 0, tab, src) == INFV_ERR_INVALID);                       // frame_src without fcu

    // ---- the table refusals of the streams form (three streams over two blocks of 1 and 2 chunks)
    const int32_t scu[4] = {0, 1, 3, 4}, sfcu[3] = {0, 1, 3}, ssrc[3] = {0, 1, 0}, stl[3] = {0, 0, 0};
    auto streams = [&](const int32_t* cu_, const int32_t* fcu_, const int32_t* src_, const infv_vqf_vc_front* fr) {
        return infv_vqf_vc_encode_img(h, nullptr, 3, cu_, tab, 0, 2, fcu_, src_, 16, &w, fr, tab, stl, nullptr, 1, nullptr, nullptr, nullptr,
                                      nullptr);
    };
    { const int32_t c[4] = {1, 1, 3, 4}; EXPECT(streams(c, sfcu, ssrc, nullptr) == INFV_ERR_INVALID && said("cu[0] = 1")); }
    { const int32_t c[4] = {0, 3, 1, 4}; EXPECT(streams(c, sfcu, ssrc, nullptr) == INFV_ERR_INVALID && said("cu is not non-decreasing")); }
    { const int32_t c[3] = {1, 1, 3}; EXPECT(streams(scu, c, ssrc, nullptr) == INFV_ERR_INVALID && said("fcu[0] = 1")); }
    { const int32_t c[3] = {0, 3, 1}; EXPECT(streams(scu, c, ssrc, nullptr) == INFV_ERR_INVALID && said("fcu is not non-decreasing")); }
    { const int32_t c[3] = {0, 2, 0}; EXPECT(streams(scu, sfcu, c, nullptr) == INFV_ERR_INVALID && said("frame_src[1] = 2 outside [0, 2)")); }
    { const int32_t c[3] = {0, -1, 0}; EXPECT(streams(scu, sfcu, c, nullptr) == INFV_ERR_INVALID && said("frame_src[1] = -1 outside")); }
    { const int32_t c[3] = {0, 0, 1}; EXPECT(streams(scu, sfcu, c, nullptr) == INFV_ERR_INVALID && said("stream 1 has 2 chunks, its block 0 has 1")); }
    { infv_vqf_vc_front g{}; g.reserved = 1; EXPECT(streams(scu, sfcu, ssrc, &g) == INFV_ERR_INVALID && said("reserved")); }

    EXPECT(std::memcmp(a0, a, kDummy) == 0);                                            // no refusal wrote to the handle
    std::free(a); std::free(a0); std::free(ids); std::free(text_len);
    std::printf(failures ? "vc front host check: %d FAILED\n" : "vc front host check: ok\n", failures);
    return failures ? 1 : 0;
}
