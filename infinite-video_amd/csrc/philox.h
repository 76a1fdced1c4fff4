// Counter-based generator of the Gibbs uniforms: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11), the generator torch's device RNG is built on.  The reference samples the sticky memory with
// torch.rand(nb_samples) on its device (long_term_attention_gibbs.py:204-206); its second nb_samples uniforms (:206, the
// position inside the drawn bin) are degenerate and never generated here.
//
// The stream (include/infv_ltm.h, DESIGN.md "Device RNG"; mirrored by infinite-video_amd/philox.py):
//   key = (seed & 0xffffffff, seed >> 32)
//   ctr = (s >> 1, layer, pos, stream_id)        s: sample slot in [0, S), pos: chunk index within the document
//   one block (w0, w1, w2, w3) serves two slots:  u[s even] = u53(w0, w1),  u[s odd] = u53(w2, w3)
//   u53(a, b) = ((a >> 5) * 2^26 + (b >> 6)) * 2^-53      a double in [0, 1), numpy's construction
// Plain C++ for the host and the device; no state, no memory traffic.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define INFV_HD __host__ __device__
#else
#define INFV_HD
#endif

namespace infv {

struct Philox4 { uint32_t w[4]; };

INFV_HD inline uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

INFV_HD inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;      // multipliers
    constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;      // Weyl constants of the key schedule
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = philox_mulhi(kM0, c0), lo0 = kM0 * c0;
        const uint32_t hi1 = philox_mulhi(kM1, c2), lo1 = kM1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += kW0; k1 += kW1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

INFV_HD inline double philox_u53(uint32_t a, uint32_t b) {
    return (double)(((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// What a kernel needs to generate a step's uniforms: by value in the launch arguments.  `pos` is the position of the step
// the launch draws for (a persistent launch adds its step index), so a captured graph replays the position it was captured with.
struct RngView {
    uint32_t on, key0, key1, stream_id, pos;
};

INFV_HD inline RngView make_rng_view(uint64_t seed, uint32_t stream_id, uint32_t pos) {
    return RngView{1u, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), stream_id, pos};
}

// the block of slots (2 * pair, 2 * pair + 1)
INFV_HD inline Philox4 gibbs_block(const RngView& g, uint32_t layer, uint32_t pos, uint32_t pair) {
    return philox4x32_10(pair, layer, pos, g.stream_id, g.key0, g.key1);
}

// the uniform of slot s (computes the whole block: callers that hold both slots of a pair use gibbs_block)
INFV_HD inline double gibbs_uniform(const RngView& g, uint32_t layer, uint32_t pos, uint32_t s) {
    const Philox4 b = gibbs_block(g, layer, pos, s >> 1);
    return (s & 1u) ? philox_u53(b.w[2], b.w[3]) : philox_u53(b.w[0], b.w[1]);
}

// uf = the smallest float >= u:  (double)c < u  <=>  c < uf  for every float c (chain_batch3_kernel searches in fp32)
INFV_HD inline float round_up_f32(double x) {
    float f = (float)x;
    if ((double)f < x) {
        union { float f; uint32_t i; } v;
        v.f = f;
        v.i += 1u;
        f = v.f;
    }
    return f;
}

}  // namespace infv
