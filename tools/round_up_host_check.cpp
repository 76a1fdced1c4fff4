// Host-side check of round_up_f32 (csrc/philox.h), the function behind chain_batch3_kernel's fp32 search: a stand-alone program
// (its own main, no GPU, not loaded into Python) under the address and undefined-behaviour sanitizers.  Build and run:
//
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -I infinite-video_amd/csrc \
//         tools/round_up_host_check.cpp -o round_up_host_check && ./round_up_host_check
//
// It walks floats c over every exponent from 2^-60 to 1, with the mantissas 0, 1, 0x400000 and 0x7fffff plus seeded ones; for each c
// it takes the doubles u = c, c -+ one double ulp, the midpoint between c and the next float, and the midpoint's two neighbours, and
// checks that
//   (1) round_up_f32(u) is the smallest float >= u;
//   (2) (c' < uf) == ((double)c' < u) for c' the float before c, c itself and the float after c -- the equivalence the kernel's
//       search in fp32 rests on ("(double)c < u  <=>  c < uf").
// The device compile of the same function is covered by tests/test_draw_edges_gpu.py on chain_batch3_kernel.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // (the header's device half uses __umulhi; a plain C++ compiler builds this file too)
#endif
#include "philox.h"

static long failures = 0, checks = 0;
#define EXPECT(cond, c, u) do { ++checks; if (!(cond)) { if (failures < 20) std::fprintf(stderr, "FAILED line %d: %s  (c = %a, u = %a)\n", \
    __LINE__, #cond, (double)(c), (double)(u)); ++failures; } } while (0)

static float float_of(uint32_t bits) { float f; std::memcpy(&f, &bits, sizeof f); return f; }

static void check_uniform(float c, double u) {
    const float uf = infv::round_up_f32(u);
    EXPECT((double)uf >= u, c, u);                                             // (1) a float >= u ...
    EXPECT((double)std::nextafterf(uf, -INFINITY) < u, c, u);                  //     ... and the one below it is not
    const float around[3] = {std::nextafterf(c, -INFINITY), c, std::nextafterf(c, INFINITY)};
    for (float cp : around) EXPECT((cp < uf) == ((double)cp < u), cp, u);      // (2)
}

static void check_float(float c) {
    const double cd = (double)c, next = (double)std::nextafterf(c, INFINITY);
    const double mid = cd + (next - cd) * 0.5;                                 // exact: a float's ulp halves exactly in double
    const double us[6] = {cd, std::nextafter(cd, -INFINITY), std::nextafter(cd, INFINITY),
                          mid, std::nextafter(mid, -INFINITY), std::nextafter(mid, INFINITY)};
    for (double u : us) check_uniform(c, u);
}

int main() {
    uint64_t state = 0x9E3779B97F4A7C15ull;                                    // splitmix64: seeded mantissas
    auto next_random = [&state]() {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    for (int e = -60; e <= 0; ++e) {
        const uint32_t exp_bits = (uint32_t)(e + 127) << 23;
        const uint32_t fixed[4] = {0u, 1u, 0x400000u, 0x7fffffu};
        for (uint32_t m : fixed) check_float(float_of(exp_bits | m));
        for (int i = 0; i < 64; ++i) check_float(float_of(exp_bits | (uint32_t)(next_random() & 0x7fffffu)));
    }
    // the ends of the uniforms' range: 0, the smallest u53 step, the largest uniform
    check_uniform(0.f, 0.0);
    check_uniform(0.f, 1.0 / 9007199254740992.0);
    check_uniform(1.f, 1.0 - 1.0 / 9007199254740992.0);
    EXPECT(infv::round_up_f32(0.0) == 0.f, 0.f, 0.0);
    EXPECT(infv::round_up_f32(1.0 - 1.0 / 9007199254740992.0) == 1.f, 1.f, 1.0);
    EXPECT(infv::round_up_f32(0.5) == 0.5f, 0.5f, 0.5);
    if (failures) std::printf("round_up_f32 host check: %ld of %ld FAILED\n", failures, checks);
    else std::printf("round_up_f32 host check: ok (%ld checks)\n", checks);
    return failures ? 1 : 0;
}
