// Host-side check of what infv_ltm_set_grid_plan, infv_ltm_set_mass_trace, infv_ltm_density and infv_ltm_masses refuse before any
// device work, under the address and undefined-behaviour sanitizers: a stand-alone program (its own main, no GPU, not loaded
// into Python).  Build and run (tests/test_density_cpu.py does):
//
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined -I include \
//         tools/density_host_check.cpp infinite-video_amd/csrc/ltm_density.hip -o density_host_check && ./density_host_check
//
// Only ltm_density.hip is linked: the three symbols it takes from ltm_capi.hip (the error text, the latched-error check, the
// launch counter) are stood in for below.  The handle is a real infv_ltm_s with no device memory behind it, so every call made
// here must return before it touches the device -- which is what the header promises of these refusals.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

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
int check_chain_error(infv_ltm_handle) { return INFV_OK; }
}  // namespace infv

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s  [%s]\n", __LINE__, #cond, infv::g_err); ++failures; } } while (0)

// a valid two-segment grid over N boxes: 2 * m points, point i in box i % N, the last point of each segment in none
struct Grid {
    std::vector<int32_t> seg, ptr, box;
    std::vector<float> w, val;
    infv_ltm_grid_plan p;
    Grid(int N, int m) {
        seg = {0, m, 2 * m};
        ptr.push_back(0);
        for (int i = 0; i < 2 * m; ++i) {
            if (i % m != m - 1) { box.push_back(i % N); val.push_back(1.f); }
            ptr.push_back((int32_t)box.size());
            w.push_back(1.f / m);
        }
        sync();
    }
    void sync() {
        p.n_points = (int32_t)w.size(); p.n_segments = (int32_t)seg.size() - 1;
        p.seg_begin = seg.data(); p.pt_weight = w.data(); p.pt_ptr = ptr.data(); p.pt_box = box.data(); p.pt_val = val.data();
    }
};

int main() {
    infv_ltm_s* h = new infv_ltm_s();
    h->N = 64; h->H = 12; h->L = 2; h->maxQ = 32; h->dh = 64; h->d = 768; h->dm = 768; h->P = 32; h->S = 512; h->maxC = 32;
    const int N = h->N;
    float dummy[4];

    // ---- infv_ltm_set_grid_plan ----
    { Grid g(N, 8); EXPECT(infv_ltm_set_grid_plan(nullptr, &g.p) == INFV_ERR_INVALID); }
    EXPECT(infv_ltm_set_grid_plan(h, nullptr) == INFV_ERR_INVALID);
    { Grid g(N, 8); g.p.seg_begin = nullptr; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.p.pt_weight = nullptr; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.p.pt_ptr = nullptr; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.p.pt_box = nullptr; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.p.pt_val = nullptr; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.p.n_points = 4097; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.p.n_points = 1; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.p.n_segments = 0; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.p.n_segments = 17; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.seg[0] = 1; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.seg[2] = 15; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.seg[1] = 15; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }       // a one-point segment
    { Grid g(N, 8); g.seg[1] = 17; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }       // a segment that runs backwards
    { Grid g(N, 8); g.ptr[0] = 1; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.ptr[3] = g.ptr[2] - 1; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.ptr[16] = 1 << 30; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }  // nnz far beyond the tables: not read
    { Grid g(N, 8); g.box[5] = N; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.box[5] = -1; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.w[3] = -1.f; EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.w[3] = __builtin_nanf(""); EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.w[3] = __builtin_inff(); EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.val[2] = __builtin_nanf(""); EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { Grid g(N, 8); g.val[2] = -__builtin_inff(); EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); }
    { h->N = 16384 - 15; Grid g(64, 8); EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_INVALID); h->N = N; }   // row + grid beyond a wave's LDS
    EXPECT(!h->grid.on);

    // ---- infv_ltm_set_mass_trace ----
    EXPECT(infv_ltm_set_mass_trace(nullptr, dummy, 1) == INFV_ERR_INVALID);
    EXPECT(infv_ltm_set_mass_trace(h, dummy, -1) == INFV_ERR_INVALID);
    EXPECT(infv_ltm_set_mass_trace(h, nullptr, 4) == INFV_ERR_INVALID);
    EXPECT(h->mass_trace == nullptr && h->mass_cap == 0);
    h->N = 528; EXPECT(infv_ltm_set_mass_trace(h, dummy, 4) == INFV_ERR_UNSUPPORTED); h->N = N;
    EXPECT(infv_ltm_set_mass_trace(h, dummy, 4) == INFV_OK && h->mass_trace == dummy && h->mass_cap == 4);
    EXPECT(infv_ltm_set_mass_trace(h, dummy, 0) == INFV_OK && h->mass_trace == nullptr && h->mass_cap == 0);
    EXPECT(infv_ltm_set_mass_trace(h, nullptr, 0) == INFV_OK);

    // ---- general-psi plans: refused by all four ----
    {
        infv::Plan* pl = new infv::Plan();
        pl->T = 8; pl->dense.on = true; pl->dense.psi_on = true;
        h->plans[8] = pl;
        Grid g(N, 8);
        EXPECT(infv_ltm_set_grid_plan(h, &g.p) == INFV_ERR_UNSUPPORTED);
        EXPECT(infv_ltm_set_mass_trace(h, dummy, 4) == INFV_ERR_UNSUPPORTED && h->mass_trace == nullptr);
        EXPECT(infv_ltm_density(h, 0, 8, dummy, nullptr) == INFV_ERR_UNSUPPORTED);
        EXPECT(infv_ltm_masses(h, 0, 8, dummy, nullptr) == INFV_ERR_UNSUPPORTED);
        pl->dense.psi_on = false;
    }

    // ---- infv_ltm_density / infv_ltm_masses: arguments and state ----
    EXPECT(infv_ltm_density(nullptr, 0, 8, dummy, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_ltm_density(h, -1, 8, dummy, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_ltm_density(h, 2, 8, dummy, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_ltm_density(h, 0, 8, nullptr, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_ltm_density(h, 0, 0, dummy, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_ltm_density(h, 0, 33, dummy, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_ltm_masses(h, 2, 8, dummy, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_ltm_masses(h, 0, 8, nullptr, nullptr) == INFV_ERR_INVALID);
    EXPECT(infv_ltm_density(h, 0, 8, dummy, nullptr) == INFV_ERR_STATE);                 // no memory
    EXPECT(infv_ltm_masses(h, 0, 8, dummy, nullptr) == INFV_ERR_STATE);
    h->mem.memory_written(1); h->mem.attended(h->plans[8], 8, 24, 1);                    // a step with Q = 8 ...
    h->mem.layer_import_begins(); h->mem.layer_imported();                               // ... then as infv_ltm_import_state leaves it
    EXPECT(h->mem.has_memory() && !h->mem.scores_ok() && h->mem.lastQ() == 8);
    EXPECT(infv_ltm_density(h, 0, 8, dummy, nullptr) == INFV_ERR_STATE);
    EXPECT(infv_ltm_masses(h, 0, 8, dummy, nullptr) == INFV_ERR_STATE);
    h->mem.memory_written(1); h->mem.attended(h->plans[8], 8, 24, 1);                    // another step: its scores are there
    EXPECT(infv_ltm_density(h, 0, 9, dummy, nullptr) == INFV_ERR_STATE);                 // another Q than the last step's
    EXPECT(infv_ltm_masses(h, 0, 9, dummy, nullptr) == INFV_ERR_STATE);
    EXPECT(infv_ltm_density(h, 0, 8, dummy, nullptr) == INFV_ERR_STATE);                 // no grid plan
    EXPECT(std::strstr(infv::g_err, "grid plan") != nullptr);

    delete h;                                                                            // (deletes the plan it holds)
    std::printf(failures ? "density host check: %d FAILED\n" : "density host check: ok\n", failures);
    return failures ? 1 : 0;
}
