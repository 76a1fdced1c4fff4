// Host-side check of the LTM memory's bookkeeping (infinite-video_amd/csrc/ltm_memory_state.h) under the address and
// undefined-behaviour sanitizers: a stand-alone program (its own main, no GPU, not loaded into Python).  The header needs no HIP,
// so a plain C++ line builds it (tests/test_memory_state_cpu.py does):
//
//   hipcc -O1 -g -std=c++17 -x c++ -Xarch_host -fsanitize=address,undefined tools/memory_state_host_check.cpp -o memory_state_host_check \
//         && ./memory_state_host_check
//
// Every expectation below is written out: the fields are the assignments the entry points made by hand before the transitions
// had names (ltm_capi.hip, ltm_consolidate.hip), the pair table is worked out from those by hand.  Nothing is expected by
// calling the struct's own code a second time.
#include <cstdint>
#include <cstdio>

#include "../infinite-video_amd/csrc/ltm_memory_state.h"

namespace infv { struct Plan { int T; }; }
using infv::MemoryState;
using infv::Plan;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static Plan P1{8}, P2{16};
static float CTX[1], CTX2[1];

// every field, in the order: cur sc parts | has_memory lastQ last_fast k_stale carry_scores scores_ok | last_plan pos | ctx sum triple
struct Fields {
    int cur, sc, parts; bool has_memory; int lastQ; bool last_fast, k_stale, carry_scores, scores_ok;
    const Plan* last_plan; uint32_t pos; const float* ctx_sum_for; int ctx_sum_chunks, ctx_sum_Q;
};

static void is(const MemoryState& m, const Fields& f, int line) {
    const bool ok = m.cur() == f.cur && m.sc() == f.sc && m.parts() == f.parts && m.has_memory() == f.has_memory && m.lastQ() == f.lastQ &&
                    m.last_fast() == f.last_fast && m.k_stale() == f.k_stale && m.carry_scores() == f.carry_scores &&
                    m.scores_ok() == f.scores_ok && m.last_plan() == f.last_plan && m.pos() == f.pos &&
                    m.ctx_sum_for() == f.ctx_sum_for && m.ctx_sum_chunks() == f.ctx_sum_chunks && m.ctx_sum_Q() == f.ctx_sum_Q;
    if (ok) return;
    std::fprintf(stderr, "FAILED line %d: cur %d sc %d parts %d | mem %d lastQ %d fast %d stale %d carry %d scores %d | plan %s pos %u | sum %s %d %d\n",
                 line, m.cur(), m.sc(), m.parts(), (int)m.has_memory(), m.lastQ(), (int)m.last_fast(), (int)m.k_stale(), (int)m.carry_scores(),
                 (int)m.scores_ok(), m.last_plan() == &P1 ? "P1" : m.last_plan() == &P2 ? "P2" : m.last_plan() ? "?" : "null", m.pos(),
                 m.ctx_sum_for() == CTX ? "CTX" : m.ctx_sum_for() == CTX2 ? "CTX2" : m.ctx_sum_for() ? "?" : "null", m.ctx_sum_chunks(), m.ctx_sum_Q());
    ++failures;
}
#define IS(m, ...) is(m, Fields{__VA_ARGS__}, __LINE__)

// ---- the six kinds of operation, as the entry points string the transitions together (Q = 8 throughout) ----
// infv_ltm_step: update launch, attend launch
static void per_call_step(MemoryState& m) { m.memory_written(1); m.attended(&P1, 8, 24, 1); }
// infv_ltm_consolidate on the fused path: on a fresh memory the document's first chunk on its own (role S, UC), then `batches`
// sub-batches of two chunks (role S of both, one UC launch), then the join, which keeps the output sum
static void fused_call(MemoryState& m, int batches) {
    const int n_chunks = (m.has_memory() ? 0 : 1) + 2 * batches;
    m.drop_ctx_sum();
    if (!m.has_memory()) { m.role_s_done(&P1, 8, 1); m.memory_written(1); }
    m.carry_consumed();
    for (int b = 0; b < batches; ++b) { m.role_s_done(&P1, 8, 2); m.memory_written(1); }
    m.fused_call_joined(true, CTX, n_chunks, 8);
}
// a lockstep videos call in which this handle's video has three chunks: the host state follows the launches of all of them
static void videos_step(MemoryState& m) { m.memory_written(3); m.attended(&P1, 8, 24, 3); }
static void chain_import(MemoryState& m) { m.chain_imported(8); }
static void layer_import(MemoryState& m) { m.layer_import_begins(); m.layer_imported(); }
static void forget(MemoryState& m) { m.forget(); }

int main() {
    const MemoryState fresh;
    IS(fresh, 0, 0, 0, false, 0, false, false, false, false, nullptr, 0, nullptr, 0, 0);
    // a fused call of 1 + 2 + 2 chunks on a fresh handle: three role-S launches, three UC launches
    MemoryState fused;
    fused_call(fused, 2);
    IS(fused, 1, 1, 1, true, 8, true, true, false, true, &P1, 5, CTX, 5, 8);
    // a chain import on a fresh handle
    MemoryState chain;
    chain.chain_imported(8);
    IS(chain, 0, 0, 1, true, 8, true, true, true, true, nullptr, 0, nullptr, 0, 0);

    // ---- each transition from a fresh state ----
    { MemoryState m = fresh; m.forget();                              IS(m, 0, 0, 0, false, 0, false, false, false, false, nullptr, 0, nullptr, 0, 0); }
    { MemoryState m = fresh; m.memory_written(3);                     IS(m, 1, 0, 0, true, 0, false, false, false, false, nullptr, 0, nullptr, 0, 0); }
    { MemoryState m = fresh; m.reprojected();                         IS(m, 0, 0, 0, false, 0, false, false, false, false, nullptr, 0, nullptr, 0, 0); }
    { MemoryState m = fresh; m.attended(&P2, 12, 24, 2);              IS(m, 0, 0, 24, false, 12, false, false, false, true, &P2, 2, nullptr, 0, 0); }
    { MemoryState m = fresh; m.role_s_done(&P2, 12, 4);               IS(m, 0, 1, 0, false, 12, true, false, false, true, &P2, 4, nullptr, 0, 0); }
    { MemoryState m = fresh; m.fused_call_joined(true, CTX2, 7, 12);  IS(m, 0, 0, 1, false, 0, false, true, false, false, nullptr, 0, CTX2, 7, 12); }
    { MemoryState m = fresh; m.fused_call_joined(false, nullptr, 7, 12); IS(m, 0, 0, 0, false, 0, false, true, false, false, nullptr, 0, nullptr, 0, 0); }
    { MemoryState m = fresh; m.chain_imported(12);                    IS(m, 0, 0, 1, true, 12, true, true, true, true, nullptr, 0, nullptr, 0, 0); }
    { MemoryState m = fresh; m.layer_import_begins();                 IS(m, 0, 0, 1, false, 0, false, false, false, false, nullptr, 0, nullptr, 0, 0); }
    { MemoryState m = fresh; m.layer_imported();                      IS(m, 0, 0, 0, true, 0, false, false, false, false, nullptr, 0, nullptr, 0, 0); }
    { MemoryState m = fresh; m.carry_consumed();                      IS(m, 0, 0, 0, false, 0, false, false, false, false, nullptr, 0, nullptr, 0, 0); }
    { MemoryState m = fresh; m.plan_erased(&P1);                      IS(m, 0, 0, 0, false, 0, false, false, false, false, nullptr, 0, nullptr, 0, 0); }
    { MemoryState m = fresh; m.drop_ctx_sum();                        IS(m, 0, 0, 0, false, 0, false, false, false, false, nullptr, 0, nullptr, 0, 0); }
    { MemoryState m = fresh; m.set_rng_position(77);                  IS(m, 0, 0, 0, false, 0, false, false, false, false, nullptr, 77, nullptr, 0, 0); }

    // ---- each transition from the state a fused call leaves ----
    // a forget leaves lastQ, last_fast and last_plan (and the buffer indices) as they were
    { MemoryState m = fused; m.forget();                              IS(m, 1, 1, 0, false, 8, true, false, false, false, &P1, 0, nullptr, 5, 8);
      EXPECT(m.lastQ() == 8 && m.last_fast() && m.last_plan() == &P1); }
    { MemoryState m = fused; m.memory_written(3);                     IS(m, 0, 1, 1, true, 8, true, true, false, true, &P1, 5, nullptr, 5, 8); }
    { MemoryState m = fused; m.memory_written(2);                     IS(m, 1, 1, 1, true, 8, true, true, false, true, &P1, 5, nullptr, 5, 8); }
    { MemoryState m = fused; m.reprojected();                         IS(m, 1, 1, 1, true, 8, true, false, false, true, &P1, 5, CTX, 5, 8); }
    { MemoryState m = fused; m.attended(&P2, 12, 24, 2);              IS(m, 1, 1, 24, true, 12, false, true, false, true, &P2, 7, CTX, 5, 8);
      m.layer_import_begins();                                        IS(m, 1, 1, 24, true, 12, false, true, false, true, &P2, 7, CTX, 5, 8); }   // a memory keeps its stride
    { MemoryState m = fused; m.role_s_done(&P2, 12, 4);               IS(m, 1, 0, 1, true, 12, true, true, false, true, &P2, 9, CTX, 5, 8); }
    { MemoryState m = fused; m.fused_call_joined(true, CTX2, 7, 12);  IS(m, 1, 1, 1, true, 8, true, true, false, true, &P1, 5, CTX2, 7, 12); }
    { MemoryState m = fused; m.fused_call_joined(false, nullptr, 7, 12); IS(m, 1, 1, 1, true, 8, true, true, false, true, &P1, 5, CTX, 5, 8); }
    { MemoryState m = fused; m.chain_imported(12);                    IS(m, 1, 1, 1, true, 12, true, true, true, true, nullptr, 5, nullptr, 5, 8); }
    { MemoryState m = fused; m.layer_import_begins();                 IS(m, 1, 1, 1, true, 8, true, true, false, true, &P1, 5, CTX, 5, 8); }
    { MemoryState m = fused; m.layer_imported();                      IS(m, 1, 1, 1, true, 8, false, true, false, false, &P1, 5, nullptr, 5, 8); }
    { MemoryState m = fused; m.carry_consumed();                      IS(m, 1, 1, 1, true, 8, true, true, false, true, &P1, 5, CTX, 5, 8); }
    { MemoryState m = fused; m.plan_erased(&P2);                      IS(m, 1, 1, 1, true, 8, true, true, false, true, &P1, 5, CTX, 5, 8);
      m.plan_erased(&P1);                                             IS(m, 1, 1, 1, true, 8, true, true, false, true, nullptr, 5, CTX, 5, 8); }
    { MemoryState m = fused; m.drop_ctx_sum();                        IS(m, 1, 1, 1, true, 8, true, true, false, true, &P1, 5, nullptr, 5, 8); }
    { MemoryState m = fused; m.set_rng_position(77);                  IS(m, 1, 1, 1, true, 8, true, true, false, true, &P1, 77, CTX, 5, 8); }

    // ---- the carry: spent by a fused call's first chunk; cleared by a layer import, after which nothing hands the scores on ----
    { MemoryState m = chain; m.carry_consumed();                      IS(m, 0, 0, 1, true, 8, true, true, false, true, nullptr, 0, nullptr, 0, 0); }
    {
        MemoryState m = chain;
        EXPECT(m.chain_exportable(8) && m.carry_fits(8) && m.last_scores_readable());
        EXPECT(!m.chain_exportable(9) && !m.carry_fits(9));
        layer_import(m);
        IS(m, 0, 0, 1, true, 8, false, true, false, false, nullptr, 0, nullptr, 0, 0);
        EXPECT(!m.chain_exportable(8) && !m.carry_fits(8) && !m.last_scores_readable());
    }
    // the kept sum answers for exactly its (ctx, n_chunks, Q)
    EXPECT(fused.ctx_sum_holds(CTX, 5, 8) && !fused.ctx_sum_holds(CTX2, 5, 8) && !fused.ctx_sum_holds(CTX, 4, 8) && !fused.ctx_sum_holds(CTX, 5, 9));
    EXPECT(!fresh.ctx_sum_holds(CTX, 0, 0));

    // ---- the 36 ordered pairs, each from a fresh state ----
    // After the pair: chain state exportable for Q 8 | carried scores fit Q 8 | last scores readable | pos = steps since the last
    // forget (the imports add none) | cur = parity of the memory writes (a per-call step 1, the lockstep call 3, a fused call one
    // per UC launch: 2 on a fresh memory, 1 on an existing one; a forget does not flip back).  One pair stands out: a forget
    // behind a chain import leaves the carry and last_fast standing, so "the carry fits" still holds -- and is never asked,
    // because consolidate_first_chunk looks at has_memory first and spends the carry at its end.
    void (*const op[6])(MemoryState&) = {per_call_step, [](MemoryState& m) { fused_call(m, 1); }, videos_step, chain_import, layer_import, forget};
    const char* const name[6] = {"step", "fused", "videos", "chain import", "layer import", "forget"};
    struct After { bool exportable, carry, readable; uint32_t pos; int cur; };
    const After want[6][6] = {
        //            step                  fused                 videos                chain import          layer import           forget
        /* step   */ {{false, false, true, 2, 0}, {true, false, true, 3, 0}, {false, false, true, 4, 0}, {true, true, true, 1, 1}, {false, false, false, 1, 1}, {false, false, false, 0, 1}},
        /* fused  */ {{false, false, true, 4, 1}, {true, false, true, 5, 1}, {false, false, true, 6, 1}, {true, true, true, 3, 0}, {false, false, false, 3, 0}, {false, false, false, 0, 0}},
        /* videos */ {{false, false, true, 4, 0}, {true, false, true, 5, 0}, {false, false, true, 6, 0}, {true, true, true, 3, 1}, {false, false, false, 3, 1}, {false, false, false, 0, 1}},
        /* chain  */ {{false, false, true, 1, 1}, {true, false, true, 2, 1}, {false, false, true, 3, 1}, {true, true, true, 0, 0}, {false, false, false, 0, 0}, {false, true, false, 0, 0}},
        /* layer  */ {{false, false, true, 1, 1}, {true, false, true, 2, 1}, {false, false, true, 3, 1}, {true, true, true, 0, 0}, {false, false, false, 0, 0}, {false, false, false, 0, 0}},
        /* forget */ {{false, false, true, 1, 1}, {true, false, true, 3, 0}, {false, false, true, 3, 1}, {true, true, true, 0, 0}, {false, false, false, 0, 0}, {false, false, false, 0, 0}},
    };
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            MemoryState m;
            op[a](m);
            op[b](m);
            const After& w = want[a][b];
            const bool ok = m.chain_exportable(8) == w.exportable && m.carry_fits(8) == w.carry && m.last_scores_readable() == w.readable &&
                            m.pos() == w.pos && m.cur() == w.cur && !m.chain_exportable(9) && !m.carry_fits(9);
            if (!ok) {
                std::fprintf(stderr, "FAILED pair %s -> %s: exportable %d carry %d readable %d pos %u cur %d\n", name[a], name[b],
                             (int)m.chain_exportable(8), (int)m.carry_fits(8), (int)m.last_scores_readable(), m.pos(), m.cur());
                ++failures;
            }
        }

    std::printf(failures ? "memory state host check: %d FAILED\n" : "memory state host check: ok\n", failures);
    return failures ? 1 : 0;
}
