// The host-side bookkeeping of one LTM memory (a member of infv_ltm_s, ltm_handle.h): which buffers hold the live memory, what the
// last step left behind, and the transitions between those conditions.  Plain C++: no HIP, no device buffers.  The fields are
// private: every entry point changes them through one of the named transitions below and reads them through the getters, so a
// new entry point cannot set half of a block.  DESIGN.md section 5 has the table of who calls what.
#pragma once
#include <cstdint>

namespace infv {

struct Plan;

class MemoryState {
  public:
    // ---- getters ----
    int cur() const { return cur_; }
    int sc() const { return sc_; }
    int parts() const { return parts_; }
    bool has_memory() const { return has_memory_; }
    int lastQ() const { return lastQ_; }
    bool last_fast() const { return last_fast_; }
    bool k_stale() const { return k_stale_; }
    bool carry_scores() const { return carry_scores_; }
    bool scores_ok() const { return scores_ok_; }
    const Plan* last_plan() const { return last_plan_; }
    uint32_t pos() const { return pos_; }
    const float* ctx_sum_for() const { return ctx_sum_for_; }
    int ctx_sum_chunks() const { return ctx_sum_chunks_; }
    int ctx_sum_Q() const { return ctx_sum_Q_; }

    // ---- what the readers ask ----
    // the fused chain's state (B, KV, Sp[sc] + cqbuf, one histogram row) can be handed on under query length Q
    // (infv_ltm_export_chain_state; the scores of infv_ltm_pack_memory, which has refused a handle without a memory before it asks)
    bool chain_exportable(int Q) const { return has_memory_ && last_fast_ && lastQ_ == Q && parts_ == 1; }
    // the one-shot carry of an import_chain_state fits a continuing fused call with query length Q
    bool carry_fits(int Q) const { return carry_scores_ && last_fast_ && lastQ_ == Q; }
    // the handle holds the full scores of the memory's last step (infv_ltm_density, infv_ltm_masses)
    bool last_scores_readable() const { return has_memory_ && scores_ok_; }
    // the accumulator holds the sum of exactly these outputs (infv_ltm_pack_memory)
    bool ctx_sum_holds(const float* ctx, int n_chunks, int Q) const {
        return ctx_sum_for_ == ctx && ctx_sum_chunks_ == n_chunks && ctx_sum_Q_ == Q;
    }

    // ---- transitions ----
    // reset, a latched chain error: no memory any more.  The buffer indices, what the last attend was and the carry stay.
    void forget() {
        has_memory_ = false; parts_ = 0; k_stale_ = false; pos_ = 0; scores_ok_ = false;
        drop_ctx_sum();
    }
    // the update launches of `n` steps have been issued: B / KV flipped n times
    void memory_written(int n) {
        cur_ ^= n & 1;
        has_memory_ = true;
        drop_ctx_sum();
    }
    // K' re-derived from B (infv_ltm_reproject, a dense step)
    void reprojected() { k_stale_ = false; }
    // the attend launches of `n` per-call (or lockstep) steps have been issued: full scores in `scores`, `parts` histogram rows
    void attended(const Plan* plan, int Q, int parts, int n) {
        parts_ = parts;
        lastQ_ = Q;
        last_fast_ = false;
        scores_ok_ = true; last_plan_ = plan;
        pos_ += (uint32_t)n;
    }
    // role S of `n` fused steps has been issued: Sp flipped, scores = Sp[sc] + cq
    void role_s_done(const Plan* plan, int Q, int n) {
        sc_ ^= 1;
        lastQ_ = Q;
        last_fast_ = true;
        scores_ok_ = true; last_plan_ = plan;
        pos_ += (uint32_t)n;
    }
    // the join of a fused call: one float histogram row if any chunk ran, K' left behind, and -- kept_ctx != nullptr -- the output
    // sum the UC kernels kept is that of (kept_ctx, n_chunks, Q)
    void fused_call_joined(bool any_chunk, const float* kept_ctx, int n_chunks, int Q) {
        if (any_chunk) parts_ = 1;
        k_stale_ = true;                 // K' is re-projected from B on demand (per-call path, continuation)
        if (kept_ctx) { ctx_sum_for_ = kept_ctx; ctx_sum_chunks_ = n_chunks; ctx_sum_Q_ = Q; }
    }
    // infv_ltm_import_chain_state: a fused chain's state, as if this handle's last call had been that chain
    void chain_imported(int Q) {
        has_memory_ = true; parts_ = 1; lastQ_ = Q; last_fast_ = true;
        scores_ok_ = true; last_plan_ = nullptr;
        k_stale_ = true;                 // the K' half came from a fast-path handle: re-projected on demand
        carry_scores_ = true;
        drop_ctx_sum();
    }
    // infv_ltm_import_state, in front of its copies: a fresh handle gets a histogram of one row, a memory keeps its stride
    void layer_import_begins() { if (parts_ <= 0) parts_ = 1; }
    // ... and behind them.  The fused chain's scores (Sp) describe the memory this one replaces: nothing may hand them on any more
    // -- neither export_chain_state nor the one-shot carry of an import_chain_state that no call consumed -- and nothing is
    // re-derived, so there are no scores of a last step either.
    void layer_imported() {
        has_memory_ = true;
        last_fast_ = false;
        carry_scores_ = false;
        scores_ok_ = false;
        drop_ctx_sum();
    }
    // the first chunk of a fused call is through: whatever it did with the carry, the carry is spent
    void carry_consumed() { carry_scores_ = false; }
    // `plan` is about to be deleted (infv_ltm_masses then takes the read-out weights of any plan: they depend on num_basis only)
    void plan_erased(const Plan* plan) { if (last_plan_ == plan) last_plan_ = nullptr; }
    void drop_ctx_sum() { ctx_sum_for_ = nullptr; }
    void set_rng_position(uint32_t p) { pos_ = p; }

  private:
    int cur_ = 0;                        // which of B[2] / KV[2] holds the memory
    int sc_ = 0;                         // which of Sp[2] holds the fused chain's bias-free scores
    int parts_ = 0;                      // row count of bin_part per layer, set by the last attend
    bool has_memory_ = false;
    int lastQ_ = 0;                      // query length of the last attend
    bool last_fast_ = false;             // last step ran in the fused chain kernel (scores = Sp + cq)
    bool k_stale_ = false;               // the K' half of KV is out of date (the fast path does not maintain it)
    bool carry_scores_ = false;          // one-shot (import_chain_state): the next consolidate continues from Sp / V' as they are
    bool scores_ok_ = false;             // the handle holds the full scores of the memory's last step (`scores`, or Sp[sc] + cqbuf)
    const Plan* last_plan_ = nullptr;    // plan of the last step (its read-out weights)
    uint32_t pos_ = 0;                   // device rng position = steps since the last forget
    // the (ctx, n_chunks, Q) of the fused call whose outputs the handle's ctx_sum accumulator holds the sum of, until the memory
    // steps again; ctx_sum_for == nullptr: not valid
    const float* ctx_sum_for_ = nullptr; int ctx_sum_chunks_ = 0, ctx_sum_Q_ = 0;
};

}  // namespace infv
