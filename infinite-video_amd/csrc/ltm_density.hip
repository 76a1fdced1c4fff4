// Read-outs of the memory's attention density (include/infv_ltm.h: infv_ltm_density, infv_ltm_masses, infv_ltm_set_mass_trace,
// infv_ltm_set_videos_mass_trace).
//
// The reference evaluates the density of the last step on a 768-point grid on every forward and pickles it
// (long_term_attention_gibbs.py:320-343):
//     s(t) = sum_n psi_n(t) S[n];  e = exp(s);  dens = e / trapz(e over the point's segment);  alphas = dens / sum dens
// (here with the segment's maximum of s subtracted before exp: the same dens, in range for any scores)
// and the read-out itself weighs basis function n with  alpha[n] = w_n e^{S_n} / (sum_m w_m e^{S_m} + w_out)  (the `integral`
// of expected_value, :282).  Three kernels, none on a default path:
//     density_grid_kernel   one wave per (h, q) score row: the row goes to LDS once, s(t) is gathered through the grid plan's
//                           CSR in fp32 in CSR order, max / exp / per-segment trapezoid sums / grand sum are wave reductions
//     box_mass_kernel       mass[n] = mean over the H*Q rows of alpha[row][n], from full score rows (the per-chunk stages and
//                           the last-step call) or from the alpha rows the fused chain leaves in its ring -- two loaders in
//                           front of ONE reduction
//     box_mass_videos_kernel  that reduction over the score rows of every video a lockstep step just advanced, written at the
//                           packed chunk index (infv_ltm_set_videos_mass_trace)
// exp is expf (1 ulp), never the fast form: the outputs are compared with a float64 restatement (density.py) at a few ulp.
// Sums over points and over rows run in float64, so their order does not show in the fp32 result.
#include "ltm_device.h"

namespace infv {

// ------------------------------------------------------------------------------------------------------
// alphas[q][h][m] of one layer.  Block = kDgWaves waves, wave = row r = h * Q + q.  LDS per wave: the score row [N] and
// e[m] [M].  A point in no box (t = 1.0 of the reference grid) has s = 0: the key-bias term of the scores is what places
// it relative to the rest, hence cq (the bias term of the fused chain's bias-free scores, or nullptr).
// ------------------------------------------------------------------------------------------------------
constexpr int kDgWaves = 4;
// point m belongs to lane m % 64 in every loop, so a lane only ever re-reads the e[m] it wrote: first point of the lane at or after `begin`
__device__ inline int first_of(int begin, int lane) { return begin + ((lane - begin) & 63); }

__global__ __launch_bounds__(64 * kDgWaves) void density_grid_kernel(const float* __restrict__ scores, const float* __restrict__ cq,
                                                                      int H, int Q, int N, GridView g, int waves,
                                                                      float* __restrict__ alphas) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * waves + wave;
    if (wave >= waves || r >= H * Q) return;                 // (no barrier below: a wave owns its slice of LDS)
    float* Srow = lds + (size_t)wave * (N + g.M);
    float* E = Srow + N;
    const float bias = cq ? cq[r] : 0.f;
    for (int n = lane; n < N; n += 64) Srow[n] = scores[(long)r * N + n] + bias;
    __builtin_amdgcn_wave_barrier();                         // (a wave's LDS operations complete in order: the gather below sees the row)
    // s(t_m), in CSR order
    for (int m = lane; m < g.M; m += 64) {
        float s = 0.f;
        for (int j = g.pt_ptr[m]; j < g.pt_ptr[m + 1]; ++j) s += g.pt_val[j] * Srow[g.pt_box[j]];
        E[m] = s;
    }
    // per segment: e = exp(s - the segment's maximum) (dens is normalised inside the segment, so the segment's own maximum is what
    // keeps it in range), z_g = trapezoid sum of e, u_g = plain sum of e;  total = sum_g u_g / z_g
    double total = 0.0;
    for (int s = 0; s < g.G; ++s) {
        float mx = -INFINITY;
        for (int m = first_of(g.seg_begin[s], lane); m < g.seg_begin[s + 1]; m += 64) mx = fmaxf(mx, E[m]);
        mx = wave_max(mx);
        double z = 0.0, u = 0.0;
        for (int m = first_of(g.seg_begin[s], lane); m < g.seg_begin[s + 1]; m += 64) {
            const float e = expf(E[m] - mx);
            E[m] = e;
            z += (double)g.pt_weight[m] * (double)e;
            u += (double)e;
        }
        z = wave_sum_f64(z);
        u = wave_sum_f64(u);
        total += u / z;
    }
    const int h = r / Q, q = r - h * Q;
    float* out = alphas + ((long)q * H + h) * g.M;
    for (int s = 0; s < g.G; ++s) {
        double z = 0.0;
        for (int m = first_of(g.seg_begin[s], lane); m < g.seg_begin[s + 1]; m += 64) z += (double)g.pt_weight[m] * (double)E[m];
        z = wave_sum_f64(z);                                 // (the same sum in the same order as above)
        const double inv = 1.0 / (z * total);
        for (int m = first_of(g.seg_begin[s], lane); m < g.seg_begin[s + 1]; m += 64) out[m] = (float)((double)E[m] * inv);
    }
}

hipError_t launch_density_grid(const float* scores, const float* cq, int H, int Q, int N, const GridView& g, float* alphas,
                               hipStream_t stream) {
    const size_t per_wave = (size_t)(N + g.M) * sizeof(float);
    int waves = kDgWaves;
    while (waves > 1 && per_wave * waves > 64 * 1024) waves >>= 1;
    if (per_wave * waves > 64 * 1024) return hipErrorInvalidValue;
    const int rows = H * Q;
    INFV_LAUNCH(density_grid_kernel, dim3((unsigned)((rows + waves - 1) / waves)), dim3(64 * kDgWaves), per_wave * waves, stream,
                scores, cq, H, Q, N, g, waves, alphas);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------
// out[item][layer][n] = (1 / rows) * sum over the rows r = h * Q + q of alpha[r][n].
// Grid (column blocks of 64, layers, items); block = kBmWaves waves.  Wave k adds rows k, k + kBmWaves, ... in increasing
// order from 0; the kBmWaves partial sums are then added in wave order from 0, and the total is multiplied by 1 / rows.  All
// of it in float64; the product is rounded to fp32 once.
// FROM_SCORES: a row is a full score row (+ cq): the wave rebuilds its softmax weights -- the arithmetic of row_phase with
// expf, the maximum clamped at 0 from below so that the w_out term e^{-max} stays finite.  Else a row is alpha itself.
// ------------------------------------------------------------------------------------------------------
constexpr int kBmWaves = 8;
constexpr int kBmMaxN = 512;                                 // columns a wave holds in registers (FROM_SCORES)

template <bool FROM_SCORES>
__global__ __launch_bounds__(64 * kBmWaves) void box_mass_kernel(BoxMassArgs a) {
    __shared__ double part[kBmWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cb = blockIdx.x, l = blockIdx.y, item = blockIdx.z;
    const int n = cb * 64 + lane;
    const long slot = a.ring > 0 ? (a.slot0 + item) % a.ring : item;
    const float* src = a.src + slot * a.item_stride + (long)l * a.rows * a.N;
    double acc = 0.0;
    for (int r = wave; r < a.rows; r += kBmWaves) {
        const float* row = src + (long)r * a.N;
        if (FROM_SCORES) {
            const float bias = a.cq ? a.cq[(long)l * a.rows + r] : 0.f;
            float sv[kBmMaxN / 64];
            float m = 0.f;                                   // max(row maximum, 0)
#pragma unroll
            for (int k = 0; k < kBmMaxN / 64; ++k) {
                const int c = lane + 64 * k;
                sv[k] = (c < a.N) ? row[c] + bias : -INFINITY;
                m = fmaxf(m, sv[k]);
            }
            m = wave_max(m);
            double esum = 0.0;
            float mine = 0.f;
#pragma unroll
            for (int k = 0; k < kBmMaxN / 64; ++k) {
                const int c = lane + 64 * k;
                const float e = (c < a.N) ? a.w[c] * expf(sv[k] - m) : 0.f;
                esum += (double)e;
                if (k == cb) mine = e;
            }
            esum = wave_sum_f64(esum);
            acc += (double)mine / (esum + (double)(a.w_out * expf(-m)));
        } else if (n < a.N) {
            acc += (double)row[n];
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && n < a.N) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < kBmWaves; ++k) t += part[k][lane];
        a.out[(long)item * a.out_item_stride + (long)l * a.N + n] = (float)(t * (1.0 / (double)a.rows));
    }
}

// The packed trace of the lockstep calls (infv_ltm_set_videos_mass_trace): grid (column blocks of 64, layers, videos still running).
// Workgroup (cb, l, j) reduces the full score rows attend_videos_kernel just left in video rank j's handle (key bias included: no
// cq) into row chunk0 + s of mass_all -- the packed index of ctx, whatever the group and the rank.  Rows at and beyond `cap` are
// not written.  The arithmetic is box_mass_kernel<true>'s, restated: sharing one __device__ body changed that kernel's registers.
__global__ __launch_bounds__(64 * kBmWaves) void box_mass_videos_kernel(VideoStep vs, int rows, int N, int n_layers,
                                                                         const float* __restrict__ w, float w_out,
                                                                         float* __restrict__ mass_all, long cap) {
    __shared__ double part[kBmWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cb = blockIdx.x, l = blockIdx.y;
    const int n = cb * 64 + lane;
    const VideoDesc* v = vs.vd + blockIdx.z;
    const long chunk = v->chunk0 + vs.s;
    if (chunk >= cap) return;                                // (uniform over the workgroup: ahead of the barrier)
    const float* src = v->scores + (long)l * rows * N;
    double acc = 0.0;
    for (int r = wave; r < rows; r += kBmWaves) {
        const float* row = src + (long)r * N;
        float sv[kBmMaxN / 64];
        float m = 0.f;                                       // max(row maximum, 0)
#pragma unroll
        for (int k = 0; k < kBmMaxN / 64; ++k) {
            const int c = lane + 64 * k;
            sv[k] = (c < N) ? row[c] : -INFINITY;            // (full scores, key bias included: no cq term)
            m = fmaxf(m, sv[k]);
        }
        m = wave_max(m);
        double esum = 0.0;
        float mine = 0.f;
#pragma unroll
        for (int k = 0; k < kBmMaxN / 64; ++k) {
            const int c = lane + 64 * k;
            const float e = (c < N) ? w[c] * expf(sv[k] - m) : 0.f;
            esum += (double)e;
            if (k == cb) mine = e;
        }
        esum = wave_sum_f64(esum);
        acc += (double)mine / (esum + (double)(w_out * expf(-m)));
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && n < N) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < kBmWaves; ++k) t += part[k][lane];
        mass_all[(chunk * n_layers + l) * N + n] = (float)(t * (1.0 / (double)rows));
    }
}

bool box_mass_supported(int N) { return N > 0 && N <= kBmMaxN; }

hipError_t launch_box_mass(const BoxMassArgs& a, hipStream_t stream) {
    if (a.n_items <= 0) return hipSuccess;
    if (!box_mass_supported(a.N) || a.n_items > 65535 || a.L > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.N + 63) / 64), (unsigned)a.L, (unsigned)a.n_items);
    if (a.from_alpha) INFV_LAUNCH(box_mass_kernel<false>, grid, dim3(64 * kBmWaves), 0, stream, a);
    else INFV_LAUNCH(box_mass_kernel<true>, grid, dim3(64 * kBmWaves), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_box_mass_videos(const VideoStep& vs, int rows, int N, int n_layers, const float* w, float w_out, float* mass_all,
                                  long cap, hipStream_t stream) {
    if (vs.n == 0 || cap <= 0) return hipSuccess;
    if (!box_mass_supported(N) || n_layers > 65535 || vs.n > 65535) return hipErrorInvalidValue;
    INFV_LAUNCH(box_mass_videos_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)n_layers, (unsigned)vs.n), dim3(64 * kBmWaves), 0,
                stream, vs, rows, N, n_layers, w, w_out, mass_all, cap);
    return hipGetLastError();
}

}  // namespace infv

// ---- the entry points (include/infv_ltm.h) ----
#include "ltm_handle.h"

#include <vector>

using namespace infv;

namespace {

bool any_psi_plan(infv_ltm_handle h) {
    for (auto& kv : h->plans)
        if (kv.second->dense.psi_on) return true;
    return false;
}

// What both last-step read-outs need: a memory whose last step left its scores, under query length Q, on a box plan.
int check_last_step(infv_ltm_handle h, const char* name, int32_t layer, int32_t Q, const void* out, const Plan** plan) {
    if (int rc = check_handle(h)) return rc;
    if (layer < 0 || layer >= h->L) return fail(INFV_ERR_INVALID, "%s: layer out of range", name);
    if (!out) return fail(INFV_ERR_INVALID, "%s: null output", name);
    if (int rc = check_q(h, Q)) return rc;
    if (int rc = check_chain_error(h)) return rc;
    if (any_psi_plan(h)) return fail(INFV_ERR_UNSUPPORTED, "%s: general-psi plans (infv_ltm_set_psi_plan) have no box density", name);
    if (!h->mem.last_scores_readable())
        return fail(INFV_ERR_STATE, "%s: the handle holds no scores of a last step (no memory yet, or infv_ltm_import_state replaced it)", name);
    if (h->mem.lastQ() != Q) return fail(INFV_ERR_STATE, "%s: the last step ran with Q=%d, not %d", name, h->mem.lastQ(), Q);
    *plan = h->mem.last_plan() ? h->mem.last_plan() : (h->plans.empty() ? nullptr : h->plans.begin()->second);
    if (!*plan) return fail(INFV_ERR_NO_PLAN, "%s: no plan registered (its read-out weights are needed)", name);
    return INFV_OK;
}

// rows of `layer`: after the fused chain the bias-free scores + their bias term, else the attend kernel's full scores
void last_rows(infv_ltm_handle h, int layer, int Q, const float** rows, const float** cq) {
    const size_t n = (size_t)h->H * Q * h->N;
    if (h->mem.last_fast()) {
        *rows = h->Sp[h->mem.sc()].as<float>() + (size_t)layer * n;
        *cq = h->cqbuf.as<float>() + (size_t)layer * h->H * Q;
    } else {
        *rows = h->scores.as<float>() + (size_t)layer * n;
        *cq = nullptr;
    }
}

}  // namespace

namespace infv {
int trace_masses_of_step(infv_ltm_handle h, const Plan& plan, int Q, hipStream_t stream) {
    if (!h->mass_trace || h->mass_at < 0 || h->mass_at >= h->mass_cap) return INFV_OK;
    BoxMassArgs a;
    memset(&a, 0, sizeof(a));
    a.src = h->scores.as<float>(); a.n_items = 1; a.L = h->L; a.rows = h->H * Q; a.N = h->N;
    a.w = plan.w.as<float>(); a.w_out = plan.w_out;
    a.out = h->mass_trace + (size_t)h->mass_at * h->L * h->N; a.out_item_stride = (long)h->L * h->N;
    HIP_TRY(launch_box_mass(a, stream));
    return INFV_OK;
}
}  // namespace infv

extern "C" {

int infv_ltm_set_grid_plan(infv_ltm_handle h, const infv_ltm_grid_plan* p) {
    if (int rc = check_handle(h)) return rc;
    if (!p || !p->seg_begin || !p->pt_weight || !p->pt_ptr) return fail(INFV_ERR_INVALID, "grid plan: null argument");
    const int M = p->n_points, G = p->n_segments;
    if (M < 2 || M > 4096) return fail(INFV_ERR_INVALID, "grid plan: n_points=%d outside [2, 4096]", M);
    if (G < 1 || G > 16) return fail(INFV_ERR_INVALID, "grid plan: n_segments=%d outside [1, 16]", G);
    if (p->seg_begin[0] != 0 || p->seg_begin[G] != M) return fail(INFV_ERR_INVALID, "grid plan: seg_begin must run from 0 to n_points");
    for (int g = 0; g < G; ++g)
        if (p->seg_begin[g + 1] - p->seg_begin[g] < 2)
            return fail(INFV_ERR_INVALID, "grid plan: segment %d has fewer than two points (no trapezoid)", g);
    if (p->pt_ptr[0] != 0) return fail(INFV_ERR_INVALID, "grid plan: pt_ptr[0] must be 0");
    for (int m = 0; m < M; ++m) {
        if (p->pt_ptr[m + 1] < p->pt_ptr[m]) return fail(INFV_ERR_INVALID, "grid plan: pt_ptr not monotone at point %d", m);
        if (p->pt_ptr[m + 1] - p->pt_ptr[m] > h->N) return fail(INFV_ERR_INVALID, "grid plan: point %d lies in more boxes than there are", m);
        if (!(p->pt_weight[m] >= 0.f) || p->pt_weight[m] > 1e30f) return fail(INFV_ERR_INVALID, "grid plan: pt_weight[%d] is negative or not finite", m);
    }
    const int nnz = p->pt_ptr[M];
    if (nnz > 0 && (!p->pt_box || !p->pt_val)) return fail(INFV_ERR_INVALID, "grid plan: null argument");
    for (int j = 0; j < nnz; ++j) {
        if (p->pt_box[j] < 0 || p->pt_box[j] >= h->N) return fail(INFV_ERR_INVALID, "grid plan: pt_box[%d]=%d outside [0, %d)", j, p->pt_box[j], h->N);
        if (!(p->pt_val[j] == p->pt_val[j]) || p->pt_val[j] > 1e30f || p->pt_val[j] < -1e30f)
            return fail(INFV_ERR_INVALID, "grid plan: pt_val[%d] is not finite", j);
    }
    if ((size_t)(h->N + M) * sizeof(float) > 64 * 1024) return fail(INFV_ERR_INVALID, "grid plan: num_basis + n_points exceed a wave's 64 KB of LDS");
    if (any_psi_plan(h)) return fail(INFV_ERR_UNSUPPORTED, "grid plan: general-psi plans (infv_ltm_set_psi_plan) have no box density");
    HIP_TRY(hipDeviceSynchronize());                            // a density call may still be reading the old tables
    GridPlan& g = h->grid;
    g.on = false;
    HIP_TRY(upload(g.seg_begin, p->seg_begin, (size_t)G + 1));
    HIP_TRY(upload(g.pt_weight, p->pt_weight, (size_t)M));
    HIP_TRY(upload(g.pt_ptr, p->pt_ptr, (size_t)M + 1));
    HIP_TRY(upload(g.pt_box, p->pt_box, (size_t)nnz));
    HIP_TRY(upload(g.pt_val, p->pt_val, (size_t)nnz));
    g.M = M; g.G = G; g.on = true;
    return INFV_OK;
}

int infv_ltm_density(infv_ltm_handle h, int32_t layer, int32_t Q, float* alphas, void* stream) {
    const Plan* plan = nullptr;
    if (int rc = check_last_step(h, "density", layer, Q, alphas, &plan)) return rc;
    if (!h->grid.on) return fail(INFV_ERR_STATE, "density: no grid plan (infv_ltm_set_grid_plan)");
    const float *rows, *cq;
    last_rows(h, layer, Q, &rows, &cq);
    HIP_TRY(launch_density_grid(rows, cq, h->H, Q, h->N, h->grid.view(), alphas, static_cast<hipStream_t>(stream)));
    return INFV_OK;
}

int infv_ltm_masses(infv_ltm_handle h, int32_t layer, int32_t Q, float* mass, void* stream) {
    const Plan* plan = nullptr;
    if (int rc = check_last_step(h, "masses", layer, Q, mass, &plan)) return rc;
    if (!box_mass_supported(h->N)) return fail(INFV_ERR_UNSUPPORTED, "masses: num_basis=%d above 512", h->N);
    BoxMassArgs a;
    memset(&a, 0, sizeof(a));
    last_rows(h, layer, Q, &a.src, &a.cq);
    a.n_items = 1; a.L = 1; a.rows = h->H * Q; a.N = h->N;
    a.w = plan->w.as<float>(); a.w_out = plan->w_out;
    a.out = mass; a.out_item_stride = h->N;
    HIP_TRY(launch_box_mass(a, static_cast<hipStream_t>(stream)));
    return INFV_OK;
}

int infv_ltm_set_mass_trace(infv_ltm_handle h, float* mass_all, int64_t capacity_chunks) {
    if (int rc = check_handle(h)) return rc;
    if (capacity_chunks < 0) return fail(INFV_ERR_INVALID, "set_mass_trace: negative capacity");
    if (capacity_chunks > 0 && !mass_all) return fail(INFV_ERR_INVALID, "set_mass_trace: null buffer");
    if (capacity_chunks > 0 && any_psi_plan(h))
        return fail(INFV_ERR_UNSUPPORTED, "set_mass_trace: general-psi plans (infv_ltm_set_psi_plan) have no box masses");
    if (capacity_chunks > 0 && !box_mass_supported(h->N)) return fail(INFV_ERR_UNSUPPORTED, "set_mass_trace: num_basis=%d above 512", h->N);
    h->mass_trace = capacity_chunks ? mass_all : nullptr;
    h->mass_cap = (long)capacity_chunks;
    return INFV_OK;
}

int infv_ltm_set_videos_mass_trace(infv_ltm_handle lead, float* mass_all, int64_t capacity_chunks) {
    if (int rc = check_handle(lead)) return rc;
    if (capacity_chunks < 0) return fail(INFV_ERR_INVALID, "set_videos_mass_trace: negative capacity");
    if (capacity_chunks > 0 && !mass_all) return fail(INFV_ERR_INVALID, "set_videos_mass_trace: null buffer");
    if (capacity_chunks > 0 && any_psi_plan(lead))
        return fail(INFV_ERR_UNSUPPORTED, "set_videos_mass_trace: general-psi plans (infv_ltm_set_psi_plan) have no box masses");
    if (capacity_chunks > 0 && !box_mass_supported(lead->N))
        return fail(INFV_ERR_UNSUPPORTED, "set_videos_mass_trace: num_basis=%d above 512", lead->N);
    lead->vmass_trace = capacity_chunks ? mass_all : nullptr;
    lead->vmass_cap = (long)capacity_chunks;
    return INFV_OK;
}

}  // extern "C"
