// The sampler's per-step arithmetic: the first-order (DDIM / DDPM) and the DPM-Solver++(2M) step of one call and of the batcher's row
// tables, the Philox normal stream they draw from, the column gather of the step noise, the guidance rescale and the weighted multi-prompt combine,
// and the two row kernels of DDPM inversion (q_sample at a timestep per row, the step noise that reproduces a given next state).  fp32 NCHW throughout.
// Row kernels are written from the parts of row_kernels.hpp.  The four step kernels decode their row into one descriptor
// (step_row) and run one loop (step_row_loop), and the two gain kernels run one two-pass routine (gain_row) on their piece policies: a
// row of a rows form is the same bits as the call form on the same inputs because it is the same code.  (The gathered-noise fields are
// still decoded and checked twice, in table_row and in q_sample_rows_kernel: see profiles/row_kernels_refactor_ab.txt.)
#include "row_kernels.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ Philox4x32-10
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
}
// Philox4x32-10 block of counter `ctr` under key `seed`, Box-Muller'd into four N(0,1) lanes; pair h (lanes 2h, 2h+1) only needs
// words 2h, 2h+1 of the block, so a caller that wants one lane computes one pair (same bits as the four-lane form)
__device__ __forceinline__ void philox_block(uint64_t seed, uint64_t ctr, uint32_t (&c)[4]) {
    c[0] = (uint32_t)ctr; c[1] = (uint32_t)(ctr >> 32); c[2] = 0u; c[3] = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float u1 = ((float)(a >> 8) + 0.5f) * (1.0f / 16777216.0f);      // (0,1)
    const float u2 = ((float)(b >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    float s, cs;
    sincospif(2.0f * u2, &s, &cs);
    z0 = r * cs;
    z1 = r * s;
}
// element e of the stream (seed, offset): lane e % 4 of counter offset + e / 4 — what ds_philox_normal writes at out[e]
__device__ __forceinline__ float philox_normal_at(uint64_t seed, uint64_t offset, uint64_t e) {
    uint32_t c[4];
    philox_block(seed, offset + e / 4, c);
    const int lane = (int)(e & 3), h = lane >> 1;
    float z0, z1;
    box_muller(c[2 * h], c[2 * h + 1], z0, z1);
    return (lane & 1) ? z1 : z0;
}

__global__ void philox_normal_kernel(float* out, size_t n, uint64_t seed, uint64_t offset) {
    const size_t nq = (n + 3) / 4;
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < nq; q += (size_t)gridDim.x * blockDim.x) {
        uint32_t c[4];
        philox_block(seed, offset + q, c);
        float z[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) box_muller(c[2 * h], c[2 * h + 1], z[2 * h], z[2 * h + 1]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q * 4 + j < n) out[q * 4 + j] = z[j];
    }
}

// ------------------------------------------------------------------------------------------------ sampler step
// Every operation below is a separately rounded IEEE fp32 op in the reference's order
// (DiffSynthSampler.py:320,327,337,343,291-293,506): contraction into FMA is switched off.
#pragma clang fp contract(off)
// cf: sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2), sigma; qc: sqrt(acp[t-1]), sqrt(1-acp[t-1]) (blend mode 1 only);
// m / g / n0: mask, guide and initial noise of the element (blend modes 1 / 2 only)
__device__ __forceinline__ float guided_eps(float eps, bool cfg, float eps_c, float cfg_scale) {
    if (cfg) {
        const float d = eps_c - eps;
        const float sd = cfg_scale * d;
        eps = eps + sd;
    }
    return eps;
}
__device__ __forceinline__ float predicted_x0(float x, float eps, float sigma_t, float alpha_t) {
    const float t0 = sigma_t * eps;
    const float t1 = x - t0;
    return t1 / alpha_t;
}
// q_sample (DiffSynthSampler.py:291-293): two products, one sum
__device__ __forceinline__ float q_sample_element(float x0, float noise, float q0, float q1) {
    const float g0 = q0 * x0;
    const float g1 = q1 * noise;
    return g0 + g1;
}
__device__ __forceinline__ float inpaint_blend(float v, int blend_mode, float m, float g, float n0, float q0, float q1) {
    if (blend_mode) {
        if (blend_mode == 1) g = q_sample_element(g, n0, q0, q1);
        const float w0 = m * g;
        const float w1 = (1.0f - m) * v;
        v = w0 + w1;
    }
    return v;
}
__device__ __forceinline__ float step_element(float x, float eps, bool cfg, float eps_c, float cfg_scale, const float (&cf)[5], float noise,
                                              int blend_mode, float m, float g, float n0, float q0, float q1) {
    eps = guided_eps(eps, cfg, eps_c, cfg_scale);
    const float x0 = predicted_x0(x, eps, cf[0], cf[1]);
    const float u0 = cf[2] * x0;
    const float u1 = cf[3] * eps;
    const float u2 = cf[4] * noise;
    return inpaint_blend((u0 + u1) + u2, blend_mode, m, g, n0, q0, q1);
}
// "dpmpp_2m" (DPM-Solver++(2M)): cf = sigma_t, alpha_t, c_x, c_0, c_1 (sampler.py: _solver_coefficients); x0 is step_element's.  `hist` is the
// previous step's x0 (used only where second, i.e. c_1 != 0) and receives this step's: the blend changes the state, never the history
__device__ __forceinline__ float dpm_element(float x, float eps, bool cfg, float eps_c, float cfg_scale, const float (&cf)[5], bool second,
                                             float& hist, int blend_mode, float m, float g, float n0, float q0, float q1) {
    eps = guided_eps(eps, cfg, eps_c, cfg_scale);
    const float x0 = predicted_x0(x, eps, cf[0], cf[1]);
    const float u0 = cf[2] * x;
    const float u1 = cf[3] * x0;
    float v = u0 + u1;
    if (second) {
        const float u2 = cf[4] * hist;
        v = v + u2;
    }
    hist = x0;
    return inpaint_blend(v, blend_mode, m, g, n0, q0, q1);
}
// The step noise that makes step_element go from x to x_prev ("edit-friendly" DDPM inversion): z = (x_prev - mu) / sigma with mu the
// first two terms of step_element's sum (cf[4] != 0: the caller's business)
__device__ __forceinline__ float edit_noise_element(float x, float x_prev, float eps, bool cfg, float eps_c, float cfg_scale, const float (&cf)[5]) {
    eps = guided_eps(eps, cfg, eps_c, cfg_scale);
    const float x0 = predicted_x0(x, eps, cf[0], cf[1]);
    const float u0 = cf[2] * x0;
    const float u1 = cf[3] * eps;
    const float mu = u0 + u1;
    const float d = x_prev - mu;
    return d / cf[4];
}

// One row (C*H*W elements of one sample) of a step launch, whichever entry point it came through.  eps_c / dup / hist may be null;
// mask / guide / init are read only as blend says (mask: H*W floats, or C*H*W where mask_chw).  Step noise (first order only):
// NZ_DENSE reads nz[i]; NZ_DRAW / NZ_PHILOX (the values of DS_SR_NOISE) gather element (c, h, j) from
// e = ((sample * C + c) * H + h) * draw_w + cols[cols_off + j] of the draw nz, or of the Philox stream (seed, offset).
enum { NZ_NONE = 0, NZ_DRAW = 1, NZ_PHILOX = 2, NZ_DENSE = 3 };
struct step_row {
    const float* x; const float* eps; const float* eps_c; float* out; float* dup; float* hist;
    const float* mask; const float* guide; const float* init;
    float cf[5], q0, q1, scale;
    int blend, mask_chw;
    int noise, sample, draw_w, cols_off;
    const float* nz;
    uint64_t seed, offset;
};

// V elements from element i0 on of the row's gathered noise (a.noise is NZ_DRAW or NZ_PHILOX; V == 4: the piece is inside one image row)
template <int V>
__device__ __forceinline__ void gathered_noise(const step_row& a, size_t i0, int W, uint64_t CH, const int32_t* cols, float (&nz)[V]) {
    const int j0 = (int)(i0 % W);
    const uint64_t e0 = ((uint64_t)a.sample * CH + i0 / W) * (uint64_t)a.draw_w;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        int col = cols[a.cols_off + j0 + k];
        col = col < 0 ? 0 : (col >= a.draw_w ? a.draw_w - 1 : col);
        nz[k] = a.noise == NZ_DRAW ? a.nz[e0 + (uint64_t)col] : philox_normal_at(a.seed, a.offset, e0 + (uint64_t)col);
    }
}

// The row in pieces of V elements, grid-strided along x.  V == 4 only when x / eps / eps_c / out / dup (and a dense noise row) are
// 16-byte aligned and a piece crosses neither a mask plane nor, for the gathered noise, an image row.  avec / hvec: the row's own blend
// operands / its history are 16-byte aligned too (V == 4 only; see row_vec).  W, CH (= C*H) and cols serve the gathered noise only.
template <int V, bool SOLVER>
__device__ __forceinline__ void step_row_loop(const step_row& a, bool avec, bool hvec, int HW, size_t CHW, int W = 0, uint64_t CH = 0,
                                              const int32_t* cols = nullptr) {
    const bool cfg = a.eps_c != nullptr, second = SOLVER && a.cf[4] != 0.f;
    DS_FOR_PIECES(V, CHW, i0) {
        float xv[V], ev[V], ecv[V] = {}, mv[V] = {}, gv[V] = {}, n0[V] = {}, o[V];
        float nh[V] = {};                                             // step noise (first order) / history (solver)
        load_v<V>(a.x + i0, true, xv);
        load_v<V>(a.eps + i0, true, ev);
        if (cfg) load_v<V>(a.eps_c + i0, true, ecv);
        if (a.blend) {
            load_v<V>(a.mask + (a.mask_chw ? i0 : i0 % HW), avec, mv);
            load_v<V>(a.guide + i0, avec, gv);
            if (a.blend == 1) load_v<V>(a.init + i0, avec, n0);
        }
        if constexpr (SOLVER) {
            if (second) load_v<V>(a.hist + i0, hvec, nh);
        } else if (a.noise == NZ_DENSE) {
            load_v<V>(a.nz + i0, true, nh);
        } else if (a.noise != NZ_NONE) {
            gathered_noise<V>(a, i0, W, CH, cols, nh);
        }
#pragma unroll
        for (int k = 0; k < V; ++k)
            o[k] = SOLVER ? dpm_element(xv[k], ev[k], cfg, ecv[k], a.scale, a.cf, second, nh[k], a.blend, mv[k], gv[k], n0[k], a.q0, a.q1)
                          : step_element(xv[k], ev[k], cfg, ecv[k], a.scale, a.cf, nh[k], a.blend, mv[k], gv[k], n0[k], a.q0, a.q1);
        store_v<V>(a.out + i0, true, o);
        if (a.dup) store_v<V>(a.dup + i0, true, o);
        if (SOLVER && a.hist) store_v<V>(a.hist + i0, hvec, nh);
    }
}
// Call form: sample b of ds_step_params / ds_dpm_step_params (no duplicate; the caller adds its noise or its history)
template <class P>
__device__ __forceinline__ step_row call_row(const P& p, int b, int HW, size_t CHW) {
    step_row a = {};
    a.x = p.x + (size_t)b * CHW;
    a.eps = p.eps + (size_t)b * CHW;
    a.eps_c = p.eps_cond ? p.eps_cond + (size_t)b * CHW : nullptr;
    a.out = p.out + (size_t)b * CHW;
#pragma unroll
    for (int k = 0; k < 5; ++k) a.cf[k] = p.coef[(size_t)b * 5 + k];
    a.scale = p.cfg_scale;
    a.blend = p.blend_mode;
    a.mask_chw = p.mask_chw;
    if (p.blend_mode) {
        a.mask = p.mask + (size_t)b * (p.mask_chw ? CHW : (size_t)HW);
        a.guide = p.guide + (size_t)b * CHW;
        if (p.blend_mode == 1) {
            a.init = p.init_noise + (size_t)b * CHW;
            a.q0 = p.qcoef[(size_t)b * 2];
            a.q1 = p.qcoef[(size_t)b * 2 + 1];
        }
    }
    return a;
}

// Table form: row r of the DS_SR_* tables, plus hrow[r] in the solver form.  The table is the host's.  A row that points outside the
// declared bounds, names an unknown mode or lacks a pointer its modes need is never read out of bounds: its output row (and its
// duplicate, when that one is in range) is filled with NaN so that a malformed table shows in the result, and a row whose output row
// itself is out of range writes nothing.  The first-order form validates its noise fields; the solver form draws no noise
// (DS_SR_NOISE must be 0) and needs a history wherever coef[4] != 0.  False: the row is finished.
template <bool SOLVER>
__device__ __forceinline__ bool table_row(const ds_step_rows_params& p, const uint64_t* hrow, int r, size_t CHW, step_row& a) {
    const int32_t* ir = p.irow + (size_t)r * DS_SR_NI;
    const float* fr = p.frow + (size_t)r * DS_SR_NF;
    const uint64_t* pr = p.prow + (size_t)r * DS_SR_NP;
    const int xr = ir[DS_SR_X], er = ir[DS_SR_EPS], ecr = ir[DS_SR_EPSC], orow = ir[DS_SR_OUT], dup = ir[DS_SR_DUP];
    const int drows = ir[DS_SR_DRAW_ROWS];
    a.blend = ir[DS_SR_BLEND];
    a.mask_chw = ir[DS_SR_MASK_CHW];
    a.noise = ir[DS_SR_NOISE];
    a.sample = ir[DS_SR_SAMPLE];
    a.draw_w = ir[DS_SR_DRAW_W];
    a.cols_off = ir[DS_SR_COLS];
    a.guide = reinterpret_cast<const float*>(pr[DS_SR_GUIDE]);
    a.init = reinterpret_cast<const float*>(pr[DS_SR_INIT]);
    a.mask = reinterpret_cast<const float*>(pr[DS_SR_MASKP]);
    a.nz = reinterpret_cast<const float*>(pr[DS_SR_DRAW]);
    a.seed = pr[DS_SR_SEED];
    a.offset = pr[DS_SR_OFFSET];
    a.hist = SOLVER ? reinterpret_cast<float*>(hrow[r]) : nullptr;
#pragma unroll
    for (int k = 0; k < 5; ++k) a.cf[k] = fr[DS_SR_COEF + k];
    a.q0 = fr[DS_SR_Q0];
    a.q1 = fr[DS_SR_Q1];
    a.scale = fr[DS_SR_CFG];
    if (orow < 0 || orow >= p.Bout) return false;
    a.out = p.out + (size_t)orow * CHW;
    a.dup = dup >= 0 && dup < p.Bout ? p.out + (size_t)dup * CHW : nullptr;
    const bool bad = xr < 0 || xr >= p.Bx || er < 0 || er >= p.Beps || ecr >= p.Beps || dup >= p.Bout || a.blend < 0 || a.blend > 2 ||
                     a.noise < 0 || a.noise > (SOLVER ? NZ_NONE : NZ_PHILOX) ||
                     (a.blend && (!a.guide || !a.mask || (a.blend == 1 && !a.init))) ||
                     (a.noise && (a.sample < 0 || a.sample >= drows || a.draw_w <= 0 || a.cols_off < 0 || a.cols_off > p.n_cols - p.W ||
                                  (a.noise == NZ_DRAW && !a.nz))) ||
                     (SOLVER && !a.hist && a.cf[4] != 0.f);
    if (bad) {
        nan_row(a.out, a.dup, CHW);
        return false;
    }
    a.x = p.x + (size_t)xr * CHW;
    a.eps = p.eps + (size_t)er * CHW;
    a.eps_c = ecr >= 0 ? p.eps + (size_t)ecr * CHW : nullptr;
    return true;
}

// grid (x: pieces of a row, y: samples, strided: B has no upper limit).  V == 4: see ds_ddim_step
template <int V>
__global__ __launch_bounds__(256) void ddim_step_kernel(const ds_step_params p) {
    for (int b = blockIdx.y; b < p.B; b += gridDim.y) {
        step_row a = call_row(p, b, p.HW, (size_t)p.CHW);
        a.noise = NZ_DENSE;
        a.nz = p.noise + (size_t)b * p.CHW;
        step_row_loop<V, false>(a, row_vec<V>(a.guide, a.init, a.mask), false, p.HW, (size_t)p.CHW);
    }
}
// grid (x: pieces of a row, y: sample).  V == 4 only when W % 4 == 0 and every pointer given is 16-byte aligned: nothing is left to
// decide per row
template <int V>
__global__ __launch_bounds__(256) void dpm_step_kernel(const ds_dpm_step_params p) {
    const int b = blockIdx.y, HW = p.H * p.W;
    const size_t CHW = (size_t)p.C * HW;
    step_row a = call_row(p, b, HW, CHW);
    a.hist = p.hist ? p.hist + (size_t)b * CHW : nullptr;
    if (!a.hist && a.cf[4] != 0.f) nan_row(a.out, nullptr, CHW);    // a second-order row without a history: nothing is read
    else step_row_loop<V, true>(a, V == 4, V == 4, HW, CHW);
}
// grid (x: pieces of a row, y: table row).  V == 4 only when W % 4 == 0 and x / eps / out are 16-byte aligned
template <int V>
__global__ __launch_bounds__(256) void step_rows_kernel(const ds_step_rows_params p) {
    const int HW = p.H * p.W;
    const size_t CHW = (size_t)p.C * HW;
    step_row a = {};
    if (table_row<false>(p, nullptr, blockIdx.y, CHW, a))
        step_row_loop<V, false>(a, row_vec<V>(a.guide, a.init, a.mask), false, HW, CHW, p.W, (uint64_t)p.C * p.H, p.cols);
}
template <int V>
__global__ __launch_bounds__(256) void dpm_step_rows_kernel(const ds_step_rows_params p, const uint64_t* hrow) {
    const int HW = p.H * p.W;
    const size_t CHW = (size_t)p.C * HW;
    step_row a = {};
    if (table_row<true>(p, hrow, blockIdx.y, CHW, a)) step_row_loop<V, true>(a, row_vec<V>(a.guide, a.init, a.mask), row_vec<V>(a.hist), HW, CHW);
}

// ds_q_sample_rows: row r of the DS_QS_* tables is q_sample of one sample with its noise gathered as the step kernels gather theirs
// (gathered_noise; the fields and their checks are table_row's).  table_row's rule for a malformed row.  grid (x: pieces of a row, y: table row); V == 4 only when
// W % 4 == 0 and x0 / out are aligned
template <int V>
__global__ __launch_bounds__(256) void q_sample_rows_kernel(const ds_q_sample_rows_params p) {
    const size_t CHW = (size_t)p.C * p.H * p.W;
    const int32_t* ir = p.irow + (size_t)blockIdx.y * DS_QS_NI;
    const float* fr = p.frow + (size_t)blockIdx.y * DS_QS_NF;
    const uint64_t* pr = p.prow + (size_t)blockIdx.y * DS_QS_NP;
    const int src = ir[DS_QS_SRC], orow = ir[DS_QS_OUT], dup = ir[DS_QS_DUP], drows = ir[DS_QS_DRAW_ROWS];
    step_row a = {};
    a.noise = ir[DS_QS_NOISE];
    a.sample = ir[DS_QS_SAMPLE];
    a.draw_w = ir[DS_QS_DRAW_W];
    a.cols_off = ir[DS_QS_COLS];
    a.nz = reinterpret_cast<const float*>(pr[DS_QS_DRAW]);
    a.seed = pr[DS_QS_SEED];
    a.offset = pr[DS_QS_OFFSET];
    a.q0 = fr[DS_QS_Q0];
    a.q1 = fr[DS_QS_Q1];
    if (orow < 0 || orow >= p.Bout) return;
    a.out = p.out + (size_t)orow * CHW;
    a.dup = dup >= 0 && dup < p.Bout ? p.out + (size_t)dup * CHW : nullptr;
    const bool bad = src < 0 || src >= p.Bx0 || dup >= p.Bout || (a.noise != NZ_DRAW && a.noise != NZ_PHILOX) || a.sample < 0 ||
                     a.sample >= drows || a.draw_w <= 0 || a.cols_off < 0 || a.cols_off > p.n_cols - p.W || (a.noise == NZ_DRAW && !a.nz);
    if (bad) {
        nan_row(a.out, a.dup, CHW);
        return;
    }
    a.x = p.x0 + (size_t)src * CHW;
    const uint64_t CH = (uint64_t)p.C * p.H;
    DS_FOR_PIECES(V, CHW, i0) {
        float xv[V], nz[V], o[V];
        load_v<V>(a.x + i0, true, xv);
        gathered_noise<V>(a, i0, p.W, CH, p.cols, nz);
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = q_sample_element(xv[k], nz[k], a.q0, a.q1);
        store_v<V>(a.out + i0, true, o);
        if (a.dup) store_v<V>(a.dup + i0, true, o);
    }
}

// ds_edit_noise_rows: row r of the DS_EN_* tables.  x_prev is a row of X or the row's own address (16-byte pieces only where that
// address allows: row_vec).  table_row's rule for a malformed row; a row with coef[4] == 0 is zeros and reads nothing.
// grid (x: pieces of a row, y: table row); V == 4 only when W % 4 == 0 and X / eps / z are aligned
template <int V>
__global__ __launch_bounds__(256) void edit_noise_rows_kernel(const ds_edit_noise_rows_params p) {
    const size_t CHW = (size_t)p.C * p.H * p.W;
    const int32_t* ir = p.irow + (size_t)blockIdx.y * DS_EN_NI;
    const float* fr = p.frow + (size_t)blockIdx.y * DS_EN_NF;
    const int xr = ir[DS_EN_X], prow = ir[DS_EN_PREV], er = ir[DS_EN_EPS], ecr = ir[DS_EN_EPSC], orow = ir[DS_EN_OUT];
    const float* prev = reinterpret_cast<const float*>(p.prow[(size_t)blockIdx.y * DS_EN_NP + DS_EN_PREVP]);
    float cf[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) cf[k] = fr[DS_EN_COEF + k];
    const float scale = fr[DS_EN_CFG];
    if (orow < 0 || orow >= p.Bz) return;
    float* out = p.z + (size_t)orow * CHW;
    if (xr < 0 || xr >= p.Bx || prow >= p.Bx || (prow < 0 && !prev) || er < 0 || er >= p.Beps || ecr >= p.Beps) {
        nan_row(out, nullptr, CHW);
        return;
    }
    if (cf[4] == 0.f) {
        fill_row(out, nullptr, CHW, 0.f);
        return;
    }
    if (prow >= 0) prev = p.X + (size_t)prow * CHW;
    const float* x = p.X + (size_t)xr * CHW;
    const float* eps = p.eps + (size_t)er * CHW;
    const float* eps_c = ecr >= 0 ? p.eps + (size_t)ecr * CHW : nullptr;
    const bool cfg = eps_c != nullptr, pvec = row_vec<V>(prev);
    DS_FOR_PIECES(V, CHW, i0) {
        float xv[V], pv[V], ev[V], ecv[V] = {}, o[V];
        load_v<V>(x + i0, true, xv);
        load_v<V>(prev + i0, pvec, pv);
        load_v<V>(eps + i0, true, ev);
        if (cfg) load_v<V>(eps_c + i0, true, ecv);
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = edit_noise_element(xv[k], pv[k], ev[k], cfg, ecv[k], scale, cf);
        store_v<V>(out + i0, true, o);
    }
}
#pragma clang fp contract(fast)

// ------------------------------------------------------------------------------------------------ guidance rescale
// out = g e with e = guided_eps(eps_u, eps_c, s) and g = phi std(eps_c) / std(e) + (1 - phi) over one row of N elements.  One block of
// CR_THREADS per row: piece v (elements [4v, 4v + 4)) belongs to thread v % CR_THREADS in the 16-byte and in the scalar form alike, a
// thread adds its elements in ascending order into float64 sums, and the sums meet in wave_sum and then wave by wave — an order that
// N alone decides.  Two passes about the mean: sums, then squares of the distances from the means (the common 1 / (N - 1) of the two
// variances cancels in the ratio).  cfg_rescale_kernel and cfg_rescale_rows_kernel both run cfg_rescale_row, so a row of
// ds_cfg_rescale_rows is the same bits as ds_cfg_rescale given the same inputs.
constexpr int CR_THREADS = 1024, CR_WAVES = CR_THREADS / 64;

// piece at element i0: n (1..4) elements are inside the row; vec only where every piece is whole
__device__ __forceinline__ void cr_load(const float* p, int i0, int n, bool vec, float (&v)[4]) {
    if (vec) {
        load_v<4>(p + i0, true, v);
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < n ? p[i0 + k] : 0.f;
}
// both totals to every thread
__device__ __forceinline__ void cr_block_sum(double& a, double& b, double (&red)[2][CR_WAVES]) {
    a = wave_sum(a);
    b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = b = 0.0;
#pragma unroll
    for (int w = 0; w < CR_WAVES; ++w) {
        a += red[0][w];
        b += red[1][w];
    }
}
#pragma clang fp contract(off)
// The gain of one row and the scaled row: g = phi std(p) / std(e) + (1 - phi), out = g e, with (p, e) the row's two sequences as the
// piece policy gives them: piece(i0, n, vec, p, e) fills the piece at element i0, of which n (1..4) elements are inside the row.
// phi == 0: g = 1 and nothing is summed; Piece::UNIT_GAIN_MULTIPLIES says whether the store pass then still multiplies by g
template <class Piece>
__device__ __forceinline__ float gain_row(const Piece& piece, float* out, int N, bool vec, float phi, double (&red)[2][2][CR_WAVES]) {
    const int nv = (N + 3) / 4;
    float g = 1.0f;
    if (phi != 0.f) {                                   // (block-uniform)
        double sp = 0.0, se = 0.0;
        for (int v = threadIdx.x; v < nv; v += CR_THREADS) {
            const int i0 = v * 4, n = min(4, N - i0);
            float p[4], e[4];
            piece(i0, n, vec, p, e);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) {
                    sp += (double)p[k];
                    se += (double)e[k];
                }
        }
        cr_block_sum(sp, se, red[0]);
        const double mp = sp / N, me = se / N;
        double qp = 0.0, qe = 0.0;
        for (int v = threadIdx.x; v < nv; v += CR_THREADS) {
            const int i0 = v * 4, n = min(4, N - i0);
            float p[4], e[4];
            piece(i0, n, vec, p, e);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) {
                    const double dp = (double)p[k] - mp, de = (double)e[k] - me;
                    qp += dp * dp;
                    qe += de * de;
                }
        }
        cr_block_sum(qp, qe, red[1]);
        const double ratio = qe > 0.0 ? sqrt(qp / qe) : 1.0;          // std(e) == 0: nothing to scale
        g = (float)((double)phi * ratio + (1.0 - (double)phi));
    }
    for (int v = threadIdx.x; v < nv; v += CR_THREADS) {
        const int i0 = v * 4, n = min(4, N - i0);
        float p[4], e[4];
        piece(i0, n, vec, p, e);
        if (Piece::UNIT_GAIN_MULTIPLIES || phi != 0.f)
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] = g * e[k];
        if (vec) store_v<4>(out + i0, true, e);
        else
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) out[i0 + k] = e[k];
    }
    return g;
}
// guidance rescale: p = eps_c, e = guided_eps(eps_u, eps_c, s); g == 1.0f multiplies the row of phi == 0 too
struct cr_piece {
    const float* u; const float* c;
    float scale;
    static constexpr bool UNIT_GAIN_MULTIPLIES = true;
    __device__ __forceinline__ void operator()(int i0, int n, bool vec, float (&p)[4], float (&e)[4]) const {
        float uv[4], cv[4];
        cr_load(u, i0, n, vec, uv);
        cr_load(c, i0, n, vec, cv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p[k] = cv[k];
            e[k] = guided_eps(uv[k], true, cv[k], scale);
        }
    }
};
__device__ __forceinline__ float cfg_rescale_row(const float* u, const float* c, float* out, int N, float scale, float phi,
                                                 double (&red)[2][2][CR_WAVES]) {
    const bool vec = N % 4 == 0 && ((((uint64_t)u | (uint64_t)c | (uint64_t)out) & 15) == 0);
    return gain_row(cr_piece{u, c, scale}, out, N, vec, phi, red);
}
#pragma clang fp contract(fast)

// grid: one block per sample
__global__ __launch_bounds__(CR_THREADS) void cfg_rescale_kernel(const ds_cfg_rescale_params p) {
    __shared__ double red[2][2][CR_WAVES];
    const size_t off = (size_t)blockIdx.x * p.CHW;
    const float g = cfg_rescale_row(p.eps_u + off, p.eps_c + off, p.out + off, p.CHW, p.cfg_scale, p.phi, red);
    if (p.gain && threadIdx.x == 0) p.gain[blockIdx.x] = g;
}

// grid: one block per table row.  The table is the host's: a row that points outside the buffer is never read out of bounds (see
// table_row)
__global__ __launch_bounds__(CR_THREADS) void cfg_rescale_rows_kernel(const ds_cfg_rescale_rows_params p) {
    __shared__ double red[2][2][CR_WAVES];
    const int r = blockIdx.x;
    const int32_t* ir = p.irow + (size_t)r * DS_CR_NI;
    const float* fr = p.frow + (size_t)r * DS_CR_NF;
    const int ur = ir[DS_CR_U], cr = ir[DS_CR_C], orow = ir[DS_CR_OUT];
    const float scale = fr[DS_CR_SCALE], phi = fr[DS_CR_PHI];
    const bool bad = ur < 0 || ur >= p.Beps || cr < 0 || cr >= p.Beps || !(phi >= 0.f && phi <= 1.f);
    float g = __builtin_nanf("");
    if (orow >= 0 && orow < p.Beps) {                   // (block-uniform, like bad)
        float* out = p.eps + (size_t)orow * p.CHW;
        if (bad) nan_row(out, nullptr, p.CHW, (int)threadIdx.x, CR_THREADS);
        else
            g = cfg_rescale_row(p.eps + (size_t)ur * p.CHW, p.eps + (size_t)cr * p.CHW, out, p.CHW, scale, phi, red);
    }
    if (p.gain && threadIdx.x == 0) p.gain[r] = g;
}

// ------------------------------------------------------------------------------------------------ multi-prompt guidance
// out = g e with acc = sum_k a_k(j) (c_k - u), p = u + acc, e = u + S acc and g = phi std(p) / std(e) + (1 - phi) over one row
// (include/diffusynth_hip.h: ds_cfg_compose).  cfg_rescale_row's structure: one block of CR_THREADS per row, piece v belongs to thread
// v % CR_THREADS in the 16-byte and in the scalar form alike, float64 sums in two passes about the mean.  The row's weight table
// ([K][wtw], wtw in {1, W}) is staged in LDS once.  cfg_compose_kernel and cfg_compose_rows_kernel both run cfg_compose_row.
struct cc_row {
    const float* u; const float* c0; float* out;        // c_k (k = 1 ... K) at c0 + (k - 1) * cstride
    long long cstride;                                  // in elements
    int K, wtw;
    float scale, phi;
};
#pragma clang fp contract(off)
// p and e of the piece at element i0 (n of its 4 elements are inside the row); wl: the row's weight table in LDS
__device__ __forceinline__ void cc_piece(const cc_row& a, const float* wl, int W, int i0, int n, bool vec, float (&p)[4], float (&e)[4]) {
    float uv[4], cv[DS_CC_MAXK][4], acc[4] = {};
    cr_load(a.u, i0, n, vec, uv);
#pragma unroll
    for (int k = 0; k < DS_CC_MAXK; ++k)
        if (k < a.K) cr_load(a.c0 + k * a.cstride, i0, n, vec, cv[k]);       // (block-uniform; every load is issued before the first use)
    const int j0 = a.wtw == 1 ? 0 : i0 % W;
#pragma unroll
    for (int k = 0; k < DS_CC_MAXK; ++k)
        if (k < a.K) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int j = 0;
                if (a.wtw != 1) {
                    j = j0 + q;
                    if (j >= W) j %= W;                 // (scalar form only: a piece may cross an image row)
                }
                const float d = cv[k][q] - uv[q];
                const float t = wl[k * a.wtw + j] * d;
                acc[q] = k == 0 ? t : acc[q] + t;
            }
        }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        p[q] = uv[q] + acc[q];
        const float sa = a.scale * acc[q];
        e[q] = uv[q] + sa;
    }
}
// multi-prompt guidance: (p, e) of cc_piece; the row of phi == 0 is multiplied by nothing
struct cc_pieces {
    const cc_row& a; const float* wl;
    int W;
    static constexpr bool UNIT_GAIN_MULTIPLIES = false;
    __device__ __forceinline__ void operator()(int i0, int n, bool vec, float (&p)[4], float (&e)[4]) const { cc_piece(a, wl, W, i0, n, vec, p, e); }
};
__device__ __forceinline__ float cfg_compose_row(const cc_row& a, const float* wt, float* wl, int N, int W, double (&red)[2][2][CR_WAVES]) {
    for (int i = threadIdx.x; i < a.K * a.wtw; i += CR_THREADS) wl[i] = wt[i];
    __syncthreads();
    uint64_t addr = (uint64_t)a.u | (uint64_t)a.out;
    for (int k = 0; k < a.K; ++k) addr |= (uint64_t)(a.c0 + k * a.cstride);
    const bool vec = W % 4 == 0 && (addr & 15) == 0;    // (N % W == 0: with W % 4 == 0 every piece is whole and inside one image row)
    return gain_row(cc_pieces{a, wl, W}, a.out, N, vec, a.phi, red);
}
#pragma clang fp contract(fast)

// grid: one block per sample
__global__ __launch_bounds__(CR_THREADS) void cfg_compose_kernel(const ds_cfg_compose_params p) {
    __shared__ double red[2][2][CR_WAVES];
    __shared__ float wl[DS_CC_MAXK * DS_CC_MAXW];
    const size_t off = (size_t)blockIdx.x * p.CHW;
    const cc_row a = {p.eps_u + off, p.eps_c + off, p.out + off, (long long)p.B * p.CHW, p.K, p.wt_w, p.cfg_scale, p.phi};
    const float g = cfg_compose_row(a, p.wt, wl, p.CHW, p.W, red);
    if (p.gain && threadIdx.x == 0) p.gain[blockIdx.x] = g;
}

// grid: one block per table row.  The table is the host's: a malformed row reads nothing (see ds_cfg_compose_rows)
__global__ __launch_bounds__(CR_THREADS) void cfg_compose_rows_kernel(const ds_cfg_compose_rows_params p) {
    __shared__ double red[2][2][CR_WAVES];
    __shared__ float wl[DS_CC_MAXK * DS_CC_MAXW];
    const int r = blockIdx.x;
    const int32_t* ir = p.irow + (size_t)r * DS_CC_NI;
    const float* fr = p.frow + (size_t)r * DS_CC_NF;
    const int ur = ir[DS_CC_U], orow = ir[DS_CC_OUT], K = ir[DS_CC_K], c0 = ir[DS_CC_C0], cs = ir[DS_CC_CSTRIDE];
    const int wo = ir[DS_CC_WT], ww = ir[DS_CC_WTW];
    const float scale = fr[DS_CC_SCALE], phi = fr[DS_CC_PHI];
    bool bad = ur < 0 || ur >= p.Beps || K < 1 || K > DS_CC_MAXK || c0 < 0 || c0 >= p.Beps || (ww != 1 && ww != p.W) || ww > DS_CC_MAXW ||
               wo < 0 || !(phi >= 0.f && phi <= 1.f);
    if (!bad) {                                         // (K and ww are small here: no overflow)
        const long long last = (long long)c0 + (long long)(K - 1) * cs;       // the rows of c_1 ... c_K lie between c0 and last
        bad = last < 0 || last >= p.Beps || (long long)wo + K * ww > p.n_wt;
    }
    float g = __builtin_nanf("");
    if (orow >= 0 && orow < p.Beps) {                   // (block-uniform, like bad)
        float* out = p.eps + (size_t)orow * p.CHW;
        if (bad) {
            nan_row(out, nullptr, p.CHW, (int)threadIdx.x, CR_THREADS);
        } else {
            const cc_row a = {p.eps + (size_t)ur * p.CHW, p.eps + (size_t)c0 * p.CHW, out, (long long)cs * p.CHW, K, ww, scale, phi};
            g = cfg_compose_row(a, p.wt + wo, wl, p.CHW, p.W, red);
        }
    }
    if (p.gain && threadIdx.x == 0) p.gain[r] = g;
}

// grid (x: pieces of a row, y: pair)
template <int V>
__global__ __launch_bounds__(256) void copy_rows_kernel(float* buf, const int32_t* pairs, int CHW, int Bbuf) {
    const int s = pairs[2 * blockIdx.y], d = pairs[2 * blockIdx.y + 1];
    if (s < 0 || s >= Bbuf || d < 0 || d >= Bbuf || s == d) return;
    const float* src = buf + (size_t)s * CHW;
    float* dst = buf + (size_t)d * CHW;
    DS_FOR_PIECES(V, CHW, i0) {
        float t[V];
        load_v<V>(src + i0, true, t);
        store_v<V>(dst + i0, true, t);
    }
}

__global__ void gather_cols_kernel(const float* src, int src_w, const int32_t* cols, int out_w, float* out, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / out_w;
        const int j = i % out_w;
        out[i] = src[row * src_w + cols[j]];
    }
}

// ------------------------------------------------------------------------------------------------ launchers of the step kernels
// the blend operands of a call form (P: ds_step_params / ds_dpm_step_params)
template <class P>
int check_blend(const P* p, const char* name) {
    DS_REQUIRE(p->blend_mode >= 0 && p->blend_mode <= 2, "%s: blend_mode %d", name, p->blend_mode);
    DS_REQUIRE(p->blend_mode == 0 || (p->guide && p->mask), "%s: blend needs guide and mask", name);
    DS_REQUIRE(p->blend_mode != 1 || (p->init_noise && p->qcoef), "%s: blend 1 needs init_noise and qcoef", name);
    return DS_OK;
}
// both rows forms: the solver form takes hrow and no column table
template <bool SOLVER>
int launch_step_rows(const ds_step_rows_params* p, const uint64_t* hrow, void* stream, const char* name) {
    DS_REQUIRE(p && p->x && p->eps && p->out && p->irow && p->frow && p->prow && (!SOLVER || hrow), "%s: null pointer", name);
    DS_REQUIRE_ROW_SIZES(name, p, R, C, H, W);
    if constexpr (SOLVER) {
        DS_REQUIRE(p->Bx > 0 && p->Beps > 0 && p->Bout > 0, "%s: bad row counts (Bx=%d Beps=%d Bout=%d)", name, p->Bx, p->Beps, p->Bout);
    } else {
        DS_REQUIRE(p->Bx > 0 && p->Beps > 0 && p->Bout > 0 && p->n_cols >= 0, "%s: bad row counts (Bx=%d Beps=%d Bout=%d n_cols=%d)", name,
                   p->Bx, p->Beps, p->Bout, p->n_cols);
        DS_REQUIRE(p->n_cols == 0 || p->cols, "%s: n_cols > 0 needs cols", name);
    }
    const bool vec = p->W % 4 == 0 && ds_aligned16(p->x) && ds_aligned16(p->eps) && ds_aligned16(p->out);
    const size_t CHW = (size_t)p->C * p->H * p->W;
    if constexpr (SOLVER) DS_LAUNCH_ROWS(dpm_step_rows_kernel, name, vec, CHW, p->R, stream, *p, hrow);
    else DS_LAUNCH_ROWS(step_rows_kernel, name, vec, CHW, p->R, stream, *p);
    return DS_OK;
}

}  // namespace

extern "C" int ds_ddim_step(const ds_step_params* p, void* stream) {
    DS_REQUIRE(p && p->x && p->eps && p->noise && p->out && p->coef, "ddim_step: null pointer");
    DS_REQUIRE(p->B > 0 && p->CHW > 0 && p->HW > 0 && p->CHW % p->HW == 0, "ddim_step: bad sizes");
    if (const int rc = check_blend(p, "ddim_step")) return rc;
    // 16-byte pieces: with HW % 4 == 0 (and CHW a multiple of HW) every sample's row is aligned as the buffer is and a piece never
    // crosses a mask plane.  (NULL is 16-byte aligned: an operand that is not given does not decide the path.)  The blend operands
    // are looked at per row
    const bool vec = p->HW % 4 == 0 && ds_aligned16(p->x) && ds_aligned16(p->eps) && ds_aligned16(p->eps_cond) && ds_aligned16(p->noise) &&
                     ds_aligned16(p->out);
    DS_LAUNCH_ROWS(ddim_step_kernel, "ddim_step", vec, (size_t)p->CHW, p->B < 65535 ? p->B : 65535, stream, *p);
    return DS_OK;
}

extern "C" int ds_step_rows(const ds_step_rows_params* p, void* stream) { return launch_step_rows<false>(p, nullptr, stream, "step_rows"); }

extern "C" int ds_dpm_step(const ds_dpm_step_params* p, void* stream) {
    DS_REQUIRE(p && p->x && p->eps && p->out && p->coef, "dpm_step: null pointer");
    DS_REQUIRE_ROW_SIZES("dpm_step", p, B, C, H, W);
    if (const int rc = check_blend(p, "dpm_step")) return rc;
    // (NULL is 16-byte aligned: an operand that is not given does not decide the path)
    const bool vec = p->W % 4 == 0 && ds_aligned16(p->x) && ds_aligned16(p->eps) && ds_aligned16(p->eps_cond) && ds_aligned16(p->hist) &&
                     ds_aligned16(p->out) && ds_aligned16(p->guide) && ds_aligned16(p->init_noise) && ds_aligned16(p->mask);
    DS_LAUNCH_ROWS(dpm_step_kernel, "dpm_step", vec, (size_t)p->C * p->H * p->W, p->B, stream, *p);
    return DS_OK;
}

extern "C" int ds_dpm_step_rows(const ds_step_rows_params* p, const uint64_t* hrow, void* stream) {
    return launch_step_rows<true>(p, hrow, stream, "dpm_step_rows");
}

extern "C" int ds_q_sample_rows(const ds_q_sample_rows_params* p, void* stream) {
    DS_REQUIRE(p && p->x0 && p->out && p->irow && p->frow && p->prow, "q_sample_rows: null pointer");
    DS_REQUIRE_ROW_SIZES("q_sample_rows", p, R, C, H, W);
    DS_REQUIRE(p->Bx0 > 0 && p->Bout > 0 && p->n_cols >= 0, "q_sample_rows: bad row counts (Bx0=%d Bout=%d n_cols=%d)", p->Bx0, p->Bout, p->n_cols);
    DS_REQUIRE(p->n_cols == 0 || p->cols, "q_sample_rows: n_cols > 0 needs cols");
    const bool vec = p->W % 4 == 0 && ds_aligned16(p->x0) && ds_aligned16(p->out);
    DS_LAUNCH_ROWS(q_sample_rows_kernel, "q_sample_rows", vec, (size_t)p->C * p->H * p->W, p->R, stream, *p);
    return DS_OK;
}

extern "C" int ds_edit_noise_rows(const ds_edit_noise_rows_params* p, void* stream) {
    DS_REQUIRE(p && p->X && p->eps && p->z && p->irow && p->frow && p->prow, "edit_noise_rows: null pointer");
    DS_REQUIRE_ROW_SIZES("edit_noise_rows", p, R, C, H, W);
    DS_REQUIRE(p->Bx > 0 && p->Beps > 0 && p->Bz > 0, "edit_noise_rows: bad row counts (Bx=%d Beps=%d Bz=%d)", p->Bx, p->Beps, p->Bz);
    const bool vec = p->W % 4 == 0 && ds_aligned16(p->X) && ds_aligned16(p->eps) && ds_aligned16(p->z);
    DS_LAUNCH_ROWS(edit_noise_rows_kernel, "edit_noise_rows", vec, (size_t)p->C * p->H * p->W, p->R, stream, *p);
    return DS_OK;
}

extern "C" int ds_cfg_rescale(const ds_cfg_rescale_params* p, void* stream) {
    DS_REQUIRE(p && p->eps_u && p->eps_c && p->out, "cfg_rescale: null pointer");
    DS_REQUIRE(p->B > 0 && p->CHW > 0 && p->CHW <= (1 << 30), "cfg_rescale: bad sizes (B=%d CHW=%d)", p->B, p->CHW);
    DS_REQUIRE(p->phi >= 0.f && p->phi <= 1.f, "cfg_rescale: phi %g is not in [0, 1]", (double)p->phi);
    hipLaunchKernelGGL(cfg_rescale_kernel, dim3((unsigned)p->B), dim3(CR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *p);
    DS_CHECK_LAUNCH("cfg_rescale");
    return DS_OK;
}

extern "C" int ds_cfg_rescale_rows(const ds_cfg_rescale_rows_params* p, void* stream) {
    DS_REQUIRE(p && p->eps && p->irow && p->frow, "cfg_rescale_rows: null pointer");
    DS_REQUIRE(p->R > 0 && p->CHW > 0 && p->CHW <= (1 << 30) && p->Beps > 0, "cfg_rescale_rows: bad sizes (R=%d CHW=%d Beps=%d)", p->R, p->CHW,
               p->Beps);
    hipLaunchKernelGGL(cfg_rescale_rows_kernel, dim3((unsigned)p->R), dim3(CR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *p);
    DS_CHECK_LAUNCH("cfg_rescale_rows");
    return DS_OK;
}

extern "C" int ds_cfg_compose(const ds_cfg_compose_params* p, void* stream) {
    DS_REQUIRE(p && p->eps_u && p->eps_c && p->wt && p->out, "cfg_compose: null pointer");
    DS_REQUIRE(p->B > 0 && p->CHW > 0 && p->CHW <= (1 << 30) && p->W > 0 && p->CHW % p->W == 0, "cfg_compose: bad sizes (B=%d CHW=%d W=%d)", p->B,
               p->CHW, p->W);
    DS_REQUIRE(p->K >= 1 && p->K <= DS_CC_MAXK, "cfg_compose: K %d is not in [1, %d]", p->K, DS_CC_MAXK);
    DS_REQUIRE(p->wt_w == 1 || (p->wt_w == p->W && p->W <= DS_CC_MAXW), "cfg_compose: wt_w %d is neither 1 nor W=%d (at most %d)", p->wt_w, p->W,
               DS_CC_MAXW);
    DS_REQUIRE(p->phi >= 0.f && p->phi <= 1.f, "cfg_compose: phi %g is not in [0, 1]", (double)p->phi);
    hipLaunchKernelGGL(cfg_compose_kernel, dim3((unsigned)p->B), dim3(CR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *p);
    DS_CHECK_LAUNCH("cfg_compose");
    return DS_OK;
}

extern "C" int ds_cfg_compose_rows(const ds_cfg_compose_rows_params* p, void* stream) {
    DS_REQUIRE(p && p->eps && p->irow && p->frow && p->wt, "cfg_compose_rows: null pointer");
    DS_REQUIRE(p->R > 0 && p->CHW > 0 && p->CHW <= (1 << 30) && p->W > 0 && p->CHW % p->W == 0 && p->Beps > 0 && p->n_wt > 0,
               "cfg_compose_rows: bad sizes (R=%d CHW=%d W=%d Beps=%d n_wt=%d)", p->R, p->CHW, p->W, p->Beps, p->n_wt);
    hipLaunchKernelGGL(cfg_compose_rows_kernel, dim3((unsigned)p->R), dim3(CR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *p);
    DS_CHECK_LAUNCH("cfg_compose_rows");
    return DS_OK;
}

extern "C" int ds_copy_rows(float* buf, const int32_t* pairs, int R, int CHW, int Bbuf, void* stream) {
    DS_REQUIRE(buf && pairs, "copy_rows: null pointer");
    DS_REQUIRE(R > 0 && R <= 65535 && CHW > 0 && Bbuf > 0, "copy_rows: bad sizes (R=%d CHW=%d Bbuf=%d)", R, CHW, Bbuf);
    const bool vec = CHW % 4 == 0 && ds_aligned16(buf);
    DS_LAUNCH_ROWS(copy_rows_kernel, "copy_rows", vec, (size_t)CHW, R, stream, buf, pairs, CHW, Bbuf);
    return DS_OK;
}

extern "C" int ds_philox_normal(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream) {
    DS_REQUIRE(out && n > 0, "philox_normal: bad args");
    hipLaunchKernelGGL(philox_normal_kernel, dim3(blocks_for((n + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), out, n, seed, offset);
    DS_CHECK_LAUNCH("philox_normal");
    return DS_OK;
}

extern "C" int ds_gather_cols(const float* src, int rows, int src_w, const int32_t* cols, int out_w, float* out, void* stream) {
    DS_REQUIRE(src && cols && out && rows > 0 && src_w > 0 && out_w > 0, "gather_cols: bad args");
    const size_t total = (size_t)rows * out_w;
    hipLaunchKernelGGL(gather_cols_kernel, dim3(blocks_for(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, src_w, cols, out_w, out, total);
    DS_CHECK_LAUNCH("gather_cols");
    return DS_OK;
}
