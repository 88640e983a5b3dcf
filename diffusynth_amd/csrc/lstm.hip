// LSTM layer of the timbre encoder (model/timbre_encoder_pretrain.py:39,71: nn.LSTM(feature, hidden, num_layers, batch_first=True)) and the
// classifier heads' log-softmax / sigmoid (:81-84).  fp32 throughout.
//
// ds_lstm_layer enqueues ONE launch per time step on the caller's stream: stream order is the only dependence between steps (and between
// layers), no block ever waits for another inside a kernel.  A block owns 16 hidden units with all four of their gates and one tile of 16
// samples: wave g multiplies h_{t-1} of the tile by the 16 rows of gate g (fp32 MFMA 16x16x4, the operand layout of linear_mfma_kernel in
// misc.hip), the four 16 x 16 gate tiles meet in LDS, and the block's 256 threads finish the cell: one (sample, unit) each.  c is read and
// written by that one thread only (in place); h goes through two buffers, since every block of a step reads all of h_{t-1}.
// The summation order over k of an output (b, unit) is a function of H alone: a row's result does not depend on what shares the batch
// with it.
#include "common.hpp"

namespace {

constexpr int KU = 8;       // 16-deep k steps whose loads are in flight together
constexpr int GP = 17;     // LDS pitch of a gate tile row (16 units + 1: the column reads of the cell update spread over the banks)

__device__ __forceinline__ float sigmoid_acc(float v) { return 1.0f / (1.0f + expf(-v)); }

// grid (H / 16, ceil(B / 16)), 256 threads.  first: step 0 (h_{t-1} = c = 0: neither is read).  pre: row t of every sample, batch stride pre_bs.
__global__ __launch_bounds__(256) void lstm_step_kernel(const float* pre, long pre_bs, const float* w_hh, const float* h_prev, float* c, float* h_out,
                                                        float* hs, long hs_bs, float* h_last, int B, int H, int first) {
    __shared__ float gates[4][16][GP];
    const int g = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
    const int n = lane & 15, kq = lane >> 4;
    if (!first) {
        const float* wr = w_hh + ((size_t)g * H + u0 + n) * H + 4 * kq;              // row of gate g, unit u0 + n (H % 16 == 0: in range)
        const float* xr = h_prev + (size_t)min(b0 + n, B - 1) * H + 4 * kq;          // sample b0 + n, clamped (its results are not stored)
        // 128 k per trip with all sixteen loads requested before the first MFMA (as a plain 16-deep loop every trip paid one memory round
        // trip: load -> s_waitcnt -> 4 MFMA), then the rest in 16-deep trips.  Four accumulators, the 16-deep step q of a trip into number
        // q % 4 and the rest into number 0: four independent MFMA chains instead of one of H / 4 dependent instructions, and each sum a
        // quarter as long.  The assignment of k to chains is a function of H alone, never of the batch.
        f32x4 acc[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
        int k0 = 0;
        for (; k0 + KU * 16 <= H; k0 += KU * 16) {
            f32x4 wv[KU], xv[KU];
#pragma unroll
            for (int q = 0; q < KU; ++q) {
                wv[q] = *reinterpret_cast<const f32x4*>(wr + k0 + 16 * q);
                xv[q] = *reinterpret_cast<const f32x4*>(xr + k0 + 16 * q);
            }
#pragma unroll
            for (int q = 0; q < KU; ++q)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[q & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[q][s], wv[q][s], acc[q & 3], 0, 0, 0);
        }
        for (; k0 < H; k0 += 16) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k0);
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + k0);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s], wv[s], acc[0], 0, 0, 0);
        }
        const f32x4 sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
        for (int r = 0; r < 4; ++r) gates[g][kq * 4 + r][n] = sum[r];                // sample kq * 4 + r, unit n
        __syncthreads();
    }
    const int s = threadIdx.x >> 4, j = threadIdx.x & 15, b = b0 + s, u = u0 + j;
    if (b >= B) return;
    const float* pr = pre + (size_t)b * pre_bs + u;
    float zi = pr[0], zf = pr[H], zg = pr[2 * (size_t)H], zo = pr[3 * (size_t)H];
    float cv = 0.f;
    if (!first) {
        zi += gates[0][s][j];
        zf += gates[1][s][j];
        zg += gates[2][s][j];
        zo += gates[3][s][j];
        cv = c[(size_t)b * H + u];
    }
    cv = sigmoid_acc(zf) * cv + sigmoid_acc(zi) * tanhf(zg);
    const float hv = sigmoid_acc(zo) * tanhf(cv);
    c[(size_t)b * H + u] = cv;
    h_out[(size_t)b * H + u] = hv;
    if (hs) hs[(size_t)b * hs_bs + u] = hv;
    if (h_last) h_last[(size_t)b * H + u] = hv;
}

// one block per (row, range): log-softmax over ranges 0 .. 2, sigmoid over range 3, in place
__global__ __launch_bounds__(256) void timbre_heads_kernel(float* y, int ys, int n0, int n1, int n2, int n3) {
    __shared__ float red[4];
    const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = r == 0 ? 0 : r == 1 ? n0 : r == 2 ? n0 + n1 : n0 + n1 + n2;
    const int len = r == 0 ? n0 : r == 1 ? n1 : r == 2 ? n2 : n3;
    float* row = y + (size_t)blockIdx.x * ys + lo;
    if (r == 3) {
        for (int i = tid; i < len; i += 256) row[i] = sigmoid_acc(row[i]);
        return;
    }
    float m = -INFINITY;
    for (int i = tid; i < len; i += 256) m = fmaxf(m, row[i]);
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int i = tid; i < len; i += 256) sum += expf(row[i] - m);
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    const float lse = m + logf((red[0] + red[1]) + (red[2] + red[3]));
    for (int i = tid; i < len; i += 256) row[i] -= lse;
}

}  // namespace

extern "C" size_t ds_lstm_ws_floats(int B, int H) { return B > 0 && H > 0 ? (size_t)3 * B * H : 0; }

extern "C" int ds_lstm_layer(const float* pre, long long pre_batch_stride, long long pre_step_stride, const float* w_hh, int B, int T, int H,
                             float* hs, float* h_last, float* ws, void* stream) {
    DS_REQUIRE(pre && w_hh && h_last && ws && B > 0 && T > 0 && H > 0, "lstm_layer: bad args");
    DS_REQUIRE(H % 16 == 0, "lstm_layer: H=%d unsupported (H %% 16 == 0)", H);
    DS_REQUIRE(pre_step_stride >= 4LL * H && pre_batch_stride >= 4LL * H, "lstm_layer: pre strides (%lld, %lld) below 4H", pre_batch_stride,
               pre_step_stride);
    DS_REQUIRE((B + 15) / 16 <= 65535, "lstm_layer: B=%d too large", B);
    if (!ds_aligned16(w_hh) || !ds_aligned16(ws)) DS_FAIL(DS_EALIGN, "lstm_layer: w_hh and ws must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t bh = (size_t)B * H;
    float* c = ws;
    float* hbuf[2] = {ws + bh, ws + 2 * bh};
    const dim3 grid(H / 16, (B + 15) / 16), blk(256);
    for (int t = 0; t < T; ++t) {
        hipLaunchKernelGGL(lstm_step_kernel, grid, blk, 0, st, pre + (size_t)t * pre_step_stride, (long)pre_batch_stride, w_hh, hbuf[(t + 1) & 1], c,
                           hbuf[t & 1], hs ? hs + (size_t)t * H : nullptr, (long)T * H, t == T - 1 ? h_last : nullptr, B, H, t == 0 ? 1 : 0);
        DS_CHECK_LAUNCH("lstm_step");
    }
    return DS_OK;
}

extern "C" int ds_timbre_heads(float* y, int y_stride, int B, int n0, int n1, int n2, int n3, void* stream) {
    DS_REQUIRE(y && B > 0 && n0 > 0 && n1 > 0 && n2 > 0 && n3 > 0, "timbre_heads: bad args");
    DS_REQUIRE((long long)n0 + n1 + n2 + n3 <= y_stride, "timbre_heads: %d + %d + %d + %d columns in rows of %d", n0, n1, n2, n3, y_stride);
    hipLaunchKernelGGL(timbre_heads_kernel, dim3(B, 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), y, y_stride, n0, n1, n2, n3);
    DS_CHECK_LAUNCH("timbre_heads");
    return DS_OK;
}
