// CLAP's text tower (a RoBERTa-base encoder, its first-token pooler and CLAP's two-layer projection): the three kinds of launch that
// ds_linear / ds_add_layernorm / ds_activation do not cover.  fp32 throughout, plain FMA and the accurate expf / tanhf: a prompt is 5 - 30
// tokens against 500 MB of weights, so the arithmetic is free and what counts is accuracy and a summation order that is fixed.
//
//   ds_text_embed       LayerNorm(word[id] + pos[position id] + type0) per token, RoBERTa's position rule computed from input_ids
//   ds_text_attention   softmax_k(q . k d^-0.5 + mask_k) v per (sample, head, query), bidirectional, from the stacked [B S][3H] q|k|v rows
//   ds_text_tail        the pooler's tanh, the projection's ReLU, and x / max(||x||_2, eps) per row
#include "common.hpp"
#include "norm_parts.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ embeddings
// one block per token.  Position id: pad + (number of non-pad tokens up to and including this one), pad for a pad token; a function of
// input_ids alone.  The LayerNorm is add_layernorm_kernel's (misc.hip), layernorm_row: two passes, double partial sums, a tree over the 256 threads.
// A row's bits depend on its own ids up to s only, never on S or B.
__global__ __launch_bounds__(256) void text_embed_kernel(const int64_t* ids, int S, int pad, const float* word, int V, const float* pos, int P,
                                                         const float* type0, const float* gamma, const float* beta, int H, float eps, float* out) {
    __shared__ double red[256];
    __shared__ int cnt[256];
    const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    const int64_t* row = ids + (size_t)b * S;
    int c = 0;
    for (int i = tid; i <= s; i += 256) c += row[i] != pad;
    block_tree_sum256(cnt, c);
    const int64_t id = row[s];
    const int pid = id != pad ? pad + cnt[0] : pad;
    float* ob = out + ((size_t)b * S + s) * H;
    if (id < 0 || id >= V || pid < 0 || pid >= P) {          // a table bug shows in the result; nothing is read out of bounds
        for (int i = tid; i < H; i += 256) ob[i] = __builtin_nanf("");
        return;
    }
    const float* wr = word + (size_t)id * H;
    const float* pr = pos + (size_t)pid * H;
    __syncthreads();
    layernorm_row([&](int i) { return (wr[i] + pr[i]) + type0[i]; }, H, gamma, beta, eps, ob, red);
}

// ------------------------------------------------------------------------------------------------ attention
constexpr int KC = 64;        // keys per staged chunk: key k lives in chunk k / 64 and belongs to lane k % 64
constexpr int QT = 8;         // queries per block, two per wave
constexpr int QPW = 2;
constexpr int DMAX = 128;     // head size limit
constexpr int SMAX = 512;     // sequence limit: a query's scores stay in LDS (QT x 2 KB)

// grid (ceil(S / QT), heads, B), 256 threads.  K and V of a head do not fit the LDS at S = 512 (256 KB at d = 64), so they pass through
// one 64-key buffer: first every K chunk (scores into LDS), then max and exp per query, then every V chunk.
//
// Why a query's output does not depend on S or on the batch, as long as the extra keys are masked:
//   - the score of (query, key) is one fmaf chain over the head's d elements in index order: it sees neither S nor B;
//   - the maximum runs over unmasked keys only (a masked or absent key enters as -inf), and a maximum has the same bits in any order;
//   - key k adds its exp to the running sum of lane k % 64 in chunk order k / 64, and the 64 lanes are added by wave_sum's fixed tree.  A masked
//     key adds exactly +0.0 and an absent key leaves the lane's +0.0 start alone; p >= 0, so x + 0.0 == x bit for bit;
//   - the output element is one fmaf chain over the keys in index order; a masked key contributes fmaf(0, v, acc) == acc (v is a finite
//     number: the value row of a real, if padded, token), and keys behind S are never visited.
// Nothing else (block shape, chunk size, lane mapping) is chosen from S or B.
__global__ __launch_bounds__(256) void text_attention_kernel(const float* qkv, const void* mask, int mask_bytes, int S, int heads, int d, float scale,
                                                             float* ctx) {
    __shared__ float kv[KC * (DMAX + 1)];
    __shared__ float qs[QT][DMAX];
    __shared__ float sc[QT][SMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * QT;
    const int H = heads * d, pitch = d + 1;                      // odd pitch: the 64 key rows of a chunk start in 64 different banks
    const size_t rs = 3 * (size_t)H;
    const float* base = qkv + (size_t)b * S * rs + (size_t)h * d;
    const int nch = (S + KC - 1) / KC;
    for (int i = tid; i < QT * d; i += 256) {
        const int qi = i / d, dd = i - qi * d;
        qs[qi][dd] = q0 + qi < S ? base[(size_t)(q0 + qi) * rs + dd] : 0.f;
    }
    float mx[QPW];
#pragma unroll
    for (int j = 0; j < QPW; ++j) mx[j] = -INFINITY;
    for (int c = 0; c < nch; ++c) {
        __syncthreads();                                         // the previous chunk has been read (first trip: qs is written)
        for (int i = tid; i < KC * d; i += 256) {
            const int key = i / d, dd = i - key * d, k = c * KC + key;
            kv[key * pitch + dd] = k < S ? base[(size_t)k * rs + H + dd] : 0.f;
        }
        __syncthreads();
        const int k = c * KC + lane;
        bool live = k < S;
        if (live && mask) live = mask_bytes == 1 ? static_cast<const unsigned char*>(mask)[(size_t)b * S + k] != 0
                                                 : static_cast<const int32_t*>(mask)[(size_t)b * S + k] != 0;
#pragma unroll
        for (int j = 0; j < QPW; ++j) {
            const int qi = wave * QPW + j;
            if (q0 + qi >= S) continue;                          // wave-uniform
            float acc = 0.f;
            for (int dd = 0; dd < d; ++dd) acc = fmaf(qs[qi][dd], kv[lane * pitch + dd], acc);
            const float sv = live ? acc * scale : -INFINITY;
            sc[qi][k] = sv;
            mx[j] = fmaxf(mx[j], sv);
        }
    }
    float sum[QPW];
#pragma unroll
    for (int j = 0; j < QPW; ++j) {
        const int qi = wave * QPW + j;
        sum[j] = 0.f;
        if (q0 + qi >= S) continue;
        const float m = wave_max(mx[j]);
        float part = 0.f;
        for (int c = 0; c < nch; ++c) {                          // the wave reads back what its own lanes wrote
            const float sv = sc[qi][c * KC + lane];
            const float p = sv == -INFINITY ? 0.f : expf(sv - m);
            part += p;
            sc[qi][c * KC + lane] = p;
        }
        sum[j] = wave_sum(part);
    }
    float acc[QPW][2];
#pragma unroll
    for (int j = 0; j < QPW; ++j) acc[j][0] = acc[j][1] = 0.f;
    for (int c = 0; c < nch; ++c) {
        __syncthreads();                                         // K (or the previous V chunk) has been read; every p is written
        for (int i = tid; i < KC * d; i += 256) {
            const int key = i / d, dd = i - key * d, k = c * KC + key;
            kv[key * pitch + dd] = k < S ? base[(size_t)k * rs + 2 * (size_t)H + dd] : 0.f;
        }
        __syncthreads();
        const int kn = min(KC, S - c * KC);
#pragma unroll
        for (int j = 0; j < QPW; ++j) {
            const int qi = wave * QPW + j;
            if (q0 + qi >= S) continue;
            for (int key = 0; key < kn; ++key) {
                const float p = sc[qi][c * KC + key];
                if (lane < d) acc[j][0] = fmaf(p, kv[key * pitch + lane], acc[j][0]);
                if (lane + 64 < d) acc[j][1] = fmaf(p, kv[key * pitch + lane + 64], acc[j][1]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < QPW; ++j) {
        const int q = q0 + wave * QPW + j;
        if (q >= S) continue;
        float* o = ctx + ((size_t)b * S + q) * H + (size_t)h * d;
        if (lane < d) o[lane] = sum[j] > 0.f ? acc[j][0] / sum[j] : 0.f;            // every key masked: zeros
        if (lane + 64 < d) o[lane + 64] = sum[j] > 0.f ? acc[j][1] / sum[j] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ tail
__global__ __launch_bounds__(256) void text_tail_map_kernel(const float* x, size_t n, int op, float* out) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = op == DS_TAIL_TANH ? tanhf(x[i]) : fmaxf(x[i], 0.0f);
}

// one block per row: out = x / max(||x||_2, eps), the squares summed in double by a fixed tree
__global__ __launch_bounds__(256) void text_l2_normalize_kernel(const float* x, int D, float eps, float* out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const float* xr = x + (size_t)blockIdx.x * D;
    double q = 0.0;
    for (int i = tid; i < D; i += 256) q += (double)xr[i] * xr[i];
    block_tree_sum256(red, q);
    const float norm = fmaxf((float)sqrt(red[0]), eps);
    for (int i = tid; i < D; i += 256) out[(size_t)blockIdx.x * D + i] = xr[i] / norm;
}

}  // namespace

extern "C" int ds_text_embed(const int64_t* input_ids, int B, int S, int pad_id, const float* word, int V, const float* pos, int P, const float* type0,
                             const float* gamma, const float* beta, int H, float eps, float* out, void* stream) {
    DS_REQUIRE(input_ids && word && pos && type0 && gamma && beta && out, "text_embed: null pointer");
    DS_REQUIRE(B > 0 && B <= 65535 && S > 0 && V > 0 && P > 0 && H > 0, "text_embed: bad sizes B=%d S=%d V=%d P=%d H=%d", B, S, V, P, H);
    DS_REQUIRE(pad_id >= 0 && pad_id < P, "text_embed: pad_id=%d outside the %d positions", pad_id, P);
    hipLaunchKernelGGL(text_embed_kernel, dim3(S, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), input_ids, S, pad_id, word, V, pos, P,
                       type0, gamma, beta, H, eps, out);
    DS_CHECK_LAUNCH("text_embed");
    return DS_OK;
}

extern "C" int ds_text_attention(const float* qkv, const void* mask, int mask_bytes, int B, int S, int heads, int d, float* ctx, void* stream) {
    DS_REQUIRE(qkv && ctx && B > 0 && heads > 0, "text_attention: bad args");
    DS_REQUIRE(S >= 1 && S <= SMAX, "text_attention: S=%d unsupported (1 .. %d)", S, SMAX);
    DS_REQUIRE(d >= 4 && d <= DMAX && d % 4 == 0, "text_attention: d=%d unsupported (a multiple of 4 up to %d)", d, DMAX);
    DS_REQUIRE(!mask || mask_bytes == 1 || mask_bytes == 4, "text_attention: mask_bytes=%d (1: uint8, 4: int32)", mask_bytes);
    DS_REQUIRE(B <= 65535 && heads <= 65535, "text_attention: B=%d or heads=%d too large", B, heads);
    const float scale = (float)(1.0 / sqrt((double)d));
    hipLaunchKernelGGL(text_attention_kernel, dim3((S + QT - 1) / QT, heads, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), qkv, mask,
                       mask_bytes, S, heads, d, scale, ctx);
    DS_CHECK_LAUNCH("text_attention");
    return DS_OK;
}

extern "C" int ds_text_tail(const float* x, int B, int D, int op, float eps, float* out, void* stream) {
    DS_REQUIRE(x && out && B > 0 && D > 0, "text_tail: bad args");
    DS_REQUIRE(op == DS_TAIL_TANH || op == DS_TAIL_RELU || op == DS_TAIL_L2NORM, "text_tail: unknown op %d", op);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (op == DS_TAIL_L2NORM) {
        hipLaunchKernelGGL(text_l2_normalize_kernel, dim3(B), dim3(256), 0, st, x, D, eps, out);
    } else {
        const size_t n = (size_t)B * D, nb = (n + 255) / 256;
        hipLaunchKernelGGL(text_tail_map_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, st, x, n, op, out);
    }
    DS_CHECK_LAUNCH("text_tail");
    return DS_OK;
}
