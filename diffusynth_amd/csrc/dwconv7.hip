// Depthwise 7x7 (+bias +time bias, two-source skip concat) with the GroupNorm partials of its output (gfx950).
// All of these are HBM-bound: 16-byte vector accesses along the channels-last C axis, fp32 math.
#include <type_traits>

#include "common.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ dwconv7
// thread = (channel vector, w, strip of TH rows); a 7-wide column of TH+6 inputs is held in registers per
// horizontal tap so every loaded value feeds up to TH outputs.
constexpr int DW_TH = 4;
constexpr int DW_BLOCK = 256;

// The source the channels from c0 on come from (the skip concat is two sources, the second one shorter and offset): one sample's base, its
// extents, the channel inside it, the offset of its origin in output coordinates and its DS_BOUNDS buffer.  ES = bytes per element.
struct DwSrc { const char* base; int Cs, cc, Hs, Ws, oh, ow, buf; };
template <int ES>
__device__ __forceinline__ DwSrc dw_src(const ds_dwconv_params& p, int b, int c0) {
    if (c0 < p.C0) return {reinterpret_cast<const char*>(p.src0) + (size_t)b * p.H * p.W * p.C0 * ES, p.C0, c0, p.H, p.W, 0, 0, DS_BX_SRC0};
    return {reinterpret_cast<const char*>(p.src1) + (size_t)b * p.H1 * p.W1 * p.C1 * ES, p.C1, c0 - p.C0, p.H1, p.W1, p.off_h1, p.off_w1, DS_BX_SRC1};
}

// One tap column of the stencil for a thread that owns SR consecutive output rows of one channel vector: the column's 7 weights from LDS
// (wcol = the column's first tap at the thread's channels, `pitch` floats from one tap row to the next), then SR + 6 input rows
// (load_row(r, x)), every value feeding up to 7 outputs.  The tile and the strip kernel share it: the same operation order per output.
template <int SR, int V, typename LoadRow>
__device__ __forceinline__ void dw_tap_column(float (&acc)[SR][V], const float* wcol, int pitch, LoadRow load_row) {
    float wv[7][V];
#pragma unroll
    for (int dh = 0; dh < 7; ++dh)
#pragma unroll
        for (int v = 0; v < V; v += 4) {
            const f32x4 t4 = *reinterpret_cast<const f32x4*>(wcol + dh * pitch + v);
            wv[dh][v] = t4[0]; wv[dh][v + 1] = t4[1]; wv[dh][v + 2] = t4[2]; wv[dh][v + 3] = t4[3];
        }
#pragma unroll
    for (int r = 0; r < SR + 6; ++r) {
        float x[V];
        load_row(r, x);
#pragma unroll
        for (int dh = 0; dh < 7; ++dh) {
            const int o = r - dh;
            if (o >= 0 && o < SR) {
#pragma unroll
                for (int v = 0; v < V; ++v) acc[o][v] = fmaf(x[v], wv[dh][v], acc[o][v]);
            }
        }
    }
}

// Stores the channel vector a[] at channel c of output pixel (h, w) of sample b and adds it to the GroupNorm sums s = (sum, sum of squares),
// which it returns.  The direct, the tile and the strip kernel share it: one statistics order.  `split` (fp32 only, the
// split-precision tier): the result as two bf16 planes (hi, then lo = v - hi) of a 2C-channel image, the input format of the split 3x3
// convolution that follows (DS_CONV_F_SPLIT_IN).  (r05 ablation: hi | lo of a block's 32 channels as ONE 128-byte line per pixel instead
// of two 64-byte runs in two planes: no consistent gain, 613 vs 595 and 591 vs 623 us on the two layer shapes tried — the plane layout stays)
// The sums go in and out by value and the row comes as a plain pointer: with reference parameters hipcc pairs the sums differently in
// its SLP pass (other floating-point instructions in the fp32 kernels, so possibly other bits in stats_part).
template <typename T>
__device__ __forceinline__ float2 dw_store_row(const ds_dwconv_params& p, bool split, int b, int h, int w, int C, int c, const float* a, float2 s) {
    if (split) {
        bf16* o2 = reinterpret_cast<bf16*>(p.out) + ((size_t)b * p.H * p.W + (size_t)(h * p.W + w)) * (2 * C) + c;
        uint2 hi, lo;
        ds_split2(a[0], a[1], hi.x, lo.x);
        ds_split2(a[2], a[3], hi.y, lo.y);
        DS_ST(bf16x4, o2, DS_BX_OUT, __builtin_bit_cast(bf16x4, hi));
        DS_ST(bf16x4, o2 + C, DS_BX_OUT, __builtin_bit_cast(bf16x4, lo));
    } else {
        T* outp = reinterpret_cast<T*>(p.out) + (size_t)b * p.H * p.W * C;
        vec16_store<T>(outp + ((size_t)(h * p.W + w) * C + c), a, DS_BX_OUT);
    }
#pragma unroll
    for (int v = 0; v < Vec16<T>::N; ++v) {
        s.x += a[v];
        s.y += a[v] * a[v];
    }
    return s;
}

template <typename T>
__global__ __launch_bounds__(DW_BLOCK) void dwconv7_kernel(const ds_dwconv_params p, int nstrip, int CV) {
    constexpr int V = Vec16<T>::N;
    __shared__ float red[2 * (DW_BLOCK / 64)];
    const int C = p.C0 + p.C1;
    const int b = blockIdx.y;
    const long gid = (long)blockIdx.x * DW_BLOCK + threadIdx.x;
    const long total = (long)nstrip * p.W * CV;
    float2 st = {0.f, 0.f};                                   // the block's GroupNorm sums (sum, sum of squares)
    if (gid < total) {
        const int cv = gid % CV;
        const int w = (gid / CV) % p.W;
        const int strip = gid / ((long)CV * p.W);
        const int h0 = strip * DW_TH;
        const int c = cv * V;
        const DwSrc s = dw_src<sizeof(T)>(p, b, c);
        const T* base = reinterpret_cast<const T*>(s.base);
        float acc[DW_TH][V];
        float init[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            init[v] = p.bias[c + v];
            if (p.tbias) init[v] += p.tbias[(size_t)b * p.tb_stride + c + v];
        }
#pragma unroll
        for (int t = 0; t < DW_TH; ++t)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[t][v] = init[v];

        for (int dw = 0; dw < 7; ++dw) {
            const int wi = w + dw - 3 - s.ow;
            if ((unsigned)wi >= (unsigned)s.Ws) continue;  // zero column
            float col[DW_TH + 6][V];
#pragma unroll
            for (int r = 0; r < DW_TH + 6; ++r) {
                const int hi = h0 + r - 3 - s.oh;
                if ((unsigned)hi < (unsigned)s.Hs) {
                    vec16_load<T>(base + ((size_t)(hi * s.Ws + wi) * s.Cs + s.cc), col[r], s.buf);
                } else {
#pragma unroll
                    for (int v = 0; v < V; ++v) col[r][v] = 0.f;
                }
            }
#pragma unroll
            for (int dh = 0; dh < 7; ++dh) {
                float wv[V];
                const float* wp = p.wt + (size_t)(dh * 7 + dw) * C + c;
#pragma unroll
                for (int v = 0; v < V; v += 4) {
                    f32x4 t4 = DS_LD(f32x4, wp + v, DS_BX_W);
                    wv[v] = t4[0]; wv[v + 1] = t4[1]; wv[v + 2] = t4[2]; wv[v + 3] = t4[3];
                }
#pragma unroll
                for (int t = 0; t < DW_TH; ++t)
#pragma unroll
                    for (int v = 0; v < V; ++v) acc[t][v] = fmaf(col[t + dh][v], wv[v], acc[t][v]);
            }
        }
#pragma unroll
        for (int t = 0; t < DW_TH; ++t)
            if (h0 + t < p.H) st = dw_store_row<T>(p, false, b, h0 + t, w, C, c, acc[t], st);
    }
    if (p.stats_part) block_stats_write(st.x, st.y, red, p.stats_part + ((size_t)b * gridDim.x + blockIdx.x) * 2);
}

// ------------------------------------------------------------------------------------------------ dwconv7, LDS-tiled
// Block = 16 x 32 output pixels x CB channels (CB = 4 x 16-byte vectors: 32 bf16 / 16 fp32 channels).
// The 22 x 38 input halo is staged once in LDS (64 B per pixel, lanes -> consecutive 16-B chunks =>
// conflict-free ds_read_b128), the 49 x CB weights next to it.  Each thread owns one channel vector of an
// 8-row output strip: per horizontal tap it walks 14 input rows, every value feeding up to 7 outputs.
// r03: the tile is 512 pixels in three shapes — 32 x 16, 16 x 32 for images at most 16 wide and 8 x 64 for images at most 8 wide (a 32-wide tile
// spent half / three quarters of its threads on columns outside a 64x16 / 32x8 image: 1.0-1.7 TB/s there against 2.4 on the wide levels).
// NV = 16-byte channel vectors per pixel held in LDS per block.  4 (32 bf16 / 16 fp32 channels, a 512-pixel tile) was the only form until the
// end of r03; fp32 tensors whose channel counts allow it now take NV = 8 (32 channels = one whole 128-byte line per pixel, a 256-pixel tile):
// with 16 channels the kernel moved 64-byte load pieces and 32-byte store pieces and sat at the L2's REQUEST rate (C = 192 at 256x64: 182 M
// requests in 1360 us = 134 G/s with six of its seven tap columns removed, i.e. without its arithmetic) — not at a byte rate.  2 measured slower.
// Output rows per thread of the tile and the strip kernel: per tap column a thread reads 7 weight + 14 input vectors for 8 x 7 outputs
// (38 % fewer LDS reads per output than at 4 rows; the kernels are LDS-bound where they are not HBM-bound).  4 and 16 rows: DESIGN, retired switches.
constexpr int LT_SR = 8;
constexpr int LT_NT = 2048 / LT_SR;                             // threads: channel vectors x tile columns x row strips = NV x (2048 / NV pixels) / LT_SR
template <int TWL, int NV>
struct LT {
    static constexpr int W = 1 << TWL, H = (2048 / NV) >> TWL, HC = W + 6, HR = H + 6, NPX = HC * HR;
};
static int lt_twl(int W, int nv) { return W <= 8 ? 3 : ((W <= 16 || nv == 8) ? 4 : 5); }     // NV = 8: 16 x 16 (8 x 32 for images at most 8 wide)

template <typename T, int TWL, int LT_NV>
__global__ __launch_bounds__(LT_NT) void dwconv7_lds_kernel(const ds_dwconv_params p, int tiles_w, int tiles_hw, int ncblk) {
    constexpr int LT_W = LT<TWL, LT_NV>::W, LT_H = LT<TWL, LT_NV>::H, LT_HC = LT<TWL, LT_NV>::HC, LT_NPX = LT<TWL, LT_NV>::NPX;
    static_assert(LT_NV * LT_W * (LT_H / LT_SR) == LT_NT && LT_H % LT_SR == 0, "thread map");
    constexpr int V = Vec16<T>::N;
    constexpr int CB = LT_NV * V;
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    uint4* xs = reinterpret_cast<uint4*>(dsm);                                          // [LT_NPX][LT_NV]
    float* wsm = reinterpret_cast<float*>(dsm + (size_t)LT_NPX * LT_NV * 16);          // [49][CB]
    float* red = wsm + 49 * CB;
    const int tid = threadIdx.x;
    // Block order: channel block fastest, then the tile, then the sample (plain hardware order).  The XCD-chunked order of the 3x3 kernels
    // (a plane's tiles consecutive on ONE XCD, for the halo rows / columns they share) measured slower (DESIGN, retired switches): a plane's
    // tiles then stream from the same few HBM channels at once; the plain order spreads every moment's requests over all of them, and this
    // kernel is bound by bytes in flight, not by bytes.
    const int wid = blockIdx.x + gridDim.x * blockIdx.y;
    const int cblk = wid % ncblk, tile = (wid / ncblk) % tiles_hw, b = wid / (tiles_hw * ncblk);
    const int bix = tile * ncblk + cblk;                      // (the block's slot in its sample's statistics partials: order-independent sum)
    const int th = tile / tiles_w, tw = tile - th * tiles_w;
    const int h0 = th * LT_H, w0 = tw * LT_W, c0 = cblk * CB;
    const int C = p.C0 + p.C1;
    const DwSrc s = dw_src<sizeof(T)>(p, b, c0);
    const T* base = reinterpret_cast<const T*>(s.base);
#if DS_BOUNDS
    for (int slot = tid; slot < LT_NPX * LT_NV; slot += LT_NT) {
        const int px = slot / LT_NV, v = slot - px * LT_NV;
        const int hr = px / LT_HC, hc = px - hr * LT_HC;
        const int hi = h0 + hr - 3 - s.oh, wi = w0 + hc - 3 - s.ow;
        uint4 val = make_uint4(0, 0, 0, 0);
        if ((unsigned)hi < (unsigned)s.Hs && (unsigned)wi < (unsigned)s.Ws)
            val = DS_LD(uint4, base + ((size_t)(hi * s.Ws + wi) * s.Cs + s.cc + v * V), s.buf);
        xs[slot] = val;
    }
    for (int i = tid; i < 49 * CB; i += LT_NT) wsm[i] = DS_LD(float, p.wt + (size_t)(i / CB) * C + c0 + (i % CB), DS_BX_W);
#else
    {
        // every halo piece of this thread is requested before the first one is written to LDS: range-checked buffer loads with arithmetic
        // out-of-range offsets (bit 31 set = beyond any sample; the launcher keeps samples below 2 GB) — `if (inside) v = load` is an
        // exec-masked region per iteration that waits for its own load before the next one is issued (seven serial round trips)
        constexpr int SLOTS = LT_NPX * LT_NV, ITS = (SLOTS + LT_NT - 1) / LT_NT;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base), (short)0, (int)((size_t)s.Hs * s.Ws * s.Cs * sizeof(T)), 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wt), (short)0, 49 * C * 4, 0x00020000);
        u32x4 hv[ITS];
#pragma unroll
        for (int it = 0; it < ITS; ++it) {
            const int slot = tid + it * LT_NT;
            const int px = slot / LT_NV, v = slot - px * LT_NV;
            const int hr = px / LT_HC, hc = px - hr * LT_HC;
            const int hi = h0 + hr - 3 - s.oh, wi = w0 + hc - 3 - s.ow;
            const unsigned bad = (unsigned)(slot >= SLOTS) | (unsigned)((unsigned)hi >= (unsigned)s.Hs) | (unsigned)((unsigned)wi >= (unsigned)s.Ws);
            const unsigned off = (unsigned)((hi * s.Ws + wi) * s.Cs + s.cc + v * V) * (unsigned)sizeof(T);
            hv[it] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)((off & 0x7fffffffu) | (bad << 31)), 0, 0);
        }
        // the block's 49 x CB weights: one 16-byte piece per thread (CB / 4 pieces per tap)
        constexpr int WP = 49 * CB / 4, WIT = (WP + LT_NT - 1) / LT_NT;
        asm volatile("" : "+v"(hv[ITS - 1]));                       // (the last, conditional piece: keep its load with the others)
        u32x4 wv4[WIT];
#pragma unroll
        for (int k = 0; k < WIT; ++k) {
            const int wp = tid + k * LT_NT, wtap = wp / (CB / 4), wj = wp - wtap * (CB / 4);
            wv4[k] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, (int)((unsigned)((wtap * C + c0 + 4 * wj) * 4) | ((unsigned)(wp >= WP) << 31)), 0, 0);
        }
#pragma unroll
        for (int it = 0; it < ITS; ++it) {
            const int slot = tid + it * LT_NT;
            if (it + 1 < ITS || slot < SLOTS) *reinterpret_cast<u32x4*>(xs + slot) = hv[it];
        }
#pragma unroll
        for (int k = 0; k < WIT; ++k)
            if (tid + k * LT_NT < WP) *reinterpret_cast<u32x4*>(wsm + 4 * (tid + k * LT_NT)) = wv4[k];
    }
#endif
    const int cv = tid % LT_NV, wl = (tid / LT_NV) % LT_W, strip = tid / (LT_NV * LT_W);
    const int c = c0 + cv * V;
    float acc[LT_SR][V];
    {
        float init[V];
#if DS_BOUNDS
#pragma unroll
        for (int v = 0; v < V; ++v) {
            init[v] = p.bias[c + v];
            if (p.tbias) init[v] += p.tbias[(size_t)b * p.tb_stride + c + v];
        }
#else
        // bias and time bias as 16-byte buffer loads requested before the barrier (a NULL time bias is a zero-length buffer: loads return 0)
        const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), (short)0, C * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_t = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.tbias ? p.tbias + (size_t)b * p.tb_stride : p.bias),
                                                                               (short)0, p.tbias ? C * 4 : 0, 0x00020000);
#pragma unroll
        for (int v = 0; v < V; v += 4) {
            const u32x4 b4 = __builtin_amdgcn_raw_buffer_load_b128(rs_b, (c + v) * 4, 0, 0), t4 = __builtin_amdgcn_raw_buffer_load_b128(rs_t, (c + v) * 4, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) init[v + j] = __uint_as_float(b4[j]) + __uint_as_float(t4[j]);
        }
#endif
        __syncthreads();
#pragma unroll
        for (int o = 0; o < LT_SR; ++o)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[o][v] = init[v];
    }
#pragma unroll 1
    for (int dw = 0; dw < 7; ++dw)     // not unrolled: keeps only one tap column of weights + inputs live
        dw_tap_column<LT_SR, V>(acc, wsm + dw * CB + cv * V, 7 * CB, [&](int r, float* x) {
            Vec16<T>::load(reinterpret_cast<const T*>(xs + ((strip * LT_SR + r) * LT_HC + wl + dw) * LT_NV + cv), x);
        });
    float2 st = {0.f, 0.f};
    const int w = w0 + wl;
#pragma unroll
    for (int o = 0; o < LT_SR; ++o) {
        const int h = h0 + strip * LT_SR + o;
        if (h < p.H && w < p.W) st = dw_store_row<T>(p, sizeof(T) == 4 && p.out_split, b, h, w, C, c, acc[o], st);
    }
    if (p.stats_part) block_stats_write(st.x, st.y, red, p.stats_part + ((size_t)b * gridDim.x + bix) * 2);
}

// ------------------------------------------------------------------------------------------------ dwconv7, LDS ring over a column strip (r05)
// The tile kernel above fetches a 22 x 22 halo for every 16 x 16 outputs: 1.89 x its input from L2 and — PMC FETCH_SIZE, r04 — 1.46 x from
// HBM (the 6 halo rows a tile shares with its vertical neighbour have usually left the L2 by the time that neighbour runs; the XCD-chunked
// order that would keep them there lost to its HBM-channel concentration).  Here a block owns a 16-column strip of one (sample, 32-channel
// block) and WALKS DOWN it, 16 output rows per iteration, over a ring of 22 input rows in LDS: every input row of the strip leaves HBM once,
// whatever the caches do (only the 6 halo COLUMNS of a strip are read twice, by its neighbour strips: 22 / 16 from L2, 19 - 22 of 16 real).
// The 16 new rows of iteration t + 1 are requested BEFORE the arithmetic of iteration t (64 registers in flight per lane) and enter the ring
// after it; the outputs of iteration t leave after that refill, so the refill waits for its loads only, not for stores.  The tile kernel's
// thread map and its stencil (dw_tap_column): bit-identical outputs; one statistics partial per strip instead of per tile.
// fp32 tensors with 32-channel blocks (NV = 8) and the split-precision tier's plane output only: that is where the bytes are.
constexpr int ST_W = 16, ST_R = 16, ST_HC = ST_W + 6, ST_HR = ST_R + 6, ST_NT = 256;
constexpr int ST_ROWB = ST_HC * 8 * 16;                 // bytes per ring row: 22 pixels x 128 B
constexpr int ST_XS = ST_HR * ST_ROWB;                  // 61 952
constexpr int ST_LDS = ST_XS + 49 * 32 * 4 + 64;

__global__ __launch_bounds__(ST_NT, 2) void dwconv7_strip_kernel(const ds_dwconv_params p, int strips_w, int ncblk, int hparts, int rows_per_part) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    char* const xs = dsm;                                                               // ring [22 rows][22 px][8 x 16 B]
    float* const wsm = reinterpret_cast<float*>(dsm + ST_XS);                           // [49][32]
    float* const red = wsm + 49 * 32;
    const int tid = threadIdx.x;
    const int nwg = gridDim.x;
    int wid = blockIdx.x;
    if ((nwg & 7) == 0) wid = (wid & 7) * (nwg >> 3) + (wid >> 3);       // XCD-chunked: consecutive items on one XCD
    // channel block fastest (the tile kernel's order)
    const int cblk = wid % ncblk, sw = (wid / ncblk) % strips_w, hp = (wid / (strips_w * ncblk)) % hparts, b = wid / (strips_w * ncblk * hparts);
    const int bix = (hp * strips_w + sw) * ncblk + cblk;      // slot in the sample's statistics partials (order-independent sum)
    const int w0 = sw * ST_W, c0 = cblk * 32;
    const int hbeg = hp * rows_per_part, hend = min(p.H, hbeg + rows_per_part);
    const int ntile = (hend - hbeg + ST_R - 1) / ST_R;
    const int C = p.C0 + p.C1;
    const DwSrc s = dw_src<4>(p, b, c0);
    // ---- staging map: thread -> (halo column hc = tid >> 3 < 22, 16-byte piece v = tid & 7); row `it` of a batch of rows.  Waves 0, 1 are
    // fully active, wave 2 three quarters, wave 3 not at all (its branch is wave-uniform)
    const int hc = tid >> 3, sv = tid & 7;
    const bool stager = hc < ST_HC;
    const int wi = w0 + hc - 3 - s.ow;
    const bool col_ok = stager && (unsigned)wi < (unsigned)s.Ws;
    const unsigned colbyte = (unsigned)((wi * s.Cs + s.cc + sv * 4) * 4);   // byte offset inside an image row (garbage when !col_ok: masked below)
    const unsigned rowpitch = (unsigned)(s.Ws * s.Cs * 4);
#if !DS_BOUNDS
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(s.base), (short)0, (int)((size_t)s.Hs * s.Ws * s.Cs * 4), 0x00020000);
#endif
    auto load_rows = [&](u32x4* dst, int row0, auto nc) {                    // image rows row0 .. row0 + n - 1 (this source's coordinates: - oh)
        constexpr int n = decltype(nc)::value;
#pragma unroll
        for (int it = 0; it < n; ++it) {
            const int hi = row0 + it - s.oh;
            const unsigned bad = (unsigned)(!col_ok) | (unsigned)((unsigned)hi >= (unsigned)s.Hs);
#if DS_BOUNDS
            dst[it] = u32x4{0u, 0u, 0u, 0u};
            if (!bad) dst[it] = DS_LD(u32x4, s.base + (size_t)hi * rowpitch + colbyte, s.buf);
#else
            const unsigned off = (unsigned)hi * rowpitch + colbyte;
            dst[it] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)((off & 0x7fffffffu) | (bad << 31)), 0, 0);
#endif
        }
    };
    auto store_rows = [&](const u32x4* src, int slot0, auto nc) {            // ring slots (slot0 + it) mod 22
        constexpr int n = decltype(nc)::value;
#pragma unroll
        for (int it = 0; it < n; ++it) {
            int sl = slot0 + it;
            sl = sl >= ST_HR ? sl - ST_HR : sl;
            *reinterpret_cast<u32x4*>(xs + sl * ST_ROWB + tid * 16) = src[it];
        }
    };
    auto lds_barrier = [&]() {          // LDS-only synchronisation: no wait for global loads / stores in flight (a __syncthreads() drains vmcnt)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    using N6 = std::integral_constant<int, 6>;
    using N16 = std::integral_constant<int, ST_R>;

    // ---- prologue: weights, bias, the first 22 rows
    u32x4 hv[ST_R];
    u32x4 h6[6];
    if (stager) {
        load_rows(h6, hbeg - 3, N6{});
        load_rows(hv, hbeg + 3, N16{});
    }
    {
        constexpr int WP = 49 * 32 / 4, WIT = (WP + ST_NT - 1) / ST_NT;     // 392 pieces of 16 B: two per thread
#pragma unroll
        for (int k = 0; k < WIT; ++k) {
            const int wp = tid + k * ST_NT, wtap = wp >> 3, wj = wp & 7;
            if (wp < WP) *reinterpret_cast<f32x4*>(wsm + 4 * wp) = DS_LD(f32x4, p.wt + (size_t)wtap * C + c0 + 4 * wj, DS_BX_W);
        }
    }
    const int cv = tid & 7, wl = (tid >> 3) & 15, strip = tid >> 7;
    const int c = c0 + cv * 4;
    float init[4];
    {
        const f32x4 b4 = DS_LD(f32x4, p.bias + c, DS_BX_BIAS);
        f32x4 t4 = {0.f, 0.f, 0.f, 0.f};
        if (p.tbias) t4 = DS_LD(f32x4, p.tbias + (size_t)b * p.tb_stride + c, DS_BX_AUX1);
#pragma unroll
        for (int j = 0; j < 4; ++j) init[j] = b4[j] + t4[j];
    }
    if (stager) {
        store_rows(h6, 0, N6{});
        store_rows(hv, 6, N16{});
    }
    lds_barrier();

    float2 st = {0.f, 0.f};
    int rbase = 0;                                               // ring slot of the tile's first input row (output row - 3)
    const int w = w0 + wl;
    const int colb = wl * 128 + cv * 16;
#pragma unroll 1
    for (int t = 0; t < ntile; ++t) {
        const int htop = hbeg + t * ST_R;
        const bool more = t + 1 < ntile;
        if (more && stager) load_rows(hv, htop + ST_R + 3, N16{});          // rows 6 .. 21 of the next tile
        // byte offsets of this thread's 14 input rows in the ring
        int roff[LT_SR + 6];
#pragma unroll
        for (int r = 0; r < LT_SR + 6; ++r) {
            int sl = rbase + strip * LT_SR + r;
            sl = sl >= ST_HR ? sl - ST_HR : sl;
            sl = sl >= ST_HR ? sl - ST_HR : sl;
            roff[r] = sl * ST_ROWB + colb;
        }
        float acc[LT_SR][4];
#pragma unroll
        for (int o = 0; o < LT_SR; ++o)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[o][v] = init[v];
#pragma unroll 1
        for (int dw = 0; dw < 7; ++dw)     // not unrolled: keeps only one tap column of weights + inputs live
            dw_tap_column<LT_SR, 4>(acc, wsm + dw * 32 + cv * 4, 7 * 32, [&](int r, float* x) {
                Vec16<float>::load(reinterpret_cast<const float*>(xs + roff[r] + dw * 128), x);
            });
        lds_barrier();                                           // every wave has read what it needs of this tile's rows
        if (more) {
            int ws = rbase + ST_R + 6;                           // slot of the next tile's row 6 = this tile's row 22 -> (rbase + 22) mod 22 = rbase
            ws = ws >= ST_HR ? ws - ST_HR : ws;
            ws = ws >= ST_HR ? ws - ST_HR : ws;
            if (stager) store_rows(hv, ws, N16{});
            rbase = rbase + ST_R >= ST_HR ? rbase + ST_R - ST_HR : rbase + ST_R;
        }
        // outputs of this tile: hi / lo bf16 planes of a 2C-channel image (DS_CONV_F_SPLIT_IN), or fp32
#pragma unroll
        for (int o = 0; o < LT_SR; ++o) {
            const int h = htop + strip * LT_SR + o;
            if (h < hend && w < p.W) st = dw_store_row<float>(p, p.out_split, b, h, w, C, c, acc[o], st);
        }
        if (more) lds_barrier();                                 // the refilled rows are visible
    }
    __syncthreads();
    if (p.stats_part) block_stats_write(st.x, st.y, red, p.stats_part + ((size_t)b * (hparts * strips_w * ncblk) + bix) * 2);
}

// ------------------------------------------------------------------------------------------------ dwconv7 on MFMA, persistent blocks
// The VALU stencil above needs 49 fma + conversions per output and is issue-bound at ~2x its own floor.  Here the
// horizontal part of the stencil becomes a banded (Toeplitz) matrix, so one channel's 16x16 output block is
//     out[h][w] = sum_{dh} sum_{w'} x[h+dh][w'] * T_c[(dh,w')][w],   T_c[(dh,w')][w] = k_c[dh][w'-w]  (0 <= w'-w < 7)
// = A[16 x 168] . T_c[168 x 16] -> 6 x v_mfma_f32_16x16x32_bf16 (K padded to 192).  3.9x more MACs than the
// stencil, on a pipe that is 16x faster, with no bf16->fp32 conversions.
//   LDS holds the input halo PLANAR ([channel][row][cols] bf16) so that a lane's 8 consecutive k (= 8 adjacent columns of one
//   channel/row) are one 16-byte read; T_c fragments are precomputed per channel (ds_pack_dw_weight_mfma).
//   K order: MFMA ks, lane group kq -> (dh, wg) = (4 * (ks & 1) + kq, ks >> 1): the four lane groups of one read differ by whole plane
//   rows only, so the 16 lanes of every ds_read_b128 group touch distinct (or identical) rows and, with the 80- / 48-byte row pitch,
//   distinct bank slots (the order (dh, wg) = (G / 3, G % 3) made every read a 2-way conflict).  dh = 7 is padding: row 6 again, zero weights.
// One block per tile of 32 channels (the first generation: two blocks per CU, 2.65 TB/s) is bound by latency and instruction issue, not by a
// pipe (profiles/r03_dw_pmc.txt: 48 % of wave cycles in s_waitcnt, MFMA pipe 11 % busy, LDS 42 %): every block pays one exposed memory round
// trip for its halo and re-fetches 24 KB of Toeplitz fragments per wave (192 KB per block against 53 KB of input).  Here ONE block per CU
// walks over CHUNKS of up to 8 tiles of one (sample, 32-channel block):
//   * the fragments of the wave's 2 channels stay in registers for the whole chunk (48 VGPRs; 16 waves per block, 128 registers per lane);
//   * the halo of tile t+1 is requested BEFORE the MFMA phase of tile t (16 VGPRs) and written into the other of two LDS plane sets after
//     tile t's output has left: the memory round trip hides behind a whole tile of work;
//   * a thread stages FOUR adjacent pixels of 8 channels (880 slots, one per thread): 8-byte LDS writes, half as many as the pixel-pair form,
//     and the plane sets are skewed by 64 bytes per 8 planes (whole planes apart the four lanes of a pixel quad hit one bank);
//   * the output tile is staged in its own 32 KB (16-byte chunks XOR-swizzled by the pixel column: the 8-byte writes of a wave were 8-way
//     bank conflicts) and leaves as whole 64-byte pixel rows;
//   * GroupNorm partials: one (sum, sum of squares) pair per chunk instead of one per tile.
// Chunks are dealt round-robin to the blocks in the XCD-chunked block order, channel block fastest: the blocks of one XCD work on the
// channel blocks of the same tiles at the same time (they share every 128-byte line of the input).
// two tile shapes of 512 pixels (two 16 x 16 MFMA blocks): WIDE 16 rows x 32 columns, TALL 32 rows x 16 columns for images at most 16 wide
constexpr int MF_CB = 32;
template <bool TALL> struct M2 {
    static constexpr int W = TALL ? 16 : 32, H = TALL ? 32 : 16;
    static constexpr int HR = H + 6;                                   // halo rows
    static constexpr int HC = TALL ? 24 : 40;                          // plane row pitch in elements (22 / 38 used): whole pixel quads
    static constexpr int PLANE = HR * HC, SKEW = 32;
    static constexpr int BLK2 = TALL ? 16 * HC : 16;                   // element offset of the second 16 x 16 block inside a plane
    static constexpr int PBYTES = (MF_CB * PLANE + 3 * SKEW) * 2;      // one plane set: 56512 / 58560 bytes
    static constexpr int OFF_O = 2 * PBYTES, OBYTES = H * W * MF_CB * 2, OFF_RED = OFF_O + OBYTES, LDS = OFF_RED + 64;
    static constexpr int SLOTS = HR * (HC / 4) * 4;                    // 880 / 912 (pixel quad, 8-channel group) pairs: one per thread
    static_assert(LDS <= 160 * 1024, "one block per CU");
};

struct Dw2Geo { int tiles_w, tiles, ncblk, tpc, nchunk, total; };
typedef __amdgpu_buffer_rsrc_t dw_rsrc_t;
__device__ __forceinline__ u32x4 dw_buf_ld16(dw_rsrc_t rs, const char* base, unsigned voff, int bounds_buf) {
#if DS_BOUNDS
    if (voff >= 0x80000000u || !ds_bx_ok(base + voff, bounds_buf, 16)) return u32x4{0u, 0u, 0u, 0u};
#endif
    (void)base; (void)bounds_buf;
    return __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, 0, 0);
}

template <int NW, bool TALL>
__global__ __launch_bounds__(NW * 64, 1) void dwconv7_mfma2_kernel(const ds_dwconv_params p, const Dw2Geo g) {
    using G = M2<TALL>;
    constexpr int M2_W = G::W, M2_H = G::H, M2_HC = G::HC, M2_PLANE = G::PLANE, M2_SKEW = G::SKEW, M2_PBYTES = G::PBYTES, M2_OFF_O = G::OFF_O,
                  M2_OFF_RED = G::OFF_RED, M2_SLOTS = G::SLOTS;
    constexpr int NT = NW * 64, CPW = MF_CB / NW, SIT = (M2_SLOTS + NT - 1) / NT, OIT = M2_H * M2_W * 4 / NT;      // channels per wave, halo slots and output pieces per thread
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    float* red = reinterpret_cast<float*>(dsm + M2_OFF_RED);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NB = gridDim.x;
    int lid = blockIdx.x;
    if (NB % 8 == 0) lid = (blockIdx.x & 7) * (NB >> 3) + (blockIdx.x >> 3);
    if (lid >= g.total) return;
    const int nmy = (g.total - lid + NB - 1) / NB;            // this block's chunks: lid, lid + NB, ...
    // ... = nt tiles, walked as one sequence.  The last chunk of a channel block is short where chunks of several whole samples do not divide
    // B (the chunk length is chosen from ds_dwconv_params.batch_hint alone): it is the last chunk of the block that owns it
    const int nt = nmy * g.tpc - ((lid + (nmy - 1) * NB) / g.ncblk == g.nchunk - 1 ? g.nchunk * g.tpc - p.B * g.tiles : 0);
    const int C = p.C0 + p.C1;
    const bf16* wexp = reinterpret_cast<const bf16*>(p.wexp);

    // ---- a tile of the sequence: channel block, sample, origin, source (the skip concat is two sources with an offset).  A chunk is
    // g.tpc consecutive (sample, tile) items of ONE channel block — part of a sample's tiles, or several whole samples where an image has
    // only one or two tiles; the divisions run once per chunk, inside a chunk the position advances incrementally (all scalar: wave-uniform)
    struct Tile { dw_rsrc_t rs; int c, j, tile, th, tw, b, c0, h0, w0; DwSrc s; };
    auto set_sample = [&](Tile& t) {
        t.s = dw_src<2>(p, t.b, t.c0);
        // one sample of the source as a range-checked buffer: halo pixels outside the image carry an out-of-range offset and read as zeros
        // (no select on the loaded data: a select would make the wave wait for the halo right where it is requested)
        t.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(t.s.base), (short)0, t.s.Hs * t.s.Ws * t.s.Cs * 2, 0x00020000);
    };
    auto start_chunk = [&](int c) {
        Tile t;
        t.c = c;
        t.j = 0;
        const int cblk = c % g.ncblk, item = (c / g.ncblk) * g.tpc;
        t.b = item / g.tiles;
        t.tile = item - t.b * g.tiles;
        t.th = t.tile / g.tiles_w;
        t.tw = t.tile - t.th * g.tiles_w;
        t.h0 = t.th * M2_H;
        t.w0 = t.tw * M2_W;
        t.c0 = cblk * MF_CB;
        set_sample(t);
        return t;
    };
    auto next_tile = [&](Tile t) {
        if (t.j + 1 == g.tpc) return start_chunk(t.c + NB);
        ++t.j;
        if (++t.tile == g.tiles) {                             // next sample, same channels
            t.tile = 0; t.th = 0; t.tw = 0;
            ++t.b;
            set_sample(t);
        } else if (++t.tw == g.tiles_w) { t.tw = 0; ++t.th; }
        t.h0 = t.th * M2_H;
        t.w0 = t.tw * M2_W;
        return t;
    };

    // ---- halo staging slots of this thread (tile-independent): slot -> (8-channel group v, halo row hr, first column hc of a pixel quad)
    int s_hr[SIT], s_hc[SIT], s_lds[SIT];
    bool s_ok[SIT];
    const int sv = tid & 3;
#pragma unroll
    for (int it = 0; it < SIT; ++it) {
        const int slot = tid + it * NT, qd = slot >> 2;
        s_ok[it] = slot < M2_SLOTS;
        s_hr[it] = qd / (M2_HC / 4);
        s_hc[it] = (qd - s_hr[it] * (M2_HC / 4)) * 4;
        s_lds[it] = ((sv * 8) * M2_PLANE + sv * M2_SKEW + s_hr[it] * M2_HC + s_hc[it]) * 2;      // bytes inside a plane set
    }
    u32x4 fv[SIT][4];
    auto issue_halo = [&](const Tile& t) {
#pragma unroll
        for (int it = 0; it < SIT; ++it) {
            const int hi = t.h0 + s_hr[it] - 3 - t.s.oh, wi = t.w0 + s_hc[it] - 3 - t.s.ow;
            // (arithmetic, not a select: any offset with bit 31 set is beyond the buffer.  The offset of a row above the image is garbage: every
            // offset is cut to 28 bits — a sample is far below 256 MB — so that bit 31 plus it plus 16 bytes cannot wrap around 2^32 into the buffer)
            const unsigned badr = (unsigned)(!s_ok[it]) | (unsigned)((unsigned)hi >= (unsigned)t.s.Hs);
            const unsigned o = (unsigned)((hi * t.s.Ws + wi) * t.s.Cs + t.s.cc + sv * 8) * 2u;       // (may be "negative": pixel quads straddle the left edge)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned bad = badr | (unsigned)((unsigned)(wi + e) >= (unsigned)t.s.Ws);
                fv[it][e] = dw_buf_ld16(t.rs, t.s.base, ((o + (unsigned)(e * t.s.Cs) * 2u) & 0x0fffffffu) | (bad << 31), t.s.buf);
            }
        }
    };
    auto fill_planes = [&](char* pl) {
#pragma unroll
        for (int it = 0; it < SIT; ++it) {
            if (s_ok[it]) {
                char* dst = pl + s_lds[it];
#pragma unroll
                for (int j = 0; j < 4; ++j) {                  // dword j of a pixel = channels 2j, 2j+1; a plane row gets 4 pixels = 8 bytes
                    const unsigned a = fv[it][0][j], b2 = fv[it][1][j], c2 = fv[it][2][j], d = fv[it][3][j];
                    typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<u32x2_t*>(dst + (2 * j) * (M2_PLANE * 2)) =
                        u32x2_t{__builtin_amdgcn_perm(b2, a, 0x05040100u), __builtin_amdgcn_perm(d, c2, 0x05040100u)};
                    *reinterpret_cast<u32x2_t*>(dst + (2 * j + 1) * (M2_PLANE * 2)) =
                        u32x2_t{__builtin_amdgcn_perm(b2, a, 0x07060302u), __builtin_amdgcn_perm(d, c2, 0x07060302u)};
                }
            }
        }
    };

    const int m = lane & 15, kq = lane >> 4;
    int aoff[6];                                               // A fragment offsets (elements): the K order above
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
        const int dh = 4 * (ks & 1) + kq, wg = ks >> 1;
        aoff[ks] = (m + (dh > 6 ? 6 : dh)) * M2_HC + 8 * wg;
    }
    bf16x8 wv[CPW][6];
    float addv[CPW];
    auto load_addv = [&](const Tile& t) {                      // bias (+ this sample's time bias) of this wave's channels
        const int cb = t.c0 + wave * CPW;
#pragma unroll
        for (int k = 0; k < CPW; ++k) {
            addv[k] = DS_LD(float, p.bias + cb + k, DS_BX_BIAS);
            if (p.tbias) addv[k] += DS_LD(float, p.tbias + (size_t)t.b * p.tb_stride + cb + k, DS_BX_AUX1);
        }
    };
    auto load_chunk_consts = [&](const Tile& t) {              // Toeplitz fragments of this wave's channels
        const int cb = t.c0 + wave * CPW;
#pragma unroll
        for (int ci = 0; ci < CPW; ++ci) {
            const bf16* we = wexp + ((size_t)(cb + ci) * 6 * 64 + lane) * 8;
#pragma unroll
            for (int ks = 0; ks < 6; ++ks) wv[ci][ks] = DS_LD(bf16x8, we + ks * 64 * 8, DS_BX_AUX0);
        }
        load_addv(t);
    };

    Tile cur = start_chunk(lid);
    issue_halo(cur);
    load_chunk_consts(cur);
    fill_planes(dsm);
    __syncthreads();
    float s1 = 0.f, s2 = 0.f;
    char* const ot = dsm + M2_OFF_O;
    // (the body is instantiated twice — with and without a next tile — so that inside the loop nothing is conditional on it: with an
    // `if (more)` around the halo request and another around the fill, the compiler's wait-count bookkeeping merges the two paths, takes the
    // halo loads for possibly still pending at the back edge and guards the next request with waits that in fact wait for the output stores)
    auto tile_body = [&](const int u, auto more_t) {
        constexpr bool more = decltype(more_t)::value;
        char* const pl = dsm + (u & 1) * M2_PBYTES;
        Tile nxt = cur;
        if constexpr (more) {
            nxt = next_tile(cur);
            issue_halo(nxt);                                   // in flight during this tile's MFMA phase
        }
        // ---- CPW channels x two 16 x 16 blocks: 12 MFMAs per channel
        float outv[2][4][CPW];                                 // [column block][row][channel]
#pragma unroll
        for (int ci = 0; ci < CPW; ++ci) {
            const int cl = wave * CPW + ci;
            const bf16* plane = reinterpret_cast<const bf16*>(pl) + cl * M2_PLANE + (cl >> 3) * M2_SKEW;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 6; ++ks) {
                const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(plane + aoff[ks]);
                const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(plane + aoff[ks] + G::BLK2);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wv[ci][ks], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wv[ci][ks], acc1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                outv[0][r][ci] = acc0[r] + addv[ci];
                outv[1][r][ci] = acc1[r] + addv[ci];
            }
        }
        // C/D layout of 16x16x32: col = lane & 15 (w), row = (lane >> 4) * 4 + r (h).  Statistics from the fp32 values.
#pragma unroll
        for (int wb = 0; wb < 2; ++wb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (cur.h0 + (TALL ? 16 * wb : 0) + kq * 4 + r < p.H && cur.w0 + (TALL ? 0 : 16 * wb) + m < p.W) {
#pragma unroll
                    for (int v = 0; v < CPW; ++v) {
                        s1 += outv[wb][r][v];
                        s2 = fmaf(outv[wb][r][v], outv[wb][r][v], s2);
                    }
                }
        // ---- output tile -> LDS [rows][cols][32 ch] bf16 (64 B per pixel; 16-byte chunk q of column col at q ^ ((col >> 1) & 3))
#pragma unroll
        for (int wb = 0; wb < 2; ++wb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                typedef __bf16 bf16xc_t __attribute__((ext_vector_type(CPW)));
                bf16xc_t pk;
#pragma unroll
                for (int v = 0; v < CPW; ++v) pk[v] = (bf16)outv[wb][r][v];
                const int col = (TALL ? 0 : 16 * wb) + m, row = (TALL ? 16 * wb : 0) + kq * 4 + r, cbyte = wave * CPW * 2;          // this wave's channels: bytes cbyte .. of the pixel's 64
                *reinterpret_cast<bf16xc_t*>(ot + (row * M2_W + col) * 64 + (((cbyte >> 4) ^ ((col >> 1) & 3)) * 16) + (cbyte & 15)) = pk;
            }
        __syncthreads();                                       // the output tile is complete; every wave is done with this plane set
        const bool chunk_end = cur.j + 1 == g.tpc, sample_end = chunk_end || cur.tile + 1 == g.tiles;
        if (sample_end && p.stats_part) {                      // (block-uniform; one barrier inside): one partial per (sample, chunk, channel block)
            const int nps = g.tiles >= g.tpc ? g.tiles / g.tpc : 1, kk = g.tiles >= g.tpc ? cur.tile / g.tpc : 0;
            block_stats_write(s1, s2, red, p.stats_part + ((size_t)cur.b * (nps * g.ncblk) + kk * g.ncblk + cur.c0 / MF_CB) * 2);
            s1 = 0.f;
            s2 = 0.f;
        }
        // the next tile's halo has had the whole MFMA phase to arrive: into the other plane set first, THEN this tile's output — its
        // stores stay in flight across the barrier and the next tile (only the LDS reads that feed them must be done before it)
        if constexpr (more) {
            if (chunk_end || sample_end) {
                if (chunk_end) load_chunk_consts(nxt);
                else load_addv(nxt);
                // consumed (= waited for) inside the branch, once per chunk: loads and stores retire out of order with respect to each other,
                // so with these left pending at the back edge the first MFMA of EVERY tile would be guarded by s_waitcnt vmcnt(0) — which
                // in the common path waits for the previous tile's output stores
#pragma unroll
                for (int ci = 0; ci < CPW; ++ci)
#pragma unroll
                    for (int ks = 0; ks < 6; ++ks) asm volatile("" : "+v"(wv[ci][ks]));
#pragma unroll
                for (int ci = 0; ci < CPW; ++ci) asm volatile("" : "+v"(addv[ci]));
            }
            fill_planes(dsm + ((u + 1) & 1) * M2_PBYTES);
        }
        {
            bf16* outp = reinterpret_cast<bf16*>(p.out) + (size_t)cur.b * p.H * p.W * C;
#pragma unroll
            for (int k = 0; k < OIT; ++k) {
                const int piece = tid + k * NT, px = piece >> 2, q = piece & 3;   // 4 consecutive lanes = one pixel's 64 bytes
                const int col = px % M2_W, h = cur.h0 + px / M2_W, w = cur.w0 + col;
                if (h < p.H && w < p.W) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(ot + px * 64 + ((q ^ ((col >> 1) & 3)) * 16));
                    DS_ST(u32x4, outp + ((size_t)(h * p.W + w) * C + cur.c0 + q * 8), DS_BX_OUT, v);
                }
            }
        }
        __syncthreads();                                       // next plane set complete, output staging free
        cur = nxt;
    };
    for (int u = 0; u + 1 < nt; ++u) tile_body(u, std::true_type{});
    tile_body(nt - 1, std::false_type{});
}

// The batch the batch-dependent choices below look at: ds_dwconv_params.batch_hint where the caller gives one (the shared prefix of a paired
// plan runs at half the batch and must group its GroupNorm partials as the plain plan does at the full batch; a caller that pins one value
// for every batch it runs), else B.  No choice looks at B itself where a hint is given.
static int dw_batch(const ds_dwconv_params* p) { return p->batch_hint > 0 ? p->batch_hint : p->B; }

static bool dw_tall(const ds_dwconv_params* p) { return p->W <= 16; }
static Dw2Geo dw2_geo(const ds_dwconv_params* p) {
    const int tw = dw_tall(p) ? 16 : 32, th = dw_tall(p) ? 32 : 16;
    Dw2Geo g;
    g.tiles_w = (p->W + tw - 1) / tw;
    g.tiles = g.tiles_w * ((p->H + th - 1) / th);
    g.ncblk = (p->C0 + p->C1) / MF_CB;
    // chunk = tpc consecutive (sample, tile) items of one channel block: a divisor of a sample's tiles, or whole samples (tpc a multiple
    // of the tiles of one, taken where that many samples divide the decision batch) — never a run that ends inside one sample and starts
    // inside the next.  Where they do not divide B itself (a hint other than B) the last chunk of a channel block is short (the kernel
    // takes it for the last chunk of its block: at most 256 channel blocks, one per block of the grid at least).
    // The longest such chunk (<= 8 items) that still leaves two chunks per CU: small batches get short chunks (parallelism before amortisation)
    g.tpc = 1;
    for (int d = 2; d <= 8; ++d)
        if ((g.tiles % d == 0 || (d % g.tiles == 0 && dw_batch(p) % (d / g.tiles) == 0 && g.ncblk <= 256)) && (long long)dw_batch(p) * g.tiles / d * g.ncblk >= 512) g.tpc = d;
    g.nchunk = (p->B * g.tiles + g.tpc - 1) / g.tpc;          // chunks per channel block (tpc divides B * tiles, or covers whole samples)
    g.total = g.nchunk * g.ncblk;
    return g;
}

__global__ void pack_dw_mfma_kernel(const float* w, int C, bf16* dst) {
    // dst[c][ks][lane][j]: B operand of 16x16x32 — lane = (n = lane & 15, kq = lane >> 4), k = ks*32 + kq*8 + j
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)C * 6 * 64 * 8) return;
    const int j = i & 7, lane = (i >> 3) & 63, ks = (i >> 9) % 6, c = i / (6 * 64 * 8);
    const int n = lane & 15, kq = lane >> 4;
    const int dh = 4 * (ks & 1) + kq, wg = ks >> 1, wp = 8 * wg + j, dw = wp - n;      // K order of dwconv7_mfma2_kernel's aoff[]
    float v = 0.f;
    if (dh < 7 && dw >= 0 && dw < 7) v = w[(size_t)c * 49 + dh * 7 + dw];
    dst[i] = (bf16)v;
}

__global__ void pack_dw_kernel(const float* w, int C, float* dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over 49*C, dst[tap][c] = w[c][tap]
    if (i < 49 * C) dst[i] = w[(size_t)(i % C) * 49 + i / C];
}

}  // namespace

static bool dw_use_mfma(const ds_dwconv_params* p) {
    const long long s0 = (long long)p->H * p->W * p->C0 * 2, s1 = (long long)p->H1 * p->W1 * p->C1 * 2;      // (28-bit halo offsets inside a sample)
    return p->dtype == DS_BF16 && p->wexp != nullptr && p->C0 % MF_CB == 0 && p->C1 % MF_CB == 0 && s0 < (1ll << 28) && s1 < (1ll << 28);
}

static int lt_nv(const ds_dwconv_params* p) { return (p->dtype == DS_F32 && p->C0 % 32 == 0 && p->C1 % 32 == 0) ? 8 : 4; }
static bool dw_use_lds(const ds_dwconv_params* p) {
    const int CB = lt_nv(p) * (p->dtype == DS_BF16 ? 8 : 4);
    const long long es = p->dtype == DS_BF16 ? 2 : 4;
    // (a sample of either source below 2 GB: the halo loads carry "outside the image" in bit 31 of a 32-bit byte offset)
    const bool small = (long long)p->H * p->W * p->C0 * es < (1ll << 31) && (long long)p->H1 * p->W1 * p->C1 * es < (1ll << 31);
    return p->C0 % CB == 0 && p->C1 % CB == 0 && small;
}

// r05: the strip kernel (LDS ring walking down a 16-column strip) for the split-precision tier's depthwise layers.  Chosen by shape AND batch
// (it needs >= 512 blocks = two per CU; images of 256 rows may be cut into 2 - 4 row ranges to get there): its outputs are the tile
// kernel's bit for bit, its statistics partials are grouped differently — like the split-K choices of this tier, never taken
// in the fp32 parity tier unless ds_dwconv_params.strip = 1 asks for it (tests).
constexpr int ST_MIN_ITEMS = 512;
struct DwStrip { int on, strips_w, ncblk, hparts, rows_per_part; };
static DwStrip dw_strip(const ds_dwconv_params* p) {
    DwStrip g{0, 0, 0, 1, 0};
    const bool forced = p->strip == 1;
    if (p->strip == 2 || p->dtype != DS_F32 || lt_nv(p) != 8 || !dw_use_lds(p) || (!p->out_split && !forced) || p->W < 16 || p->H < 2 * ST_R)
        return g;
    g.strips_w = (p->W + ST_W - 1) / ST_W;
    g.ncblk = (p->C0 + p->C1) / 32;
    const long n0 = (long)dw_batch(p) * g.ncblk * g.strips_w;
    while (n0 * g.hparts < 2 * ST_MIN_ITEMS && p->H / (2 * g.hparts) >= 2 * ST_R) g.hparts *= 2;
    if (n0 * g.hparts < ST_MIN_ITEMS && !forced) return g;
    g.rows_per_part = ((p->H + g.hparts - 1) / g.hparts + ST_R - 1) / ST_R * ST_R;
    g.hparts = (p->H + g.rows_per_part - 1) / g.rows_per_part;
    g.on = 1;
    return g;
}

// What ds_dwconv7 launches for p: the kernel family, its geometry and the GroupNorm partials per sample that follow from it.  The one place
// where the families are told apart and a tile or a block is counted: the launcher's grids, the size ds_dwconv_stats_parts gives the
// partials buffer and the answers of ds_dwconv_launch_choice all read it.
struct DwPlan {
    int family;                                   // DS_DW_DIRECT / TILE / STRIP / MFMA
    int parts;                                    // partials per sample = the per-sample stride of stats_part (tile, direct: blocks per sample)
    int ranges, samples_per_chunk;                // what ds_dwconv_launch_choice reports
    Dw2Geo mfma;                                  // the geometry of `family`; the others stay zero
    DwStrip strip;
    struct { int nv, twl, tiles_w, tiles_h, ncblk; size_t lds; } tile;
    struct { int nstrip, CV; } direct;
};
static DwPlan dw_plan(const ds_dwconv_params* p) {
    const int V = p->dtype == DS_BF16 ? 8 : 4, C = p->C0 + p->C1;
    DwPlan pl{};
    pl.ranges = pl.samples_per_chunk = 1;
    if (dw_use_mfma(p)) {
        const Dw2Geo& g = pl.mfma = dw2_geo(p);
        pl.family = DS_DW_MFMA;
        pl.ranges = g.tiles >= g.tpc ? g.tiles / g.tpc : 1;            // chunks per image, or chunks of whole samples: one partial each
        pl.samples_per_chunk = g.tpc > g.tiles ? g.tpc / g.tiles : 1;
        pl.parts = pl.ranges * g.ncblk;
    } else if (const DwStrip g = dw_strip(p); g.on) {
        pl.family = DS_DW_STRIP;
        pl.strip = g;
        pl.ranges = g.hparts;
        pl.parts = g.hparts * g.strips_w * g.ncblk;
    } else if (dw_use_lds(p)) {
        auto& t = pl.tile;
        pl.family = DS_DW_TILE;
        t.nv = lt_nv(p);
        t.twl = lt_twl(p->W, t.nv);
        const int tw = 1 << t.twl, th = (2048 / t.nv) >> t.twl;
        t.tiles_w = (p->W + tw - 1) / tw;
        t.tiles_h = (p->H + th - 1) / th;
        t.ncblk = C / (t.nv * V);
        t.lds = (size_t)(tw + 6) * (th + 6) * t.nv * 16 + (size_t)49 * t.nv * V * sizeof(float) + 64;
        pl.parts = t.tiles_h * t.tiles_w * t.ncblk;
    } else {
        auto& d = pl.direct;
        pl.family = DS_DW_DIRECT;
        d.nstrip = (p->H + DW_TH - 1) / DW_TH;
        d.CV = C / V;
        pl.parts = (int)(((long)d.nstrip * p->W * d.CV + DW_BLOCK - 1) / DW_BLOCK);         // one partial per block
    }
    return pl;
}

extern "C" int ds_dwconv_stats_parts(const ds_dwconv_params* p) { return dw_plan(p).parts; }

extern "C" int ds_dwconv_launch_choice(const ds_dwconv_params* p, int32_t* family, int32_t* ranges, int32_t* samples_per_chunk) {
    DS_REQUIRE(p && family && ranges && samples_per_chunk, "dwconv_launch_choice: null pointer");
    const DwPlan pl = dw_plan(p);
    *family = pl.family;
    *ranges = pl.ranges;
    *samples_per_chunk = pl.samples_per_chunk;
    return DS_OK;
}

extern "C" int ds_dwconv7(const ds_dwconv_params* p, void* stream) {
    DS_REQUIRE(p && p->src0 && p->wt && p->bias && p->out, "dwconv7: null pointer");
    DS_REQUIRE(p->dtype == DS_F32 || p->dtype == DS_BF16, "dwconv7: dtype %d", p->dtype);
    const int V = p->dtype == DS_BF16 ? 8 : 4;
    const int C = p->C0 + p->C1;
    DS_REQUIRE(p->C0 > 0 && p->C0 % V == 0 && p->C1 % V == 0, "dwconv7: channels (%d,%d) must be multiples of %d", p->C0, p->C1, V);
    DS_REQUIRE(p->C1 == 0 || (p->src1 && p->H1 > 0 && p->W1 > 0), "dwconv7: second source incomplete");
    DS_REQUIRE(p->B > 0 && p->H > 0 && p->W > 0, "dwconv7: empty problem");
    DS_REQUIRE(p->batch_hint >= 0, "dwconv7: batch_hint must be 0 (use B) or the batch the launch decisions look at, got %d", p->batch_hint);
    DS_REQUIRE(p->strip >= 0 && p->strip <= 2, "dwconv7: strip must be 0 (library's choice), 1 (strip kernel) or 2 (tile kernel), got %d", p->strip);
    const DwPlan pl = dw_plan(p);
    DS_REQUIRE(!p->out_split || (p->dtype == DS_F32 && (pl.family == DS_DW_TILE || pl.family == DS_DW_STRIP)),
               "dwconv7: out_split needs the fp32 LDS-tile kernel (channels multiples of %d, samples below 2 GB)", 16);
    if (!ds_aligned16(p->src0) || !ds_aligned16(p->out) || !ds_aligned16(p->wt) || (p->C1 && !ds_aligned16(p->src1)))
        DS_FAIL(DS_EALIGN, "dwconv7: pointers must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        const long long es = V == 8 ? 2 : 4;
        DsBxHost h(pl.family == DS_DW_MFMA ? DS_K_DWCONV_MFMA : (pl.family == DS_DW_DIRECT ? DS_K_DWCONV : DS_K_DWCONV_LDS));   // (the strip kernel reports as the tile kernel)
        h.set(DS_BX_SRC0, p->src0, (long long)p->B * p->H * p->W * p->C0 * es);
        h.set(DS_BX_SRC1, p->C1 ? p->src1 : nullptr, (long long)p->B * p->H1 * p->W1 * p->C1 * es);
        h.set(DS_BX_W, p->wt, (long long)49 * C * 4);
        h.set(DS_BX_AUX0, p->wexp, (long long)C * 6 * 64 * 8 * 2);
        h.set(DS_BX_BIAS, p->bias, (long long)C * 4);
        h.set(DS_BX_AUX1, p->tbias, p->tbias ? ((long long)(p->B - 1) * p->tb_stride + C) * 4 : 0);
        h.set(DS_BX_OUT, p->out, (long long)p->B * p->H * p->W * C * es);
        h.set(DS_BX_STATS, p->stats_part, (long long)p->B * pl.parts * 2 * 4);
        h.publish(st);
    }
#endif
    if (pl.family == DS_DW_MFMA) {
        const Dw2Geo& g = pl.mfma;
        const int nb = g.total < 256 ? g.total : 256;           // one block per CU
        // 16 waves of 2 channels (128 registers per lane); 8 waves of 4 channels (256) measured 25 % slower: too few waves to cover a phase
        if (dw_tall(p)) {
            DS_SET_MAX_LDS((dwconv7_mfma2_kernel<16, true>), M2<true>::LDS, "dwconv7_mfma2");
            hipLaunchKernelGGL((dwconv7_mfma2_kernel<16, true>), dim3(nb), dim3(1024), M2<true>::LDS, st, *p, g);
        } else {
            DS_SET_MAX_LDS((dwconv7_mfma2_kernel<16, false>), M2<false>::LDS, "dwconv7_mfma2");
            hipLaunchKernelGGL((dwconv7_mfma2_kernel<16, false>), dim3(nb), dim3(1024), M2<false>::LDS, st, *p, g);
        }
        DS_CHECK_LAUNCH("dwconv7_mfma2");
    } else if (pl.family == DS_DW_STRIP) {
        const DwStrip& g = pl.strip;
        // XCD-chunked item order (consecutive items = the channel blocks of one strip on ONE XCD: the 64-byte halves of an output line two
        // channel blocks share merge in that L2; +2 % on 8 of 9 layer shapes, same box; strip fastest instead of channel block fastest: no
        // consistent gain).  r05 timing ablations at C = 96, 256 x 64, batch 128: 555 us whole; arithmetic alone 347 (784 v_pk_fma_f32 per
        // thread and tile: ~12 k cycles per pair of co-resident tiles against 6.3 k of issue slots), stores alone 264, loads alone 157, none 111
        DS_SET_MAX_LDS(dwconv7_strip_kernel, ST_LDS, "dwconv7_strip");
        hipLaunchKernelGGL(dwconv7_strip_kernel, dim3(pl.parts * p->B), dim3(ST_NT), ST_LDS, st, *p, g.strips_w, g.ncblk, g.hparts, g.rows_per_part);
        DS_CHECK_LAUNCH("dwconv7_strip");
    } else if (pl.family == DS_DW_TILE) {
        const auto& t = pl.tile;
        // (above 64 KB — the 8-wide tile of NV = 4 and both NV = 8 tiles — a kernel has to ask for its dynamic LDS)
#define DS_DW_LDS_LAUNCH(T_, TWL_, NV_)                                                                                                                        \
        do {                                                                                                                                                  \
            if (t.lds > 65536) DS_SET_MAX_LDS((dwconv7_lds_kernel<T_, TWL_, NV_>), t.lds, "dwconv7_lds");                                                      \
            hipLaunchKernelGGL((dwconv7_lds_kernel<T_, TWL_, NV_>), dim3(pl.parts, p->B), dim3(LT_NT), t.lds, st, *p, t.tiles_w, t.tiles_w * t.tiles_h, t.ncblk); \
        } while (0)
        if (p->dtype == DS_BF16) {
            if (t.twl == 5) DS_DW_LDS_LAUNCH(bf16, 5, 4); else if (t.twl == 4) DS_DW_LDS_LAUNCH(bf16, 4, 4); else DS_DW_LDS_LAUNCH(bf16, 3, 4);
        } else if (t.nv == 8) {
            if (t.twl == 4) DS_DW_LDS_LAUNCH(float, 4, 8); else DS_DW_LDS_LAUNCH(float, 3, 8);
        } else {
            if (t.twl == 5) DS_DW_LDS_LAUNCH(float, 5, 4); else if (t.twl == 4) DS_DW_LDS_LAUNCH(float, 4, 4); else DS_DW_LDS_LAUNCH(float, 3, 4);
        }
#undef DS_DW_LDS_LAUNCH
        DS_CHECK_LAUNCH("dwconv7_lds");
    } else {
        const auto& d = pl.direct;
        if (p->dtype == DS_BF16) hipLaunchKernelGGL(dwconv7_kernel<bf16>, dim3(pl.parts, p->B), dim3(DW_BLOCK), 0, st, *p, d.nstrip, d.CV);
        else hipLaunchKernelGGL(dwconv7_kernel<float>, dim3(pl.parts, p->B), dim3(DW_BLOCK), 0, st, *p, d.nstrip, d.CV);
        DS_CHECK_LAUNCH("dwconv7");
    }
    return DS_OK;
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_dwconv7(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif

extern "C" int ds_pack_dw_weight(const float* w, int C, float* dst, void* stream) {
    DS_REQUIRE(w && dst && C > 0, "pack_dw: bad args");
    hipLaunchKernelGGL(pack_dw_kernel, dim3((49 * C + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), w, C, dst);
    DS_CHECK_LAUNCH("pack_dw");
    return DS_OK;
}

extern "C" int ds_pack_dw_weight_mfma(const float* w, int C, void* dst, void* stream) {
    DS_REQUIRE(w && dst && C > 0, "pack_dw_mfma: bad args");
    const long total = (long)C * 6 * 64 * 8;
    hipLaunchKernelGGL(pack_dw_mfma_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), w, C,
                       reinterpret_cast<bf16*>(dst));
    DS_CHECK_LAUNCH("pack_dw_mfma");
    return DS_OK;
}
