// Launcher of the 3x3 halo kernel (conv3x3_halo3_kernel.hpp) and its bf16 instantiations; the split-precision instantiations are compiled
// in conv3x3_halo3_hp.hip.
#include "conv3x3_halo3_kernel.hpp"

int ds_conv3x3_halo3_hp_run(const ds_conv_params* p, dim3 grid, bool pair, hipStream_t st);      // conv3x3_halo3_hp.hip

// statistics partials of a whole-K launch: one per block (pixel tile x N-block)
int ds_conv3x3_halo3_parts(const ds_conv_params* p) {
    const int twl = halo_twl(p->W), TW = 1 << twl, TH = BM >> twl;
    return ((p->H + TH - 1) / TH) * ((p->W + TW - 1) / TW) * (p->cout_pad / BN);
}

// The batch the pair predicate below looks at: ds_conv_params.batch_hint where the caller gives one, else B.
static int halo3_batch(const ds_conv_params* p) { return p->batch_hint > 0 ? p->batch_hint : p->B; }

int ds_conv3x3_halo3_launch(const ds_conv_params* p, hipStream_t st) {
    DS_REQUIRE(p->dtype == DS_BF16, "conv3x3_halo3: bf16 only");
    DS_REQUIRE(p->KH == 3 && p->KW == 3 && p->stride == 1 && p->pad_h == 1 && p->pad_w == 1 && !p->transposed,
               "conv3x3_halo3: 3x3 stride 1 pad 1 only");
    DS_REQUIRE(p->C1 == 0 && p->C0 % 32 == 0, "conv3x3_halo3: single source, Cin multiple of 32 (got %d+%d)", p->C0, p->C1);
    DS_REQUIRE(p->Ho == p->H && p->Wo == p->W && !p->out_nchw_f32, "conv3x3_halo3: same-size NHWC output only");
    DS_REQUIRE(p->cout_pad % BN == 0 && p->wk_order == 1, "conv3x3_halo3: cout_pad %% 96 == 0 and chunk-major weights (wk_order = 1)");
    const bool split_in = (p->flags & DS_CONV_F_SPLIT_IN) != 0;
    // (K slices of a split input are whole source chunks = triples of virtual chunks: C0 = 2C, C / 32 source chunks)
    DS_REQUIRE(p->ksplit <= 1 || (p->slab && (p->flags == 0 || split_in) && ((split_in ? p->C0 / 64 : p->C0 / 32) % p->ksplit) == 0 && !p->res_steps),
               "conv3x3_halo3: ksplit=%d needs a slab, must divide the %d source chunks and excludes the fused res_conv", p->ksplit, split_in ? p->C0 / 64 : p->C0 / 32);
    const int out_mode = (p->flags >> 1) & 3;
    DS_REQUIRE(out_mode <= 2 && (p->flags & ~7) == 0, "conv3x3_halo3: unknown flags %d", p->flags);
    DS_REQUIRE(!split_in || (p->C0 % 64 == 0 && !p->res_steps), "conv3x3_halo3: split input needs C0 = 2C with C %% 32 == 0 and no fused res_conv");
    DS_REQUIRE(p->flags == 0 || split_in, "conv3x3_halo3: the split-precision launches (flags != 0) take a split input (DS_CONV_F_SPLIT_IN)");
    DS_REQUIRE(out_mode == 0 || !p->res_steps, "conv3x3_halo3: split / fp32 output excludes the fused res_conv");
    DS_REQUIRE(out_mode != 2 || p->act == DS_ACT_NONE, "conv3x3_halo3: fp32 output has no activation variant");
    DS_REQUIRE(!p->res || out_mode == 2 || p->flags == 0, "conv3x3_halo3: in the split-precision modes a residual needs the fp32 output");
    DS_REQUIRE(out_mode != 1 || p->out_C >= p->out_c0 + 2 * p->Cout, "conv3x3_halo3: split output needs out_C >= 2 Cout");
    const int nchunks = split_in ? (p->C0 / 32) * 3 / 2 : p->C0 / 32;
    if (p->res_steps) {
        DS_REQUIRE(!p->res, "conv3x3_halo3: a fused res_conv excludes a residual tensor");
        DS_REQUIRE(p->res_src0 && p->res_C0 > 0 && p->res_C0 % 32 == 0 && p->res_C1 % 32 == 0 && p->res_steps == (p->res_C0 + p->res_C1) / 32 &&
                       p->res_steps % 3 == 0,
                   "conv3x3_halo3: res_conv channels (%d,%d) must be multiples of 32 (96 in total) and res_steps = their chunks", p->res_C0, p->res_C1);
        DS_REQUIRE(p->res_C1 == 0 || (p->res_src1 && p->res_H1 > 0 && p->res_W1 > 0), "conv3x3_halo3: second res_conv source incomplete");
        DS_REQUIRE(ds_aligned16(p->res_src0) && (!p->res_C1 || ds_aligned16(p->res_src1)), "conv3x3_halo3: res_conv sources must be 16-byte aligned");
    }
    DS_REQUIRE((long long)p->H * p->W * (p->C0 > p->res_C0 ? p->C0 : p->res_C0) * 2 < (1ll << 31) &&
                   (long long)(nchunks * 9 + p->res_steps) * p->cout_pad * 64 < (1ll << 31),
               "conv3x3_halo3: one sample / the packed weights must stay below 2 GiB (32-bit buffer offsets)");
    DS_REQUIRE((long long)p->H * p->W * p->out_C * (out_mode == 2 ? 4 : 2) < (1ll << 31), "conv3x3_halo3: one output sample must stay below 2 GiB (32-bit buffer offsets)");
    const int twl = halo_twl(p->W), TW = 1 << twl, TH = BM >> twl;
    // r05: two samples per block where an image fills at most half of the 8 x 32 tile (the deepest level at 128 x 64 latents: 16 x 8) — by
    // the batch the caller decides from (halo3_batch), so that a sample gets the same kernel in every batch; a lone last sample (B odd, or
    // B = 1 under a larger batch_hint) has its block to itself
    const bool pair = p->flags != 0 && twl == 3 && 2 * p->H <= TH && p->W <= TW && p->ksplit <= 1 && !p->res_steps && halo3_batch(p) >= 2;
    dim3 grid(((p->H + TH - 1) / TH) * ((p->W + TW - 1) / TW), p->cout_pad / BN, pair ? (p->B + 1) / 2 : p->B * (p->ksplit > 1 ? p->ksplit : 1));
    {
        static DsDevOnce once;                               // the GELU table of this device (module-scope __device__ array)
        int dev;
        if (once.need(&dev)) {
            float h[GELU_TAB_N];
            auto T = [](double a) { return a * 0.5 * erfc(a * 0.70710678118654752440); };
            for (int i = 0; i < GELU_TAB_N; ++i) {
                const unsigned lo = (unsigned)(GELU_TAB_BASE + i) << 16, hi = lo + 0x10000u;        // the bucket [lo, hi) of fp32 patterns
                float flo, fhi;
                memcpy(&flo, &lo, 4);
                memcpy(&fhi, &hi, 4);
                h[i] = (float)T(0.5 * ((double)flo + (double)fhi));
            }
            hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_gelu_lut), h, sizeof(h));
            if (e != hipSuccess) DS_FAIL(DS_ELAUNCH, "conv3x3_halo3: GELU table upload: %s", hipGetErrorString(e));
            once.done(dev);
        }
    }
    return p->flags ? ds_conv3x3_halo3_hp_run(p, grid, pair, st) : halo3_run<false>(*p, grid, false, st);
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_conv_halo3(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
