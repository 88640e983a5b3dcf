// Launcher of the Down / Upsample halo kernel (conv_quad_halo3_kernel.hpp) and its plain-input (bf16 tier) instantiations; the
// split-precision tier's are compiled in conv_quad_halo3_split.hip.
#include "conv_quad_halo3_kernel.hpp"

int ds_conv_quad_halo3_split_run(const ds_conv_params* p, dim3 grid, hipStream_t st);      // conv_quad_halo3_split.hip

int ds_conv_quad_halo3_parts(const ds_conv_params* p) {
    const int twl = halo_twl(p->Wo), TW = 1 << twl, TH = BM >> twl;
    return ((p->Ho + TH - 1) / TH) * ((p->Wo + TW - 1) / TW) * (p->cout_pad / BN);
}

int ds_conv_quad_halo3_launch(const ds_conv_params* p, hipStream_t st) {
    DS_REQUIRE(p->dtype == DS_BF16, "conv_quad_halo3: bf16 only");
    // (ds_conv_params describes a transposed convolution by its 2x2 phases: KH = KW = 2, stride 1, pad 0, Ho x Wo = the input grid)
    DS_REQUIRE(p->transposed ? (p->KH == 2 && p->KW == 2) : (p->KH == 4 && p->KW == 4 && p->pad_h == 1 && p->pad_w == 1 && p->stride == 2),
               "conv_quad_halo3: Conv2d(4, 2, 1) or ConvTranspose2d(4, 2, 1) only");
    const bool split_in = (p->flags & DS_CONV_F_SPLIT_IN) != 0, out_f32 = (p->flags & DS_CONV_F_OUT_F32) != 0;
    DS_REQUIRE((p->flags & ~(DS_CONV_F_SPLIT_IN | DS_CONV_F_OUT_F32)) == 0 && (!out_f32 || p->act == DS_ACT_NONE), "conv_quad_halo3: unsupported flags %d", p->flags);
    DS_REQUIRE(!split_in || p->C0 % 64 == 0, "conv_quad_halo3: split input needs C0 = 2C with C %% 32 == 0");
    const int plane_chunks = split_in ? (p->C0 / 32) * 3 / 2 : p->C0 / 32;
    DS_REQUIRE(p->C1 == 0 && p->C0 % 32 == 0 && ((p->transposed ? 1 : 4) * plane_chunks) % 6 == 0,
               "conv_quad_halo3: single source, Cin %% 32 == 0 and a chunk count that is a multiple of 6 (Cin=%d)", p->C0);
    DS_REQUIRE(p->wk_order == 2 && p->cout_pad % BN == 0, "conv_quad_halo3: quad-packed weights (wk_order = 2), cout_pad %% 96 == 0");
    if (p->transposed) {
        DS_REQUIRE(p->Cout % BN == 0 && p->cout_pad == 4 * p->Cout && p->Ho == p->H && p->Wo == p->W,
                   "conv_quad_halo3: transposed needs Cout %% 96 == 0, cout_pad = 4 Cout and the input grid in Ho / Wo");
    } else {
        DS_REQUIRE(p->H % 2 == 0 && p->W % 2 == 0 && p->Ho == p->H / 2 && p->Wo == p->W / 2, "conv_quad_halo3: strided needs even H, W and Ho = H / 2");
    }
    DS_REQUIRE(!p->gn_ab && !p->gn_part && !p->res && !p->out_nchw_f32 && !p->res_steps, "conv_quad_halo3: no GroupNorm fold, residual or NCHW output");
    const int nchunks = (p->transposed ? 1 : 4) * plane_chunks;
    DS_REQUIRE(p->ksplit <= 1 || (p->slab && nchunks % p->ksplit == 0 && (nchunks / p->ksplit) % 6 == 0),
               "conv_quad_halo3: ksplit=%d needs a slab and slices of a multiple of 6 chunks (%d chunks)", p->ksplit, nchunks);
    const long long oHW = (long long)p->Ho * p->Wo * (p->transposed ? 4 : 1);
    DS_REQUIRE((long long)p->H * p->W * p->C0 * 2 < (1ll << 31) && oHW * p->out_C * (out_f32 ? 4 : 2) < (1ll << 31) &&
                   (long long)(p->transposed ? 1 : 4) * plane_chunks * 4 * p->cout_pad * 64 < (1ll << 31),
               "conv_quad_halo3: one sample / the packed weights must stay below 2 GiB (32-bit buffer offsets)");
    const int twl = halo_twl(p->Wo), TW = 1 << twl, TH = BM >> twl;
    dim3 grid(((p->Ho + TH - 1) / TH) * ((p->Wo + TW - 1) / TW), p->cout_pad / BN, p->B * (p->ksplit > 1 ? p->ksplit : 1));
    return split_in ? ds_conv_quad_halo3_split_run(p, grid, st) : quad_halo3_run<false>(*p, grid, st);
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_conv_quad(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
