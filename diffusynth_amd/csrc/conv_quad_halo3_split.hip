// Down / Upsample halo kernel (conv_quad_halo3_kernel.hpp): the split-precision tier's instantiations (hi / lo input planes,
// DS_CONV_F_SPLIT_IN), launched by ds_conv_quad_halo3_launch (conv_quad_halo3.hip).
#include "conv_quad_halo3_kernel.hpp"

int ds_conv_quad_halo3_split_run(const ds_conv_params* p, dim3 grid, hipStream_t st) { return quad_halo3_run<true>(*p, grid, st); }

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_conv_quad_split(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
