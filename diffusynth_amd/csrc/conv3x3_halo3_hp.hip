// 3x3 halo kernel (conv3x3_halo3_kernel.hpp): the split-precision instantiations (ds_conv_params.flags != 0; the three tile widths and
// the two-samples-per-block form of the 8-wide tile), launched by ds_conv3x3_halo3_launch (conv3x3_halo3.hip).
#include "conv3x3_halo3_kernel.hpp"

int ds_conv3x3_halo3_hp_run(const ds_conv_params* p, dim3 grid, bool pair, hipStream_t st) { return halo3_run<true>(*p, grid, pair, st); }

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_conv_halo3_hp(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
