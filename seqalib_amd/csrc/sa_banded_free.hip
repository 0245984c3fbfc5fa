// Ends-free (kBandAlgFree) instantiations of the banded NW fill and walk (sa_align_batch_banded_ends_free,
// sa_score_batch_banded_ends_free with SA_NW / SA_HIRSCHBERG): kMatchEq and kMatchLut, recording and
// record-free, every variant.  A translation unit of their own, so sa_banded.hip's code object is unchanged.
// DESIGN.md §2.15.
#include "sa_banded_fill.h"

namespace sa {
hipError_t launch_banded_free_fill(int variant, bool lut, bool rec, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return lut ? launch_band_fill_alg<kBandAlgFree, kMatchLut>(variant, rec, p, s)
               : launch_band_fill_alg<kBandAlgFree, kMatchEq>(variant, rec, p, s);
}

hipError_t launch_banded_free_tb(bool lut, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    const dim3 grid((p.count + 63) / 64), block(64);
    if (lut) hipLaunchKernelGGL((banded_tb_kernel<kBandAlgFree, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((banded_tb_kernel<kBandAlgFree, false>), grid, block, 0, s, p);
    return hipGetLastError();
}
}  // namespace sa
