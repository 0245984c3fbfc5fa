// Seeded (kBandAlgSeeded) instantiations of the banded NW fill and walk (sa_align_batch_banded_seeded,
// sa_score_batch_banded_seeded with SA_NW / SA_HIRSCHBERG): the ends-free mode with every pair's band
// placed round its seed diagonal.  kMatchEq and kMatchLut, recording and record-free, every variant.
// A translation unit of their own, so the code objects of sa_banded.hip and sa_banded_free.hip are
// unchanged.  DESIGN.md §2.16.
#include "sa_banded_fill.h"

namespace sa {
hipError_t launch_banded_seeded_fill(int variant, bool lut, bool rec, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return lut ? launch_band_fill_alg<kBandAlgSeeded, kMatchLut>(variant, rec, p, s)
               : launch_band_fill_alg<kBandAlgSeeded, kMatchEq>(variant, rec, p, s);
}

hipError_t launch_banded_seeded_tb(bool lut, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    const dim3 grid((p.count + 63) / 64), block(64);
    if (lut) hipLaunchKernelGGL((banded_tb_kernel<kBandAlgSeeded, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((banded_tb_kernel<kBandAlgSeeded, false>), grid, block, 0, s, p);
    return hipGetLastError();
}
}  // namespace sa
