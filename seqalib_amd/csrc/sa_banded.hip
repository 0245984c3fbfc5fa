// sa_banded.hip — banded Needleman-Wunsch / Smith-Waterman (sa_align_batch_banded,
// sa_score_batch_banded): an anti-diagonal sweep over the in-band cells only, the whole band of a
// pair in the registers of one wave (or of 16 / 32 lanes of it), 2-bit direction records laid out by
// anti-diagonal, and a one-lane-per-pair walk over them.  DESIGN.md §2.11.  The fill template
// and the walk template live in sa_banded_fill.h; this unit holds the fill's kMatchEq / kMatchLut
// instantiations and the walk's, which the matrix band calls use too (on symbol codes, with the label
// bit table over codes).
#include "sa_banded_fill.h"

namespace sa {

hipError_t launch_banded_fill(int algo, int variant, int mm, bool rec, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    if (mm == kMatchSub) return launch_banded_fill_sub(algo, variant, rec, p, s);
    if (mm == kMatchLut)
        return algo == SA_SW ? launch_band_fill_alg<SA_SW, kMatchLut>(variant, rec, p, s)
                             : launch_band_fill_alg<SA_NW, kMatchLut>(variant, rec, p, s);
    return algo == SA_SW ? launch_band_fill_alg<SA_SW, kMatchEq>(variant, rec, p, s)
                         : launch_band_fill_alg<SA_NW, kMatchEq>(variant, rec, p, s);
}

hipError_t launch_banded_tb(int algo, bool lut, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    const dim3 grid((p.count + 63) / 64), block(64);
    if (algo == SA_SW) {
        if (lut) hipLaunchKernelGGL((banded_tb_kernel<SA_SW, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((banded_tb_kernel<SA_SW, false>), grid, block, 0, s, p);
    } else {
        if (lut) hipLaunchKernelGGL((banded_tb_kernel<SA_NW, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((banded_tb_kernel<SA_NW, false>), grid, block, 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace sa
