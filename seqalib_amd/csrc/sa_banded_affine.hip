// sa_banded_affine.hip — banded LocalGotoh / GlobalGotoh (sa_align_batch_banded_affine,
// sa_score_batch_banded_affine): the anti-diagonal sweep of sa_banded.hip with three values per cell
// (M, X vertical, Y horizontal), 4-bit records laid out by anti-diagonal, and a one-lane-per-pair walk
// that carries the reference's `type` state over them.  DESIGN.md §2.13.
// The sweep lives in sa_band_sweep.h, the cell and the walk in sa_banded_affine_fill.h; this unit holds
// the corridor's kMatchEq / kMatchLut fills and its walks, which the matrix band calls use too (on symbol
// codes, with the label bit table over codes).
#include "sa_banded_affine_fill.h"

namespace sa {

hipError_t launch_banded_affine_fill(int algo, int variant, int mm, bool rec, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    if (mm == kMatchSub) return launch_banded_affine_fill_sub(algo, variant, rec, p, s);
    if (mm == kMatchLut)
        return algo == SA_LOCAL_GOTOH ? launch_band_sweep<BandAffineFill, SA_LOCAL_GOTOH, kBandCorridor, kMatchLut>(variant, rec, p, s)
                                      : launch_band_sweep<BandAffineFill, SA_GLOBAL_GOTOH, kBandCorridor, kMatchLut>(variant, rec, p, s);
    return algo == SA_LOCAL_GOTOH ? launch_band_sweep<BandAffineFill, SA_LOCAL_GOTOH, kBandCorridor, kMatchEq>(variant, rec, p, s)
                                  : launch_band_sweep<BandAffineFill, SA_GLOBAL_GOTOH, kBandCorridor, kMatchEq>(variant, rec, p, s);
}

hipError_t launch_banded_affine_tb(int algo, bool lut, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return launch_band_affine_tb<kBandCorridor>(algo, lut, p, s);
}

}  // namespace sa
