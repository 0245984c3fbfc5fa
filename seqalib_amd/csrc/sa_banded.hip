// sa_banded.hip — banded Needleman-Wunsch / Smith-Waterman (sa_align_batch_banded,
// sa_score_batch_banded): an anti-diagonal sweep over the in-band cells only, the whole band of a
// pair in the registers of one wave (or of 16 / 32 lanes of it), 2-bit direction records laid out by
// anti-diagonal, and a one-lane-per-pair walk over them.  DESIGN.md §2.11.  The sweep lives in
// sa_band_sweep.h, the cell and the walk in sa_banded_fill.h; this unit holds the corridor's kMatchEq /
// kMatchLut fills and its walks, which the matrix band calls use too (on symbol codes, with the label
// bit table over codes).
#include "sa_banded_fill.h"

namespace sa {

hipError_t launch_banded_fill(int algo, int variant, int mm, bool rec, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    if (mm == kMatchSub) return launch_banded_fill_sub(algo, variant, rec, p, s);
    if (mm == kMatchLut)
        return algo == SA_SW ? launch_band_sweep<BandFill, SA_SW, kBandCorridor, kMatchLut>(variant, rec, p, s)
                             : launch_band_sweep<BandFill, SA_NW, kBandCorridor, kMatchLut>(variant, rec, p, s);
    return algo == SA_SW ? launch_band_sweep<BandFill, SA_SW, kBandCorridor, kMatchEq>(variant, rec, p, s)
                         : launch_band_sweep<BandFill, SA_NW, kBandCorridor, kMatchEq>(variant, rec, p, s);
}

hipError_t launch_banded_tb(int algo, bool lut, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return launch_band_tb<kBandCorridor>(algo, lut, p, s);
}

}  // namespace sa
