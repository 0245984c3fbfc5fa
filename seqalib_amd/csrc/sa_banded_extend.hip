// Extension (kBandExtend) instantiations of the banded NW fill and walk (sa_align_batch_banded_extend,
// sa_score_batch_banded_extend with SA_NW / SA_HIRSCHBERG): NW anchored at (0, 0) in the band round
// diagonal 0, free to end at any interior cell, with the X-drop test and its early exit.  kMatchEq and
// kMatchLut, recording and record-free, every variant.  A translation unit of their own, so the code
// objects of the other banded units are unchanged.  DESIGN.md §2.18.
#include "sa_banded_fill.h"

namespace sa {
hipError_t launch_banded_extend_fill(int variant, bool lut, bool rec, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return lut ? launch_band_sweep<BandFill, SA_NW, kBandExtend, kMatchLut>(variant, rec, p, s)
               : launch_band_sweep<BandFill, SA_NW, kBandExtend, kMatchEq>(variant, rec, p, s);
}

hipError_t launch_banded_extend_tb(bool lut, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return launch_band_tb<kBandExtend>(SA_NW, lut, p, s);
}
}  // namespace sa
