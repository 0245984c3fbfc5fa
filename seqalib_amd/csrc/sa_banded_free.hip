// Ends-free (kBandFree) instantiations of the banded NW fill and walk (sa_align_batch_banded_ends_free,
// sa_score_batch_banded_ends_free with SA_NW / SA_HIRSCHBERG): kMatchEq and kMatchLut, recording and
// record-free, every variant.  A translation unit of their own, so sa_banded.hip's code object is unchanged.
// DESIGN.md §2.15.
#include "sa_banded_fill.h"

namespace sa {
hipError_t launch_banded_free_fill(int variant, bool lut, bool rec, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return lut ? launch_band_sweep<BandFill, SA_NW, kBandFree, kMatchLut>(variant, rec, p, s)
               : launch_band_sweep<BandFill, SA_NW, kBandFree, kMatchEq>(variant, rec, p, s);
}

hipError_t launch_banded_free_tb(bool lut, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return launch_band_tb<kBandFree>(SA_NW, lut, p, s);
}
}  // namespace sa
