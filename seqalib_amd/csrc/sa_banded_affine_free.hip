// Ends-free (kBandFree) instantiations of the banded GlobalGotoh fill and walk (sa_align_batch_banded_ends_free,
// sa_score_batch_banded_ends_free with SA_GLOBAL_GOTOH): kMatchEq and kMatchLut, recording and
// record-free, every affine variant.  A translation unit of their own, so sa_banded_affine.hip's code
// object is unchanged.  DESIGN.md §2.15.
#include "sa_banded_affine_fill.h"

namespace sa {
hipError_t launch_banded_affine_free_fill(int variant, bool lut, bool rec, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return lut ? launch_band_sweep<BandAffineFill, SA_GLOBAL_GOTOH, kBandFree, kMatchLut>(variant, rec, p, s)
               : launch_band_sweep<BandAffineFill, SA_GLOBAL_GOTOH, kBandFree, kMatchEq>(variant, rec, p, s);
}

hipError_t launch_banded_affine_free_tb(bool lut, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return launch_band_affine_tb<kBandFree>(SA_GLOBAL_GOTOH, lut, p, s);
}
}  // namespace sa
