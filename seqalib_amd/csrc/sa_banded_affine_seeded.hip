// Seeded (kBandSeeded) instantiations of the banded GlobalGotoh fill and walk (sa_align_batch_banded_seeded,
// sa_score_batch_banded_seeded with SA_GLOBAL_GOTOH): the ends-free mode with every pair's band placed
// round its seed diagonal, read from behind the launch's idx entries.  kMatchEq and kMatchLut, recording and
// record-free, every affine variant.  A translation unit of their own, so the code objects of
// sa_banded_affine.hip and sa_banded_affine_free.hip are unchanged.  DESIGN.md §2.16.
#include "sa_banded_affine_fill.h"

namespace sa {
hipError_t launch_banded_affine_seeded_fill(int variant, bool lut, bool rec, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return lut ? launch_band_sweep<BandAffineFill, SA_GLOBAL_GOTOH, kBandSeeded, kMatchLut>(variant, rec, p, s)
               : launch_band_sweep<BandAffineFill, SA_GLOBAL_GOTOH, kBandSeeded, kMatchEq>(variant, rec, p, s);
}

hipError_t launch_banded_affine_seeded_tb(bool lut, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return launch_band_affine_tb<kBandSeeded>(SA_GLOBAL_GOTOH, lut, p, s);
}
}  // namespace sa
