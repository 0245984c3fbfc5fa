// Seeded (kBandSeeded) instantiations of the banded NW fill and walk (sa_align_batch_banded_seeded,
// sa_score_batch_banded_seeded with SA_NW / SA_HIRSCHBERG): the ends-free mode with every pair's band
// placed round its seed diagonal.  kMatchEq and kMatchLut, recording and record-free, every variant.
// A translation unit of their own, so the code objects of sa_banded.hip and sa_banded_free.hip are
// unchanged.  DESIGN.md §2.16.
#include "sa_banded_fill.h"

namespace sa {
hipError_t launch_banded_seeded_fill(int variant, bool lut, bool rec, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return lut ? launch_band_sweep<BandFill, SA_NW, kBandSeeded, kMatchLut>(variant, rec, p, s)
               : launch_band_sweep<BandFill, SA_NW, kBandSeeded, kMatchEq>(variant, rec, p, s);
}

hipError_t launch_banded_seeded_tb(bool lut, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return launch_band_tb<kBandSeeded>(SA_NW, lut, p, s);
}
}  // namespace sa
