// Device-planned seeded (kBandSeededDev) instantiations of the banded GlobalGotoh fill and walk
// (sa_align_batch_banded_seeded_device, sa_score_batch_banded_seeded_device with SA_GLOBAL_GOTOH): the seeded
// mode with the lists' lengths and every pair's description read from device memory, where the planner
// (sa_band_planner.hip) left them.  kMatchEq and kMatchLut, recording and record-free, every affine variant.
// A translation unit of their own, so the code objects of the other banded units are unchanged.  DESIGN.md §2.20.
#include "sa_banded_affine_fill.h"

namespace sa {
// p.count: the pairs of the chunk (the grid of every variant; blocks past the variant's list return at once).
hipError_t launch_banded_affine_seeded_dev_fill(int variant, bool lut, bool rec, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return lut ? launch_band_sweep<BandAffineFill, SA_GLOBAL_GOTOH, kBandSeededDev, kMatchLut>(variant, rec, p, s)
               : launch_band_sweep<BandAffineFill, SA_GLOBAL_GOTOH, kBandSeededDev, kMatchEq>(variant, rec, p, s);
}

// One launch over the chunk's plan records: a lane per pair, R and L from the pair's variant.
hipError_t launch_banded_affine_seeded_dev_tb(bool lut, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return launch_band_affine_tb<kBandSeededDev>(SA_GLOBAL_GOTOH, lut, p, s);
}
}  // namespace sa
