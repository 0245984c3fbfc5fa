// Device-planned seeded (kBandSeededDev) instantiations of the banded NW fill and walk
// (sa_align_batch_banded_seeded_device, sa_score_batch_banded_seeded_device with SA_NW / SA_HIRSCHBERG): the
// seeded mode with the lists' lengths and every pair's description read from device memory, where the planner
// (sa_band_planner.hip) left them.  kMatchEq and kMatchLut, recording and record-free, every variant.  A
// translation unit of their own, so the code objects of the other banded units are unchanged.  DESIGN.md §2.20.
#include "sa_banded_fill.h"

namespace sa {
// p.count: the pairs of the chunk.  The grid covers that many pairs in this variant; the blocks past the
// variant's list return at once.
hipError_t launch_banded_seeded_dev_fill(int variant, bool lut, bool rec, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return lut ? launch_band_sweep<BandFill, SA_NW, kBandSeededDev, kMatchLut>(variant, rec, p, s)
               : launch_band_sweep<BandFill, SA_NW, kBandSeededDev, kMatchEq>(variant, rec, p, s);
}

// One launch over the chunk's plan records: a lane per pair, R and L from the pair's variant.
hipError_t launch_banded_seeded_dev_tb(bool lut, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return launch_band_tb<kBandSeededDev>(SA_NW, lut, p, s);
}
}  // namespace sa
