// Substitution-table (kMatchSub) instantiations of the banded SW / NW fill (the matrix band calls,
// sa_align_batch_banded_matrix): a translation unit of their own, so sa_banded.hip's code object is unchanged.
#include "sa_banded_fill.h"

namespace sa {
hipError_t launch_banded_fill_sub(int algo, int variant, bool rec, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    if (!p.submat || p.sub_k < 1 || p.sub_k > (uint32_t)kSubMaxSyms) return hipErrorInvalidValue;
    return algo == SA_SW ? launch_band_sweep<BandFill, SA_SW, kBandCorridor, kMatchSub>(variant, rec, p, s)
                         : launch_band_sweep<BandFill, SA_NW, kBandCorridor, kMatchSub>(variant, rec, p, s);
}
}  // namespace sa
