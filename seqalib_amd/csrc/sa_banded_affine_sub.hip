// Substitution-table (kMatchSub) instantiations of the banded LocalGotoh / GlobalGotoh fill (the matrix
// band calls, sa_align_batch_banded_matrix): a translation unit of their own, so sa_banded_affine.hip's
// code object is unchanged.
#include "sa_banded_affine_fill.h"

namespace sa {
hipError_t launch_banded_affine_fill_sub(int algo, int variant, bool rec, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    if (!p.submat || p.sub_k < 1 || p.sub_k > (uint32_t)kSubMaxSyms) return hipErrorInvalidValue;
    return algo == SA_LOCAL_GOTOH ? launch_band_sweep<BandAffineFill, SA_LOCAL_GOTOH, kBandCorridor, kMatchSub>(variant, rec, p, s)
                                  : launch_band_sweep<BandAffineFill, SA_GLOBAL_GOTOH, kBandCorridor, kMatchSub>(variant, rec, p, s);
}
}  // namespace sa
