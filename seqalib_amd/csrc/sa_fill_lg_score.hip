// Record-free int32 fill instantiations for SA_LOCAL_GOTOH (the score calls, sa_score_batch*): one translation
// unit per algorithm, beside sa_fill_lg.hip, so the parallel build time stays flat.
#include "sa_fill_impl.h"

namespace sa {
hipError_t launch_fill_lg_score(const FillVariant& v, const FillParams& p, uint32_t grid, hipStream_t s) {
    return launch_fill_int32<SA_LOCAL_GOTOH, true>(v, p, grid, s);
}
}  // namespace sa
