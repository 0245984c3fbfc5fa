// Record-free substitution-table (kMatchSub) fill instantiations for SA_NW (sa_score_batch_matrix),
// beside sa_fill_nw_sub.hip as sa_fill_nw_score.hip stands beside sa_fill_nw.hip.
#include "sa_fill_impl.h"

namespace sa {
hipError_t launch_fill_nw_sub_score(const FillVariant& v, const FillParams& p, uint32_t grid, hipStream_t s) {
    return launch_fill_sub_alg<SA_NW, true>(v, p, grid, s);
}
}  // namespace sa
