// Substitution-table (kMatchSub) fill instantiations for SA_GLOBAL_GOTOH (the matrix calls,
// sa_align_batch_matrix): a translation unit of their own, so sa_fill_gg.hip's code object is unchanged.
#include "sa_fill_impl.h"

namespace sa {
hipError_t launch_fill_gg_sub(const FillVariant& v, const FillParams& p, uint32_t grid, hipStream_t s) {
    return launch_fill_sub_alg<SA_GLOBAL_GOTOH, false>(v, p, grid, s);
}
}  // namespace sa
