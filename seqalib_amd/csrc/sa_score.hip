// sa_score.hip — what the score calls (sa_score_batch*) run besides the fills: the dispatch to the
// record-free int32 fills and the kernel that stands in for the walks' bookkeeping.
#include "sa_internal.h"

namespace sa {

hipError_t launch_fill_score(int algo, const FillVariant& v, const FillParams& p, uint32_t grid, hipStream_t stream) {
    switch (algo) {
        case SA_SW: return launch_fill_sw_score(v, p, grid, stream);
        case SA_NW: return launch_fill_nw_score(v, p, grid, stream);
        case SA_LOCAL_GOTOH: return launch_fill_lg_score(v, p, grid, stream);
        case SA_GLOBAL_GOTOH: return launch_fill_gg_score(v, p, grid, stream);
        default: return hipErrorInvalidValue;
    }
}

// One thread per pair.  A walk clears the internal flags of the pair it walked (tb_clear_mask) and
// the end-cell replay's chunk word; with no walk this kernel does, and it writes the contract's
// start = (-1, -1), nops = 0.  SA_FLAG_BAD_SHAPE (and an SA_FLAG_TIMEOUT no fallback re-ran, tests)
// stay as the fills left them.
__global__ __launch_bounds__(256) void score_finish_kernel(sa_result* res, uint32_t pair_base, uint32_t count) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= count) return;
    sa_result r = res[pair_base + q];
    r.start_i = -1;
    r.start_j = -1;
    r.nops = 0;
    r.flags &= ~(kFlagRetry | kFlagRerun | kFlagRedo);
    r.reserved = 0;
    res[pair_base + q] = r;
}

hipError_t launch_score_finish(sa_result* res, uint32_t pair_base, uint32_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(score_finish_kernel, dim3((count + 255) / 256), dim3(256), 0, s, res, pair_base, count);
    return hipGetLastError();
}

}  // namespace sa
