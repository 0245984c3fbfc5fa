// Device-planned seeded instantiations of the banded GlobalGotoh fill (sa_align_batch_banded_seeded_device,
// sa_score_batch_banded_seeded_device with SA_GLOBAL_GOTOH): the seeded mode (kMatchFreeBit | kMatchSeedBit)
// with kMatchPlanBit -- the lists' lengths and every pair's description are read from device memory, where
// the planner (sa_band_planner.hip) left them.  kMatchEq and kMatchLut, recording and record-free, every
// affine variant, and their walk.  A translation unit of their own, so the code objects of the other banded
// units are unchanged.  DESIGN.md §2.20.
#include "sa_banded_affine_fill.h"

namespace sa {
namespace {

// The planned walk: banded_affine_seeded_tb_kernel (sa_banded_affine_seeded.hip) over the chunk's plan
// records, one launch for every variant: R and L are the pair's own.  A kernel of its own for that kernel's
// reason.
template <bool LUT>
__global__ __launch_bounds__(64) void banded_affine_seeded_dev_tb_kernel(BandAffineParams P) {
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= P.count) return;
    const BandPlanRec& pr = reinterpret_cast<const BandPlanRec*>(P.off1)[q];
    if (pr.v < 0) return;   // refused by the planner: its result is written, it has no ops
    const int32_t m = pr.m, n = pr.n;
    const uint8_t* s1 = pr.s1;
    const uint8_t* s2 = pr.s2;
    const BandGeom bg = band_geom_seeded(m, n, (int32_t)P.band, pr.diag);
    const uint32_t* rec = P.rec + pr.recoff;
    sa_result* res = P.res + pr.pair;
    uint8_t* ops = P.ops + pr.opsoff;
    const int R = kBandR[pr.v], L = kBandL[pr.v], S = R <= 8 ? 8 / R : 1, WPS = R <= 8 ? 1 : R / 8;
    const bool stop_i0 = (P.free_ends & kFreeSeq2Begin) != 0, stop_j0 = (P.free_ends & kFreeSeq1Begin) != 0;
    int32_t i = res->end_i, j = res->end_j;
    if (i < 0 || i > m || j < 0 || j > n) i = j = 0;   // (never: the fill's end cell is a cell)
    uint32_t nops = 0;
    const uint32_t cap = (uint32_t)(m + n);            // (never reached: every op consumes a symbol)
    int type = 0;
    while ((i > 0 || j > 0) && nops < cap) {
        if ((i == 0 && stop_i0) || (j == 0 && stop_j0)) break;
        if (i == 0) { ops[nops++] = 'L'; --j; continue; }
        if (j == 0) { ops[nops++] = 'U'; --i; continue; }
        const int32_t tp = i + j - bg.lo - bg.tb, c = j - i - bg.lo;
        if (c < 0 || c >= bg.beff) break;   // (never: the walk stays inside the band)
        const int32_t l = c / (2 * R), rr = (c % (2 * R)) >> 1;
        uint32_t w;
        if (R <= 8) w = rec[(uint64_t)(tp / S) * L + l] >> (((tp % S) * R + rr) * 4);
        else w = rec[((uint64_t)tp * WPS + (rr >> 3)) * L + l] >> ((rr & 7) * 4);
        if (type == 0) {
            const uint32_t code = w & 3u;
            if (code == 0) break;   // (never: a global cell's M has a source)
            if (code == 1) {
                const uint32_t a = s1[i - 1], b = s2[j - 1];
                const bool v = LUT ? ((P.lutbits[(a << 3) | (b >> 5)] >> (b & 31)) & 1u) != 0 : a == b;
                ops[nops++] = (v || P.allow) ? (v ? 'M' : 'S') : 'X';
                --i;
                --j;
                continue;
            }
            type = (int)code - 1;
        }
        if (type == 1) {
            ops[nops++] = 'U';
            --i;
            if (!(w & 4u)) type = 0;
        } else {
            ops[nops++] = 'L';
            --j;
            if (!(w & 8u)) type = 0;
        }
    }
    res->start_i = i;
    res->start_j = j;
    res->nops = nops;
    res->flags = 0;
    res->reserved = 0;
}

}  // namespace

// p.count: the pairs of the chunk (the grid of every variant; blocks past the variant's list return at once).
hipError_t launch_banded_affine_seeded_dev_fill(int variant, bool lut, bool rec, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    constexpr int kMode = kMatchFreeBit | kMatchSeedBit | kMatchPlanBit;
    return lut ? launch_band_affine_fill_alg<false, kMatchLut | kMode>(variant, rec, p, s)
               : launch_band_affine_fill_alg<false, kMatchEq | kMode>(variant, rec, p, s);
}

hipError_t launch_banded_affine_seeded_dev_tb(bool lut, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    const dim3 grid((p.count + 63) / 64), block(64);
    if (lut) hipLaunchKernelGGL((banded_affine_seeded_dev_tb_kernel<true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((banded_affine_seeded_dev_tb_kernel<false>), grid, block, 0, s, p);
    return hipGetLastError();
}
}  // namespace sa
