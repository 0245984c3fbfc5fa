// Extension instantiations of the banded GlobalGotoh fill (sa_align_batch_banded_extend,
// sa_score_batch_banded_extend with SA_GLOBAL_GOTOH): GlobalGotoh anchored at (0, 0) in the band round
// diagonal 0, free to end at any interior cell, with the X-drop test and its early exit (kMatchExtBit).
// kMatchEq and kMatchLut, recording and record-free, every affine variant, and their walk.  A translation
// unit of their own, so the code objects of the other banded affine units are unchanged.  DESIGN.md §2.18.
#include "sa_banded_affine_fill.h"

namespace sa {
namespace {

// The extension walk: banded_affine_seeded_tb_kernel (sa_banded_affine_seeded.hip) on the band round
// diagonal 0, with no free begin -- it walks to (0, 0) -- and the fill's SA_FLAG_DROPPED kept.  A kernel
// of its own for that kernel's reason.
template <bool LUT>
__global__ __launch_bounds__(64) void banded_affine_extend_tb_kernel(BandAffineParams P) {
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= P.count) return;
    const uint32_t pair = P.idx[q];
    const uint64_t a1 = P.off1[pair], a2 = P.off2[pair];
    const int32_t m = (int32_t)(P.off1[pair + 1] - a1), n = (int32_t)(P.off2[pair + 1] - a2);
    const uint8_t* s1 = P.seq1 + a1;
    const uint8_t* s2 = P.seq2 + a2;
    const BandGeom bg = band_geom_seeded(m, n, (int32_t)P.band, 0);
    const uint32_t* rec = P.rec + P.recoff[q];
    sa_result* res = P.res + pair;
    uint8_t* ops = P.ops + a1 + a2 + pair;
    const int R = P.R, L = P.L, S = R <= 8 ? 8 / R : 1, WPS = R <= 8 ? 1 : R / 8;
    int32_t i = res->end_i, j = res->end_j;
    if (i < 0 || i > m || j < 0 || j > n) i = j = 0;   // (never: the fill's end cell is a cell)
    uint32_t nops = 0;
    const uint32_t cap = (uint32_t)(m + n);            // (never reached: every op consumes a symbol)
    int type = 0;
    while ((i > 0 || j > 0) && nops < cap) {
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
    res->flags &= SA_FLAG_DROPPED;   // (the fill's flag)
    res->reserved = 0;
}

}  // namespace

hipError_t launch_banded_affine_extend_fill(int variant, bool lut, bool rec, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    return lut ? launch_band_affine_fill_alg<false, kMatchLut | kMatchExtBit>(variant, rec, p, s)
               : launch_band_affine_fill_alg<false, kMatchEq | kMatchExtBit>(variant, rec, p, s);
}

hipError_t launch_banded_affine_extend_tb(bool lut, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    const dim3 grid((p.count + 63) / 64), block(64);
    if (lut) hipLaunchKernelGGL((banded_affine_extend_tb_kernel<true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((banded_affine_extend_tb_kernel<false>), grid, block, 0, s, p);
    return hipGetLastError();
}
}  // namespace sa
