// sa_banded.hip — banded Needleman-Wunsch / Smith-Waterman (sa_align_batch_banded,
// sa_score_batch_banded): an anti-diagonal sweep over the in-band cells only, the whole band of a
// pair in the registers of one wave (or of 16 / 32 lanes of it), 2-bit direction records laid out by
// anti-diagonal, and a one-lane-per-pair walk over them.  DESIGN.md §2.11.  The fill template lives
// in sa_banded_fill.h; this unit holds its kMatchEq / kMatchLut instantiations and the walk, which
// the matrix band calls use too (on symbol codes, with the label bit table over codes).
#include "sa_banded_fill.h"

namespace sa {
namespace {

// The walk: one lane per pair over the 2-bit records (0 stop, 1 diagonal, 2 up, 3 left).
template <int ALG, bool LUT>
__global__ __launch_bounds__(64) void banded_tb_kernel(BandParams P) {
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= P.count) return;
    const uint32_t pair = P.idx[q];
    const uint64_t a1 = P.off1[pair], a2 = P.off2[pair];
    const int32_t m = (int32_t)(P.off1[pair + 1] - a1), n = (int32_t)(P.off2[pair + 1] - a2);
    const uint8_t* s1 = P.seq1 + a1;
    const uint8_t* s2 = P.seq2 + a2;
    const BandGeom bg = band_geom(m, n, (int32_t)P.band);
    const uint32_t* rec = P.rec + P.recoff[q];
    sa_result* res = P.res + pair;
    uint8_t* ops = P.ops + a1 + a2 + pair;
    const int R = P.R, L = P.L, S = R <= 16 ? 16 / R : 1;
    int32_t i = res->end_i, j = res->end_j;
    if (ALG == SA_SW && (m == 0 || n == 0)) i = j = 0;
    if (i < 0 || i > m || j < 0 || j > n) i = j = 0;   // (never: the fill's end cell is a cell)
    uint32_t nops = 0;
    while (i > 0 || j > 0) {
        if (ALG == SA_SW) {
            if (i == 0 || j == 0) break;
        } else {
            if (i == 0) { ops[nops++] = 'L'; --j; continue; }
            if (j == 0) { ops[nops++] = 'U'; --i; continue; }
        }
        const int32_t tp = i + j - bg.lo - bg.tb, c = j - i - bg.lo;
        if (c < 0 || c >= bg.beff) break;   // (never: the walk stays inside the band)
        const int32_t l = c / (2 * R), rr = (c % (2 * R)) >> 1;
        uint32_t w;
        if (R <= 16) w = rec[(uint64_t)(tp / S) * L + l] >> (((tp % S) * R + rr) * 2);
        else w = rec[((uint64_t)tp * 2 + (rr >> 4)) * L + l] >> ((rr & 15) * 2);
        const uint32_t code = w & 3u;
        if (code == 0) break;
        if (code == 1) {
            const uint32_t a = s1[i - 1], b = s2[j - 1];
            const bool v = LUT ? ((P.lutbits[(a << 3) | (b >> 5)] >> (b & 31)) & 1u) != 0 : a == b;
            ops[nops++] = (v || P.allow) ? (v ? 'M' : 'S') : 'X';
            --i;
            --j;
        } else if (code == 2) {
            ops[nops++] = 'U';
            --i;
        } else {
            ops[nops++] = 'L';
            --j;
        }
    }
    res->start_i = i;
    res->start_j = j;
    res->nops = nops;
    res->flags = 0;
    res->reserved = 0;
}

}  // namespace

hipError_t launch_banded_fill(int algo, int variant, int mm, bool rec, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    if (mm == kMatchSub) return launch_banded_fill_sub(algo, variant, rec, p, s);
    if (mm == kMatchLut)
        return algo == SA_SW ? launch_band_fill_alg<SA_SW, kMatchLut>(variant, rec, p, s)
                             : launch_band_fill_alg<SA_NW, kMatchLut>(variant, rec, p, s);
    return algo == SA_SW ? launch_band_fill_alg<SA_SW, kMatchEq>(variant, rec, p, s)
                         : launch_band_fill_alg<SA_NW, kMatchEq>(variant, rec, p, s);
}

hipError_t launch_banded_tb(int algo, bool lut, const BandParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    const dim3 grid((p.count + 63) / 64), block(64);
    if (algo == SA_SW) {
        if (lut) hipLaunchKernelGGL((banded_tb_kernel<SA_SW, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((banded_tb_kernel<SA_SW, false>), grid, block, 0, s, p);
    } else {
        if (lut) hipLaunchKernelGGL((banded_tb_kernel<SA_NW, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((banded_tb_kernel<SA_NW, false>), grid, block, 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace sa
