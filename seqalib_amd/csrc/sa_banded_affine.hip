// sa_banded_affine.hip — banded LocalGotoh / GlobalGotoh (sa_align_batch_banded_affine,
// sa_score_batch_banded_affine): the anti-diagonal sweep of sa_banded.hip with three values per cell
// (M, X vertical, Y horizontal), 4-bit records laid out by anti-diagonal, and a one-lane-per-pair walk
// that carries the reference's `type` state over them.  DESIGN.md §2.13.
// The fill template lives in sa_banded_affine_fill.h (geometry, register mapping, records); this
// unit holds its kMatchEq / kMatchLut instantiations and the walk, which the matrix band calls use
// too (on symbol codes, with the label bit table over codes).
#include "sa_banded_affine_fill.h"

namespace sa {
namespace {

// The walk: one lane per pair over the 4-bit records, carrying the reference's `type`
// (0 in M, 1 in a vertical gap, 2 in a horizontal one).
template <bool LOCAL, bool LUT>
__global__ __launch_bounds__(64) void banded_affine_tb_kernel(BandAffineParams P) {
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
    const int R = P.R, L = P.L, S = R <= 8 ? 8 / R : 1, WPS = R <= 8 ? 1 : R / 8;
    int32_t i = res->end_i, j = res->end_j;
    if (i < 0 || i > m || j < 0 || j > n) i = j = 0;   // (never: the fill's end cell is a cell)
    uint32_t nops = 0;
    const uint32_t cap = (uint32_t)(m + n);            // (never reached: every op consumes a symbol)
    int type = 0;
    while ((i > 0 || j > 0) && nops < cap) {
        if (LOCAL) {
            if (i == 0 || j == 0) break;
        } else {
            if (i == 0) { ops[nops++] = 'L'; --j; continue; }
            if (j == 0) { ops[nops++] = 'U'; --i; continue; }
        }
        const int32_t tp = i + j - bg.lo - bg.tb, c = j - i - bg.lo;
        if (c < 0 || c >= bg.beff) break;   // (never: the walk stays inside the band)
        const int32_t l = c / (2 * R), rr = (c % (2 * R)) >> 1;
        uint32_t w;
        if (R <= 8) w = rec[(uint64_t)(tp / S) * L + l] >> (((tp % S) * R + rr) * 4);
        else w = rec[((uint64_t)tp * WPS + (rr >> 3)) * L + l] >> ((rr & 7) * 4);
        if (type == 0) {
            const uint32_t code = w & 3u;
            if (code == 0) break;
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

hipError_t launch_banded_affine_fill(int algo, int variant, int mm, bool rec, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    if (mm == kMatchSub) return launch_banded_affine_fill_sub(algo, variant, rec, p, s);
    if (mm == kMatchLut)
        return algo == SA_LOCAL_GOTOH ? launch_band_affine_fill_alg<true, kMatchLut>(variant, rec, p, s)
                                      : launch_band_affine_fill_alg<false, kMatchLut>(variant, rec, p, s);
    return algo == SA_LOCAL_GOTOH ? launch_band_affine_fill_alg<true, kMatchEq>(variant, rec, p, s)
                                  : launch_band_affine_fill_alg<false, kMatchEq>(variant, rec, p, s);
}

hipError_t launch_banded_affine_tb(int algo, bool lut, const BandAffineParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    const dim3 grid((p.count + 63) / 64), block(64);
    if (algo == SA_LOCAL_GOTOH) {
        if (lut) hipLaunchKernelGGL((banded_affine_tb_kernel<true, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((banded_affine_tb_kernel<true, false>), grid, block, 0, s, p);
    } else {
        if (lut) hipLaunchKernelGGL((banded_affine_tb_kernel<false, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((banded_affine_tb_kernel<false, false>), grid, block, 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace sa
