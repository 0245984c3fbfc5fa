// sa_banded_affine_fill.h — the banded LocalGotoh / GlobalGotoh cell and walk (sa_align_batch_banded_affine,
// sa_score_batch_banded_affine, the affine half of sa_align_batch_banded_matrix, and the GlobalGotoh halves
// of the ends-free, seeded and device-planned calls; the cell and the walk know the extension mode too, but
// sa_banded_affine_extend.hip does not instantiate them yet, for the reason it gives): the sweep of sa_band_sweep.h
// with three values per cell (M, X vertical, Y horizontal) and 4-bit records laid out by anti-diagonal.
// DESIGN.md §2.13, §2.14.  The sweep, the match modes and the band modes are described in sa_band_sweep.h.
//
// Geometry and register mapping are those of sa_band_sweep.h (BandGeom, sa_internal.h): lane l of the
// pair's L lanes owns the 2R diagonals c = 2lR .. 2lR + 2R - 1 in an even set (EM/EX/EY[r], c = 2lR +
// 2r) and an odd set (OM/OX/OY[r], c = 2lR + 2r + 1).  Per step:
//   even step: left (i, j-1) = O[r-1] supplies M and Y (r = 0: lane l-1's O[R-1], two DPP wave shifts),
//              up (i-1, j) = O[r] supplies M and X, diagonal (i-1, j-1) = EM[r] before the update;
//   odd step:  left = E[r], up = E[r+1] (r = R-1: lane l+1's E[0], two DPP wave shifts), diagonal OM[r].
// A cell that does not exist (outside the matrix, outside the band, c >= B') holds kBandNeg in all
// three values.  X of a cell whose upper neighbour does not exist is max(kBandNeg + open, kBandNeg +
// extend): below every real score (the host admits |score| + 10000 < 2^29 only, and |open| < 2^29),
// so it is never the maximum, never equal to a real value, and one more "+ extend" on it (the cell
// below reads it once, beside a real open term) does not wrap.  Y likewise.  That is how "a term that
// would read a cell outside the band is no candidate" is kept without a flag per value.
//
// Record of a cell (4 bits): bits 0-1 the M code (0 stop: local and M = 0, 1 diagonal, 2 M = X,
// 3 M = Y, tested in that order), bit 2 "X = X(i-1, j) + extend" (tested before the open term, as the
// walk does), bit 3 "Y = Y(i, j-1) + extend".  With gap_extend <= 0 these decide the walk (DESIGN.md
// §2.13): it never needs a value.
//
// Ends-free modes: BandParams::free_ends zeroes M on row 0 (SA_FREE_SEQ2_BEGIN) and column 0
// (SA_FREE_SEQ1_BEGIN), X = Y = kBorderXY there as on every border; a cell past the end of its diagonal keeps
// that diagonal's last M, and end_cell() keys (M << 32 | position).  Extension: the running `best` and the
// X-drop test are over M of the interior cells.  An empty local pair scores 0: M[0][0], as the unbanded raw path.
#pragma once
#include "sa_band_sweep.h"

namespace sa {
namespace {

constexpr int32_t kBorderXY = -10000;   // X and Y of every border cell (the reference's constant)

template <int ALG, BandMode MODE, int R, int L, int MM, bool REC>
struct BandAffineFill {
    static_assert(ALG == SA_LOCAL_GOTOH || ALG == SA_GLOBAL_GOTOH, "the affine cell's algorithms");
    static_assert(ALG == SA_GLOBAL_GOTOH || MODE == kBandCorridor, "every mode but the corridor is GlobalGotoh's, the extension with its own end cell");
    using Params = BandAffineParams;
    static constexpr BandMode kMode = MODE;
    static constexpr int kR = R, kL = L, kMM = MM, kVariants = kBandAffineVariants;
    static constexpr bool kRec = REC, kAlgLocal = ALG == SA_LOCAL_GOTOH;
    static constexpr bool LOCAL = kAlgLocal, FREE = band_mode_free(MODE), EXT = band_mode_ext(MODE);
    static constexpr int BITS = 4, S = BandRecShape<BITS, R>::S, WPS = BandRecShape<BITS, R>::WPS;
    static constexpr int32_t kEmptyLocalScore = 0;
    int32_t EM[R], EX[R], EY[R], OM[R], OX[R], OY[R];
    uint32_t A[R], Bw[R + 1];
    int32_t m, n, lo, beff, rlimE, rlimO, l;
    int32_t goe, ge, gopen, match, mism;   // goe = gap_open + gap_extend
    const uint32_t* lut;
    const int16_t* sub;  // kMatchSub: the K x K table in LDS
    long long best;      // local: (M << 32 | i * beff + c) of the last row-major maximum; ends-free: (M << 32 | position)
    bool z_row0, z_col0; // ends-free: row 0 / column 0 hold M = 0 (a free begin)
    int32_t imin, jmin;  // ends-free: candidates are (i, n) with i >= imin and (m, j) with j >= jmin
    int32_t score;       // global: M[m][n]
    uint32_t w[WPS];     // the step's 4-bit records
    int32_t wmax;        // extension: the maximum of M over the lane's interior cells since the last checkpoint
    bool dropped;        // extension: the X-drop rule has stopped the pair

    __device__ __forceinline__ void load_scoring(const Params& P, uint32_t fe) {   // fe: the ends-free modes' free_ends, else 0
        gopen = P.gap_open;
        ge = P.gap_extend;
        goe = P.gap_open + P.gap_extend;
        match = P.match;
        mism = P.mismatch;
        z_row0 = (fe & kFreeSeq2Begin) != 0;
        z_col0 = (fe & kFreeSeq1Begin) != 0;
    }
    __device__ __forceinline__ void reset(int r) {
        EM[r] = EX[r] = EY[r] = kBandNeg;
        OM[r] = OX[r] = OY[r] = kBandNeg;
    }
    __device__ __forceinline__ void store_words(uint32_t* rec, int32_t tp) const {   // the words of an R = 16 step
#pragma unroll
        for (int k = 0; k < WPS; ++k) rec[((uint64_t)tp * WPS + k) * L + l] = w[k];
    }

    // One step.  PAR: 0 even (E), 1 odd (O).  EDGE: the step may hold border cells or cells outside
    // the matrix; otherwise every cell with c < B' is an interior cell.
    template <int PAR, bool EDGE>
    __device__ __forceinline__ void step(int32_t h) {
        int32_t shM, shG;   // the neighbour lane's M and its Y (even step) / X (odd step)
        if (PAR == 0) {
            shM = from_lower_lane(OM[R - 1]);
            shG = from_lower_lane(OY[R - 1]);
            if (l == 0) shM = shG = kBandNeg;
        } else {
            shM = from_upper_lane(EM[0]);
            shG = from_upper_lane(EX[0]);
            if (l == L - 1) shM = shG = kBandNeg;
        }
        const int32_t i0 = h - l * R, j0 = h + l * R + lo + PAR;
        const int32_t rlim = PAR ? rlimO : rlimE;
        uint32_t pos = (uint32_t)i0 * (uint32_t)beff + (uint32_t)(2 * l * R + PAR);
        const uint32_t dpos = 2u - (uint32_t)beff;
#pragma unroll
        for (int k = 0; k < WPS; ++k) w[k] = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int32_t leftM, leftY, upM, upX, dg;
            uint32_t a = A[r], b;
            if (PAR == 0) {
                leftM = r ? OM[r > 0 ? r - 1 : 0] : shM;
                leftY = r ? OY[r > 0 ? r - 1 : 0] : shG;
                upM = OM[r];
                upX = OX[r];
                dg = EM[r];
                b = Bw[r];
            } else {
                leftM = EM[r];
                leftY = EY[r];
                upM = r < R - 1 ? EM[r < R - 1 ? r + 1 : r] : shM;
                upX = r < R - 1 ? EX[r < R - 1 ? r + 1 : r] : shG;
                dg = OM[r];
                b = Bw[r + 1];
            }
            int32_t cd;
            if (MM == kMatchSub) {
                cd = dg + sub[a + b];
            } else {
                bool mt;
                if (MM == kMatchLut) mt = (lut[(a << 3) | (b >> 5)] >> (b & 31)) & 1u;
                else mt = a == b;
                cd = dg + (mt ? match : mism);
            }
            const int32_t xe = upX + ge, ye = leftY + ge;
            const int32_t x = max(upM + goe, xe), y = max(leftM + goe, ye);
            int32_t hv = max(max(cd, x), y);
            if (LOCAL) hv = max(hv, 0);
            uint32_t code = hv == cd ? 1u : hv == x ? 2u : 3u;
            if (LOCAL && hv == 0) code = 0;
            code |= (x == xe ? 4u : 0u) | (y == ye ? 8u : 0u);
            const int32_t i = i0 - r, j = j0 + r;
            const bool inb = r < rlim;
            bool interior = inb;
            int32_t vM, vX, vY;
            if (EDGE) {
                interior = inb && (uint32_t)(i - 1) < (uint32_t)m && (uint32_t)(j - 1) < (uint32_t)n;
                const bool border = inb && ((i == 0 && (uint32_t)j <= (uint32_t)n) || (j == 0 && (uint32_t)i <= (uint32_t)m));
                const int32_t kk = i == 0 ? j : i;
                const bool zero = LOCAL || kk == 0 || (FREE && (i == 0 ? z_row0 : z_col0));
                const int32_t bval = zero ? 0 : (int32_t)((uint32_t)gopen + (uint32_t)kk * (uint32_t)ge);
                // (ends-free: a cell past the end of its diagonal keeps the diagonal's last M)
                const int32_t out = FREE && inb && (i > m || j > n) ? dg : kBandNeg;
                vM = interior ? hv : border ? bval : out;
                vX = interior ? x : border ? kBorderXY : kBandNeg;
                vY = interior ? y : border ? kBorderXY : kBandNeg;
                if (!LOCAL && !FREE && !EXT && inb && i == m && j == n) score = vM;
            } else {
                vM = inb ? hv : kBandNeg;
                vX = inb ? x : kBandNeg;
                vY = inb ? y : kBandNeg;
            }
            if (LOCAL || EXT) {
                const long long key = (long long)(((unsigned long long)(uint32_t)hv << 32) | pos);
                if (interior && key > best) best = key;
                pos += dpos;
            }
            if (EXT) wmax = interior ? max(wmax, hv) : wmax;
            if (PAR == 0) {
                EM[r] = vM;
                EX[r] = vX;
                EY[r] = vY;
            } else {
                OM[r] = vM;
                OX[r] = vX;
                OY[r] = vY;
            }
            if (REC) w[r / 8] |= code << (4 * (r & 7));
        }
    }

    // Ends-free, after the sweep: the lane's maximum key over the last cells of its diagonals.
    __device__ __forceinline__ void end_cell() {
#pragma unroll
        for (int x = 0; x < 2 * R; ++x) {
            const int32_t c = 2 * l * R + x, k = lo + c;
            const int32_t i = k <= n - m ? m : n - k, j = i + k;
            const int32_t val = (x & 1) ? OM[x / 2] : EM[x / 2];
            const bool cand = c < beff && (i == m ? j >= jmin : i >= imin);
            const long long key = (long long)(((unsigned long long)(uint32_t)val << 32) | (uint32_t)(i == m ? m + j : i));
            if (cand && key > best) best = key;
        }
    }
};

// The walk: one lane per pair over the 4-bit records, carrying the reference's `type`
// (0 in M, 1 in a vertical gap, 2 in a horizontal one), from the fill's end cell, in type 0.  Ends-free
// modes: it stops at a border whose begin is free.  Extension: it walks to (0, 0) and keeps the fill's flag.
// Device-planned: one launch over the chunk's plan records, R and L the pair's own.
template <BandMode MODE, bool LOCAL, bool LUT>
__global__ __launch_bounds__(64) void banded_affine_tb_kernel(BandAffineParams P) {
    static_assert(!LOCAL || MODE == kBandCorridor, "every mode but the corridor is GlobalGotoh's");
    constexpr bool FREE = band_mode_free(MODE), PLANNED = band_mode_planned(MODE);
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= P.count) return;
    // (planned: a pair the planner refused has its result written and no ops.  The return stands before the
    // pair's description is read, not inside it: there it changes the code of everything that follows)
    if (PLANNED && reinterpret_cast<const BandPlanRec*>(P.off1)[q].v < 0) return;
    int32_t m, n;
    const uint8_t* s1;
    const uint8_t* s2;
    BandGeom bg;
    const uint32_t* rec;
    sa_result* res;
    uint8_t* ops;
    int R, L;
    if (PLANNED) {
        const BandPlanRec& pr = reinterpret_cast<const BandPlanRec*>(P.off1)[q];
        m = pr.m;
        n = pr.n;
        s1 = pr.s1;
        s2 = pr.s2;
        bg = band_mode_geom<MODE>(m, n, (int32_t)P.band, pr.diag);
        rec = P.rec + pr.recoff;
        res = P.res + pr.pair;
        ops = P.ops + pr.opsoff;
        R = kBandR[pr.v];
        L = kBandL[pr.v];
    } else {
        const uint32_t pair = P.idx[q];
        const uint64_t a1 = P.off1[pair], a2 = P.off2[pair];
        m = (int32_t)(P.off1[pair + 1] - a1);
        n = (int32_t)(P.off2[pair + 1] - a2);
        s1 = P.seq1 + a1;
        s2 = P.seq2 + a2;
        bg = band_mode_geom<MODE>(m, n, (int32_t)P.band, band_mode_diag_behind_idx(MODE) ? (int32_t)P.idx[P.count + q] : 0);
        rec = P.rec + P.recoff[q];
        res = P.res + pair;
        ops = P.ops + a1 + a2 + pair;
        R = P.R;
        L = P.L;
    }
    const int S = R <= 8 ? 8 / R : 1, WPS = R <= 8 ? 1 : R / 8;
    const bool stop_i0 = FREE && (P.free_ends & kFreeSeq2Begin) != 0, stop_j0 = FREE && (P.free_ends & kFreeSeq1Begin) != 0;
    int32_t i = res->end_i, j = res->end_j;
    if (i < 0 || i > m || j < 0 || j > n) i = j = 0;   // (never: the fill's end cell is a cell)
    uint32_t nops = 0;
    const uint32_t cap = (uint32_t)(m + n);            // (never reached: every op consumes a symbol)
    int type = 0;
    while ((i > 0 || j > 0) && nops < cap) {
        if (LOCAL) {
            if (i == 0 || j == 0) break;
        } else {
            if ((i == 0 && stop_i0) || (j == 0 && stop_j0)) break;
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
    res->flags = band_mode_ext(MODE) ? res->flags & SA_FLAG_DROPPED : 0;   // (extension: the fill's flag)
    res->reserved = 0;
}


// A mode's walk: the algorithm's and the label table's instance.
template <BandMode MODE>
hipError_t launch_band_affine_tb(int algo, bool lut, const BandAffineParams& p, hipStream_t s) {
    const dim3 grid((p.count + 63) / 64), block(64);
    if constexpr (MODE == kBandCorridor) {
        if (algo == SA_LOCAL_GOTOH) {
            if (lut) hipLaunchKernelGGL((banded_affine_tb_kernel<MODE, true, true>), grid, block, 0, s, p);
            else hipLaunchKernelGGL((banded_affine_tb_kernel<MODE, true, false>), grid, block, 0, s, p);
            return hipGetLastError();
        }
    }
    if (lut) hipLaunchKernelGGL((banded_affine_tb_kernel<MODE, false, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((banded_affine_tb_kernel<MODE, false, false>), grid, block, 0, s, p);
    return hipGetLastError();
}

}  // namespace
}  // namespace sa
