// sa_banded_fill.h — the banded Needleman-Wunsch / Smith-Waterman cell and walk (sa_align_batch_banded,
// sa_score_batch_banded, the linear half of sa_align_batch_banded_matrix, and the NW halves of the ends-free,
// seeded, extension and device-planned calls): one value H per cell, 2-bit direction records (0 stop,
// 1 diagonal, 2 up, 3 left).  DESIGN.md §2.11, §2.14.  The sweep that drives the cell, its geometry, the
// match modes and the band modes are described in sa_band_sweep.h; what is the linear cell's own:
//   borders hold k * gap (SW: 0; ends-free: 0 where BandParams::free_ends frees the begin, g_row0 / g_col0);
//   best's key is (H << 32 | i * beff + c) for SW and the extension mode, (H << 32 | position) ends-free;
//   an empty SW pair scores INT_MIN.
#pragma once
#include "sa_band_sweep.h"

namespace sa {
namespace {

template <int ALG, BandMode MODE, int R, int L, int MM, bool REC>
struct BandFill {
    static_assert(ALG == SA_SW || ALG == SA_NW, "the linear cell's algorithms");
    static_assert(ALG == SA_NW || MODE == kBandCorridor, "every mode but the corridor is NW's");
    using Params = BandParams;
    static constexpr BandMode kMode = MODE;
    static constexpr int kR = R, kL = L, kMM = MM, kVariants = kBandVariants;
    static constexpr bool kRec = REC, kAlgLocal = ALG == SA_SW;
    static constexpr bool FREE = band_mode_free(MODE);
    static constexpr bool EXT = band_mode_ext(MODE);   // NW's cell and borders throughout
    static constexpr int BITS = 2, S = BandRecShape<BITS, R>::S, WPS = BandRecShape<BITS, R>::WPS;
    static constexpr int32_t kEmptyLocalScore = INT_MIN;
    static_assert(WPS <= 2, "step() and store_words() write w[0] and w[1] out");
    int32_t E[R], O[R];
    uint32_t A[R], Bw[R + 1];
    int32_t m, n, lo, beff, rlimE, rlimO, l;
    int32_t G, match, mism;
    const uint32_t* lut;
    const int16_t* sub;  // kMatchSub: the K x K table in LDS
    long long best;      // SW: (h << 32 | i * beff + c) of the last row-major maximum; ends-free: (h << 32 | position)
    int32_t g_row0, g_col0;   // ends-free: the border's gap per symbol in row 0 / column 0 (0 where the begin is free)
    int32_t imin, jmin;       // ends-free: candidates are (i, n) with i >= imin and (m, j) with j >= jmin
    int32_t score;       // NW: H[m][n]
    uint32_t w[WPS];     // the step's 2-bit codes
    int32_t wmax;        // extension: the maximum of the lane's interior cells since the last checkpoint
    bool dropped;        // extension: the X-drop rule has stopped the pair

    __device__ __forceinline__ void load_scoring(const Params& P, uint32_t fe) {   // fe: the ends-free modes' free_ends, else 0
        G = P.gap;
        match = P.match;
        mism = P.mismatch;
        g_row0 = (fe & kFreeSeq2Begin) ? 0 : P.gap;
        g_col0 = (fe & kFreeSeq1Begin) ? 0 : P.gap;
    }
    __device__ __forceinline__ void reset(int r) { E[r] = O[r] = kBandNeg; }
    // The two words of an R = 32 step.  Written out, here and where step() fills them: as a loop over k
    // the same statements compile to other code (sa_band_sweep.h).
    __device__ __forceinline__ void store_words(uint32_t* rec, int32_t tp) const {
        rec[(uint64_t)tp * 2 * L + l] = w[0];
        rec[((uint64_t)tp * 2 + 1) * L + l] = w[WPS - 1];
    }

    // One step.  PAR: 0 even (E), 1 odd (O).  EDGE: the step may hold border cells or cells outside
    // the matrix; otherwise every cell with c < B' is an interior cell.
    template <int PAR, bool EDGE>
    __device__ __forceinline__ void step(int32_t h) {
        int32_t sh;
        if (PAR == 0) {
            sh = from_lower_lane(O[R - 1]);
            if (l == 0) sh = kBandNeg;
        } else {
            sh = from_upper_lane(E[0]);
            if (l == L - 1) sh = kBandNeg;
        }
        const int32_t i0 = h - l * R, j0 = h + l * R + lo + PAR;
        const int32_t rlim = PAR ? rlimO : rlimE;
        uint32_t pos = (uint32_t)i0 * (uint32_t)beff + (uint32_t)(2 * l * R + PAR);
        const uint32_t dpos = 2u - (uint32_t)beff;
        w[0] = 0;
        if (WPS > 1) w[WPS - 1] = 0;   // (WPS <= 2.  Not a loop over k: see store_words)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int32_t left, up, dg;
            uint32_t a = A[r], b;
            if (PAR == 0) {
                left = r ? O[r > 0 ? r - 1 : 0] : sh;
                up = O[r];
                dg = E[r];
                b = Bw[r];
            } else {
                left = E[r];
                up = r < R - 1 ? E[r < R - 1 ? r + 1 : r] : sh;
                dg = O[r];
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
            const int32_t cu = up + G, cl = left + G;
            int32_t hv = max(max(cd, cu), cl);
            if (ALG == SA_SW) hv = max(hv, 0);
            uint32_t code = hv == cd ? 1u : hv == cu ? 2u : 3u;
            if (ALG == SA_SW && hv == 0) code = 0;
            const int32_t i = i0 - r, j = j0 + r;
            const bool inb = r < rlim;
            bool interior = inb;
            int32_t val;
            if (EDGE) {
                interior = inb && (uint32_t)(i - 1) < (uint32_t)m && (uint32_t)(j - 1) < (uint32_t)n;
                const bool border = inb && ((i == 0 && (uint32_t)j <= (uint32_t)n) || (j == 0 && (uint32_t)i <= (uint32_t)m));
                const int32_t bval = FREE           ? (int32_t)((uint32_t)(i == 0 ? j : i) * (uint32_t)(i == 0 ? g_row0 : g_col0))
                                     : ALG == SA_NW || EXT ? (int32_t)((uint32_t)(i == 0 ? j : i) * (uint32_t)G)
                                                    : 0;
                // (ends-free: a cell past the end of its diagonal keeps the diagonal's last value)
                const int32_t out = FREE && inb && (i > m || j > n) ? dg : kBandNeg;
                val = interior ? hv : border ? bval : out;
                if (ALG == SA_NW && !FREE && !EXT && inb && i == m && j == n) score = val;
            } else {
                val = inb ? hv : kBandNeg;
            }
            if (ALG == SA_SW || EXT) {
                const long long key = (long long)(((unsigned long long)(uint32_t)hv << 32) | pos);
                if (interior && key > best) best = key;
                pos += dpos;
            }
            if (EXT) wmax = interior ? max(wmax, hv) : wmax;
            if (PAR == 0) E[r] = val;
            else O[r] = val;
            if (REC) {
                if (r < 16) w[0] |= code << (2 * (r & 15));
                else w[WPS - 1] |= code << (2 * (r & 15));
            }
        }
    }

    // Ends-free, after the sweep: the lane's maximum key over the last cells of its diagonals.
    __device__ __forceinline__ void end_cell() {
#pragma unroll
        for (int x = 0; x < 2 * R; ++x) {
            const int32_t c = 2 * l * R + x, k = lo + c;
            const int32_t i = k <= n - m ? m : n - k, j = i + k;
            const int32_t val = (x & 1) ? O[x / 2] : E[x / 2];
            const bool cand = c < beff && (i == m ? j >= jmin : i >= imin);
            const long long key = (long long)(((unsigned long long)(uint32_t)val << 32) | (uint32_t)(i == m ? m + j : i));
            if (cand && key > best) best = key;
        }
    }
};

// The walk: one lane per pair over the 2-bit records (0 stop, 1 diagonal, 2 up, 3 left).  Ends-free
// modes: it starts at the fill's end cell and stops at a border whose begin is free.  Extension: it
// starts at the fill's end cell too, walks to (0, 0) and keeps the fill's flag.
template <BandMode MODE, int ALG, bool LUT>
__global__ __launch_bounds__(64) void banded_tb_kernel(BandParams P) {
    static_assert(ALG == SA_NW || MODE == kBandCorridor, "every mode but the corridor is NW's");
    constexpr bool FREE = band_mode_free(MODE);
    constexpr bool PLANNED = band_mode_planned(MODE);   // one launch over the chunk's plan records, R and L per pair
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= P.count) return;
    uint32_t pair;
    int32_t m, n;
    const uint8_t* s1;
    const uint8_t* s2;
    BandGeom bg;
    const uint32_t* rec;
    uint8_t* ops;
    int R, L;
    if (PLANNED) {
        const BandPlanRec& pr = reinterpret_cast<const BandPlanRec*>(P.off1)[q];
        if (pr.v < 0) return;   // refused by the planner: its result is written, it has no ops
        pair = pr.pair;
        m = pr.m;
        n = pr.n;
        s1 = pr.s1;
        s2 = pr.s2;
        bg = band_mode_geom<MODE>(m, n, (int32_t)P.band, pr.diag);
        rec = P.rec + pr.recoff;
        ops = P.ops + pr.opsoff;
        R = kBandR[pr.v];
        L = kBandL[pr.v];
    } else {
        pair = P.idx[q];
        const uint64_t a1 = P.off1[pair], a2 = P.off2[pair];
        m = (int32_t)(P.off1[pair + 1] - a1);
        n = (int32_t)(P.off2[pair + 1] - a2);
        s1 = P.seq1 + a1;
        s2 = P.seq2 + a2;
        bg = band_mode_geom<MODE>(m, n, (int32_t)P.band, band_mode_diag_behind_idx(MODE) ? (int32_t)P.idx[P.count + q] : 0);
        rec = P.rec + P.recoff[q];
        ops = P.ops + a1 + a2 + pair;
        R = P.R;
        L = P.L;
    }
    sa_result* res = P.res + pair;
    const int S = R <= 16 ? 16 / R : 1;
    int32_t i = res->end_i, j = res->end_j;
    if (ALG == SA_SW && (m == 0 || n == 0)) i = j = 0;
    if (i < 0 || i > m || j < 0 || j > n) i = j = 0;   // (never: the fill's end cell is a cell)
    uint32_t nops = 0;
    while (i > 0 || j > 0) {
        if (ALG == SA_SW) {
            if (i == 0 || j == 0) break;
        } else {
            if (FREE && ((i == 0 && (P.free_ends & kFreeSeq2Begin)) || (j == 0 && (P.free_ends & kFreeSeq1Begin)))) break;
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
    res->flags = band_mode_ext(MODE) ? res->flags & SA_FLAG_DROPPED : 0;   // (extension: the fill's flag)
    res->reserved = 0;
}

// A mode's walk: the algorithm's and the label table's instance.
template <BandMode MODE>
hipError_t launch_band_tb(int algo, bool lut, const BandParams& p, hipStream_t s) {
    const dim3 grid((p.count + 63) / 64), block(64);
    if constexpr (MODE == kBandCorridor) {
        if (algo == SA_SW) {
            if (lut) hipLaunchKernelGGL((banded_tb_kernel<MODE, SA_SW, true>), grid, block, 0, s, p);
            else hipLaunchKernelGGL((banded_tb_kernel<MODE, SA_SW, false>), grid, block, 0, s, p);
            return hipGetLastError();
        }
    }
    if (lut) hipLaunchKernelGGL((banded_tb_kernel<MODE, SA_NW, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((banded_tb_kernel<MODE, SA_NW, false>), grid, block, 0, s, p);
    return hipGetLastError();
}

}  // namespace
}  // namespace sa
