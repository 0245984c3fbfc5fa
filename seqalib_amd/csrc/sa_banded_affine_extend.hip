// sa_banded_affine_extend.hip — the GlobalGotoh extension band (sa_align_batch_banded_extend,
// sa_score_batch_banded_extend with SA_GLOBAL_GOTOH), LEFT OUT of the shared sweep of sa_band_sweep.h.
//
// Every other banded unit instantiates band_sweep_kernel<F> and the one walk per cell.  This
// unit does not: a GPU run of tests/test_gpu_banded_extend.py::test_every_variant[3-1023] on the shared source
// ended in `an illegal memory access` -- the open fault of DESIGN.md §2.18, in this unit's R = 16 recording fill,
// whose cause is not found.  Until it is, nothing this unit compiles changes: below stand, verbatim, the affine
// fill header and this unit as they were before the shared sweep (the mode as kMatch*Bit in the fill's
// match-mode value, the sweep driver and the walk written out), and the unit includes neither sa_band_sweep.h
// nor sa_banded_affine_fill.h.  Its device code is byte for byte what it was
// (profiles/banded_sweep_refactor_device_code.txt).  To put it on the shared code once the cause is known:
// replace everything below by the two launchers of sa_banded_affine_seeded.hip with kBandExtend.
//
// ---- the former sa_banded_affine_fill.h ----
// sa_banded_affine_fill.h — the banded LocalGotoh / GlobalGotoh fill (sa_align_batch_banded_affine,
// sa_score_batch_banded_affine, and the affine half of sa_align_batch_banded_matrix): the anti-diagonal
// sweep of sa_banded_fill.h with three values per cell (M, X vertical, Y horizontal) and 4-bit records
// laid out by anti-diagonal.  DESIGN.md §2.13, §2.14.  Instantiated by sa_banded_affine.hip (kMatchEq,
// kMatchLut) and sa_banded_affine_sub.hip (kMatchSub); the match modes are those of sa_banded_fill.h.
//
// Geometry and register mapping are those of sa_banded_fill.h (BandGeom, sa_internal.h): lane l of the
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
// Ends-free mode (FREE, GlobalGotoh only; the sa_*_batch_banded_ends_free calls, instantiated by
// sa_banded_affine_free.hip): as in sa_banded_fill.h.  BandParams::free_ends zeroes M on row 0
// (SA_FREE_SEQ2_BEGIN) and column 0 (SA_FREE_SEQ1_BEGIN), X = Y = kBorderXY there as on every border; a
// cell past the end of its diagonal keeps that diagonal's last M (EDGE steps only), and after the sweep
// end_cell() takes the maximum of M over the last cells of the diagonals the END flags admit, keyed
// (M << 32 | position).  The kernel's parameters are bools and shapes, and one more
// would rename every existing kernel, so the mode travels as kMatchFreeBit in its match-mode value.
//
// Seeded mode (kMatchSeedBit beside kMatchFreeBit; the sa_*_batch_banded_seeded calls, instantiated by
// sa_banded_affine_seeded.hip): the ends-free mode with band_geom_seeded, as in sa_banded_fill.h.
//
// Extension mode (kMatchExtBit alone; the sa_*_batch_banded_extend calls, instantiated by
// sa_banded_affine_extend.hip): GlobalGotoh's cell and borders in the band band_geom_seeded(m, n, w, 0),
// the local mode's running `best` over M of the interior cells, from the key of (0, 0) on, and the X-drop
// test with its wave-uniform early exit, all as sa_banded_fill.h describes them.
//
// Device-planned seeded mode (kMatchPlanBit beside the seeded mode's two; the sa_*_batch_banded_seeded_device
// calls, instantiated by sa_banded_affine_seeded_dev.hip): the launch is described in device memory, as in
// sa_banded_fill.h -- off1 the plan records, off2 this variant's {first entry, length}, idx the lists.
#include "sa_band_plan.h"
#include "sa_internal.h"

namespace sa {
namespace {

constexpr int32_t kBorderXY = -10000;   // X and Y of every border cell (the reference's constant)
constexpr int kMatchFreeBit = 8;        // in the fill kernel's match-mode template value: the ends-free mode
constexpr int kMatchSeedBit = 16;       // with kMatchFreeBit: the seeded band (band_geom_seeded, diagonals behind idx)
constexpr int kMatchExtBit = 32;        // alone: the extension mode (xdrop in BandParams::free_ends)
constexpr int kMatchPlanBit = 64;       // with kMatchFreeBit | kMatchSeedBit: the pairs come from plan records

__device__ __forceinline__ int32_t aff_from_lower_lane(int32_t v) {   // lane l takes lane l - 1's, lane 0 kBandNeg
    return __builtin_amdgcn_update_dpp(kBandNeg, v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ int32_t aff_from_upper_lane(int32_t v) {   // lane l takes lane l + 1's, lane 63 kBandNeg
    return __builtin_amdgcn_update_dpp(kBandNeg, v, 0x130, 0xf, 0xf, false);
}

template <bool LOCAL, int R, int L, int MM, bool REC, bool FREE, bool EXT = false>
struct BandAffineFill {
    static_assert(!(LOCAL && FREE), "the ends-free mode is GlobalGotoh's");
    static_assert(!(EXT && (LOCAL || FREE)), "the extension mode is GlobalGotoh's, with its own end cell");
    static constexpr int S = R <= 8 ? 8 / R : 1;         // steps per record word
    static constexpr int WPS = R <= 8 ? 1 : R / 8;       // record words per step
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

    // One step.  PAR: 0 even (E), 1 odd (O).  EDGE: the step may hold border cells or cells outside
    // the matrix; otherwise every cell with c < B' is an interior cell.
    template <int PAR, bool EDGE>
    __device__ __forceinline__ void step(int32_t h) {
        int32_t shM, shG;   // the neighbour lane's M and its Y (even step) / X (odd step)
        if (PAR == 0) {
            shM = aff_from_lower_lane(OM[R - 1]);
            shG = aff_from_lower_lane(OY[R - 1]);
            if (l == 0) shM = shG = kBandNeg;
        } else {
            shM = aff_from_upper_lane(EM[0]);
            shG = aff_from_upper_lane(EX[0]);
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

template <bool LOCAL, int R, int L, int MMF, bool REC>   // MMF: the match mode [| kMatchFreeBit [| kMatchSeedBit] | kMatchExtBit]
__global__ __launch_bounds__(64) void banded_affine_fill_kernel(BandAffineParams P) {
    constexpr int MM = MMF & ~(kMatchFreeBit | kMatchSeedBit | kMatchExtBit | kMatchPlanBit);
    constexpr bool FREE = (MMF & kMatchFreeBit) != 0, SEEDED = (MMF & kMatchSeedBit) != 0, EXT = (MMF & kMatchExtBit) != 0;
    constexpr bool PLANNED = (MMF & kMatchPlanBit) != 0;
    static_assert(FREE || !SEEDED, "the seeded band is an ends-free one");
    static_assert(SEEDED || !PLANNED, "the planned mode is the seeded band's");
    using F = BandAffineFill<LOCAL, R, L, MM, REC, FREE, EXT>;
    constexpr int PPW = 64 / L, S = F::S, WPS = F::WPS;
    uint32_t lfirst = 0, lcount = 0;
    if (PLANNED) {   // the list's place and length, from device memory
        const uint32_t* const li = reinterpret_cast<const uint32_t*>(P.off2);
        lfirst = li[0];
        lcount = li[1];
        if (blockIdx.x * PPW >= lcount) return;   // (the whole block: the grid covers a full chunk)
    }
    __shared__ uint32_t lut_s[MM != kMatchEq ? 2048 : 1];
    if (MM == kMatchLut) {
        for (int k = threadIdx.x; k < 2048; k += 64) lut_s[k] = P.lutbits[k];
        __syncthreads();
    }
    const uint32_t K = MM == kMatchSub ? P.sub_k : 1u;
    if (MM == kMatchSub) {   // K <= kSubMaxSyms: at most 2048 words (the host pads the table to a whole word)
        const uint32_t* src = reinterpret_cast<const uint32_t*>(P.submat);
        const int words = min((int)((K * K + 1) / 2), 2048);
        for (int k = threadIdx.x; k < words; k += 64) lut_s[k] = src[k];
        __syncthreads();
    }
    const int lane = threadIdx.x, g = lane / L;
    F f;
    f.l = lane % L;
    const uint32_t q = blockIdx.x * PPW + g;
    const bool live = q < (PLANNED ? lcount : P.count);
    uint32_t pair = 0;
    const uint8_t* s1 = P.seq1;
    const uint8_t* s2 = P.seq2;
    f.m = 0;
    f.n = 0;
    BandGeom bg{0, 0, 0, 0x7ffffffe, -1};
    uint64_t plan_recoff = 0;
    if (PLANNED) {
        if (live) {
            const BandPlanRec& pr = reinterpret_cast<const BandPlanRec*>(P.off1)[P.idx[lfirst + q]];
            pair = pr.pair;
            f.m = pr.m;
            f.n = pr.n;
            s1 = pr.s1;
            s2 = pr.s2;
            plan_recoff = pr.recoff;
            bg = band_geom_seeded(f.m, f.n, (int32_t)P.band, pr.diag);
        }
    } else if (live) {
        pair = P.idx[q];
        const uint64_t a1 = P.off1[pair], a2 = P.off2[pair];
        f.m = (int32_t)(P.off1[pair + 1] - a1);
        f.n = (int32_t)(P.off2[pair + 1] - a2);
        s1 += a1;
        s2 += a2;
        bg = SEEDED ? band_geom_seeded(f.m, f.n, (int32_t)P.band, (int32_t)P.idx[P.count + q])
             : EXT  ? band_geom_seeded(f.m, f.n, (int32_t)P.band, 0)
                    : band_geom(f.m, f.n, (int32_t)P.band);
    }
    f.lo = bg.lo;
    f.beff = bg.beff;
    f.rlimE = (bg.beff - 2 * f.l * R + 1) >> 1;
    f.rlimO = (bg.beff - 2 * f.l * R) >> 1;
    f.gopen = P.gap_open;
    f.ge = P.gap_extend;
    f.goe = P.gap_open + P.gap_extend;
    f.match = P.match;
    f.mism = P.mismatch;
    f.lut = lut_s;
    f.sub = reinterpret_cast<const int16_t*>(lut_s);
    f.best = FREE ? LLONG_MIN : (long long)(((unsigned long long)(uint32_t)kBandNeg) << 32);
    if (EXT) f.best = (long long)(uint32_t)(-bg.lo);   // the key of (0, 0): M = 0 on diagonal c = -lo'
    if (EXT) f.wmax = kBandNeg;
    const int32_t xdrop = EXT ? (int32_t)P.free_ends : SA_XDROP_OFF;
    if (EXT) f.dropped = false;
    f.score = INT_MIN;
    const uint32_t fe = FREE ? P.free_ends : 0u;
    f.z_row0 = (fe & kFreeSeq2Begin) != 0;
    f.z_col0 = (fe & kFreeSeq1Begin) != 0;
    f.imin = (fe & kFreeSeq1End) ? 0 : f.m;
    f.jmin = (fe & kFreeSeq2End) ? 0 : f.n;
    // steps without border cells and without cells outside the matrix: tA < t <= tB (idle lanes: all)
    int32_t tA = INT_MIN, tB = INT_MAX;
    if (live) {
        tA = max(bg.hi, -bg.lo) - bg.lo;
        tB = min(min(2 * f.m + bg.lo, 2 * f.n - bg.hi) - bg.lo, bg.tend - 1);   // (the last step takes M[m][n])
    }
    int32_t t0 = bg.tb, t1 = bg.tend;
    for (int off = 32; off >= 1; off >>= 1) {
        t0 = min(t0, __shfl_xor(t0, off));
        t1 = max(t1, __shfl_xor(t1, off));
        tA = max(tA, __shfl_xor(tA, off));
        tB = min(tB, __shfl_xor(tB, off));
    }
    t0 = __builtin_amdgcn_readfirstlane(t0);
    t1 = __builtin_amdgcn_readfirstlane(t1);
    tA = __builtin_amdgcn_readfirstlane(tA);
    tB = __builtin_amdgcn_readfirstlane(tB);

    // (kMatchSub: a Seq1 symbol becomes its row base here, once, not in every cell that reads it)
    auto sym1 = [&](int32_t x) -> uint32_t {
        if (MM == kMatchSub) return (uint32_t)x < (uint32_t)f.m ? s1[x] * K : 0u;
        return (uint32_t)x < (uint32_t)f.m ? s1[x] : 0u;
    };
    auto sym2 = [&](int32_t x) -> uint32_t { return (uint32_t)x < (uint32_t)f.n ? s2[x] : 0u; };
    const int32_t h0 = t0 >> 1;
    int32_t h1 = t1 >> 1;   // (extension: falls when pairs stop)
    const int32_t ab = -f.l * R - 1, bb = f.l * R + f.lo - 1;   // A[r] = Seq1[h + ab - r], Bw[r] = Seq2[h + bb + r]
#pragma unroll
    for (int r = 0; r < R; ++r) {
        f.EM[r] = f.EX[r] = f.EY[r] = kBandNeg;
        f.OM[r] = f.OX[r] = f.OY[r] = kBandNeg;
        f.A[r] = sym1(h0 + ab - r);
    }
#pragma unroll
    for (int r = 0; r <= R; ++r) f.Bw[r] = sym2(h0 + bb + r);

    uint32_t* rec = REC && live ? P.rec + (PLANNED ? plan_recoff : P.recoff[q]) : nullptr;
    uint32_t acc = 0;
    auto store = [&](int32_t t) {
        if (!REC) return;
        const int32_t tp = t - bg.tb;
        if (tp < 0 || t > bg.tend) return;
        if (EXT && f.dropped) return;
        if (R <= 8) {
            const int32_t s = tp % S;
            acc |= f.w[0] << (s * 4 * R);
            if (s == S - 1 || t == bg.tend) {
                rec[(uint64_t)(tp / S) * L + f.l] = acc;
                acc = 0;
            }
        } else {
#pragma unroll
            for (int k = 0; k < WPS; ++k) rec[((uint64_t)tp * WPS + k) * L + f.l] = f.w[k];
        }
    };

    // symbols enter the windows PF iterations after their loads were issued (as sa_banded.hip)
    constexpr int PF = 4;
    uint32_t ca[PF], cb[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        ca[u] = sym1(h0 + u + 1 + ab);
        cb[u] = sym2(h0 + u + 1 + bb + R);
    }
    for (int32_t hb = h0; hb <= h1; hb += PF) {
        uint32_t na[PF], nb[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            na[u] = sym1(hb + PF + u + 1 + ab);
            nb[u] = sym2(hb + PF + u + 1 + bb + R);
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int32_t h = hb + u, t = 2 * h;
            if (h > h1) break;
            if (t > tA && t + 1 <= tB) {
                f.template step<0, false>(h);
                store(t);
                f.template step<1, false>(h);
                store(t + 1);
            } else {
                f.template step<0, true>(h);
                store(t);
                f.template step<1, true>(h);
                store(t + 1);
            }
            if (EXT && (t & (SA_XDROP_PERIOD - 1)) == SA_XDROP_PERIOD - 2) {   // a checkpoint follows step t + 1
                int32_t bs = (int32_t)(f.best >> 32), recent = f.wmax;
                for (int off = L / 2; off >= 1; off >>= 1) {
                    bs = max(bs, __shfl_xor(bs, off));
                    recent = max(recent, __shfl_xor(recent, off));
                }
                f.wmax = kBandNeg;
                // (recent == kBandNeg: the window held no interior cell; bs - recent < 2^30 otherwise)
                const bool stop = !f.dropped && t + 1 < bg.tend && xdrop >= 0 && recent > kBandNeg && bs - recent > xdrop;
                if (__any(stop)) {
                    if (stop) {
                        const int32_t tp = t + 1 - bg.tb;   // (>= 0: the window held a cell of this pair)
                        if (REC && R <= 8 && tp % S != S - 1) rec[(uint64_t)(tp / S) * L + f.l] = acc;   // the open record word
                        f.dropped = true;
                        f.rlimE = f.rlimO = 0;
                    }
                    int32_t te = f.dropped ? -1 : bg.tend;
                    for (int off = 32; off >= 1; off >>= 1) te = max(te, __shfl_xor(te, off));
                    h1 = __builtin_amdgcn_readfirstlane(te) >> 1;
                }
            }
#pragma unroll
            for (int r = R - 1; r > 0; --r) f.A[r] = f.A[r - 1];
            f.A[0] = ca[u];
#pragma unroll
            for (int r = 0; r < R; ++r) f.Bw[r] = f.Bw[r + 1];
            f.Bw[R] = cb[u];
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            ca[u] = na[u];
            cb[u] = nb[u];
        }
    }

    // fold the pair's lanes
    int32_t sc_i = 0, sc_j = 0, sc = f.score;
    if (EXT) {   // best is a candidate's key: (0, 0)'s or an interior cell's
        long long b = f.best;
        for (int off = L / 2; off >= 1; off >>= 1) {
            const long long o = __shfl_xor(b, off);
            b = o > b ? o : b;
        }
        sc = (int32_t)(b >> 32);
        const uint32_t pos = (uint32_t)b;
        // (an idle lane group has beff = 0 and divides by 1: a division by zero is undefined, and the CPU run of
        // this source, tests/test_banded_emu.py, traps on it; only live pairs are written below)
        const uint32_t bdiv = (uint32_t)max(f.beff, 1);
        sc_i = (int32_t)(pos / bdiv);
        sc_j = sc_i + f.lo + (int32_t)(pos % bdiv);
    } else if (FREE) {   // (m, n) is a candidate of every pair, so b is a cell's key
        f.end_cell();
        long long b = f.best;
        for (int off = L / 2; off >= 1; off >>= 1) {
            const long long o = __shfl_xor(b, off);
            b = o > b ? o : b;
        }
        sc = (int32_t)(b >> 32);
        const int32_t pos = (int32_t)(uint32_t)b;
        sc_i = pos < f.m ? pos : f.m;
        sc_j = pos < f.m ? f.n : pos - f.m;
    } else if (!LOCAL) {
        for (int off = L / 2; off >= 1; off >>= 1) sc = max(sc, __shfl_xor(sc, off));
        sc_i = f.m;
        sc_j = f.n;
    } else {
        long long b = f.best;
        for (int off = L / 2; off >= 1; off >>= 1) {
            const long long o = __shfl_xor(b, off);
            b = o > b ? o : b;
        }
        sc = (int32_t)(b >> 32);
        if (sc < 0) {   // no interior cell (an empty input): M[0][0], as the unbanded raw path
            sc = 0;
        } else {
            const uint32_t pos = (uint32_t)b;
            sc_i = (int32_t)(pos / (uint32_t)f.beff);
            sc_j = sc_i + f.lo + (int32_t)(pos % (uint32_t)f.beff);
        }
    }
    if (live && f.l == 0) {
        sa_result* r = P.res + pair;
        r->score = sc;
        r->end_i = sc_i;
        r->end_j = sc_j;
        if (!REC) {
            r->start_i = -1;
            r->start_j = -1;
            r->nops = 0;
            r->flags = 0;
            r->reserved = 0;
        }
        if (EXT) r->flags = f.dropped ? SA_FLAG_DROPPED : 0;   // (the walk keeps it)
    }
}

// The recording / record-free kernel of one (algorithm, R, L, match mode).
template <bool LOCAL, int R, int L, int MM>
hipError_t launch_band_affine_fill_rl(bool rec, const BandAffineParams& p, hipStream_t s) {
    const uint32_t grid = (p.count + 64 / L - 1) / (64 / L);
    if (rec) hipLaunchKernelGGL((banded_affine_fill_kernel<LOCAL, R, L, MM, true>), dim3(grid), dim3(64), 0, s, p);
    else hipLaunchKernelGGL((banded_affine_fill_kernel<LOCAL, R, L, MM, false>), dim3(grid), dim3(64), 0, s, p);
    return hipGetLastError();
}

template <bool LOCAL, int MM>
hipError_t launch_band_affine_fill_alg(int variant, bool rec, const BandAffineParams& p, hipStream_t s) {
    static_assert(kBandAffineVariants == 7, "one case per variant of kBandR / kBandL below");
    switch (variant) {
        case 0: return launch_band_affine_fill_rl<LOCAL, 1, 16, MM>(rec, p, s);
        case 1: return launch_band_affine_fill_rl<LOCAL, 2, 16, MM>(rec, p, s);
        case 2: return launch_band_affine_fill_rl<LOCAL, 4, 16, MM>(rec, p, s);
        case 3: return launch_band_affine_fill_rl<LOCAL, 4, 32, MM>(rec, p, s);
        case 4: return launch_band_affine_fill_rl<LOCAL, 4, 64, MM>(rec, p, s);
        case 5: return launch_band_affine_fill_rl<LOCAL, 8, 64, MM>(rec, p, s);
        case 6: return launch_band_affine_fill_rl<LOCAL, 16, 64, MM>(rec, p, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace
}  // namespace sa

// ---- the former sa_banded_affine_extend.hip ----
// Extension instantiations of the banded GlobalGotoh fill (sa_align_batch_banded_extend,
// sa_score_batch_banded_extend with SA_GLOBAL_GOTOH): GlobalGotoh anchored at (0, 0) in the band round
// diagonal 0, free to end at any interior cell, with the X-drop test and its early exit (kMatchExtBit).
// kMatchEq and kMatchLut, recording and record-free, every affine variant, and their walk.  A translation
// unit of their own, so the code objects of the other banded affine units are unchanged.  DESIGN.md §2.18.

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
