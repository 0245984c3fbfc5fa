// sa_band_sweep.h — the sweep every banded fill runs: an anti-diagonal sweep over the in-band cells only, the
// whole band of a pair in the registers of one wave (or of 16 / 32 lanes of it), direction records laid out by
// anti-diagonal.  DESIGN.md §2.11, §2.14, §2.21.  band_sweep_kernel<F> is the one driver; what a cell computes,
// keeps and records is its cell type F: BandFill (sa_banded_fill.h: one value per cell, 2-bit records) or
// BandAffineFill (sa_banded_affine_fill.h: three values, 4-bit records).  A cell type is a template over
// <algorithm, BandMode, R, L, match mode, REC>; each banded unit instantiates its mode's and match modes'
// kernels through launch_band_sweep below, so that no unit changes another's code object.
//
// What the driver asks of a cell type F: Params (the launch's parameter block), kAlgLocal / kMode / kR / kL /
// kMM / kRec (its template arguments), kVariants (how many entries of kBandR / kBandL it is built for), BITS
// per record code and with them S and WPS (BandRecShape), kEmptyLocalScore, the members the driver sets and
// reads (m, n, lo, beff, rlimE, rlimO, l, lut, sub, best, imin, jmin, score, w[WPS], wmax, dropped, A[R],
// Bw[R + 1]), load_scoring(P, fe), reset(r), step<PAR, EDGE>(h), end_cell(), and store_words(rec, tp): the
// step's WPS > 1 words to rec[(tp * WPS + k) * L + l].  That one line per word is each cell's own because the
// compiler's output follows its spelling: the linear R = 32 kernels are the parent's with two statements, the
// affine R = 16 ones with the unrolled loop, and neither with the other's.
//
// Geometry (BandGeom, sa_internal.h).  Cell (i, j) lies on diagonal k = j - i and anti-diagonal
// d = i + j.  The band [lo, hi] is clipped to the matrix, lo' = max(lo, -m), hi' = min(hi, n) (the
// cells cut off do not exist), c = k - lo' in [0, B') indexes its diagonals and t = d - lo' its
// steps: step t holds the cells with c = t (mod 2), i = (t - c) / 2, j = i + lo' + c.  Lane l of the
// pair's L lanes owns the 2R diagonals c = 2lR .. 2lR + 2R - 1; an even step computes its R even
// ones (the cell's E registers, c = 2lR + 2r), an odd step its R odd ones (O, c = 2lR + 2r + 1):
//   even step: left (i, j-1) = O[r-1] (r = 0: lane l-1's O[R-1], a DPP wave shift per value),
//              up (i-1, j) = O[r], diagonal (i-1, j-1) = E[r] before the update;
//   odd step:  left = E[r], up = E[r+1] (r = R-1: lane l+1's E[0], a DPP wave shift per value), diagonal O[r].
// A cell that does not exist (outside the matrix, outside the band, c >= B') holds kBandNeg, so a
// candidate read from it is below every real score (|score| < 2^29 is checked on the host) and is
// neither the maximum nor equal to it.  With h = t / 2 the lane's cells of both steps are in rows
// h - lR - r, so it keeps R Seq1 symbols and R + 1 Seq2 symbols in registers and slides both windows
// by one symbol per h.
//
// Match modes (MM).  kMatchEq: byte equality.  kMatchLut: the 256 x 256 bit table, 8 KiB of LDS.
// kMatchSub (the matrix calls): the sequences hold symbol codes 0..K-1 and the diagonal term is
// S[code(a)][code(b)], read from the dense K x K int16 table that takes the bit table's LDS slot;
// A[r] holds the row base code(a) * K, multiplied once when the symbol is loaded, Bw[] plain codes,
// so the cell's term is one add and one 16-bit LDS read, and match / mism are not read.  A window
// position outside its sequence holds 0 in every mode: entry 0 of the table (the host never passes
// an empty one).
//
// Band modes (BandMode, sa_internal.h; every one but the corridor is the global algorithm's).
//
// Ends-free (kBandFree, the sa_*_batch_banded_ends_free calls): the global cell, with
// BandParams::free_ends (wave-uniform) deciding two things.  Borders: row 0 is free under
// SA_FREE_SEQ2_BEGIN and column 0 under SA_FREE_SEQ1_BEGIN, computed in EDGE steps as every border value
// is.  End cell: every diagonal of the band ends in exactly one cell of the last row (k <= n - m) or the
// last column (k >= n - m), and those cells are the candidates.  A cell past that end (i > m or j > n) is
// read by cells past the end only, so instead of kBandNeg it keeps the value of the cell before it on its
// diagonal -- the `dg` the step holds anyway; such cells are met in EDGE steps only, so the interior step
// is the global one, untouched, and tB stays its.  After the sweep every register slot therefore holds its
// diagonal's last cell, and end_cell() takes the maximum once per pair: a candidate's key is
// (H << 32 | position), position = i for (i, n) with i < m and m + j for (m, j), so the signed 64-bit
// maximum is the last row-major maximum, for negative H and border candidates alike (m = 0 or n = 0: every
// candidate is a border cell), within a lane and across the pair's lanes.
//
// Seeded (kBandSeeded, the sa_*_batch_banded_seeded calls): the ends-free mode with the pair's band placed
// round its seed diagonal (band_geom_seeded; the diagonal is read from behind the launch's idx entries).
// Nothing else differs: t, c, the windows and end_cell() are written in lo' / hi'.  tA: a step
// t > max(hi', -lo') - lo' has t - c >= 2 (i >= 1) and t + c + 2 lo' >= 2 (j >= 1) for every c = t (mod 2)
// in [0, B'), whatever the signs of lo' and hi' -- a band that begins on row 0 (lo' > 0) has
// tA = hi' - lo', one that begins on column 0 (hi' < 0) tA = -2 lo'.  tB: a step
// t <= min(2m, 2n - hi' - lo') has i <= m (t - c <= 2m) and j <= n (t + c + 2 lo' <= 2n) for every such c,
// for a band that ends on the last row (hi' < n - m) or the last column (lo' > n - m) alike.  Steps before
// a pair's tb (another pair of the wave begins earlier) hold cells with i < 0 or j < 0 only, which stay
// kBandNeg.  (m, n) is a candidate only when n - m is in the band, which `j >= jmin` / `i >= imin` say
// already.  The host admits a pair only if a legal begin and a candidate exist, so `best` leaves LLONG_MIN.
//
// Extension (kBandExtend, the sa_*_batch_banded_extend calls): the global cell and borders in the band
// band_geom_seeded(m, n, w, 0), with the local algorithm's running `best` over the interior cells, which
// starts at the key of (0, 0) -- a candidate that holds 0 and precedes every interior cell in row-major
// order -- and the X-drop test.  t = 2h + PAR is a pair's own step number and the same for every pair of
// the wave, so the checkpoints (after every step t = 15 mod SA_XDROP_PERIOD) are wave-uniform: each lane
// keeps `wmax`, the maximum of its interior cells since the last checkpoint, and the pair's L lanes fold it
// and best's score there.  A pair that stops sets rlimE = rlimO = 0: every later cell of it is kBandNeg and
// no candidate, and it stores no record.  The sweep's last iteration h1 is then taken again over the pairs
// still running, so a wave whose pairs have all stopped leaves the loop at once; the exit is wave-uniform
// and nothing waits.  xdrop (the same for every pair) travels in BandParams::free_ends, which no other part
// of this mode reads.
//
// Device-planned seeded (kBandSeededDev, the sa_*_batch_banded_seeded_device calls): the seeded mode with
// the launch described in device memory.  BandParams keeps its layout and is read differently: off1 holds
// the chunk's plan records (BandPlanRec, sa_band_plan.h), off2 the {first entry, length} of this variant's
// list, idx the chunk's lists (entries are plan record numbers), count the pairs of the chunk (what the grid
// covers).  A block past the list's length returns before it touches anything; a pair's slices, lengths,
// diagonal, record offset, ops offset and result index come from its plan record.
//
// The driver's body stands in the __global__ function itself: moved into a __device__ function that kernels
// call, the same statements are scheduled and allocated differently.
#pragma once
#include "sa_band_plan.h"
#include "sa_internal.h"

namespace sa {
namespace {

__device__ __forceinline__ int32_t from_lower_lane(int32_t v) {   // lane l takes lane l - 1's, lane 0 kBandNeg
    return __builtin_amdgcn_update_dpp(kBandNeg, v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ int32_t from_upper_lane(int32_t v) {   // lane l takes lane l + 1's, lane 63 kBandNeg
    return __builtin_amdgcn_update_dpp(kBandNeg, v, 0x130, 0xf, 0xf, false);
}

// Records of BITS per cell: a lane's R codes of a step fill 1 / S of a 32-bit word, or WPS whole words.
template <int BITS, int R>
struct BandRecShape {
    static constexpr int CPW = 32 / BITS;                    // codes per word
    static constexpr int S = R <= CPW ? CPW / R : 1;         // steps per record word
    static constexpr int WPS = R <= CPW ? 1 : R / CPW;       // record words per step
};

template <class F>
__global__ __launch_bounds__(64) void band_sweep_kernel(typename F::Params P) {
    constexpr int R = F::kR, L = F::kL, MM = F::kMM;
    constexpr bool REC = F::kRec, LOCAL = F::kAlgLocal;
    constexpr bool FREE = band_mode_free(F::kMode), EXT = band_mode_ext(F::kMode), PLANNED = band_mode_planned(F::kMode);
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
            bg = band_mode_geom<F::kMode>(f.m, f.n, (int32_t)P.band, pr.diag);
        }
    } else if (live) {
        pair = P.idx[q];
        const uint64_t a1 = P.off1[pair], a2 = P.off2[pair];
        f.m = (int32_t)(P.off1[pair + 1] - a1);
        f.n = (int32_t)(P.off2[pair + 1] - a2);
        s1 += a1;
        s2 += a2;
        bg = band_mode_geom<F::kMode>(f.m, f.n, (int32_t)P.band, band_mode_diag_behind_idx(F::kMode) ? (int32_t)P.idx[P.count + q] : 0);
    }
    f.lo = bg.lo;
    f.beff = bg.beff;
    f.rlimE = (bg.beff - 2 * f.l * R + 1) >> 1;
    f.rlimO = (bg.beff - 2 * f.l * R) >> 1;
    const uint32_t fe = FREE ? P.free_ends : 0u;
    f.load_scoring(P, fe);
    f.lut = lut_s;
    f.sub = reinterpret_cast<const int16_t*>(lut_s);
    f.best = FREE ? LLONG_MIN : (long long)(((unsigned long long)(uint32_t)kBandNeg) << 32);
    if (EXT) f.best = (long long)(uint32_t)(-bg.lo);   // the key of (0, 0): 0 on diagonal c = -lo'
    if (EXT) f.wmax = kBandNeg;
    const int32_t xdrop = EXT ? (int32_t)P.free_ends : SA_XDROP_OFF;
    if (EXT) f.dropped = false;
    f.score = INT_MIN;
    f.imin = (fe & kFreeSeq1End) ? 0 : f.m;
    f.jmin = (fe & kFreeSeq2End) ? 0 : f.n;
    // steps without border cells and without cells outside the matrix: tA < t <= tB (idle lanes: all)
    int32_t tA = INT_MIN, tB = INT_MAX;
    if (live) {
        tA = max(bg.hi, -bg.lo) - bg.lo;
        tB = min(min(2 * f.m + bg.lo, 2 * f.n - bg.hi) - bg.lo, bg.tend - 1);   // (the last step takes the cell (m, n))
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
        f.reset(r);
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
        if (WPS == 1) {
            const int32_t s = tp % S;
            acc |= f.w[0] << (s * F::BITS * R);
            if (s == S - 1 || t == bg.tend) {
                rec[(uint64_t)(tp / S) * L + f.l] = acc;
                acc = 0;
            }
        } else {
            f.store_words(rec, tp);
        }
    };

    // The symbols that enter the windows after iteration h are loaded PF iterations ahead,
    // a block at a time, so that no step waits for a load issued in its own iteration.
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
                        if (REC && WPS == 1 && tp % S != S - 1) rec[(uint64_t)(tp / S) * L + f.l] = acc;   // the open record word
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
    } else if (FREE) {   // (m, n) is a candidate of every pair (seeded: the host admits a pair with a candidate only), so b is a cell's key
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
        if (sc < 0) {   // no interior cell: an empty input
            sc = F::kEmptyLocalScore;
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

// The launch table: the recording or record-free kernel of one (cell, algorithm, mode, match mode) in the
// variant's R and L.  Cell<ALG, MODE, R, L, MM, REC> is BandFill or BandAffineFill.
template <class F>
hipError_t launch_band_sweep_kernel(const typename F::Params& p, hipStream_t s) {
    const uint32_t grid = (p.count + 64 / F::kL - 1) / (64 / F::kL);
    hipLaunchKernelGGL((band_sweep_kernel<F>), dim3(grid), dim3(64), 0, s, p);
    return hipGetLastError();
}

template <template <int, BandMode, int, int, int, bool> class Cell, int ALG, BandMode MODE, int MM, int V>
hipError_t launch_band_sweep_variant(bool rec, const typename Cell<ALG, MODE, 1, 16, MM, false>::Params& p, hipStream_t s) {
    return rec ? launch_band_sweep_kernel<Cell<ALG, MODE, kBandR[V], kBandL[V], MM, true>>(p, s)
               : launch_band_sweep_kernel<Cell<ALG, MODE, kBandR[V], kBandL[V], MM, false>>(p, s);
}

template <template <int, BandMode, int, int, int, bool> class Cell, int ALG, BandMode MODE, int MM>
hipError_t launch_band_sweep(int variant, bool rec, const typename Cell<ALG, MODE, 1, 16, MM, false>::Params& p, hipStream_t s) {
    constexpr int NV = Cell<ALG, MODE, 1, 16, MM, false>::kVariants;   // the linear cell takes all of kBandR / kBandL, the affine one stops short
    static_assert(kBandVariants == 8 && kBandAffineVariants == 7 && (NV == 7 || NV == 8), "one case per variant of kBandR / kBandL below");
    switch (variant) {
        case 0: return launch_band_sweep_variant<Cell, ALG, MODE, MM, 0>(rec, p, s);
        case 1: return launch_band_sweep_variant<Cell, ALG, MODE, MM, 1>(rec, p, s);
        case 2: return launch_band_sweep_variant<Cell, ALG, MODE, MM, 2>(rec, p, s);
        case 3: return launch_band_sweep_variant<Cell, ALG, MODE, MM, 3>(rec, p, s);
        case 4: return launch_band_sweep_variant<Cell, ALG, MODE, MM, 4>(rec, p, s);
        case 5: return launch_band_sweep_variant<Cell, ALG, MODE, MM, 5>(rec, p, s);
        case 6: return launch_band_sweep_variant<Cell, ALG, MODE, MM, 6>(rec, p, s);
        case 7:
            if constexpr (NV == 8) return launch_band_sweep_variant<Cell, ALG, MODE, MM, 7>(rec, p, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace
}  // namespace sa
