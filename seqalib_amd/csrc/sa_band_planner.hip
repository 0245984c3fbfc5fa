// sa_band_planner.hip — the planner of the device-resident seeded band calls
// (sa_align_batch_banded_seeded_device, sa_score_batch_banded_seeded_device): what sa_band_group.h does on the
// host for the host-buffer calls, done on the device for one chunk of pairs, because only the device knows the
// lengths.  Four steps on the call's stream, no host read between them:
//   zero      the chunk's head words (key counters, list offsets, cursors, list info);
//   classify  one thread per pair: read the descriptors, refuse what the call refuses (the result gets its one
//             flag, the pair enters no list), else band_plan_pair (sa_band_plan.h), the pair's plan record
//             and its key's counter -- counted in LDS per block, then one atomicAdd per key the block met;
//   scan      exclusive prefix sum over the kBandPlanKeys counters: keys are variant-major, longest sweep
//             bucket first, so a variant's list is one run of the chunk's list array; its {first, length};
//   scatter   every planned pair takes the next entry of its key's run.
// The order inside a bucket is that of the atomics, and nothing depends on it: a pair's records lie at its
// slot in the chunk times the bound's words, and its results and ops at its own descriptors' places.
#include "sa_band_plan.h"

namespace sa {
namespace {

constexpr int kPlanBlock = 256;

__device__ __forceinline__ void refuse(sa_result* r, uint32_t flag) {
    r->score = 0;
    r->end_i = 0;
    r->end_j = 0;
    r->start_i = 0;
    r->start_j = 0;
    r->nops = 0;
    r->flags = flag;
    r->reserved = 0;
}

__global__ __launch_bounds__(kPlanBlock) void band_plan_classify_kernel(BandPlannerParams P) {
    __shared__ uint32_t cnt[kBandPlanKeys];
    for (int k = threadIdx.x; k < kBandPlanKeys; k += kPlanBlock) cnt[k] = 0;
    __syncthreads();
    const uint32_t q = blockIdx.x * kPlanBlock + threadIdx.x;
    if (q < P.count) {
        const uint32_t pair = P.first + q;
        const uint64_t len1 = P.len1[pair], len2 = P.len2[pair];
        const uint64_t st1 = P.start1[pair], st2 = P.start2[pair];
        const int64_t diag = P.diag[pair];
        const uint64_t need = len1 + len2 + 1;
        const uint64_t oo = P.ops_off ? P.ops_off[pair] : 0;
        BandPlanRec pr;
        pr.s1 = P.seq1 + st1;
        pr.s2 = P.seq2 + st2;
        pr.recoff = (uint64_t)q * P.bound_words;
        pr.opsoff = oo;
        pr.m = (int32_t)len1;
        pr.n = (int32_t)len2;
        pr.diag = (int32_t)diag;
        pr.v = -1;
        pr.pair = pair;
        pr.key = kBandPlanNoKey;
        pr.pad[0] = pr.pad[1] = 0;
        uint32_t flag = 0;
        if (len1 > P.max_m || len2 > P.max_n || len1 > P.seq1_bytes || st1 > P.seq1_bytes - len1 || len2 > P.seq2_bytes ||
            st2 > P.seq2_bytes - len2 || (P.ops_off && (need > P.ops_bytes || oo > P.ops_bytes - need))) {
            flag = SA_FLAG_BAD_SHAPE;
        } else if (diag < -(int64_t)len1 || diag > (int64_t)len2) {
            flag = SA_FLAG_BAD_BAND;
        } else {
            const BandPlanPair pp = band_plan_pair(pr.m, pr.n, P.w, pr.diag, P.affine != 0, P.span);
            if (band_seed_legality(pp.g, pr.m, pr.n, P.free_ends) != kBandSeedLegal) {
                flag = SA_FLAG_BAD_BAND;
            } else if (pp.v < 0 || pp.v > P.vmax || (P.ops_off && pp.rec_words > P.bound_words)) {
                flag = SA_FLAG_BAD_SHAPE;   // (never: band_plan_bound_seeded bounds every pair inside max_m x max_n)
            } else {
                pr.v = pp.v;
                pr.key = pp.key;
                atomicAdd(&cnt[pp.key], 1u);
            }
        }
        if (flag) refuse(P.res + pair, flag);
        P.plans[q] = pr;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kBandPlanKeys; k += kPlanBlock)
        if (cnt[k]) atomicAdd(&P.head[kBandPlanHeadCounts + k], cnt[k]);
}

// One block, a thread per key.
__global__ __launch_bounds__(kBandPlanKeys) void band_plan_scan_kernel(uint32_t* head) {
    __shared__ uint32_t s[kBandPlanKeys];
    const int k = threadIdx.x;
    const uint32_t own = head[kBandPlanHeadCounts + k];
    s[k] = own;
    __syncthreads();
    for (int off = 1; off < kBandPlanKeys; off <<= 1) {
        const uint32_t add = k >= off ? s[k - off] : 0u;
        __syncthreads();
        s[k] += add;
        __syncthreads();
    }
    const uint32_t excl = s[k] - own;
    head[kBandPlanHeadOffsets + k] = excl;
    if (k % kBandPlanBuckets == 0) {   // the variant's list: the run of its buckets
        const int v = k / kBandPlanBuckets;
        const uint32_t end = s[k + kBandPlanBuckets - 1];
        head[kBandPlanHeadLists + 2 * v] = excl;
        head[kBandPlanHeadLists + 2 * v + 1] = end - excl;
    }
}

__global__ __launch_bounds__(kPlanBlock) void band_plan_scatter_kernel(BandPlannerParams P) {
    const uint32_t q = blockIdx.x * kPlanBlock + threadIdx.x;
    if (q >= P.count) return;
    const uint32_t key = P.plans[q].key;
    if (key == kBandPlanNoKey) return;
    const uint32_t slot = P.head[kBandPlanHeadOffsets + key] + atomicAdd(&P.head[kBandPlanHeadCursors + key], 1u);
    if (slot < P.count) P.lists[slot] = q;   // (always: the counters count these very pairs)
}

// The caller's 256 x 256 byte table as the fills' bit table (2048 words), as sa_align_batch_device makes it.
__global__ void band_lut_bits_kernel(const uint8_t* lut, uint32_t* bits) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= 2048) return;
    const int a = w >> 3, b0 = (w & 7) * 32;
    uint32_t v = 0;
    for (int k = 0; k < 32; ++k) v |= (lut[a * 256 + b0 + k] != 0 ? 1u : 0u) << k;
    bits[w] = v;
}

}  // namespace

hipError_t launch_band_planner(const BandPlannerParams& p, hipStream_t s) {
    if (!p.count) return hipSuccess;
    hipError_t e = hipMemsetAsync(p.head, 0, 4ull * kBandPlanHeadWords, s);
    if (e != hipSuccess) return e;
    const dim3 grid((p.count + kPlanBlock - 1) / kPlanBlock), block(kPlanBlock);
    hipLaunchKernelGGL(band_plan_classify_kernel, grid, block, 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(band_plan_scan_kernel, dim3(1), dim3(kBandPlanKeys), 0, s, p.head);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(band_plan_scatter_kernel, grid, block, 0, s, p);
    return hipGetLastError();
}

hipError_t launch_band_lut_bits(const uint8_t* d_lut, uint32_t* bits, hipStream_t s) {
    hipLaunchKernelGGL(band_lut_bits_kernel, dim3(8), dim3(256), 0, s, d_lut, bits);
    return hipGetLastError();
}
}  // namespace sa
