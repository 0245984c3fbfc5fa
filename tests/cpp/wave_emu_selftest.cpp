// The wave shim (tests/cpp/wave_emu/hip/hip_runtime.h) against the definitions written in it: every
// cross-lane operation at lanes 0 and 63, in L = 16 / 32 / 64 lane groups, with lanes that have exited,
// and a two-wave block with atomicAdd and __syncthreads.  A stand-alone host program; prints "ok".
// With an argument it runs one of the operations the shim must refuse and is expected to abort:
//   shfl-exited   __shfl_xor from a lane that has exited
//   first-exited  readfirstlane after lane 0 has exited
//   dpp-control   update_dpp with a control other than 0x138 / 0x130
#include <hip/hip_runtime.h>

#include <string>

namespace {

int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s (thread %u)\n", __FILE__, __LINE__, #c, threadIdx.x); \
            __atomic_fetch_add(&failures, 1, __ATOMIC_RELAXED);           \
        }                                                                 \
    } while (0)

constexpr int kOld = -777;

__global__ void shifts_kernel(int* down, int* up) {
    const int l = threadIdx.x;
    down[l] = __builtin_amdgcn_update_dpp(kOld, 100 + l, 0x138, 0xf, 0xf, false);
    up[l] = __builtin_amdgcn_update_dpp(kOld, 100 + l, 0x130, 0xf, 0xf, false);
}

// Lanes 5 and 40..47 return first; their neighbours keep `old`.
__global__ void shifts_exited_kernel(int* down, int* up) {
    const int l = threadIdx.x;
    down[l] = up[l] = -1;
    if (l == 5 || (l >= 40 && l < 48)) return;
    down[l] = __builtin_amdgcn_update_dpp(kOld, 100 + l, 0x138, 0xf, 0xf, false);
    up[l] = __builtin_amdgcn_update_dpp(kOld, 100 + l, 0x130, 0xf, 0xf, false);
}

template <int L>
__global__ void fold_kernel(int* mx, long long* key, int* first, int* any_one, int* any_none) {
    const int l = threadIdx.x, g = l / L;
    int v = (l * 37) % 101 + 1000 * g;          // the group's maximum is found by the fold below
    long long k = ((long long)v << 32) | (unsigned)l;
    for (int off = L / 2; off >= 1; off >>= 1) {
        v = max(v, __shfl_xor(v, off));
        const long long o = __shfl_xor(k, off);
        k = o > k ? o : k;
    }
    mx[l] = v;
    key[l] = k;
    first[l] = __builtin_amdgcn_readfirstlane(l + 7);
    any_one[l] = __any(l == 63);
    any_none[l] = __any(l == 64);
}

// The upper half of the wave returns; folds within the lower 32 lanes, __any and readfirstlane go on.
__global__ void half_wave_kernel(int* mx, int* any_hi, int* any_lo, int* first) {
    const int l = threadIdx.x;
    mx[l] = any_hi[l] = any_lo[l] = first[l] = -1;
    if (l >= 32) return;
    int v = l;
    for (int off = 16; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off));
    mx[l] = v;
    any_hi[l] = __any(1);
    any_lo[l] = __any(l == 40);   // (no running lane has it)
    first[l] = __builtin_amdgcn_readfirstlane(l + 3);
}

// Two waves: LDS counters, a barrier, one atomicAdd per block on global memory, and a lane-dependent
// early return before the second barrier.
__global__ __launch_bounds__(128) void two_wave_kernel(uint32_t* global_sum, uint32_t* seen, uint32_t* wave_first) {
    __shared__ uint32_t cnt[4];
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    __syncthreads();
    atomicAdd(&cnt[threadIdx.x % 4], threadIdx.x);
    __syncthreads();
    if (threadIdx.x >= 4 && threadIdx.x != 64) return;   // the rest wait for nobody who has left
    __syncthreads();
    if (threadIdx.x < 4) {
        seen[blockIdx.x * 4 + threadIdx.x] = cnt[threadIdx.x];
        atomicAdd(global_sum, cnt[threadIdx.x]);
    }
    // each wave exchanges among its own lanes: wave 0 has lanes 0..3 left, wave 1 its lane 0
    wave_first[blockIdx.x * 128 + threadIdx.x] = (uint32_t)__builtin_amdgcn_readfirstlane((int)threadIdx.x);
}

// A block that is no whole number of waves: lanes 32..63 of wave 1 never existed.
__global__ void partial_kernel(int* down, int* up, int* dims) {
    const int t = threadIdx.x;
    down[t] = __builtin_amdgcn_update_dpp(kOld, t, 0x138, 0xf, 0xf, false);
    up[t] = __builtin_amdgcn_update_dpp(kOld, t, 0x130, 0xf, 0xf, false);
    dims[t] = (int)blockDim.x;
}

__global__ void shfl_exited_kernel(int* out) {
    if (threadIdx.x == 17) return;
    out[threadIdx.x] = __shfl_xor((int)threadIdx.x, 1);
}
__global__ void first_exited_kernel(int* out) {
    if (threadIdx.x == 0) return;
    out[threadIdx.x] = __builtin_amdgcn_readfirstlane((int)threadIdx.x);
}
__global__ void dpp_control_kernel(int* out) {
    out[threadIdx.x] = __builtin_amdgcn_update_dpp(0, (int)threadIdx.x, 0x111, 0xf, 0xf, false);
}

template <int L>
void check_folds() {
    int mx[64], first[64], a1[64], a0[64];
    long long key[64];
    hipLaunchKernelGGL((fold_kernel<L>), dim3(1), dim3(64), 0, nullptr, mx, key, first, a1, a0);
    for (int l = 0; l < 64; ++l) {
        const int g = l / L;
        int want = INT_MIN, at = -1;
        for (int x = g * L; x < (g + 1) * L; ++x) {
            const int v = (x * 37) % 101 + 1000 * g;
            if (v > want || (v == want && x > at)) want = v, at = x;
        }
        CHECK(mx[l] == want);
        CHECK(key[l] == (((long long)want << 32) | (unsigned)at));
        CHECK(first[l] == 7);
        CHECK(a1[l] == 1);
        CHECK(a0[l] == 0);
    }
}

}  // namespace

int main(int argc, char** argv) {
    int out[128];
    if (argc > 1) {
        const std::string what = argv[1];
        if (what == "shfl-exited") hipLaunchKernelGGL(shfl_exited_kernel, dim3(1), dim3(64), 0, nullptr, out);
        else if (what == "first-exited") hipLaunchKernelGGL(first_exited_kernel, dim3(1), dim3(64), 0, nullptr, out);
        else if (what == "dpp-control") hipLaunchKernelGGL(dpp_control_kernel, dim3(1), dim3(64), 0, nullptr, out);
        puts("not refused");
        return 0;
    }
    int down[128], up[128], dims[128];
    hipLaunchKernelGGL(shifts_kernel, dim3(1), dim3(64), 0, nullptr, down, up);
    for (int l = 0; l < 64; ++l) {
        CHECK(down[l] == (l == 0 ? kOld : 100 + l - 1));
        CHECK(up[l] == (l == 63 ? kOld : 100 + l + 1));
    }
    hipLaunchKernelGGL(shifts_exited_kernel, dim3(1), dim3(64), 0, nullptr, down, up);
    for (int l = 0; l < 64; ++l) {
        const bool gone = l == 5 || (l >= 40 && l < 48);
        const bool lower_gone = l == 0 || l - 1 == 5 || (l - 1 >= 40 && l - 1 < 48);
        const bool upper_gone = l == 63 || l + 1 == 5 || (l + 1 >= 40 && l + 1 < 48);
        CHECK(down[l] == (gone ? -1 : lower_gone ? kOld : 100 + l - 1));
        CHECK(up[l] == (gone ? -1 : upper_gone ? kOld : 100 + l + 1));
    }
    check_folds<16>();
    check_folds<32>();
    check_folds<64>();

    int mx[64], any_hi[64], any_lo[64], first[64];
    hipLaunchKernelGGL(half_wave_kernel, dim3(1), dim3(64), 0, nullptr, mx, any_hi, any_lo, first);
    for (int l = 0; l < 64; ++l) {
        CHECK(mx[l] == (l < 32 ? 31 : -1));
        CHECK(any_hi[l] == (l < 32 ? 1 : -1));
        CHECK(any_lo[l] == (l < 32 ? 0 : -1));
        CHECK(first[l] == (l < 32 ? 3 : -1));
    }

    uint32_t sum = 0, seen[3 * 4], wave_first[3 * 128];
    memset(wave_first, 0xff, sizeof(wave_first));
    hipLaunchKernelGGL(two_wave_kernel, dim3(3), dim3(128), 0, nullptr, &sum, seen, wave_first);
    uint32_t per_block = 0;
    for (int k = 0; k < 4; ++k) {
        uint32_t want = 0;
        for (uint32_t t = k; t < 128; t += 4) want += t;
        per_block += want;
        for (int b = 0; b < 3; ++b) CHECK(seen[b * 4 + k] == want);
    }
    CHECK(sum == 3 * per_block);
    for (int b = 0; b < 3; ++b)
        for (int t = 0; t < 128; ++t)
            CHECK(wave_first[b * 128 + t] == (t < 4 ? 0u : t == 64 ? 64u : 0xffffffffu));

    hipLaunchKernelGGL(partial_kernel, dim3(1), dim3(96), 0, nullptr, down, up, dims);
    for (int t = 0; t < 96; ++t) {
        CHECK(down[t] == (t % 64 == 0 ? kOld : t - 1));
        CHECK(up[t] == (t % 64 == 63 || t == 95 ? kOld : t + 1));
        CHECK(dims[t] == 96);
    }

    int32_t words[8];
    memset(words, 0x5a, sizeof(words));
    CHECK(hipMemsetAsync(words + 2, 0, 16, nullptr) == hipSuccess && hipGetLastError() == hipSuccess);
    for (int k = 0; k < 8; ++k) CHECK(words[k] == (k >= 2 && k < 6 ? 0 : 0x5a5a5a5a));

    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    puts("ok");
    return 0;
}
