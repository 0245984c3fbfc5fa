// wave_emu/hip/hip_runtime.h — a host-only stand-in for <hip/hip_runtime.h>, for running the banded
// kernels' own source on a CPU under the host sanitizers (tests/cpp/banded_emu.cpp).
// With this directory first on the include path and `-x c++`, seqalib_amd/csrc/sa_banded*.hip and
// sa_band_planner.hip compile unmodified with g++ -std=c++20.
//
// It supplies exactly what those units and sa_internal.h use, and nothing else: an intrinsic a kernel
// starts to use is a compile error here, so the harness fails loudly and is extended on purpose.
//
// Execution model.  One block at a time.  A block is blockDim.x host threads, one per lane, in waves
// of 64 (kWave).  Lanes run freely between cross-lane operations; every cross-lane operation is a
// two-phase exchange through the wave's slot array: each lane publishes its value and the operation's
// tag, the wave's barrier closes, each lane reads its source lane's slot, the barrier closes again.
// __syncthreads is the block's barrier.  A lane whose kernel function returns leaves both barriers:
// the others no longer wait for it, and its slot is marked as exited.  Lanes of the last wave beyond
// blockDim.x never existed and count as exited.
//
// What an operation returns is written next to it below; where the hardware's answer is undefined the
// shim aborts with a message instead of inventing one.  Lanes that meet at a barrier with different
// operations abort too ("lanes diverged"): the kernels claim every cross-lane operation is reached
// by all the lanes of a wave that are still running.
#pragma once
#include <atomic>
#include <climits>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
// One block runs at a time, so a function-local static is the block's LDS.  (Not zeroed between blocks:
// LDS is not either.)
#define __shared__ static

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1 };
typedef struct wave_emu_stream* hipStream_t;
typedef struct wave_emu_event* hipEvent_t;

struct dim3 {
    uint32_t x, y, z;
    constexpr dim3(uint32_t x_ = 1, uint32_t y_ = 1, uint32_t z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct int4 {
    int x, y, z, w;
};

// The device overloads the kernels call unqualified.
inline int min(int a, int b) { return b < a ? b : a; }
inline int max(int a, int b) { return a < b ? b : a; }

inline thread_local dim3 threadIdx;
inline dim3 blockIdx, blockDim;

namespace wave_emu {

constexpr int kWave = 64;

[[noreturn]] inline void die(const char* what) {
    fprintf(stderr, "wave_emu: %s (block %u, thread %u)\n", what, blockIdx.x, threadIdx.x);
    fflush(stderr);
    abort();
}

// A barrier whose party can shrink: wait() blocks until every remaining lane has arrived, leave()
// takes the caller out for good (and releases the others if they were waiting for it alone).
class Barrier {
public:
    void reset(unsigned parties) {
        expected_ = parties;
        arrived_ = 0;
    }
    void wait() {
        unsigned long g;
        {
            std::lock_guard<std::mutex> lk(m_);
            g = generation_.load(std::memory_order_relaxed);
            if (++arrived_ == expected_) {
                release();
                return;
            }
        }
        // A wave has more lanes than most hosts have cores, and waking 63 sleepers per barrier costs more than
        // the kernels' work between two barriers: yield a bounded number of times first, then sleep, so that a
        // host that accounts for spinning lanes' time is not kept busy by them.
        for (int k = 0; k < kSpins; ++k) {
            if (generation_.load(std::memory_order_acquire) != g) return;
            std::this_thread::yield();
        }
        std::unique_lock<std::mutex> lk(m_);
        ++sleepers_;
        cv_.wait(lk, [&] { return generation_.load(std::memory_order_relaxed) != g; });
        --sleepers_;
    }
    template <class F>
    void leave(F&& mark) {
        std::lock_guard<std::mutex> lk(m_);
        mark();
        --expected_;
        if (expected_ && arrived_ == expected_) release();
    }

private:
#ifndef WAVE_EMU_SPINS
#define WAVE_EMU_SPINS 100
#endif
    static constexpr int kSpins = WAVE_EMU_SPINS;
    void release() {   // (m_ is held)
        arrived_ = 0;
        generation_.fetch_add(1, std::memory_order_release);
        if (sleepers_) cv_.notify_all();
    }
    std::mutex m_;
    std::condition_variable cv_;
    unsigned expected_ = 0, arrived_ = 0, sleepers_ = 0;
    std::atomic<unsigned long> generation_{0};
};

struct Wave {
    Barrier bar;
    uint64_t slot[kWave];
    uint32_t tag[kWave];
    bool exited[kWave];
};
struct Block {
    Barrier bar;
    std::unique_ptr<Wave[]> waves;
};
struct Lane {
    Block* block = nullptr;
    Wave* wave = nullptr;
    int lane = 0;
};
inline thread_local Lane self;

enum : uint32_t { kOpShfl = 1, kOpDpp = 2, kOpFirst = 3, kOpAny = 4 };

// Phase one of an exchange: publish, then wait for the wave.  Phase two is the caller's reads and done().
template <class T>
inline Wave& publish(uint32_t op, T v) {
    static_assert(sizeof(T) <= 8, "a slot holds 64 bits");
    Wave& w = *self.wave;
    uint64_t bits = 0;
    memcpy(&bits, &v, sizeof(T));
    w.slot[self.lane] = bits;
    w.tag[self.lane] = op;
    w.bar.wait();
    return w;
}
template <class T>
inline T read(const Wave& w, int src, uint32_t op) {
    if (w.tag[src] != op) die("lanes diverged: a source lane is in another cross-lane operation");
    T v;
    memcpy(&v, &w.slot[src], sizeof(T));
    return v;
}
inline void done(Wave& w) { w.bar.wait(); }

// Runs fn once per lane of every block of the grid, block after block.
template <class F>
inline void launch(dim3 grid, dim3 block, F fn) {
    if (grid.y != 1 || grid.z != 1 || block.y != 1 || block.z != 1) die("only one-dimensional launches are emulated");
    if (block.x == 0 || block.x > 1024) die("block size outside 1 .. 1024");
    const unsigned nthreads = block.x, nwaves = (nthreads + kWave - 1) / kWave;
    blockDim = block;
    for (uint32_t b = 0; b < grid.x; ++b) {
        blockIdx = dim3(b);
        Block blk;
        blk.bar.reset(nthreads);
        blk.waves.reset(new Wave[nwaves]);
        for (unsigned wv = 0; wv < nwaves; ++wv) {
            const unsigned lanes = nthreads - wv * kWave < (unsigned)kWave ? nthreads - wv * kWave : (unsigned)kWave;
            blk.waves[wv].bar.reset(lanes);
            for (int l = 0; l < kWave; ++l) {
                blk.waves[wv].slot[l] = 0;
                blk.waves[wv].tag[l] = 0;
                blk.waves[wv].exited[l] = (unsigned)l >= lanes;
            }
        }
        std::vector<std::thread> threads;
        threads.reserve(nthreads);
        for (unsigned t = 0; t < nthreads; ++t)
            threads.emplace_back([&blk, &fn, t] {
                threadIdx = dim3(t);
                self.block = &blk;
                self.wave = &blk.waves[t / kWave];
                self.lane = (int)(t % kWave);
                fn();
                // the lane has returned: it leaves the wave's exchanges and the block's barrier
                self.wave->bar.leave([] { self.wave->exited[self.lane] = true; });
                self.block->bar.leave([] {});
            });
        for (std::thread& th : threads) th.join();
    }
}

}  // namespace wave_emu

// ---------------------------------------------------------------------------------- the runtime calls
inline hipError_t hipGetLastError() { return hipSuccess; }
// (the emulated stream is the calling thread: the fill has finished when the call returns)
inline hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
    memset(dst, value, bytes);
    return hipSuccess;
}
// The kernel's parameters are converted as a launch converts them (a BandAffineParams to the BandParams
// a linear kernel takes), once per lane.
template <class K, class... A>
inline void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, size_t /*lds*/, hipStream_t, A... args) {
    wave_emu::launch(grid, block, [&] { kernel(args...); });
}

// ---------------------------------------------------------------------------- the cross-lane operations
// __shfl_xor(v, mask): lane l takes the value lane l ^ mask of the same wave passed (width 64).  The
// hardware's result for a source lane that has exited is undefined and the kernels claim never to ask
// for one: abort.
template <class T>
inline T __shfl_xor(T v, int mask) {
    using namespace wave_emu;
    Wave& w = publish(kOpShfl, v);
    const int src = (self.lane ^ mask) & (kWave - 1);
    if (w.exited[src]) die("__shfl_xor reads a lane that has exited");
    const T r = read<T>(w, src, kOpShfl);
    done(w);
    return r;
}

// __builtin_amdgcn_update_dpp(old, v, ctrl, 0xf, 0xf, false), the two whole-wave shifts by one lane:
//   ctrl 0x138 (wave shift right): lane l takes lane l - 1's v; lane 0 has no source lane;
//   ctrl 0x130 (wave shift left):  lane l takes lane l + 1's v; lane 63 has no source lane.
// A lane with no source lane, or whose source lane has exited (it is disabled in the hardware's
// execution mask, and with bound_ctrl false a disabled source leaves the destination alone), keeps
// `old`.  Any other control, row mask, bank mask or bound_ctrl aborts: not emulated.
inline int __builtin_amdgcn_update_dpp(int old, int v, int ctrl, int row_mask, int bank_mask, bool bound_ctrl) {
    using namespace wave_emu;
    if ((ctrl != 0x138 && ctrl != 0x130) || row_mask != 0xf || bank_mask != 0xf || bound_ctrl)
        die("update_dpp: only controls 0x138 / 0x130 with full masks and bound_ctrl false are emulated");
    Wave& w = publish(kOpDpp | (uint32_t)ctrl << 8, v);
    const int src = ctrl == 0x138 ? self.lane - 1 : self.lane + 1;
    int r = old;
    if (src >= 0 && src < kWave && !w.exited[src]) r = read<int>(w, src, kOpDpp | (uint32_t)ctrl << 8);
    done(w);
    return r;
}

// __builtin_amdgcn_readfirstlane(v): every lane takes lane 0's v.  The kernels read it after folds that
// every lane of the wave took part in, so lane 0 is running; were it not, the hardware would pick the
// lowest lane still enabled, a value the source does not mean to read: abort.
inline int __builtin_amdgcn_readfirstlane(int v) {
    using namespace wave_emu;
    Wave& w = publish(kOpFirst, v);
    if (w.exited[0]) die("readfirstlane reads lane 0, which has exited");
    const int r = read<int>(w, 0, kOpFirst);
    done(w);
    return r;
}

// __any(pred): non-zero when pred is non-zero on some lane of the wave that is still running.
inline int __any(int pred) {
    using namespace wave_emu;
    Wave& w = publish(kOpAny, pred);
    int r = 0;
    for (int l = 0; l < kWave; ++l)
        if (!w.exited[l] && read<int>(w, l, kOpAny) != 0) r = 1;
    done(w);
    return r;
}

// __syncthreads(): every lane of the block that is still running.
inline void __syncthreads() { wave_emu::self.block->bar.wait(); }

// atomicAdd on a 32-bit word in LDS or global memory: returns the value before.
inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
