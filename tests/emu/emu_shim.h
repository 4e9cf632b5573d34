// TEST INFRASTRUCTURE ONLY — a minimal SIMT emulator so the *same kernel source*
// (mlx-audio-primitives_amd/csrc/kernels_*.h) can be executed on the CPU: one
// fiber (ucontext) per GPU thread of a workgroup, all on the calling OS thread and
// resumed round-robin; __syncthreads() hands over to the next fiber until the whole
// workgroup has arrived; workgroups run one after another.  (One OS thread per GPU
// thread with std::barrier computes the same, but each barrier then costs a futex
// wake-up per thread, which on a virtual machine takes the suite from minutes to
// hours.)  Used by tests/test_emu_kernels.py (and for ASan/UBSan runs, which the GPU
// pool does not allow).  Never loaded by the product package.
//
// LDS.  Dynamic LDS (`extern __shared__ char ap_smem[]`) is the 160 KB array below, guarded by
// emu_lds_limit().  `__shared__` itself is defined away, so a STATIC `__shared__ float a[N]` inside a
// kernel would become a private array of every emulated thread.  A translation unit that emulates such
// kernels (kernels_features.h is the one header that has them; tests/emu/emu_features.cpp) includes the
// headers that only use dynamic LDS first, then switches
//     #undef __shared__
//     #define __shared__ static
// around the header with the static arrays: one instance per kernel, shared by all threads, which models
// a workgroup's LDS because emu_launch runs the workgroups of a launch one after another.  The headers
// included before the switch are `#pragma once` and are not read again, so their extern declaration of
// ap_smem keeps its meaning.  Static arrays have no guard band: a twin that can size a tile checks it
// against the array bound before it launches.
#pragma once
#include <sys/mman.h>
#include <ucontext.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <memory>
#include <vector>

struct emu_dim3 {
    unsigned x = 1, y = 1, z = 1;
};

inline thread_local emu_dim3 threadIdx, blockIdx;
inline emu_dim3 blockDim, gridDim;

// ---- fibers: the GPU threads of the running workgroup -----
struct emu_barrier {                  // `need` fibers arrive, then all of them go on
    unsigned need = 0, arrived = 0, generation = 0;
};
constexpr size_t EMU_STACK_BYTES = size_t(1) << 20;       // per fiber; pages are committed when touched
inline ucontext_t emu_scheduler_ctx;
inline std::vector<ucontext_t> emu_fiber_ctx;
inline std::vector<unsigned char> emu_fiber_done;
inline unsigned emu_fiber_cur = 0;
inline std::function<void(unsigned)> emu_fiber_body;
inline char *emu_stacks = nullptr;
inline size_t emu_stacks_fibers = 0;
inline emu_barrier emu_block_barrier, emu_wave_barriers[16];

inline void emu_yield() {             // threadIdx / blockIdx are the running fiber's: carry them across
    const emu_dim3 t = threadIdx, b = blockIdx;
    swapcontext(&emu_fiber_ctx[emu_fiber_cur], &emu_scheduler_ctx);
    threadIdx = t;
    blockIdx = b;
}
inline void emu_arrive_and_wait(emu_barrier &bar) {
    const unsigned g = bar.generation;
    if (++bar.arrived == bar.need) {
        bar.arrived = 0;
        ++bar.generation;
        return;
    }
    while (bar.generation == g) emu_yield();
}
inline void emu_fiber_entry() {
    emu_fiber_body(emu_fiber_cur);
    emu_fiber_done[emu_fiber_cur] = 1;                    // uc_link returns to the scheduler
}

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__
#define __launch_bounds__(...)
#define AP_DEV inline
#define AP_HOST_EMU 1

// ---- wave-level helpers used by kernels_wave.h: wave w = threads [64w, 64w+64) -----
inline float emu_xchg[1024];
inline void __syncthreads() { emu_arrive_and_wait(emu_block_barrier); }
inline void emu_wave_sync() { emu_arrive_and_wait(emu_wave_barriers[threadIdx.x >> 6]); }
inline float emu_lane_xor(float x, int mask) {
    emu_xchg[threadIdx.x] = x;
    emu_wave_sync();
    const float y = emu_xchg[threadIdx.x ^ mask];
    emu_wave_sync();
    return y;
}
inline float emu_lane_perm(float x, int src_lane) {      // value of lane `src_lane` of the same wave
    emu_xchg[threadIdx.x] = x;
    emu_wave_sync();
    const float y = emu_xchg[(threadIdx.x & ~63u) | (unsigned)(src_lane & 63)];
    emu_wave_sync();
    return y;
}
inline float ap_quad_xor1(float x) { return emu_lane_xor(x, 1); }
inline float ap_quad_xor2(float x) { return emu_lane_xor(x, 2); }

alignas(16) inline char ap_smem_storage[160 * 1024];
// kernels declare:  extern __shared__ __attribute__((aligned(16))) char ap_smem[];
// -> after the macros above that is an extern char array; define it here.
extern char ap_smem[];

// Dynamic-LDS guard: a launcher that knows the kernel's lds_bytes calls emu_lds_limit(bytes) first; everything
// past that offset is poisoned for the launch and checked afterwards (a kernel writing beyond the LDS the host
// asked for corrupts a neighbour or faults on the GPU; here it would go unnoticed inside the 160 KB array).
inline int emu_lds_limit_bytes = 0;
inline int emu_lds_overruns = 0;
inline void emu_lds_limit(int bytes) { emu_lds_limit_bytes = bytes; }

template <class F>
void emu_launch(unsigned grid, unsigned block, F &&body) {
    const int guard_from = emu_lds_limit_bytes;
    emu_lds_limit_bytes = 0;
    if (guard_from > 0)
        for (int i = guard_from; i < 160 * 1024; ++i) ap_smem[i] = (char)0xA5;
    gridDim.x = grid;
    blockDim.x = block;
    if (block > emu_stacks_fibers) {
        if (emu_stacks) munmap(emu_stacks, emu_stacks_fibers * EMU_STACK_BYTES);
        void *m = mmap(nullptr, block * EMU_STACK_BYTES, PROT_READ | PROT_WRITE,
                       MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (m == MAP_FAILED) abort();
        emu_stacks = (char *)m;
        emu_stacks_fibers = block;
        for (unsigned t = 0; t < block; ++t)          // lowest page of every stack: an overflow faults, not corrupts
            mprotect(emu_stacks + t * EMU_STACK_BYTES, 4096, PROT_NONE);
    }
    emu_block_barrier = emu_barrier{block, 0, 0};
    for (unsigned w = 0; w * 64 < block; ++w)
        emu_wave_barriers[w] = emu_barrier{block - w * 64 < 64 ? block - w * 64 : 64, 0, 0};
    emu_fiber_body = [&](unsigned t) {
        threadIdx.x = t;
        for (unsigned b = 0; b < grid; ++b) {
            blockIdx.x = b;
            body();
            emu_arrive_and_wait(emu_block_barrier);   // workgroups of one launch share ap_smem
        }
    };
    emu_fiber_ctx.assign(block, ucontext_t{});
    emu_fiber_done.assign(block, 0);
    for (unsigned t = 0; t < block; ++t) {
        getcontext(&emu_fiber_ctx[t]);
        emu_fiber_ctx[t].uc_stack.ss_sp = emu_stacks + t * EMU_STACK_BYTES;
        emu_fiber_ctx[t].uc_stack.ss_size = EMU_STACK_BYTES;
        emu_fiber_ctx[t].uc_link = &emu_scheduler_ctx;
        makecontext(&emu_fiber_ctx[t], emu_fiber_entry, 0);
    }
    const emu_dim3 t0 = threadIdx, b0 = blockIdx;
    for (unsigned left = block; left > 0;)
        for (unsigned t = 0; t < block; ++t)
            if (!emu_fiber_done[t]) {
                emu_fiber_cur = t;
                swapcontext(&emu_scheduler_ctx, &emu_fiber_ctx[t]);
                left -= emu_fiber_done[t];
            }
    threadIdx = t0;
    blockIdx = b0;
    emu_fiber_body = nullptr;
    if (guard_from > 0)
        for (int i = guard_from; i < 160 * 1024; ++i)
            if (ap_smem[i] != (char)0xA5) { ++emu_lds_overruns; break; }
}
