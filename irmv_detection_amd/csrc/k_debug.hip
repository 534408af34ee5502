// LDS fill / probe (test hooks irmv_debug_lds_fill / irmv_debug_lds_probe; tests/test_gpu_lds_residue.py).  No production
// path launches these.
//
// LDS is not cleared between kernels: a workgroup that reads a word it has not written gets what the previous workgroup on
// that CU left there.  In a test suite that is nearly always the same kernel's own earlier data -- finite, plausible
// activations -- so such a read passes every bitwise comparison.  lds_fill_kernel lets a test choose the residue: every
// workgroup claims the whole 160 KiB a gfx950 workgroup may have (so exactly one is resident per CU, and the dispatcher
// spreads the grid over every CU), writes one pattern to every word and stays for kLdsDwellTicks so that the first round
// of workgroups is still resident when the last CU receives its own.  lds_probe_kernel has the same geometry, writes
// nothing and counts the words that still hold the pattern.
#include "irmv_common.hpp"

namespace irmv {

constexpr int kLdsThreads = 1024;
constexpr unsigned long long kLdsDwellTicks = 2000;   // of the 100 MHz wall clock: 20 us

__device__ __forceinline__ void lds_dwell(unsigned long long t0)
{
    while (wall_clock64() - t0 < kLdsDwellTicks) __builtin_amdgcn_s_sleep(8);
}

// (check: a word another lane wrote is read back after the barrier and a mismatch reported, so the stores have a reader)
__global__ __launch_bounds__(kLdsThreads) void lds_fill_kernel(uint32_t pattern, uint32_t *check)
{
    extern __shared__ uint32_t lds[];
    const unsigned long long t0 = wall_clock64();
    for (int i = threadIdx.x; i < kDebugLdsWords; i += kLdsThreads) lds[i] = pattern;
    __syncthreads();
    if (check && lds[(threadIdx.x * 41 + 7) % kDebugLdsWords] != pattern) atomicAdd(check, 1u);
    lds_dwell(t0);
}

// out[wg] = {words equal to the pattern, the value of word `word` (never written here), HW_ID, XCC_ID}; out is zero on entry.
// The kernel has no LDS variable of its own and writes no LDS word: the count goes through wave shuffles and global atomics.
__global__ __launch_bounds__(kLdsThreads) void lds_probe_kernel(uint32_t pattern, uint32_t word, uint32_t *out)
{
    extern __shared__ uint32_t lds[];
    const unsigned long long t0 = wall_clock64();
    uint32_t n = 0;
    for (int i = threadIdx.x; i < kDebugLdsWords; i += kLdsThreads) n += lds[i] == pattern;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
    uint32_t *o = out + (size_t)blockIdx.x * 4;
    if ((threadIdx.x & 63) == 0) atomicAdd(&o[0], n);
    if (threadIdx.x == 0) {
        o[1] = lds[word < (uint32_t)kDebugLdsWords ? word : 0u];
        o[2] = __builtin_amdgcn_s_getreg(4 | (31 << 11));    // HW_REG_HW_ID, all 32 bits: CU_ID [11:8], SH_ID [12], SE_ID [15:13]
        o[3] = __builtin_amdgcn_s_getreg(20 | (31 << 11));   // HW_REG_XCC_ID
    }
    lds_dwell(t0);
}

int debug_lds_workgroups(int cus) { return 4 * cus; }

hipError_t launch_lds_fill(uint32_t pattern, uint32_t *check, int workgroups, hipStream_t s)
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(lds_fill_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kDebugLdsWords * 4);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lds_fill_kernel, dim3(workgroups), dim3(kLdsThreads), kDebugLdsWords * 4, s, pattern, check);
    return hipGetLastError();
}

hipError_t launch_lds_probe(uint32_t pattern, uint32_t word, uint32_t *out, int workgroups, hipStream_t s)
{
    const int bytes = kDebugLdsWords * 4;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(lds_probe_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lds_probe_kernel, dim3(workgroups), dim3(kLdsThreads), bytes, s, pattern, word, out);
    return hipGetLastError();
}

}  // namespace irmv
