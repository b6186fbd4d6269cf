// dp_dev.h -- the device-side pieces that two of dp.hip, dp_bytes.hip and dp_wide.hip share, nothing else.
#pragma once
#include <cstdint>

#define DP_NONE 0xffffffffu
#define DPW 1024   // steps / items staged in LDS per refill (multiple of 64): k_dp_wave, k_dp_tile
#define DPB_INF 255u
typedef unsigned short dp_u16x2 __attribute__((ext_vector_type(2)));      // v_pk_max_u16 / v_pk_min_u16 operands
__device__ __forceinline__ dp_u16x2 dp_bits(uint32_t x) { return __builtin_bit_cast(dp_u16x2, x); }
__device__ __forceinline__ uint32_t dp_word(dp_u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ dp_u16x2 dp_pair(uint32_t x) { return dp_bits(x | (x << 16)); }

// A barrier between phases that exchange through LDS only: __syncthreads() also waits for every global load and store in flight
// (its fence covers global memory), which would put the latency of the rows fetched ahead back on every step of a chain
//
// THE BARRIER COUNT.  k_dp_chain6 and k_dpw_chain2 are one workgroup each whose waves play different roles (the waves that
// compute, the one that stores, the one that touches lines ahead), and every role walks the groups / blocks in a loop of its
// own.  s_barrier counts arrivals, it does not know which barrier of the source a wave stands at: the kernels are correct only
// because every role's loop executes exactly the same number of dpw_lds_barrier() per group -- one in k_dp_chain6, three in
// k_dpw_chain2 (one under its timing-only probe bit 128) -- in every wave, for every group, the last one included.  A `continue`, `break` or `return` inside one role's
// loop that skips a barrier, or a barrier under a condition that is not uniform over the whole workgroup, leaves the other
// waves waiting for an arrival that never comes: the single workgroup hangs, and nothing else on the device notices.  A role
// may leave only after its loop (as the storing and the touching waves do).
__device__ __forceinline__ void dpw_lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
