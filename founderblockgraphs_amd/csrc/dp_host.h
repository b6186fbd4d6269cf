// dp_host.h -- what the host code of dp.hip, dp_bytes.hip and dp_wide.hip shares: the state of a sweep, the rungs that live
// in another file, and the runtime R as a template argument.
#pragma once
#include <type_traits>
#include "fbg_internal.h"
#include "dp_plan.h"

// What the rungs of fbg_dp_minmax's ladder (dp_plan.h) share.  A rung launches its kernels, counts itself in ctx->dp_attempts
// and ends in fbg_dp_settled.
struct DpSweep {
    uint64_t n = 0;
    uint32_t first_valid = 0;               // f[0] + 1: no block ends before that step (k_dp_expand)
    const uint32_t *e = nullptr;            // f[x] + 1 (k_dp_keys)
    uint32_t *mml = nullptr, *bt = nullptr; // minmaxlength[], backtrack[]
    unsigned long long *sc = nullptr;       // FbgScalars::dp
    bool buckets_ready = false;             // dp.hip: the bucket order of the wave and the literal sweep is built
    bool wide_built = false, wide_declined = false;   // dp_wide.hip
};
// a rung with a window clears the window word before its launches and after them copies, waits for and tests it: its one wait
int fbg_dp_clear_window(fbg_ctx *ctx, unsigned long long *sc);                                           // dp.hip
int fbg_dp_settled(fbg_ctx *ctx, unsigned long long *sc, bool *settled);                                 // dp.hip
int fbg_rung_bytes(fbg_ctx *ctx, DpSweep &sw, const DpRung &r, bool *settled);                           // dp_bytes.hip
int fbg_rung_wide(fbg_ctx *ctx, DpSweep &sw, const DpRung &r, bool *settled);                            // dp_wide.hip
// the runtime R as a template argument: fn(std::integral_constant<int, R>), R = 1, 2, 4 and, with RMAX = 16, 8 and 16
// (an R outside that set goes to the largest instance, 4 or 16, as the switches before did; no caller passes one: dp_plan caps
// the BYTES rungs at 4, the non-elastic DP's dp_tier is capped at 4, and a WAVE rung carries dp_tier's R)
template <int RMAX, class F> inline int dp_for_R(int R, F &&fn)
{
    if (R == 1) return fn(std::integral_constant<int, 1>());
    if (R == 2) return fn(std::integral_constant<int, 2>());
    if constexpr (RMAX > 4) {
        if (R == 8) return fn(std::integral_constant<int, 8>());
        if (R != 4) return fn(std::integral_constant<int, 16>());
    }
    return fn(std::integral_constant<int, 4>());
}
