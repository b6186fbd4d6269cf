// dp_plan.h -- which sweeps fbg_dp_minmax tries for an input, and in which order.  Host only, no HIP: pure functions of
// max_ext (the longest f[x] + 1 - x, k_dp_keys), f[0], n and four options; no kernel launch appears here
// (fbg_host_selftest dp_plan prints the plans, tests/test_dp_plan_host.py compares them with the rule of DESIGN.md 6).
//
// The ladder is flat.  With R = dp_tier(2 max_ext + 2, f[0]), taken as 0 under dp_literal or when f[0] >= n, the order is
//   1. BYTES(Rt)  iff R != 0 and (!dp_wave or f[0] != 0): Rt from the smallest of 1, 2, 4 with 64 Rt >= max_ext + 2 (4 beyond
//                 that), or from R under dp_safe_window, doubling while Rt <= 4 and Rt <= R
//   2. WIDE(WS)   iff dp_wide_ok: WS from the smallest of 1024 .. 16384 that is >= max_ext + 2, up to 16384
//   3. WAVE(R)    iff R != 0 and f[0] == 0 and (R > 4 or dp_wave)
//   4. LITERAL    always
// and a rung runs when none before it settled.  Whether a rung is there does not depend on what ran before it.
// A quirk that is kept: the byte matrices end at Rt = 4, so dp_safe_window with R = 8 or 16 gives no BYTES rung at all.
#pragma once
#include <cstdint>

enum DpFamily { DP_BYTES, DP_WIDE, DP_WAVE, DP_LITERAL };
struct DpRung {
    DpFamily family;
    uint32_t size;      // BYTES: Rt (a window of 64 Rt columns), WIDE: WS, WAVE: R, LITERAL: 0
    bool tile;          // BYTES(1) in its k_dp_tile form (dp_tile, f[0] == 0)
};
struct DpPlanOptions { bool literal, wave, safe_window, tile; };
struct DpPlan {
    static constexpr int CAP = 12;   // at most 3 BYTES + 5 WIDE + WAVE + LITERAL
    DpRung rung[CAP];
    int count = 0;
    void add(DpFamily family, uint32_t size, bool tile = false) { rung[count++] = DpRung{family, size, tile}; }
};

constexpr uint64_t DP_WIDE_MIN_N = 256;          // two blocks of the wide chain (2 * DPW_B, dp_wide.hip)
constexpr uint32_t DP_WIDE_MAX_WS = 16384;

// R = window / 64 that holds every value: minmaxlength[j] <= bound - 1.  The byte matrices reach R = 4 (254: 255 is their
// "none"), the wave sweep 8 and 16 and needs f[0] == 0; 0 = no tier.  The non-elastic DP has no wave sweep and asks with
// f0 != 0: its cap is 4.
inline int dp_tier(unsigned long long bound, uint64_t f0)
{
    return bound <= 64 ? 1 : bound <= 128 ? 2 : bound <= 254 ? 4 : (f0 == 0 && bound <= 512) ? 8 : (f0 == 0 && bound <= 1024) ? 16 : 0;
}

// extensions of hundreds of columns: the matrix chain with 16-bit entries (dp_wide.hip)
inline bool dp_wide_ok(unsigned long long max_ext, uint64_t f0, uint64_t n, const DpPlanOptions &o)
{
    return f0 < n && !o.literal && !o.wave && max_ext + 2 > 256 && max_ext + 2 <= DP_WIDE_MAX_WS && n >= DP_WIDE_MIN_N;
}

inline DpPlan dp_plan(unsigned long long max_ext, uint64_t f0, uint64_t n, const DpPlanOptions &o)
{
    DpPlan p;
    const int R = (o.literal || f0 >= n) ? 0 : dp_tier(2 * max_ext + 2, f0);
    if (R != 0 && (!o.wave || f0 != 0)) {
        // the window that is provably enough (64 R >= 2 max_ext + 2) is rarely needed: the smallest one that holds every
        // extension first, wider ones when a value reaches the limit
        int Rt = 1;
        while (64ull * Rt < max_ext + 2 && Rt < 4) Rt *= 2;
        if (o.safe_window) Rt = R;
        for (; Rt <= 4 && Rt <= R; Rt *= 2) p.add(DP_BYTES, (uint32_t)Rt, Rt == 1 && o.tile && f0 == 0);
    }
    if (dp_wide_ok(max_ext, f0, n, o)) {
        uint32_t WS = 1024;
        while (WS < max_ext + 2) WS *= 2;
        for (; WS <= DP_WIDE_MAX_WS; WS *= 2) p.add(DP_WIDE, WS);
    }
    if (R != 0 && f0 == 0 && (R > 4 || o.wave)) p.add(DP_WAVE, (uint32_t)R);
    p.add(DP_LITERAL, 0);
    return p;
}

// dp_kind of the rung that settled: 1 byte matrices, 3 .. 7 the wide chain with WS = 1024 .. 16384, 2 wave sweep, 0 literal
inline int dp_kind_of(const DpRung &r)
{
    switch (r.family) {
    case DP_BYTES: return 1;
    case DP_WIDE: { int k = 3; for (uint32_t w = 1024; w < r.size; w *= 2) k++; return k; }
    case DP_WAVE: return 2;
    default: return 0;
    }
}
