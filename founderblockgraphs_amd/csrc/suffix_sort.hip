// suffix_sort.hip -- the suffixes of the indexed text, sorted by their first symbols, and the choice of who finishes the index.
//
// Stands in for the suffix sorting inside sdsl::construct(cst, file, 1) (fbg.cpp:428): suffixes of
// T (bytes, unique smallest sentinel 0 at the end) in unsigned-byte lexicographic order.
//
// Every suffix gets a 64-bit key holding its first K symbols (alphabet compacted to b bits, K <= 64/b: keys.h) and the (key,
// position) slots are sorted: by the MSD sorts fused with the key packing (msd_sort.hip, msd_sort_pairs.hip) where the sizes suit
// them, else packed by k_pack and sorted by rocPRIM.  A sample of the keys tells rows that resemble each other (ties everywhere)
// from rows that differ.  Three paths (fbg_suffix_sort), and this file keeps the keys' geometry, the samples and the sorts:
//   ranked  a gap-free MSA: compact keys, then the whole extension scan in rank order (rank_scan.hip, pure_scan.hip);
//   pairs   any MSA: keys in the code of any alphabet with their values, then the span scan (span_scan.hip) or the
//           gapped rank scan (gapped_rank.hip) on the sorted slots;
//   record  what no scan in suffix order finished: prefix doubling to records by text position (record_sort.hip).
#include "fbg_internal.h"
#include "keys.h"
#include "sort_config.h"
#include "text_cmp.h"
#include "twin_hash.h"
#include <rocprim/rocprim.hpp>
#include <cmath>

#define SS_THREADS 256

// key[p] = the key of suffix p (keys.h), zero beyond the text.  Each thread owns PK_ITEMS consecutive positions: the rolling
// builder, one LDS byte read per position; COMPACT (rank-order scans only; positions beyond the text are separators too):
// symbol by symbol where a separator is in reach.  Such a key is the smallest one with its leading symbols, i.e. the suffix
// lands where it belongs up to ties, and the scan knows from the row arithmetic how many symbols of a key are real
// (rank_scan.hip).  LAYOUT (FBG_SLOTS_*): pairs, one packed word per suffix, or wide pairs.  FILTER: keep keys in [lo, hi)
// only, compacted in no particular order (partitioned index).
#define PK_ITEMS FBG_KEY_ITEMS
struct PackArgs {
    const uint8_t *T;
    uint64_t N;
    const uint8_t *code;
    int b, K, pb;
    uint64_t *keys;            // PACKED: items
    uint32_t *vals;
    uint64_t lo, hi, cap;      // FILTER
    int nohi;
    unsigned long long *counter;
    const uint64_t *ebits = nullptr;   // PAIRS: bit 31 of the value = an irregular position among the K from p on (gapped_rank.hip)
    const uint32_t *payload = nullptr; // PAIRS: the value of position p is payload[p] (span_scan.hip: cell | flags)
    const uint8_t *key_flags = nullptr; // PAIRS: two bits per position that go below the key (span_scan.hip, 2^30 cells and more)
};

// any irregular position among [p, p + K)?  (K <= 32; the bitmap is padded beyond the text)
__device__ __forceinline__ uint32_t pack_flag(const uint64_t *__restrict__ ebits, uint64_t p, int K)
{
    const uint64_t *e = ebits + (p >> 6);
    const unsigned sh = (unsigned)(p & 63);
    uint64_t bits = e[0] >> sh;
    if (sh) bits |= e[1] << (64 - sh);
    return (bits & ((1ull << K) - 1)) ? 0x80000000u : 0u;
}

template <bool COMPACT, int LAYOUT, bool FILTER>
__global__ __launch_bounds__(SS_THREADS) void k_pack(PackArgs a)
{
    constexpr int TILE = SS_THREADS * PK_ITEMS;
    __shared__ uint8_t tile[TILE + 64];      // symbol codes of the block's positions (+K lookahead)
    __shared__ uint8_t cd[256];
    __shared__ uint64_t skeys[TILE];         // keys leave through LDS so that the global stores are coalesced
    const int b = a.b, K = a.K;
    cd[threadIdx.x] = a.code[threadIdx.x];
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * TILE;
    for (int k = threadIdx.x; k < TILE + 64; k += SS_THREADS) {
        const uint64_t p = base + k;
        tile[k] = p < a.N ? cd[a.T[p]] : (COMPACT ? FBG_SEP : 0);
    }
    __syncthreads();
    const int t0 = threadIdx.x * PK_ITEMS;
    const uint32_t seen = fbg_keys_rolling(tile, t0, b, K, skeys + t0);
    if (COMPACT && (seen & FBG_SEP)) fbg_keys_by_symbol(tile, t0, b, K, skeys + t0);
    __syncthreads();
    if (!FILTER) {
#pragma unroll
        for (int i = 0; i < PK_ITEMS; i++) {
            const int j = threadIdx.x + i * SS_THREADS;
            const uint64_t p = base + j;
            if (p < a.N) {
                if (LAYOUT == FBG_SLOTS_PACKED) a.keys[p] = (skeys[j] << a.pb) | p;
                else if (LAYOUT == FBG_SLOTS_WIDE) { a.keys[p] = (skeys[j] << a.pb) | (p >> 32); a.vals[p] = (uint32_t)p; }
                else { a.keys[p] = a.key_flags ? (skeys[j] << 2) | a.key_flags[p] : skeys[j]; a.vals[p] = a.payload ? a.payload[p] : (uint32_t)p | (a.ebits ? pack_flag(a.ebits, p, K) : 0u); }
            }
        }
        return;
    }
    __shared__ uint32_t wsum[SS_THREADS / 64];
    __shared__ unsigned long long s_base;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long keep[PK_ITEMS];
    uint32_t wtot = 0;
#pragma unroll
    for (int i = 0; i < PK_ITEMS; i++) {
        const int j = threadIdx.x + i * SS_THREADS;
        const uint64_t kj = skeys[j];
        keep[i] = __ballot(base + j < a.N && kj >= a.lo && (a.nohi || kj < a.hi));
        wtot += (uint32_t)__popcll(keep[i]);
    }
    if (lane == 0) wsum[w] = wtot;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int q = 0; q < SS_THREADS / 64; q++) tot += wsum[q];
        s_base = tot ? atomicAdd(a.counter, (unsigned long long)tot) : 0ull;     // one counter update per workgroup
    }
    __syncthreads();
    uint64_t off = s_base;
    for (int q = 0; q < w; q++) off += wsum[q];
#pragma unroll
    for (int i = 0; i < PK_ITEMS; i++) {
        const int j = threadIdx.x + i * SS_THREADS;
        if ((keep[i] >> lane) & 1ull) {
            const uint64_t o = off + (uint64_t)__popcll(keep[i] & ((1ull << lane) - 1));
            if (o < a.cap) {
                const uint64_t p = base + j;
                if (LAYOUT == FBG_SLOTS_PACKED) a.keys[o] = (skeys[j] << a.pb) | p;
                else if (LAYOUT == FBG_SLOTS_WIDE) { a.keys[o] = (skeys[j] << a.pb) | (p >> 32); a.vals[o] = (uint32_t)p; }
                else { a.keys[o] = a.key_flags ? (skeys[j] << 2) | a.key_flags[p] : skeys[j]; a.vals[o] = a.payload ? a.payload[p] : (uint32_t)p | (a.ebits ? pack_flag(a.ebits, p, K) : 0u); }
            }
        }
        off += (uint64_t)__popcll(keep[i]);
    }
}

static void launch_pack(fbg_ctx *ctx, const KeyGeom &g, bool filter, PackArgs &a, const SortExtras &x)
{
    a.ebits = x.ebits; a.payload = x.payload;
    a.key_flags = x.key_flags ? ctx->sp_flagT.as<uint8_t>() : nullptr;
    const dim3 grid(fbg_blocks(a.N, SS_THREADS * PK_ITEMS)), block(SS_THREADS);
    hipStream_t st = ctx->stream;
#define FBG_PACK(C, L) do { if (filter) hipLaunchKernelGGL((k_pack<C, L, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_pack<C, L, false>), grid, block, 0, st, a); } while (0)
    if (!g.compact) FBG_PACK(false, FBG_SLOTS_PAIRS);
    else if (g.packed) FBG_PACK(true, FBG_SLOTS_PACKED);
    else if (g.wide) FBG_PACK(true, FBG_SLOTS_WIDE);
    else FBG_PACK(true, FBG_SLOTS_PAIRS);
#undef FBG_PACK
}

// keys of every stride-th position (same definition as k_pack): splitters and the regime pre-test
__device__ __forceinline__ uint64_t sample_key(const uint8_t *__restrict__ T, uint64_t N, const uint8_t *cd, int b, int K, int compact, uint64_t p)
{
    // the code table in LDS (cd), the text 8 bytes at a time (T is zero padded beyond N): K dependent byte loads through
    // a table in global memory made this small kernel take 0.3 ms
    uint64_t key = 0;
    bool dead = false;
    for (int k0 = 0; k0 < K; k0 += 8) {
        const uint64_t x = p + k0 < N ? fbg_load8(T, p + k0) : 0ull;
        for (int k = k0; k < K && k < k0 + 8; k++) {
            const uint32_t c = p + k < N ? cd[(x >> (8 * (k - k0))) & 255u] : (compact ? FBG_SEP : 0);
            key = (key << b) | fbg_key_symbol(c, compact, dead);
        }
    }
    return key;
}

__global__ void k_sample_keys(const uint8_t *__restrict__ T, uint64_t N, const uint8_t *__restrict__ code, int b, int K,
                              int compact, uint64_t stride, uint64_t S, uint64_t *__restrict__ out)
{
    __shared__ uint8_t cd[256];
    if (threadIdx.x < 256) cd[threadIdx.x] = code[threadIdx.x];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    out[i] = sample_key(T, N, cd, b, K, compact, i * stride);
}

// The same keys, not written out: every thread puts its key into an open-addressing table of 2^bits words (twin_hash.h;
// filled with all-ones, as are the two counter words behind it) and counts a twin when the key is there already.
// counters[0] += twins, counters[1] += keys that are all-ones themselves and cannot be stored: one atomic per wave each.
__global__ __launch_bounds__(256) void k_sample_twins(const uint8_t *__restrict__ T, uint64_t N, const uint8_t *__restrict__ code, int b, int K,
                                                      int compact, uint64_t stride, uint64_t S, unsigned long long *__restrict__ table, int bits)
{
    __shared__ uint8_t cd[256];
    cd[threadIdx.x] = code[threadIdx.x];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t twin = 0, ones = 0;
    if (i < S) {
        const uint64_t key = sample_key(T, N, cd, b, K, compact, i * stride);
        if (key == FBG_TWIN_EMPTY) ones = 1;
        else twin = fbg_twin_insert(key, bits, [&](uint64_t slot, uint64_t k) -> uint64_t {
            return atomicCAS(&table[slot], (unsigned long long)FBG_TWIN_EMPTY, (unsigned long long)k);
        });
    }
    unsigned long long *counters = table + (1ull << bits);
    const unsigned long long mt = __ballot(twin), mo = __ballot(ones);
    if ((threadIdx.x & 63) == 0) {
        if (mt) atomicAdd(&counters[0], (unsigned long long)__popcll(mt));
        if (mo) atomicAdd(&counters[1], (unsigned long long)__popcll(mo));
    }
}

__global__ void k_count_equal_neighbours(const uint64_t *__restrict__ keys, uint64_t S, unsigned long long *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool eq = i + 1 < S && keys[i] == keys[i + 1];
    __shared__ uint32_t blk;
    if (threadIdx.x == 0) blk = 0;
    __syncthreads();
    const unsigned long long m = __ballot(eq);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&blk, (uint32_t)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0 && blk) atomicAdd(out, (unsigned long long)blk);
}

// Alphabet compaction (order preserving) and the key geometry: b bits per symbol, K symbols per key.
// compact = true asks for the separator-free coding of the rank-order scan; g->compact tells whether it applies.
int fbg_key_setup(fbg_ctx *ctx, bool compact, KeyGeom *g, int *launches)
{
    const uint64_t N = ctx->N;
    hipStream_t st = ctx->stream;
    uint8_t *d_code = fbg_small(ctx)->code_tab;
    const uint64_t *hist = ctx->byte_hist;                // made by fbg_build_text
    if (hist[0] != 1)
        return fbg_fail(ctx, FBG_ERR_INVALID, "the MSA contains a NUL byte; the text needs a unique 0 sentinel");
    // the compact coding needs '#' to be smaller than every symbol of the rows, and room for the separator flag
    int below = 0, real = 0;
    for (int c = 1; c < 256; c++)
        if (hist[c] && c != '#') { real++; if (c < '#') below++; }
    compact = compact && below == 0 && real >= 1 && real < FBG_SEP;
    uint8_t *code = ctx->code_host;                       // (in the context: the copy below needs no wait)
    int sigma = 0;
    if (compact) {
        for (int c = 0; c < 256; c++) {
            if (c == 0 || c == '#') { code[c] = FBG_SEP; continue; }
            code[c] = (uint8_t)sigma;
            if (hist[c]) sigma++;
        }
    } else {
        for (int c = 0; c < 256; c++) { code[c] = (uint8_t)sigma; if (hist[c]) sigma++; }
    }
    int b = 1;
    while ((1 << b) < sigma) b++;
    // symbols per key: enough that only a few percent of the suffixes tie on the whole key (those are ordered by
    // text comparison afterwards), rounded up to whole 9-bit radix passes, at most 64 bits.  The symbol entropy H
    // of the text tells how many symbols that takes: ties ~ N * 2^(-H*K)  =>  K >= (log2 N + 5) / H.
    double H = 0;
    for (int c = 1; c < 256; c++)
        if (hist[c] && !(compact && c == '#')) { const double q = (double)hist[c] / (double)N; H -= q * log2(q); }
    if (H < 0.05) H = 0.05;
    int K = (int)ceil((log2((double)N) + 5.0) / H);
    if (ctx->opt.full_keys || K > 64 / b) K = 64 / b;
    {
        const int passes = (K * b + 8) / 9;                  // 9-bit digits
        const int Kfill = (9 * passes) / b;                  // symbols that fit the same number of passes
        K = Kfill < 64 / b ? Kfill : 64 / b;
    }
    g->compact = compact; g->packed = false; g->wide = false; g->pb = 0;
    if (N >= (1ull << 32) || (compact && ctx->opt.force_wide)) {
        // positions beyond 32 bits: their high bits ride in the low bits of the key word
        if (!compact) return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "text length %llu needs >32-bit positions", (unsigned long long)N);
        int pb = 1;
        while ((1ull << (32 + pb)) < N) pb++;
        g->wide = true; g->pb = pb;
        if (K > (64 - pb) / b) K = (64 - pb) / b;
    } else if (compact && !ctx->opt.no_packed) {
        // one 64-bit word per suffix if the position leaves room for enough symbols (ties up to ~10% are fine:
        // small tie groups are settled inside the scan)
        int pb = 1;
        while ((1ull << pb) < N) pb++;
        const int Kroom = (64 - pb) / b;
        const int Kmin = (int)ceil((log2((double)N) + 3.2) / H);
        if (Kroom >= Kmin) { g->packed = true; g->pb = pb; if (K > Kroom) K = Kroom; }
    }
    g->b = b; g->K = K; g->key_bits = K * b; g->d_code = d_code;
    fbg_note_key_geom(ctx, *g);
    FBG_HIP_TRY(ctx, hipMemcpyAsync(d_code, code, 256, hipMemcpyHostToDevice, st));
    *launches += 1;
    return FBG_OK;
}

// sorted (by key) slots of the first `count` entries of the A buffers -> B buffers (+ offset); key_flags: two flag bits
// below the key of a pair (span_scan.hip)
static int sort_slots(fbg_ctx *ctx, const KeyGeom &g, bool key_flags, uint64_t count, uint64_t out_offset)
{
    hipStream_t st = ctx->stream;
    uint64_t *ka = ctx->keysA.as<uint64_t>(), *kb = ctx->keysB.as<uint64_t>() + out_offset;
    if (g.packed) {
        // rocPRIM 7.2's merge-sort path (inputs below a few million words) mis-sorts a bit range that starts above
        // bit 0 and ends at bit 64 (scripts/micro/sortcheck.hip); whole words sort correctly and cost nothing there
        unsigned lo = (unsigned)g.pb;
        const unsigned hi = (unsigned)(g.pb + g.key_bits);
        if (hi == 64 && count < (1u << 23)) lo = 0;
        return fbg_with_tmp(ctx, [&](void *tmp, size_t &bytes) {
            return rocprim::radix_sort_keys<fbg_sort_config>(tmp, bytes, ka, kb, (size_t)count, lo, hi, st);
        });
    }
    uint32_t *va = ctx->valsA.as<uint32_t>(), *vb = ctx->valsB.as<uint32_t>() + out_offset;
    unsigned lo = g.wide ? (unsigned)g.pb : key_flags ? 2u : 0u;
    const unsigned hi = lo + (unsigned)g.key_bits;
    if (hi == 64 && count < (1u << 23)) lo = 0;        // same caution as above
    return fbg_with_tmp(ctx, [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs<fbg_sort_config>(tmp, bytes, ka, kb, va, vb, (size_t)count, lo, hi, st);
    });
}

// k_pack's arguments for the slots of (ctx, g) into the A buffers, every position kept (a filter adds range, cap and counter)
static PackArgs pack_args(fbg_ctx *ctx, const KeyGeom &g)
{
    PackArgs pa;
    pa.T = ctx->text.as<uint8_t>(); pa.N = ctx->N; pa.code = g.d_code; pa.b = g.b; pa.K = g.K; pa.pb = g.pb;
    pa.keys = ctx->keysA.as<uint64_t>(); pa.vals = ctx->valsA.as<uint32_t>();
    pa.lo = pa.hi = pa.cap = 0; pa.nohi = 1; pa.counter = nullptr;
    return pa;
}

static int reserve_slots(fbg_ctx *ctx, const KeyGeom &g)
{
    for (DevBuf *d : {&ctx->keysA, &ctx->keysB}) FBG_TRY(fbg_reserve(ctx, *d, ctx->N * 8));
    if (!g.packed) for (DevBuf *d : {&ctx->valsA, &ctx->valsB}) FBG_TRY(fbg_reserve(ctx, *d, ctx->N * 4));
    return FBG_OK;
}

// where the sort fused with the packing declines: all N slots packed into the A buffers, sorted by rocPRIM into the B buffers
static int pack_and_sort(fbg_ctx *ctx, const KeyGeom &g, const SortExtras &x, int *launches)
{
    FBG_TRY(reserve_slots(ctx, g));
    PackArgs pa = pack_args(ctx, g);
    launch_pack(ctx, g, false, pa, x);
    *launches += 1;
    return sort_slots(ctx, g, x.key_flags, ctx->N, 0);
}

// ---- the key sample ----------------------------------------------------------------------------------------------------------
// Rows that resemble each other tie on almost every key: the rank-order scan is not for them.  Cheap look before
// the sort: twins among the keys of a sample (the exact test follows after the sort, rank_scan.hip).
//
// Option twin_hash (default 1): one kernel counts the twins with an open-addressing table (k_sample_twins, twin_hash.h) and
// the count travels to pinned words of the context; nobody waits.  sample_verdict reads it where the answer is first needed.
// twin_hash = 0: the sample is written out, sorted by rocPRIM (22 launches) and equal neighbours are counted; the host waits.
#define SS_SAMPLE_LOG 20                       // keys in the sample of the verdict: 2^20, from texts of 2^22 symbols on

static int sample_launch(fbg_ctx *ctx, const KeyGeom &g, int *launches)
{
    const uint64_t N = ctx->N;
    hipStream_t st = ctx->stream;
    ctx->twin_pending = false;
    if (N < (1u << 22)) return FBG_OK;
    constexpr int BITS = SS_SAMPLE_LOG + FBG_TWIN_SPARE;
    const uint64_t S = 1u << SS_SAMPLE_LOG, stride = N / S;
    if (!ctx->pin_twins) {
        FBG_HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->pin_twins), 2 * sizeof(unsigned long long), hipHostMallocDefault));
        FBG_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->twin_ev, hipEventDisableTiming));
    }
    FBG_TRY(fbg_reserve(ctx, ctx->dp_g, ((1ull << BITS) + 2) * 8));
    unsigned long long *table = ctx->dp_g.as<unsigned long long>();
    FBG_HIP_TRY(ctx, hipMemsetAsync(table, 0xff, ((1ull << BITS) + 2) * 8, st));       // the table and its two counters: one fill
    hipLaunchKernelGGL(k_sample_twins, dim3(fbg_blocks(S, 256)), dim3(256), 0, st, ctx->text.as<uint8_t>(), N, g.d_code, g.b, g.K,
                       g.compact ? 1 : 0, stride, S, table, BITS);
    FBG_HIP_TRY(ctx, hipMemcpyAsync(ctx->pin_twins, table + (1ull << BITS), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipEventRecord(ctx->twin_ev, st));
    ctx->twin_pending = true;
    *launches += 1;
    return FBG_OK;
}

static bool twins_say_similar(fbg_ctx *ctx, uint64_t twins)
{
    ctx->diag.sample_twins = (int64_t)twins;
    return fbg_twins_say_similar(twins, ctx->N, 1u << SS_SAMPLE_LOG);
}

// the answer of the sample sample_launch started (false when the text was too short for one); waits for the count only
// when the stream has not got that far yet
static int sample_verdict(fbg_ctx *ctx, bool *similar)
{
    *similar = false;
    if (!ctx->twin_pending) return FBG_OK;
    ctx->twin_pending = false;
    FBG_HIP_TRY(ctx, hipEventSynchronize(ctx->twin_ev));
    *similar = twins_say_similar(ctx, fbg_twin_total(ctx->pin_twins[0], ctx->pin_twins[1]));
    return FBG_OK;
}

// the keys of the S positions `stride` apart, written out (dp_g) and sorted by rocPRIM (dp_h, *sorted): two launches
static int sorted_sample(fbg_ctx *ctx, const KeyGeom &g, uint64_t S, uint64_t stride, const uint64_t **sorted)
{
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_reserve(ctx, ctx->dp_g, S * 8));
    FBG_TRY(fbg_reserve(ctx, ctx->dp_h, S * 8));
    uint64_t *smp = ctx->dp_g.as<uint64_t>(), *srt = ctx->dp_h.as<uint64_t>();
    hipLaunchKernelGGL(k_sample_keys, dim3(fbg_blocks(S, 256)), dim3(256), 0, st, ctx->text.as<uint8_t>(), ctx->N, g.d_code, g.b, g.K,
                       g.compact ? 1 : 0, stride, S, smp);
    *sorted = srt;
    return fbg_with_tmp(ctx, [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_keys(tmp, bytes, smp, srt, (size_t)S, 0u, (unsigned)g.key_bits, st);
    });
}

// equal neighbours among the S keys of a sorted sample, counted in the caller's scalar word and brought back (the host waits)
int fbg_count_equal_neighbours(fbg_ctx *ctx, const uint64_t *sorted, uint64_t S, unsigned long long *d_word, unsigned long long *twins)
{
    hipStream_t st = ctx->stream;
    FBG_HIP_TRY(ctx, hipMemsetAsync(d_word, 0, 8, st));
    hipLaunchKernelGGL(k_count_equal_neighbours, dim3(fbg_blocks(S, 256)), dim3(256), 0, st, sorted, S, d_word);
    FBG_HIP_TRY(ctx, hipMemcpyAsync(twins, d_word, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return FBG_OK;
}

static int sample_says_similar(fbg_ctx *ctx, const KeyGeom &g, bool *similar, int *launches)
{
    const uint64_t N = ctx->N, S = 1u << SS_SAMPLE_LOG;
    *similar = false;
    if (ctx->opt.twin_hash) {
        FBG_TRY(sample_launch(ctx, g, launches));
        return sample_verdict(ctx, similar);
    }
    if (N < (1u << 22)) return FBG_OK;
    const uint64_t *srt = nullptr;
    unsigned long long twins = 0;
    FBG_TRY(sorted_sample(ctx, g, S, N / S, &srt));
    FBG_TRY(fbg_count_equal_neighbours(ctx, srt, S, &fbg_scalars(ctx)->sample_count, &twins));
    *launches += 3;
    *similar = twins_say_similar(ctx, twins);
    return FBG_OK;
}

// ---- the three paths -----------------------------------------------------------------------------------------------------------
// A gap-free MSA without ignore characters: compact keys (keys.h), sort, and the whole extension scan in rank order.  A byte
// below '#' or 128 distinct symbols and more leave the keys in the coding of any alphabet: not done, the other paths take those.
static int ranked_path(fbg_ctx *ctx, int *done, int *launches)
{
    KeyGeom g;
    // (a streamed upload has set the keys up and run pass 1 of the sort already: same geometry)
    if (!fbg_msd_pre_geom(ctx, &g)) FBG_TRY(fbg_key_setup(ctx, true, &g, launches));
    if (!g.compact) return FBG_OK;
    // (nothing before the sort reads the sample's answer: with twin_hash it is fetched behind the sort, which has waited
    // on the stream by then)
    bool similar = false;
    if (ctx->opt.twin_hash) FBG_TRY(sample_launch(ctx, g, launches));
    else FBG_TRY(sample_says_similar(ctx, g, &similar, launches));
    // packed slots of a large text: three-pass MSD sort fused with the key packing (msd_sort.hip); else, or when
    // its optimistic bucket capacities do not hold, pack and sort with rocPRIM's onesweep
    uint64_t *sorted = nullptr;
    int msd_ok = 0;
    FBG_TRY(fbg_msd_sort(ctx, g, &sorted, &msd_ok, launches));
    if (!msd_ok) {
        FBG_TRY(pack_and_sort(ctx, g, SortExtras(), launches));
        sorted = ctx->keysB.as<uint64_t>();
    }
    uint32_t *svals = g.packed ? nullptr : ctx->valsB.as<uint32_t>();
    if (ctx->opt.twin_hash) FBG_TRY(sample_verdict(ctx, &similar));
    // rows that differ: the scan slot by slot (rank_scan.hip).  Rows that resemble each other (judged from key twins in a
    // sample, or by the slot-level scan itself, which gives up where a quarter of the slots tie): group by group
    if (!similar && ctx->opt.pure_scan != 1) FBG_TRY(fbg_rank_scan_try(ctx, sorted, svals, g, done));
    if (!*done && ctx->opt.pure_scan != -1) FBG_TRY(fbg_pure_scan_try(ctx, sorted, svals, g, done));
    return FBG_OK;
}

// Any MSA: all suffixes sorted by their first K symbols as (key, value) pairs, keys in the code of any alphabet (*g), into keysB /
// valsB; then the scan in suffix order that suits the input, if one does.  Not done: the values are the text positions again.
static int pairs_path(fbg_ctx *ctx, KeyGeom *g, int *done, int *launches)
{
    SortExtras x;
    FBG_TRY(fbg_key_setup(ctx, false, g, launches));
    FBG_TRY(reserve_slots(ctx, *g));
    ctx->pairs_similar = false;
    // rows that resemble each other (twins among the keys of a sample; option span_scan = 1: whatever the rows): the
    // group-level scan on column spans (span_scan.hip), whose sort carries cells instead of positions
    bool try_span = fbg_span_eligible(ctx, *g);
    if (try_span && ctx->opt.span_scan != 1 && ctx->opt.span_scan != 3) FBG_TRY(sample_says_similar(ctx, *g, &try_span, launches));
    // MSAs with gaps / ignore characters: the scan in rank order follows the sort (gapped_rank.hip); its table of the
    // text's irregular positions is made now, the pack kernels fold it into the values' top bit
    const bool try_grs = !try_span && (!ctx->gapfree || ctx->have_ignore) && !ctx->reversed && !ctx->grs_skip && ctx->opt.gapped_rank != -1 && g->K <= 32;
    if (try_grs || try_span) FBG_TRY(fbg_grs_prepare(ctx, &x.ebits, launches));
    if (try_span) {
        x.ebits = nullptr; ctx->ix.grs_flagged = false;               // (the bitmap goes into the cells' flags instead)
        x.key_flags = fbg_span_key_flags(ctx, *g);                    // (2^30 cells and more: may shorten the key by a symbol)
        FBG_TRY(fbg_span_prepare(ctx, *g, x, launches));
        x.payload = ctx->sp_cells.as<uint32_t>();
    }
    // three passes of a sample sort fused with the key packing (msd_sort_pairs.hip) where the sizes suit it; else,
    // or when a capacity does not hold, pack and sort with rocPRIM's onesweep
    int ss_ok = 0;
    FBG_TRY(fbg_sample_sort_pairs(ctx, *g, x, &ss_ok, launches));
    if (!ss_ok) FBG_TRY(pack_and_sort(ctx, *g, x, launches));
    ctx->ix.sp_key_flags_sorted = x.key_flags;
    // (the sample sort sizes the buffers itself: their addresses are taken behind it)
    uint64_t *keys = ctx->keysB.as<uint64_t>();
    uint32_t *vals = ctx->valsB.as<uint32_t>();
    ctx->ix.sa_ptr = vals;                     // the sorted positions ARE the suffix array
    if (try_span) return fbg_span_try(ctx, keys, vals, *g, done);    // (declined: the values are text positions again)
    if (!try_grs) return FBG_OK;
    // similar rows: tie groups of hundreds, not for that scan
    if (!ctx->pairs_similar) FBG_TRY(fbg_grs_try(ctx, keys, vals, *g, done));
    if (!*done) FBG_TRY(fbg_grs_strip(ctx, vals));    // the record path reads the values as the suffix array
    return FBG_OK;
}

int fbg_suffix_sort(fbg_ctx *ctx)
{
    FBG_TRY(fbg_stage_begin(ctx, FBG_STAGE_SUFFIX_SORT));
    int launches = 0, done = 0;
    KeyGeom g;
    if (ctx->gapfree && !ctx->have_ignore && !ctx->opt.no_ranked) FBG_TRY(ranked_path(ctx, &done, &launches));
    if (!done) FBG_TRY(pairs_path(ctx, &g, &done, &launches));
    if (!done) FBG_TRY(fbg_record_sort(ctx, g, &launches));
    FBG_HIP_TRY(ctx, hipGetLastError());
    return fbg_stage_end(ctx, FBG_STAGE_SUFFIX_SORT, launches);
}


// ---- partitioned index: this GPU sorts only the suffixes whose key lies in its range ------------------------
// Every rank of a multi-GPU job holds the whole text (MSAs are small next to their index: 1 byte per symbol
// against 16-24 bytes of sort state), computes the same splitters from the same key sample, and then packs,
// sorts and scans only its own key range: sort state and sort time divide by the number of GPUs.  The ranks
// exchange nothing but FBG_PART_HALO edge slots each and the per-column maxima (rank_scan.hip, distributed.py).
int fbg_part_sort(fbg_ctx *ctx, int part, int nparts, uint8_t *d_blob, int *ok)
{
    const uint64_t N = ctx->N;
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_stage_begin(ctx, FBG_STAGE_SUFFIX_SORT));
    int launches = 0;
    KeyGeom g;
    SortExtras x;
    int pre_ok = ctx->gapfree && !ctx->have_ignore && !ctx->opt.no_ranked;
    FBG_TRY(fbg_key_setup(ctx, pre_ok != 0, &g, &launches));
    pre_ok = pre_ok && g.compact;
    // MSAs with gaps / ignore characters: the same partitioning on (key, position) pairs in the code of any alphabet,
    // scanned by gapped_rank.hip
    const bool gapped = (!ctx->gapfree || ctx->have_ignore) && !ctx->reversed && ctx->opt.gapped_rank != -1 && !g.compact && g.K <= 32 &&
                        N < (1ull << 32);
    if (gapped) FBG_TRY(fbg_grs_prepare(ctx, &x.ebits, &launches));
    if (pre_ok) {
        // similar rows tie almost everywhere: not for the slot-level scan of the partitions (every rank draws the same
        // sample and declines alike); the caller builds the whole index, whose group-level scan is made for them
        bool similar = false;
        FBG_TRY(sample_says_similar(ctx, g, &similar, &launches));
        if (similar) pre_ok = 0;
    }
    ctx->ix.part = part; ctx->ix.nparts = nparts; ctx->ix.part_active = true;
    uint64_t count = 0;
    // splitters: quantiles of a sorted key sample -- the same on every rank, ties never straddle a boundary
    uint64_t S = N / 64;
    if (S > (1u << 20)) S = 1u << 20;
    if (S < 1024) S = N < 1024 ? N : 1024;
    const uint64_t stride = N / S;
    uint64_t lo = 0, hi = 0;
    if ((pre_ok || gapped) && nparts > 1) {
        const uint64_t *smp_sorted = nullptr;
        FBG_TRY(sorted_sample(ctx, g, S, stride, &smp_sorted));
        launches += 2;
        if (part > 0)
            FBG_HIP_TRY(ctx, hipMemcpyAsync(&lo, smp_sorted + (uint64_t)part * S / nparts, 8, hipMemcpyDeviceToHost, st));
        if (part + 1 < nparts)
            FBG_HIP_TRY(ctx, hipMemcpyAsync(&hi, smp_sorted + (uint64_t)(part + 1) * S / nparts, 8, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    int msd_ok = 0;
    if (pre_ok)     // three passes over 12-byte slots, packing and filtering fused into the first (msd_sort_pairs.hip)
        FBG_TRY(fbg_msd_sort_part(ctx, g, lo, hi, part + 1 >= nparts, nparts, FBG_PART_HALO, &count, &msd_ok, &launches));
    if ((pre_ok || gapped) && !msd_ok) {
        unsigned long long *d_count = &fbg_scalars(ctx)->sample_count;
        uint64_t cap = N / nparts + N / 8 + 65536;
        if (cap > N) cap = N;
        for (int attempt = 0; attempt < 2; attempt++) {
            FBG_TRY(fbg_reserve(ctx, ctx->keysA, cap * 8));
            if (!g.packed) FBG_TRY(fbg_reserve(ctx, ctx->valsA, cap * 4));
            FBG_HIP_TRY(ctx, hipMemsetAsync(d_count, 0, 8, st));
            PackArgs pa = pack_args(ctx, g);
            pa.lo = lo; pa.hi = hi; pa.cap = cap; pa.nohi = part + 1 >= nparts; pa.counter = d_count;
            launch_pack(ctx, g, true, pa, x);
            launches++;
            unsigned long long hc = 0;
            FBG_HIP_TRY(ctx, hipMemcpyAsync(&hc, d_count, 8, hipMemcpyDeviceToHost, st));
            FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
            count = hc;
            if (count <= cap) break;
            cap = count;                               // a skewed sample: once more with room for all of them
        }
    }
    const uint64_t slots = count + 2 * FBG_PART_HALO;
    FBG_TRY(fbg_reserve(ctx, ctx->keysB, slots * 8));
    if (!g.packed) FBG_TRY(fbg_reserve(ctx, ctx->valsB, slots * 4));
    if ((pre_ok || gapped) && !msd_ok && count > 0) FBG_TRY(sort_slots(ctx, g, false, count, FBG_PART_HALO));
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_TRY(fbg_stage_end(ctx, FBG_STAGE_SUFFIX_SORT, launches));
    if (gapped)
        return fbg_grs_part_classify(ctx, ctx->keysB.as<uint64_t>(), ctx->valsB.as<uint32_t>(), count, g, 1, d_blob, ok);
    return fbg_rank_part_classify(ctx, ctx->keysB.as<uint64_t>(), g.packed ? nullptr : ctx->valsB.as<uint32_t>(), count, g,
                                  pre_ok, d_blob, ok);
}
