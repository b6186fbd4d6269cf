// locate.hip -- batched pattern search in the pattern index of a founder graph (the reference's backward_search,
// founder_block_index.hpp:86-145) and the places of what it finds.  pindex.h lists the other files of the index.
//
//   k_px_walk<true>                  the batched search of rule 4 (restarts included), one lane per pattern,
//                                    patterns handed out in order of length;
//   k_px_walk<true, *, true>         the same search for fbg_pindex_occurrences: it also keeps the final range, the
//                                    range after the '#' step of the first restart and the restart count;
//   k_px_walk<false>                 B / E of a build: every label searched from [0, N], flags at lhs / rhs;
//   k_px_seeds                       fbg_pindex_seeds: that search run to the end of every read, restarted from [0, N]
//                                    wherever it stops; a counting instantiation and a writing one (one record per
//                                    maximal piece, which k_po_sizes / k_po_expand then treat as a pattern);
//   k_po_sizes / k_po_expand         capped list sizes per pattern (scanned into CSR offsets), then one lane per
//                                    reported place: SA slot -> (edge source, edge destination, offset);
//   k_po_expand_msa                  k_po_expand's walk from a reported place to its edge and offset, then through the
//                                    MSA coordinate table to the MSA row and column of the place.
#include "pindex_dev.h"
#include <rocprim/rocprim.hpp>
// tests/test_chain_edges.py as it stood before the split reads these here; a copy that differs from pindex.h is an error
#pragma clang diagnostic error "-Wmacro-redefined"
#define PX_THREADS 256
#define PC_SUB 16
#define PC_SMALL 32
#define PC_LDS 1024

// One lane per pattern.  SEARCH: rule 4 of the index (a failed step may restart at a block pair boundary), results
// count / pos by pattern id, patterns taken in the order `order` (by length).  !SEARCH: B / E of the node labels, no
// restart; a label whose search finds nothing sets no flag (the reference asserts there); every label's range goes to
// rng[id] = (l, r), (1, 0) when nothing was found, for fbg_pindex_validate.  OCC (with SEARCH): the search also records
// rng[3 id] = the final (l, r), rng[3 id + 1] = (sl, sr), the range after the '#' step of the first restart that went
// on, rng[3 id + 2] = (symbols matched at that restart, restarts that went on), for fbg_pindex_occurrences.
template <bool SEARCH, bool COMPACT, bool OCC = false>
__global__ __launch_bounds__(PX_THREADS) void k_px_walk(PxDev d, const uint16_t *code_g, const uint32_t *C_g, const uint8_t *pats,
                                                       const uint64_t *poff, const uint32_t *order, uint64_t n,
                                                       unsigned long long *count_out, unsigned long long *pos_out,
                                                       uint8_t *bflag, uint8_t *eflag, unsigned long long *lines_ctr,
                                                       uint2 *rng)
{
    __shared__ uint16_t code[256];
    __shared__ uint32_t C[256];
    for (int c = threadIdx.x; c < 256; c += blockDim.x) { code[c] = code_g[c]; C[c] = C_g[c]; }
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t nlines = 0;
    if (t < n) {
        const uint64_t id = order ? order[t] : t;
        const uint64_t a = poff[id], len = poff[id + 1] - a;
        uint32_t l = 0, r = d.N, cnt = 0;
        uint64_t pos = 0, word = 0;
        bool ok = true;
        uint32_t restarts = 0, fsl = 1, fsr = 0, fk = 0;
        for (uint64_t k = 0; k < len; k++) {
            const uint64_t q = a + k;
            if (k == 0 || (q & 7) == 0) word = *(const uint64_t *)(pats + (q & ~7ull));   // buffer padded to 8 bytes
            const uint32_t ch = (uint32_t)(word >> (8 * (q & 7))) & 0xffu;
            uint32_t nl, nr;
            cnt = px_bs<COMPACT>(d, code, C, ch, l, r, nl, nr, nlines);
            if (cnt) {
                l = nl; r = nr;
            } else {
                if (!SEARCH) { ok = false; break; }
                // restart: the range must be able to step over '#', and B / E must enclose it
                uint32_t sl, sr;
                if (!px_bs<COMPACT>(d, code, C, '#', l, r, sl, sr, nlines)) { ok = false; break; }
                uint32_t lo = 0, hi = d.nb;       // r1 = #B positions <= l
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) / 2;
                    if (d.bpos[mid] <= l) lo = mid + 1; else hi = mid;
                }
                const uint32_t r1 = lo;
                if (r1 == 0 || r1 > d.ne) { ok = false; break; }
                const uint32_t bl = d.bpos[r1 - 1], br = d.epos[r1 - 1];
                if (!(bl <= l && r <= br)) { ok = false; break; }
                cnt = px_bs<COMPACT>(d, code, C, ch, bl, br, nl, nr, nlines);
                if (!cnt) { ok = false; break; }
                if (OCC) {
                    if (!restarts) { fsl = sl; fsr = sr; fk = (uint32_t)pos; }
                    restarts++;
                }
                l = nl; r = nr;
            }
            pos++;
        }
        if (SEARCH) {
            count_out[id] = ok ? cnt : 0u;
            pos_out[id] = pos;
            if (OCC) {
                rng[3 * id] = make_uint2(l, r);
                rng[3 * id + 1] = make_uint2(fsl, fsr);
                rng[3 * id + 2] = make_uint2(fk, restarts);
            }
        } else {
            if (ok) {
                bflag[l] = 1;
                eflag[r] = 1;
            }
            rng[id] = ok ? make_uint2(l, r) : make_uint2(1u, 0u);
        }
    }
    if (SEARCH) {
        unsigned long long s = nlines;
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((threadIdx.x % FBG_WAVE) == 0 && s) atomicAdd(lines_ctr, s);
    }
}

// fbg_pindex_seeds: the search of k_px_walk<true, *, true>, run to the end of every read.  One lane per read, reads
// taken in the order `order` (by length).  When a step finally fails, or the read ends, after pos > 0 symbols, those
// symbols are a seed: the state is the one the search of exactly those symbols ends in, so (l, r), the record of the
// first restart and the restart count are what fbg_pindex_occurrences keeps for that substring.  The search then starts
// again from [0, N] at the failing symbol, or at the next one when it failed at once (pos == 0).  k moves by at most one
// symbol per step, so the pattern word held is always the one of symbol k, wherever in a word a seed starts.
// !WRITE: num[id] = seeds of at least min_len symbols.  WRITE: seed j of read id goes to entry num[id] + j (num: the
// exclusive scan of the counts) of cnt / len64 (u64, as k_po_sizes reads count and pos), rec (3 x uint2), qs and ln.
template <bool COMPACT, bool WRITE>
__global__ __launch_bounds__(PX_THREADS) void k_px_seeds(PxDev d, const uint16_t *code_g, const uint32_t *C_g, const uint8_t *pats,
                                                        const uint64_t *poff, const uint32_t *order, uint64_t n, uint32_t min_len,
                                                        uint64_t *num, unsigned long long *cnt_out, unsigned long long *len64,
                                                        uint2 *rec, uint32_t *qs, uint32_t *ln)
{
    __shared__ uint16_t code[256];
    __shared__ uint32_t C[256];
    for (int c = threadIdx.x; c < 256; c += blockDim.x) { code[c] = code_g[c]; C[c] = C_g[c]; }
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint64_t id = order[t];
    const uint64_t a = poff[id];
    const uint32_t len = (uint32_t)(poff[id + 1] - a);       // < 2^32: checked by the host
    uint64_t at = WRITE ? num[id] : 0;                        // next entry (WRITE) or seeds counted so far
    uint32_t l = 0, r = d.N, pos = 0, nlines = 0;
    uint32_t restarts = 0, fsl = 1, fsr = 0, fk = 0;
    uint64_t word = 0;
    uint32_t k = 0;
    while (true) {
        bool ok = false;
        if (k < len) {
            const uint64_t q = a + k;
            if (k == 0 || (q & 7) == 0) word = *(const uint64_t *)(pats + (q & ~7ull));   // buffer padded to 8 bytes
            const uint32_t ch = (uint32_t)(word >> (8 * (q & 7))) & 0xffu;
            uint32_t nl, nr;
            ok = px_bs<COMPACT>(d, code, C, ch, l, r, nl, nr, nlines) != 0;
            if (!ok) {
                // restart: the branch of k_px_walk
                uint32_t sl, sr;
                if (px_bs<COMPACT>(d, code, C, '#', l, r, sl, sr, nlines)) {
                    uint32_t lo = 0, hi = d.nb;       // r1 = #B positions <= l
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) / 2;
                        if (d.bpos[mid] <= l) lo = mid + 1; else hi = mid;
                    }
                    const uint32_t r1 = lo;
                    if (r1 != 0 && r1 <= d.ne) {
                        const uint32_t bl = d.bpos[r1 - 1], br = d.epos[r1 - 1];
                        if (bl <= l && r <= br && px_bs<COMPACT>(d, code, C, ch, bl, br, nl, nr, nlines)) {
                            if (!restarts) { fsl = sl; fsr = sr; fk = pos; }
                            restarts++;
                            ok = true;
                        }
                    }
                }
            }
            if (ok) { l = nl; r = nr; pos++; k++; continue; }
        }
        // the search stopped at symbol k (k == len: the read ended)
        if (pos) {
            if (pos >= min_len) {
                if (WRITE) {
                    cnt_out[at] = (unsigned long long)r - l + 1;
                    len64[at] = pos;
                    rec[3 * at] = make_uint2(l, r);
                    rec[3 * at + 1] = make_uint2(fsl, fsr);
                    rec[3 * at + 2] = make_uint2(fk, restarts);
                    qs[at] = k - pos;
                    ln[at] = pos;
                }
                at++;
            }
            l = 0; r = d.N; pos = 0; restarts = 0; fsl = 1; fsr = 0; fk = 0;
        } else {
            if (k < len) k++;                                 // symbol k starts no match: skipped
        }
        if (k >= len) break;
    }
    if (!WRITE) num[id] = at;
}

__global__ void k_px_lenkey(const uint64_t *poff, uint64_t n, uint32_t *key, uint32_t *id)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint64_t len = poff[t + 1] - poff[t];
    key[t] = len > 0xffffffffull ? 0xffffffffu : (uint32_t)len;
    id[t] = (uint32_t)t;
}

__global__ void k_px_rebase(uint64_t *off, uint64_t n, uint64_t base)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n) off[t] -= base;
}

// fbg_pindex_seeds_strands: the reverse virtual reads.  pats[0 .. total) and poff[0 .. n] (rebased: poff[0] = 0,
// poff[n] = total) are the given reads; the kernel writes pats[total + j] = comp[pats[poff[R] + poff[R + 1] - 1 - j]]
// for every j in [poff[R], poff[R + 1]) and poff[n + R] = total + poff[R] for R = 1 .. n (R = 0 is poff[n] itself and
// already holds total).  One lane per aligned 8-byte word of the destination: it finds the read of its first byte by
// a search of poff, walks on through poff where reads end inside the word (empty reads are stepped over) and stores
// the word whole; the two words that the range [total, 2 * total) covers only in part are stored byte by byte, so the
// forward bytes that share the first one are left alone.  The table sits in LDS.  The first n lanes of the grid also
// write the offsets.  n > 0.
__global__ __launch_bounds__(PX_THREADS) void k_px_revcomp(const uint8_t *comp_g, uint8_t *pats, uint64_t *poff, uint64_t n,
                                                          uint64_t total)
{
    __shared__ uint8_t comp[256];
    for (int c = threadIdx.x; c < 256; c += blockDim.x) comp[c] = comp_g[c];
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t b0 = (total / 8 + t) * 8;                  // the word's first byte in pats
    const uint64_t lo = b0 > total ? b0 : total, hi = b0 + 8 < 2 * total ? b0 + 8 : 2 * total;
    if (lo < hi) {
        uint64_t j = lo - total;
        uint64_t R = 0, top = n;                              // poff[R] <= j < poff[top]
        while (top - R > 1) {
            const uint64_t mid = R + (top - R) / 2;
            if (poff[mid] <= j) R = mid; else top = mid;
        }
        uint64_t a = poff[R], e = poff[R + 1];
        uint64_t word = 0;
        for (uint64_t b = lo; b < hi; b++, j++) {
            while (j >= e) { R++; a = e; e = poff[R + 1]; }   // j < total = poff[n]: R stays below n
            word |= (uint64_t)comp[pats[a + (e - 1 - j)]] << (8 * (b - b0));
        }
        if (hi - lo == 8) {
            *(uint64_t *)(pats + b0) = word;
        } else {
            for (uint64_t b = lo; b < hi; b++) pats[b] = (uint8_t)(word >> (8 * (b - b0)));
        }
    }
    if (t < n) poff[n + 1 + t] = total + poff[1 + t];
}

// ---- occurrences (fbg_pindex_occurrences / _fetch) ---------------------------------------------------------------
// Per pattern: the totals, the capped sizes of both lists (entry n = 0, so that their exclusive scans are the n + 1
// CSR offsets) and what the expansion reads: the first slot of either list, and for the starts k (restarts > 0) or
// |P| (= pos of a found pattern).  A graph without edges has no places: sizes 0, the totals stand.
__global__ void k_po_sizes(const unsigned long long *count, const unsigned long long *pos, const uint2 *rec, uint64_t n, uint64_t cap,
                           int has_edges, uint64_t *etot, uint64_t *stot, uint64_t *esz, uint64_t *ssz, uint32_t *restarts,
                           uint32_t *el, uint32_t *ss, uint32_t *sk)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n) return;
    if (t == n) { esz[n] = 0; ssz[n] = 0; return; }
    const uint64_t cnt = count[t];
    const uint2 lr = rec[3 * t], s = rec[3 * t + 1], kr = rec[3 * t + 2];
    const uint64_t st = cnt == 0 ? 0 : kr.y ? (uint64_t)s.y - s.x + 1 : cnt;
    etot[t] = cnt;
    stot[t] = st;
    esz[t] = has_edges ? (cnt < cap ? cnt : cap) : 0;
    ssz[t] = has_edges ? (st < cap ? st : cap) : 0;
    restarts[t] = kr.y;
    el[t] = lr.x;
    ss[t] = kr.y ? s.x : lr.x;
    sk[t] = kr.y ? kr.x : (uint32_t)pos[t];
}

// One lane per reported place, item i of a list's CSR order (off[n] = total items): the wave finds the patterns of
// its first and last item by a search of all n offsets that is the same in every lane, each lane then searches only
// between those two.  Item j of pattern q is SA slot first[q] + j; the place follows as in pv_allowed.  Lanes write
// consecutive entries: a pattern's places are contiguous and in slot order.  STARTS: offsets of the match's start.
template <bool STARTS>
__global__ __launch_bounds__(PX_THREADS) void k_po_expand(PvDev d, const uint64_t *off, uint64_t n, uint64_t total,
                                                         const uint32_t *first, const uint32_t *sk, const uint32_t *restarts,
                                                         uint32_t *osrc, uint32_t *odst, uint32_t *oofs)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t w0 = po_uniform(i & ~(uint64_t)(FBG_WAVE - 1));
    if (w0 >= total) return;
    const uint64_t w1 = w0 + FBG_WAVE - 1 < total ? w0 + FBG_WAVE - 1 : total - 1;
    const uint64_t q0 = po_uniform(po_find(off, 0, n - 1, w0));
    const uint64_t q1 = po_uniform(po_find(off, q0, n - 1, w1));
    if (i >= total) return;
    const uint64_t q = po_find(off, q0, q1, i);
    const uint32_t p = d.sa[first[q] + (uint32_t)(i - off[q])];
    const uint32_t e = pv_edge(d, p);
    const uint32_t base = d.estart[e] + 1, ne = d.estart[e + 1] - base;
    uint32_t o = ne - 1 - (p - base);                 // of the pattern's last symbol (starts after a restart: p = base - 1)
    if (STARTS) o = restarts[q] ? ne - sk[q] : o - sk[q] + 1;
    osrc[i] = d.esrc[e];
    odst[i] = d.edst[e];
    oofs[i] = o;
}

// k_po_expand for the MSA coordinate of every place: the same lane per place, the same search of the offsets and the
// same SA slot -> edge -> offset; then the node and offset of Occurrences.as_nodes (the source below |label(src)|, else
// the destination), and through the table the row and column of that cell of the node's representative row.  An offset
// outside S_e (a pattern with '#' or a zero byte) gets PM_NONE in both.  Lanes write consecutive entries of orow / ocol.
template <bool STARTS>
__global__ __launch_bounds__(PX_THREADS) void k_po_expand_msa(PvDev d, PmDev m, const uint64_t *off, uint64_t n, uint64_t total,
                                                             const uint32_t *first, const uint32_t *sk, const uint32_t *restarts,
                                                             uint32_t *orow, uint32_t *ocol)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t w0 = po_uniform(i & ~(uint64_t)(FBG_WAVE - 1));
    if (w0 >= total) return;
    const uint64_t w1 = w0 + FBG_WAVE - 1 < total ? w0 + FBG_WAVE - 1 : total - 1;
    const uint64_t q0 = po_uniform(po_find(off, 0, n - 1, w0));
    const uint64_t q1 = po_uniform(po_find(off, q0, n - 1, w1));
    if (i >= total) return;
    const uint64_t q = po_find(off, q0, q1, i);
    const uint32_t p = d.sa[first[q] + (uint32_t)(i - off[q])];
    const uint32_t e = pv_edge(d, p);
    const uint32_t base = d.estart[e] + 1, ne = d.estart[e + 1] - base;
    uint32_t o = ne - 1 - (p - base);
    if (STARTS) o = restarts[q] ? ne - sk[q] : o - sk[q] + 1;
    uint32_t u = d.esrc[e];
    const uint32_t la = d.len[u];
    if (o >= la) { u = d.edst[e]; o -= la; }
    uint32_t row = PM_NONE, col = PM_NONE;
    if (o < d.len[u]) {
        const uint4 nd = m.node[u];
        col = pm_col(m, nd, o);
        row = col == PM_NONE ? PM_NONE : nd.x;
    }
    orow[i] = row;
    ocol[i] = col;
}

// f<COMPACT, B>(...) by the index's occ layout and a second switch of the call
#define PX_BY_COMPACT2(f, compact, b, ...) \
    ((compact) ? ((b) ? f<true, true>(__VA_ARGS__) : f<true, false>(__VA_ARGS__)) : ((b) ? f<false, true>(__VA_ARGS__) : f<false, false>(__VA_ARGS__)))

// ---- launchers for the build (pindex_build.hip) ------------------------------------------------------------------------
void px_walk_labels(fbg_pindex *ix, const uint8_t *labels, const uint64_t *loff, uint64_t n_nodes, uint8_t *bflag, uint8_t *eflag)
{
    const auto walk = ix->compact ? k_px_walk<false, true> : k_px_walk<false, false>;
    hipLaunchKernelGGL(walk, dim3(fbg_blocks(n_nodes, PX_THREADS)), dim3(PX_THREADS), 0, ix->ctx->stream, px_dev(ix),
                       ix->code.as<uint16_t>(), ix->C.as<uint32_t>(), labels, loff, (const uint32_t *)nullptr, n_nodes,
                       (unsigned long long *)nullptr, (unsigned long long *)nullptr, bflag, eflag, (unsigned long long *)nullptr,
                       ix->vrng.as<uint2>());
}

void px_rebase(hipStream_t st, uint64_t *off, uint64_t n, uint64_t base)
{
    hipLaunchKernelGGL(k_px_rebase, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, off, n, base);
}

// ---- the front of a search -------------------------------------------------------------------------------------------
enum PxMode { PX_LOCATE, PX_OCC, PX_SEEDS };

// The per-pattern (or per-seed) buffers of a place state, for n of them.
static int po_reserve(fbg_pindex *ix, PoState &s, uint64_t n)
{
    for (DevBuf *b : {&s.etot, &s.stot}) FBG_TRY(px_reserve(ix, *b, n * 8));
    for (DevBuf *b : {&s.esz, &s.ssz, &s.eoff, &s.soff}) FBG_TRY(px_reserve(ix, *b, (n + 1) * 8));
    for (DevBuf *b : {&s.rs, &s.el, &s.ss, &s.sk}) FBG_TRY(px_reserve(ix, *b, n * 4));
    return FBG_OK;
}

// The front of fbg_pindex_locate, fbg_pindex_occurrences and fbg_pindex_seeds: checks, every allocation of the call
// that depends on n only (after hipSetDevice), patterns onto the device, ev0, and the pattern ids sorted by length into
// oval2.  n > 0.  The patterns go to the buffers of the mode: the reads of a seeds call to the read batch, which the later
// stages read, the patterns of the other two to pats / poff; so neither search disturbs the other's.  comp (PX_SEEDS only;
// NULL: the reads as given): the complement table of fbg_pindex_seeds_strands.  Everything is then reserved for 2n reads
// and twice the bytes, k_px_revcomp appends the reverse virtual reads after ev0, and the sort runs over the 2n.
static int px_front(fbg_pindex *ix, const char *who, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns, PxMode mode,
                    const uint8_t *comp = nullptr)
{
    fbg_ctx *ctx = ix->ctx;
    DevBuf &pats = mode == PX_SEEDS ? ix->batch.reads : ix->pats, &offs = mode == PX_SEEDS ? ix->batch.roff : ix->poff;
    for (uint64_t k = 0; k < n_patterns; k++)
        if (pat_off[k + 1] < pat_off[k]) return fbg_fail(ctx, FBG_ERR_INVALID, "pattern offsets decrease at pattern %llu", (unsigned long long)k);
    if (mode == PX_SEEDS)
        for (uint64_t k = 0; k < n_patterns; k++)
            if (pat_off[k + 1] - pat_off[k] >= (1ull << 32))
                return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: pattern %llu has 2^32 symbols or more", who, (unsigned long long)k);
    const uint64_t base = pat_off[0], total = pat_off[n_patterns] - base;
    if (total && !patterns) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: missing patterns", who);
    if (comp && total > (0xffffffffffffffffull - 64) / 2)
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: the patterns and their reverse complements hold 2^64 bytes or more", who);
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n = comp ? 2 * n_patterns : n_patterns;     // reads on the device
    const uint64_t pbytes = comp ? 2 * total : total;
    if (mode == PX_SEEDS) ix->batch.bytes = pbytes;
    FBG_TRY(px_reserve(ix, pats, ((pbytes + 7) & ~7ull) + 16));     // the kernels read whole words past the last pattern
    FBG_TRY(px_reserve(ix, offs, (n + 1) * 8));
    for (DevBuf *b : {&ix->okey, &ix->oval, &ix->okey2, &ix->oval2}) FBG_TRY(px_reserve(ix, *b, n * 4));
    if (mode == PX_SEEDS) {
        for (DevBuf *b : {&ix->snum, &ix->soff}) FBG_TRY(px_reserve(ix, *b, (n + 1) * 8));
    } else {
        for (DevBuf *b : {&ix->cnt_out, &ix->pos_out}) FBG_TRY(px_reserve(ix, *b, n * 8));
        FBG_TRY(px_reserve(ix, ix->lines_ctr, 8));
    }
    if (mode == PX_OCC) {
        FBG_TRY(px_reserve(ix, ix->orec, n * 24));
        FBG_TRY(po_reserve(ix, ix->occ, n));
    }
    if (comp) FBG_TRY(px_reserve(ix, ix->batch.comp, 256));
    if (total) FBG_HIP_TRY(ctx, hipMemcpyAsync(pats.p, patterns + base, total, hipMemcpyHostToDevice, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(offs.p, pat_off, (n_patterns + 1) * 8, hipMemcpyHostToDevice, st));
    if (comp) FBG_HIP_TRY(ctx, hipMemcpyAsync(ix->batch.comp.p, comp, 256, hipMemcpyHostToDevice, st));
    if (mode != PX_SEEDS) FBG_HIP_TRY(ctx, hipMemsetAsync(ix->lines_ctr.p, 0, 8, st));
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    uint64_t *poff = offs.as<uint64_t>();
    if (base) px_rebase(st, poff, n_patterns, base);
    if (comp) {
        const uint64_t words = (2 * total + 7) / 8 - total / 8;
        hipLaunchKernelGGL(k_px_revcomp, dim3(fbg_blocks(std::max(words, n_patterns), PX_THREADS)), dim3(PX_THREADS), 0, st,
                           ix->batch.comp.as<uint8_t>(), pats.as<uint8_t>(), poff, n_patterns, total);
    }
    // lanes of a wave take patterns of similar length: pattern ids sorted by length
    uint32_t *ka = ix->okey.as<uint32_t>(), *va = ix->oval.as<uint32_t>(), *kb = ix->okey2.as<uint32_t>(), *vb = ix->oval2.as<uint32_t>();
    hipLaunchKernelGGL(k_px_lenkey, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, poff, n, ka, va);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, ka, kb, va, vb, (size_t)n, 0u, 32u, st);
    }));
    return FBG_OK;
}

// The walk of a search over the n patterns that px_front left on the device, in its order by length
template <bool COMPACT, bool OCC> static void px_walk_launch(fbg_pindex *ix, uint64_t n)
{
    hipLaunchKernelGGL((k_px_walk<true, COMPACT, OCC>), dim3(fbg_blocks(n, PX_THREADS)), dim3(PX_THREADS), 0, ix->ctx->stream, px_dev(ix),
                       ix->code.as<uint16_t>(), ix->C.as<uint32_t>(), ix->pats.as<uint8_t>(), ix->poff.as<uint64_t>(),
                       ix->oval2.as<uint32_t>(), n, ix->cnt_out.as<unsigned long long>(), ix->pos_out.as<unsigned long long>(),
                       (uint8_t *)nullptr, (uint8_t *)nullptr, ix->lines_ctr.as<unsigned long long>(),
                       OCC ? ix->orec.as<uint2>() : (uint2 *)nullptr);
}

// px_front and the walk (occ: the instantiation that records the ranges into orec).  n > 0.
static int px_search(fbg_pindex *ix, const char *who, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns, bool occ)
{
    fbg_ctx *ctx = ix->ctx;
    FBG_TRY(px_front(ix, who, patterns, pat_off, n_patterns, occ ? PX_OCC : PX_LOCATE));
    PX_BY_COMPACT2(px_walk_launch, ix->compact, occ, ix, n_patterns);
    FBG_HIP_TRY(ctx, hipGetLastError());
    return FBG_OK;
}

// k_po_sizes over n > 0 items (count, pos and rec on the device; s reserved for n) and the scans of the capped sizes
// into the CSR offsets s.eoff / s.soff.  Shared by the occurrence and the seed calls.
static int po_sizes(fbg_pindex *ix, PoState &s, const DevBuf &count, const DevBuf &pos, const DevBuf &rec, uint64_t n, uint64_t cap)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    uint64_t *esz = s.esz.as<uint64_t>(), *ssz = s.ssz.as<uint64_t>(), *eoff = s.eoff.as<uint64_t>(), *soff = s.soff.as<uint64_t>();
    hipLaunchKernelGGL(k_po_sizes, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, count.as<unsigned long long>(),
                       pos.as<unsigned long long>(), (const uint2 *)rec.as<uint2>(), n, cap, ix->n_edges != 0,
                       s.etot.as<uint64_t>(), s.stot.as<uint64_t>(), esz, ssz, s.rs.as<uint32_t>(), s.el.as<uint32_t>(),
                       s.ss.as<uint32_t>(), s.sk.as<uint32_t>());
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, esz, eoff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
    }));
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, ssz, soff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    return FBG_OK;
}

// k_po_expand_msa over one list of a place state (STARTS: its starts, else its ends; the list is not empty) into orow /
// ocol on the device, on the context's stream.
template <bool STARTS> static void po_expand_msa_launch(fbg_pindex *ix, const PoState &s, uint32_t *orow, uint32_t *ocol)
{
    const PvDev d = pv_dev(ix);
    const PmDev m = {ix->mnode.as<uint4>(), ix->mbits.as<uint64_t>()};
    const uint64_t total = STARTS ? s.stotal : s.etotal;
    hipLaunchKernelGGL(k_po_expand_msa<STARTS>, dim3(fbg_blocks(total, PX_THREADS)), dim3(PX_THREADS), 0, ix->ctx->stream, d, m,
                       (const uint64_t *)(STARTS ? s.soff : s.eoff).as<uint64_t>(), s.n, total,
                       (const uint32_t *)(STARTS ? s.ss : s.el).as<uint32_t>(), (const uint32_t *)s.sk.as<uint32_t>(),
                       (const uint32_t *)s.rs.as<uint32_t>(), orow, ocol);
}

void po_expand_msa(fbg_pindex *ix, const PoState &s, bool starts, uint32_t *orow, uint32_t *ocol)
{
    if (starts) po_expand_msa_launch<true>(ix, s, orow, ocol);
    else po_expand_msa_launch<false>(ix, s, orow, ocol);
}

// The places of a place state (that of stage: PS_OCC or PS_SEEDS) into the caller's arrays: source, destination and
// offset of every place (end / start: three arrays each; fbg_pindex_occurrences_fetch, fbg_pindex_seeds_places) or, msa,
// its MSA row and column (two arrays each; fbg_pindex_occurrences_msa, fbg_pindex_seeds_msa) through k_po_expand_msa and
// a buffer of its own, so that neither s.place nor a later fetch sees it.
static int po_fetch(fbg_pindex *ix, const char *who, PsStage stage, PoState &s, bool msa, uint32_t *const (&end)[3],
                    uint32_t *const (&start)[3], double *device_ms)
{
    fbg_ctx *ctx = ix->ctx;
    const int K = msa ? 2 : 3;
    if (device_ms) *device_ms = 0;
    if (msa && (!ix->from_segmentation || !ix->has_map))
        return fbg_fail(ctx, FBG_ERR_INVALID, "%s: only an index built by fbg_pindex_build_segmentation knows MSA coordinates", who);
    FBG_TRY(px_need(ix, who, stage));
    const int e_given = std::count_if(end, end + K, [](uint32_t *q) { return q != nullptr; });
    const int s_given = std::count_if(start, start + K, [](uint32_t *q) { return q != nullptr; });
    if ((e_given && e_given != K) || (s_given && s_given != K))
        return fbg_fail(ctx, FBG_ERR_INVALID, msa ? "%s: a list takes both of its arrays or none" : "%s: a list takes all three of its arrays or none", who);
    const uint64_t ne = e_given ? s.etotal : 0, ns = s_given ? s.stotal : 0, n = s.n;
    if (ne + ns == 0) return FBG_OK;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf &buf = msa ? s.msa : s.place;
    FBG_TRY(px_reserve(ix, buf, K * (ne + ns) * 4));
    // the K arrays of the ends, then those of the starts
    uint32_t *pe = buf.as<uint32_t>(), *ps = pe + K * ne;
    const PvDev d = pv_dev(ix);
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    if (msa) {
        if (ne) po_expand_msa(ix, s, false, pe, pe + ne);
        if (ns) po_expand_msa(ix, s, true, ps, ps + ns);
    } else {
        if (ne)
            hipLaunchKernelGGL(k_po_expand<false>, dim3(fbg_blocks(ne, PX_THREADS)), dim3(PX_THREADS), 0, st, d, (const uint64_t *)s.eoff.as<uint64_t>(),
                               n, ne, (const uint32_t *)s.el.as<uint32_t>(), (const uint32_t *)s.sk.as<uint32_t>(),
                               (const uint32_t *)s.rs.as<uint32_t>(), pe, pe + ne, pe + 2 * ne);
        if (ns)
            hipLaunchKernelGGL(k_po_expand<true>, dim3(fbg_blocks(ns, PX_THREADS)), dim3(PX_THREADS), 0, st, d, (const uint64_t *)s.soff.as<uint64_t>(),
                               n, ns, (const uint32_t *)s.ss.as<uint32_t>(), (const uint32_t *)s.sk.as<uint32_t>(),
                               (const uint32_t *)s.rs.as<uint32_t>(), ps, ps + ns, ps + 2 * ns);
    }
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_TRY(px_record_end(ix));
    for (int k = 0; k < K && ne; k++) FBG_HIP_TRY(ctx, hipMemcpyAsync(end[k], pe + k * ne, ne * 4, hipMemcpyDeviceToHost, st));
    for (int k = 0; k < K && ns; k++) FBG_HIP_TRY(ctx, hipMemcpyAsync(start[k], ps + k * ns, ns * 4, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    return FBG_OK;
}

// ---- seeds (fbg_pindex_seeds / _fetch / _places) -------------------------------------------------------------------
// Count, then write: k_px_seeds<*, false> counts the reported seeds of every read, an exclusive scan places them (reads
// in input order, a read's seeds contiguous and by q_start), the host learns the total and sizes the per-seed buffers,
// k_px_seeds<*, true> walks again and writes.  From there the seeds are the patterns of po_sizes / po_fetch.
template <bool COMPACT, bool WRITE> static void px_seeds_launch(fbg_pindex *ix, const PxDev &d, uint64_t n, uint32_t min_len)
{
    hipLaunchKernelGGL((k_px_seeds<COMPACT, WRITE>), dim3(fbg_blocks(n, PX_THREADS)), dim3(PX_THREADS), 0, ix->ctx->stream, d,
                       ix->code.as<uint16_t>(), ix->C.as<uint32_t>(), ps_reads(ix), ps_roff(ix),
                       ix->oval2.as<uint32_t>(), n, min_len, (WRITE ? ix->soff : ix->snum).as<uint64_t>(),
                       ix->scnt.as<unsigned long long>(), ix->spos.as<unsigned long long>(), ix->srec.as<uint2>(),
                       ix->sq.as<uint32_t>(), ix->slen.as<uint32_t>());
}

// The body of fbg_pindex_seeds (comp == NULL) and fbg_pindex_seeds_strands (comp: the 256-byte table; the device then
// searches the 2 * n_patterns virtual reads and seed_off has that many entries and one).
static int px_seeds(fbg_pindex *ix, const char *who, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                    const uint8_t *comp, uint64_t min_length, uint64_t max_per_seed, uint64_t *seed_off, double *device_ms)
{
    fbg_ctx *ctx = ix->ctx;
    PoState &s = ix->sd;
    px_begin(ix, PS_SEEDS);       // the chains, and all that is made from them, belong to the seeds they were made from
    if (device_ms) *device_ms = 0;
    if (!seed_off || (n_patterns && !pat_off)) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: missing argument", who);
    if (min_length == 0) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: min_length is 1 or more", who);
    if (n_patterns >= 0xffffffffull) return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: at most 2^32 - 2 patterns per call", who);
    if (comp && 2 * n_patterns >= 0xffffffffull)
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: at most 2^31 - 1 patterns per call (both strands: 2^32 - 2 reads)", who);
    seed_off[0] = 0;
    s.n = 0;
    s.etotal = s.stotal = 0;
    const uint64_t n = comp ? 2 * n_patterns : n_patterns;
    ix->batch.n = n;
    ix->batch.stranded = comp != nullptr;
    if (n == 0) { px_finish(ix, PS_SEEDS); return FBG_OK; }
    FBG_TRY(px_front(ix, who, patterns, pat_off, n_patterns, PX_SEEDS, comp));
    hipStream_t st = ctx->stream;
    const bool none = min_length >= (1ull << 32);   // no pattern has 2^32 symbols: nothing can be reported
    const uint32_t L = none ? 0xffffffffu : (uint32_t)min_length;
    const PxDev d = px_dev(ix);
    uint64_t *num = ix->snum.as<uint64_t>(), *soff = ix->soff.as<uint64_t>();
    auto walk = [&](bool write) { PX_BY_COMPACT2(px_seeds_launch, ix->compact, write, ix, d, n, L); };
    if (none) {
        std::fill(seed_off, seed_off + n + 1, (uint64_t)0);
    } else {
        FBG_HIP_TRY(ctx, hipMemsetAsync(num + n, 0, 8, st));
        walk(false);
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::exclusive_scan(tmp, bytes, num, soff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
        }));
        FBG_HIP_TRY(ctx, hipGetLastError());
        FBG_HIP_TRY(ctx, hipMemcpyAsync(seed_off, soff, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    const uint64_t S = seed_off[n];
    if (S >= (1ull << 32))
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: %llu seeds to report; a call takes fewer than 2^32 (raise min_length or "
                        "split the batch)", who, (unsigned long long)S);
    uint64_t tot[2] = {0, 0};
    if (S) {
        FBG_TRY(px_reserve(ix, ix->srec, S * 24));
        for (DevBuf *b : {&ix->scnt, &ix->spos}) FBG_TRY(px_reserve(ix, *b, S * 8));
        for (DevBuf *b : {&ix->sq, &ix->slen}) FBG_TRY(px_reserve(ix, *b, S * 4));
        FBG_TRY(po_reserve(ix, s, S));
        walk(true);
        FBG_TRY(po_sizes(ix, s, ix->scnt, ix->spos, ix->srec, S, max_per_seed));
    }
    FBG_TRY(px_record_end(ix));
    if (S) {
        FBG_HIP_TRY(ctx, hipMemcpyAsync(&tot[0], s.eoff.as<uint64_t>() + S, 8, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(&tot[1], s.soff.as<uint64_t>() + S, 8, hipMemcpyDeviceToHost, st));
    }
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    if (tot[0] >= (1ull << 32) || tot[1] >= (1ull << 32))
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: %llu ends and %llu starts to report; a list takes fewer than 2^32 "
                        "entries (lower max_per_seed or split the batch)", who, (unsigned long long)tot[0], (unsigned long long)tot[1]);
    s.n = S;
    s.etotal = tot[0];
    s.stotal = tot[1];
    px_finish(ix, PS_SEEDS);
    return FBG_OK;
}

extern "C" int fbg_pindex_locate(fbg_pindex *ix, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                                 uint64_t *count, uint64_t *pos)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    if (n_patterns && (!pat_off || !count || !pos)) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_locate: missing argument");
    if (n_patterns >= 0xffffffffull) return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "fbg_pindex_locate: at most 2^32 - 2 patterns per call");
    ix->search_ms = 0;
    ix->occ_lines = 0;
    if (n_patterns == 0) return FBG_OK;
    FBG_TRY(px_search(ix, "fbg_pindex_locate", patterns, pat_off, n_patterns, false));
    hipStream_t st = ctx->stream;
    const uint64_t n = n_patterns;
    FBG_TRY(px_record_end(ix));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(count, ix->cnt_out.p, n * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(pos, ix->pos_out.p, n * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&ix->occ_lines, ix->lines_ctr.p, 8, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, &ix->search_ms));
    return FBG_OK;
}

extern "C" int fbg_pindex_occurrences(fbg_pindex *ix, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                                      uint64_t max_per_pattern, uint64_t *count, uint64_t *pos, uint32_t *restarts,
                                      uint64_t *end_off, uint64_t *start_off, uint64_t *end_total, uint64_t *start_total,
                                      double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PoState &s = ix->occ;
    px_begin(ix, PS_OCC);
    if (device_ms) *device_ms = 0;
    if (!end_off || !start_off || (n_patterns && (!pat_off || !count || !pos || !restarts || !end_total || !start_total)))
        return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_occurrences: missing argument");
    if (n_patterns >= 0xffffffffull) return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "fbg_pindex_occurrences: at most 2^32 - 2 patterns per call");
    end_off[0] = start_off[0] = 0;
    s.n = n_patterns;
    s.etotal = s.stotal = 0;
    if (n_patterns == 0) { px_finish(ix, PS_OCC); return FBG_OK; }
    const uint64_t n = n_patterns;
    FBG_TRY(px_search(ix, "fbg_pindex_occurrences", patterns, pat_off, n, true));
    hipStream_t st = ctx->stream;
    FBG_TRY(po_sizes(ix, s, ix->cnt_out, ix->pos_out, ix->orec, n, max_per_pattern));
    FBG_TRY(px_record_end(ix));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(count, ix->cnt_out.p, n * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(pos, ix->pos_out.p, n * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(restarts, s.rs.p, n * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(end_total, s.etot.p, n * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(start_total, s.stot.p, n * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(end_off, s.eoff.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(start_off, s.soff.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    if (end_off[n] >= (1ull << 32) || start_off[n] >= (1ull << 32))
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "fbg_pindex_occurrences: %llu ends and %llu starts to report; a list takes fewer than 2^32 "
                        "entries (lower max_per_pattern or split the batch)", (unsigned long long)end_off[n], (unsigned long long)start_off[n]);
    s.etotal = end_off[n];
    s.stotal = start_off[n];
    px_finish(ix, PS_OCC);
    return FBG_OK;
}

extern "C" int fbg_pindex_occurrences_fetch(fbg_pindex *ix, uint32_t *end_src, uint32_t *end_dst, uint32_t *end_offset,
                                            uint32_t *start_src, uint32_t *start_dst, uint32_t *start_offset, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    return po_fetch(ix, "fbg_pindex_occurrences_fetch", PS_OCC, ix->occ, false, {end_src, end_dst, end_offset},
                    {start_src, start_dst, start_offset}, device_ms);
}

extern "C" int fbg_pindex_occurrences_msa(fbg_pindex *ix, uint32_t *end_row, uint32_t *end_col, uint32_t *start_row,
                                          uint32_t *start_col, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    return po_fetch(ix, "fbg_pindex_occurrences_msa", PS_OCC, ix->occ, true, {end_row, end_col, nullptr},
                    {start_row, start_col, nullptr}, device_ms);
}

extern "C" int fbg_pindex_seeds(fbg_pindex *ix, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                                uint64_t min_length, uint64_t max_per_seed, uint64_t *seed_off, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    return px_seeds(ix, "fbg_pindex_seeds", patterns, pat_off, n_patterns, nullptr, min_length, max_per_seed, seed_off, device_ms);
}

extern "C" int fbg_pindex_seeds_strands(fbg_pindex *ix, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                                        const uint8_t *complement, uint64_t min_length, uint64_t max_per_seed, uint64_t *seed_off,
                                        double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    uint8_t table[256];
    if (!complement) {
        for (int c = 0; c < 256; c++) table[c] = (uint8_t)c;
        const char *pairs = "ATCGatcg";
        for (int k = 0; k < 8; k += 2) { table[(uint8_t)pairs[k]] = pairs[k + 1]; table[(uint8_t)pairs[k + 1]] = pairs[k]; }
        complement = table;
    }
    return px_seeds(ix, "fbg_pindex_seeds_strands", patterns, pat_off, n_patterns, complement, min_length, max_per_seed, seed_off,
                    device_ms);
}

extern "C" int fbg_pindex_seeds_fetch(fbg_pindex *ix, uint32_t *q_start, uint32_t *length, uint64_t *count, uint32_t *restarts,
                                      uint64_t *end_total, uint64_t *start_total, uint64_t *end_off, uint64_t *start_off,
                                      double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PoState &s = ix->sd;
    if (device_ms) *device_ms = 0;
    FBG_TRY(px_need(ix, "fbg_pindex_seeds_fetch", PS_SEEDS));
    const uint64_t S = s.n;
    if (S == 0) {
        if (end_off) end_off[0] = 0;
        if (start_off) start_off[0] = 0;
        return FBG_OK;
    }
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    auto get = [&](void *dst, const DevBuf &src, size_t bytes) {
        return dst ? hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    FBG_HIP_TRY(ctx, get(q_start, ix->sq, S * 4));
    FBG_HIP_TRY(ctx, get(length, ix->slen, S * 4));
    FBG_HIP_TRY(ctx, get(count, ix->scnt, S * 8));
    FBG_HIP_TRY(ctx, get(restarts, s.rs, S * 4));
    FBG_HIP_TRY(ctx, get(end_total, s.etot, S * 8));
    FBG_HIP_TRY(ctx, get(start_total, s.stot, S * 8));
    FBG_HIP_TRY(ctx, get(end_off, s.eoff, (S + 1) * 8));
    FBG_HIP_TRY(ctx, get(start_off, s.soff, (S + 1) * 8));
    FBG_TRY(px_record_end(ix));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    return FBG_OK;
}

extern "C" int fbg_pindex_seeds_places(fbg_pindex *ix, uint32_t *end_src, uint32_t *end_dst, uint32_t *end_offset,
                                       uint32_t *start_src, uint32_t *start_dst, uint32_t *start_offset, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    return po_fetch(ix, "fbg_pindex_seeds_places", PS_SEEDS, ix->sd, false, {end_src, end_dst, end_offset},
                    {start_src, start_dst, start_offset}, device_ms);
}

extern "C" int fbg_pindex_seeds_msa(fbg_pindex *ix, uint32_t *end_row, uint32_t *end_col, uint32_t *start_row, uint32_t *start_col,
                                    double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    return po_fetch(ix, "fbg_pindex_seeds_msa", PS_SEEDS, ix->sd, true, {end_row, end_col, nullptr}, {start_row, start_col, nullptr},
                    device_ms);
}
