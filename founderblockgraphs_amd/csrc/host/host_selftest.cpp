// host_selftest.cpp -- the host-side pieces of the program that need no GPU (FASTA input with the reference's row
// filters, xGFA writer, graph statistics) behind a command line, for the CPU tests (tests/test_host_io.py) and for
// sanitizer runs:
//     fbg_host_selftest FASTA GAP_LIMIT ELASTIC(0|1) PATHS(0|1) OUT.gfa [GRAPH=file] [BOUNDARY ...]
// GRAPH=file: the node / edge arrays as fbg_block_graph returns them (u64 nb, u64 m, u32 node_of[nb*m], u32 rep_row[nb*m],
// u64 first_node[nb+1], u64 edge_count[nb], u64 edges[nb*m]); the xGFA is then formatted from them (write_xgfa_graph),
// as the program does with the GPU's arrays, instead of from labels hashed on the host (write_xgfa).
// prints "m n" of the MSA as read, then (with boundaries given: inclusive block ends, the last one == n, fbg.cpp:2027-2039)
// writes the xGFA and prints "nodes total_label_length founders edges".
//     fbg_host_selftest tie-extent
// checks fbg_tie_extent (tie_extent.h, the size of a tie group as rank_tail.hip's k_tie_groups finds it) against the plain count
// it replaces: groups of 1 .. 70 and 8191 .. 8194 slots at the start of a sorted array, in its middle and ending exactly at
// `hi`, each also with `hi` cutting the group short; prints "tie_extent ok CASES" or the first case that differs.
//     fbg_host_selftest twin-hash KEYS.bin BITS
// counts the twins among the 64-bit keys of a file the way suffix_sort.hip's k_sample_twins does (twin_hash.h: a table of 2^BITS
// words and two counters, all filled with all-ones; one insertion per key) and prints "twin_hash TWINS PROBES", PROBES being
// the longest probe sequence of an insertion.
//     fbg_host_selftest twin-slots KEYS.bin BITS
// prints the first slot of every key, one per line.
//     fbg_host_selftest cand-tail
// checks cand_tail.h (the rank-order scan's tail by member: rank_tail.hip's k_cand_region, k_cand_runs) against brute force: the
// places of the members of tie groups of 2 .. 70 suffixes of a text of rows, with and without members that have fewer than K
// symbols left; heads and sizes of the tie groups of a sorted slot array seen through candidate regions that cut them; the two
// running minima of runs of 1 .. 200 members in one piece and in pieces of 64, 7 and 1.  Prints "cand_tail ok GROUPS HEADS RUNS"
// or the first case that differs.
//     fbg_host_selftest pindex-stages
// prints the table of pindex_stage.h as it acts: "stages NAME ...", then per stage X "begin X" and the stages still done when
// every stage was done and X begins, then per subset of done stages (bit i of MASK: stage i, marked by ps_finish) "need MASK"
// and per stage "-" where ps_missing finds it and its ancestors done, else the stage it names.
//     fbg_host_selftest keys
// checks keys.h against the plain definition of a key (the codes of a position up to the first separator, then zeros, most
// significant first): msd_build_keys, k_pack's two steps (rolling, then symbol by symbol when a separator was seen), the 2-bit
// gather and the one-symbol rule, over tiles with one separator at every offset in reach and beyond, with two and with none, in
// the compact coding and (rolling alone, codes up to 255) in the plain one, at the geometries where a path or a mask changes;
// fbg_key_lcp against a comparison symbol by symbol on pairs that part at every symbol.  Prints "keys ok GEOMETRIES TILES PAIRS"
// or the first case that differs.
//     fbg_host_selftest dp_plan
// reads lines "max_ext f0 n dp_literal dp_wave dp_safe_window dp_tile" from stdin and prints the ladder of sweeps dp_plan.h plans
// for each, one line of rungs per input line: B<Rt> a byte-matrix rung (T1: its k_dp_tile form), W<WS> a wide rung, V<R> the wave
// sweep, L the literal sweep, each followed by ":" and its dp_kind_of -- e.g. "B4:1 W1024:3 W2048:4 ... V16:2 L:0".
//     fbg_host_selftest locate-options
// checks fbg_locate's command line (locate_options.cpp) against what the tool has always answered: every numeric flag absent,
// bare, with a number and with what is no number, --pairs=MIN,MAX, both spellings of --graph, --help, an unknown argument, and
// every prerequisite rule with its message, two of them broken at once included.  Prints "locate_options ok CASES" or the first
// command line that is answered differently.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "fasta.hpp"
#include "xgfa.hpp"
#include "locate_options.hpp"
#include <algorithm>
#include <cstring>
#include "../tie_extent.h"
#include "../cand_tail.h"
#include "../twin_hash.h"
#include "../pindex_stage.h"
#include "../keys.h"
#include "../dp_plan.h"

static int tie_extent_selftest()
{
    const uint32_t cap = 8192;                          // rank_tail.hip: RS_BIG_MEMBERS
    std::vector<uint32_t> sizes;
    for (uint32_t s = 1; s <= 70; s++) sizes.push_back(s);
    for (uint32_t s = 8191; s <= 8194; s++) sizes.push_back(s);
    unsigned long long cases = 0;
    for (const uint32_t s : sizes)
        for (int where = 0; where < 3; where++) {       // the group at the array's start, in the middle, ending exactly at hi
            const uint64_t before = where == 0 ? 0 : 37, after = where == 2 ? 0 : 29;
            std::vector<uint64_t> keys;
            for (uint64_t i = 0; i < before; i++) keys.push_back(10 + i / 3);          // (small groups before and after)
            const uint64_t key = 1000;
            for (uint32_t i = 0; i < s; i++) keys.push_back(key);
            for (uint64_t i = 0; i < after; i++) keys.push_back(2000 + i / 2);
            const uint64_t k0 = before;
            uint64_t reads = 0;
            auto key_at = [&](uint64_t k) -> uint64_t {
                reads++;
                if (k >= keys.size()) { std::fprintf(stderr, "tie_extent: read of slot %llu beyond the array\n", (unsigned long long)k); std::exit(1); }
                return keys[k];
            };
            // hi: the array's end, and every place that cuts the group short by 0 .. 3 slots
            std::vector<uint64_t> his = {keys.size()};
            for (uint64_t cut = 0; cut <= 3 && cut < s; cut++) his.push_back(k0 + s - cut);
            for (const uint64_t hi : his) {
                uint32_t want = 1;
                while (k0 + want < hi && want <= cap && keys[k0 + want] == key) want++;
                reads = 0;
                const uint32_t got = fbg_tie_extent(k0, hi, cap, key, key_at);
                // FBG_TIE_PROBE slots one by one, then two reads per doubling: far below one read per member
                const uint64_t most = FBG_TIE_PROBE + 2 * 14;
                if (got != want || reads > most) {
                    std::printf("tie_extent differs: size %u position %d hi %llu: got %u, want %u, %llu reads\n", s, where,
                                (unsigned long long)hi, got, want, (unsigned long long)reads);
                    return 1;
                }
                cases++;
            }
        }
    std::printf("tie_extent ok %llu\n", cases);
    return 0;
}

static int cand_tail_selftest()
{
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto rnd = [&](uint32_t mod) -> uint32_t { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng >> 33) % mod; };
    unsigned long long n_groups = 0, n_heads = 0, n_runs = 0;
    // ---- tie groups: rows of n symbols over ACGT, '#' after each, 0 at the very end; K symbols make a key ------------------
    const uint32_t K = 8, n = 60, rows = 80;
    for (int shorts = 0; shorts < 2; shorts++)
        for (uint32_t g = 2; g <= 70; g++) {
            std::string T;
            std::vector<uint32_t> pos;
            const uint32_t col = rnd(n - K - 4);
            std::string stretch;
            for (uint32_t i = 0; i < K; i++) stretch += shorts ? 'A' : "ACGT"[rnd(4)];
            for (uint32_t r = 0; r < rows; r++) {
                std::string row;
                for (uint32_t i = 0; i < n; i++) row += "ACGT"[rnd(4)];
                if (shorts && r < K && r < g) {                                 // a member with r symbols left: the row ends in r times A
                    for (uint32_t i = 0; i < r; i++) row[n - 1 - i] = 'A';
                    if (r < n) row[n - 1 - r] = 'C';
                    pos.push_back((uint32_t)T.size() + n - r);
                } else if (pos.size() < g) {                                    // a member with the whole stretch, at its own column
                    const uint32_t c = shorts ? col + r % 4 : col;
                    row.replace(c, K, stretch);
                    pos.push_back((uint32_t)T.size() + c);
                }
                T += row + '#';
            }
            T.back() = '\0';
            T += std::string(64, '\0');
            if (pos.size() != g) { std::printf("cand_tail: group of %u not built\n", g); return 1; }
            const uint32_t row_len = n + 1;
            auto rem_at = [&](uint32_t i) { return n - pos[i] % row_len; };
            const uint32_t from = fbg_ct_from(g, K, rem_at);
            if (from != (shorts ? 0u : K)) { std::printf("cand_tail: from %u, group of %u, shorts %d\n", from, g, shorts); return 1; }
            auto less_from = [&](uint32_t x, uint32_t y, uint32_t f) { return x != y && std::strcmp(T.c_str() + pos[x] + f, T.c_str() + pos[y] + f) < 0; };
            std::vector<uint32_t> order(g);
            for (uint32_t i = 0; i < g; i++) order[i] = i;
            std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return less_from(x, y, 0); });   // brute force: whole suffixes
            std::vector<bool> taken(g, false);
            for (uint32_t me = 0; me < g; me++) {
                const uint32_t rank = fbg_ct_rank(me, g, [&](uint32_t j, uint32_t i) { return less_from(j, i, from); });
                if (rank >= g || order[rank] != me || taken[rank]) { std::printf("cand_tail: rank %u of member %u, group of %u, shorts %d\n", rank, me, g, shorts); return 1; }
                taken[rank] = true;
            }
            if (g <= 4) {
                uint32_t rank[4];
                fbg_ct_small_ranks<4>(g, [&](int x, int y) { return less_from((uint32_t)x, (uint32_t)y, from); }, rank);
                for (uint32_t me = 0; me < g; me++)
                    if (rank[me] >= g || order[rank[me]] != me) { std::printf("cand_tail: small rank %u of member %u, group of %u\n", rank[me], me, g); return 1; }
            }
            n_groups++;
        }
    // ---- heads and sizes through candidate regions ---------------------------------------------------------------------------
    {
        std::vector<uint64_t> keys;
        std::vector<uint32_t> cand;
        uint64_t key = 5;
        for (uint32_t g = 1; g <= 70; g++)
            for (uint32_t rep = 0; rep < 2; rep++) {
                key += 1 + rnd(3);
                const uint32_t s = rep ? 1 + rnd(3) : g;
                for (uint32_t i = 0; i < s; i++) {
                    if (s > 1 || rnd(2)) cand.push_back((uint32_t)keys.size());     // every member of a group; some of the others
                    keys.push_back(key);
                }
            }
        const uint64_t N = keys.size();
        for (const uint32_t region : {7u, 64u, 100u, 4096u})
            for (size_t r0 = 0; r0 < cand.size(); r0 += region) {
                const uint32_t c = (uint32_t)std::min<size_t>(region, cand.size() - r0);
                std::vector<uint64_t> local(c);
                for (uint32_t i = 0; i < c; i++) local[i] = keys[cand[r0 + i]];
                for (uint32_t i = 0; i < c; i++) {
                    const uint64_t k0 = cand[r0 + i];
                    const bool want_head = !(k0 > 0 && keys[k0 - 1] == keys[k0]) && k0 + 1 < N && keys[k0 + 1] == keys[k0];
                    if (fbg_ct_heads_group(k0, 0, N, [&](uint64_t k) { return keys[k]; }) != want_head) { std::printf("cand_tail: head test at slot %llu\n", (unsigned long long)k0); return 1; }
                    if (!want_head) continue;
                    uint32_t want = 1;
                    while (k0 + want < N && keys[k0 + want] == keys[k0]) want++;
                    uint64_t local_reads = 0;
                    auto key_at = [&](uint64_t k) {
                        return fbg_ct_key_from(i, c, k0, k, [&](uint32_t j) { return (uint64_t)cand[r0 + j]; }, [&](uint32_t j) { local_reads++; return local[j]; },
                                               [&](uint64_t q) { return keys[q]; });
                    };
                    const uint32_t got = fbg_tie_extent(k0, N, 8192, keys[k0], key_at);
                    // (a group that lies in the region whole is measured on the region's copy: its second member at the least)
                    if (got != want || (i + want <= c && local_reads == 0)) { std::printf("cand_tail: size %u of the group at slot %llu, want %u, region %u, %llu local reads\n", got, (unsigned long long)k0, want, region, (unsigned long long)local_reads); return 1; }
                    n_heads++;
                }
            }
    }
    // ---- running minima of runs, in pieces --------------------------------------------------------------------------------------
    for (uint32_t len = 1; len <= 200; len++) {
        std::vector<uint32_t> lp(len + 1);
        for (auto &v : lp) v = rnd(len % 3 ? 50 : 5);
        std::vector<uint32_t> want(len);
        for (uint32_t i = 0; i < len; i++) {
            uint32_t a = FBG_CT_NONE, b = FBG_CT_NONE;
            for (uint32_t j = 0; j <= i; j++) a = std::min(a, lp[j]);
            for (uint32_t j = i + 1; j <= len; j++) b = std::min(b, lp[j]);
            want[i] = std::max(a, b) + 1;
        }
        for (const uint32_t piece : {len, 64u, 7u, 1u}) {
            std::vector<uint32_t> pm(len, 12345), got(len, 0);
            uint32_t carry = FBG_CT_NONE;
            for (uint32_t i0 = 0; i0 < len; i0 += piece)
                carry = fbg_ct_min_forward(i0, std::min(len, i0 + piece), carry, [&](uint32_t i) { return lp[i]; }, [&](uint32_t i, uint32_t v) { pm[i] = v; });
            carry = FBG_CT_NONE;
            for (uint32_t i0 = (len - 1) / piece * piece;; i0 -= piece) {
                carry = fbg_ct_min_backward(i0, std::min(len, i0 + piece), carry, [&](uint32_t i) { return lp[i + 1]; }, [&](uint32_t i) { return pm[i]; },
                                            [&](uint32_t i, uint32_t g) { got[i] = g; });
                if (i0 == 0) break;
            }
            if (got != want) { std::printf("cand_tail: run of %u in pieces of %u differs\n", len, piece); return 1; }
            n_runs++;
        }
    }
    std::printf("cand_tail ok %llu %llu %llu\n", n_groups, n_heads, n_runs);
    return 0;
}

// the definition: the codes of position p up to the first separator, then zeros
static uint64_t naive_key(const uint8_t *codes, int p, int b, int K, bool compact)
{
    uint64_t key = 0;
    int k = 0;
    for (; k < K && !(compact && codes[p + k] >= 0x80); k++) key = (key << b) | codes[p + k];
    for (; k < K; k++) key <<= b;
    return key;
}

static int keys_selftest()
{
    struct Geom { int b, K; bool compact; };
    std::vector<Geom> geoms;
    const int bk[][2] = {{1, 64}, {2, 1}, {2, 16}, {2, 25}, {2, 26}, {3, 1}, {3, 21}, {5, 1}, {5, 12}, {7, 1}, {7, 9}, {8, 1}, {8, 8}};
    for (const auto &g : bk) {
        if (g[0] < 8) geoms.push_back({g[0], g[1], true});      // the compact coding keeps bit 7 for the separator flag
        geoms.push_back({g[0], g[1], false});
    }
    const int t0 = 8, items = FBG_KEY_ITEMS;
    uint64_t store[16];                                         // 128 codes, aligned for the gather's 8-byte reads
    uint8_t *tile = reinterpret_cast<uint8_t *>(store);
    uint64_t seed = 0x9e3779b97f4a7c15ull;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
    unsigned long long n_tiles = 0, n_pairs = 0;
    for (const Geom &g : geoms) {
        const int b = g.b, K = g.K, reach = K + items - 1;
        const int far = reach > 40 ? reach : 40;                // (the gather reads 32 codes, more than it needs for a short key)
        // sep = t0 + o: one separator there; o == far + 1: none; o == far + 2: one as the first symbol and one three further on
        for (int o = 0; o <= far + 2; o++) {
            if (!g.compact && o <= far) continue;               // no separators in the plain coding: two tiles of plain codes
            for (int k = 0; k < 128; k++) tile[k] = (uint8_t)(next() & ((1u << b) - 1));
            if (g.compact && o <= far) tile[t0 + o] = FBG_SEP;
            if (g.compact && o == far + 2) tile[t0] = tile[t0 + 3] = FBG_SEP;
            uint64_t want[FBG_KEY_ITEMS], w[FBG_KEY_ITEMS];
            for (int i = 0; i < items; i++) want[i] = naive_key(tile, t0 + i, b, K, g.compact);
            auto differs = [&](const char *what) {
                for (int i = 0; i < items; i++)
                    if (w[i] != want[i]) {
                        std::printf("keys: %s differs: b %d K %d compact %d tile %d position %d: %llx, not %llx\n", what, b, K, (int)g.compact, o, i,
                                    (unsigned long long)w[i], (unsigned long long)want[i]);
                        return true;
                    }
                return false;
            };
            // k_pack: rolling, and in the compact coding symbol by symbol when a separator was seen
            std::memset(w, 0xee, sizeof w);
            const uint32_t seen = fbg_keys_rolling(tile, t0, b, K, w);
            if (g.compact && (seen & FBG_SEP)) fbg_keys_by_symbol(tile, t0, b, K, w);
            if (differs("k_pack's two steps")) return 1;
            if (g.compact) {
                std::memset(w, 0xee, sizeof w);
                msd_build_keys(tile, t0, b, K, w);
                if (differs("msd_build_keys")) return 1;
                std::memset(w, 0xee, sizeof w);
                fbg_keys_by_symbol(tile, t0, b, K, w);
                if (differs("fbg_keys_by_symbol")) return 1;
            }
            if (g.compact && b == 2 && reach <= 32 && o >= 32 && o <= far + 1) {      // no separator among the 32 codes it reads
                std::memset(w, 0xee, sizeof w);
                if (fbg_keys_gather2(tile, t0, K, w)) { std::printf("keys: the gather saw a separator that is not there\n"); return 1; }
                if (differs("fbg_keys_gather2")) return 1;
            }
            // the one-symbol rule, as sample_key applies it
            for (int i = 0; i < items; i++) {
                bool dead = false;
                w[i] = 0;
                for (int k = 0; k < K; k++) w[i] = (w[i] << b) | fbg_key_symbol(tile[t0 + i + k], g.compact ? 1 : 0, dead);
            }
            if (differs("fbg_key_symbol")) return 1;
            n_tiles++;
        }
    }
    // LCP of two keys that part at symbol j
    for (int b = 1; b <= 8; b++)
        for (const int K : {1, 64 / b}) {
            const int key_bits = K * b;
            const uint64_t sym = (1ull << b) - 1;
            for (int j = 0; j < K; j++) {
                uint64_t a = 0, c = 0;
                for (int k = 0; k < K; k++) {
                    const uint64_t x = next() & sym, y = k < j ? x : k == j ? (x + 1 + next() % sym) & sym : next() & sym;
                    a = (a << b) | x;
                    c = (c << b) | y;
                }
                uint32_t want = 0;
                while (((a >> (b * (K - 1 - (int)want))) & sym) == ((c >> (b * (K - 1 - (int)want))) & sym)) want++;
                const uint32_t got = fbg_key_lcp(a, c, b, key_bits), back = fbg_key_lcp(c, a, b, key_bits);
                const uint32_t inv = fbg_key_lcp_inv(a, c, fbg_key_inv(b), key_bits);
                if ((int)want != j || got != want || back != want || inv != want) {
                    std::printf("keys: LCP differs: b %d K %d symbol %d: %u %u %u, not %u\n", b, K, j, got, back, inv, want);
                    return 1;
                }
                n_pairs++;
            }
        }
    std::printf("keys ok %llu %llu %llu\n", (unsigned long long)geoms.size(), n_tiles, n_pairs);
    return 0;
}

static int pindex_stages_selftest()
{
    std::printf("stages");
    for (int s = 0; s < PS_COUNT; s++) std::printf(" %s", ps_table[s].name);
    std::printf("\n");
    for (int x = 0; x < PS_COUNT; x++) {
        bool done[PS_COUNT] = {};
        for (int s = 0; s < PS_COUNT; s++) ps_finish(done, (PsStage)s);
        ps_begin(done, (PsStage)x);
        std::printf("begin %s", ps_table[x].name);
        for (int s = 0; s < PS_COUNT; s++)
            if (done[s]) std::printf(" %s", ps_table[s].name);
        std::printf("\n");
    }
    for (unsigned mask = 0; mask < 1u << PS_COUNT; mask++) {
        bool done[PS_COUNT] = {};
        for (int s = 0; s < PS_COUNT; s++)
            if (mask >> s & 1) ps_finish(done, (PsStage)s);
        std::printf("need %u", mask);
        for (int y = 0; y < PS_COUNT; y++) {
            const int miss = ps_missing(done, (PsStage)y);
            std::printf(" %s", miss == PS_COUNT ? "-" : ps_table[miss].name);
        }
        std::printf("\n");
    }
    return 0;
}

static int twin_hash_selftest(const char *path, int bits, bool slots_only)
{
    FILE *fh = std::fopen(path, "rb");
    if (!fh || bits < 1 || bits > 30) { std::fprintf(stderr, "twin-hash: cannot read %s, or BITS not in 1 .. 30\n", path); return 2; }
    std::vector<uint64_t> keys;
    uint64_t k;
    while (std::fread(&k, 8, 1, fh) == 1) keys.push_back(k);
    std::fclose(fh);
    if (slots_only) {
        for (const uint64_t key : keys) std::printf("%llu\n", (unsigned long long)fbg_twin_slot(key, bits));
        return 0;
    }
    std::vector<uint64_t> table((1ull << bits) + 2, FBG_TWIN_EMPTY);
    uint64_t *counters = table.data() + (1ull << bits);
    uint64_t longest = 0;
    for (const uint64_t key : keys) {
        if (key == FBG_TWIN_EMPTY) { counters[1]++; continue; }
        uint64_t probes = 0;
        counters[0] += fbg_twin_insert(key, bits, [&](uint64_t slot, uint64_t kk) -> uint64_t {
            if (slot >= (1ull << bits)) { std::fprintf(stderr, "twin-hash: slot %llu beyond the table\n", (unsigned long long)slot); std::exit(1); }
            probes++;
            const uint64_t seen = table[slot];
            if (seen == FBG_TWIN_EMPTY) table[slot] = kk;
            return seen;
        });
        if (probes > longest) longest = probes;
    }
    std::printf("twin_hash %llu %llu\n", (unsigned long long)fbg_twin_total(counters[0], counters[1]), (unsigned long long)longest);
    return 0;
}

static int dp_plan_selftest()
{
    unsigned long long max_ext, f0, n;
    int lit, wave, safe, tile;
    while (std::scanf("%llu %llu %llu %d %d %d %d", &max_ext, &f0, &n, &lit, &wave, &safe, &tile) == 7) {
        const DpPlan p = dp_plan(max_ext, f0, n, DpPlanOptions{lit != 0, wave != 0, safe != 0, tile != 0});
        for (int i = 0; i < p.count; i++) {
            const DpRung &r = p.rung[i];
            const char tag = r.family == DP_BYTES ? (r.tile ? 'T' : 'B') : r.family == DP_WIDE ? 'W' : r.family == DP_WAVE ? 'V' : 'L';
            if (r.family == DP_LITERAL) std::printf("%sL:%d", i ? " " : "", dp_kind_of(r));
            else std::printf("%s%c%u:%d", i ? " " : "", tag, r.size, dp_kind_of(r));
        }
        std::printf("\n");
    }
    return 0;
}

struct LocateParse { bool ok; LocateOptions o; std::string error; };

static LocateParse locate_parse(std::vector<std::string> args)
{
    args.insert(args.begin(), "fbg_locate");
    std::vector<char *> argv;
    for (std::string &a : args) argv.push_back(&a[0]);
    LocateParse p;
    p.ok = parse_locate_options((int)argv.size(), argv.data(), p.o, p.error);
    return p;
}

static int locate_options_selftest()
{
    typedef std::vector<std::string> Args;
    unsigned long long cases = 0;
    auto differs = [&](const Args &args, const char *what) {
        std::printf("locate_options: %s:", what);
        for (const std::string &a : args) std::printf(" %s", a.c_str());
        std::printf("\n");
        return 1;
    };
    // `args` after --graph=g must be refused with exactly `message`
    auto refused = [&](Args args, const std::string &message) {
        args.insert(args.begin(), "--graph=g");
        const LocateParse p = locate_parse(args);
        cases++;
        return !p.ok && p.error == message;
    };
    // ---- the numeric flags: absent, bare, =0, =7, and what is no number ---------------------------------------------------------
    const struct { const char *name, *noun; bool LocateOptions::*on; uint64_t LocateOptions::*n; uint64_t preset; bool zero; } numeric[] = {
        {"--occurrences", "a count", &LocateOptions::occurrences, &LocateOptions::max_places, 64, true},
        {"--seeds", "a positive count", &LocateOptions::seeds, &LocateOptions::min_seed, 1, false},
        {"--chain", "a band", &LocateOptions::chain, &LocateOptions::band, UINT64_MAX, true},
        {"--align", "a pad", &LocateOptions::align, &LocateOptions::pad, 16, true},
        {"--graph-align", "a pad", &LocateOptions::graph_align, &LocateOptions::graph_pad, 16, true},
        {"--mapq", "a margin", &LocateOptions::mapq, &LocateOptions::margin, 0, true},
        {"--pair-align", "a number of edits", &LocateOptions::pair_align, &LocateOptions::max_edits, 0xffffffffu, true},
    };
    // every prerequisite at once, so that a flag that parses is accepted
    const Args all = {"--graph=g", "--msa=m", "--seeds", "--occurrences", "--chain", "--strands", "--rows", "--pairs=2,3"};
    for (const auto &f : numeric) {
        const std::string name = f.name;
        auto with = [&](const std::string &arg) {
            Args args = all;
            args.erase(std::remove(args.begin(), args.end(), name), args.end());
            if (!arg.empty()) args.push_back(arg);
            cases++;
            return locate_parse(args);
        };
        LocateParse p = with("");
        if (p.o.*f.on || p.o.*f.n != f.preset) return differs({name}, "absent");
        p = with(name);
        if (!p.ok || !(p.o.*f.on) || p.o.*f.n != f.preset) return differs({name}, "bare");
        p = with(name + "=7");
        if (!p.ok || !(p.o.*f.on) || p.o.*f.n != 7) return differs({name + "=7"}, "a number");
        p = with(name + "=0");
        if (f.zero ? !(p.o.*f.on) || p.o.*f.n != 0 : p.ok) return differs({name + "=0"}, "zero");
        if (!f.zero && p.error != name + " takes " + f.noun + ", not '0'") return differs({name + "=0"}, "the message");
        for (const char *v : {"", "x", "-1", "123456789012345678901", "18446744073709551616", "+3", "3 ", "0x10"})
            if (!refused({name + "=" + v}, name + " takes " + f.noun + ", not '" + v + "'")) return differs({name + "=" + v}, "no number");
    }
    if (!refused({"--seeds=0"}, "--seeds takes a positive count, not '0'")) return differs({"--seeds=0"}, "zero");
    if (!refused({"--pair-align=4294967296"}, "--pair-align takes a number of edits, not '4294967296'")) return differs({"--pair-align=4294967296"}, "33 bits");
    {
        Args args = all;
        args.push_back("--pair-align=4294967295");
        const LocateParse p = locate_parse(args);
        cases++;
        if (!p.ok || !p.o.pair_align || p.o.max_edits != 0xffffffffu) return differs(args, "32 bits");
    }
    // ---- --pairs=MIN,MAX --------------------------------------------------------------------------------------------------------
    {
        const LocateParse p = locate_parse(all);
        cases++;
        if (!p.ok || !p.o.pairs || p.o.min_insert != 2 || p.o.max_insert != 3) return differs(all, "--pairs");
    }
    for (const char *v : {"3,2", "3", ",3", "2,", "", "x", "1,2,3", "-1,4", "1,123456789012345678901"})
        if (!refused({std::string("--pairs=") + v}, std::string("--pairs takes MIN,MAX with MIN <= MAX, not '") + v + "'"))
            return differs({std::string("--pairs=") + v}, "no pair");
    if (!refused({"--pairs"}, "unknown argument --pairs")) return differs({"--pairs"}, "bare");
    // ---- --graph in both spellings, --help, what is unknown ---------------------------------------------------------------------
    for (const Args &args : {Args{"--graph=efg.xgfa"}, Args{"--graph", "efg.xgfa"}}) {
        const LocateParse p = locate_parse(args);
        cases++;
        if (!p.ok || !p.o.have_graph || p.o.graph != "efg.xgfa" || p.o.help) return differs(args, "--graph");
    }
    for (const Args &args : {Args{"--help", "--bogus"}, Args{"-h"}}) {
        const LocateParse p = locate_parse(args);
        cases++;
        if (!p.ok || !p.o.help) return differs(args, "--help");
    }
    if (!refused({"--bogus"}, "unknown argument --bogus")) return differs({"--bogus"}, "unknown");
    if (!refused({"--graph"}, "unknown argument --graph")) return differs({"--graph"}, "no value");
    if (!refused({"--bogus", "--help"}, "unknown argument --bogus")) return differs({"--bogus", "--help"}, "the first fault");
    // ---- the prerequisite rules, each with its message; the last two lines break two rules and the earlier one answers ------------
    const Args chained = {"--msa=m", "--seeds", "--occurrences", "--chain"};
    auto plus = [](Args a, const Args &b) { a.insert(a.end(), b.begin(), b.end()); return a; };
    const struct { Args args; const char *message; } rules[] = {
        {{"--msa="}, "--msa takes a FASTA file"},
        {{"--chain"}, "--chain needs --seeds, --msa and --occurrences[=M] with M > 0"},
        {{"--msa=m", "--seeds", "--chain"}, "--chain needs --seeds, --msa and --occurrences[=M] with M > 0"},
        {{"--msa=m", "--seeds", "--occurrences=0", "--chain"}, "--chain needs --seeds, --msa and --occurrences[=M] with M > 0"},
        {{"--seeds", "--occurrences", "--chain"}, "--chain needs --seeds, --msa and --occurrences[=M] with M > 0"},
        {{"--strands"}, "--strands needs --seeds"},
        {{"--seeds", "--rows"}, "--rows needs --seeds and --msa"},
        {{"--msa=m", "--rows"}, "--rows needs --seeds and --msa"},
        {plus(chained, {"--by-row"}), "--by-row needs --chain and --rows"},
        {{"--msa=m", "--seeds", "--rows", "--by-row"}, "--by-row needs --chain and --rows"},
        {plus(chained, {"--rows", "--cigar"}), "--cigar needs --align"},
        {plus(chained, {"--align"}), "--align needs --chain and --rows"},
        {plus(chained, {"--graph-align=3"}), "--graph-align needs --chain and --rows"},
        {plus(chained, {"--rows", "--graph-cigar"}), "--graph-cigar needs --graph-align"},
        {plus(chained, {"--rows", "--graph-align", "--gaf=f"}), "--gaf needs --graph-cigar"},
        {{"--seeds", "--mapq"}, "--mapq needs --chain"},
        {plus(chained, {"--pairs=0,9"}), "--pairs needs --chain and --strands"},
        {{"--seeds", "--strands", "--pairs=0,9"}, "--pairs needs --chain and --strands"},
        {plus(chained, {"--strands", "--pairs=0,9", "--pair-align"}), "--pair-align needs --pairs and --rows"},
        {plus(chained, {"--rows", "--pair-align=2"}), "--pair-align needs --pairs and --rows"},
        {plus(chained, {"--rows", "--graph-align", "--graph-cigar", "--gaf="}), "--gaf takes a file"},
        {{"--seeds", "--complement=AT"}, "--complement needs --strands"},
        {{"--seeds", "--strands", "--complement=ATC"}, "--complement takes pairs of characters"},
        {{"--seeds", "--strands", "--complement="}, "--complement takes pairs of characters"},
        {{"--cigar", "--graph-cigar"}, "--cigar needs --align"},
        {{"--mapq", "--pair-align", "--strands"}, "--strands needs --seeds"},
    };
    for (const auto &r : rules)
        if (!refused(r.args, r.message)) return differs(r.args, r.message);
    for (const Args &args : {Args{}, Args{"--graph="}, Args{"--seeds", "--strands"}}) {
        const LocateParse p = locate_parse(args);
        cases++;
        if (p.ok || p.error != "--graph is required") return differs(args, "--graph is required");
    }
    std::printf("locate_options ok %llu\n", cases);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && std::string(argv[1]) == "locate-options") return locate_options_selftest();
    if (argc == 2 && std::string(argv[1]) == "dp_plan") return dp_plan_selftest();
    if (argc == 4 && (std::string(argv[1]) == "twin-hash" || std::string(argv[1]) == "twin-slots"))
        return twin_hash_selftest(argv[2], std::atoi(argv[3]), std::string(argv[1]) == "twin-slots");
    if (argc == 2 && std::string(argv[1]) == "tie-extent") return tie_extent_selftest();
    if (argc == 2 && std::string(argv[1]) == "cand-tail") return cand_tail_selftest();
    if (argc == 2 && std::string(argv[1]) == "pindex-stages") return pindex_stages_selftest();
    if (argc == 2 && std::string(argv[1]) == "keys") return keys_selftest();
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s FASTA GAP_LIMIT ELASTIC PATHS OUT.gfa [BOUNDARY ...]\n", argv[0]);
        return 2;
    }
    Msa msa;
    if (!read_msa(argv[1], std::atol(argv[2]), std::atoi(argv[3]) != 0, std::atoi(argv[4]) != 0, msa)) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 3;
    }
    std::printf("%llu %llu\n", (unsigned long long)msa.m, (unsigned long long)msa.n);
    if (argc == 6 || msa.m == 0) return 0;
    std::vector<uint64_t> boundaries;
    int first_boundary = 6;
    BlockGraph g;
    bool have_graph = false;
    if (std::string(argv[6]).rfind("GRAPH=", 0) == 0) {
        first_boundary = 7;
        have_graph = true;
        FILE *fh = std::fopen(argv[6] + 6, "rb");
        uint64_t hdr[2];
        if (!fh || std::fread(hdr, 8, 2, fh) != 2) { std::fprintf(stderr, "cannot read %s\n", argv[6] + 6); return 5; }
        const uint64_t nb = hdr[0], m = hdr[1];
        g.node_of.resize(nb * m); g.rep_row.resize(nb * m); g.first_node.resize(nb + 1); g.edge_count.resize(nb); g.edges.resize(nb * m);
        const bool ok = std::fread(g.node_of.data(), 4, nb * m, fh) == nb * m && std::fread(g.rep_row.data(), 4, nb * m, fh) == nb * m &&
                        std::fread(g.first_node.data(), 8, nb + 1, fh) == nb + 1 && std::fread(g.edge_count.data(), 8, nb, fh) == nb &&
                        std::fread(g.edges.data(), 8, nb * m, fh) == nb * m;
        std::fclose(fh);
        if (!ok || m != msa.m) { std::fprintf(stderr, "%s does not hold the arrays of this MSA\n", argv[6] + 6); return 5; }
    }
    for (int i = first_boundary; i < argc; i++) boundaries.push_back(std::strtoull(argv[i], nullptr, 10));
    std::string error;
    const bool paths = std::atoi(argv[4]) != 0;
    if (!(have_graph ? write_xgfa_graph(msa, boundaries, g, paths, argv[5], error) : write_xgfa(msa, boundaries, paths, argv[5], error))) {
        std::fprintf(stderr, "%s\n", error.c_str());
        return 4;
    }
    const GraphStats st = segment_stats(msa, boundaries);
    std::printf("%llu %llu %llu %llu\n", (unsigned long long)st.nodes, (unsigned long long)st.total_label_length,
                (unsigned long long)st.founders, (unsigned long long)st.edges);
    return 0;
}
