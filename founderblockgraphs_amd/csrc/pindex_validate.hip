// pindex_validate.hip -- the semi-repeat-free check of a pattern index (fbg_pindex_validate) and, on top of it, the
// validation and repair of a segmentation (fbg_segmentation_validate / _repair).
//
//   k_pv_node / k_pv_wave            the SA range of every label, kept from the B / E walk of the build, scanned against
//                                    the block of each occurrence's node, one lane per short range and one wave per long
//                                    one;
//   k_sv_cuts                        the cuts before blocks that hold an INVALID node.
#include "pindex_dev.h"

// The occurrence of a label (m symbols, node in block bu) whose reversed copy starts at text position p: the node and
// offset it starts at in label(a) + label(b) of its edge; true iff that is offset 0 of a node of block bu.
__device__ __forceinline__ bool pv_allowed(const PvDev &d, uint32_t p, uint32_t m, uint32_t bu, uint32_t &node, uint32_t &off)
{
    const uint32_t e = pv_edge(d, p);
    const uint32_t base = d.estart[e] + 1, ne = d.estart[e + 1] - base;   // ne = |a| + |b|
    const uint32_t a = d.esrc[e], la = d.len[a];
    const uint32_t s = ne - (p - base) - m;                                 // forward offset in label(a) + label(b)
    if (s < la) { node = a; off = s; } else { node = d.edst[e]; off = s - la; }
    return off == 0 && d.block[node] == bu;
}

__device__ __forceinline__ void pv_add_slots(unsigned long long *ctr, unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x % FBG_WAVE) == 0 && v) atomicAdd(ctr, v);
}

// One lane per node: rules 1-3, then a range of at most PV_SHORT slots scanned in slot order up to its first
// disallowed occurrence; longer ranges go to `list` for k_pv_wave (status VALID until that kernel finds otherwise).
// ctr[0]: list length, ctr[1]: SA slots scanned.
__global__ __launch_bounds__(PX_THREADS) void k_pv_node(PvDev d, uint64_t n, PvMask ig, int has_ig, uint8_t *status, uint32_t *wn,
                                                       uint32_t *wo, uint32_t *list, unsigned long long *ctr)
{
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long slots = 0;
    if (u < n) {
        uint8_t st = FBG_NODE_VALID;
        uint32_t wnode = PV_NONE, woff = PV_NONE;
        const uint32_t m = d.len[u];
        bool ignored = false;
        if ((d.flag[u] & (PV_IN | PV_OUT)) == (PV_IN | PV_OUT) && has_ig) {
            const uint8_t *lab = d.text + d.tpos[u];        // reverse(label(u)): the order does not matter here
            for (uint32_t k = 0; k < m && !ignored; k++) {
                const uint32_t c = lab[k];
                ignored = (ig.w[c >> 6] >> (c & 63)) & 1u;
            }
        }
        if ((d.flag[u] & (PV_IN | PV_OUT)) != (PV_IN | PV_OUT)) st = FBG_NODE_SKIP_SOURCE_SINK;
        else if (ignored) st = FBG_NODE_SKIP_IGNORED;
        else if (m == 0) st = FBG_NODE_SKIP_EMPTY;
        else {
            const uint2 lr = d.rng[u];
            const uint32_t bu = d.block[u];
            if (lr.x <= lr.y && lr.y - lr.x < PV_SHORT) {
                for (uint32_t i = lr.x; i <= lr.y; i++) {
                    slots++;
                    uint32_t node, off;
                    if (!pv_allowed(d, d.sa[i], m, bu, node, off)) {
                        st = FBG_NODE_INVALID; wnode = node; woff = off;
                        break;
                    }
                }
            } else if (lr.x <= lr.y) {
                list[atomicAdd(&ctr[0], 1ull)] = (uint32_t)u;
            }
        }
        status[u] = st;
        wn[u] = wnode;
        wo[u] = woff;
    }
    pv_add_slots(&ctr[1], slots);
}

// One wave per listed node (a grid-stride loop over ctr[0] entries): 64 slots per step in ascending slot order; the
// lowest lane whose occurrence is disallowed is the witness, and the node's scan ends with that step.
__global__ __launch_bounds__(PX_THREADS) void k_pv_wave(PvDev d, const uint32_t *list, unsigned long long *ctr, uint8_t *status,
                                                       uint32_t *wn, uint32_t *wo)
{
    const uint64_t nlist = ctr[0];
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x / FBG_WAVE);
    const unsigned lane = threadIdx.x % FBG_WAVE;
    unsigned long long slots = 0;
    for (uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FBG_WAVE; k < nlist; k += nw) {
        const uint32_t u = list[k];
        const uint32_t m = d.len[u], bu = d.block[u];
        const uint2 lr = d.rng[u];
        for (uint64_t b = lr.x; b <= lr.y; b += FBG_WAVE) {
            const uint64_t i = b + lane;
            uint32_t node = 0, off = 0;
            bool bad = false;
            if (i <= lr.y) {
                slots++;
                bad = !pv_allowed(d, d.sa[i], m, bu, node, off);
            }
            const uint64_t bal = __ballot(bad);
            if (bal) {
                if (lane == (unsigned)__builtin_ctzll(bal)) {
                    status[u] = FBG_NODE_INVALID;
                    wn[u] = node;
                    wo[u] = off;
                }
                break;
            }
        }
    }
    pv_add_slots(&ctr[1], slots);
}

// cut[b - 1] = 1 for every block b > 0 that holds an INVALID node (the reference's to_remove); *count: INVALID nodes
__global__ void k_sv_cuts(const uint8_t *status, const uint32_t *node_block, uint64_t n, uint8_t *cut, unsigned long long *count)
{
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool bad = u < n && status[u] == FBG_NODE_INVALID;
    if (bad && node_block[u] > 0) cut[node_block[u] - 1] = 1;
    const uint64_t bal = __ballot(bad);
    if ((threadIdx.x % FBG_WAVE) == 0 && bal) atomicAdd(count, (unsigned long long)__popcll(bal));
}

// The validation kernels over the index's n_nodes > 0 nodes, blocks from d_block (device), between ev0 and ev1; status,
// witnesses and counters stay in vstatus / vwn / vwo / vctr.
static int pv_launch(fbg_pindex *ix, const uint32_t *d_block, const PvMask &ig, int has_ig)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = ix->n_nodes;
    FBG_TRY(px_reserve(ix, ix->vstatus, n));
    for (DevBuf *b : {&ix->vwn, &ix->vwo, &ix->vlist}) FBG_TRY(px_reserve(ix, *b, n * 4));
    FBG_TRY(px_reserve(ix, ix->vctr, 16));
    FBG_HIP_TRY(ctx, hipMemsetAsync(ix->vctr.p, 0, 16, st));
    PvDev d = pv_dev(ix);
    d.block = d_block;
    auto *ctr = ix->vctr.as<unsigned long long>();
    uint8_t *dst = ix->vstatus.as<uint8_t>();
    uint32_t *wn = ix->vwn.as<uint32_t>(), *wo = ix->vwo.as<uint32_t>();
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    hipLaunchKernelGGL(k_pv_node, dim3(fbg_blocks(n, PX_THREADS)), dim3(PX_THREADS), 0, st, d, n, ig, has_ig, dst, wn, wo,
                       ix->vlist.as<uint32_t>(), ctr);
    const uint64_t wave_blocks = std::min<uint64_t>(fbg_blocks(n * FBG_WAVE, PX_THREADS), 2048);
    hipLaunchKernelGGL(k_pv_wave, dim3(wave_blocks), dim3(PX_THREADS), 0, st, d, (const uint32_t *)ix->vlist.as<uint32_t>(), ctr, dst,
                       wn, wo);
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_TRY(px_record_end(ix));
    return FBG_OK;
}

static PvMask pv_mask(const uint8_t *ignore_chars, uint64_t ignore_len, int *has_ig)
{
    PvMask ig = {{0, 0, 0, 0}};
    for (uint64_t k = 0; k < ignore_len; k++) ig.w[ignore_chars[k] >> 6] |= 1ull << (ignore_chars[k] & 63);
    *has_ig = (ig.w[0] | ig.w[1] | ig.w[2] | ig.w[3]) != 0;
    return ig;
}

extern "C" int fbg_pindex_validate(fbg_pindex *ix, const uint32_t *node_block, const uint8_t *ignore_chars, uint64_t ignore_len,
                                   uint8_t *status, uint64_t *witness_node, uint64_t *witness_offset, uint64_t *n_invalid,
                                   double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    const uint64_t n = ix->n_nodes;
    if (n && (!node_block || !status)) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_validate: missing argument");
    if (ignore_len && !ignore_chars) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_validate: missing ignore characters");
    if (n_invalid) *n_invalid = 0;
    if (device_ms) *device_ms = 0;
    ix->validate_ms = 0;
    ix->v_slots = ix->v_wave_nodes = 0;
    if (n == 0) return FBG_OK;
    int has_ig = 0;
    const PvMask ig = pv_mask(ignore_chars, ignore_len, &has_ig);
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(px_reserve(ix, ix->vblock, n * 4));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(ix->vblock.p, node_block, n * 4, hipMemcpyHostToDevice, st));
    FBG_TRY(pv_launch(ix, ix->vblock.as<uint32_t>(), ig, has_ig));
    auto *ctr = ix->vctr.as<unsigned long long>();
    uint8_t *dst = ix->vstatus.as<uint8_t>();
    uint32_t *wn = ix->vwn.as<uint32_t>(), *wo = ix->vwo.as<uint32_t>();
    std::vector<uint32_t> hwn(witness_node ? n : 0), hwo(witness_offset ? n : 0);
    uint64_t hctr[2] = {0, 0};
    FBG_HIP_TRY(ctx, hipMemcpyAsync(status, dst, n, hipMemcpyDeviceToHost, st));
    if (witness_node) FBG_HIP_TRY(ctx, hipMemcpyAsync(hwn.data(), wn, n * 4, hipMemcpyDeviceToHost, st));
    if (witness_offset) FBG_HIP_TRY(ctx, hipMemcpyAsync(hwo.data(), wo, n * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(hctr, ctr, 16, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, &ix->validate_ms));
    ix->v_wave_nodes = hctr[0];
    ix->v_slots = hctr[1];
    uint64_t bad = 0;
    for (uint64_t u = 0; u < n; u++) bad += status[u] == FBG_NODE_INVALID;
    for (uint64_t u = 0; u < hwn.size(); u++) witness_node[u] = hwn[u] == PV_NONE ? UINT64_MAX : hwn[u];
    for (uint64_t u = 0; u < hwo.size(); u++) witness_offset[u] = hwo[u] == PV_NONE ? UINT64_MAX : hwo[u];
    if (n_invalid) *n_invalid = bad;
    if (device_ms) *device_ms = ix->validate_ms;
    return FBG_OK;
}

extern "C" int fbg_pindex_validate_stats(const fbg_pindex *ix, uint64_t *slots_scanned, uint64_t *wave_nodes, uint64_t *table_bytes)
{
    if (!ix) return FBG_ERR_INVALID;
    if (slots_scanned) *slots_scanned = ix->v_slots;
    if (wave_nodes) *wave_nodes = ix->v_wave_nodes;
    if (table_bytes) *table_bytes = 17 * ix->n_nodes + 12 * ix->n_edges + 4 + 4 * ix->nctab;
    return FBG_OK;
}

// One round: the index of the segmentation into ix (its buffers and the scratch are reused from round to round), the
// validation kernels on the device's own node_block, the flagged cuts.  The events sv0 / sv1 enclose all of it.
static int sv_round(fbg_pindex *ix, PxScratch &s, const uint64_t *boundaries, uint64_t nb, const PvMask &ig, int has_ig,
                    uint8_t *cut_bad, uint64_t *n_invalid, double *ms)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    FBG_HIP_TRY(ctx, hipEventRecord(ix->sv0, st));
    FBG_TRY(px_build_segmentation(ix, s, boundaries, nb, false));
    const uint64_t n = ix->n_nodes;
    FBG_TRY(px_reserve(ix, ix->scut, nb + 8));
    FBG_TRY(px_reserve(ix, ix->sctr, 8));
    FBG_HIP_TRY(ctx, hipMemsetAsync(ix->scut.p, 0, nb + 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(ix->sctr.p, 0, 8, st));
    if (n) {
        FBG_TRY(pv_launch(ix, ix->snode_block.as<uint32_t>(), ig, has_ig));
        hipLaunchKernelGGL(k_sv_cuts, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, (const uint8_t *)ix->vstatus.as<uint8_t>(),
                           (const uint32_t *)ix->snode_block.as<uint32_t>(), n, ix->scut.as<uint8_t>(), ix->sctr.as<unsigned long long>());
        FBG_HIP_TRY(ctx, hipGetLastError());
    }
    FBG_HIP_TRY(ctx, hipEventRecord(ix->sv1, st));
    unsigned long long bad = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(cut_bad, ix->scut.p, nb, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&bad, ix->sctr.p, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float f = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&f, ix->sv0, ix->sv1));
    *ms += f;
    *n_invalid = bad;
    return FBG_OK;
}

extern "C" int fbg_segmentation_validate(fbg_ctx *ctx, const uint64_t *boundaries, uint64_t nb, const uint8_t *ignore_chars,
                                         uint64_t ignore_len, uint8_t *cut_bad, uint64_t *n_nodes, uint64_t *n_invalid,
                                         double *device_ms)
{
    if (!ctx) return FBG_ERR_INVALID;
    if (!ctx->d_msa) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_segmentation_validate: no MSA set");
    if (!boundaries || nb == 0 || !cut_bad) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_segmentation_validate: missing argument");
    if (ignore_len && !ignore_chars) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_segmentation_validate: missing ignore characters");
    if (n_nodes) *n_nodes = 0;
    if (n_invalid) *n_invalid = 0;
    if (device_ms) *device_ms = 0;
    int has_ig = 0;
    const PvMask ig = pv_mask(ignore_chars, ignore_len, &has_ig);
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    fbg_pindex *ix = nullptr;
    FBG_TRY(px_new(ctx, &ix));
    uint64_t bad = 0;
    double ms = 0;
    int rc;
    {
        PxScratch s;
        rc = sv_round(ix, s, boundaries, nb, ig, has_ig, cut_bad, &bad, &ms);
    }
    if (rc == FBG_OK) {
        if (n_nodes) *n_nodes = ix->n_nodes;
        if (n_invalid) *n_invalid = bad;
        if (device_ms) *device_ms = ms;
    }
    px_destroy(ix);
    return rc;
}

extern "C" int fbg_segmentation_repair(fbg_ctx *ctx, uint64_t *boundaries, uint64_t *nb, const uint8_t *ignore_chars,
                                       uint64_t ignore_len, uint64_t *rounds, uint64_t *removed, double *device_ms)
{
    if (!ctx) return FBG_ERR_INVALID;
    if (!ctx->d_msa) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_segmentation_repair: no MSA set");
    if (!boundaries || !nb || *nb == 0 || !rounds || !removed) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_segmentation_repair: missing argument");
    if (ignore_len && !ignore_chars) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_segmentation_repair: missing ignore characters");
    *rounds = 0;
    if (device_ms) *device_ms = 0;
    int has_ig = 0;
    const PvMask ig = pv_mask(ignore_chars, ignore_len, &has_ig);
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    fbg_pindex *ix = nullptr;
    FBG_TRY(px_new(ctx, &ix));
    std::vector<uint8_t> cut(*nb);
    double ms = 0;
    int rc = FBG_OK;
    {
        PxScratch s;
        // fbg.cpp:3471-3497: validate, drop the flagged boundaries, again until none is flagged.  Every round with a
        // flagged cut shortens the list, and a single block has no node with both an in- and an out-edge.
        for (;;) {
            uint64_t bad = 0;
            rc = sv_round(ix, s, boundaries, *nb, ig, has_ig, cut.data(), &bad, &ms);
            if (rc != FBG_OK) break;
            uint64_t flagged = 0, keep = 0;
            for (uint64_t k = 0; k < *nb; k++) flagged += cut[k] != 0;
            if (!flagged) break;
            removed[(*rounds)++] = flagged;
            for (uint64_t k = 0; k < *nb; k++)
                if (!cut[k]) boundaries[keep++] = boundaries[k];
            *nb = keep;
        }
    }
    if (rc == FBG_OK && device_ms) *device_ms = ms;
    px_destroy(ix);
    return rc;
}
