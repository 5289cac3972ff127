// rx_flows_host.h -- the call skeleton of the two multi-flow device receivers: ldpc_amd_fec_rx_flows (wire_dev.hip, two open blocks
// per flow) and ldpc_amd_fec_rxw_flows (rx_window_flows_dev.hip, a window of W).  rx_host.h holds what all four receivers share on
// the decode tail; this header holds what the two multi-flow ones share in front of it and around it: the argument checks and their
// order, the plan (reserve, read-back, upload, partition, headers, scan, ONE copy back, ONE synchronisation, the flow table), the
// push and the decode call, the commit loop, the batch flush and its flow list, the allocation ladder of create and the free list
// of destroy.  No kernel lives here and none is named here: the two units cannot see each other's scan record (rx_host.h says why),
// so everything below is a function template over a POLICY P that each unit defines next to its kernels:
//   P::Rx                                   the receiver object: ctx, nflows, n, k, S, unrouted, stage_sym, stage_er, the scratches dense /
//                                           dest / win / res / slots / order, in_dev / in_host, tab_dev / tab_host, res_host(_cap), fl
//   planes_per_flow(rx)                     staging planes of a flow: 2 or W
//   fill_in(rx, f, begin, len)              in_host[f]: the flow's segment and the state its scan starts from
//   launch_headers(rx, aligned4, packets, flow_of, base, order, np, plen, dense)   (a); order != null: a mixed call's -- the partition
//                                           (flows_demux_dev.h; it writes base and every in_dev[f]'s segment), then (a') on it
//   launch_scan(rx, dense, max_blocks, dest, res)                              (b)
//   rec_words(max_blocks), err(h), closes(h), consumed(h)                      one flow's result record and its readers
//   tab_entry(rx, f, begin, used, base, closes)                                tab_host[f]
//   launch_slots(rx), launch_winners(rx, pl, gx, win)                          the slot map and (c)
//   launch_move(rx, pl, packets, gather, first, count, sym, er, v16, items)    (d) / (e)
//   launch_left(rx, pl, gx, left), launch_sources(rx, T, src, er)              a mixed call's `left`; (d') of the fused decode
//   commit_flow(rx, f, h, closes)                                              flow f's mirror behind a call
//   record_info(ctx, fused, T, launches, scratch)                              the info words of a decode call
//   flush_fill(rx, f, rounds, pl)           appends the blocks and planes a flush of flow f hands out; returns how many
//   flush_gather(rx, first, count, sym, er), flush_after(rx, fused, T)         the planes -> dense slots; what stands behind them
//   launch_flush_sources(rx, T, src, er)                                       the row sources of the fused decode of a flush
//   flush_commit_flow(rx, f, count)         flow f's mirror behind a flush of `count` blocks
//   record_flush(ctx, path, T, n, launches, scratch)                           the info words of a flush call (path 3: no decode)
// A refused call changes nothing: every check and every reserve stands in front of the first launch, and the mirror and the info
// words are written last.  Everything here has internal linkage, as in rx_host.h.
#ifndef LDPC_ERASURE_AMD_RX_FLOWS_HOST_H
#define LDPC_ERASURE_AMD_RX_FLOWS_HOST_H

#include <vector>

#include "rx_host.h"
#include "flows_demux_dev.h"   // the partition of a mixed call

namespace ldpc_amd {
namespace {

constexpr int kRxfHdr = 8;         // LDPC_AMD_FEC_HEADER_BYTES
constexpr int kRxfThreads = 256;   // work items of a workgroup of the per-flow launches

// Where the packets of a call are: segmented by the caller (flow_begin, host) or interleaved with a flow number each (flow_of, device)
struct RxFlowsSrc {
    bool mixed = false;
    const int64_t *flow_begin = nullptr;
    const int32_t *flow_of = nullptr;
};

// the host outputs of a call (all may be null) and a mixed call's `left` (device, may be null)
struct RxFlowsOut {
    int *blocks, *closes;
    int64_t *consumed, *offered;
    uint8_t *left;
};

// One call's PLAN for all flows: (a) + (b), ONE read-back, the slot bases.  Nothing of any flow's state changes before rxf_commit.
struct RxFlowsPlan {
    int T = 0;             // closed blocks of all flows
    int64_t max_used = 0;  // the longest consumed prefix
    size_t rec = 0;        // words of one flow's result record
    // a mixed call (else null / 0): the partition, the flow bases as read back behind the scan records ([nflows + 1], the last one =
    // the routed packets), the longest remainder behind a consumed prefix
    const uint32_t *order = nullptr, *base = nullptr;
    int64_t max_left = 0;
};

template <class Rx>
int rxf_check_limits(const Rx *rx, const char *who, int64_t P, int max_blocks)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    if (P < 0 || P >= ((int64_t)1 << 31)) return set_error(ctx, LDPC_AMD_EINVAL, "%s: need fewer than 2^31 packets in all", who);
    if (max_blocks < 1) return set_error(ctx, LDPC_AMD_EINVAL, "%s: need max_blocks_per_flow >= 1", who);
    if ((int64_t)rx->nflows * max_blocks * rx->n >= ((int64_t)1 << 31) - 2)
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: nflows * max_blocks_per_flow * n must be below 2^31 - 2", who);
    return LDPC_AMD_OK;
}

// the packets of the call and the limits: P is the segmented call's flow_begin[nflows], or the mixed call's argument
template <class Rx>
int rxf_check_call(const Rx *rx, const char *who, const RxFlowsSrc &src, int max_blocks, int64_t &P)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    if (src.mixed) return rxf_check_limits(rx, who, P, max_blocks);
    const int64_t *flow_begin = src.flow_begin;
    if (!flow_begin || flow_begin[0] != 0) return set_error(ctx, LDPC_AMD_EINVAL, "%s: flow_begin must not be null and must start at 0", who);
    for (int f = 0; f < rx->nflows; f++)
        if (flow_begin[f + 1] < flow_begin[f]) return set_error(ctx, LDPC_AMD_EINVAL, "%s: flow_begin decreases at flow %d", who, f);
    P = flow_begin[rx->nflows];
    return rxf_check_limits(rx, who, P, max_blocks);
}

// the mixed calls' own arguments, P > 0 (the device is set)
template <class Rx>
int rxf_check_mixed(const Rx *rx, const char *who, const int32_t *flow_of, const uint8_t *left)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    if (!flow_of || !is_device_ptr(ctx, flow_of))
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: flow_of must be a device pointer of device %d", who, ctx->device);
    if ((uintptr_t)flow_of & 3) return set_error(ctx, LDPC_AMD_EINVAL, "%s: flow_of must be 4-byte aligned", who);
    if (left && !is_device_ptr(ctx, left)) return set_error(ctx, LDPC_AMD_EINVAL, "%s: left must be a device pointer of device %d", who, ctx->device);
    return LDPC_AMD_OK;
}

// a call of no packets
template <class Rx>
int rxf_nothing(const Rx *rx, const RxFlowsOut &o)
{
    if (o.closes) std::fill(o.closes, o.closes + rx->nflows, 0);
    if (o.consumed) std::fill(o.consumed, o.consumed + rx->nflows, (int64_t)0);
    if (o.offered) std::fill(o.offered, o.offered + rx->nflows, (int64_t)0);
    return 0;
}

// grid x of the launches that have one grid row per flow
inline unsigned rxf_grid_x(int64_t items, int nflows)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kRxfThreads - 1) / kRxfThreads, std::max(1, 32768 / nflows)));
}

template <class P>
int rxf_plan(typename P::Rx *rx, const char *who, const uint8_t *packets, const RxFlowsSrc &src, int64_t npackets, int max_blocks, RxFlowsPlan &pl)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int n = rx->n, nf = rx->nflows;
    const int64_t plen = (int64_t)rx->S + kRxfHdr;
    const int64_t *flow_begin = src.flow_begin;
    const bool mixed = src.mixed;
    pl.rec = P::rec_words(max_blocks);
    const size_t res_bytes = sizeof(int32_t) * (pl.rec * (size_t)nf + (mixed ? (size_t)nf + 1 : 0));   // mixed: the flow bases behind the records
    int rc;
    if ((rc = scratch_reserve(ctx, rx->dense, sizeof(uint32_t) * (size_t)npackets)) ||
        (rc = scratch_reserve(ctx, rx->dest, sizeof(int32_t) * (size_t)npackets)) || (rc = scratch_reserve(ctx, rx->res, res_bytes)))
        return rc;
    if (mixed && ((rc = scratch_reserve(ctx, rx->order, sizeof(uint32_t) * (size_t)npackets)) || (rc = demux_reserve(ctx, npackets, nf)))) return rc;
    if ((rc = rx_readback_grow(ctx, rx, res_bytes))) return rc;
    uint32_t *dense = (uint32_t *)rx->dense.p;
    int32_t *dest = (int32_t *)rx->dest.p, *res = (int32_t *)rx->res.p;
    for (int f = 0; f < nf; f++)   // (the copy of the previous call's records is behind that call's synchronisation)
        P::fill_in(rx, f, mixed ? 0 : flow_begin[f], mixed ? 0 : flow_begin[f + 1] - flow_begin[f]);
    LDPC_HIP_TRY(ctx, hipMemcpyAsync(rx->in_dev, rx->in_host, sizeof(*rx->in_host) * (size_t)nf, hipMemcpyHostToDevice, ctx->stream));
    // (a) + (b): the plan; a mixed call's on the partition, which also fills in every flow's segment (begin, len) on the device
    const bool aligned4 = plen % 4 == 0 && ((uintptr_t)packets & 3) == 0;
    uint32_t *base = mixed ? (uint32_t *)res + pl.rec * (size_t)nf : nullptr, *order = mixed ? (uint32_t *)rx->order.p : nullptr;
    if ((rc = P::launch_headers(rx, aligned4, packets, src.flow_of, base, order, npackets, (int)plen, dense))) return rc;
    if (mixed) {
        pl.order = order;
        pl.base = (const uint32_t *)rx->res_host + pl.rec * (size_t)nf;
    }
    LDPC_HIP_TRY(ctx, hipGetLastError());
    P::launch_scan(rx, (const uint32_t *)dense, max_blocks, dest, res);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    LDPC_HIP_TRY(ctx, hipMemcpyAsync(rx->res_host, res, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    LDPC_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = check_device_error(ctx))) return rc;
    int64_t slot = 0;   // the flow's first closed slot
    for (int f = 0; f < nf; f++) {   // the tables of the kernels behind the plan (their copy of the previous call is behind this synchronisation)
        const int32_t *h = rx->res_host + (size_t)f * pl.rec;
        if (P::err(h))
            return set_error(ctx, LDPC_AMD_EHIP, "%s: the plan scan of flow %d hit its iteration cap (internal error); every flow's state is unchanged",
                             who, f);
        const int64_t used = P::consumed(h);
        rx->tab_host[f] = P::tab_entry(rx, f, mixed ? (int64_t)pl.base[f] : flow_begin[f], used, (int)slot, P::closes(h));
        slot += P::closes(h);
        pl.max_used = std::max(pl.max_used, used);
        if (mixed) pl.max_left = std::max(pl.max_left, (int64_t)(pl.base[f + 1] - pl.base[f]) - used);
    }
    pl.T = (int)slot;   // <= nflows * max_blocks < 2^31
    if ((rc = scratch_reserve(ctx, rx->win, sizeof(int32_t) * ((size_t)pl.T + (size_t)P::planes_per_flow(rx) * (size_t)nf) * (size_t)n)) ||
        (rc = scratch_reserve(ctx, rx->slots, sizeof(int32_t) * (size_t)std::max(pl.T, 1))))
        return rc;
    return LDPC_AMD_OK;
}

// the flow table, the slot map and (c): the winners' table of the call, [(T + planes_per_flow nflows)][n]
template <class P>
int rxf_winners(typename P::Rx *rx, const RxFlowsPlan &pl)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int nf = rx->nflows;
    int32_t *win = (int32_t *)rx->win.p;
    LDPC_HIP_TRY(ctx, hipMemcpyAsync(rx->tab_dev, rx->tab_host, sizeof(*rx->tab_host) * (size_t)nf, hipMemcpyHostToDevice, ctx->stream));
    if (pl.T > 0) {
        P::launch_slots(rx);
        LDPC_HIP_TRY(ctx, hipGetLastError());
    }
    LDPC_HIP_TRY(ctx, hipMemsetAsync(win, 0xff, sizeof(int32_t) * ((size_t)pl.T + (size_t)P::planes_per_flow(rx) * (size_t)nf) * (size_t)rx->n,
                                     ctx->stream));   // -1: no packet
    return P::launch_winners(rx, pl, rxf_grid_x(pl.max_used, nf), win);
}

// (d) for the closed slots first .. first + count - 1 (gather) or (e) for the open blocks of every flow
template <class P>
int rxf_move(typename P::Rx *rx, const RxFlowsPlan &pl, const uint8_t *packets, bool gather, int first, int count, uint8_t *sym, uint8_t *er)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int n = rx->n, S = rx->S;
    if (gather && count <= 0) return LDPC_AMD_OK;
    const bool v16 = S % 16 == 0 && ((uintptr_t)packets & 7) == 0 && ((uintptr_t)sym & 15) == 0;
    const int64_t items = (gather ? (int64_t)count : (int64_t)P::planes_per_flow(rx) * rx->nflows) * n * (v16 ? S / 16 : S);
    P::launch_move(rx, pl, packets, gather, first, count, sym, er, v16, items);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

// a mixed call's `left` (may be null): zero, then 1 behind every flow's consumed prefix
template <class P>
int rxf_left(typename P::Rx *rx, const RxFlowsPlan &pl, int64_t npackets, uint8_t *left)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    if (!left) return LDPC_AMD_OK;
    LDPC_HIP_TRY(ctx, hipMemsetAsync(left, 0, (size_t)npackets, ctx->stream));
    if (pl.max_left <= 0) return LDPC_AMD_OK;
    P::launch_left(rx, pl, rxf_grid_x(pl.max_left, rx->nflows), left);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

// every flow's mirror and the host outputs: the last step of a call (a mixed call: offered and the unrouted count too)
template <class P>
void rxf_commit(typename P::Rx *rx, const RxFlowsPlan &pl, const RxFlowsOut &o, int64_t npackets)
{
    if (pl.base) {
        rx->unrouted += npackets - (int64_t)pl.base[rx->nflows];
        for (int f = 0; o.offered && f < rx->nflows; f++) o.offered[f] = (int64_t)(pl.base[f + 1] - pl.base[f]);
    }
    for (int f = 0; f < rx->nflows; f++) {
        const int32_t *h = rx->res_host + (size_t)f * pl.rec;
        const auto &t = rx->tab_host[f];
        P::commit_flow(rx, f, h, t.closes);
        if (o.blocks) memcpy(o.blocks + t.base, h + P::rec_words(0), sizeof(int) * (size_t)t.closes);
        if (o.closes) o.closes[f] = t.closes;
        if (o.consumed) o.consumed[f] = t.used;
    }
}

// push_many and push_mixed
template <class P>
int rxf_push(typename P::Rx *rx, const char *who, const uint8_t *packets, const RxFlowsSrc &src, int64_t np, uint8_t *sym_batch,
             uint8_t *erased_batch, int max_blocks_per_flow, const RxFlowsOut &o)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    int rc;
    if ((rc = rxf_check_call(rx, who, src, max_blocks_per_flow, np))) return rc;
    if (!sym_batch || !erased_batch || (np > 0 && !packets))
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: packets / sym_batch / erased_batch must not be null", who);
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((np > 0 && !is_device_ptr(ctx, packets)) || !is_device_ptr(ctx, sym_batch) || !is_device_ptr(ctx, erased_batch))
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: packets / sym_batch / erased_batch must be device pointers of device %d", who, ctx->device);
    if (np == 0) return rxf_nothing(rx, o);
    if (src.mixed && (rc = rxf_check_mixed(rx, who, src.flow_of, o.left))) return rc;
    RxFlowsPlan pl;
    if ((rc = rxf_plan<P>(rx, who, packets, src, np, max_blocks_per_flow, pl))) return rc;
    // (c), (d), (e): the data movement, asynchronous
    if ((rc = rxf_winners<P>(rx, pl)) || (rc = rxf_move<P>(rx, pl, packets, true, 0, pl.T, sym_batch, erased_batch)) ||
        (rc = rxf_move<P>(rx, pl, packets, false, 0, 0, sym_batch, nullptr)) || (rc = rxf_left<P>(rx, pl, np, o.left)))
        return rc;
    rxf_commit<P>(rx, pl, o, np);
    return pl.T;
}

// push + decode_frames in one call (rx_host.h: the decode driver): ONE launch_decode over the T closed slots of all flows where the
// decoder can fetch its rows from the packets itself (FUSED: (d) shrinks to the row-source kernel, the planes of all flows being
// one `stage` base), else one per chunk of gathered slots (COMPOSED).  (e) is launched BEHIND the decode in both forms: it
// overwrites the staging planes of the carried blocks, which the fused decode reads.
template <class P>
int rxf_decode(typename P::Rx *rx, const char *who, int code, const uint8_t *packets, const RxFlowsSrc &src, int64_t np, int max_sweeps, int do_ml,
               const RxResults &res, int max_blocks_per_flow, const RxFlowsOut &o)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    if (code < 0 || code >= (int)ctx->codes.size()) return set_error(ctx, LDPC_AMD_ENOCODE, "unknown code handle %d", code);
    int rc;
    if ((rc = rxf_check_call(rx, who, src, max_blocks_per_flow, np))) return rc;
    if (np == 0) return rxf_nothing(rx, o);
    if ((rc = rx_decode_check(ctx, rx, who, code, max_sweeps, res))) return rc;
    if (!packets || !is_device_ptr(ctx, packets))
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: packets must be a device pointer of device %d", who, ctx->device);
    if (src.mixed && (rc = rxf_check_mixed(rx, who, src.flow_of, o.left))) return rc;
    const DevCode &cd = ctx->codes[code]->dev;
    const int n = rx->n, S = rx->S;
    const bool fused = ctx->knobs.rx_pkt != 0 && ((uintptr_t)packets & 7) == 0 && decode_reads_packets(ctx, cd, S);
    const size_t frame = (size_t)n * S;

    RxFlowsPlan pl;
    if ((rc = rxf_plan<P>(rx, who, packets, src, np, max_blocks_per_flow, pl))) return rc;
    const int T = pl.T;
    const int64_t chunk = rx_chunk(T, frame);
    size_t scratch = 0;
    if ((rc = rx_decode_reserve(ctx, T, n, frame, fused, chunk, &scratch))) return rc;
    if ((rc = rxf_winners<P>(rx, pl))) return rc;
    DecodeArgs d = rx_decode_args(cd, n, S, max_sweeps, do_ml);
    const PacketRows pin{nullptr, packets, rx->stage_sym, S + kRxfHdr};
    auto sources = [&](uint32_t *rows, uint8_t *er) -> int {
        P::launch_sources(rx, T, rows, er);
        LDPC_HIP_TRY(ctx, hipGetLastError());
        return LDPC_AMD_OK;
    };
    auto gather = [&](int first, int count, uint8_t *sym, uint8_t *er) { return rxf_move<P>(rx, pl, packets, true, first, count, sym, er); };
    int launches = 0;
    if ((rc = rx_decode_slots(ctx, d, res, T, chunk, fused, pin, sources, gather, &launches))) return rc;
    if ((rc = rxf_move<P>(rx, pl, packets, false, 0, 0, nullptr, nullptr))) return rc;   // (e)
    if ((rc = rxf_left<P>(rx, pl, np, o.left))) return rc;
    rxf_commit<P>(rx, pl, o, np);
    P::record_info(ctx, fused, T, launches, scratch);
    return T;
}

// ---- the batch flush ------------------------------------------------------------------------------------------------------------------
// The PLAN is the host's: the mirror knows every flow's state, so which blocks are handed out, in which order and from which plane
// is decided without the device.  Every handed-out block lies complete in ONE staging plane; one int32 plane number per slot goes up.
struct RxFlushPlan {
    std::vector<int> sel;          // the listed flows, in list order
    std::vector<int> closes;       // blocks handed out per list entry
    std::vector<int> blocks;       // [T] their wire numbers, in slot order
    std::vector<int32_t> planes;   // [T] their staging planes, f * planes_per_flow + b
    int T = 0;
};

// flows: the list (null: every flow, in order); rounds: the policy's (flush_fill)
template <class P>
int rxf_flush_plan(const typename P::Rx *rx, const char *who, const int32_t *flows, int nsel, int rounds, RxFlushPlan &pl)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    if (flows) {
        if (nsel < 0 || nsel > rx->nflows) return set_error(ctx, LDPC_AMD_EINVAL, "%s: need 0 <= nsel <= nflows = %d (got %d)", who, rx->nflows, nsel);
        std::vector<uint8_t> seen((size_t)rx->nflows, 0);
        for (int j = 0; j < nsel; j++) {
            const int f = flows[j];
            if (f < 0 || f >= rx->nflows) return set_error(ctx, LDPC_AMD_EINVAL, "%s: no flow %d (nflows = %d)", who, f, rx->nflows);
            if (seen[(size_t)f]) return set_error(ctx, LDPC_AMD_EINVAL, "%s: flow %d is given twice", who, f);
            seen[(size_t)f] = 1;
        }
    } else {
        nsel = rx->nflows;
    }
    pl.sel.resize((size_t)nsel);
    pl.closes.resize((size_t)nsel);
    for (int j = 0; j < nsel; j++) {
        pl.sel[(size_t)j] = flows ? flows[j] : j;
        pl.closes[(size_t)j] = P::flush_fill(rx, pl.sel[(size_t)j], rounds, pl);
    }
    pl.T = (int)pl.planes.size();   // <= planes_per_flow nflows
    return LDPC_AMD_OK;
}

// a flush that hands nothing out
inline int rxf_flush_nothing(const RxFlushPlan &pl, int *closes)
{
    if (closes) std::fill(closes, closes + pl.sel.size(), 0);
    return 0;
}

// the mirror of every listed flow behind its flush, the host outputs, the info words
template <class P>
void rxf_flush_commit(typename P::Rx *rx, const RxFlushPlan &pl, int *blocks, int *closes, int path, int launches, size_t scratch)
{
    for (size_t j = 0; j < pl.sel.size(); j++) {
        if (closes) closes[j] = pl.closes[j];
        P::flush_commit_flow(rx, pl.sel[j], pl.closes[j]);
    }
    if (blocks && pl.T > 0) memcpy(blocks, pl.blocks.data(), sizeof(int) * (size_t)pl.T);
    P::record_flush(rx->ctx, path, pl.T, rx->n, launches, scratch);
}

template <class P>
int rxf_flush_many(typename P::Rx *rx, const char *who, const int32_t *flows, int nsel, int rounds, uint8_t *sym_batch, uint8_t *erased_batch,
                   int *blocks, int *closes)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    RxFlushPlan pl;
    int rc;
    if ((rc = rxf_flush_plan<P>(rx, who, flows, nsel, rounds, pl))) return rc;
    if (!sym_batch || !erased_batch) return set_error(ctx, LDPC_AMD_EINVAL, "%s: sym_batch / erased_batch must not be null", who);
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!is_device_ptr(ctx, sym_batch) || !is_device_ptr(ctx, erased_batch))
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: sym_batch / erased_batch must be device pointers of device %d", who, ctx->device);
    if (pl.T == 0) return rxf_flush_nothing(pl, closes);
    if ((rc = rx_upload_planes(ctx, who, rx->fl, (size_t)P::planes_per_flow(rx) * (size_t)rx->nflows, pl.planes.data(), pl.T)) ||
        (rc = P::flush_gather(rx, 0, pl.T, sym_batch, erased_batch)) || (rc = P::flush_after(rx, false, pl.T)))
        return rc;
    rxf_flush_commit<P>(rx, pl, blocks, closes, 3, 0, 0);
    return pl.T;
}

// flush_many + decode.  FUSED where the decoder has the packets-in form and S % 16 == 0: every row of every block is staged (or
// erased), the policy's flush row sources name it and ONE launch_decode follows the words into the planes.  Else COMPOSED: a chunk
// of planes goes to the scratch and through the decoder.  flush_after stands BEHIND the decode, which reads the planes.
template <class P>
int rxf_decode_flush_many(typename P::Rx *rx, const char *who, int code, const int32_t *flows, int nsel, int rounds, int max_sweeps, int do_ml,
                          const RxResults &o, int *blocks, int *closes)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    RxFlushPlan pl;
    int rc;
    if ((rc = rxf_flush_plan<P>(rx, who, flows, nsel, rounds, pl))) return rc;
    if ((rc = rx_decode_check(ctx, rx, who, code, max_sweeps, o))) return rc;
    const int T = pl.T;
    if (T == 0) return rxf_flush_nothing(pl, closes);
    const DevCode &cd = ctx->codes[code]->dev;
    const int n = rx->n, S = rx->S;
    const bool fused = ctx->knobs.rx_pkt != 0 && S % 16 == 0 && decode_reads_packets(ctx, cd, S);   // (word-sized symbols: composed)
    const size_t frame = (size_t)n * S;
    const int64_t chunk = rx_chunk(T, frame);
    size_t scratch = 0;
    if ((rc = rx_decode_reserve(ctx, T, n, frame, fused, chunk, &scratch))) return rc;
    if ((rc = rx_upload_planes(ctx, who, rx->fl, (size_t)P::planes_per_flow(rx) * (size_t)rx->nflows, pl.planes.data(), pl.T))) return rc;
    DecodeArgs d = rx_decode_args(cd, n, S, max_sweeps, do_ml);
    // no word of the table names a packet, so the packet base is never added to: any valid aligned address
    const PacketRows pin{nullptr, rx->stage_sym, rx->stage_sym, S + kRxfHdr};
    auto sources = [&](uint32_t *src, uint8_t *er) -> int {
        P::launch_flush_sources(rx, T, src, er);
        LDPC_HIP_TRY(ctx, hipGetLastError());
        return LDPC_AMD_OK;
    };
    auto gather = [&](int first, int count, uint8_t *sym, uint8_t *er) { return P::flush_gather(rx, first, count, sym, er); };
    int launches = 0;
    if ((rc = rx_decode_slots(ctx, d, o, T, chunk, fused, pin, sources, gather, &launches))) return rc;
    if ((rc = P::flush_after(rx, fused, T))) return rc;
    rxf_flush_commit<P>(rx, pl, blocks, closes, fused ? 1 : 2, launches, scratch);
    return T;
}

// ---- create and destroy ---------------------------------------------------------------------------------------------------------------
template <class Rx>
void rxf_destroy(Rx *rx)
{
    if (!rx) return;
    (void)hipSetDevice(rx->ctx->device);
    (void)hipStreamSynchronize(rx->ctx->stream);   // pending work of this object may still use its buffers
    Scratch *sc[] = {&rx->dense, &rx->dest, &rx->win, &rx->res, &rx->slots, &rx->order};
    for (Scratch *s : sc)
        if (s->p) (void)hipFree(s->p);
    void *dev[] = {rx->stage_sym, rx->stage_er, rx->in_dev, rx->tab_dev};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    void *host[] = {rx->in_host, rx->tab_host, rx->res_host};
    for (void *p : host)
        if (p) (void)hipHostFree(p);
    rx_upload_free(rx->fl);
    delete rx;
}

// The device and pinned memory of an object whose host members are set; on failure the object is destroyed.
template <class P>
int rxf_create_buffers(ldpc_amd_ctx *ctx, typename P::Rx *rx, const char *who, typename P::Rx **out)
{
    const size_t nf = (size_t)rx->nflows, planes = (size_t)P::planes_per_flow(rx) * nf, plane = (size_t)rx->n * rx->S;
    // (a request beyond the device's memory is not always answered with hipErrorOutOfMemory: a staging plane that cannot be had is ENOMEM)
    hipError_t e = hipMalloc((void **)&rx->stage_sym, planes * plane);
    if (e == hipSuccess) e = hipMalloc((void **)&rx->stage_er, planes * (size_t)rx->n);
    const bool no_planes = e != hipSuccess;
    if (e == hipSuccess) e = hipMalloc((void **)&rx->in_dev, sizeof(*rx->in_dev) * nf);
    if (e == hipSuccess) e = hipMalloc((void **)&rx->tab_dev, sizeof(*rx->tab_dev) * nf);
    if (e == hipSuccess) e = hipHostMalloc((void **)&rx->in_host, sizeof(*rx->in_host) * nf, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&rx->tab_host, sizeof(*rx->tab_host) * nf, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemsetAsync(rx->stage_sym, 0, planes * plane, ctx->stream);   // payload zero, every symbol erased
    if (e == hipSuccess) e = hipMemsetAsync(rx->stage_er, 1, planes * (size_t)rx->n, ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        rxf_destroy(rx);
        return set_error(ctx, no_planes || e == hipErrorOutOfMemory ? LDPC_AMD_ENOMEM : LDPC_AMD_EHIP, "%s: %s%s", who,
                         no_planes ? "the staging planes do not fit: " : "", hipGetErrorString(e));
    }
    *out = rx;
    return LDPC_AMD_OK;
}

}  // namespace
}  // namespace ldpc_amd

#endif  // LDPC_ERASURE_AMD_RX_FLOWS_HOST_H
