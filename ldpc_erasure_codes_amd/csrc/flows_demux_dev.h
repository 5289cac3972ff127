// flows_demux_dev.h -- the partition of interleaved packets by flow (include/ldpc_erasure_amd_flows_mixed.h), shared by the device
// units whose receivers take a packet array in arrival order with a flow number each: wire_dev.hip (the two-buffer flows, and the
// partition on its own) and rx_window_flows_dev.hip (the windowed flows).
// Everything here has internal linkage: each unit that includes the header gets its own copy.
//
// Nothing behind a receiver's plan needs a flow's packets side by side -- the plan reads the dense header words, the gather and the
// decoder address a payload by packet index -- so only the packet INDICES are partitioned by flow: order[q] = the q-th packet when
// the routed packets are listed flow by flow, each flow in arrival order.  The plan then runs on positions q (dense[q] = header of
// packets[order[q]], flow f's segment is base[f] .. base[f+1]-1).
//
// The partition is a stable counting sort in three steps over TILES of consecutive packets (tile length a multiple of 64):
//   (i)   fec_demux_count   one workgroup per tile: histogram of the tile's flows in LDS -> row `tile` of table[tiles][nflows]
//   (ii)  fec_demux_tiles   per flow an exclusive scan down the tiles, in place; the flow's total -> base[f]
//         fec_demux_bases   one wavefront: exclusive scan of the totals across flows, in place; base[nflows] = routed packets
//   (iii) fec_demux_place   ONE WAVEFRONT per tile walks it in index order, 64 packets at a time, with a running position per flow in
//                           LDS (base[f] + table[tile][f] at the start).  Within a group a lane finds the lanes of its own flow with
//                           one ballot per bit of the flow number (at most 12) and takes its rank among them from a prefix popcount;
//                           the packet goes to position[flow] + rank, and the first lane of each flow advances the position by the
//                           flow's lanes.
// Stability and determinism: packets of flow f in an earlier tile come first (ii), inside a tile those of an earlier group come first
// (one wavefront executes its groups in order, so a group reads the positions the group before it wrote), inside a group the lower
// lane comes first (the prefix popcount).  No atomic decides a position; those of (i) only count.
// A flow number outside 0 .. nflows-1 (compared unsigned, so negative ones too) is no flow: the packet is counted nowhere and gets no position.
#ifndef LDPC_ERASURE_AMD_FLOWS_DEMUX_DEV_H
#define LDPC_ERASURE_AMD_FLOWS_DEMUX_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "internal.h"

namespace {

constexpr int kMaxFlows = 4096;
constexpr int kDemuxThreads = 256;
constexpr int64_t kDemuxMaxTiles = 1024, kDemuxMinTile = 1024;   // the table is at most kDemuxMaxTiles * kMaxFlows words: the tile grows instead

__global__ __launch_bounds__(kDemuxThreads) void fec_demux_count(const int32_t *__restrict__ flow_of, int64_t np, int64_t tile, int nflows,
                                                                uint32_t *__restrict__ table)
{
    __shared__ uint32_t cnt[kMaxFlows];
    for (int f = threadIdx.x; f < nflows; f += kDemuxThreads) cnt[f] = 0;
    __syncthreads();
    const int64_t p0 = (int64_t)blockIdx.x * tile, p1 = p0 + tile < np ? p0 + tile : np;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += kDemuxThreads) {
        const uint32_t f = (uint32_t)flow_of[p];
        if (f < (uint32_t)nflows) atomicAdd(&cnt[f], 1u);
    }
    __syncthreads();
    uint32_t *row = table + (int64_t)blockIdx.x * nflows;
    for (int f = threadIdx.x; f < nflows; f += kDemuxThreads) row[f] = cnt[f];
}

// Workgroup: 64 flows x kDemuxChunks runs of consecutive tiles.  A thread sums its run of its flow's column (loads only, so they
// overlap), the runs' sums are scanned through LDS, and the thread walks its run again, eight tiles at a time, writing the exclusive
// prefix over each count.  A column read one tile after the other would cost a memory latency per tile.
constexpr int kDemuxChunks = 16;
__global__ __launch_bounds__(64 * kDemuxChunks) void fec_demux_tiles(uint32_t *__restrict__ table, int tiles, int nflows,
                                                                    uint32_t *__restrict__ base)
{
    __shared__ uint32_t part[kDemuxChunks][64];
    const int f = blockIdx.x * 64 + threadIdx.x, c = threadIdx.y;
    const int per = (tiles + kDemuxChunks - 1) / kDemuxChunks;
    const int t0 = c * per < tiles ? c * per : tiles, t1 = t0 + per < tiles ? t0 + per : tiles;
    const bool live = f < nflows;
    uint32_t sum = 0;
    if (live)
        for (int t = t0; t < t1; t++) sum += table[(int64_t)t * nflows + f];
    part[c][threadIdx.x] = sum;
    __syncthreads();
    if (!live) return;
    uint32_t run = 0;
    for (int j = 0; j < c; j++) run += part[j][threadIdx.x];
    if (c == kDemuxChunks - 1) base[f] = run + sum;
    for (int t = t0; t < t1; t += 8) {
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = t + u < t1 ? table[(int64_t)(t + u) * nflows + f] : 0u;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (t + u < t1) table[(int64_t)(t + u) * nflows + f] = run;
            run += v[u];
        }
    }
}

// Lane l owns the flows l * chunk .. (l + 1) * chunk - 1.  With `in` it also writes every flow's segment of the q-space, where the
// plan scan looks for it (the host has uploaded the rest of the record).  Rec: the unit's flow record, with int64 begin and len.
template <typename Rec>
__global__ __launch_bounds__(64) void fec_demux_bases(uint32_t *__restrict__ base, int nflows, Rec *__restrict__ in)
{
    const int lane = threadIdx.x, chunk = (nflows + 63) / 64;
    const int f0 = lane * chunk, f1 = f0 + chunk < nflows ? f0 + chunk : nflows;
    uint32_t sum = 0;
    for (int f = f0; f < f1; f++) sum += base[f];
    uint32_t incl = sum;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    const uint32_t total = __shfl(incl, 63);
    uint32_t run = incl - sum;
    for (int f = f0; f < f1; f++) {
        const uint32_t v = base[f];
        base[f] = run;
        if (in) {
            in[f].begin = run;
            in[f].len = v;
        }
        run += v;
    }
    if (lane == 0) base[nflows] = total;
}

__global__ __launch_bounds__(64) void fec_demux_place(const int32_t *__restrict__ flow_of, int64_t np, int64_t tile, int nflows,
                                                     int bits, const uint32_t *__restrict__ table, const uint32_t *__restrict__ base,
                                                     uint32_t *__restrict__ order)
{
    __shared__ uint32_t pos[kMaxFlows];
    const int lane = threadIdx.x;
    const uint32_t *row = table + (int64_t)blockIdx.x * nflows;
    for (int f = lane; f < nflows; f += 64) pos[f] = base[f] + row[f];
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1;   // lanes below this one
    const int64_t p0 = (int64_t)blockIdx.x * tile, p1 = p0 + tile < np ? p0 + tile : np;
    uint32_t fn = p0 + lane < p1 ? (uint32_t)flow_of[p0 + lane] : ~0u;
    for (int64_t g = p0; g < p1; g += 64) {
        const int64_t p = g + lane;
        const uint32_t f = fn;
        fn = p + 64 < p1 ? (uint32_t)flow_of[p + 64] : ~0u;   // the next group's flows in flight while this one is ranked
        const bool routed = f < (uint32_t)nflows;              // (a lane past the end holds ~0u: no flow)
        // the lanes of this lane's flow: those that agree with it in every bit of the flow number.  `bits` ballots (nflows <= 2^bits)
        // that do not depend on one another, instead of a pass per distinct flow of the group, each waiting for the one before
        uint64_t same = __ballot(routed);
        for (int b = 0; b < bits; b++) {
            const uint64_t one = __ballot((f >> b) & 1u);
            same &= ((f >> b) & 1u) ? one : ~one;
        }
        const uint32_t rank = (uint32_t)__popcll(same & lt), lanes = (uint32_t)__popcll(same);
        uint32_t start = 0;
        if (routed) {
            start = pos[f];
            if ((int64_t)start + rank < np) order[start + rank] = (uint32_t)p;   // (always, unless flow_of changed under the call)
        }
        if (routed && rank == 0) pos[f] = start + lanes;   // behind the read above: a wavefront's LDS accesses keep their order
    }
}

// the partition's tiling for P packets: at most kDemuxMaxTiles tiles of a multiple of 64 packets
inline void demux_tiling(int64_t P, int64_t &tile, int64_t &tiles)
{
    tile = std::max<int64_t>(kDemuxMinTile, ((P + kDemuxMaxTiles - 1) / kDemuxMaxTiles + 63) / 64 * 64);
    tiles = (P + tile - 1) / tile;
}

// the context's table for P packets of nflows flows, with room for the nflows + 1 bases behind it
inline int demux_reserve(ldpc_amd_ctx *ctx, int64_t P, int nflows)
{
    int64_t tile, tiles;
    demux_tiling(P, tile, tiles);
    return ldpc_amd::scratch_reserve(ctx, ctx->demux_tab, sizeof(uint32_t) * ((size_t)tiles * (size_t)nflows + (size_t)nflows + 1));
}

// (i) - (iii) on the context's stream, P > 0; base: [nflows + 1] device words; in: the flows' records or null.  demux_reserve came first.
template <typename Rec>
inline int demux_launch(ldpc_amd_ctx *ctx, const int32_t *flow_of, int64_t P, int nflows, uint32_t *base, Rec *in, uint32_t *order)
{
    int64_t tile, tiles;
    demux_tiling(P, tile, tiles);
    uint32_t *table = (uint32_t *)ctx->demux_tab.p;
    hipLaunchKernelGGL(fec_demux_count, dim3((unsigned)tiles), dim3(kDemuxThreads), 0, ctx->stream, flow_of, P, tile, nflows, table);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fec_demux_tiles, dim3((unsigned)((nflows + 63) / 64)), dim3(64, kDemuxChunks), 0, ctx->stream, table, (int)tiles, nflows, base);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fec_demux_bases<Rec>, dim3(1), dim3(64), 0, ctx->stream, base, nflows, in);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    int bits = 0;
    while ((1 << bits) < nflows) bits++;
    hipLaunchKernelGGL(fec_demux_place, dim3((unsigned)tiles), dim3(64), 0, ctx->stream, flow_of, P, tile, nflows, bits, (const uint32_t *)table,
                       (const uint32_t *)base, order);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    ctx->demux_tile = tile;
    ctx->demux_tiles = tiles;
    return LDPC_AMD_OK;
}

}  // namespace
#endif /* LDPC_ERASURE_AMD_FLOWS_DEMUX_DEV_H */
