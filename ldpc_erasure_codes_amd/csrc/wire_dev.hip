// wire_dev.hip -- device-resident FEC wire path (include/ldpc_erasure_amd_wire_dev.h): the packetiser and the two-buffer
// reassembler of csrc/wire.cpp for data that is already in GPU memory, byte for byte the host functions' output.
//
// Reference: OpenCL/device/ldpc_erasure_encoder_VITA_in_UDP_out.cl:84-129,168-211 (headers written in a kernel) and
// OpenCL/device/ldpc_erasure_decoder_with_reordering_logic.cl:44-141,214-243 (reassembly in a kernel in front of the decoder).
//
// The reassembler's rule depends only on the headers, never on the payloads, so one push_many call is split into a PLAN and a
// DATA MOVEMENT:
//   (a) fec_rx_headers   every packet's header -> one dense u32, block << 16 | symbol                         (parallel)
//   (b) fec_rx_scan      one wavefront replays ldpc_amd_fec_rx_push over the dense headers, 64 packets per step; per packet
//                        it writes a destination (the SERIAL of the block it went to, or -1 = dropped), per close the wire
//                        block number, and at the end the state.  The host reads the state back (the call returns it).
//   (c) fec_rx_winners   atomicMax of the packet index into a [(closes + 2)][n] table: the host copies duplicates in stream
//                        order, so the last one is what stays                                                   (parallel)
//   (d) fec_rx_move<1>   closed blocks -> sym_batch / erased_batch                                              (parallel)
//   (e) fec_rx_move<0>   the two blocks still open -> the two staging planes                                    (parallel)
// Serials: the block that is current when the call starts is serial 0, the next one serial 1, and the t-th close of the call
// (0-based) opens serial t + 2.  Blocks close in the order they were opened (cur closes, next becomes cur), so serial s is closed
// slot s of the call when s < closes; serials closes and closes + 1 are the blocks still open at the end (current, next).  A
// serial s lives in staging buffer (cb + s) & 1, cb = the current block's buffer at the start of the call (the buffers rotate
// on every close, :241).  Serials 0 and 1 were carried in from earlier calls: their staging planes hold what those calls
// received; every other serial starts erased.  (d) reads the staging planes of carried blocks that close; (e) rewrites the
// plane of serial s >= 2, which is the plane of serial s - 2 -- a block (d) may read -- so (e) is a launch after (d).
// The host code every device receiver needs -- the argument check and the decode tail of the decode calls, the upload of a batch
// flush's plane numbers -- is csrc/rx_host.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "rx_flows_host.h"   // the multi-flow call skeleton; with it rx_host.h and flows_demux_dev.h
#include "fec_header_dev.h"
#include "../../include/ldpc_erasure_amd_wire_dev.h"
#include "../../include/ldpc_erasure_amd_sender.h"
#include "../../include/ldpc_erasure_amd_sender_flows.h"
#include "../../include/ldpc_erasure_amd_interleave.h"
#include "../../include/ldpc_erasure_amd_interleave_flows.h"
#include "../../include/ldpc_erasure_amd_rs_wire.h"
#include "../../include/ldpc_erasure_amd_receiver.h"
#include "../../include/ldpc_erasure_amd_flows.h"
#include "../../include/ldpc_erasure_amd_flows_mixed.h"
#include "../../include/ldpc_erasure_amd_flows_flush.h"

using namespace ldpc_amd;

namespace {

constexpr int kHdr = LDPC_AMD_FEC_HEADER_BYTES;
constexpr int kThreads = 256;
constexpr int kScanPrefetch = 16;   // groups of 64 dense headers a scan lane holds in flight ahead of the one it works on

// Result record of one scan, read back by the host (32-bit words, then the closed blocks' wire numbers).
enum : int { R_CUR, R_NEXT, R_CCNT, R_NCNT, R_CLOSES, R_ERR, R_CONSUMED_LO, R_CONSUMED_HI, R_DROPPED_LO, R_DROPPED_HI, R_WORDS = 16 };

constexpr size_t kSenderScratchMax = (size_t)256 << 20;   // composed sender: codewords of one chunk of frames

inline unsigned grid_for(int64_t items)
{
    const int64_t b = (items + kThreads - 1) / kThreads;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(b, (int64_t)1 << 20));   // grid-stride loops cover the rest
}

// ---- packetiser ------------------------------------------------------------------------------------------------------
// Tuned path (S % 16 == 0, frames 16-byte and packets 8-byte aligned): one work item per 16-byte piece of a row; the piece is read
// as one 16-byte load and written as two 8-byte stores (the payload sits at offset 8 of a packet of stride 8 + S); the item of
// piece 0 also writes the header.
__global__ __launch_bounds__(kThreads) void fec_packetize_v16(const uint4 *__restrict__ frames, int64_t rows, int n, int q,
                                                             unsigned fec_class, unsigned block0, uint8_t *__restrict__ packets)
{
    const int64_t total = rows * q, plen = (int64_t)q * 16 + kHdr;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int64_t r = t / q;
        const int c = (int)(t - r * q);
        const uint4 v = frames[t];
        uint2 *dst = reinterpret_cast<uint2 *>(packets + r * plen + kHdr + (int64_t)c * 16);
        dst[0] = make_uint2(v.x, v.y);
        dst[1] = make_uint2(v.z, v.w);
        if (c == 0) {
            const int64_t f = r / n;
            *reinterpret_cast<uint64_t *>(packets + r * plen) = fec_header(fec_class, block0 + (unsigned)f, (unsigned)(r - f * n));
        }
    }
}

// Any S: one work item per output byte.
__global__ __launch_bounds__(kThreads) void fec_packetize_bytes(const uint8_t *__restrict__ frames, int64_t rows, int n, int S,
                                                               unsigned fec_class, unsigned block0, uint8_t *__restrict__ packets)
{
    const int64_t plen = (int64_t)S + kHdr, total = rows * plen;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int64_t r = t / plen;
        const int o = (int)(t - r * plen);
        uint8_t b;
        if (o < kHdr) {
            const int64_t f = r / n;
            b = (uint8_t)(fec_header(fec_class, block0 + (unsigned)f, (unsigned)(r - f * n)) >> (8 * o));   // little endian
        } else {
            b = frames[r * S + (o - kHdr)];
        }
        packets[t] = b;
    }
}

// ---- multi-flow sender: the composed path's packetisers and flow_of (include/ldpc_erasure_amd_sender_flows.h) -----------------
// One descriptor per frame: row j of the frame is packet first + j * stride, its header class = hdr >> 8, block = hdr & 0xff.  The
// same 16 bytes the descriptor form of the packet encoder reads (ScatterArgs::flow_desc in kernels.hip).
struct TxFrameDesc {
    uint64_t first;
    uint32_t stride;
    uint32_t hdr;
};
static_assert(sizeof(TxFrameDesc) == 16, "the encoder reads a descriptor as one uint4");

// fec_packetize_v16 with the packet of a row taken from its frame's descriptor.  frames: [nf][n][16 q] codewords of the frames
// desc[0 .. nf-1] (the caller passes the table at the chunk's first frame).
__global__ __launch_bounds__(kThreads) void fec_packetize_flows_v16(const uint4 *__restrict__ frames, int64_t rows, int n, int q,
                                                                   const TxFrameDesc *__restrict__ desc, uint8_t *__restrict__ packets)
{
    const int64_t total = rows * q, plen = (int64_t)q * 16 + kHdr;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int64_t r = t / q;
        const int c = (int)(t - r * q);
        const int64_t f = r / n;
        const unsigned j = (unsigned)(r - f * n);
        const TxFrameDesc d = desc[f];
        uint8_t *pk = packets + (int64_t)(d.first + (uint64_t)j * d.stride) * plen;
        const uint4 v = frames[t];
        uint2 *dst = reinterpret_cast<uint2 *>(pk + kHdr + (int64_t)c * 16);
        dst[0] = make_uint2(v.x, v.y);
        dst[1] = make_uint2(v.z, v.w);
        if (c == 0) *reinterpret_cast<uint64_t *>(pk) = fec_header(d.hdr >> 8, d.hdr, j);
    }
}

// fec_packetize_bytes likewise: any S and alignment (S = 1, the word form, a packet array that is not 8-byte aligned).
__global__ __launch_bounds__(kThreads) void fec_packetize_flows_bytes(const uint8_t *__restrict__ frames, int64_t rows, int n, int S,
                                                                     const TxFrameDesc *__restrict__ desc, uint8_t *__restrict__ packets)
{
    const int64_t plen = (int64_t)S + kHdr, total = rows * plen;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int64_t r = t / plen;
        const int o = (int)(t - r * plen);
        const int64_t f = r / n;
        const unsigned j = (unsigned)(r - f * n);
        const TxFrameDesc d = desc[f];
        uint8_t b;
        if (o < kHdr) b = (uint8_t)(fec_header(d.hdr >> 8, d.hdr, j) >> (8 * o));   // little endian
        else b = frames[r * S + (o - kHdr)];
        packets[(int64_t)(d.first + (uint64_t)j * d.stride) * plen + o] = b;
    }
}

// flow_of[p] = the flow of packet p, one 4-byte store per packet: work item (frame, row) stores its frame's flow at the row's packet.
__global__ __launch_bounds__(kThreads) void fec_tx_flow_of(const TxFrameDesc *__restrict__ desc, const int32_t *__restrict__ frame_flow,
                                                          int64_t rows, int n, int32_t *__restrict__ flow_of)
{
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kThreads) {
        const int64_t f = r / n;
        const unsigned j = (unsigned)(r - f * n);
        const TxFrameDesc d = desc[f];
        flow_of[d.first + (uint64_t)j * d.stride] = frame_flow[f];
    }
}

// ---- (a) headers -----------------------------------------------------------------------------------------------------
// Only the first 32-bit half of the header is read, as the host's ldpc_amd_fec_header_unpack does (symbol = bytes 0-1,
// block = byte 2).
template <bool ALIGNED4>
__global__ __launch_bounds__(kThreads) void fec_rx_headers(const uint8_t *__restrict__ packets, int64_t np, int plen,
                                                          uint32_t *__restrict__ dense)
{
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < np; p += (int64_t)gridDim.x * kThreads) {
        const uint8_t *h = packets + p * plen;
        uint32_t w;
        if (ALIGNED4) w = *reinterpret_cast<const uint32_t *>(h) & 0x00ffffffu;
        else w = (uint32_t)h[0] | (uint32_t)h[1] << 8 | (uint32_t)h[2] << 16;
        dense[p] = w;
    }
}

// ---- (b) the plan scan -----------------------------------------------------------------------------------------------
// :139 -- kd = k + round(0.8 (n-k)), km = k + round(0.2 (n-k))
__device__ __forceinline__ bool close_rule(int c, int x, int n, int kd, int km)
{
    return c == n || (c > kd && x > 10) || (c > km && x > 100);
}

// One wavefront.  Every value but the lane's own packet is wave-uniform.  For a group of 64 packets from lane `start` on:
//   isC / isN    this lane's packet goes to the current / next block (symbol < n and the block number matches);
//   c_l, x_l     the counts after this lane's packet: the counts before the group + the ballots' inclusive prefix popcounts;
//   bz           the lanes where :139 holds after their packet; the first of them (ffs) is where the host closes.
// Exactness: the host's state after packet l depends on the packets before it only through (cur, next, ccnt, ncnt), and as
// long as no close happens cur / next are fixed, so each count after packet l is exactly the count before the group plus the
// matching packets among start..l -- the prefix popcount.  The condition after packet l is a function of those two counts
// alone, so the first lane where it holds is the first packet after which the host closes, and every lane up to it is
// assigned as the host assigns it.  The close rotates the state exactly as close_current does, and the lanes after it are
// evaluated again with the new state.  A dropped packet changes no count but is still a point where :139 is tested, as on the
// host (a block whose count reached n through the next block's packets closes at the packet after the rotation).
// The loop is bounded: every iteration assigns at least one packet or ends its group, so a call takes at most
// npackets + closes + groups iterations; a cap on that reports R_ERR instead of spinning on a bad stream.
// The body is one function: fec_rx_scan runs it on a call's packets, fec_rx_scan_flows on the segment of one flow per workgroup.
__device__ __forceinline__ void fec_rx_scan_body(const uint32_t *__restrict__ dense, int64_t np, int n, int kd, int km,
                                                 int max_blocks, int cur, int nxt, int ccnt, int ncnt,
                                                 int32_t *__restrict__ dest, int32_t *__restrict__ res)
{
    const int lane = threadIdx.x;
    const uint64_t le = (lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1);   // lanes <= this one
    int closes = 0, err = 0;
    int64_t dropped = 0, consumed = np, iters = 0;
    const int64_t iter_cap = np + (int64_t)max_blocks + (np + 63) / 64 + 1;
    bool done = false;
    uint32_t nb[kScanPrefetch];
#pragma unroll
    for (int u = 0; u < kScanPrefetch; u++) {
        const int64_t p = (int64_t)u * 64 + lane;
        nb[u] = p < np ? dense[p] : 0u;
    }
    for (int64_t base0 = 0; base0 < np && !done; base0 += 64 * kScanPrefetch) {
        uint32_t hb[kScanPrefetch];
#pragma unroll
        for (int u = 0; u < kScanPrefetch; u++) hb[u] = nb[u];
#pragma unroll
        for (int u = 0; u < kScanPrefetch; u++) {   // headers of the next chunk in flight while this one is scanned
            const int64_t p = base0 + (int64_t)(kScanPrefetch + u) * 64 + lane;
            nb[u] = p < np ? dense[p] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kScanPrefetch; u++) {
            const int64_t base = base0 + (int64_t)u * 64;
            if (done || base >= np) continue;   // (not break: the loop must unroll to keep hb[] in registers)
            const int64_t p = base + lane;
            const bool valid = p < np;
            const int blk = (int)(hb[u] >> 16), sym = (int)(hb[u] & 0xffffu);
            if (cur < 0) {   // :88-91, the first packet of the stream -- before its symbol check
                cur = __shfl(blk, 0);
                nxt = (cur + 1) & 0xff;
            }
            int d = -1;
            int start = 0;
            for (;;) {
                if (++iters > iter_cap) { err = 1; done = true; consumed = base; break; }
                const bool live = valid && lane >= start;
                const bool ok = live && sym < n;
                const bool isC = ok && blk == cur, isN = ok && blk == nxt;
                const uint64_t bc = __ballot(isC), bn = __ballot(isN);
                const int c = ccnt + __popcll(bc & le), x = ncnt + __popcll(bn & le);
                const uint64_t bz = __ballot(live && close_rule(c, x, n, kd, km));
                const uint64_t upto = bz ? ((bz & (0ull - bz)) << 1) - 1 : ~0ull;   // lanes up to the first close (all if none)
                const bool mine = live && ((upto >> lane) & 1);
                if (mine) d = isC ? closes : (isN ? closes + 1 : -1);
                dropped += __popcll(__ballot(mine && !isC && !isN));
                ccnt += __popcll(bc & upto);
                ncnt += __popcll(bn & upto);
                if (!bz) break;
                const int L = __ffsll((long long)bz) - 1;
                if (lane == 0) res[R_WORDS + closes] = cur;   // close_current (:214-243)
                closes++;
                cur = nxt;
                nxt = (nxt + 1) & 0xff;
                ccnt = ncnt;
                ncnt = 0;
                if (closes == max_blocks) { consumed = base + L + 1; done = true; break; }
                start = L + 1;
                if (start >= 64) break;
            }
            if (valid) dest[p] = d;
        }
    }
    if (lane == 0) {
        res[R_CUR] = cur; res[R_NEXT] = nxt; res[R_CCNT] = ccnt; res[R_NCNT] = ncnt; res[R_CLOSES] = closes; res[R_ERR] = err;
        res[R_CONSUMED_LO] = (int32_t)(uint32_t)consumed; res[R_CONSUMED_HI] = (int32_t)(consumed >> 32);
        res[R_DROPPED_LO] = (int32_t)(uint32_t)dropped; res[R_DROPPED_HI] = (int32_t)(dropped >> 32);
    }
}

__global__ __launch_bounds__(64) void fec_rx_scan(const uint32_t *__restrict__ dense, int64_t np, int n, int kd, int km,
                                                 int max_blocks, int cur, int nxt, int ccnt, int ncnt,
                                                 int32_t *__restrict__ dest, int32_t *__restrict__ res)
{
    fec_rx_scan_body(dense, np, n, kd, km, max_blocks, cur, nxt, ccnt, ncnt, dest, res);
}

// ---- (c) last writer wins ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void fec_rx_winners(const uint32_t *__restrict__ dense, const int32_t *__restrict__ dest,
                                                          int64_t consumed, int n, int32_t *__restrict__ win)
{
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < consumed; p += (int64_t)gridDim.x * kThreads) {
        const int s = dest[p];
        if (s >= 0) atomicMax(&win[(int64_t)s * n + (dense[p] & 0xffffu)], (int32_t)p);   // dest >= 0 only for symbol < n
    }
}

// ---- (d) gather into the closed slots, (e) staging planes ------------------------------------------------------------
struct MoveArgs {
    const uint8_t *packets;
    int64_t plen;
    const int32_t *win;   // [(closes + 2)][n]
    uint8_t *stage_sym;   // [2][n][S]
    uint8_t *stage_er;    // [2][n]
    uint8_t *sym_out;     // gather: [count][n][S], the closed slots first .. first + count - 1
    uint8_t *er_out;      // gather: [count][n]
    int n, S, cb, closes;
    int first, count;     // gather: the slots of this launch (the composed receiver gathers chunk by chunk)
};

// Row r of the gather (slot j = first + r / n, symbol i): the last packet that went there, else -- for a block carried in from an earlier
// call -- its staging row, else zero and erased (the decoder kernels' assumption 2).
// Row r of the staging update (serial s = closes + r / n): the last packet, else for a block opened in this call zero and erased;
// a carried block keeps its staging row.
template <bool GATHER, bool V16>
__global__ __launch_bounds__(kThreads) void fec_rx_move(MoveArgs a)
{
    const int q = V16 ? a.S / 16 : a.S;   // 16-byte pieces or bytes of a row
    const int64_t rows = GATHER ? (int64_t)a.count * a.n : 2 * (int64_t)a.n;
    const int64_t total = rows * q;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int64_t r = t / q;
        const int c = (int)(t - r * q);
        const int s = (int)(r / a.n) + (GATHER ? a.first : a.closes);   // serial of the block
        const int i = (int)(r - (int64_t)(r / a.n) * a.n);
        const int w = a.win[(int64_t)s * a.n + i];
        const int b = (a.cb + s) & 1;
        const bool carried = s < 2;
        const int64_t srow = ((int64_t)b * a.n + i) * a.S;   // the block's staging row
        uint8_t *dst = GATHER ? a.sym_out + r * a.S : a.stage_sym + srow;
        if (!GATHER && w < 0 && carried) continue;
        if (V16) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (w >= 0) {
                const uint2 *src = reinterpret_cast<const uint2 *>(a.packets + (int64_t)w * a.plen + kHdr + (int64_t)c * 16);
                const uint2 lo = src[0], hi = src[1];
                v = make_uint4(lo.x, lo.y, hi.x, hi.y);
            } else if (carried) {
                v = *reinterpret_cast<const uint4 *>(a.stage_sym + srow + (int64_t)c * 16);
            }
            *reinterpret_cast<uint4 *>(dst + (int64_t)c * 16) = v;
        } else {
            uint8_t v = 0;
            if (w >= 0) v = a.packets[(int64_t)w * a.plen + kHdr + c];
            else if (carried) v = a.stage_sym[srow + c];
            dst[c] = v;
        }
        if (c == 0) {
            const uint8_t e = w >= 0 ? 0 : (carried ? a.stage_er[(int64_t)b * a.n + i] : 1);
            if (GATHER) a.er_out[r] = e;
            else a.stage_er[(int64_t)b * a.n + i] = e;
        }
    }
}

// ---- (d') the fused receiver: instead of the gather, WHERE every row of the closed slots lies --------------------------------------
// The rule of the gather's row r, as a word the packets-in decoder follows (internal.h, PacketRows), and the erasure flag the
// gather would have written.  A carried block's symbol that no packet of this call brought keeps what its staging plane holds: the
// row if it was received by an earlier call, else erased.  (An erased row's bytes are never read: the decoder zero-fills or solves it.)
__global__ __launch_bounds__(kThreads) void fec_rx_sources(const int32_t *__restrict__ win, const uint8_t *__restrict__ stage_er, int n,
                                                          int cb, int closes, uint32_t *__restrict__ src, uint8_t *__restrict__ er)
{
    const int64_t total = (int64_t)closes * n;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < total; r += (int64_t)gridDim.x * kThreads) {
        const int s = (int)(r / n);
        const int i = (int)(r - (int64_t)s * n);
        const int w = win[r];
        const int row = ((cb + s) & 1) * n + i;   // the block's staging row
        uint32_t word = kRowErased;
        if (w >= 0) word = (uint32_t)w;
        else if (s < 2 && stage_er[row] == 0) word = kRowStaged | (uint32_t)row;
        src[r] = word;
        er[r] = word == kRowErased ? 1 : 0;
    }
}

// ---- the multi-flow receiver (include/ldpc_erasure_amd_flows.h) ---------------------------------------------------------
// The same five steps for nflows streams whose packets lie in one array, flow f's in begin .. begin + len - 1.  (a) is flow-agnostic.
// (b) runs fec_rx_scan's body once per flow, one wavefront each: serials, and with them `dest`, are LOCAL to the flow.  The host
// reads every flow's result record back in one copy, takes the prefix sum of the closes -- flow f's closed blocks are the GLOBAL
// slots base[f] .. base[f] + closes[f] - 1, T slots in all -- and hands the kernels behind it one record per flow (FlowTab).
// The winners' table is [(T + 2 nflows)][n]: the closed slots first, then the two open blocks of flow 0, of flow 1, ...
// The staging planes are [nflows][2][n][S] / [nflows][2][n]: serial s of flow f lives in plane f * 2 + ((cb[f] + s) & 1), so row i
// of it is staging row (f * 2 + b) * n + i of ONE base -- the row-source word of the packets-in decoder (PacketRows) needs no more.
struct FlowIn {    // written by the host before the plan
    int64_t begin, len;   // the flow's segment of the packet array
    int cur, nxt, ccnt, ncnt;
};
struct FlowTab {   // written by the host behind the plan
    int64_t begin, used;   // the packets the flow consumed: begin .. begin + used - 1
    int base, closes, cb, pad;
};

// (b) grid: nflows workgroups of one wavefront; res: [nflows][R_WORDS + max_blocks]
__global__ __launch_bounds__(64) void fec_rx_scan_flows(const uint32_t *__restrict__ dense, const FlowIn *__restrict__ in, int n, int kd,
                                                       int km, int max_blocks, int32_t *__restrict__ dest, int32_t *__restrict__ res)
{
    const FlowIn f = in[blockIdx.x];
    fec_rx_scan_body(dense + f.begin, f.len, n, kd, km, max_blocks, f.cur, f.nxt, f.ccnt, f.ncnt, dest + f.begin,
                     res + (int64_t)blockIdx.x * (R_WORDS + max_blocks));
}

// slot -> flow, [T]: one workgroup per flow
__global__ __launch_bounds__(64) void fec_rx_flow_slots(const FlowTab *__restrict__ tab, int32_t *__restrict__ slot_flow)
{
    const FlowTab f = tab[blockIdx.x];
    for (int s = threadIdx.x; s < f.closes; s += 64) slot_flow[f.base + s] = (int)blockIdx.x;
}

// (c) grid: (x, nflows); over each flow's consumed prefix only.  The packet index is the global one: the last copy wins, as on the host.
__global__ __launch_bounds__(kThreads) void fec_rx_winners_flows(const uint32_t *__restrict__ dense, const int32_t *__restrict__ dest,
                                                                const FlowTab *__restrict__ tab, int n, int T, int32_t *__restrict__ win)
{
    const FlowTab f = tab[blockIdx.y];
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < f.used; q += (int64_t)gridDim.x * kThreads) {
        const int64_t p = f.begin + q;
        const int s = dest[p];
        if (s < 0) continue;
        const int64_t row = s < f.closes ? (int64_t)f.base + s : (int64_t)T + 2 * (int64_t)blockIdx.y + (s - f.closes);
        atomicMax(&win[row * n + (dense[p] & 0xffffu)], (int32_t)p);
    }
}

struct FlowMoveArgs {
    const uint8_t *packets;
    int64_t plen;
    const int32_t *win;         // [(T + 2 nflows)][n]
    const FlowTab *tab;         // [nflows]
    const int32_t *slot_flow;   // [T]
    uint8_t *stage_sym;         // [nflows][2][n][S]
    uint8_t *stage_er;          // [nflows][2][n]
    uint8_t *sym_out;           // gather: [count][n][S], the closed slots first .. first + count - 1
    uint8_t *er_out;            // gather: [count][n]
    int n, S, T, nflows;
    int first, count;
};

// fec_rx_move for all flows.  Gather: row r is symbol i of global slot j = first + r / n, which is serial j - base[f] of flow f =
// slot_flow[j].  Staging update: row r is symbol i of open block o = 0, 1 of flow f = r / (2 n), its serial closes[f] + o.
template <bool GATHER, bool V16>
__global__ __launch_bounds__(kThreads) void fec_rx_move_flows(FlowMoveArgs a)
{
    const int q = V16 ? a.S / 16 : a.S;
    const int64_t rows = GATHER ? (int64_t)a.count * a.n : 2 * (int64_t)a.nflows * a.n;
    const int64_t total = rows * q;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int64_t r = t / q;
        const int c = (int)(t - r * q);
        const int64_t blk = r / a.n;
        const int i = (int)(r - blk * a.n);
        int f, s;
        int64_t wrow;
        if (GATHER) {
            wrow = a.first + blk;
            f = a.slot_flow[wrow];
            s = (int)wrow - a.tab[f].base;
        } else {
            f = (int)(blk >> 1);
            s = a.tab[f].closes + (int)(blk & 1);
            wrow = (int64_t)a.T + blk;
        }
        const int w = a.win[wrow * a.n + i];
        const int b = (a.tab[f].cb + s) & 1;
        const bool carried = s < 2;
        const int64_t erow = ((int64_t)f * 2 + b) * a.n + i;   // the block's staging row
        const int64_t srow = erow * a.S;
        uint8_t *dst = GATHER ? a.sym_out + r * a.S : a.stage_sym + srow;
        if (!GATHER && w < 0 && carried) continue;
        if (V16) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (w >= 0) {
                const uint2 *src = reinterpret_cast<const uint2 *>(a.packets + (int64_t)w * a.plen + kHdr + (int64_t)c * 16);
                const uint2 lo = src[0], hi = src[1];
                v = make_uint4(lo.x, lo.y, hi.x, hi.y);
            } else if (carried) {
                v = *reinterpret_cast<const uint4 *>(a.stage_sym + srow + (int64_t)c * 16);
            }
            *reinterpret_cast<uint4 *>(dst + (int64_t)c * 16) = v;
        } else {
            uint8_t v = 0;
            if (w >= 0) v = a.packets[(int64_t)w * a.plen + kHdr + c];
            else if (carried) v = a.stage_sym[srow + c];
            dst[c] = v;
        }
        if (c == 0) {
            const uint8_t e = w >= 0 ? 0 : (carried ? a.stage_er[erow] : 1);
            if (GATHER) a.er_out[r] = e;
            else a.stage_er[erow] = e;
        }
    }
}

// fec_rx_sources for all flows: the row-source words and flags of the T closed slots
__global__ __launch_bounds__(kThreads) void fec_rx_sources_flows(const int32_t *__restrict__ win, const uint8_t *__restrict__ stage_er,
                                                                const FlowTab *__restrict__ tab, const int32_t *__restrict__ slot_flow, int n,
                                                                int T, uint32_t *__restrict__ src, uint8_t *__restrict__ er)
{
    const int64_t total = (int64_t)T * n;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < total; r += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(r / n);
        const int i = (int)(r - (int64_t)j * n);
        const int f = slot_flow[j];
        const int s = j - tab[f].base;
        const int w = win[r];
        const int64_t row = ((int64_t)f * 2 + ((tab[f].cb + s) & 1)) * n + i;   // the block's staging row, < 2^31 - 2 (create)
        uint32_t word = kRowErased;
        if (w >= 0) word = (uint32_t)w;
        else if (s < 2 && stage_er[row] == 0) word = kRowStaged | (uint32_t)row;
        src[r] = word;
        er[r] = word == kRowErased ? 1 : 0;
    }
}

// ---- interleaved packets (include/ldpc_erasure_amd_flows_mixed.h) ----------------------------------------------------------
// The packets of a call lie in arrival order and flow_of[p] names the flow of packet p.  Nothing behind the plan needs a flow's
// packets side by side -- the plan reads the dense header words, the gather and the decoder address a payload by packet index -- so
// only the packet INDICES are partitioned by flow: order[q] = the q-th packet when the routed packets are listed flow by flow, each
// flow in arrival order.  The plan then runs on positions q (dense[q] = header of packets[order[q]], flow f's segment is
// base[f] .. base[f+1]-1), and one pass over the winners' table turns the winning positions back into packet indices.
// The partition itself -- fec_demux_count / _tiles / _bases / _place and their launcher -- is csrc/flows_demux_dev.h, shared with the
// windowed flows of rx_window_flows_dev.hip.

// (a) on the permutation: dense[q] = the header word of packet order[q], for the *routed positions q
template <bool ALIGNED4>
__global__ __launch_bounds__(kThreads) void fec_rx_headers_idx(const uint8_t *__restrict__ packets, const uint32_t *__restrict__ order,
                                                              const uint32_t *__restrict__ routed, int plen, uint32_t *__restrict__ dense)
{
    const int64_t nq = *routed;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < nq; q += (int64_t)gridDim.x * kThreads) {
        const uint8_t *h = packets + (int64_t)order[q] * plen;
        uint32_t w;
        if (ALIGNED4) w = *reinterpret_cast<const uint32_t *>(h) & 0x00ffffffu;
        else w = (uint32_t)h[0] | (uint32_t)h[1] << 8 | (uint32_t)h[2] << 16;
        dense[q] = w;
    }
}

// (c) left the winning POSITION in every cell of the winners' table: the packet index instead, which is what everything behind reads
__global__ __launch_bounds__(kThreads) void fec_rx_win_order(int32_t *__restrict__ win, int64_t cells, const uint32_t *__restrict__ order)
{
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < cells; r += (int64_t)gridDim.x * kThreads) {
        const int32_t q = win[r];
        if (q >= 0) win[r] = (int32_t)order[q];   // a packet index is below 2^31
    }
}

// left[p] = 1 for the packets behind a flow's consumed prefix (the caller has zeroed left); grid: (x, nflows)
__global__ __launch_bounds__(kThreads) void fec_rx_left_flows(const FlowTab *__restrict__ tab, const FlowIn *__restrict__ in,
                                                             const uint32_t *__restrict__ order, uint8_t *__restrict__ left)
{
    const FlowTab f = tab[blockIdx.y];
    const int64_t len = in[blockIdx.y].len;
    for (int64_t q = f.used + (int64_t)blockIdx.x * kThreads + threadIdx.x; q < len; q += (int64_t)gridDim.x * kThreads)
        left[order[f.begin + q]] = 1;
}

// ---- the batch flush (include/ldpc_erasure_amd_flows_flush.h) -----------------------------------------------------------------
// Every block a flush closes lies complete in ONE staging plane, and which plane that is follows from the host's mirror of the
// flows' states: the host writes one word per closed slot, desc[j] = the plane f * 2 + b of slot j, and the three kernels below take
// everything else from it.  No packet array, no winners' table, no scan.

// fec_rx_sources_flows for blocks that are all staged: the flag the gather would have copied, and the word of the row -- row
// desc[j] * n + i of the planes' one base (below 2^31 - 2: create) -- or erased.
__global__ __launch_bounds__(kThreads) void fec_rx_flush_sources(const int32_t *__restrict__ desc, const uint8_t *__restrict__ stage_er, int n,
                                                                int T, uint32_t *__restrict__ src, uint8_t *__restrict__ er)
{
    const int64_t total = (int64_t)T * n;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < total; r += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(r / n);
        const int i = (int)(r - (int64_t)j * n);
        const int64_t row = (int64_t)desc[j] * n + i;
        const uint8_t e = stage_er[row];
        src[r] = e ? kRowErased : (kRowStaged | (uint32_t)row);
        er[r] = e;
    }
}

// Plane -> dense slot for the slots first .. first + count - 1, grid (x, count): the rows (an erased row of a plane is zero by
// construction) and the flags.  A plane is n * S contiguous bytes, copied in pieces of W bytes (16, 4, 1; W divides S, and S >= W, so
// a plane has at least n pieces: piece u < n also copies flag u).  sym_out / er_out: [count][n][S] / [count][n], er_out may be null.
template <int W>
__global__ __launch_bounds__(kThreads) void fec_rx_flush_gather(const int32_t *__restrict__ desc, const uint8_t *__restrict__ stage_sym,
                                                               const uint8_t *__restrict__ stage_er, int n, int S, int first,
                                                               uint8_t *__restrict__ sym_out, uint8_t *__restrict__ er_out)
{
    const int64_t upp = (int64_t)n * S / W;   // pieces of a plane
    const int64_t s = blockIdx.y, plane = desc[first + s];
    const uint8_t *from = stage_sym + plane * upp * W;
    uint8_t *to = sym_out + s * upp * W;
    for (int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x; u < upp; u += (int64_t)gridDim.x * kThreads) {
        if (W == 16) reinterpret_cast<uint4 *>(to)[u] = reinterpret_cast<const uint4 *>(from)[u];
        else if (W == 4) reinterpret_cast<uint32_t *>(to)[u] = reinterpret_cast<const uint32_t *>(from)[u];
        else to[u] = from[u];
        if (er_out && u < n) er_out[s * n + u] = stage_er[plane * n + u];
    }
}

// The planes of the T closed slots back to symbols 0 and flags 1 (csrc/wire.cpp: close_current), grid (x, T).  W as above.
template <int W>
__global__ __launch_bounds__(kThreads) void fec_rx_flush_reset(const int32_t *__restrict__ desc, uint8_t *__restrict__ stage_sym,
                                                              uint8_t *__restrict__ stage_er, int n, int S)
{
    const int64_t upp = (int64_t)n * S / W;
    const int64_t plane = desc[blockIdx.y];
    uint8_t *to = stage_sym + plane * upp * W;
    for (int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x; u < upp; u += (int64_t)gridDim.x * kThreads) {
        if (W == 16) reinterpret_cast<uint4 *>(to)[u] = make_uint4(0, 0, 0, 0);
        else if (W == 4) reinterpret_cast<uint32_t *>(to)[u] = 0u;
        else to[u] = 0;
        if (u < n) stage_er[plane * n + u] = 1;
    }
}

}  // namespace

struct ldpc_amd_fec_rx_dev {
    ldpc_amd_ctx *ctx = nullptr;
    int n = 0, k = 0, S = 0, kd = 0, km = 0;
    // host mirror of the receiver's state (csrc/wire.cpp's ldpc_amd_fec_rx); cb: staging buffer of the current block
    int cur = -1, next = -1, ccnt = 0, ncnt = 0, cb = 0;
    int64_t dropped = 0;
    uint8_t *stage_sym = nullptr;   // [2][n][S]
    uint8_t *stage_er = nullptr;    // [2][n]
    Scratch dense, dest, win, res;  // per-call scratch, grown on demand
    int32_t *res_host = nullptr;    // pinned copy of res
    size_t res_host_cap = 0;
};

namespace {

// ---- the packet senders' common part (ldpc_amd_fec_encode_packets_dev, _flows_dev, _ilv_dev, _flows_ilv_dev and
// ldpc_amd_fec_rs_encode_packets_dev) ----------------------------------------------------------------------------------------------
// What an entry point has of its call.  A single stream is the one-flow case: its constructor describes it as flow 0 of one, in
// segmented order.  Where the entry points differ in WHICH checks tx_check makes, the difference is a flag here, set at the entry
// point (DESIGN.md has the table); the ORDER of the checks is tx_check's, one for all.
struct TxCall {
    const char *who;
    const char *unit;   // what the call counts, in the texts that say so: "frames", or "blocks" (the RS sender)
    int n, k, S;
    bool triangle;      // the code has a systematic encoder
    int64_t F;          // a single stream: the caller's count; a multi-flow call: frame_begin[nflows], set by tx_check
    int depth;
    const uint8_t *source;
    uint8_t *packets;
    bool multi;         // a multi-flow call: nflows .. flow_of are the caller's
    int nflows;
    const int64_t *frame_begin;
    const uint8_t *fec_class, *block0;
    int order;
    int32_t *flow_of;
    bool check_range = true;   // refuse F * n >= 2^31
    bool check_words = true;   // refuse a source off the 4-byte grid when S is word-sized
    int64_t one_begin[2];      // a single stream as one flow
    uint8_t one_class, one_block0;

    TxCall(const char *who_, const char *unit_, int n_, int k_, bool triangle_, int S_, int64_t F_, unsigned fec_class_, unsigned block0_, int depth_,
           const uint8_t *source_, uint8_t *packets_)
        : who(who_), unit(unit_), n(n_), k(k_), S(S_), triangle(triangle_), F(F_), depth(depth_), source(source_), packets(packets_), multi(false),
          nflows(1), frame_begin(one_begin), fec_class(&one_class), block0(&one_block0), order(LDPC_AMD_FEC_TX_SEGMENTED), flow_of(nullptr),
          one_begin{0, F_}, one_class((uint8_t)(fec_class_ & 0xffu)), one_block0((uint8_t)(block0_ & 0xffu))
    {
    }
    TxCall(const char *who_, int n_, int k_, bool triangle_, int S_, int nflows_, const int64_t *frame_begin_, const uint8_t *fec_class_,
           const uint8_t *block0_, int order_, int depth_, const uint8_t *source_, uint8_t *packets_, int32_t *flow_of_)
        : who(who_), unit("frames"), n(n_), k(k_), S(S_), triangle(triangle_), F(0), depth(depth_), source(source_), packets(packets_), multi(true),
          nflows(nflows_), frame_begin(frame_begin_), fec_class(fec_class_), block0(block0_), order(order_), flow_of(flow_of_), one_begin{0, 0},
          one_class(0), one_block0(0)
    {
    }
    TxCall(const TxCall &) = delete;   // (frame_begin .. block0 may point into the object)
};

// the code of an LDPC sender's handle; nullptr: LDPC_AMD_ENOCODE is set
const DevCode *tx_code(ldpc_amd_ctx *ctx, int code)
{
    if (code >= 0 && code < (int)ctx->codes.size()) return &ctx->codes[code]->dev;
    set_error(ctx, LDPC_AMD_ENOCODE, "unknown code handle %d", code);
    return nullptr;
}

// the first flow that breaks the whole-group condition of ROUND_ROBIN at depth D > 1 (a non-empty flow whose block0 or frame count
// is no multiple of D), -1: none
int tx_flows_part_group(int nflows, const int64_t *frame_begin, const uint8_t *block0, int depth)
{
    if (depth <= 1) return -1;
    for (int f = 0; f < nflows; f++) {
        const int64_t c = frame_begin[f + 1] - frame_begin[f];
        if (c > 0 && (block0[f] % depth != 0 || c % depth != 0)) return f;
    }
    return -1;
}

// A sender call's checks, in the one order all five entry points refuse in.  OK with c.F == 0: nothing to send, and nothing below the
// count was looked at (an unsupported S, null pointers and a code without encoder all pass).
int tx_check(ldpc_amd_ctx *ctx, TxCall &c)
{
    const char *who = c.who;
    if (c.multi) {
        if (c.nflows < 1 || c.nflows > LDPC_AMD_FEC_TX_MAX_FLOWS)
            return set_error(ctx, LDPC_AMD_EINVAL, "%s: nflows must be 1..%d (got %d)", who, LDPC_AMD_FEC_TX_MAX_FLOWS, c.nflows);
        if (!c.frame_begin || !c.fec_class || !c.block0)
            return set_error(ctx, LDPC_AMD_EINVAL, "%s: frame_begin / fec_class / block0 must not be null", who);
        if (c.S < 1) return set_error(ctx, LDPC_AMD_EINVAL, "%s: bad S", who);
        if (c.order != LDPC_AMD_FEC_TX_SEGMENTED && c.order != LDPC_AMD_FEC_TX_ROUND_ROBIN)
            return set_error(ctx, LDPC_AMD_EINVAL, "%s: unknown order %d", who, c.order);
        if (c.frame_begin[0] != 0) return set_error(ctx, LDPC_AMD_EINVAL, "%s: frame_begin must start at 0", who);
        for (int f = 0; f < c.nflows; f++)
            if (c.frame_begin[f + 1] < c.frame_begin[f]) return set_error(ctx, LDPC_AMD_EINVAL, "%s: frame_begin decreases at flow %d", who, f);
    } else if (c.F < 0 || c.S < 1)
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: bad n%s/S", who, c.unit);
    if (!LDPC_AMD_FEC_ILV_DEPTH_OK(c.depth)) return set_error(ctx, LDPC_AMD_EINVAL, "%s: depth must be 1, 2, 4, 8 or 16 (got %d)", who, c.depth);
    if (c.multi) {
        const int f = c.order == LDPC_AMD_FEC_TX_ROUND_ROBIN ? tx_flows_part_group(c.nflows, c.frame_begin, c.block0, c.depth) : -1;
        if (f >= 0)
            return set_error(ctx, LDPC_AMD_EINVAL,
                             "%s: round robin at depth %d needs whole aligned groups, block0 %% depth == 0 and frames %% depth == 0 for every flow "
                             "(flow %d: block0=%d frames=%lld)",
                             who, c.depth, f, (int)c.block0[f], (long long)(c.frame_begin[f + 1] - c.frame_begin[f]));
        c.F = c.frame_begin[c.nflows];
    }
    const int64_t F = c.F;
    if (c.check_range && F > (((int64_t)1 << 31) - 1) / c.n)
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: %lld %s of %d packets are not below 2^31 packets", who, (long long)F, c.unit, c.n);
    if (F == 0) return LDPC_AMD_OK;
    if (!c.triangle) return set_error(ctx, LDPC_AMD_EUNSUP, "code is not in triangle form: no systematic encoder");
    if (!symbol_len_ok(ctx, c.S)) return refuse_symbol_len(ctx, c.S, "S must be 1 or a multiple of 16 (got %d)");
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!c.source || !c.packets || !is_device_ptr(ctx, c.source) || !is_device_ptr(ctx, c.packets) || (c.flow_of && !is_device_ptr(ctx, c.flow_of)))
        return set_error(ctx, LDPC_AMD_EINVAL, c.multi ? "%s: source / packets / flow_of must be device pointers of device %d"
                                                       : "%s: source / packets must be device pointers of device %d", who, ctx->device);
    if (((uintptr_t)c.flow_of & 3) != 0) return set_error(ctx, LDPC_AMD_EINVAL, "%s: flow_of must be 4-byte aligned", who);
    if (c.check_words && symbol_len_words(c.S) && ((uintptr_t)c.source & 3) != 0)
        return set_error(ctx, LDPC_AMD_EINVAL, "word-sized symbols (S = %d) need 4-byte aligned symbol arrays", c.S);
    const uintptr_t s0 = (uintptr_t)c.source, s1 = s0 + (size_t)c.k * c.S * (size_t)F;
    const uintptr_t p0 = (uintptr_t)c.packets, p1 = p0 + (size_t)c.n * ((size_t)c.S + kHdr) * (size_t)F;
    const uintptr_t q0 = (uintptr_t)c.flow_of, q1 = q0 + sizeof(int32_t) * (size_t)(F * c.n);
    if (s0 < p1 && p0 < s1) return set_error(ctx, LDPC_AMD_EINVAL, "%s: source and packets overlap", who);
    if (c.flow_of && ((q0 < p1 && p0 < q1) || (q0 < s1 && s0 < q1))) return set_error(ctx, LDPC_AMD_EINVAL, "%s: flow_of overlaps source or packets", who);
    return LDPC_AMD_OK;
}

// The composed paths go through the context's codeword scratch, at most kSenderScratchMax bytes of it: reserves it for F frames of
// cw_frame bytes.  *chunk: the frames of one round.  The rounds follow one another on the context's stream, so the scratch is free
// again when the next encode starts.
int tx_reserve_chunk(ldpc_amd_ctx *ctx, int64_t F, size_t cw_frame, int64_t *chunk)
{
    *chunk = std::max<int64_t>(1, std::min<int64_t>(F, (int64_t)(kSenderScratchMax / cw_frame)));
    return scratch_reserve(ctx, ctx->sender_cw, (size_t)*chunk * cw_frame);
}

// The multi-flow orders as arithmetic, the body of ldpc_amd_fec_tx_flows_layout (depth 1; block0 may be null there) and
// ldpc_amd_fec_tx_flows_ilv_layout.  SEGMENTED: every flow's single-flow interleaved layout, shifted to the flow's first packet.
// ROUND_ROBIN on GROUPS of `depth` frames -- while group r of every flow is on the wire the active flows are those with more than r D
// frames, A_r of them, and a round takes one packet of each in ascending order: member i' of the group starts at base_r + rank + i' A_r
// (rank: the active flows below it), its rows are D A_r packets apart, base_r = n D (A_0 + ... + A_{r-1}).  The active list only ever
// loses flows, so it is compacted in place as r grows: the work is the sum of the A_r.  At depth 1 a group is a frame: first =
// base_i + rank, stride = A_i.
int64_t tx_flows_layout(int nflows, const int64_t *frame_begin, int n, const uint8_t *block0, int depth, int order, int64_t *first, int32_t *stride)
{
    if (!LDPC_AMD_FEC_ILV_DEPTH_OK(depth) || (!block0 && depth != 1)) return LDPC_AMD_EINVAL;
    if (nflows < 1 || nflows > LDPC_AMD_FEC_TX_MAX_FLOWS || !frame_begin || n < 1 || frame_begin[0] != 0) return LDPC_AMD_EINVAL;
    if (order != LDPC_AMD_FEC_TX_SEGMENTED && order != LDPC_AMD_FEC_TX_ROUND_ROBIN) return LDPC_AMD_EINVAL;
    for (int f = 0; f < nflows; f++)
        if (frame_begin[f + 1] < frame_begin[f]) return LDPC_AMD_EINVAL;
    const int64_t F = frame_begin[nflows];
    if (F > (((int64_t)1 << 31) - 1) / n) return LDPC_AMD_EINVAL;   // F * n < 2^31
    if (order == LDPC_AMD_FEC_TX_SEGMENTED) {
        for (int f = 0; f < nflows; f++) {
            const int64_t t0 = frame_begin[f], c = frame_begin[f + 1] - t0;
            if (ldpc_amd_fec_tx_ilv_layout(c, n, block0 ? block0[f] : 0, depth, first ? first + t0 : nullptr, stride ? stride + t0 : nullptr) != c * n)
                return LDPC_AMD_EINVAL;
            for (int64_t i = 0; first && i < c; i++) first[t0 + i] += t0 * n;
        }
        return F * n;
    }
    if (tx_flows_part_group(nflows, frame_begin, block0, depth) >= 0) return LDPC_AMD_EINVAL;
    std::vector<int> active;
    active.reserve((size_t)nflows);
    for (int f = 0; f < nflows; f++)
        if (frame_begin[f + 1] > frame_begin[f]) active.push_back(f);
    int64_t base = 0;
    for (int64_t r = 0; !active.empty(); r++) {
        const int64_t A = (int64_t)active.size();
        size_t keep = 0;
        for (size_t rank = 0; rank < active.size(); rank++) {
            const int f = active[rank];
            const int64_t t = frame_begin[f] + r * depth;
            for (int i = 0; i < depth; i++) {
                if (first) first[t + i] = base + (int64_t)rank + i * A;
                if (stride) stride[t + i] = (int32_t)(depth * A);
            }
            if (frame_begin[f + 1] - frame_begin[f] > (r + 1) * depth) active[keep++] = f;
        }
        active.resize(keep);
        base += A * n * depth;
    }
    return F * n;
}

// ---- the descriptor-driven senders (all but ldpc_amd_fec_encode_packets_dev) -------------------------------------------------------
// The call's table on the host: [F] descriptors {first packet, stride, class << 8 | block} by the layout of its flows, a multi-flow
// call's [F] flow numbers behind them.  *max_stride: the largest stride.
int tx_fill_described(ldpc_amd_ctx *ctx, const TxCall &c, TxFrameDesc *hd, int64_t *max_stride)
{
    const int64_t F = c.F;
    int32_t *hflow = c.multi ? (int32_t *)(hd + F) : nullptr;
    std::vector<int64_t> first((size_t)F);
    std::vector<int32_t> stride((size_t)F);
    if (tx_flows_layout(c.nflows, c.frame_begin, c.n, c.block0, c.depth, c.order, first.data(), stride.data()) != F * c.n)
        return set_error(ctx, LDPC_AMD_EINVAL, c.multi ? "%s: bad frame_begin" : "%s: bad layout arguments", c.who);
    for (int f = 0; f < c.nflows; f++)
        for (int64_t t = c.frame_begin[f]; t < c.frame_begin[f + 1]; t++) {
            hd[t].first = (uint64_t)first[(size_t)t];
            hd[t].stride = (uint32_t)stride[(size_t)t];
            hd[t].hdr = ((uint32_t)c.fec_class[f] << 8) | (((uint32_t)c.block0[f] + (uint32_t)(t - c.frame_begin[f])) & 0xffu);
            if (hflow) hflow[t] = f;
            *max_stride = std::max<int64_t>(*max_stride, stride[(size_t)t]);
        }
    return LDPC_AMD_OK;
}

// Stages the table: filled in a slot of the context's pinned ring (internal.h: PinnedRing) and copied to the context's device table
// on the stream.  *dd_out: the device table.
int tx_stage_described(ldpc_amd_ctx *ctx, const TxCall &c, const TxFrameDesc **dd_out, int64_t *max_stride_out)
{
    const size_t tab_bytes = (sizeof(TxFrameDesc) + (c.multi ? sizeof(int32_t) : 0)) * (size_t)c.F;
    int rc;
    if ((rc = scratch_reserve(ctx, ctx->txf_desc, tab_bytes))) return rc;
    void *hd = nullptr;
    size_t want = 0;
    if ((rc = pinned_ring_acquire(ctx, ctx->txf_ring, tab_bytes, &hd, &want)))
        return rc == LDPC_AMD_ENOMEM ? set_error(ctx, LDPC_AMD_ENOMEM, "%s: no pinned memory for %zu descriptor bytes", c.who, want) : rc;
    *max_stride_out = 1;
    if ((rc = tx_fill_described(ctx, c, (TxFrameDesc *)hd, max_stride_out))) return rc;
    LDPC_HIP_TRY(ctx, hipMemcpyAsync(ctx->txf_desc.p, hd, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = pinned_ring_commit(ctx, ctx->txf_ring))) return rc;
    *dd_out = (const TxFrameDesc *)ctx->txf_desc.p;
    return LDPC_AMD_OK;
}

// the composed senders' packetiser: the codewords cw of the `cnt` frames that dd describes -> their packets
inline int tx_packetize_described(ldpc_amd_ctx *ctx, const uint8_t *cw, int64_t cnt, int n, int S, const TxFrameDesc *dd, uint8_t *packets)
{
    const int64_t rows = cnt * n;
    if (S % 16 == 0 && ((uintptr_t)packets & 7) == 0)   // (the scratch is 16-byte aligned)
        hipLaunchKernelGGL(fec_packetize_flows_v16, dim3(grid_for(rows * (S / 16))), dim3(kThreads), 0, ctx->stream, reinterpret_cast<const uint4 *>(cw),
                           rows, n, S / 16, dd, packets);
    else
        hipLaunchKernelGGL(fec_packetize_flows_bytes, dim3(grid_for(rows * (S + kHdr))), dim3(kThreads), 0, ctx->stream, cw, rows, n, S, dd, packets);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

// Sends a checked call of c.F > 0 frames by its descriptors: stages the table; then fused(dd, max_stride), the descriptor form of the
// code's packet encoder (path 1), where that has the call -- it answers kEncodeNotFused, with nothing launched, where not --, else
// encode(cnt, source, cw) into the context's codeword scratch and the descriptor-driven packetisers, chunk by chunk (path 2,
// composed); then a multi-flow call's flow_of; and records the call as the last of its kind.
template <class Fused, class Encode>
int tx_send_described(ldpc_amd_ctx *ctx, const TxCall &c, TxKind kind, Fused fused, Encode encode)
{
    const int64_t F = c.F;
    const size_t src_frame = (size_t)c.k * c.S, cw_frame = (size_t)c.n * c.S;
    int rc;
    const TxFrameDesc *dd = nullptr;
    int64_t max_stride = 1;
    if ((rc = tx_stage_described(ctx, c, &dd, &max_stride))) return rc;
    rc = fused(dd, max_stride);
    if (rc != LDPC_AMD_OK && rc != kEncodeNotFused) return rc;
    const int path = rc == LDPC_AMD_OK ? 1 : 2;
    if (path == 2) {
        int64_t chunk = 0;
        if ((rc = tx_reserve_chunk(ctx, F, cw_frame, &chunk))) return rc;
        uint8_t *cw = (uint8_t *)ctx->sender_cw.p;
        for (int64_t f0 = 0; f0 < F; f0 += chunk) {
            const int64_t cnt = std::min(chunk, F - f0);
            if ((rc = encode(cnt, c.source + (size_t)f0 * src_frame, cw))) return rc;
            if ((rc = tx_packetize_described(ctx, cw, cnt, c.n, c.S, dd + f0, c.packets))) return rc;
        }
    }
    if (c.flow_of) {   // (a multi-flow call's: the frames' flows lie behind the descriptors)
        const int64_t P = F * c.n;
        hipLaunchKernelGGL(fec_tx_flow_of, dim3(grid_for(P)), dim3(kThreads), 0, ctx->stream, dd, (const int32_t *)(dd + F), P, c.n, c.flow_of);
        LDPC_HIP_TRY(ctx, hipGetLastError());
    }
    ctx->tx_last[kind] = TxLast{path, F};
    return LDPC_AMD_OK;
}

// the checks, then the LDPC launchers behind tx_send_described: the three descriptor-driven LDPC senders
int tx_send_ldpc(ldpc_amd_ctx *ctx, const DevCode &cd, TxCall &c, TxKind kind)
{
    const int rc = tx_check(ctx, c);
    if (rc || c.F == 0) return rc;
    return tx_send_described(
        ctx, c, kind, [&](const TxFrameDesc *dd, int64_t max_stride) { return launch_encode_packets_flows(ctx, cd, c.S, c.F, c.source, dd, max_stride, c.packets); },
        [&](int64_t cnt, const uint8_t *src, uint8_t *cw) { return launch_encode(ctx, cd, c.S, cnt, src, cw); });
}

// the four words of the descriptor-driven senders' info calls
int tx_info(ldpc_amd_ctx *ctx, const char *who, TxKind kind, int64_t info[4])
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!info) return set_error(ctx, LDPC_AMD_EINVAL, "%s: info must not be null", who);
    info[0] = ctx->tx_last[kind].path;
    info[1] = (int64_t)ctx->sender_cw.cap;
    info[2] = (int64_t)(ctx->txf_desc.cap + ctx->txf_ring.bytes());
    info[3] = ctx->tx_last[kind].count;
    return LDPC_AMD_OK;
}

}  // namespace

extern "C" {

int ldpc_amd_fec_packetize_dev(ldpc_amd_ctx *ctx, const uint8_t *frames, int64_t nframes, int n, int S, unsigned fec_class,
                               unsigned block0, uint8_t *packets)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (nframes < 0 || n <= 0 || n > 65536 || S <= 0) return set_error(ctx, LDPC_AMD_EINVAL, "fec_packetize_dev: bad nframes/n/S");
    if (nframes == 0) return LDPC_AMD_OK;
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!frames || !packets || !is_device_ptr(ctx, frames) || !is_device_ptr(ctx, packets))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_packetize_dev: frames / packets must be device pointers of device %d", ctx->device);
    const int64_t rows = nframes * n;
    if (S % 16 == 0 && ((uintptr_t)frames & 15) == 0 && ((uintptr_t)packets & 7) == 0) {
        hipLaunchKernelGGL(fec_packetize_v16, dim3(grid_for(rows * (S / 16))), dim3(kThreads), 0, ctx->stream,
                           reinterpret_cast<const uint4 *>(frames), rows, n, S / 16, fec_class, block0, packets);
    } else {
        hipLaunchKernelGGL(fec_packetize_bytes, dim3(grid_for(rows * (S + kHdr))), dim3(kThreads), 0, ctx->stream,
                           frames, rows, n, S, fec_class, block0, packets);
    }
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

// ---- the sender (include/ldpc_erasure_amd_sender.h) ---------------------------------------------------------------------
// Fused where the encoder has a packet-output form (launch_encode_packets: the persistent scatter encoder stores its rows at their
// places in the packet array and the headers beside them -- the reference's one-kernel sender, ...VITA_in_UDP_out.cl:84-129,168-211);
// else composed: encode a chunk of frames into the context's scratch, packetise it, next chunk.  Its kernels take a class and a first
// block number, no descriptors: of the common part it shares the checks and the chunks.
int ldpc_amd_fec_encode_packets_dev(ldpc_amd_ctx *ctx, int code, int S, int64_t nframes, const uint8_t *source, unsigned fec_class,
                                    unsigned block0, uint8_t *packets)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    const DevCode *cdp = tx_code(ctx, code);
    if (!cdp) return LDPC_AMD_ENOCODE;
    const DevCode &cd = *cdp;
    TxCall c("fec_encode_packets_dev", "frames", cd.n, cd.k, cd.enc_nlevels != 0, S, nframes, fec_class, block0, 1, source, packets);
    c.check_range = false;   // this sender has never refused a count: its packetisers index the packets in 64 bits
    c.check_words = false;   // ... nor a word-sized S's source off the 4-byte grid itself: the encoder it launches does (launch_encode)
    int rc = tx_check(ctx, c);
    if (rc || nframes == 0) return rc;
    rc = launch_encode_packets(ctx, cd, S, nframes, source, fec_class, block0, packets);
    if (rc != kEncodeNotFused) {
        if (rc == LDPC_AMD_OK) ctx->tx_last[kTxPlain] = TxLast{1, nframes};
        return rc;
    }
    const size_t src_frame = (size_t)cd.k * S, pk_frame = (size_t)cd.n * ((size_t)S + kHdr);
    int64_t chunk = 0;
    if ((rc = tx_reserve_chunk(ctx, nframes, (size_t)cd.n * S, &chunk))) return rc;
    uint8_t *cw = (uint8_t *)ctx->sender_cw.p;
    for (int64_t f0 = 0; f0 < nframes; f0 += chunk) {
        const int64_t cnt = std::min(chunk, nframes - f0);
        if ((rc = launch_encode(ctx, cd, S, cnt, source + (size_t)f0 * src_frame, cw))) return rc;
        if ((rc = ldpc_amd_fec_packetize_dev(ctx, cw, cnt, cd.n, S, fec_class, (block0 + (unsigned)(f0 & 0xff)) & 0xffu, packets + (size_t)f0 * pk_frame)))
            return rc;
    }
    ctx->tx_last[kTxPlain] = TxLast{2, nframes};
    return LDPC_AMD_OK;
}

int ldpc_amd_fec_sender_info(ldpc_amd_ctx *ctx, int info[4])
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!info) return set_error(ctx, LDPC_AMD_EINVAL, "fec_sender_info: info must not be null");
    info[0] = ctx->tx_last[kTxPlain].path;
    info[1] = (int)std::min<size_t>(ctx->sender_cw.cap, (size_t)INT32_MAX);
    info[2] = info[3] = 0;
    return LDPC_AMD_OK;
}

// ---- the multi-flow senders (include/ldpc_erasure_amd_sender_flows.h; with a depth: include/ldpc_erasure_amd_interleave_flows.h) ----
int64_t ldpc_amd_fec_tx_flows_layout(int nflows, const int64_t *frame_begin, int n, int order, int64_t *first, int32_t *stride)
{
    return tx_flows_layout(nflows, frame_begin, n, nullptr, 1, order, first, stride);
}

int64_t ldpc_amd_fec_tx_flows_ilv_layout(int nflows, const int64_t *frame_begin, int n, const uint8_t *block0, int depth, int order, int64_t *first,
                                         int32_t *stride)
{
    if (!block0) return LDPC_AMD_EINVAL;
    return tx_flows_layout(nflows, frame_begin, n, block0, depth, order, first, stride);
}

// The body of both: depth 1 is the order of include/ldpc_erasure_amd_sender_flows.h.  packet_begin is written when something was sent.
static int tx_flows_send(ldpc_amd_ctx *ctx, const char *who, TxKind kind, int code, int S, int nflows, const int64_t *frame_begin, const uint8_t *source,
                         const uint8_t *fec_class, const uint8_t *block0, int order, int depth, uint8_t *packets, int32_t *flow_of,
                         int64_t *packet_begin)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    const DevCode *cd = tx_code(ctx, code);
    if (!cd) return LDPC_AMD_ENOCODE;
    TxCall c(who, cd->n, cd->k, cd->enc_nlevels != 0, S, nflows, frame_begin, fec_class, block0, order, depth, source, packets, flow_of);
    const int rc = tx_send_ldpc(ctx, *cd, c, kind);
    if (rc == LDPC_AMD_OK && c.F > 0 && packet_begin)
        for (int f = 0; f <= nflows; f++) packet_begin[f] = frame_begin[f] * cd->n;
    return rc;
}

int ldpc_amd_fec_encode_packets_flows_dev(ldpc_amd_ctx *ctx, int code, int S, int nflows, const int64_t *frame_begin, const uint8_t *source,
                                          const uint8_t *fec_class, const uint8_t *block0, int order, uint8_t *packets, int32_t *flow_of,
                                          int64_t *packet_begin)
{
    return tx_flows_send(ctx, "fec_encode_packets_flows_dev", kTxFlows, code, S, nflows, frame_begin, source, fec_class, block0, order, 1, packets, flow_of,
                         packet_begin);
}

int ldpc_amd_fec_encode_packets_flows_ilv_dev(ldpc_amd_ctx *ctx, int code, int S, int nflows, const int64_t *frame_begin, const uint8_t *source,
                                              const uint8_t *fec_class, const uint8_t *block0, int order, uint8_t *packets, int32_t *flow_of,
                                              int64_t *packet_begin, int depth)
{
    return tx_flows_send(ctx, "fec_encode_packets_flows_ilv_dev", kTxFlowsIlv, code, S, nflows, frame_begin, source, fec_class, block0, order, depth,
                         packets, flow_of, packet_begin);
}

int ldpc_amd_fec_sender_flows_info(ldpc_amd_ctx *ctx, int64_t info[4]) { return tx_info(ctx, "fec_sender_flows_info", kTxFlows, info); }
int ldpc_amd_fec_sender_flows_ilv_info(ldpc_amd_ctx *ctx, int64_t info[4]) { return tx_info(ctx, "fec_sender_flows_ilv_info", kTxFlowsIlv, info); }

// ---- the block-interleaved sender (include/ldpc_erasure_amd_interleave.h) ------------------------------------------------------
// The order as arithmetic: walk the frames run by run.  A run is the frames s .. s+m-1 of one group of D block numbers; its member i
// starts at packet n s + i and its rows are m packets apart.
int64_t ldpc_amd_fec_tx_ilv_layout(int64_t nframes, int n, unsigned block0, int depth, int64_t *first, int32_t *stride)
{
    if (!LDPC_AMD_FEC_ILV_DEPTH_OK(depth) || n < 1 || nframes < 0) return LDPC_AMD_EINVAL;
    if (nframes > (((int64_t)1 << 31) - 1) / n) return LDPC_AMD_EINVAL;   // nframes * n < 2^31
    for (int64_t s = 0; s < nframes;) {
        const int b = (int)((block0 + (uint64_t)s) & 0xffu);
        const int64_t m = std::min<int64_t>(depth - b % depth, nframes - s);
        for (int64_t i = 0; i < m; i++) {
            if (first) first[s + i] = s * n + i;
            if (stride) stride[s + i] = (int32_t)m;
        }
        s += m;
    }
    return nframes * n;
}

int ldpc_amd_fec_encode_packets_ilv_dev(ldpc_amd_ctx *ctx, int code, int S, int64_t nframes, const uint8_t *source, unsigned fec_class,
                                        unsigned block0, int depth, uint8_t *packets)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    const DevCode *cd = tx_code(ctx, code);
    if (!cd) return LDPC_AMD_ENOCODE;
    TxCall c("fec_encode_packets_ilv_dev", "frames", cd->n, cd->k, cd->enc_nlevels != 0, S, nframes, fec_class, block0, depth, source, packets);
    return tx_send_ldpc(ctx, *cd, c, kTxIlv);
}

int ldpc_amd_fec_sender_ilv_info(ldpc_amd_ctx *ctx, int64_t info[4]) { return tx_info(ctx, "fec_sender_ilv_info", kTxIlv, info); }

// ---- the Reed-Solomon sender (include/ldpc_erasure_amd_rs_wire.h) ------------------------------------------------------------------
// The interleaved sender for the blocks of an RS code: the packet encoder of rs_wire_dev.hip (path 1, fused) where
// launch_rs_encode_packets has it for this call, else the RS encoder into the context's codeword scratch (path 2, composed).
int ldpc_amd_fec_rs_encode_packets_dev(ldpc_amd_ctx *ctx, int rs, int S, int64_t nblocks, const uint8_t *source, unsigned fec_class,
                                       unsigned block0, int depth, uint8_t *packets)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (rs < 0 || rs >= (int)ctx->rs.size()) return set_error(ctx, LDPC_AMD_ENOCODE, "unknown RS handle %d", rs);
    const HostRs &r = *ctx->rs[rs];
    TxCall c("fec_rs_encode_packets_dev", "blocks", r.n, r.k, /* every RS code has a systematic encoder */ true, S, nblocks, fec_class, block0, depth, source,
             packets);
    const int rc = tx_check(ctx, c);
    if (rc || nblocks == 0) return rc;
    return tx_send_described(
        ctx, c, kTxRs, [&](const TxFrameDesc *dd, int64_t max_stride) { return launch_rs_encode_packets(ctx, r, S, nblocks, source, dd, max_stride, packets); },
        [&](int64_t cnt, const uint8_t *src, uint8_t *cw) { return launch_rs_encode(ctx, r, S, cnt, src, cw); });
}

int ldpc_amd_fec_rs_sender_info(ldpc_amd_ctx *ctx, int64_t info[4]) { return tx_info(ctx, "fec_rs_sender_info", kTxRs, info); }

int ldpc_amd_fec_rx_dev_create(ldpc_amd_ctx *ctx, int n, int k, int S, ldpc_amd_fec_rx_dev **out)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!out || n <= 0 || n > 65536 || k <= 0 || k >= n || S <= 0)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rx_dev_create: need n <= 65536, 0 < k < n, S >= 1 (n=%d k=%d S=%d)", n, k, S);
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ldpc_amd_fec_rx_dev *rx = new (std::nothrow) ldpc_amd_fec_rx_dev();
    if (!rx) return set_error(ctx, LDPC_AMD_ENOMEM, "fec_rx_dev_create: out of host memory");
    rx->ctx = ctx;
    rx->n = n; rx->k = k; rx->S = S;
    rx->kd = k + (int)lround((n - k) * 0.8);   // desired_parity_rx, :54
    rx->km = k + (int)lround((n - k) * 0.2);   // min_parity_rx, :55
    const size_t plane = (size_t)n * S;
    hipError_t e = hipMalloc((void **)&rx->stage_sym, 2 * plane);
    if (e == hipSuccess) e = hipMalloc((void **)&rx->stage_er, 2 * (size_t)n);
    // :62-71 all symbols erased until a packet produces them, payload zero
    if (e == hipSuccess) e = hipMemsetAsync(rx->stage_sym, 0, 2 * plane, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(rx->stage_er, 1, 2 * (size_t)n, ctx->stream);
    if (e != hipSuccess) {
        ldpc_amd_fec_rx_dev_destroy(rx);
        return set_error(ctx, e == hipErrorOutOfMemory ? LDPC_AMD_ENOMEM : LDPC_AMD_EHIP, "fec_rx_dev_create: %s", hipGetErrorString(e));
    }
    *out = rx;
    return LDPC_AMD_OK;
}

void ldpc_amd_fec_rx_dev_destroy(ldpc_amd_fec_rx_dev *rx)
{
    if (!rx) return;
    (void)hipSetDevice(rx->ctx->device);
    (void)hipStreamSynchronize(rx->ctx->stream);   // pending work of this receiver may still use its buffers
    Scratch *sc[] = {&rx->dense, &rx->dest, &rx->win, &rx->res};
    for (Scratch *s : sc)
        if (s->p) (void)hipFree(s->p);
    if (rx->stage_sym) (void)hipFree(rx->stage_sym);
    if (rx->stage_er) (void)hipFree(rx->stage_er);
    if (rx->res_host) (void)hipHostFree(rx->res_host);
    delete rx;
}

int64_t ldpc_amd_fec_rx_dev_dropped(const ldpc_amd_fec_rx_dev *rx) { return rx ? rx->dropped : -1; }

}  // extern "C"

// One call's PLAN: (a) + (b) and the read-back.  Nothing of the receiver's state changes before rx_commit.
struct RxPlan {
    int closes = 0;
    int64_t used = 0, dropped = 0;
    const int32_t *h = nullptr;   // the scan's result record (pinned), the closed blocks' numbers behind R_WORDS
};

static int rx_plan(ldpc_amd_fec_rx_dev *rx, const char *who, const uint8_t *packets, int64_t npackets, int max_blocks, RxPlan &pl)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int n = rx->n;
    const int64_t plen = (int64_t)rx->S + kHdr;
    const size_t res_bytes = sizeof(int32_t) * ((size_t)R_WORDS + (size_t)max_blocks);
    int rc;
    if ((rc = scratch_reserve(ctx, rx->dense, sizeof(uint32_t) * (size_t)npackets)) ||
        (rc = scratch_reserve(ctx, rx->dest, sizeof(int32_t) * (size_t)npackets)) ||
        (rc = scratch_reserve(ctx, rx->win, sizeof(int32_t) * ((size_t)max_blocks + 2) * (size_t)n)) ||
        (rc = scratch_reserve(ctx, rx->res, res_bytes)))
        return rc;
    if ((rc = rx_readback_grow(ctx, rx, res_bytes))) return rc;
    uint32_t *dense = (uint32_t *)rx->dense.p;
    int32_t *dest = (int32_t *)rx->dest.p, *res = (int32_t *)rx->res.p;

    // (a) + (b): the plan
    if (plen % 4 == 0 && ((uintptr_t)packets & 3) == 0)
        hipLaunchKernelGGL(fec_rx_headers<true>, dim3(grid_for(npackets)), dim3(kThreads), 0, ctx->stream, packets, npackets, (int)plen, dense);
    else
        hipLaunchKernelGGL(fec_rx_headers<false>, dim3(grid_for(npackets)), dim3(kThreads), 0, ctx->stream, packets, npackets, (int)plen, dense);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fec_rx_scan, dim3(1), dim3(64), 0, ctx->stream, dense, npackets, n, rx->kd, rx->km, max_blocks, rx->cur,
                       rx->next, rx->ccnt, rx->ncnt, dest, res);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    LDPC_HIP_TRY(ctx, hipMemcpyAsync(rx->res_host, res, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    LDPC_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = check_device_error(ctx))) return rc;
    const int32_t *h = rx->res_host;
    if (h[R_ERR])
        return set_error(ctx, LDPC_AMD_EHIP, "%s: the plan scan hit its iteration cap (internal error); the receiver's state is unchanged", who);
    pl.h = h;
    pl.closes = h[R_CLOSES];
    pl.used = (int64_t)(((uint64_t)(uint32_t)h[R_CONSUMED_HI] << 32) | (uint32_t)h[R_CONSUMED_LO]);
    pl.dropped = (int64_t)(((uint64_t)(uint32_t)h[R_DROPPED_HI] << 32) | (uint32_t)h[R_DROPPED_LO]);
    return LDPC_AMD_OK;
}

// (c): the winners' table of the call, [(closes + 2)][n]
static int rx_winners(ldpc_amd_fec_rx_dev *rx, const RxPlan &pl)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    int32_t *win = (int32_t *)rx->win.p;
    LDPC_HIP_TRY(ctx, hipMemsetAsync(win, 0xff, sizeof(int32_t) * ((size_t)pl.closes + 2) * (size_t)rx->n, ctx->stream));   // -1: no packet
    hipLaunchKernelGGL(fec_rx_winners, dim3(grid_for(pl.used)), dim3(kThreads), 0, ctx->stream, (const uint32_t *)rx->dense.p,
                       (const int32_t *)rx->dest.p, pl.used, rx->n, win);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

// (d) for the closed slots first .. first + count - 1 (gather) or (e) for the two open blocks
template <bool GATHER>
static int rx_move(ldpc_amd_fec_rx_dev *rx, const RxPlan &pl, const uint8_t *packets, int first, int count, uint8_t *sym, uint8_t *er)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int n = rx->n, S = rx->S;
    MoveArgs a{};
    a.packets = packets; a.plen = (int64_t)S + kHdr; a.win = (const int32_t *)rx->win.p; a.stage_sym = rx->stage_sym; a.stage_er = rx->stage_er;
    a.sym_out = sym; a.er_out = er; a.n = n; a.S = S; a.cb = rx->cb; a.closes = pl.closes; a.first = first; a.count = count;
    const bool v16 = S % 16 == 0 && ((uintptr_t)packets & 7) == 0 && ((uintptr_t)sym & 15) == 0;
    const int64_t q = v16 ? S / 16 : S;
    const int64_t items = (GATHER ? (int64_t)count : 2) * n * q;
    if (GATHER && count <= 0) return LDPC_AMD_OK;
    if (v16) hipLaunchKernelGGL((fec_rx_move<GATHER, true>), dim3(grid_for(items)), dim3(kThreads), 0, ctx->stream, a);
    else hipLaunchKernelGGL((fec_rx_move<GATHER, false>), dim3(grid_for(items)), dim3(kThreads), 0, ctx->stream, a);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

static void rx_commit(ldpc_amd_fec_rx_dev *rx, const RxPlan &pl, int *blocks, int64_t *consumed)
{
    const int32_t *h = pl.h;
    rx->cur = h[R_CUR]; rx->next = h[R_NEXT]; rx->ccnt = h[R_CCNT]; rx->ncnt = h[R_NCNT];
    rx->cb ^= pl.closes & 1;   // :241, once per close
    rx->dropped += pl.dropped;
    if (blocks) memcpy(blocks, h + R_WORDS, sizeof(int) * (size_t)pl.closes);
    if (consumed) *consumed = pl.used;
}

extern "C" {

int ldpc_amd_fec_rx_dev_push_many(ldpc_amd_fec_rx_dev *rx, const uint8_t *packets, int64_t npackets, uint8_t *sym_batch,
                                  uint8_t *erased_batch, int *blocks, int max_blocks, int64_t *consumed)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    if (npackets < 0 || npackets >= ((int64_t)1 << 31) || max_blocks < 1)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rx_dev_push_many: need 0 <= npackets < 2^31 and max_blocks >= 1");
    if (!sym_batch || !erased_batch || (npackets > 0 && !packets))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rx_dev_push_many: packets / sym_batch / erased_batch must not be null");
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((npackets > 0 && !is_device_ptr(ctx, packets)) || !is_device_ptr(ctx, sym_batch) || !is_device_ptr(ctx, erased_batch))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rx_dev_push_many: packets / sym_batch / erased_batch must be device pointers of device %d",
                         ctx->device);
    if (consumed) *consumed = 0;
    if (npackets == 0) return 0;
    int rc;
    RxPlan pl;
    if ((rc = rx_plan(rx, "fec_rx_dev_push_many", packets, npackets, max_blocks, pl))) return rc;
    // (c), (d), (e): the data movement, asynchronous
    if ((rc = rx_winners(rx, pl)) || (rc = rx_move<true>(rx, pl, packets, 0, pl.closes, sym_batch, erased_batch)) ||
        (rc = rx_move<false>(rx, pl, packets, 0, 0, sym_batch, nullptr)))
        return rc;
    rx_commit(rx, pl, blocks, consumed);
    return pl.closes;
}

int ldpc_amd_fec_rx_dev_flush(ldpc_amd_fec_rx_dev *rx, uint8_t *sym_out, uint8_t *erased_out, int *block_out)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    if (rx->cur == -1 || (rx->ccnt == 0 && rx->ncnt == 0)) return 0;
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((sym_out && !is_device_ptr(ctx, sym_out)) || (erased_out && !is_device_ptr(ctx, erased_out)))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rx_dev_flush: sym_out / erased_out must be device pointers of device %d", ctx->device);
    const size_t plane = (size_t)rx->n * rx->S;
    uint8_t *ps = rx->stage_sym + (size_t)rx->cb * plane, *pe = rx->stage_er + (size_t)rx->cb * rx->n;
    // close_current: hand the current block out, reset its buffer, rotate
    if (sym_out) LDPC_HIP_TRY(ctx, hipMemcpyAsync(sym_out, ps, plane, hipMemcpyDeviceToDevice, ctx->stream));
    if (erased_out) LDPC_HIP_TRY(ctx, hipMemcpyAsync(erased_out, pe, rx->n, hipMemcpyDeviceToDevice, ctx->stream));
    LDPC_HIP_TRY(ctx, hipMemsetAsync(ps, 0, plane, ctx->stream));
    LDPC_HIP_TRY(ctx, hipMemsetAsync(pe, 1, rx->n, ctx->stream));
    if (block_out) *block_out = rx->cur;
    rx->cur = rx->next;
    rx->next = (rx->next + 1) & 0xff;
    rx->ccnt = rx->ncnt;
    rx->ncnt = 0;
    rx->cb ^= 1;
    return 1;
}

// ---- the receiver (include/ldpc_erasure_amd_receiver.h) -------------------------------------------------------------------
// push_many + decode_frames in one call.  FUSED where the decoder can fetch its rows from the packets itself (decode_reads_packets:
// the scatter kernels' packets-in form): (d) shrinks to fec_rx_sources -- n flags and n words per closed block instead of n rows -- and the
// decode follows the words; the reference's receiver is one kernel that reassembles and decodes (...with_reordering_logic.cl:44-141,
// 214-243).  Else COMPOSED: (d) gathers a chunk of closed blocks into the context's scratch, the decoder runs on it, next chunk; the
// chunks follow one another on the context's stream, so the scratch is free again when the next gather starts.
// (e) is launched BEHIND the decode in both paths: it overwrites the staging planes of the carried blocks, which the fused decode reads.
// The tail of the call -- reserve, row sources or gather, decode -- is rx_host.h's decode driver, as for every receiver below.
int ldpc_amd_fec_rx_dev_decode_many(ldpc_amd_fec_rx_dev *rx, int code, const uint8_t *packets, int64_t npackets, int max_sweeps, int do_ml,
                                    uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status, uint8_t *erased_out,
                                    int32_t *residual_src, int *blocks, int max_blocks, int64_t *consumed)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    if (code < 0 || code >= (int)ctx->codes.size()) return set_error(ctx, LDPC_AMD_ENOCODE, "unknown code handle %d", code);
    if (npackets < 0 || npackets >= ((int64_t)1 << 31) || max_blocks < 1)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rx_dev_decode_many: need 0 <= npackets < 2^31 and max_blocks >= 1");
    if (npackets == 0) {
        if (consumed) *consumed = 0;
        return 0;
    }
    int rc;
    const RxResults o{out, sweeps, residual, status, erased_out, residual_src};
    if ((rc = rx_decode_check(ctx, rx, "fec_rx_dev_decode_many", code, max_sweeps, o))) return rc;
    if (!packets || !is_device_ptr(ctx, packets))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rx_dev_decode_many: packets must be a device pointer of device %d", ctx->device);
    const DevCode &cd = ctx->codes[code]->dev;
    const int n = rx->n, S = rx->S;
    const bool fused = ctx->knobs.rx_pkt != 0 && ((uintptr_t)packets & 7) == 0 && decode_reads_packets(ctx, cd, S);
    const size_t frame = (size_t)n * S;
    const int64_t chunk = rx_chunk(max_blocks, frame);

    RxPlan pl;
    if ((rc = rx_plan(rx, "fec_rx_dev_decode_many", packets, npackets, max_blocks, pl))) return rc;
    const int closes = pl.closes;
    size_t scratch = 0;
    if ((rc = rx_decode_reserve(ctx, closes, n, frame, fused, chunk, &scratch))) return rc;
    if ((rc = rx_winners(rx, pl))) return rc;
    DecodeArgs d = rx_decode_args(cd, n, S, max_sweeps, do_ml);
    const PacketRows pin{nullptr, packets, rx->stage_sym, S + kHdr};
    auto sources = [&](uint32_t *src, uint8_t *er) -> int {
        hipLaunchKernelGGL(fec_rx_sources, dim3(grid_for((int64_t)closes * n)), dim3(kThreads), 0, ctx->stream, (const int32_t *)rx->win.p,
                           rx->stage_er, n, rx->cb, closes, src, er);
        LDPC_HIP_TRY(ctx, hipGetLastError());
        return LDPC_AMD_OK;
    };
    auto gather = [&](int first, int count, uint8_t *sym, uint8_t *er) { return rx_move<true>(rx, pl, packets, first, count, sym, er); };
    int launches = 0;
    if ((rc = rx_decode_slots(ctx, d, o, closes, chunk, fused, pin, sources, gather, &launches))) return rc;
    if ((rc = rx_move<false>(rx, pl, packets, 0, 0, nullptr, nullptr))) return rc;   // (e)
    rx_commit(rx, pl, blocks, consumed);
    ctx->receiver_path = fused ? 1 : 2;
    ctx->receiver_blocks = closes;
    return closes;
}

int ldpc_amd_fec_rx_dev_decode_flush(ldpc_amd_fec_rx_dev *rx, int code, int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps,
                                     int32_t *residual, int32_t *status, uint8_t *erased_out, int32_t *residual_src, int *block_out)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    int rc;
    const RxResults o{out, sweeps, residual, status, erased_out, residual_src};
    if ((rc = rx_decode_check(ctx, rx, "fec_rx_dev_decode_flush", code, max_sweeps, o))) return rc;
    const size_t frame = (size_t)rx->n * rx->S;
    if ((rc = scratch_reserve(ctx, ctx->rx_sym, frame)) || (rc = scratch_reserve(ctx, ctx->rx_er, (size_t)rx->n))) return rc;
    if ((rc = ldpc_amd_fec_rx_dev_flush(rx, (uint8_t *)ctx->rx_sym.p, (uint8_t *)ctx->rx_er.p, block_out)) != 1) return rc;
    DecodeArgs d{};
    d.code = ctx->codes[code]->dev; d.S = rx->S; d.in_rows = rx->n; d.max_sweeps = max_sweeps; d.do_ml = do_ml ? 1 : 0; d.nframes = 1;
    d.sym = (const uint8_t *)ctx->rx_sym.p; d.erased = (const uint8_t *)ctx->rx_er.p; d.out = out;
    d.sweeps = sweeps; d.residual = residual; d.status = status; d.erased_out = erased_out; d.residual_src = residual_src;
    if ((rc = launch_decode(ctx, d))) return rc;
    return 1;
}

int ldpc_amd_fec_receiver_info(ldpc_amd_ctx *ctx, int info[4])
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!info) return set_error(ctx, LDPC_AMD_EINVAL, "fec_receiver_info: info must not be null");
    info[0] = ctx->receiver_path;
    info[1] = (int)std::min<size_t>(ctx->rx_sym.cap, (size_t)INT32_MAX);
    info[2] = ctx->receiver_blocks;
    info[3] = 0;
    return LDPC_AMD_OK;
}

}  // extern "C"

// ---- the multi-flow receiver (include/ldpc_erasure_amd_flows.h) ---------------------------------------------------------
struct ldpc_amd_fec_rx_flows {
    ldpc_amd_ctx *ctx = nullptr;
    int nflows = 0, n = 0, k = 0, S = 0, kd = 0, km = 0;
    // host mirror of every flow's state, as in ldpc_amd_fec_rx_dev
    std::vector<int> cur, next, ccnt, ncnt, cb;
    std::vector<int64_t> dropped;
    int64_t unrouted = 0;           // packets of no flow the mixed calls were given
    uint8_t *stage_sym = nullptr;   // [nflows][2][n][S]
    uint8_t *stage_er = nullptr;    // [nflows][2][n]
    Scratch dense, dest, win, res, slots, order;   // per-call scratch, grown on demand (order: the mixed calls' partition, u32 [P])
    FlowIn *in_dev = nullptr, *in_host = nullptr;      // [nflows]; the host copies are pinned
    FlowTab *tab_dev = nullptr, *tab_host = nullptr;   // [nflows]
    int32_t *res_host = nullptr;    // pinned copy of res
    size_t res_host_cap = 0;
    RxPlaneUpload fl;   // the batch flush: the closed slots' planes on the device, [2 nflows]
};

// What the two-block receiver puts into the multi-flow call skeleton (rx_flows_host.h)
struct FlowsPolicy {
    typedef ldpc_amd_fec_rx_flows Rx;
    static int planes_per_flow(const Rx *) { return 2; }
    static void fill_in(Rx *rx, int f, int64_t begin, int64_t len)
    {
        rx->in_host[f] = FlowIn{begin, len, rx->cur[f], rx->next[f], rx->ccnt[f], rx->ncnt[f]};
    }
    static int launch_headers(Rx *rx, bool aligned4, const uint8_t *packets, const int32_t *flow_of, uint32_t *base, uint32_t *order, int64_t np,
                              int plen, uint32_t *dense)
    {
        hipStream_t st = rx->ctx->stream;
        const int nf = rx->nflows;
        int rc;
        if (order && (rc = demux_launch(rx->ctx, flow_of, np, nf, base, rx->in_dev, order))) return rc;
        const uint32_t *ord = order, *routed = order ? base + nf : nullptr;   // the routed count, as the partition's bases kernel wrote it
        if (order && aligned4) hipLaunchKernelGGL(fec_rx_headers_idx<true>, dim3(grid_for(np)), dim3(kThreads), 0, st, packets, ord, routed, plen, dense);
        else if (order) hipLaunchKernelGGL(fec_rx_headers_idx<false>, dim3(grid_for(np)), dim3(kThreads), 0, st, packets, ord, routed, plen, dense);
        else if (aligned4) hipLaunchKernelGGL(fec_rx_headers<true>, dim3(grid_for(np)), dim3(kThreads), 0, st, packets, np, plen, dense);
        else hipLaunchKernelGGL(fec_rx_headers<false>, dim3(grid_for(np)), dim3(kThreads), 0, st, packets, np, plen, dense);
        return LDPC_AMD_OK;
    }
    static void launch_scan(Rx *rx, const uint32_t *dense, int max_blocks, int32_t *dest, int32_t *res)
    {
        hipLaunchKernelGGL(fec_rx_scan_flows, dim3(rx->nflows), dim3(64), 0, rx->ctx->stream, dense, rx->in_dev, rx->n, rx->kd, rx->km, max_blocks, dest,
                           res);
    }
    static size_t rec_words(int max_blocks) { return (size_t)R_WORDS + (size_t)max_blocks; }
    static bool err(const int32_t *h) { return h[R_ERR] != 0; }
    static int closes(const int32_t *h) { return h[R_CLOSES]; }
    static int64_t consumed(const int32_t *h) { return (int64_t)(((uint64_t)(uint32_t)h[R_CONSUMED_HI] << 32) | (uint32_t)h[R_CONSUMED_LO]); }
    static FlowTab tab_entry(const Rx *rx, int f, int64_t begin, int64_t used, int base, int closes)
    {
        return FlowTab{begin, used, base, closes, rx->cb[f], 0};
    }
    static void launch_slots(Rx *rx)
    {
        hipLaunchKernelGGL(fec_rx_flow_slots, dim3(rx->nflows), dim3(64), 0, rx->ctx->stream, rx->tab_dev, (int32_t *)rx->slots.p);
    }
    static int launch_winners(Rx *rx, const RxFlowsPlan &pl, unsigned gx, int32_t *win)
    {
        ldpc_amd_ctx *ctx = rx->ctx;
        const int nf = rx->nflows;
        hipLaunchKernelGGL(fec_rx_winners_flows, dim3(gx, nf), dim3(kThreads), 0, ctx->stream, (const uint32_t *)rx->dense.p,
                           (const int32_t *)rx->dest.p, rx->tab_dev, rx->n, pl.T, win);
        LDPC_HIP_TRY(ctx, hipGetLastError());
        if (pl.order) {   // a mixed call planned on positions: every winner back to its packet index
            const int64_t cells = ((int64_t)pl.T + 2 * (int64_t)nf) * rx->n;
            hipLaunchKernelGGL(fec_rx_win_order, dim3(grid_for(cells)), dim3(kThreads), 0, ctx->stream, win, cells, pl.order);
            LDPC_HIP_TRY(ctx, hipGetLastError());
        }
        return LDPC_AMD_OK;
    }
    static void launch_move(Rx *rx, const RxFlowsPlan &pl, const uint8_t *packets, bool gather, int first, int count, uint8_t *sym, uint8_t *er,
                            bool v16, int64_t items)
    {
        FlowMoveArgs a{};
        a.packets = packets; a.plen = (int64_t)rx->S + kHdr; a.win = (const int32_t *)rx->win.p; a.tab = rx->tab_dev;
        a.slot_flow = (const int32_t *)rx->slots.p; a.stage_sym = rx->stage_sym; a.stage_er = rx->stage_er;
        a.sym_out = sym; a.er_out = er; a.n = rx->n; a.S = rx->S; a.T = pl.T; a.nflows = rx->nflows; a.first = first; a.count = count;
        const dim3 grid(grid_for(items)), block(kThreads);
        hipStream_t st = rx->ctx->stream;
        if (gather && v16) hipLaunchKernelGGL((fec_rx_move_flows<true, true>), grid, block, 0, st, a);
        else if (gather) hipLaunchKernelGGL((fec_rx_move_flows<true, false>), grid, block, 0, st, a);
        else if (v16) hipLaunchKernelGGL((fec_rx_move_flows<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((fec_rx_move_flows<false, false>), grid, block, 0, st, a);
    }
    static void launch_left(Rx *rx, const RxFlowsPlan &pl, unsigned gx, uint8_t *left)
    {
        hipLaunchKernelGGL(fec_rx_left_flows, dim3(gx, rx->nflows), dim3(kThreads), 0, rx->ctx->stream, (const FlowTab *)rx->tab_dev,
                           (const FlowIn *)rx->in_dev, pl.order, left);
    }
    static void launch_sources(Rx *rx, int T, uint32_t *rows, uint8_t *er)
    {
        hipLaunchKernelGGL(fec_rx_sources_flows, dim3(grid_for((int64_t)T * rx->n)), dim3(kThreads), 0, rx->ctx->stream, (const int32_t *)rx->win.p,
                           rx->stage_er, rx->tab_dev, (const int32_t *)rx->slots.p, rx->n, T, rows, er);
    }
    static void commit_flow(Rx *rx, int f, const int32_t *h, int closes)
    {
        rx->cur[f] = h[R_CUR]; rx->next[f] = h[R_NEXT]; rx->ccnt[f] = h[R_CCNT]; rx->ncnt[f] = h[R_NCNT];
        rx->cb[f] ^= closes & 1;   // :241, once per close
        rx->dropped[f] += (int64_t)(((uint64_t)(uint32_t)h[R_DROPPED_HI] << 32) | (uint32_t)h[R_DROPPED_LO]);
    }
    static void record_info(ldpc_amd_ctx *ctx, bool fused, int T, int, size_t)
    {
        ctx->receiver_path = fused ? 1 : 2;
        ctx->receiver_blocks = T;
    }
    // the batch flush's members: defined with the flush, below
    static int flush_fill(const Rx *rx, int f, int rounds, RxFlushPlan &pl);
    static int flush_gather(Rx *rx, int first, int count, uint8_t *sym, uint8_t *er);
    static int flush_after(Rx *rx, bool fused, int T);
    static void launch_flush_sources(Rx *rx, int T, uint32_t *src, uint8_t *er);
    static void flush_commit_flow(Rx *rx, int f, int count);
    static void record_flush(ldpc_amd_ctx *ctx, int path, int T, int n, int launches, size_t scratch);
};

extern "C" {

int ldpc_amd_fec_rx_flows_create(ldpc_amd_ctx *ctx, int nflows, int n, int k, int S, ldpc_amd_fec_rx_flows **out)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!out || nflows < 1 || nflows > 4096 || n <= 0 || n > 65536 || k <= 0 || k >= n || S <= 0)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rx_flows_create: need 1 <= nflows <= 4096, n <= 65536, 0 < k < n, S >= 1 (nflows=%d n=%d k=%d S=%d)",
                         nflows, n, k, S);
    if ((int64_t)nflows * 2 * n >= ((int64_t)1 << 31) - 2)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rx_flows_create: nflows * 2 * n must be below 2^31 - 2");
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ldpc_amd_fec_rx_flows *rx = new (std::nothrow) ldpc_amd_fec_rx_flows();
    if (!rx) return set_error(ctx, LDPC_AMD_ENOMEM, "fec_rx_flows_create: out of host memory");
    rx->ctx = ctx;
    rx->nflows = nflows; rx->n = n; rx->k = k; rx->S = S;
    rx->kd = k + (int)lround((n - k) * 0.8);   // desired_parity_rx, :54
    rx->km = k + (int)lround((n - k) * 0.2);   // min_parity_rx, :55
    rx->cur.assign(nflows, -1); rx->next.assign(nflows, -1);
    rx->ccnt.assign(nflows, 0); rx->ncnt.assign(nflows, 0); rx->cb.assign(nflows, 0);
    rx->dropped.assign(nflows, 0);
    return rxf_create_buffers<FlowsPolicy>(ctx, rx, "fec_rx_flows_create", out);
}

void ldpc_amd_fec_rx_flows_destroy(ldpc_amd_fec_rx_flows *rx) { rxf_destroy(rx); }

int64_t ldpc_amd_fec_rx_flows_dropped(const ldpc_amd_fec_rx_flows *rx, int flow)
{
    return rx && flow >= 0 && flow < rx->nflows ? rx->dropped[flow] : -1;
}

// ---- the calls: each fills in where its packets are and runs the skeleton (rx_flows_host.h) under its own name -----------------------
int ldpc_amd_fec_rx_flows_push_many(ldpc_amd_fec_rx_flows *rx, const uint8_t *packets, const int64_t *flow_begin, uint8_t *sym_batch,
                                    uint8_t *erased_batch, int *blocks, int *closes, int max_blocks_per_flow, int64_t *consumed)
{
    return rxf_push<FlowsPolicy>(rx, "fec_rx_flows_push_many", packets, RxFlowsSrc{false, flow_begin, nullptr}, 0, sym_batch, erased_batch,
                                 max_blocks_per_flow, RxFlowsOut{blocks, closes, consumed, nullptr, nullptr});
}

int ldpc_amd_fec_rx_flows_push_mixed(ldpc_amd_fec_rx_flows *rx, const uint8_t *packets, const int32_t *flow_of, int64_t P, uint8_t *sym_batch,
                                     uint8_t *erased_batch, int *blocks, int *closes, int max_blocks_per_flow, int64_t *consumed,
                                     int64_t *offered, uint8_t *left)
{
    return rxf_push<FlowsPolicy>(rx, "fec_rx_flows_push_mixed", packets, RxFlowsSrc{true, nullptr, flow_of}, P, sym_batch, erased_batch,
                                 max_blocks_per_flow, RxFlowsOut{blocks, closes, consumed, offered, left});
}

int64_t ldpc_amd_fec_rx_flows_unrouted(const ldpc_amd_fec_rx_flows *rx) { return rx ? rx->unrouted : -1; }

int ldpc_amd_fec_rx_flows_flush(ldpc_amd_fec_rx_flows *rx, int flow, uint8_t *sym_out, uint8_t *erased_out, int *block_out)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    if (flow < 0 || flow >= rx->nflows) return set_error(ctx, LDPC_AMD_EINVAL, "fec_rx_flows_flush: no flow %d (nflows = %d)", flow, rx->nflows);
    const int f = flow;
    if (rx->cur[f] == -1 || (rx->ccnt[f] == 0 && rx->ncnt[f] == 0)) return 0;
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((sym_out && !is_device_ptr(ctx, sym_out)) || (erased_out && !is_device_ptr(ctx, erased_out)))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rx_flows_flush: sym_out / erased_out must be device pointers of device %d", ctx->device);
    const size_t plane = (size_t)rx->n * rx->S, pi = (size_t)f * 2 + (size_t)rx->cb[f];
    uint8_t *ps = rx->stage_sym + pi * plane, *pe = rx->stage_er + pi * rx->n;
    // close_current: hand the current block out, reset its buffer, rotate
    if (sym_out) LDPC_HIP_TRY(ctx, hipMemcpyAsync(sym_out, ps, plane, hipMemcpyDeviceToDevice, ctx->stream));
    if (erased_out) LDPC_HIP_TRY(ctx, hipMemcpyAsync(erased_out, pe, rx->n, hipMemcpyDeviceToDevice, ctx->stream));
    LDPC_HIP_TRY(ctx, hipMemsetAsync(ps, 0, plane, ctx->stream));
    LDPC_HIP_TRY(ctx, hipMemsetAsync(pe, 1, rx->n, ctx->stream));
    if (block_out) *block_out = rx->cur[f];
    rx->cur[f] = rx->next[f];
    rx->next[f] = (rx->next[f] + 1) & 0xff;
    rx->ccnt[f] = rx->ncnt[f];
    rx->ncnt[f] = 0;
    rx->cb[f] ^= 1;
    return 1;
}

// ldpc_amd_fec_rx_dev_decode_many for all flows: ONE launch_decode over the T closed slots (composed: one per chunk of slots).  The
// staging update of all flows is one launch BEHIND the decode, for the reason given there.
int ldpc_amd_fec_rx_flows_decode_many(ldpc_amd_fec_rx_flows *rx, int code, const uint8_t *packets, const int64_t *flow_begin, int max_sweeps,
                                      int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status, uint8_t *erased_out,
                                      int32_t *residual_src, int *blocks, int *closes, int max_blocks_per_flow, int64_t *consumed)
{
    return rxf_decode<FlowsPolicy>(rx, "fec_rx_flows_decode_many", code, packets, RxFlowsSrc{false, flow_begin, nullptr}, 0, max_sweeps, do_ml,
                                   RxResults{out, sweeps, residual, status, erased_out, residual_src}, max_blocks_per_flow,
                                   RxFlowsOut{blocks, closes, consumed, nullptr, nullptr});
}

int ldpc_amd_fec_rx_flows_decode_mixed(ldpc_amd_fec_rx_flows *rx, int code, const uint8_t *packets, const int32_t *flow_of, int64_t P,
                                       int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status,
                                       uint8_t *erased_out, int32_t *residual_src, int *blocks, int *closes, int max_blocks_per_flow,
                                       int64_t *consumed, int64_t *offered, uint8_t *left)
{
    return rxf_decode<FlowsPolicy>(rx, "fec_rx_flows_decode_mixed", code, packets, RxFlowsSrc{true, nullptr, flow_of}, P, max_sweeps, do_ml,
                                   RxResults{out, sweeps, residual, status, erased_out, residual_src}, max_blocks_per_flow,
                                   RxFlowsOut{blocks, closes, consumed, offered, left});
}

int ldpc_amd_fec_rx_flows_decode_flush(ldpc_amd_fec_rx_flows *rx, int flow, int code, int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps,
                                       int32_t *residual, int32_t *status, uint8_t *erased_out, int32_t *residual_src, int *block_out)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    if (flow < 0 || flow >= rx->nflows)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rx_flows_decode_flush: no flow %d (nflows = %d)", flow, rx->nflows);
    int rc;
    const RxResults o{out, sweeps, residual, status, erased_out, residual_src};
    if ((rc = rx_decode_check(ctx, rx, "fec_rx_flows_decode_flush", code, max_sweeps, o))) return rc;
    const size_t frame = (size_t)rx->n * rx->S;
    if ((rc = scratch_reserve(ctx, ctx->rx_sym, frame)) || (rc = scratch_reserve(ctx, ctx->rx_er, (size_t)rx->n))) return rc;
    if ((rc = ldpc_amd_fec_rx_flows_flush(rx, flow, (uint8_t *)ctx->rx_sym.p, (uint8_t *)ctx->rx_er.p, block_out)) != 1) return rc;
    DecodeArgs d{};
    d.code = ctx->codes[code]->dev; d.S = rx->S; d.in_rows = rx->n; d.max_sweeps = max_sweeps; d.do_ml = do_ml ? 1 : 0; d.nframes = 1;
    d.sym = (const uint8_t *)ctx->rx_sym.p; d.erased = (const uint8_t *)ctx->rx_er.p; d.out = out;
    d.sweeps = sweeps; d.residual = residual; d.status = status; d.erased_out = erased_out; d.residual_src = residual_src;
    if ((rc = launch_decode(ctx, d))) return rc;
    return 1;
}

}  // extern "C"

// ---- the batch flush (include/ldpc_erasure_amd_flows_flush.h) -------------------------------------------------------------
// ldpc_amd_fec_rx_flows_flush / _decode_flush for many flows and up to two blocks of each in one call.  The PLAN is the host's: the
// mirror knows every flow's state, so which blocks close, in which order and from which plane is decided without the device
// (flush_replay: the rule of ldpc_amd_fec_rx_flows_flush, replayed on a copy of the flow's state).  The DATA MOVEMENT is all-staged --
// a block that a flush closes got its last packet in an earlier call -- so the decode form is the carried-block case of
// the decode calls for every row: fec_rx_flush_sources writes a staged (or erased) row-source word per symbol and ONE launch_decode
// follows them into the planes; where the decoder has no packets-in form, fec_rx_flush_gather copies the planes into the context's
// scratch, chunk by chunk, as the decode calls do.  fec_rx_flush_reset, ONE launch for all closed planes, stands BEHIND the decode,
// which reads them.  Nothing is read back and nothing waits: the mirror is advanced on the host when everything is enqueued.
// The two calls themselves are rx_flows_host.h's (rxf_flush_many, rxf_decode_flush_many); here are FlowsPolicy's flush members.

// how many blocks `rounds` flushes of flow f close, from its mirror; with out: their numbers and planes
static int flush_replay(const ldpc_amd_fec_rx_flows *rx, int f, int rounds, RxFlushPlan *out)
{
    int cur = rx->cur[f], next = rx->next[f], ccnt = rx->ccnt[f], ncnt = rx->ncnt[f], cb = rx->cb[f], c = 0;
    for (; c < rounds; c++) {
        if (cur == -1 || (ccnt == 0 && ncnt == 0)) break;   // ldpc_amd_fec_rx_flows_flush: nothing open
        if (out) {
            out->blocks.push_back(cur);
            out->planes.push_back(f * 2 + cb);
        }
        cur = next; next = (next + 1) & 0xff; ccnt = ncnt; ncnt = 0; cb ^= 1;
    }
    return c;
}

int FlowsPolicy::flush_fill(const Rx *rx, int f, int rounds, RxFlushPlan &pl) { return flush_replay(rx, f, rounds, &pl); }

// the piece of the plane kernels: the widest of 16, 4, 1 bytes that divides S and that `p` (null: the planes alone) is aligned to
static int flush_piece(int S, const void *p)
{
    if (S % 16 == 0 && ((uintptr_t)p & 15) == 0) return 16;
    if (S % 4 == 0 && ((uintptr_t)p & 3) == 0) return 4;
    return 1;
}

int FlowsPolicy::flush_gather(Rx *rx, int first, int count, uint8_t *sym, uint8_t *er)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int n = rx->n, S = rx->S, W = flush_piece(S, sym);
    const int64_t upp = (int64_t)n * S / W;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((upp + kThreads - 1) / kThreads, 256)), (unsigned)count);
    if (W == 16) hipLaunchKernelGGL(fec_rx_flush_gather<16>, grid, dim3(kThreads), 0, ctx->stream, rx->fl.dev, rx->stage_sym, rx->stage_er, n, S, first, sym, er);
    else if (W == 4) hipLaunchKernelGGL(fec_rx_flush_gather<4>, grid, dim3(kThreads), 0, ctx->stream, rx->fl.dev, rx->stage_sym, rx->stage_er, n, S, first, sym, er);
    else hipLaunchKernelGGL(fec_rx_flush_gather<1>, grid, dim3(kThreads), 0, ctx->stream, rx->fl.dev, rx->stage_sym, rx->stage_er, n, S, first, sym, er);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

// ONE launch for all handed-out planes, behind whatever read them: the gather, or the decode (fused or composed)
int FlowsPolicy::flush_after(Rx *rx, bool, int T)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int n = rx->n, S = rx->S, W = flush_piece(S, nullptr);
    const int64_t upp = (int64_t)n * S / W;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((upp + kThreads - 1) / kThreads, 256)), (unsigned)T);
    if (W == 16) hipLaunchKernelGGL(fec_rx_flush_reset<16>, grid, dim3(kThreads), 0, ctx->stream, rx->fl.dev, rx->stage_sym, rx->stage_er, n, S);
    else if (W == 4) hipLaunchKernelGGL(fec_rx_flush_reset<4>, grid, dim3(kThreads), 0, ctx->stream, rx->fl.dev, rx->stage_sym, rx->stage_er, n, S);
    else hipLaunchKernelGGL(fec_rx_flush_reset<1>, grid, dim3(kThreads), 0, ctx->stream, rx->fl.dev, rx->stage_sym, rx->stage_er, n, S);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

void FlowsPolicy::launch_flush_sources(Rx *rx, int T, uint32_t *src, uint8_t *er)
{
    hipLaunchKernelGGL(fec_rx_flush_sources, dim3(grid_for((int64_t)T * rx->n)), dim3(kThreads), 0, rx->ctx->stream, (const int32_t *)rx->fl.dev,
                       (const uint8_t *)rx->stage_er, rx->n, T, src, er);
}

// the mirror of a listed flow advanced once per closed block (ldpc_amd_fec_rx_flows_flush)
void FlowsPolicy::flush_commit_flow(Rx *rx, int f, int count)
{
    for (int c = 0; c < count; c++) {
        rx->cur[f] = rx->next[f];
        rx->next[f] = (rx->next[f] + 1) & 0xff;
        rx->ccnt[f] = rx->ncnt[f];
        rx->ncnt[f] = 0;
        rx->cb[f] ^= 1;
    }
}

// [2]: the device memory the call used: the plane numbers; with a decode the row flags and the row-source words or the scratch
void FlowsPolicy::record_flush(ldpc_amd_ctx *ctx, int path, int T, int n, int launches, size_t scratch)
{
    size_t bytes = sizeof(int32_t) * (size_t)T;
    if (path != 3) bytes += (path == 1 ? sizeof(uint32_t) * (size_t)T * n : scratch) + (size_t)T * n;
    ctx->flush_info[0] = path; ctx->flush_info[1] = T; ctx->flush_info[2] = (int64_t)bytes; ctx->flush_info[3] = launches;
}

extern "C" {

int ldpc_amd_fec_rx_flows_pending(const ldpc_amd_fec_rx_flows *rx, int32_t *cur_block, int32_t *cur_cnt, int32_t *next_cnt)
{
    if (!rx) return -1;
    int total = 0;
    for (int f = 0; f < rx->nflows; f++) {
        if (cur_block) cur_block[f] = rx->cur[f];
        if (cur_cnt) cur_cnt[f] = rx->ccnt[f];
        if (next_cnt) next_cnt[f] = rx->ncnt[f];
        total += flush_replay(rx, f, 2, nullptr);
    }
    return total;
}

// (the number of rounds is looked at before the list)
static int flush_check_rounds(const ldpc_amd_fec_rx_flows *rx, const char *who, int rounds)
{
    if (!rx) return LDPC_AMD_EINVAL;
    if (rounds < 1 || rounds > 2) return set_error(rx->ctx, LDPC_AMD_EINVAL, "%s: rounds must be 1 or 2 (got %d)", who, rounds);
    return LDPC_AMD_OK;
}

int ldpc_amd_fec_rx_flows_flush_many(ldpc_amd_fec_rx_flows *rx, const int32_t *flows, int nsel, int rounds, uint8_t *sym_batch,
                                     uint8_t *erased_batch, int *blocks, int *closes)
{
    const char *who = "fec_rx_flows_flush_many";
    const int rc = flush_check_rounds(rx, who, rounds);
    return rc ? rc : rxf_flush_many<FlowsPolicy>(rx, who, flows, nsel, rounds, sym_batch, erased_batch, blocks, closes);
}

int ldpc_amd_fec_rx_flows_decode_flush_many(ldpc_amd_fec_rx_flows *rx, int code, const int32_t *flows, int nsel, int rounds, int max_sweeps,
                                            int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status, uint8_t *erased_out,
                                            int32_t *residual_src, int *blocks, int *closes)
{
    const char *who = "fec_rx_flows_decode_flush_many";
    const int rc = flush_check_rounds(rx, who, rounds);
    return rc ? rc : rxf_decode_flush_many<FlowsPolicy>(rx, who, code, flows, nsel, rounds, max_sweeps, do_ml,
                                                        RxResults{out, sweeps, residual, status, erased_out, residual_src}, blocks, closes);
}

int ldpc_amd_fec_flows_flush_info(ldpc_amd_ctx *ctx, int64_t info[4])
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!info) return set_error(ctx, LDPC_AMD_EINVAL, "fec_flows_flush_info: info must not be null");
    for (int i = 0; i < 4; i++) info[i] = ctx->flush_info[i];
    return LDPC_AMD_OK;
}

// ---- the partition on its own (include/ldpc_erasure_amd_flows_mixed.h) ----------------------------------------------------
int64_t ldpc_amd_fec_flows_demux_dev(ldpc_amd_ctx *ctx, const int32_t *flow_of, int64_t P, int nflows, uint32_t *order, int64_t *counts)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (nflows < 1 || nflows > kMaxFlows || P < 0 || P >= ((int64_t)1 << 31))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_flows_demux_dev: need 1 <= nflows <= 4096 and 0 <= P < 2^31 (nflows=%d)", nflows);
    if (P == 0) {
        if (counts) std::fill(counts, counts + nflows, (int64_t)0);
        ctx->demux_tile = kDemuxMinTile;
        ctx->demux_tiles = 0;
        return 0;
    }
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!flow_of || !order || !is_device_ptr(ctx, flow_of) || !is_device_ptr(ctx, order))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_flows_demux_dev: flow_of / order must be device pointers of device %d", ctx->device);
    if (((uintptr_t)flow_of | (uintptr_t)order) & 3) return set_error(ctx, LDPC_AMD_EINVAL, "fec_flows_demux_dev: flow_of / order must be 4-byte aligned");
    int rc;
    if ((rc = demux_reserve(ctx, P, nflows))) return rc;
    int64_t tile, tiles;
    demux_tiling(P, tile, tiles);
    uint32_t *base = (uint32_t *)ctx->demux_tab.p + (size_t)tiles * (size_t)nflows;   // behind the table
    if ((rc = demux_launch(ctx, flow_of, P, nflows, base, (FlowIn *)nullptr, order))) return rc;
    std::vector<uint32_t> h((size_t)nflows + 1);
    LDPC_HIP_TRY(ctx, hipMemcpyAsync(h.data(), base, sizeof(uint32_t) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
    LDPC_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = check_device_error(ctx))) return rc;
    for (int f = 0; counts && f < nflows; f++) counts[f] = (int64_t)(h[f + 1] - h[f]);
    return (int64_t)h[nflows];
}

int ldpc_amd_fec_flows_demux_info(ldpc_amd_ctx *ctx, int64_t info[4])
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!info) return set_error(ctx, LDPC_AMD_EINVAL, "fec_flows_demux_info: info must not be null");
    info[0] = ctx->demux_tile;
    info[1] = ctx->demux_tiles;
    info[2] = (int64_t)ctx->demux_tab.cap;
    info[3] = 0;
    return LDPC_AMD_OK;
}

}  // extern "C"
