/* ldpc_erasure_amd_link.h -- the link between sender and receiver, on the device: a deterministic, counter-based emulator of a
 * channel that loses, delays (and so re-orders), duplicates and damages the packets of a FEC wire, on a fixed-stride packet array
 * and on the trimmed wire (ldpc_erasure_amd_wire_ragged.h).  With it a whole run stays device-resident:
 *   sender -> PLAN + APPLY -> receiver
 * PLAN works out who arrives where and with what damage (it needs no payload), APPLY / APPLY_RAGGED move the bytes.
 * Implemented in csrc/link_dev.hip, same shared library.
 *
 * Reference: the paper names this as its goal -- "Testing the codec over an internet link, which can introduce delay, bursty error
 * patterns and out-of-order packet reception" (Latex/Milcom_2022_ErasureCodes.tex:230); the FPGA's data_in kernel
 * (OpenCL/device/ldpc_erasure_decoder_top.cl:74-110) stops at erasure flags of symbols, as ldpc_amd_synth_erasures_* do.
 *
 * THE MODEL (normative; csrc/link_dev.hip and tools/link_model.py compute exactly this).  A call sees P packets in send order,
 * i = 0 .. P-1; `first` is the position of packet 0 in the link's life and every draw is indexed by g = first + i (64-bit,
 * wrapping), so successive calls with first advanced by P continue one stream of DRAWS: two calls of P1 and P2 packets make the
 * draws of one call of P1 + P2 packets.  PACKETS DO NOT CROSS A CALL BOUNDARY: every packet of a call arrives in that call, the
 * arrival order is worked out inside the call alone.  With the functions of ldpc_erasure_amd_synth.h and t(p) =
 * ldpc_synth_threshold(p):
 *   loss       is an INPUT, lost[i] != 0 (NULL: nothing is lost); make it with ldpc_amd_synth_erasures_uniform / _bursty called
 *              with n = 1, frame0 = first, nframes = P, or bring a trace.
 *   entries    packet i has two virtual entries e = 2i + c: c = 0 the original, c = 1 a copy.
 *              exists(2i) = !lost[i];  exists(2i+1) = !lost[i] && ldpc_synth_bernoulli(seed, LDPC_AMD_LINK_STREAM_DUP, g, t(dup))
 *   delay      delay(e) = (ldpc_synth_u32(seed, LDPC_AMD_LINK_STREAM_DELAY, 2g + c) * (uint64)(window + 1)) >> 32, in 0 .. window
 *   time       time(e) = i + c + delay(e)
 *   order      the existing entries sorted by the pair (time, e); Q = their number <= 2P; entry e arrives at position q(e), its rank
 *   damage     x = ldpc_synth_u64(seed, LDPC_AMD_LINK_STREAM_DAMAGE, 2g + c), r = x >> 32: BADSYM iff r < t(bad_sym), else FOREIGN
 *              iff r < t(bad_sym) + t(foreign) (64-bit sum); a FOREIGN entry's block value is (x >> 8) & 0xff (not the top byte,
 *              which is small exactly when r is below a threshold)
 *   flip       FLIPPED iff c == 1 and LDPC_AMD_LINK_DUP_FLIP is set
 * What damage does to a packet: BADSYM sets the symbol number to 0xFFFF in both halves of the header word (bytes 0, 1, 4, 5) -- the
 * number of the slot ldpc_amd_fec_wire_land_dev makes for a rejected datagram, above any n a code can have, so every receiver drops
 * the packet and counts it; FOREIGN sets the block byte to the drawn value in both halves (bytes 2 and 6); FLIPPED XORs every
 * payload byte (byte 8 on) with 0x5A: the receivers keep the last copy of a duplicate, the flip shows which one that was.
 * time(e) lies in [i, i + 1 + window]: an entry of packet i changes places only with entries of packets i' with
 * |i' - i| <= window + 1, which makes the order a local, exact computation -- no atomics, the same bytes on every run.
 *
 * Errors: negative LDPC_AMD_E* codes, text in ldpc_amd_last_error(ctx); everything the host can check is checked before anything
 * is enqueued, a refused call touches nothing and leaves the context usable.  A NULL context is LDPC_AMD_EINVAL before any
 * device is touched.  The calls are asynchronous on the context's stream; nothing is read back, nothing synchronises.
 */
#ifndef LDPC_ERASURE_AMD_LINK_H
#define LDPC_ERASURE_AMD_LINK_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* stream ids of the link's draws (ldpc_erasure_amd_synth.h has 1 .. 6) */
#define LDPC_AMD_LINK_STREAM_DUP 16u    /* duplicate draw of packet g: idx = g             */
#define LDPC_AMD_LINK_STREAM_DELAY 17u  /* delay draw of entry (g, c): idx = 2g + c        */
#define LDPC_AMD_LINK_STREAM_DAMAGE 18u /* damage draw of entry (g, c): idx = 2g + c       */

#define LDPC_AMD_LINK_MAX_WINDOW 4096 /* (256 + 2 (window + 1)) * 8 bytes of LDS per workgroup: 67.6 KB of the CU's 160 KB */

typedef struct {
    uint64_t seed, first;
    int32_t window, flags;
    double dup, bad_sym, foreign;
} ldpc_amd_link_params;

/* ldpc_amd_link_params.flags */
#define LDPC_AMD_LINK_DUP_FLIP 1
/* fate bits (low byte of a uint16; high byte = the FOREIGN block value, else 0) */
#define LDPC_AMD_LINK_COPY 1
#define LDPC_AMD_LINK_BADSYM 2
#define LDPC_AMD_LINK_FOREIGN 4
#define LDPC_AMD_LINK_FLIPPED 8

/* PLAN: src_out[q] = i and fate_out[q] = the fate of the entry that arrives at position q, for every q < Q, each position written
 * exactly once; *count_out = Q; nothing at or beyond Q is written.  cap, the entries of src_out and fate_out, must be at least
 * 2 * npackets (cap >= 2P): overflow is then impossible.  npackets == 0 writes *count_out = 0 and nothing else.
 * LDPC_AMD_EINVAL: params NULL, npackets < 0 or >= 2^30, cap < 2 * npackets, window outside 0 .. LDPC_AMD_LINK_MAX_WINDOW, a
 * probability outside [0, 1] (or no number), bad_sym + foreign > 1, flags with an unknown bit, a NULL or host pointer where a device
 * pointer of the context's device is due (lost may be NULL), src_out not 4-byte, fate_out not 2-byte or count_out not 8-byte
 * aligned, an output overlapping lost or another output. */
int ldpc_amd_fec_link_plan_dev(ldpc_amd_ctx *ctx, const ldpc_amd_link_params *params, int64_t npackets,
                               const uint8_t *lost /* device [P], may be NULL */, int32_t *src_out /* device [cap] */,
                               uint16_t *fate_out /* device [cap] */, int64_t cap, int64_t *count_out /* device [1] */);

/* APPLY: packets_out[q] = damage(packets[src[q]], fate[q]) for q < *count, the gather of a fixed-stride packet array.  count is
 * read on the device (a value outside 0 .. cap counts as the nearer end); the host knows only cap.  No slot at or beyond *count is
 * written.  A src[q] outside 0 .. npackets-1 can only come from a caller's own plan: slot q then becomes the BADSYM slot of zeros
 * (bytes 0, 1, 4, 5 = 0xFF, every other byte 0), nothing is read for it, and flow_of_out[q] = -1, a packet of no flow.  A fate
 * with both damage bits gets both.  flow_of_out[q] = flow_of[src[q]]: a mixed multi-flow wire keeps its flow numbers, the result
 * goes straight into ldpc_amd_fec_rx_flows_decode_mixed.  flow_of_out is NULL iff flow_of is.  packets may be NULL only when
 * npackets == 0.  cap == 0 returns OK and touches nothing.
 * LDPC_AMD_EUNSUP: S not a multiple of 4, below 8 or above 2^30.  LDPC_AMD_EINVAL: npackets or cap negative or >= 2^31, a NULL or
 * host pointer where a device pointer of the context's device is due, exactly one of flow_of / flow_of_out NULL, packets,
 * packets_out, src, flow_of or flow_of_out not 4-byte, fate not 2-byte or count not 8-byte aligned, an output overlapping an input
 * or the other output. */
int ldpc_amd_fec_link_apply_dev(ldpc_amd_ctx *ctx, const uint8_t *packets /* device [P][8+S] */, int64_t npackets, int S,
                                const int32_t *src /* device [cap] */, const uint16_t *fate /* device [cap] */,
                                const int64_t *count /* device [1] */, int64_t cap, uint8_t *packets_out /* device [cap][8+S] */,
                                const int32_t *flow_of /* device [P], may be NULL */,
                                int32_t *flow_of_out /* device [cap], NULL iff flow_of is */);

/* APPLY on a trimmed wire: datagram q of the output = the bytes of datagram src[q] of the input, bytes[offset[s] .. offset[s+1]),
 * with the damage of fate[q] applied inside the copy, for q < *count.  The boundaries live on the device and are vetted there
 * exactly as ldpc_amd_fec_wire_land_dev vets them, but for the upper bound 8 + S (no S is given): datagram s is good iff
 * 0 <= offset[s] <= offset[s+1] <= nbytes and offset[s+1] - offset[s] >= 8.  A datagram with bad boundaries, one shorter than 8
 * bytes and a src[q] outside 0 .. npackets-1 go out with length 0; no byte is read for them.  offset_out[q] = the exclusive prefix
 * sum of the lengths, q = 0 .. Q; offset_out[Q] and *total_out (may be NULL) hold the total.  Nothing of offset_out beyond
 * entry Q and no byte of bytes_out at or beyond the total is written; every byte below it is written once.  bytes and bytes_out may
 * lie at any alignment; the loads are aligned 4-byte ones, so the up to 3 bytes that share an aligned dword with the first or last
 * byte of a datagram may be touched (as land touches them).  bytes_cap, the size of bytes_out, must be at least 2 * nbytes: a plan
 * of ldpc_amd_fec_link_plan_dev names every packet at most twice and cannot overflow it.  A caller's own plan can: a datagram that
 * would end beyond bytes_cap is then NOT WRITTEN, offset_out and the total still count it -- a total above bytes_cap says so.
 * bytes may be NULL only when nbytes == 0, src and fate only when cap == 0 (offset_out[0] and the total are then 0).
 * LDPC_AMD_EINVAL: npackets, cap, nbytes or bytes_cap negative, npackets or cap >= 2^31, bytes_cap < 2 * nbytes, a NULL or host
 * pointer where a device pointer of the context's device is due, src not 4-byte, fate not 2-byte, offset, count, offset_out or
 * total_out not 8-byte aligned, an output overlapping an input or another output. */
int ldpc_amd_fec_link_apply_ragged_dev(ldpc_amd_ctx *ctx, const uint8_t *bytes /* device, any alignment */, int64_t nbytes,
                                       const int64_t *offset /* device [P+1] */, int64_t npackets, const int32_t *src /* device [cap] */,
                                       const uint16_t *fate /* device [cap] */, const int64_t *count /* device [1] */, int64_t cap,
                                       uint8_t *bytes_out /* device [bytes_cap], any alignment */, int64_t bytes_cap,
                                       int64_t *offset_out /* device [cap+1] */, int64_t *total_out /* device [1], may be NULL */);

/* info[0]: bytes of device scratch held for the context's link calls (tile sums); info[1]: packets of the last plan; info[2]: of the
 * last apply; info[3]: of the last apply_ragged.  The scratch is kept in the link's own table, by context, for the life of the
 * process: a context created where a closed one was takes its block over. */
int ldpc_amd_fec_link_info(ldpc_amd_ctx *ctx, int64_t info[4]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_LINK_H */
