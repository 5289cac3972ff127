/* ldpc_erasure_amd_wire_ragged.h -- the trimmed wire: the last hop between the fixed-stride packet arrays of the senders and
 * receivers and a wire that carries datagrams of different lengths.  TRIM cuts every packet of a packet array to the bytes that
 * have to be sent and lays them back to back; LAND takes datagrams that lie back to back (an RDMA receive queue, a recvmmsg
 * ring, a capture file) with their boundaries and puts every one into its slot of a packet array, zero fill included.  With
 * them the variable-length path is device-resident end to end:
 *   datagrams -> pack -> encode -> TRIM -> wire bytes -> LAND -> decode -> unpack -> datagrams
 * (pack / unpack: ldpc_erasure_amd_datagrams.h).  Implemented in csrc/wire_ragged_dev.hip, same shared library.
 *
 * Reference: the sender reads every packet's length from the packet itself, OpenCL/device/
 * ldpc_erasure_encoder_VITA_in_UDP_out.cl:140-162 (packetLen = (din & 0xffff) + 2); trim does the same with the length prefix of
 * the datagram symbol, so the host needs no per-packet table on the sending side.
 *
 * Errors: negative LDPC_AMD_E* codes, text in ldpc_amd_last_error(ctx); everything the host can check is checked before anything
 * is enqueued, a refused call touches nothing and leaves the context usable.  A NULL context is LDPC_AMD_EINVAL before any
 * device is touched.  The calls are asynchronous on the context's stream; nothing is read back, nothing synchronises.  S is a
 * multiple of 4, at least 8 and at most 2^30, else LDPC_AMD_EUNSUP.  npackets < 2^31; every byte address is a 64-bit one.
 */
#ifndef LDPC_ERASURE_AMD_WIRE_RAGGED_H
#define LDPC_ERASURE_AMD_WIRE_RAGGED_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* states of a datagram, ldpc_amd_fec_wire_land_dev */
#define LDPC_AMD_WIRE_LANDED 0   /* slot p = the datagram's bytes, then zeros */
#define LDPC_AMD_WIRE_REJECTED 1 /* bad boundaries or length: slot p = eight bytes 0xFF, then zeros; no byte of it was read */

/* packets [P][8+S] -> bytes_out = the first len[p] bytes of every packet back to back in packet order, offset_out[P+1] = the
 * exclusive prefix sum of the lengths (offset_out[P] is the total).  len[p] is taken on the device from the packet alone: with
 * i = the symbol number of its header (bytes 0..1, little-endian), a packet with i < k is a source row and L = the little-endian
 * uint32 at payload bytes 0..3 its length prefix: len = 8 + 4 + L if L <= S - 4, else 8 + S (a row that is no datagram symbol
 * is sent whole); a packet with i >= k is a repair row, len = 8 + S.  For packets made by ldpc_amd_fec_dgram_pack_dev and any
 * sender of the library (single-flow or multi-flow, either order) this is ldpc_amd_fec_dgram_wire_len entry for entry.
 * NOT CHECKED: that the bytes cut off are zero.  Trim is for packets whose source rows pack made; of any other source row
 * whose first four bytes happen to read as L <= S - 4 it sends the first 12 + L bytes and nothing says so.
 * No byte of bytes_out at or beyond the total is written.  cap, the size of bytes_out, must be at least P * (8 + S): overflow
 * is then impossible.  npackets == 0 returns OK and touches nothing.
 * LDPC_AMD_EUNSUP: S as above.  LDPC_AMD_EINVAL: npackets < 0 or >= 2^31, k < 1, cap too small, a NULL or host pointer where
 * a device pointer of the context's device is due, packets not 4-byte or offset_out not 8-byte aligned, an output overlapping
 * the input or the other output. */
int ldpc_amd_fec_wire_trim_dev(ldpc_amd_ctx *ctx, const uint8_t *packets /* device [P][8+S] */, int64_t npackets, int k, int S,
                               uint8_t *bytes_out /* device [cap] */, int64_t cap, int64_t *offset_out /* device [P+1] */);

/* Datagram p = bytes[offset[p] .. offset[p+1]) -> slot p of packets [P][8+S].  The offsets live on the DEVICE (offset_out of trim
 * is a valid input as it is; a host receive loop uploads its own), so the host cannot vet them and the kernel does: datagram p
 * is LANDED iff 0 <= offset[p] <= offset[p+1] <= nbytes and 8 <= offset[p+1] - offset[p] <= 8 + S, and slot p is then its
 * bytes followed by zeros up to 8 + S.  Every other datagram is REJECTED: no byte of bytes is read for it and slot p becomes
 * eight bytes 0xFF followed by zeros -- a header with symbol number 0xFFFF, above any n a code can have (n <= 65534), so every
 * receiver of the library drops the slot and counts it in its `dropped`.  state[p] = LDPC_AMD_WIRE_LANDED / _REJECTED; state may
 * be NULL.  Every byte of packets is written exactly once: no memset is needed in front.  (The receivers take their first block
 * number from the first packet they are given, dropped or not -- ldpc_amd_fec_rx_push -- and a rejected slot reads as block 255:
 * a receiver that has seen nothing yet should not be handed one as its very first packet.)
 * READS: no byte outside bytes[0 .. nbytes) is needed for the result; the loads are aligned 4-byte ones, so the up to 3 bytes
 * that share an aligned dword with the first or the last byte of a landed datagram may be touched (as pack touches them).
 * bytes may be NULL only when nbytes == 0 (every datagram is then REJECTED).  npackets == 0 returns OK and touches nothing.
 * LDPC_AMD_EUNSUP: S as above.  LDPC_AMD_EINVAL: npackets < 0 or >= 2^31, nbytes < 0, bytes NULL with nbytes > 0, a NULL or
 * host pointer where a device pointer of the context's device is due, packets not 4-byte or offset not 8-byte aligned,
 * packets or state overlapping each other, bytes or offset. */
int ldpc_amd_fec_wire_land_dev(ldpc_amd_ctx *ctx, const uint8_t *bytes /* device, any alignment */, int64_t nbytes,
                               const int64_t *offset /* DEVICE [P+1] */, int64_t npackets, int S,
                               uint8_t *packets /* device [P][8+S] */, uint8_t *state /* device [P], may be NULL */);

/* info[0]: bytes of device scratch the context holds for trim (lengths, tile sums); info[1]: packets of the last trim;
 * info[2]: packets of the last land. */
int ldpc_amd_fec_wire_ragged_info(ldpc_amd_ctx *ctx, int64_t info[3]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_WIRE_RAGGED_H */
