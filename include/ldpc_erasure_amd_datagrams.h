/* ldpc_erasure_amd_datagrams.h -- datagrams of any length in front of the sender and behind the receiver: a length-carrying
 * symbol format, a device call that packs datagrams into the source array of ldpc_amd_fec_encode_packets_dev
 * (ldpc_erasure_amd_sender.h) and its multi-flow form, a device call that cuts the delivered datagrams back out of what
 * ldpc_amd_decode_frames / ..._decode_many / ..._decode_flush_many return, and the host arithmetic that says how many bytes of
 * each wire packet have to be transmitted.  Implemented in csrc/datagram_dev.hip, same shared library.
 *
 * Reference: the sender reads every packet's length from the packet itself, OpenCL/device/
 * ldpc_erasure_encoder_VITA_in_UDP_out.cl:140-162 (packetLen = (din & 0xffff) + 2, num_longs_used recomputed per packet); its
 * two packet kinds are context packets of 28 words and data packets of 367 words.  VRT headers are not parsed here: the length
 * is given by the caller and travels inside the protected symbol, so that the length of a lost datagram is recovered with it.
 *
 * THE FORMAT.  A datagram symbol is a row of S bytes, S a multiple of 4 and at least 8:
 *   bytes 0..3        the datagram's length L, a little-endian uint32 (the byte order of the FEC header), 0 <= L <= S - 4
 *   bytes 4..4+L-1    the datagram
 *   every other byte  zero
 * L == 0 is a FILLER, a row that carries no datagram; the caller may supply fillers (a datagram of length 0) and pack completes
 * the last frame with them.  Datagram i of a call is row i of source [F][k][S], F = ceil(N / k).  The repair symbols are whatever
 * the encoder makes of these rows, so a recovered source row describes its own length.
 *
 * Errors: negative LDPC_AMD_E* codes, text in ldpc_amd_last_error(ctx); everything is checked on the host before anything is
 * enqueued, a refused call touches nothing and leaves the context usable.  A NULL context is LDPC_AMD_EINVAL before any device
 * is touched.  Both device calls are asynchronous on the context's stream; neither reads anything back nor synchronises (pack
 * waits for a staging slot only when two earlier calls are still in flight).
 */
#ifndef LDPC_ERASURE_AMD_DATAGRAMS_H
#define LDPC_ERASURE_AMD_DATAGRAMS_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_AMD_DGRAM_PREFIX_BYTES 4

/* states of a row, ldpc_amd_fec_dgram_unpack_dev */
#define LDPC_AMD_DGRAM_DELIVERED 0 /* 1 <= L <= S - 4: the datagram is in bytes_out */
#define LDPC_AMD_DGRAM_FILLER 1    /* L == 0 */
#define LDPC_AMD_DGRAM_LOST 2      /* the row's erased flag is set: the decoder did not recover it; its prefix is not read */
#define LDPC_AMD_DGRAM_MALFORMED 3 /* L > S - 4: not a datagram symbol; nothing is copied */

/* Datagram i = bytes[offset[i] .. offset[i+1]), at any byte alignment -> row i of source [F][k][S]; returns F = ceil(ndgrams / k).
 * Every byte of source is written exactly once (the zero fill and the filler rows of the last frame included): no memset is
 * needed in front.  offset is a HOST array of ndgrams + 1 entries; it is staged in pinned memory, so it is free when the call
 * returns and two calls may be in flight.  ndgrams == 0 returns 0 and touches nothing.
 * LDPC_AMD_EUNSUP: S not a multiple of 4 or below 8.  LDPC_AMD_EINVAL: ndgrams < 0, k < 1, offset NULL, an offset negative or
 * decreasing, a length above S - 4 (the text names the first such index), F * k >= 2^31, bytes (needed when offset[ndgrams] >
 * offset[0]) or source not a device pointer of the context's device, source not 4-byte aligned, bytes overlapping source. */
int64_t ldpc_amd_fec_dgram_pack_dev(ldpc_amd_ctx *ctx, const uint8_t *bytes /* device */, const int64_t *offset /* host [ndgrams+1] */,
                                    int64_t ndgrams, int k, int S, uint8_t *source /* device [F][k][S] */);

/* Rows 0..k-1 of every frame of frames [B][n][S] (out and erased_out of the decode calls; erased NULL = nothing erased) ->
 * state[B*k] (LDPC_AMD_DGRAM_*), offset_out[B*k+1] = the exclusive prefix sum in row order of L over the DELIVERED rows (the
 * last entry is the total), bytes_out = the delivered datagrams back to back in row order.  No byte of bytes_out at or beyond
 * the total is written.  cap, the size of bytes_out, must be at least B * k * (S - 4): overflow is then impossible.
 * nframes == 0 returns OK and touches nothing.
 * LDPC_AMD_EUNSUP: S as above.  LDPC_AMD_EINVAL: nframes < 0, k < 1, n < k, B * k >= 2^31, cap too small, a NULL or host
 * pointer where a device pointer is due, frames not 4-byte or offset_out not 8-byte aligned, an output overlapping an input or
 * another output. */
int ldpc_amd_fec_dgram_unpack_dev(ldpc_amd_ctx *ctx, const uint8_t *frames /* device [B][n][S] */,
                                  const uint8_t *erased /* device [B][n], may be NULL */, int64_t nframes, int n, int k, int S,
                                  uint8_t *bytes_out /* device [cap] */, int64_t cap, int64_t *offset_out /* device [B*k+1] */,
                                  uint8_t *state /* device [B*k] */);

/* Host arithmetic only -- no context, no device.  Packet f * n + i of the sender's output for the source pack makes of these
 * offsets needs wire_len[f * n + i] bytes on the wire: 8 + 4 + L for a source row (12 for a filler), 8 + S for a repair row.
 * Every byte of the packet behind that is zero, so a receive path that zero-fills each landed datagram to the stride 8 + S
 * reproduces the packet array exactly.  wire_len may be NULL.  Returns F * n, or LDPC_AMD_EINVAL (ndgrams < 0, offset NULL,
 * k < 1, n < k, S not a multiple of 4 or below 8, an offset negative or decreasing, a length above S - 4, F * n >= 2^31). */
int64_t ldpc_amd_fec_dgram_wire_len(int64_t ndgrams, const int64_t *offset, int n, int k, int S, int32_t *wire_len /* host [F*n] */);

/* info[0]: bytes of device scratch the context holds for the two calls (pack's offsets; unpack's lengths and tile sums);
 * info[1]: bytes of pinned staging; info[2]: rows (F * k) of the last pack; info[3]: rows (B * k) of the last unpack. */
int ldpc_amd_fec_dgram_info(ldpc_amd_ctx *ctx, int64_t info[4]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_DATAGRAMS_H */
