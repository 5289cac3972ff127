/* ldpc_erasure_amd_receiver.h -- the fused receiver: FEC wire packets in GPU memory straight to decoded frames, the received
 * symbols never stored as an array of their own.  Implemented in csrc/wire_dev.hip (the calls) and csrc/kernels.hip (the
 * packets-in form of the scatter decoder), same shared library.
 *
 * Reference: the receiver is one kernel, OpenCL/device/ldpc_erasure_decoder_with_reordering_logic.cl:44-141,214-243 -- it sorts
 * the packets into its two block buffers and decodes a block when it closes.  The packet layout, the header and the rule by which
 * blocks open and close are those of ldpc_erasure_amd_wire.h / ldpc_erasure_amd_wire_dev.h.
 *
 * Two paths, the same bytes.  FUSED: the plan of ldpc_amd_fec_rx_dev_push_many is made on the headers, then one small kernel
 * writes, per closed block and symbol, an erasure flag and a 32-bit word that says where the row lies (payload of packet p, row i
 * of the receiver's staging planes, or nowhere), and the decoder's streaming phase fetches every row from there: per frame it
 * reads the received n S bytes once and writes n S.  COMPOSED: the closed blocks are gathered into a scratch of the context and
 * decoded from it, in chunks of blocks so that the scratch never exceeds 256 MiB.  The fused path is taken whenever the same
 * ldpc_amd_decode_frames call would run the scatter kernels (S a multiple of 16, column degree at most 16, LDPC_AMD_APPLY not
 * gather, a launch plan exists -- with 2 n bytes of LDS more than that call needs), the knob LDPC_AMD_RX_PKT is 1 and the packets
 * pointer is 8-byte aligned; ldpc_amd_fec_receiver_info says which one ran.
 *
 * Every data pointer is a device pointer of the receiver's context (host pointers: LDPC_AMD_EINVAL, as in the wire_dev header).
 * Errors: negative LDPC_AMD_E* codes, text in ldpc_amd_last_error(ctx).  A refused call leaves the receiver's state and the
 * context untouched and usable.
 */
#ifndef LDPC_ERASURE_AMD_RECEIVER_H
#define LDPC_ERASURE_AMD_RECEIVER_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_wire_dev.h"

#ifdef __cplusplus
extern "C" {
#endif

/* packets -> closed blocks -> decoded frames, in one call.  Everything ldpc_amd_fec_rx_dev_push_many followed by
 * ldpc_amd_decode_frames on its sym_batch / erased_batch would return, byte for byte, without the caller ever holding
 * (or, on the fused path, the library ever writing) a [B][n][S] array of received symbols.
 * Returns the number of closed blocks; *consumed and blocks[] are final when the call returns, the decoded arrays of slots
 * 0 .. closes - 1 are written asynchronously on the context's stream, slots at or beyond closes are not touched.  The receiver
 * is afterwards in the state ldpc_amd_fec_rx_dev_push_many would have left (ldpc_amd_fec_rx_dev_dropped included): the two
 * calls and the two flushes can be mixed freely on one receiver.
 * The caller must keep `packets` alive and unchanged until the context's stream has passed the call: the decoder reads the
 * payloads from it (as ldpc_amd_fec_rx_dev_push_many's gather does).
 * code: a handle of the receiver's context whose (n, k) are the receiver's (else LDPC_AMD_EINVAL; unknown handle:
 * LDPC_AMD_ENOCODE).  The decoder's own refusals pass through: S neither 1 nor a multiple of 16 (LDPC_AMD_EUNSUP; or,
 * with symbol unit 4, see ldpc_erasure_amd_words.h),
 * max_sweeps < 1 (LDPC_AMD_EINVAL).  max_blocks < 1: LDPC_AMD_EINVAL.  npackets == 0: returns 0, nothing is touched. */
int ldpc_amd_fec_rx_dev_decode_many(ldpc_amd_fec_rx_dev *rx, int code, const uint8_t *packets, int64_t npackets,
                                    int max_sweeps, int do_ml,
                                    uint8_t *out,            /* [max_blocks][n][S]  device */
                                    int32_t *sweeps, int32_t *residual, int32_t *status,      /* [max_blocks] device, may be NULL */
                                    uint8_t *erased_out, int32_t *residual_src,               /* device, may be NULL */
                                    int *blocks /* host, may be NULL */, int max_blocks, int64_t *consumed);

/* end of stream: ldpc_amd_fec_rx_dev_flush + decode of that one block (composed; a single frame).  Returns 1 and the block's
 * number in *block_out, or 0 when no block is open. */
int ldpc_amd_fec_rx_dev_decode_flush(ldpc_amd_fec_rx_dev *rx, int code, int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps,
                                     int32_t *residual, int32_t *status, uint8_t *erased_out, int32_t *residual_src, int *block_out);

/* info[0]: path of the last decode_many of this context (0 none yet, 1 fused, 2 composed); info[1]: bytes of received-symbol
 * scratch the context holds for the composed path; info[2]: blocks the last call decoded; info[3]: 0, reserved */
int ldpc_amd_fec_receiver_info(ldpc_amd_ctx *ctx, int info[4]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_RECEIVER_H */
