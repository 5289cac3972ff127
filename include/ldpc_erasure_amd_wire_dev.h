/* ldpc_erasure_amd_wire_dev.h -- device-resident FEC wire path: the packetiser and the two-buffer reassembler of
 * include/ldpc_erasure_amd_wire.h for packets and frames that are already in GPU memory.  Implemented in
 * csrc/wire_dev.hip, same shared library.
 *
 * Reference: the sender writes the FEC headers in a kernel, OpenCL/device/ldpc_erasure_encoder_VITA_in_UDP_out.cl:84-129,
 * 168-211; the receiver reassembles in a kernel in front of the decoder,
 * OpenCL/device/ldpc_erasure_decoder_with_reordering_logic.cl:44-141,214-243.  The rule, its three stated deviations and
 * the packet layout are those of ldpc_erasure_amd_wire.h: every function here produces the same bytes as its host
 * counterpart (ldpc_amd_fec_packetize, ldpc_amd_fec_rx_push_many / _flush / _dropped) on the same stream.
 *
 * Every data pointer is a device pointer of the context's device; a host pointer (pageable or pinned) is refused with
 * LDPC_AMD_EINVAL -- the host functions cover host data.  All data movement is enqueued on the context's stream and is
 * ordered before later work on it.  Errors: negative LDPC_AMD_E* codes, text in ldpc_amd_last_error(ctx).
 * Limits: n <= 65536, 0 < k < n, any S >= 1, npackets < 2^31 per call.  The tuned path is S % 16 == 0 (payload 8-byte
 * aligned in a packet of stride 8 + S, 16-byte aligned in a frame row); every other S takes a byte-wise path.
 */
#ifndef LDPC_ERASURE_AMD_WIRE_DEV_H
#define LDPC_ERASURE_AMD_WIRE_DEV_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_wire.h"

#ifdef __cplusplus
extern "C" {
#endif

/* frames [nframes][n][S] -> packets [nframes * n][8 + S]; bytes identical to ldpc_amd_fec_packetize.  Asynchronous. */
int ldpc_amd_fec_packetize_dev(ldpc_amd_ctx *ctx, const uint8_t *frames, int64_t nframes, int n, int S,
                               unsigned fec_class, unsigned block0, uint8_t *packets);

/* A receiver bound to one context (destroy it before the context).  It holds the two codeword buffers on the device. */
typedef struct ldpc_amd_fec_rx_dev ldpc_amd_fec_rx_dev;
int ldpc_amd_fec_rx_dev_create(ldpc_amd_ctx *ctx, int n, int k, int S, ldpc_amd_fec_rx_dev **rx);
void ldpc_amd_fec_rx_dev_destroy(ldpc_amd_fec_rx_dev *rx);
/* Same contract as ldpc_amd_fec_rx_push_many; packets / sym_batch / erased_batch are device pointers.  Returns the number
 * of closed blocks (>= 0), *consumed and blocks[] (host array, may be NULL) synchronously; the payload movement into
 * sym_batch / erased_batch is enqueued on the context's stream.  packets may be NULL when npackets == 0. */
int ldpc_amd_fec_rx_dev_push_many(ldpc_amd_fec_rx_dev *rx, const uint8_t *packets, int64_t npackets,
                                  uint8_t *sym_batch, uint8_t *erased_batch, int *blocks, int max_blocks,
                                  int64_t *consumed);
/* End of stream, like ldpc_amd_fec_rx_flush: 1 = the current block was closed into sym_out [n][S] / erased_out [n]
 * (device pointers, may be NULL) and *block_out (host); 0 = nothing left.  Decided on the host, no synchronisation. */
int ldpc_amd_fec_rx_dev_flush(ldpc_amd_fec_rx_dev *rx, uint8_t *sym_out, uint8_t *erased_out, int *block_out);
/* Packets dropped so far (block neither current nor next, or symbol number >= n); -1 for a NULL receiver. */
int64_t ldpc_amd_fec_rx_dev_dropped(const ldpc_amd_fec_rx_dev *rx);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_WIRE_DEV_H */
