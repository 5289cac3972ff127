/* ldpc_erasure_amd_sender.h -- the fused sender: source symbols in GPU memory straight to FEC wire packets, the codeword never
 * stored as an array of its own.  Implemented in csrc/wire_dev.hip (the call) and csrc/kernels.hip (the packet-output form of
 * the persistent encoder), same shared library.
 *
 * Reference: the sender is one kernel, OpenCL/device/ldpc_erasure_encoder_VITA_in_UDP_out.cl:84-129,168-211 -- it computes a
 * parity symbol, writes the FEC header and emits the packet; the block number advances once per frame (:134).  The packet layout
 * and the header are those of ldpc_erasure_amd_wire.h; VITA-49 framing and UDP headers are not produced.
 *
 * Two paths, the same bytes.  FUSED: one launch of the encoder that stores every row at its place in the packet array and the
 * header beside it (per frame it reads k S and writes n (8 + S) bytes).  COMPOSED: ldpc_amd_encode_batch into a scratch of
 * the context, then ldpc_amd_fec_packetize_dev, in chunks of frames so that the scratch never exceeds 256 MiB.  The fused path is
 * taken whenever the same ldpc_amd_encode_batch call would run the persistent packet encoder (S a multiple of 128 for the
 * built-in codes), the knob LDPC_AMD_ENC_PKT is 1, the packets pointer is 8-byte and the source pointer 16-byte aligned;
 * ldpc_amd_fec_sender_info says which one ran.
 *
 * Every data pointer is a device pointer of the context's device.  Errors: negative LDPC_AMD_E* codes, text in
 * ldpc_amd_last_error(ctx); a refused call leaves the context usable.
 */
#ifndef LDPC_ERASURE_AMD_SENDER_H
#define LDPC_ERASURE_AMD_SENDER_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_wire.h"

#ifdef __cplusplus
extern "C" {
#endif

/* source [nframes][k][S] -> packets [nframes*n][8+S] in transmission order: byte for byte
 * ldpc_amd_fec_packetize_dev(ldpc_amd_encode_batch(source)).  Device pointers of the context's device only
 * (host pointers: LDPC_AMD_EINVAL, as in the wire_dev header).  Asynchronous on the context's stream.
 * S: 1 or a multiple of 16 or, with symbol unit 4, see ldpc_erasure_amd_words.h -- there every word-sized S takes the fused
 * path, the source pointer 4-byte aligned -- (else LDPC_AMD_EUNSUP, the encoder's rule); code not in triangle form: LDPC_AMD_EUNSUP;
 * unknown handle: LDPC_AMD_ENOCODE; nframes == 0: OK, nothing touched; source and packets must not overlap (EINVAL).
 * Block number of frame f = (block0 + f) & 0xff, symbol number = row, header = ldpc_amd_fec_header_pack. */
int ldpc_amd_fec_encode_packets_dev(ldpc_amd_ctx *ctx, int code, int S, int64_t nframes, const uint8_t *source,
                                    unsigned fec_class, unsigned block0, uint8_t *packets);

/* info[0]: path of the last ldpc_amd_fec_encode_packets_dev call of this context (0 none yet, 1 fused kernel, 2 composed);
 * info[1]: bytes of codeword scratch the context holds for the composed path; info[2..3]: 0, reserved. */
int ldpc_amd_fec_sender_info(ldpc_amd_ctx *ctx, int info[4]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_SENDER_H */
