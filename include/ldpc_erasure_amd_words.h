/* ldpc_erasure_amd_words.h -- word-sized symbols: a context that accepts any symbol length S that is a multiple of 4 bytes.
 * Implemented in csrc/api.cpp (the switch) and csrc/kernels.hip, csrc/ml_kernel.inc, csrc/rs_kernels.inc (the kernels' word form),
 * same shared library.
 *
 * Reference: the sender takes its payload length from the VRT header in 32-bit words, OpenCL/device/
 * ldpc_erasure_encoder_VITA_in_UDP_out.cl:141-162 -- packetLen = (din & 0xffff) + 2, payloadSize = packetLen * 4; the one length
 * it names, 367 words, is a 1460-byte symbol behind the 8-byte FEC header.  A datagram cut to an MTU (1400, 1460) is a multiple of
 * 4 and not of 16.
 *
 * The switch is per context and is NOT a knob (a knob never changes a result; this changes which inputs are accepted): it does
 * not appear in ldpc_amd_knobs and no environment variable sets it.  With unit 16 -- the default -- nothing changes.  With unit 4
 *   - S == 1 or S a multiple of 4 that is at least 16 is accepted; anything else (4, 8, 12 included) is refused with
 *     LDPC_AMD_EUNSUP, "S must be 1 or a multiple of 4 that is at least 16 (got %d)";
 *   - a multiple of 16 runs exactly the kernels it runs with unit 16;
 *   - any other S runs the kernels' word form: the same B-byte row pieces, the last piece of a row moved back so that it ends
 *     with the row (it overlaps its neighbour; the bytes in the overlap are computed twice, to the same value), every access a
 *     4-byte one.  The bytes are those of the same call with every row zero-padded to the next multiple of 16;
 *   - with LDPC_AMD_DEVICE_PTRS the symbol arrays must be 4-byte aligned (LDPC_AMD_EINVAL otherwise).
 * Covered: ldpc_amd_decode_batch, ldpc_amd_decode_frames (LDPC_AMD_INPLACE included), ldpc_amd_encode_batch,
 * ldpc_amd_rs_encode_batch, ldpc_amd_rs_decode_batch, ldpc_amd_rs_decode_frames, ldpc_amd_fec_encode_packets_dev,
 * ldpc_amd_fec_rx_dev_decode_many and ldpc_amd_fec_rx_dev_decode_flush (a device receiver reads the unit of its context when it
 * decodes; ldpc_amd_fec_rx_dev_create takes any S as before).  The contexts of a multi-device group keep unit 16.
 */
#ifndef LDPC_ERASURE_AMD_WORDS_H
#define LDPC_ERASURE_AMD_WORDS_H

#include "ldpc_erasure_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* unit: 16 (default) or 4.  With 4, every entry point of this context that takes a symbol length S accepts
 * S == 1 or any multiple of 4 that is >= 16.  Anything else: LDPC_AMD_EINVAL, the context keeps its unit. */
int ldpc_amd_set_symbol_unit(ldpc_amd_ctx *ctx, int unit);
int ldpc_amd_get_symbol_unit(ldpc_amd_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_WORDS_H */
