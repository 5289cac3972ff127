/* ldpc_erasure_amd_frames.h -- the frame format (sym [F][n][S], erased [F][n]) on the OUTPUT side of the LDPC decoder and on
 * the INPUT side of the Reed-Solomon comparator.  Implemented in csrc/api.cpp and csrc/kernels.hip, same shared library.
 *
 * The library takes erasures as one flag per symbol; these two calls also give them back and accept them where the older entry
 * points do not:
 *   ldpc_amd_decode_frames      ldpc_amd_decode_batch + the flags of the symbols that are STILL unknown afterwards.  The
 *                               reference keeps them: Matlab's Msg holds -1 there (My_LDPC_HybridML_NonBinary_Erasure_Decoder.m:9,129),
 *                               the FPGA symbol_type carries is_erasure on the way out as well as in, and the FPGA frame
 *                               criterion asks exactly "are the first k symbols known" (ldpc_erasure_decoder_perf_tests.cl:213-220).
 *   ldpc_amd_rs_decode_frames   the loop step of ReedSolomonErasureCodes.m:64-91 -- keep the first k received positions, decode,
 *                               or return zeros when fewer than k arrived -- on the same (sym, erased) buffers the LDPC decoder,
 *                               the synthetic channels and the device reassembler speak.  The payload is read in place: there
 *                               is no gathered copy.
 *
 * Pointer conventions are those of ldpc_erasure_amd.h: host pointers are staged and the call is synchronous; with
 * LDPC_AMD_DEVICE_PTRS every data pointer is a device pointer and the call is asynchronous on the context's stream (a host
 * pointer for erased_out / residual_src / received / status is then refused with LDPC_AMD_EINVAL).  Errors: negative
 * LDPC_AMD_E* codes, text in ldpc_amd_last_error(ctx); a refused call leaves the context usable.
 */
#ifndef LDPC_ERASURE_AMD_FRAMES_H
#define LDPC_ERASURE_AMD_FRAMES_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ldpc_amd_decode_batch plus two outputs, either of which may be NULL; with both NULL the call IS ldpc_amd_decode_batch (the
 * same launches, nothing more stored).  out, sweeps, residual and status are byte for byte those of ldpc_amd_decode_batch in
 * every case; LDPC_AMD_INPLACE is accepted exactly where ldpc_amd_decode_batch accepts it.
 *
 *   erased_out   [nframes][n], 0 / 1: 1 exactly when out[f][j] is neither a received nor a recovered symbol
 *   residual_src [nframes]: how many of those have an index < k (0 = the source part of the frame is complete)
 *
 *   status[f]                      erased_out[f]                           residual_src[f]
 *   0 MP_DONE, 1 ML_SOLVED         all zero                                0
 *   3 ML_SKIPPED, 2 ML_RANKDEF     the erasures left after the sweeps      those with index < k
 *
 * For status 2 and 3, the flags of a frame sum to residual[f].
 * DEVIATION from the reference for status 2 (rank-deficient residual system): Matlab writes the partially reduced right-hand
 * side back unconditionally (...Decoder.m:127), so no -1 is left in Msg and the oracle's out_erased is cleared.  The bytes at
 * those positions (kept here, byte-exact) are NOT the transmitted symbols, so a flag that says "known" would be wrong: the
 * flags of such a frame stay those the sweeps left.
 * The payload of erased input symbols is ignored.  status may be NULL (the call then keeps the words it needs internally). */
int ldpc_amd_decode_frames(ldpc_amd_ctx *ctx, int code, int S, int64_t nframes, const uint8_t *sym, const uint8_t *erased,
                           int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status,
                           uint8_t *erased_out, int32_t *residual_src, unsigned flags);

#define LDPC_AMD_RS_ST_DECODED 0
#define LDPC_AMD_RS_ST_SHORT 1 /* fewer than k symbols received: msg is all zero (ReedSolomonErasureCodes.m:78,80) */

/* (n, k) of a handle ldpc_amd_rs_create returned. */
int ldpc_amd_rs_info(ldpc_amd_ctx *ctx, int rs, int *n, int *k);

/* Per block: P = the ascending positions with erased == 0.  |P| >= k: msg is what ldpc_amd_rs_decode_batch returns for
 * recv_idx = P[0:k], recv_val = sym[P[0:k]] (nothing received beyond the k-th symbol is read, ReedSolomonErasureCodes.m:81;
 * nor is the payload of an erased symbol), status 0.  Otherwise msg is all zero, status 1.  received[b] = |P|.
 *   sym [nblocks][n][S], erased [nblocks][n], msg [nblocks][k][S]; received, status [nblocks], each may be NULL.
 * S: 1 or a multiple of 16 (or, with symbol unit 4, see ldpc_erasure_amd_words.h), like ldpc_amd_rs_decode_batch.
 * The selection cannot produce malformed positions: after this call
 * ldpc_amd_rs_bad_blocks reports 0. */
int ldpc_amd_rs_decode_frames(ldpc_amd_ctx *ctx, int rs, int S, int64_t nblocks, const uint8_t *sym, const uint8_t *erased,
                              uint8_t *msg, int32_t *received, int32_t *status, unsigned flags);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_FRAMES_H */
