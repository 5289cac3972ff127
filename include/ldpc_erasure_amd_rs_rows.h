/* ldpc_erasure_amd_rs_rows.h -- the Reed-Solomon erasure decoder on rows in place.  Included by ldpc_erasure_amd_rs_wire.h, whose
 * section THE DECODER ON ROWS IN PLACE states the contract; implemented in csrc/rs_wire_dev.hip, same shared library.
 *
 * A block's n rows are not handed over as a frame: one 32-bit SOURCE WORD per (block, symbol) says where the row lies --
 *     p < 2^31                       the payload of packet p:  packets + p * (8 + S) + 8
 *     LDPC_AMD_ROW_STAGED | i        row i of the staging rows: stage + i * S
 *     LDPC_AMD_ROW_ERASED            erased: nothing is fetched
 * -- the words the windowed receivers write for their packets-in LDPC decoders.  The same packet or staged row may be named by any
 * number of words.  A word that names a packet >= npackets or a staged row >= nstage_rows counts as erased: no row outside the two
 * arrays is ever fetched.
 */
#ifndef LDPC_ERASURE_AMD_RS_ROWS_H
#define LDPC_ERASURE_AMD_RS_ROWS_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_AMD_ROW_STAGED 0x80000000u
#define LDPC_AMD_ROW_ERASED 0xFFFFFFFFu

/* src [nblocks][n] source words, packets [npackets][8 + S], stage [nstage_rows][S] -> msg [nblocks][k][S], received and status
 * [nblocks], erased_out [nblocks][n] (the flags after vetting).  All device pointers; packets / stage may be NULL with a count of 0;
 * received, status and erased_out may each be NULL.  See THE DECODER ON ROWS IN PLACE in ldpc_erasure_amd_rs_wire.h. */
int ldpc_amd_rs_decode_rows_dev(ldpc_amd_ctx *ctx, int rs, int S, int64_t nblocks, const uint32_t *src, const uint8_t *packets,
                                int64_t npackets, const uint8_t *stage, int64_t nstage_rows, uint8_t *msg, int32_t *received,
                                int32_t *status, uint8_t *erased_out);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_RS_ROWS_H */
