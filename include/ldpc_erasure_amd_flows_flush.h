/* ldpc_erasure_amd_flows_flush.h -- the multi-flow receiver's batch flush: the open blocks of many flows closed, handed out
 * (and decoded) by one call.  Implemented in csrc/wire_dev.hip, same shared library.
 *
 * Reference: a stream's close rule only closes a block when the NEXT block has received more than 10 or more than 100 packets
 * (ldpc_erasure_amd_wire.h, OpenCL/device/ldpc_erasure_decoder_with_reordering_logic.cl:139), so a stream that ends or pauses
 * keeps up to two blocks open.  ldpc_amd_fec_rx_flows_flush / _decode_flush (ldpc_erasure_amd_flows.h) close ONE block of ONE
 * flow per call.  The calls of this header close up to two blocks of every selected flow at once: the plan is made on the host
 * from the object's mirror of the flows' states, the decode form runs ONE decoder launch over all T blocks.
 *
 * CONTRACT.
 *   Equality with the loop.  For each selected flow, in list order, a call does exactly what `rounds` successive
 * ldpc_amd_fec_rx_flows_flush / _decode_flush calls on that flow would do: the same blocks in the same order, every byte, flag
 * and result word the same, the same state afterwards.  That includes the EMPTY current block, which is handed out with every
 * symbol erased when only the next block holds packets, and a flow with nothing open, which gives closes = 0.
 *   Slot order.  Output slots are dense in list order: the blocks of list entry j are the slots closes[0] + ... + closes[j-1]
 * onward, in closing order, and blocks[] follows the same order.  The calls return the total T; slots at or beyond T are not
 * touched.
 *   Untouched and reset.  A flow that is not selected is not touched in any byte.  The staging planes of every closed block are
 * reset to symbols 0 and flags 1 by ONE launch behind the decode (or the gather) on the context's stream.
 *   Host-only plan.  The calls neither synchronise nor read anything back: blocks and closes are final when a call returns,
 * device arrays are written asynchronously on the context's stream.
 *   Atomic refusals.  Everything is validated and every scratch reserved before any state changes: a refused call leaves every
 * flow, the object and the context as they were.  LDPC_AMD_EINVAL: a NULL object (before any device is touched; pending: -1);
 * rounds outside 1..2; nsel outside 0..nflows with a non-NULL list; a flow number out of range or given twice; a NULL output
 * array or a host pointer where a device pointer is required; a code whose (n, k) are not the object's.  Otherwise the refusals
 * of ldpc_amd_fec_rx_flows_decode_flush and the decoder's own pass through unchanged (the word-symbol rules of
 * ldpc_erasure_amd_words.h included).  nsel == 0 or T == 0 returns 0 (closes[] zero) and touches nothing else.
 *
 * The decode form is FUSED -- no array of received symbols is written: the packets-in decoder takes every row from the staging
 * planes through its row-source words (ldpc_erasure_amd_receiver.h) -- where ldpc_amd_fec_rx_dev_decode_many would be fused for
 * the same code, S and knobs and S is a multiple of 16; else COMPOSED through the context's received-symbol scratch of at most
 * 256 MiB, in chunks of slots, one decoder launch per chunk.  Word-sized symbols take the composed form.
 */
#ifndef LDPC_ERASURE_AMD_FLOWS_FLUSH_H
#define LDPC_ERASURE_AMD_FLOWS_FLUSH_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_flows.h"

#ifdef __cplusplus
extern "C" {
#endif

/* State of every flow, from the host mirror: no device work.  Each array is host [nflows], may be NULL.
 * cur_block[f] = -1 for a flow that has not started (its next block is cur_block[f] + 1 modulo 256 otherwise); cur_cnt / next_cnt
 * = packets the current / the next block took so far.  Returns the number of blocks a full drain (flows = NULL, rounds = 2) would
 * close now. */
int ldpc_amd_fec_rx_flows_pending(const ldpc_amd_fec_rx_flows *rx, int32_t *cur_block, int32_t *cur_cnt, int32_t *next_cnt);

/* push form: close up to `rounds` (1 or 2) blocks of every selected flow, hand them out as push_many hands out closed blocks */
int ldpc_amd_fec_rx_flows_flush_many(ldpc_amd_fec_rx_flows *rx, const int32_t *flows /* host [nsel], NULL = all flows, nsel ignored */,
                                     int nsel, int rounds, uint8_t *sym_batch, uint8_t *erased_batch /* device, nsel*rounds slots */,
                                     int *blocks /* host [nsel*rounds], may be NULL */, int *closes /* host [nsel], may be NULL */);

/* decode form: the same blocks, decoded by ONE decoder launch (composed: one per chunk of the 256 MiB scratch).  out and the
 * result arrays hold nsel*rounds slots; sweeps .. residual_src may be NULL. */
int ldpc_amd_fec_rx_flows_decode_flush_many(ldpc_amd_fec_rx_flows *rx, int code, const int32_t *flows, int nsel, int rounds,
                                            int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status,
                                            uint8_t *erased_out, int32_t *residual_src, int *blocks, int *closes);

/* info[0] path of the last *_flush_many that closed a block (0 none, 1 fused, 2 composed, 3 push form), [1] blocks T,
 * [2] scratch bytes the call used, [3] decoder launches */
int ldpc_amd_fec_flows_flush_info(ldpc_amd_ctx *ctx, int64_t info[4]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_FLOWS_FLUSH_H */
