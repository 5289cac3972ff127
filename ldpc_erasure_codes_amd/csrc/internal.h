// internal.h -- shared between the C-ABI translation unit and the HIP kernel translation units.
// Not installed; the public interface is include/ldpc_erasure_amd.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/ldpc_erasure_amd.h"
#include "../../include/ldpc_erasure_amd_frames.h"

namespace ldpc_amd {

// ---------------------------------------------------------------------------------------------
// GF(2^8), primitive polynomial x^8+x^6+x^5+x^4+1 = 0x171 (369).  The reference fixes it at
// Matlab/ErasureCodes_NonBinaryLDPCSim.m:70 ([1 0 1 1 1 0 0 0 1], MSB first) and ships the resulting
// tables in Matlab/GF_256_add_mult_inv_tables.mat; tests compare ldpc_amd_gf_tables() with that file.
// ---------------------------------------------------------------------------------------------
constexpr int kPrimPoly = 0x171;

struct GfHost {
    uint8_t log[256];   // log[0] unused (0)
    uint8_t exp[512];   // exp[i] = alpha^(i mod 255)
    uint8_t inv[256];   // inv[0] = 0
    uint8_t mul(uint8_t a, uint8_t b) const { return (a && b) ? exp[log[a] + log[b]] : 0; }
};
const GfHost &gf_host();

// Per-coefficient byte-permute tables for the packed multiply (see gf256_dev.h): 8 dwords per coefficient.
void build_mul3_tables(uint32_t *tab /* [256*8] */);

// ---------------------------------------------------------------------------------------------
// Device view of one LDPC code
// ---------------------------------------------------------------------------------------------
struct DevCode {
    int n, k, m, nnz;
    int maxdeg;   // largest row degree
    int maxcoldeg;  // largest column degree (width of the per-frame padded source->target edge lists)
    int degpad;   // template bucket the kernels are instantiated for (8, 14, 16 or 24) >= maxdeg
    int mpad;     // m rounded up to a multiple of 64
    const uint32_t *row_ptr;  // [m+1]
    const uint32_t *edges;    // [nnz]  col | coef << 16 | log(coef) << 24   (CSR order, ascending cols)
    const uint16_t *ell_col;  // [degpad][mpad]  transposed padded rows, 0xFFFF = none
    const uint8_t *ell_logc;  // [degpad][mpad]  log(coef)
    const uint8_t *ell_coef;  // [degpad][mpad]  coef
    const uint32_t *ell_pk;   // [degpad][mpad]  col | log(coef) << 16 (S = 1 kernel: one LDS read per neighbour)
    const uint16_t *rx_off;   // [mpad / 64][degpad][64]  col * 2, padding n * 2: byte offset of the neighbour's 16-bit key word (peel_relax.inc;
                              // chunk-major: the entries of a check are a compile-time stride apart, the lanes of a chunk read consecutive ones)
    const uint8_t *rx_logc;   // [mpad / 64][degpad][64]  log(coef), same order
    const uint8_t *enc_invc;  // [m]  inverse of the coefficient each static encode step divides by
    const uint32_t *cell;     // [n][1 << cdw_shift]  column lists: check | coef << 16, 0xFFFFFFFF = none
    int cdw_shift;            // log2 of the padded column-list width (>= maxcoldeg)
    // static encode schedule (all parity symbols erased): rows sorted by dependency level
    const uint32_t *enc_steps;   // [m] row | (k+row) << 16
    const uint16_t *enc_lvlend;  // [enc_nlevels+1], [L] = end offset of level L, [0] = 0
    int enc_nlevels;
    const uint32_t *enc_src;     // [n][1 << cdw_shift] static symbol -> (slot * 128 | coef << 24) lists of the encoder (LDS offset of the slot's 128-byte piece)
    const uint16_t *enc_order;   // [k] source symbols ordered by the number of checks they feed (most first; index order within)
    const uint32_t *enc_lst;     // [enc_lst_n] the enc_src lists of the parity symbols, compact, in schedule order (level phase of the encoder)
    const uint16_t *enc_lst_off; // [m + 1] step -> first word of its list
    int enc_lst_n;               // 0: not available (more than 65534 words)
    // Grouped static encode schedule (round 4; DESIGN.md section 4.2 "encoder: levels collapsed offline").  The parity triangle's
    // dependency levels (27 for (2040,1530), 100 for (4080,3060)) are a chain of barriers in which the workgroup streams nothing.
    // The schedule is static per code, so the host collapses consecutive levels into GROUPS: a step of a group does not wait for
    // the in-group parities it depends on but PULLS their raw accumulators with composite coefficients
    //     val_r = inv_r * (acc_r ^ XOR_a c_ra * acc_a),   c_ra = sum over the dependency paths a -> r of prod (h * inv)
    // (GF(256) products are associative and distributive: the same bytes), and an in-group parity is not scattered into in-group
    // accumulators.  One barrier per group; a step pulls at most ENC_CAP accumulators.
    const uint32_t *encg_steps;   // [m] row | (k+row) << 16, sorted by group
    const uint16_t *encg_lvlend;  // [encg_nlevels + 1] end offsets of the groups
    const uint8_t *encg_invc;     // [m]
    const uint32_t *encg_src;     // [n][1 << cdw_shift] like enc_src, slots of the grouped order, in-group parity edges left out
    const uint32_t *encg_ent;     // [encg_ent_n] per step: its pull entries, then its scatter entries (slot * 128 | coef << 24)
    const uint16_t *encg_ent_off; // [m + 1]
    const uint8_t *encg_npull;    // [m] how many of a step's entries are pulls
    int encg_nlevels;             // number of groups, 0: no grouped schedule
    int encg_ent_n;
};

struct HostCode {
    int n = 0, k = 0, m = 0, nnz = 0, maxdeg = 0;
    std::vector<uint32_t> row_ptr;
    std::vector<uint16_t> cols;
    std::vector<uint8_t> coefs;
    DevCode dev{};
    int enc_info[5] = {0, 0, 0, 0, 0};   // levels of the plain static schedule, groups, pull entries, scatter entries, longest pull list
    std::vector<void *> allocs;
};

struct HostRs {
    int n = 0, k = 0;
    std::vector<uint8_t> g;  // [k][n] systematic generator
    uint8_t *d_g = nullptr;  // device copy, [k][n]
    uint8_t *d_pt = nullptr; // device copy of the parity part transposed: [n-k][k]
};

// Tuning / diagnostic knobs.  The defaults are what is shipped.  They are read from the environment
// (LDPC_AMD_<NAME>) ONCE, by ldpc_amd_init, and can be changed per context with ldpc_amd_configure: nothing on the call path
// looks at the process environment (a C-ABI library must not depend on getenv in a multi-threaded host).
struct Knobs {
    int apply_gather = 0;        // APPLY=gather: packet kernel in gather form (A/B baseline)
    int scatter_b = 256;         // SCATTER_B: bytes of every row per packet-kernel workgroup (256, 128, 64)
    int scatter_tiers = 2;       // SCATTER_TIERS: 1 = single tier
    int scatter_nt = 1;          // SCATTER_NT: non-temporal row loads / stores
    int scatter_xcd = 1;         // SCATTER_XCD: slices of a frame placed on one XCD
    int scatter_dyn = 1;         // SCATTER_DYN: 1 LDS counter, 0 fixed stride, 2 compacted list, 3 sorted list, 4 list sorted inside 64-row windows
    int scatter_r = 2;           // SCATTER_R: row pieces in flight per lane group, tier 1 (1, 2, 4)
    int scatter_r2 = 3;          // SCATTER_R2: ... tier 2 (2, 3, 4)
    int scatter_lists = 0;       // SCATTER_LISTS: the relaxation's schedules carry the steps' column lists (set-up of the packet kernel: one global round trip
                                 // instead of two).  Measured: packet kernels unchanged (3.143 / 4.327 / 6.439 against 3.138 / 4.334 / 6.442 ms), peel +0.005...0.06: off
    int scatter_pairs = 1;       // SCATTER_PAIRS: the relaxation's schedules group the levels in pairs (one barrier per pair, second halves pull); 0: plain levels
    int scatter_xl = 1;          // SCATTER_XL: the level phase's lists are translated to accumulator addresses at set-up (0: inside every level)
    int scatter_t2b = 256;       // SCATTER_T2B: bytes of every row per TIER-2 workgroup (256: one workgroup per CU; 128: two)
    int peel_wpb = 0;            // PEEL_WPB: frames per peel workgroup (0 = auto)
    int peel_gt = -1;            // PEEL_GT: S = 1 kernel reads the code tables from global memory (-1 = auto; a code whose tables do not fit the LDS takes them from there whatever this says)
    int enc_persist = 1;         // ENC_PERSIST: packet encoder as persistent workgroups (tables and lists set up once per workgroup); 0: one workgroup per (frame, slice)
    int scatter_t2p = 2;         // SCATTER_T2P: tier 2 -- consecutive pieces of a frame per work item (1, 2, 4, 8): the frame's set-up is done once per item
    int scatter_t2p_force = 0;   // SCATTER_T2P_FORCE: 1 = SCATTER_T2P pieces per item whatever the length of the tier-2 list (tests)
    int peel_relax = 1;          // PEEL_RELAX: S = 1 decode (and the pattern-only runs) by time-stamp relaxation (peel_relax.inc); 0: the serial per-solve loop
    int ml_solve = 1;            // ML_SOLVE: 1 solve schedules + solve kernel, 0 solve inside the ML kernel, 2 emit only (diagnostic)
    int ml_dbg = 0;              // ML_DBG: diagnostic build only
    int ml_solve_b = 128;        // ML_SOLVE_B: bytes of every row per solve-kernel workgroup
    long long ml_arena_words = 0;   // ML_ARENA_WORDS: size of the schedule arena in 64-bit words (0 = auto)
    int ml_threads = 0;          // ML_THREADS: threads of the ML kernel's workgroup (0 = 1024 / ML_PACK)
    int ml_pi = 1;               // ML_PI: packets -- the fast path (ml_pi.inc: peel on + inactivation) before the exact elimination.  1: verified
                                 // (frames that fail the consistency test are redone exactly: the reference's bytes on ANY input); 2: not
                                 // verified (the reference's bytes when the received symbols are a codeword with erasures); 0: exact only
    int ml_pi_adaptive = 1;      // ML_PI_ADAPTIVE: skip the fast path's launches for a batch when the previous batch had no residual frame
    int ml_pi_imax = 256;        // ML_PI_IMAX: fast path -- frames that need more inactivations than this go to the exact elimination
    int ml_pi_wgs = 0;           // ML_PI_WGS: fast path -- at most this many workgroups (0: one per CU's LDS share)
    int ml_pi_waves = 4;         // ML_PI_WAVES: fast path -- at most this many wavefronts (frames) per workgroup
    int ml_pi_lds = 160;         // ML_PI_LDS: KB of LDS per fast-path workgroup (160: one workgroup of up to four frames per CU)
    int ml_overlap_prio = 0;     // ML_OVERLAP_PRIO: 1 = that second stream has the lowest priority (measured slower: 5.67 against 5.45 ms on cfg 3)
    int ml_overlap = 2;          // ML_OVERLAP: packets -- the factorisation runs on a second stream beside the packet kernel; 0 = behind it
    int ml_pack = 2;             // ML_PACK: ML-kernel workgroups per CU (1, 2, 3, 4): 1024 / P threads and 160 KB / P of LDS each
    int enc_clist = 1;           // ENC_CLIST: encoder -- the level phase reads the parity symbols' lists from LDS (compact copy); 0: from global memory
    int enc_b = 128;             // ENC_B: encoder piece size (128: two workgroups per CU; 256: the decoder's plan)
    int enc_list = 0;            // ENC_LIST: encoder streams the source rows in the order of their column degree
    int enc_group = 1;           // ENC_GROUP: encoder runs the grouped (level-collapsed) static schedule when the code has one; 0: level by level
    int enc_pkt = 1;             // ENC_PKT: ldpc_amd_fec_encode_packets_dev -- the encoder writes the wire packets itself where it has that form (the persistent
                                 // scatter encoder); 0: always encode into a scratch, then packetise (DESIGN.md section 7 has the two numbers)
    int rx_pkt = 1;              // RX_PKT: ldpc_amd_fec_rx_dev_decode_many -- the decoder fetches its rows from the wire packets itself where it has that form (the
                                 // scatter kernels); 0: always gather the closed blocks into a scratch, then decode (DESIGN.md section 7 has the two numbers)
    int enc_cap = 8;             // ENC_CAP: read when a code is REGISTERED -- a step of the grouped schedule pulls at most this many accumulators (0: no grouped schedule)
    int rs_generic = 0;          // RS=generic: RS decode always through the generic LDS kernel
    int rs_vw = 0;               // RS_VW: dwords per lane of the packet RS kernel (0 = auto = 1; 2 and 4 where S allows)
    int host_pipeline = 1;       // HOST_PIPELINE: chunked upload / compute / download pipeline for large host buffers
    long fpga_chunk = 65536;     // FPGA_CHUNK: frames per chunk of the streamed FPGA-harness run
    long chunk_s1 = 65536;       // CHUNK_S1: S = 1 decode -- frames per launch of a long batch (packets always 16384: their schedules are per-frame workspaces).
                                 // Every launch drains the device once: 65536 (4080,3060) frames 2.233 ms in four launches, 2.082 in one (tools/ab_chunk_s1.py)
};
// key: "LDPC_AMD_SCATTER_B" or "SCATTER_B" (case-insensitive); value nullptr or "" restores the default.  0 = OK, -1 = unknown key / bad value.
int knob_set(Knobs &k, const char *key, const char *value);
bool knobs_from_env(Knobs &k, std::string *rejected);   // false: *rejected = "LDPC_AMD_X=value" of the first value a knob refused

// Growable device scratch
struct Scratch {
    void *p = nullptr;
    size_t cap = 0;
};

// Pinned host staging of a table that is copied to the device on the context's stream: two slots used in turn, each with the event of
// its last copy, so that a slot is never rewritten under a copy in flight (two calls enqueued back to back are both right).
// pinned_ring_acquire / pinned_ring_commit / pinned_ring_free below.
struct PinnedRing {
    void *slot[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0};
    hipEvent_t event[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
    unsigned calls = 0;
    size_t bytes() const { return cap[0] + cap[1]; }
};

// The packet senders of wire_dev.hip, and what the context keeps of the last call of each that sent something
enum TxKind { kTxPlain, kTxFlows, kTxIlv, kTxFlowsIlv, kTxRs, kTxKinds };
struct TxLast {
    int path = 0;        // 0 none yet, 1 fused kernel, 2 composed
    int64_t count = 0;   // its frames (kTxRs: blocks)
};

}  // namespace ldpc_amd

struct ldpc_amd_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t aux_ml = nullptr;                      // packets: the ML factorisation beside the packet kernel (created on first use)
    hipEvent_t ml_events[2] = {nullptr, nullptr};      // fork / join of that stream
    hipStream_t aux_in = nullptr, aux_out = nullptr;   // host-pointer pipeline: H2D / D2H streams (created on first use)
    hipEvent_t pipe_events[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // ... and its events (created once)
    std::string err;
    std::vector<ldpc_amd::HostCode *> codes;
    std::vector<ldpc_amd::HostRs *> rs;
    // workspaces
    ldpc_amd::Scratch sched;    // per-frame schedules (packet path)
    ldpc_amd::Scratch schedlists;  // ... the steps' column lists in schedule order (relaxation schedules)
    ldpc_amd::Scratch schedpull;   // ... their per-step records when the levels come in pairs (16 bytes per step)
    ldpc_amd::Scratch mlws;     // ML stage matrices
    ldpc_amd::Scratch mlstate;  // residual erasure masks of the frames handed to the ML stage
    ldpc_amd::Scratch mlops;    // packets: arena of the ML stage's solve schedules
    ldpc_amd::Scratch mlrec;    // packets: [ML-list slot][8] u32 schedule records
    ldpc_amd::Scratch mllist;   // [1 + nframes] int32: count, frame ids
    ldpc_amd::Scratch biglist;  // [1 + nframes] int32: frames with many steps (scatter tier 2)
    ldpc_amd::Scratch encctr;   // persistent encoder: ring of (item counter, workgroups done) pairs, self-resetting
    unsigned enc_launches = 0;
    ldpc_amd::Scratch stage_in, stage_er, stage_out, stage_i32;  // host-pointer staging
    ldpc_amd::Scratch stage_fr;                                   // ... of the frames calls' extra outputs
    bool ml_head_valid = false;                   // a packet-mode ML stage has copied its demand there at least once
    unsigned long long *ml_head_host = nullptr;   // pinned: arena words the last packet-mode ML stage asked for
    int *dev_err_host = nullptr;   // pinned, device-visible: error bits set by kernels (check_device_error turns them into LDPC_AMD_EHIP)
    size_t ml_arena_words = 0;  // current size of the solve-schedule arena (64-bit words), grown on demand
    void *pin = nullptr;        // pinned host bounce block of the small-call path
    size_t pin_cap = 0;
    ldpc_amd::Scratch rsws;
    ldpc_amd::Scratch rsbad;    // int: malformed blocks of the last RS decode (decoded to zeros)
    ldpc_amd::Scratch rssel;    // RS from frames: [nblocks] int32 symbols received, then [nblocks][k] u16 the first k received positions
    ldpc_amd::Scratch frstatus; // decode_frames without a status array: the status words the finalise kernel reads
    ldpc_amd::Scratch sender_cw;   // the packet senders' composed paths: codewords of one chunk of frames (at most 256 MiB)
    // the last call of every packet sender that sent something, by ldpc_amd::TxKind: never written on a refusal or for a call of no
    // frames (ldpc_amd_fec_sender_info, _sender_flows_info, _sender_ilv_info, _sender_flows_ilv_info, _rs_sender_info)
    ldpc_amd::TxLast tx_last[ldpc_amd::kTxKinds];
    // the descriptor-driven senders (all but kTxPlain): the frames' descriptors on the device (16 bytes each, the multi-flow senders'
    // flow table behind them; the stream orders a call's copy behind the kernels of the call before), and their pinned staging
    ldpc_amd::Scratch txf_desc;
    ldpc_amd::PinnedRing txf_ring;
    // fec_dgram_pack_dev / fec_dgram_unpack_dev (datagram_dev.hip): pack's offsets on the device and their pinned staging; unpack's
    // per-row lengths and per-tile sums
    ldpc_amd::Scratch dgram_off, dgram_len;
    ldpc_amd::PinnedRing dgram_ring;
    int64_t dgram_rows[2] = {0, 0};   // rows of the last pack, of the last unpack (ldpc_amd_fec_dgram_info)
    ldpc_amd::Scratch wire_len;       // fec_wire_trim_dev (wire_ragged_dev.hip): the per-tile sums, then the per-packet lengths
    int64_t wire_packets[2] = {0, 0};   // packets of the last trim, of the last land (ldpc_amd_fec_wire_ragged_info)
    ldpc_amd::Scratch rx_sym;      // fec_rx_dev_decode_many, composed path: received symbols of one chunk of closed blocks (at most 256 MiB)
    ldpc_amd::Scratch rx_er;       // ... both paths: erasure flags of the closed blocks, [closes][n]
    ldpc_amd::Scratch rx_src;      // ... fused path: row-source words of the closed blocks, [closes][n] u32 (PacketRows)
    int receiver_path = 0;         // ... path of the last call: 0 none yet, 1 fused, 2 composed (ldpc_amd_fec_receiver_info)
    int receiver_blocks = 0;       // ... blocks it decoded
    ldpc_amd::Scratch demux_tab;   // fec_flows_demux: the [tiles][nflows] u32 histogram table, the flow bases behind it (at most 16 MiB + 64 KiB)
    int64_t demux_tile = 0, demux_tiles = 0;   // ... tile length in packets and tiles of the last partition (ldpc_amd_fec_flows_demux_info)
    // fec_rx_flows_*_flush_many: path (0 none, 1 fused, 2 composed, 3 push form), blocks, scratch bytes and decoder launches of the
    // last call that closed a block (ldpc_amd_fec_flows_flush_info)
    int64_t flush_info[4] = {0, 0, 0, 0};
    // FPGA-harness emulation state (ldpc_amd_data_in / _ldpc_erasure_decoder / _data_out)
    // The run is streamed in chunks like the FPGA's frame loop (ldpc_erasure_decoder_perf_tests.cl:52): fpga_erased holds the
    // flags of ONE chunk, fpga_stats the two running counters (+ per-frame results: of the whole run when it is short
    // enough to keep them for ldpc_amd_fpga_frame_stats, else of one chunk).
    ldpc_amd::Scratch fpga_erased, fpga_stats;
    long fpga_frames = -1;        // numFrames of the last ldpc_amd_data_in, -1 = none
    long fpga_first = 0;          // first frame of the run in the source's stream (ldpc_amd_data_in_at: a shard of a multi-device run)
    long fpga_decoded = -1;       // numFrames the last decoder call ran over, -1 = no decoder call since data_in
    bool fpga_kept = false;       // per-frame results of the whole run are in fpga_stats
    int fpga_code_ind = -1;
    int fpga_per64 = 0;
    int fpga_seed = 0;
    int fpga_binary_code[4] = {-1, -1, -1, -1};
    int sm_count = 256;
    ldpc_amd::Knobs knobs;
    // profiling (ldpc_amd_set_profiling): event pairs per kernel kind
    int profiling = 0;          // 0 off, 1 the three kinds of a call, 2 + the nested brackets (tier 2 alone, solve kernel alone)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events[LDPC_AMD_PROF_KINDS];
    std::vector<hipEvent_t> prof_pool;
    std::string prof_names[LDPC_AMD_PROF_KINDS + LDPC_AMD_NAME_KINDS];   // template instantiation the last launch of each kind used; then the name-only kinds
    int last_plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // launch plan of the last decode (ldpc_amd_last_plan)
    int last_enc_grouped = 0;                      // the last packet-mode encode ran the grouped static schedule (ldpc_amd_encode_info)
    int symbol_unit = 16;                          // 16, or 4: word-sized symbols (include/ldpc_erasure_amd_words.h; not a knob)
    // fec_rxw_dev_decode_many / _decode_flush (rx_window_dev.hip): path (0 none, 1 fused, 2 composed), blocks, decoder launches and
    // scratch bytes of the last call (ldpc_amd_fec_rxw_info)
    int64_t rxw_info[4] = {0, 0, 0, 0};
    // fec_rxw_flows_decode_many / _decode_flush_many (rx_window_flows_dev.hip): the same four words (ldpc_amd_fec_rxw_flows_info)
    int64_t rxwf_info[4] = {0, 0, 0, 0};
    // fec_rs_encode_packets_dev (include/ldpc_erasure_amd_rs_wire.h): the packed-multiply table and the padded coefficients the packet
    // encoder of rs_wire_dev.hip reads (its last call: tx_last[kTxRs])
    ldpc_amd::Scratch rsw_tab, rsw_coef;
    // fec_rxw_dev_rs_decode_many / _rs_decode_flush (rx_window_dev.hip): blocks, RS decode launches, scratch bytes and path (0 none,
    // 1 fused, 2 composed) of the last call (ldpc_amd_fec_rs_receiver_info)
    int64_t rsrx_info[4] = {0, 0, 0, 0};
    // the RS decoder on rows in place (rs_wire_dev.hip, launch_rs_decode_rows): per block of one chunk its header, the records of its
    // selected rows and its coefficient table (at most 256 MiB)
    ldpc_amd::Scratch rsr_plan;
};

namespace ldpc_amd {

// ---- launchers implemented in the .hip files (all asynchronous on ctx->stream) -----------------
// Where the rows of a packets-in decode lie (the fused receiver, wire_dev.hip): one word per (frame, symbol) --
//   p < 2^31        payload of packet p: packets + p * plen + 8
//   2^31 | i        row i of the staging planes: stage + i * S   (a carried block that got no newer packet for the symbol)
//   0xFFFFFFFF      erased: nothing is fetched
// src == nullptr: an ordinary decode, rows from DecodeArgs::sym.
struct PacketRows {
    const uint32_t *src = nullptr;      // [nframes][n]
    const uint8_t *packets = nullptr;   // 8-byte aligned
    const uint8_t *stage = nullptr;     // [2][n][S], 16-byte aligned
    int plen = 0;                       // 8 + S
};
constexpr uint32_t kRowErased = 0xFFFFFFFFu, kRowStaged = 0x80000000u;

struct DecodeArgs {
    DevCode code;
    int S;
    int64_t nframes;
    const uint8_t *sym;     // [nframes][in_rows][S]
    const uint8_t *erased;  // [nframes][n] or nullptr (encode mode: rows >= in_rows are erased)
    int in_rows;            // n (decode) or k (encode)
    int max_sweeps;
    int do_ml;
    uint8_t *out;           // [nframes][n][S]
    int32_t *sweeps, *residual, *status;  // may be nullptr
    int flags_only = 0;                   // peel only (no data movement): FPGA-harness statistics
    int32_t *residual_sys = nullptr;      // [nframes] unknown symbols among the first k, or nullptr
    int inplace = 0;                      // out == sym: received rows are not rewritten
    // frames out (ldpc_amd_decode_frames): the flags of the symbols still unknown after the call, and how many of them are source
    // symbols -- the post-sweep mask, cleared behind the ML stage for the frames it solved.  Both nullptr: nothing is stored or launched
    uint8_t *erased_out = nullptr;        // [nframes][n] 0 / 1
    PacketRows pin;                       // packets-in decode (sym == nullptr, S % 16 == 0, out of place; only where decode_reads_packets says so)
    int32_t *residual_src = nullptr;      // [nframes]; the kernels' ONE residual_sys outlet: set residual_src or residual_sys, never both
                                          // (launch_decode refuses both; flags_only runs use residual_sys, decode_frames residual_src)
};

hipError_t upload_constants(hipStream_t s);
// Words of the residual list's header (the first 32 ints of the ML list: [0] the residual frames, [1..16] the size-class counts)
// that hold the ML stage's work counters and statistics.  Every decode zeroes them with the header; ldpc_amd_ml_stats reads them back.
enum MlHdrWord {
    kMlHdrCount = 0,        // residual frames
    kMlHdrWork2 = 17,       // hand-out counter of the launch that solves the deferred frames (mode 2)
    kMlHdrWork = 18,        // MlArgs::work: [0] frame hand-out counter of the factorisation, and the five words behind it:
    kMlHdrDeferred = 19,    //   [1] frames deferred by the launch beside the packet kernel
    kMlHdrOpsHead = 20,     //   [2..3] arena bump pointer (u64)
    kMlHdrSolveWork = 22,   //   [4] task counter of the solve kernel
    kMlHdrPiWork = 23,      //   [5] frame hand-out counter of the fast path (ldpc_ml_pi_kernel)
    kMlHdrNfail = 24,       // frames whose fast-path solution failed the consistency check (not codewords)
    kMlHdrWork3 = 25,       // hand-out counter of the launch that factors them again, exactly (mode 3)
    kMlHdrSolveWork2 = 26,  // task counter of the solve kernel's second round, which redoes them
    kMlHdrPiDone = 27,      // frames the fast path emitted
    kMlHdrWords = 32,
};
int launch_decode(ldpc_amd_ctx *ctx, const DecodeArgs &a);
bool decode_reads_packets(ldpc_amd_ctx *ctx, const DevCode &code, int S);   // launch_decode would take DecodeArgs::pin for this code and S
int launch_encode(ldpc_amd_ctx *ctx, const DevCode &code, int S, int64_t nframes, const uint8_t *src, uint8_t *cw);
// The fused sender: source [nframes][k][S] -> packets [nframes * n][8 + S], the encoder storing packets instead of codewords.
// Returns kEncodeNotFused, with nothing launched, where this call's encoder has no packet-output form (or ENC_PKT = 0).
constexpr int kEncodeNotFused = 1;
int launch_encode_packets(ldpc_amd_ctx *ctx, const DevCode &code, int S, int64_t nframes, const uint8_t *src, unsigned fec_class,
                          unsigned block0, uint8_t *packets);
// ... every frame placed and numbered by a descriptor {first packet: u64, stride in packets: u32, class << 8 | block: u32} in device
// memory (the multi-flow sender); max_stride = the largest stride of the table.  kEncodeNotFused as above, or where max_stride * (8 + S)
// does not fit 32 bits.
int launch_encode_packets_flows(ldpc_amd_ctx *ctx, const DevCode &code, int S, int64_t nframes, const uint8_t *src, const void *flow_desc,
                                int64_t max_stride, uint8_t *packets);
int launch_fpga_halves(ldpc_amd_ctx *ctx, const DevCode &code, int64_t nframes, const uint8_t *erased, int num_iter,
                       int32_t *residual_sys, int32_t *iterations);
int launch_selftest(ldpc_amd_ctx *ctx);
int launch_copy_probe(ldpc_amd_ctx *ctx, const uint8_t *src, uint8_t *dst, uint64_t bytes, int reps, double *ms);
int launch_synth_source(ldpc_amd_ctx *ctx, uint64_t seed, int64_t frame0, int64_t nframes, int k, int S, uint8_t *d);
int launch_synth_erasures(ldpc_amd_ctx *ctx, uint64_t seed, uint32_t stream_id, int64_t first, int64_t count,
                          uint64_t thresh, uint8_t *d);
int launch_synth_bursty(ldpc_amd_ctx *ctx, uint64_t seed, int64_t first, int64_t count, double alpha, double beta,
                        double bias, uint8_t *d);
int launch_synth_fpga(ldpc_amd_ctx *ctx, uint32_t seed, uint64_t first, int64_t count, int per64, uint8_t *d);
int launch_rs_decode(ldpc_amd_ctx *ctx, const HostRs &rs, int S, int64_t nblocks, const uint16_t *idx,
                     const uint8_t *val, uint8_t *msg);
// frames in (ldpc_amd_rs_decode_frames): first-k selection from the flags, then the decode kernels on the rows in place
int launch_rs_decode_frames(ldpc_amd_ctx *ctx, const HostRs &rs, int S, int64_t nblocks, const uint8_t *sym, const uint8_t *erased,
                            uint8_t *msg, int32_t *received, int32_t *status);
int launch_rs_encode(ldpc_amd_ctx *ctx, const HostRs &rs, int S, int64_t nblocks, const uint8_t *src, uint8_t *cw);
// The RS sender's fused form (rs_wire_dev.hip): source [nblocks][k][S] -> packets [nblocks * n][8 + S], every block placed and numbered
// by its 16-byte descriptor in device memory, as launch_encode_packets_flows places a frame.  Returns kEncodeNotFused, with nothing
// launched, where the kernel does not apply: S = 1, ENC_PKT = 0, packets not 8-byte aligned, a source the fused LDPC sender would not
// take, max_stride * (8 + S) beyond 32 bits.
int launch_rs_encode_packets(ldpc_amd_ctx *ctx, const HostRs &rs, int S, int64_t nblocks, const uint8_t *src, const void *desc, int64_t max_stride,
                             uint8_t *packets);
// The RS decoder on rows in place (rs_wire_dev.hip; include/ldpc_erasure_amd_rs_rows.h): the rows of block b lie where the words
// rows.src[b][n] say (PacketRows above; rows.stage holds nstage_rows rows of S bytes, rows.packets npackets packets of rows.plen = 8 + S
// bytes), a word that points outside either array counts as erased.  msg [nblocks][k][S]; er_out [nblocks][n] the flags after
// vetting, received and status [nblocks]: each may be nullptr.  First-k selection as launch_rs_decode_frames.
// rs_decode_rows_takes: the shapes the kernels take -- launch_rs_decode_rows returns kDecodeNotFused, with nothing launched, where it
// says no.  rs_decode_rows_fused: the one eligibility rule of the receivers -- takes, less the shapes where the composed path is the
// faster one.  rs_decode_rows_reserve: every workspace nblocks blocks will need (rx_host.h, rule 1), *bytes what one chunk uses.
constexpr int kDecodeNotFused = 1;
bool rs_decode_rows_takes(const ldpc_amd_ctx *ctx, const HostRs &rs, int S, const uint8_t *packets, const uint8_t *stage, const uint8_t *msg);
bool rs_decode_rows_fused(const ldpc_amd_ctx *ctx, const HostRs &rs, int S, const uint8_t *packets, const uint8_t *stage, const uint8_t *msg);
int rs_decode_rows_reserve(ldpc_amd_ctx *ctx, const HostRs &rs, int64_t nblocks, size_t *bytes);
int launch_rs_decode_rows(ldpc_amd_ctx *ctx, const HostRs &rs, int S, int64_t nblocks, const PacketRows &rows, int64_t npackets,
                          int64_t nstage_rows, uint8_t *er_out, uint8_t *msg, int32_t *received, int32_t *status, int *launches = nullptr);
int launch_fpga_stats(ldpc_amd_ctx *ctx, const DevCode &code, int rs_n, int rs_k, int64_t nframes,
                      const uint8_t *erased0, const int32_t *residual_k, unsigned long long *stats /* [2], accumulated */);

int scratch_reserve(ldpc_amd_ctx *ctx, Scratch &s, size_t bytes);
// This call's slot of a ring, at least `bytes` long: waits for the copy that last read the slot (two calls ago), grows the slot in
// 64 KiB steps.  LDPC_AMD_ENOMEM, with *want = the bytes asked for and NO error text (the caller has its own), when there is no
// pinned memory.  The caller fills *host, enqueues its copy on ctx->stream and commits.
int pinned_ring_acquire(ldpc_amd_ctx *ctx, PinnedRing &r, size_t bytes, void **host, size_t *want);
// Behind the copy: records the slot's event on ctx->stream and turns to the other slot.
int pinned_ring_commit(ldpc_amd_ctx *ctx, PinnedRing &r);
void pinned_ring_free(PinnedRing &r);
// Brackets one kernel launch with events when profiling is on (no-ops otherwise).
hipEvent_t prof_begin(ldpc_amd_ctx *ctx, int level = 1);
void prof_end(ldpc_amd_ctx *ctx, int kind, hipEvent_t start);
int set_error(ldpc_amd_ctx *ctx, int code, const char *fmt, ...);
// Symbol lengths (include/ldpc_erasure_amd_words.h).  A context accepts S = 1 and the multiples of its unit: of 16, or -- unit 4 --
// of 4 from 16 bytes up.  The lengths only unit 4 accepts run the WORD FORM of the payload kernels: the same B-byte row pieces,
// ceil(S / B) of them, piece sl starting at min(sl * B, S - B) -- the last one overlaps its neighbour and ends with the row -- and
// every global access a 4-byte one (rows start on 4-byte boundaries only).  A multiple of 16 runs what it runs with unit 16.
inline bool symbol_len_ok(const ldpc_amd_ctx *ctx, int S) { return S == 1 || (ctx->symbol_unit == 4 ? (S >= 16 && (S % 4) == 0) : (S % 16) == 0); }
inline bool symbol_len_words(int S) { return S != 1 && (S % 16) != 0; }
// the refusal: LDPC_AMD_EUNSUP with the words header's text under unit 4, else with text16 (the entry point's own, S its one argument)
int refuse_symbol_len(ldpc_amd_ctx *ctx, int S, const char *text16);
// After a synchronisation: LDPC_AMD_EHIP (and the word cleared) if a kernel of this context reported a violated assumption.
int check_device_error(ldpc_amd_ctx *ctx);
// A pointer of this context's device (hipMalloc / torch), not host memory.
bool is_device_ptr(const ldpc_amd_ctx *ctx, const void *p);

#define LDPC_HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess)                                                                    \
            return ldpc_amd::set_error((ctx), LDPC_AMD_EHIP, "%s failed: %s (%s:%d)", #expr,      \
                                       hipGetErrorString(e__), __FILE__, __LINE__);               \
    } while (0)

}  // namespace ldpc_amd
