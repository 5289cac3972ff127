"""ctypes binding of the C ABI (include/ldpc_erasure_amd.h -> libldpc_erasure_amd.so).

Host-side mirror of the reference's interfaces for the hot path, so that tests read like the reference's
own harnesses:

    Context()                        ~ init_opencl()            OpenCL/host/src/main.cpp:439
    Context.close()                  ~ cleanup()                main.cpp:668
    Context.decode(...)              ~ My_LDPC_HybridML_NonBinary_Erasure_Decoder(recv, Vlist, Clist, H, n, k, ...)
                                       Matlab/My_LDPC_HybridML_NonBinary_Erasure_Decoder.m:4   (batched)
    Context.rs_decode(...)           ~ My_RS_Decode(recv_vec_ind, recv_vec_gf256_val, m, n, k, ...)
                                       Matlab/My_RS_Decode.m:14                                   (batched)

There is NO CPU fallback here: if the HIP library is missing or no gfx950 device is present every call
raises.  Arrays may be numpy (host pointers; the library stages them) or torch CUDA tensors (device
pointers; asynchronous on the context's stream).
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libldpc_erasure_amd.so")

OK = 0
DEVICE_PTRS = 1
INPLACE = 2
ST_MP_DONE, ST_ML_SOLVED, ST_ML_RANKDEF, ST_ML_SKIPPED = 0, 1, 2, 3
RS_ST_DECODED, RS_ST_SHORT = 0, 1
# LDPC_AMD_PROF_*: "apply" = both tiers of the packet kernel ("apply_tier2" is the tier-2 launch alone), "ml" = factorisation + solve
# ("ml_solve" is the solve kernel alone)
PROF_KINDS = ("peel", "apply", "ml", "apply_tier2", "ml_solve")
# LDPC_AMD_NAME_RS / LDPC_AMD_NAME_ENCODE: names only, no time; the header numbers them after the timed kinds (LDPC_AMD_PROF_KINDS + 0, + 1)
NAME_RS, NAME_ENCODE = len(PROF_KINDS), len(PROF_KINDS) + 1

# every symbol include/ldpc_erasure_amd.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "ldpc_amd_init", "ldpc_amd_cleanup", "ldpc_amd_last_error", "ldpc_amd_set_stream", "ldpc_amd_synchronize", "ldpc_amd_configure",
    "ldpc_amd_code_params", "ldpc_amd_load_builtin_code", "ldpc_amd_register_code", "ldpc_amd_code_info", "ldpc_amd_encode_info", "ldpc_amd_knobs",
    "ldpc_amd_code_csr", "ldpc_amd_decode_batch", "ldpc_amd_encode_batch", "ldpc_amd_rs_create",
    "ldpc_amd_rs_generator", "ldpc_amd_rs_encode_batch", "ldpc_amd_rs_decode_batch", "ldpc_amd_rs_bad_blocks", "ldpc_amd_synth_source",
    "ldpc_amd_synth_erasures_uniform", "ldpc_amd_synth_erasures_bursty", "ldpc_amd_data_in", "ldpc_amd_data_in_at",
    "ldpc_amd_shard_frames", "ldpc_amd_group_create", "ldpc_amd_group_destroy", "ldpc_amd_group_size", "ldpc_amd_group_device", "ldpc_amd_group_ctx",
    "ldpc_amd_group_last_error", "ldpc_amd_group_load_builtin_code", "ldpc_amd_group_register_code", "ldpc_amd_group_decode_batch",
    "ldpc_amd_group_decode_resident", "ldpc_amd_group_fpga_run", "ldpc_amd_group_bench_resident", "ldpc_amd_ldpc_erasure_decoder", "ldpc_amd_data_out",
    "ldpc_amd_ldpc_erasure_decoder_perf_tests", "ldpc_amd_fpga_frame_stats", "ldpc_amd_profile_kernel_name", "ldpc_amd_last_plan", "ldpc_amd_ml_stats",
    "ldpc_amd_fec_header_pack", "ldpc_amd_fec_header_unpack", "ldpc_amd_fec_packetize", "ldpc_amd_fec_rx_create",
    "ldpc_amd_fec_rx_destroy", "ldpc_amd_fec_rx_push", "ldpc_amd_fec_rx_push_many", "ldpc_amd_fec_rx_flush", "ldpc_amd_fec_rx_dropped",
    "ldpc_amd_set_profiling", "ldpc_amd_get_profile", "ldpc_amd_selftest", "ldpc_amd_copy_probe", "ldpc_amd_gf_tables", "ldpc_amd_version",
]
# every symbol include/ldpc_erasure_amd_wire_dev.h declares (the device-resident wire path)
EXPORTS_WIRE_DEV = [
    "ldpc_amd_fec_packetize_dev", "ldpc_amd_fec_rx_dev_create", "ldpc_amd_fec_rx_dev_destroy", "ldpc_amd_fec_rx_dev_push_many",
    "ldpc_amd_fec_rx_dev_flush", "ldpc_amd_fec_rx_dev_dropped",
]
# every symbol include/ldpc_erasure_amd_frames.h declares (erasure flags out of the LDPC decoder, RS decode from erased frames)
EXPORTS_FRAMES = ["ldpc_amd_decode_frames", "ldpc_amd_rs_info", "ldpc_amd_rs_decode_frames"]

# every symbol include/ldpc_erasure_amd_sender.h declares (the fused sender: source symbols straight to wire packets)
EXPORTS_SENDER = ["ldpc_amd_fec_encode_packets_dev", "ldpc_amd_fec_sender_info"]
SENDER_PATHS = ("none", "fused", "composed")
_SENDER_KEYS = ("path", "scratch_bytes", "descriptor_bytes", "frames")   # the four words of the descriptor-driven senders' info calls
# every symbol include/ldpc_erasure_amd_sender_flows.h declares (the multi-flow sender: many FEC streams to one multiplexed wire)
EXPORTS_SENDER_FLOWS = ["ldpc_amd_fec_tx_flows_layout", "ldpc_amd_fec_encode_packets_flows_dev", "ldpc_amd_fec_sender_flows_info"]
TX_SEGMENTED, TX_ROUND_ROBIN = 0, 1   # LDPC_AMD_FEC_TX_SEGMENTED / LDPC_AMD_FEC_TX_ROUND_ROBIN
# every symbol include/ldpc_erasure_amd_interleave.h declares (the block-interleaved wire: depth-D sender, depth-D windowed receivers)
EXPORTS_INTERLEAVE = [
    "ldpc_amd_fec_tx_ilv_layout", "ldpc_amd_fec_encode_packets_ilv_dev", "ldpc_amd_fec_sender_ilv_info", "ldpc_amd_fec_rxw_create_depth",
    "ldpc_amd_fec_rxw_dev_create_depth", "ldpc_amd_fec_rxw_depth", "ldpc_amd_fec_rxw_dev_depth",
]
ILV_DEPTHS = (1, 2, 4, 8, 16)
# every symbol include/ldpc_erasure_amd_interleave_flows.h declares (depth on the multi-flow wire: sender and windowed receiver)
EXPORTS_INTERLEAVE_FLOWS = [
    "ldpc_amd_fec_tx_flows_ilv_layout", "ldpc_amd_fec_encode_packets_flows_ilv_dev", "ldpc_amd_fec_sender_flows_ilv_info",
    "ldpc_amd_fec_rxw_flows_create_depth", "ldpc_amd_fec_rxw_flows_depth",
]
# every symbol include/ldpc_erasure_amd_receiver.h declares (the fused receiver: wire packets straight to decoded frames)
# include/ldpc_erasure_amd_rs_wire.h: Reed-Solomon on the FEC wire
EXPORTS_RS_WIRE = [
    "ldpc_amd_fec_rs_encode_packets_dev", "ldpc_amd_fec_rs_sender_info", "ldpc_amd_fec_rxw_dev_rs_decode_many",
    "ldpc_amd_fec_rxw_dev_rs_decode_flush", "ldpc_amd_fec_rs_receiver_info",
]
FEC_CLASS_RS = 2   # LDPC_AMD_FEC_CLASS_RS
# include/ldpc_erasure_amd_rs_rows.h: the RS decoder on rows in place, and the two constants of a source word
EXPORTS_RS_ROWS = ["ldpc_amd_rs_decode_rows_dev"]
ROW_STAGED, ROW_ERASED = 0x80000000, 0xFFFFFFFF   # LDPC_AMD_ROW_STAGED | row of `stage`; LDPC_AMD_ROW_ERASED
EXPORTS_RECEIVER = ["ldpc_amd_fec_rx_dev_decode_many", "ldpc_amd_fec_rx_dev_decode_flush", "ldpc_amd_fec_receiver_info"]
RECEIVER_PATHS = ("none", "fused", "composed")
# every symbol include/ldpc_erasure_amd_words.h declares (word-sized symbols: any S that is a multiple of 4)
EXPORTS_WORDS = ["ldpc_amd_set_symbol_unit", "ldpc_amd_get_symbol_unit"]
# every symbol include/ldpc_erasure_amd_flows.h declares (the multi-flow device receiver: many FEC streams per call)
EXPORTS_FLOWS = [
    "ldpc_amd_fec_rx_flows_create", "ldpc_amd_fec_rx_flows_destroy", "ldpc_amd_fec_rx_flows_push_many", "ldpc_amd_fec_rx_flows_decode_many",
    "ldpc_amd_fec_rx_flows_flush", "ldpc_amd_fec_rx_flows_decode_flush", "ldpc_amd_fec_rx_flows_dropped",
]
# every symbol include/ldpc_erasure_amd_flows_mixed.h declares (the multi-flow receiver fed with interleaved packets and a flow id each)
EXPORTS_FLOWS_MIXED = [
    "ldpc_amd_fec_rx_flows_push_mixed", "ldpc_amd_fec_rx_flows_decode_mixed", "ldpc_amd_fec_rx_flows_unrouted", "ldpc_amd_fec_flows_demux_dev",
    "ldpc_amd_fec_flows_demux_info",
]
# every symbol include/ldpc_erasure_amd_flows_flush.h declares (the multi-flow receiver's batch flush)
EXPORTS_FLOWS_FLUSH = [
    "ldpc_amd_fec_rx_flows_pending", "ldpc_amd_fec_rx_flows_flush_many", "ldpc_amd_fec_rx_flows_decode_flush_many",
    "ldpc_amd_fec_flows_flush_info",
]
FLUSH_PATHS = ("none", "fused", "composed", "push")
# every symbol include/ldpc_erasure_amd_datagrams.h declares (datagrams of any length: pack to source symbols, unpack after decode)
EXPORTS_DATAGRAMS = ["ldpc_amd_fec_dgram_pack_dev", "ldpc_amd_fec_dgram_unpack_dev", "ldpc_amd_fec_dgram_wire_len", "ldpc_amd_fec_dgram_info"]
DGRAM_DELIVERED, DGRAM_FILLER, DGRAM_LOST, DGRAM_MALFORMED = 0, 1, 2, 3   # LDPC_AMD_DGRAM_*: the state of a row after unpack
DGRAM_PREFIX_BYTES = 4
Datagrams = collections.namedtuple("Datagrams", "bytes offset state")
# every symbol include/ldpc_erasure_amd_wire_ragged.h declares (the trimmed wire: packets cut to their sent bytes, and landed back)
EXPORTS_WIRE_RAGGED = ["ldpc_amd_fec_wire_trim_dev", "ldpc_amd_fec_wire_land_dev", "ldpc_amd_fec_wire_ragged_info"]
WIRE_LANDED, WIRE_REJECTED = 0, 1   # LDPC_AMD_WIRE_*: the state of a datagram after land
Wire = collections.namedtuple("Wire", "bytes offset")
# every symbol include/ldpc_erasure_amd_link.h declares (the link emulator: reorder, duplicate, damage, on the device)
EXPORTS_LINK = ["ldpc_amd_fec_link_plan_dev", "ldpc_amd_fec_link_apply_dev", "ldpc_amd_fec_link_apply_ragged_dev", "ldpc_amd_fec_link_info"]
LINK_STREAM_DUP, LINK_STREAM_DELAY, LINK_STREAM_DAMAGE = 16, 17, 18   # LDPC_AMD_LINK_STREAM_*
LINK_MAX_WINDOW = 4096
LINK_DUP_FLIP = 1                                                       # LDPC_AMD_LINK_DUP_FLIP, a flag of the parameters
LINK_COPY, LINK_BADSYM, LINK_FOREIGN, LINK_FLIPPED = 1, 2, 4, 8         # LDPC_AMD_LINK_*: the fate bits (the high byte: the FOREIGN block value)
FlowsPending = collections.namedtuple("FlowsPending", "cur_block cur_cnt next_cnt blocks")
# every symbol include/ldpc_erasure_amd_rx_window.h declares (the windowed receiver: W open blocks, resynchronises after an outage)
EXPORTS_RX_WINDOW = [
    "ldpc_amd_fec_rxw_create", "ldpc_amd_fec_rxw_destroy", "ldpc_amd_fec_rxw_push", "ldpc_amd_fec_rxw_push_many", "ldpc_amd_fec_rxw_flush",
    "ldpc_amd_fec_rxw_stats", "ldpc_amd_fec_rxw_dropped", "ldpc_amd_fec_rxw_state",
    "ldpc_amd_fec_rxw_dev_create", "ldpc_amd_fec_rxw_dev_destroy", "ldpc_amd_fec_rxw_dev_push_many", "ldpc_amd_fec_rxw_dev_flush",
    "ldpc_amd_fec_rxw_dev_decode_many", "ldpc_amd_fec_rxw_dev_decode_flush", "ldpc_amd_fec_rxw_dev_stats", "ldpc_amd_fec_rxw_dev_dropped",
    "ldpc_amd_fec_rxw_dev_state", "ldpc_amd_fec_rxw_info",
]
RX_WINDOW_PATHS = ("none", "fused", "composed")
_RXW_KEYS = ("path", "blocks", "launches", "scratch_bytes")   # the four words of the windowed receivers' info calls
RX_WINDOW_TOTALS = ("bad_symbol", "late", "ahead_total", "resyncs", "closed")   # LDPC_AMD_RXW_*: the order of the totals
RX_WINDOW_MIN, RX_WINDOW_MAX = 2, 32
# every symbol include/ldpc_erasure_amd_rx_window_flows.h declares (the windowed multi-flow receiver and its batch flush)
EXPORTS_RX_WINDOW_FLOWS = [
    "ldpc_amd_fec_rxw_flows_create", "ldpc_amd_fec_rxw_flows_destroy", "ldpc_amd_fec_rxw_flows_push_many",
    "ldpc_amd_fec_rxw_flows_decode_many", "ldpc_amd_fec_rxw_flows_flush_many", "ldpc_amd_fec_rxw_flows_decode_flush_many",
    "ldpc_amd_fec_rxw_flows_pending", "ldpc_amd_fec_rxw_flows_state", "ldpc_amd_fec_rxw_flows_stats", "ldpc_amd_fec_rxw_flows_dropped",
    "ldpc_amd_fec_rxw_flows_info",
]
WindowFlowsPending = collections.namedtuple("WindowFlowsPending", "base cnt blocks")
# every symbol include/ldpc_erasure_amd_rx_window_flows_mixed.h declares (the windowed multi-flow receiver fed with interleaved packets)
EXPORTS_RX_WINDOW_FLOWS_MIXED = ["ldpc_amd_fec_rxw_flows_push_mixed", "ldpc_amd_fec_rxw_flows_decode_mixed", "ldpc_amd_fec_rxw_flows_unrouted"]
# every symbol include/ldpc_erasure_amd_rx_rule.h declares (the close rule of the windowed receivers as a value)
EXPORTS_RX_RULE = [
    "ldpc_amd_fec_rx_rule_default", "ldpc_amd_fec_rx_rule_mds", "ldpc_amd_fec_rx_rule_check", "ldpc_amd_fec_rxw_create_rule",
    "ldpc_amd_fec_rxw_dev_create_rule", "ldpc_amd_fec_rxw_flows_create_rule", "ldpc_amd_fec_rxw_get_rule", "ldpc_amd_fec_rxw_dev_get_rule",
    "ldpc_amd_fec_rxw_flows_get_rule",
]

DecodedFrames = collections.namedtuple("DecodedFrames", "out sweeps residual status erased_out residual_src")
RsDecodedFrames = collections.namedtuple("RsDecodedFrames", "msg received status")


class LdpcAmdError(RuntimeError):
    pass


class ErrorType(C.Structure):
    _fields_ = [("num_LDPC_errors", C.c_int), ("num_RS_errors", C.c_int)]


class RxRule(C.Structure):
    """ldpc_amd_fec_rx_rule"""
    _fields_ = [("c_hi", C.c_int32), ("later_hi", C.c_int32), ("c_lo", C.c_int32), ("later_lo", C.c_int32)]


class LinkParams(C.Structure):
    """ldpc_amd_link_params"""
    _fields_ = [("seed", C.c_uint64), ("first", C.c_uint64), ("window", C.c_int32), ("flags", C.c_int32), ("dup", C.c_double),
                ("bad_sym", C.c_double), ("foreign", C.c_double)]


_lib = None


def load_library():
    """Loads libldpc_erasure_amd.so (built in-tree by __graft_entry__.build()).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LdpcAmdError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
    # PyTorch-ROCm ships its own libamdhip64.so.7 / libhsa-runtime64; two HIP runtimes in one process do not
    # both see the GPU.  Loading torch first makes our library bind to the runtime torch uses (same SONAME),
    # so device pointers, streams and events are shared between the two.
    try:
        import torch  # noqa: F401
    except Exception:  # torch is optional plumbing: without it the system ROCm runtime is used
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
    L.ldpc_amd_init.argtypes = [i32, C.POINTER(vp)]
    L.ldpc_amd_cleanup.argtypes = [vp]
    L.ldpc_amd_cleanup.restype = None
    L.ldpc_amd_last_error.argtypes = [vp]
    L.ldpc_amd_last_error.restype = C.c_char_p
    L.ldpc_amd_set_stream.argtypes = [vp, vp]
    L.ldpc_amd_synchronize.argtypes = [vp]
    if hasattr(L, "ldpc_amd_configure"):   # (tools/ab_lib.py and tools/time_latency.py also load older builds of the library)
        L.ldpc_amd_configure.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.ldpc_amd_code_params.argtypes = [i32, C.POINTER(i32)]
    L.ldpc_amd_load_builtin_code.argtypes = [vp, i32, u64]
    L.ldpc_amd_register_code.argtypes = [vp, i32, i32, vp, vp, vp]
    L.ldpc_amd_code_info.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.ldpc_amd_encode_info.argtypes = [vp, i32, C.POINTER(i32)]
    if hasattr(L, "ldpc_amd_knobs"):
        L.ldpc_amd_knobs.argtypes = [vp, C.c_char_p, i32]
    # multi-device layer (include/ldpc_erasure_amd_multi.h)
    L.ldpc_amd_shard_frames.argtypes = [i64, i32, i32, C.POINTER(i64), C.POINTER(i64)]
    L.ldpc_amd_shard_frames.restype = None
    L.ldpc_amd_group_create.argtypes = [i32, C.POINTER(i32), C.POINTER(vp)]
    L.ldpc_amd_group_destroy.argtypes = [vp]
    L.ldpc_amd_group_destroy.restype = None
    L.ldpc_amd_group_size.argtypes = [vp]
    L.ldpc_amd_group_device.argtypes = [vp, i32]
    L.ldpc_amd_group_ctx.argtypes = [vp, i32]
    L.ldpc_amd_group_ctx.restype = vp
    L.ldpc_amd_group_last_error.argtypes = [vp]
    L.ldpc_amd_group_last_error.restype = C.c_char_p
    L.ldpc_amd_group_load_builtin_code.argtypes = [vp, i32, u64]
    L.ldpc_amd_group_register_code.argtypes = [vp, i32, i32, vp, vp, vp]
    L.ldpc_amd_group_decode_batch.argtypes = [vp, i32, i32, i64, vp, vp, i32, i32, vp, vp, vp, vp]
    L.ldpc_amd_group_decode_resident.argtypes = [vp, i32, i32, i64, C.POINTER(vp), C.POINTER(vp), i32, i32, C.POINTER(vp), C.POINTER(vp), vp, vp,
                                                 C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ldpc_amd_group_fpga_run.argtypes = [vp, C.c_ushort, i32, i32, i32, C.c_long, C.c_short, i32, C.POINTER(ErrorType)]
    L.ldpc_amd_group_bench_resident.argtypes = [vp, i32, u64, i32, i64, C.c_double, i32, i32, C.POINTER(C.c_double)]
    L.ldpc_amd_data_in_at.argtypes = [vp, vp, C.c_ushort, i32, i32, i32, C.c_long, C.c_long]
    L.ldpc_amd_code_csr.argtypes = [vp, i32, vp, vp, vp]
    L.ldpc_amd_decode_batch.argtypes = [vp, i32, i32, i64, vp, vp, i32, i32, vp, vp, vp, vp, C.c_uint]
    L.ldpc_amd_encode_batch.argtypes = [vp, i32, i32, i64, vp, vp, C.c_uint]
    L.ldpc_amd_rs_create.argtypes = [vp, i32, i32]
    L.ldpc_amd_rs_generator.argtypes = [vp, i32, vp]
    L.ldpc_amd_rs_encode_batch.argtypes = [vp, i32, i32, i64, vp, vp, C.c_uint]
    L.ldpc_amd_rs_decode_batch.argtypes = [vp, i32, i32, i64, vp, vp, vp, C.c_uint]
    if hasattr(L, "ldpc_amd_rs_bad_blocks"):
        L.ldpc_amd_rs_bad_blocks.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.ldpc_amd_synth_source.argtypes = [vp, u64, i64, i64, i32, i32, vp]
    L.ldpc_amd_synth_erasures_uniform.argtypes = [vp, u64, i64, i64, i32, C.c_double, vp]
    L.ldpc_amd_synth_erasures_bursty.argtypes = [vp, u64, i64, i64, i32, C.c_double, C.c_double, C.c_double, vp]
    L.ldpc_amd_data_in.argtypes = [vp, vp, C.c_ushort, i32, i32, i32, C.c_long]
    L.ldpc_amd_ldpc_erasure_decoder.argtypes = [vp, C.c_short, i32]
    L.ldpc_amd_ldpc_erasure_decoder_perf_tests.argtypes = [vp, C.c_short, i32]
    L.ldpc_amd_fpga_frame_stats.argtypes = [vp, C.c_long, vp, vp]
    # host-side wire format (include/ldpc_erasure_amd_wire.h)
    L.ldpc_amd_fec_header_pack.argtypes = [C.c_uint, C.c_uint, C.c_uint]
    L.ldpc_amd_fec_header_pack.restype = C.c_uint64
    L.ldpc_amd_fec_header_unpack.argtypes = [C.c_uint64, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.ldpc_amd_fec_header_unpack.restype = None
    L.ldpc_amd_fec_packetize.argtypes = [vp, C.c_long, i32, i32, C.c_uint, C.c_uint, vp]
    L.ldpc_amd_fec_rx_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
    L.ldpc_amd_fec_rx_destroy.argtypes = [vp]
    L.ldpc_amd_fec_rx_destroy.restype = None
    L.ldpc_amd_fec_rx_push.argtypes = [vp, vp, vp, vp, C.POINTER(i32)]
    L.ldpc_amd_fec_rx_flush.argtypes = [vp, vp, vp, C.POINTER(i32)]
    L.ldpc_amd_fec_rx_push_many.argtypes = [vp, vp, C.c_long, vp, vp, vp, i32, C.POINTER(C.c_long)]
    L.ldpc_amd_fec_rx_dropped.argtypes = [vp]
    L.ldpc_amd_fec_rx_dropped.restype = C.c_long
    # device-resident wire path (include/ldpc_erasure_amd_wire_dev.h)
    L.ldpc_amd_fec_packetize_dev.argtypes = [vp, vp, i64, i32, i32, C.c_uint, C.c_uint, vp]
    L.ldpc_amd_fec_rx_dev_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    L.ldpc_amd_fec_rx_dev_destroy.argtypes = [vp]
    L.ldpc_amd_fec_rx_dev_destroy.restype = None
    L.ldpc_amd_fec_rx_dev_push_many.argtypes = [vp, vp, i64, vp, vp, vp, i32, C.POINTER(i64)]
    L.ldpc_amd_fec_rx_dev_flush.argtypes = [vp, vp, vp, C.POINTER(i32)]
    L.ldpc_amd_fec_rx_dev_dropped.argtypes = [vp]
    L.ldpc_amd_fec_rx_dev_dropped.restype = i64
    # the fused sender (include/ldpc_erasure_amd_sender.h)
    if hasattr(L, "ldpc_amd_fec_encode_packets_dev"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_encode_packets_dev.argtypes = [vp, i32, i32, i64, vp, C.c_uint, C.c_uint, vp]
        L.ldpc_amd_fec_sender_info.argtypes = [vp, C.POINTER(i32)]
    # the multi-flow sender (include/ldpc_erasure_amd_sender_flows.h)
    if hasattr(L, "ldpc_amd_fec_tx_flows_layout"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_tx_flows_layout.argtypes = [i32, vp, i32, i32, vp, vp]
        L.ldpc_amd_fec_tx_flows_layout.restype = i64
        L.ldpc_amd_fec_encode_packets_flows_dev.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp]
        L.ldpc_amd_fec_sender_flows_info.argtypes = [vp, C.POINTER(i64)]
    # the fused receiver (include/ldpc_erasure_amd_receiver.h)
    if hasattr(L, "ldpc_amd_fec_rx_dev_decode_many"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_rx_dev_decode_many.argtypes = [vp, i32, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(i64)]
        L.ldpc_amd_fec_rx_dev_decode_flush.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(i32)]
        L.ldpc_amd_fec_receiver_info.argtypes = [vp, C.POINTER(i32)]
    # the multi-flow receiver (include/ldpc_erasure_amd_flows.h)
    if hasattr(L, "ldpc_amd_fec_rx_flows_create"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_rx_flows_create.argtypes = [vp, i32, i32, i32, i32, C.POINTER(vp)]
        L.ldpc_amd_fec_rx_flows_destroy.argtypes = [vp]
        L.ldpc_amd_fec_rx_flows_destroy.restype = None
        L.ldpc_amd_fec_rx_flows_push_many.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp]
        L.ldpc_amd_fec_rx_flows_decode_many.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]
        L.ldpc_amd_fec_rx_flows_flush.argtypes = [vp, i32, vp, vp, C.POINTER(i32)]
        L.ldpc_amd_fec_rx_flows_decode_flush.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(i32)]
        L.ldpc_amd_fec_rx_flows_dropped.argtypes = [vp, i32]
        L.ldpc_amd_fec_rx_flows_dropped.restype = i64
    # ... fed with interleaved packets (include/ldpc_erasure_amd_flows_mixed.h)
    if hasattr(L, "ldpc_amd_fec_rx_flows_push_mixed"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_rx_flows_push_mixed.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, i32, vp, vp, vp]
        L.ldpc_amd_fec_rx_flows_decode_mixed.argtypes = [vp, i32, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
        L.ldpc_amd_fec_rx_flows_unrouted.argtypes = [vp]
        L.ldpc_amd_fec_rx_flows_unrouted.restype = i64
        L.ldpc_amd_fec_flows_demux_dev.argtypes = [vp, vp, i64, i32, vp, vp]
        L.ldpc_amd_fec_flows_demux_dev.restype = i64
        L.ldpc_amd_fec_flows_demux_info.argtypes = [vp, C.POINTER(i64)]
    # ... and its batch flush (include/ldpc_erasure_amd_flows_flush.h)
    if hasattr(L, "ldpc_amd_fec_rx_flows_flush_many"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_rx_flows_pending.argtypes = [vp, vp, vp, vp]
        L.ldpc_amd_fec_rx_flows_flush_many.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp]
        L.ldpc_amd_fec_rx_flows_decode_flush_many.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.ldpc_amd_fec_flows_flush_info.argtypes = [vp, C.POINTER(i64)]
    # datagrams of any length (include/ldpc_erasure_amd_datagrams.h)
    if hasattr(L, "ldpc_amd_fec_dgram_pack_dev"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_dgram_pack_dev.argtypes = [vp, vp, vp, i64, i32, i32, vp]
        L.ldpc_amd_fec_dgram_pack_dev.restype = i64
        L.ldpc_amd_fec_dgram_unpack_dev.argtypes = [vp, vp, vp, i64, i32, i32, i32, vp, i64, vp, vp]
        L.ldpc_amd_fec_dgram_wire_len.argtypes = [i64, vp, i32, i32, i32, vp]
        L.ldpc_amd_fec_dgram_wire_len.restype = i64
        L.ldpc_amd_fec_dgram_info.argtypes = [vp, C.POINTER(i64)]
    # the trimmed wire (include/ldpc_erasure_amd_wire_ragged.h)
    if hasattr(L, "ldpc_amd_fec_wire_trim_dev"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_wire_trim_dev.argtypes = [vp, vp, i64, i32, i32, vp, i64, vp]
        L.ldpc_amd_fec_wire_land_dev.argtypes = [vp, vp, i64, vp, i64, i32, vp, vp]
        L.ldpc_amd_fec_wire_ragged_info.argtypes = [vp, C.POINTER(i64)]
    # the link emulator (include/ldpc_erasure_amd_link.h)
    if hasattr(L, "ldpc_amd_fec_link_plan_dev"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_link_plan_dev.argtypes = [vp, C.POINTER(LinkParams), i64, vp, vp, vp, i64, vp]
        L.ldpc_amd_fec_link_apply_dev.argtypes = [vp, vp, i64, i32, vp, vp, vp, i64, vp, vp, vp]
        L.ldpc_amd_fec_link_apply_ragged_dev.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, i64, vp, i64, vp, vp]
        L.ldpc_amd_fec_link_info.argtypes = [vp, C.POINTER(i64)]
    # the windowed receiver (include/ldpc_erasure_amd_rx_window.h)
    if hasattr(L, "ldpc_amd_fec_rxw_create"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_rxw_create.argtypes = [i32, i32, i32, i32, i32, C.POINTER(vp)]
        L.ldpc_amd_fec_rxw_destroy.argtypes = [vp]
        L.ldpc_amd_fec_rxw_destroy.restype = None
        L.ldpc_amd_fec_rxw_push.argtypes = [vp, vp, vp, vp, C.POINTER(i32)]
        L.ldpc_amd_fec_rxw_push_many.argtypes = [vp, vp, C.c_long, vp, vp, vp, i32, C.POINTER(C.c_long)]
        L.ldpc_amd_fec_rxw_flush.argtypes = [vp, vp, vp, vp]
        L.ldpc_amd_fec_rxw_stats.argtypes = [vp, C.POINTER(i64)]
        L.ldpc_amd_fec_rxw_dropped.argtypes = [vp]
        L.ldpc_amd_fec_rxw_dropped.restype = C.c_long
        L.ldpc_amd_fec_rxw_state.argtypes = [vp, C.POINTER(i32), vp, C.POINTER(i64)]
        L.ldpc_amd_fec_rxw_dev_create.argtypes = [vp, i32, i32, i32, i32, i32, C.POINTER(vp)]
        L.ldpc_amd_fec_rxw_dev_destroy.argtypes = [vp]
        L.ldpc_amd_fec_rxw_dev_destroy.restype = None
        L.ldpc_amd_fec_rxw_dev_push_many.argtypes = [vp, vp, i64, vp, vp, vp, i32, C.POINTER(i64)]
        L.ldpc_amd_fec_rxw_dev_flush.argtypes = [vp, vp, vp, vp]
        L.ldpc_amd_fec_rxw_dev_decode_many.argtypes = [vp, i32, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(i64)]
        L.ldpc_amd_fec_rxw_dev_decode_flush.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        L.ldpc_amd_fec_rxw_dev_stats.argtypes = [vp, C.POINTER(i64)]
        L.ldpc_amd_fec_rxw_dev_dropped.argtypes = [vp]
        L.ldpc_amd_fec_rxw_dev_dropped.restype = i64
        L.ldpc_amd_fec_rxw_dev_state.argtypes = [vp, C.POINTER(i32), vp, C.POINTER(i64)]
        L.ldpc_amd_fec_rxw_info.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "ldpc_amd_fec_tx_ilv_layout"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_tx_ilv_layout.argtypes = [i64, i32, C.c_uint, i32, vp, vp]
        L.ldpc_amd_fec_tx_ilv_layout.restype = i64
        L.ldpc_amd_fec_encode_packets_ilv_dev.argtypes = [vp, i32, i32, i64, vp, C.c_uint, C.c_uint, i32, vp]
        L.ldpc_amd_fec_sender_ilv_info.argtypes = [vp, C.POINTER(i64)]
        L.ldpc_amd_fec_rxw_create_depth.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
        L.ldpc_amd_fec_rxw_dev_create_depth.argtypes = [vp, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
        L.ldpc_amd_fec_rxw_depth.argtypes = [vp]
        L.ldpc_amd_fec_rxw_dev_depth.argtypes = [vp]
    if hasattr(L, "ldpc_amd_fec_rxw_flows_create"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_rxw_flows_create.argtypes = [vp, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
        L.ldpc_amd_fec_rxw_flows_destroy.argtypes = [vp]
        L.ldpc_amd_fec_rxw_flows_destroy.restype = None
        L.ldpc_amd_fec_rxw_flows_push_many.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp]
        L.ldpc_amd_fec_rxw_flows_decode_many.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]
        L.ldpc_amd_fec_rxw_flows_flush_many.argtypes = [vp, vp, i32, vp, vp, vp, vp]
        L.ldpc_amd_fec_rxw_flows_decode_flush_many.argtypes = [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.ldpc_amd_fec_rxw_flows_pending.argtypes = [vp, vp, vp]
        L.ldpc_amd_fec_rxw_flows_state.argtypes = [vp, i32, C.POINTER(i32), vp, C.POINTER(i64)]
        L.ldpc_amd_fec_rxw_flows_stats.argtypes = [vp, i32, C.POINTER(i64)]
        L.ldpc_amd_fec_rxw_flows_dropped.argtypes = [vp, i32]
        L.ldpc_amd_fec_rxw_flows_dropped.restype = i64
        L.ldpc_amd_fec_rxw_flows_info.argtypes = [vp, C.POINTER(i64)]
    # ... fed with interleaved packets (include/ldpc_erasure_amd_rx_window_flows_mixed.h)
    if hasattr(L, "ldpc_amd_fec_rxw_flows_push_mixed"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_rxw_flows_push_mixed.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, i32, vp, vp, vp]
        L.ldpc_amd_fec_rxw_flows_decode_mixed.argtypes = [vp, i32, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
        L.ldpc_amd_fec_rxw_flows_unrouted.argtypes = [vp]
        L.ldpc_amd_fec_rxw_flows_unrouted.restype = i64
    # depth on the multi-flow wire (include/ldpc_erasure_amd_interleave_flows.h)
    if hasattr(L, "ldpc_amd_fec_rs_encode_packets_dev"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_rs_encode_packets_dev.argtypes = [vp, i32, i32, i64, vp, C.c_uint, C.c_uint, i32, vp]
        L.ldpc_amd_fec_rs_sender_info.argtypes = [vp, C.POINTER(i64)]
        L.ldpc_amd_fec_rxw_dev_rs_decode_many.argtypes = [vp, i32, vp, i64, vp, vp, vp, vp, vp, i32, C.POINTER(i64)]
        L.ldpc_amd_fec_rxw_dev_rs_decode_flush.argtypes = [vp, i32, vp, vp, vp, vp, vp]
        L.ldpc_amd_fec_rs_receiver_info.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "ldpc_amd_rs_decode_rows_dev"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_rs_decode_rows_dev.argtypes = [vp, i32, i32, i64, vp, vp, i64, vp, i64, vp, vp, vp, vp]
    if hasattr(L, "ldpc_amd_fec_tx_flows_ilv_layout"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_fec_tx_flows_ilv_layout.argtypes = [i32, vp, i32, vp, i32, i32, vp, vp]
        L.ldpc_amd_fec_tx_flows_ilv_layout.restype = i64
        L.ldpc_amd_fec_encode_packets_flows_ilv_dev.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32]
        L.ldpc_amd_fec_sender_flows_ilv_info.argtypes = [vp, C.POINTER(i64)]
        L.ldpc_amd_fec_rxw_flows_create_depth.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
        L.ldpc_amd_fec_rxw_flows_depth.argtypes = [vp]
    # the close rule as a value (include/ldpc_erasure_amd_rx_rule.h)
    if hasattr(L, "ldpc_amd_fec_rx_rule_default"):   # (absent from the older builds tools/ab_lib.py loads)
        rp = C.POINTER(RxRule)
        L.ldpc_amd_fec_rx_rule_default.argtypes = [i32, i32, rp]
        L.ldpc_amd_fec_rx_rule_mds.argtypes = [i32, i32, i32, i32, rp]
        L.ldpc_amd_fec_rx_rule_check.argtypes = [i32, rp]
        L.ldpc_amd_fec_rxw_create_rule.argtypes = [i32, i32, i32, i32, i32, i32, rp, C.POINTER(vp)]
        L.ldpc_amd_fec_rxw_dev_create_rule.argtypes = [vp, i32, i32, i32, i32, i32, i32, rp, C.POINTER(vp)]
        L.ldpc_amd_fec_rxw_flows_create_rule.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, rp, C.POINTER(vp)]
        L.ldpc_amd_fec_rxw_get_rule.argtypes = [vp, rp]
        L.ldpc_amd_fec_rxw_dev_get_rule.argtypes = [vp, rp]
        L.ldpc_amd_fec_rxw_flows_get_rule.argtypes = [vp, rp]
    # frames out / frames in (include/ldpc_erasure_amd_frames.h)
    L.ldpc_amd_decode_frames.argtypes = [vp, i32, i32, i64, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, C.c_uint]
    L.ldpc_amd_rs_info.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.ldpc_amd_rs_decode_frames.argtypes = [vp, i32, i32, i64, vp, vp, vp, vp, vp, C.c_uint]
    # word-sized symbols (include/ldpc_erasure_amd_words.h)
    if hasattr(L, "ldpc_amd_set_symbol_unit"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_set_symbol_unit.argtypes = [vp, i32]
        L.ldpc_amd_get_symbol_unit.argtypes = [vp]
    L.ldpc_amd_data_out.argtypes = [vp, vp, i32, C.c_long, C.POINTER(ErrorType)]
    L.ldpc_amd_set_profiling.argtypes = [vp, i32]
    L.ldpc_amd_get_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i64)]
    L.ldpc_amd_last_plan.argtypes = [vp, C.POINTER(i32)]
    if hasattr(L, "ldpc_amd_ml_stats"):   # (absent from the older builds tools/ab_lib.py loads)
        L.ldpc_amd_ml_stats.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.ldpc_amd_profile_kernel_name.argtypes = [vp, i32]
    L.ldpc_amd_profile_kernel_name.restype = C.c_char_p
    L.ldpc_amd_selftest.argtypes = [vp]
    L.ldpc_amd_copy_probe.argtypes = [vp, vp, vp, C.c_uint64, C.c_int, C.POINTER(C.c_double)]
    L.ldpc_amd_gf_tables.argtypes = [vp, vp]
    L.ldpc_amd_version.restype = C.c_char_p
    _lib = L
    return L


def gf_tables():
    """(mult[256,256], inv[256]) the kernels use -- host computation, no GPU needed."""
    L = load_library()
    mult = np.zeros((256, 256), dtype=np.uint8)
    inv = np.zeros(256, dtype=np.uint8)
    L.ldpc_amd_gf_tables(mult.ctypes.data, inv.ctypes.data)
    return mult, inv


def fec_rx_rule_default(n, k):
    """The close rule the windowed receivers follow when none is given (include/ldpc_erasure_amd_rx_rule.h), as the 4-tuple
    (c_hi, later_hi, c_lo, later_lo) = (kd + 1, 11, km + 1, 101).  Host arithmetic, no GPU needed."""
    r = RxRule()
    if load_library().ldpc_amd_fec_rx_rule_default(n, k, C.byref(r)) != 0:
        raise LdpcAmdError(f"fec_rx_rule_default: need 0 < k < n <= 65536 (n={n} k={k})")
    return (r.c_hi, r.later_hi, r.c_lo, r.later_lo)


def fec_rx_rule_mds(n, k, depth=1, giveup=0):
    """The close rule for a code that decodes from any k symbols (Reed-Solomon) on a wire that is roughly in order: (k, 1, 0, giveup),
    giveup == 0 meaning max(1, depth * k // 2).  Slot 0 leaves at its k-th symbol once a later group has begun, and in any case once
    the later groups have sent `giveup` packets (include/ldpc_erasure_amd_rx_rule.h)."""
    r = RxRule()
    if load_library().ldpc_amd_fec_rx_rule_mds(n, k, depth, giveup, C.byref(r)) != 0:
        raise LdpcAmdError(f"fec_rx_rule_mds: bad arguments (n={n} k={k} depth={depth} giveup={giveup})")
    return (r.c_hi, r.later_hi, r.c_lo, r.later_lo)


def _rx_rule(rule):
    """A 4-tuple (c_hi, later_hi, c_lo, later_lo) as the C struct."""
    rule = tuple(int(v) for v in rule)
    if len(rule) != 4:
        raise LdpcAmdError("a close rule is a 4-tuple (c_hi, later_hi, c_lo, later_lo)")
    return RxRule(*rule)


def code_params(code_ind):
    L = load_library()
    p = (C.c_int * 6)()
    if L.ldpc_amd_code_params(code_ind, p) != OK:
        raise LdpcAmdError(f"no built-in code {code_ind}")
    return list(p)


def fec_tx_flows_layout(frame_begin, n, order):
    """Where the multi-flow sender puts its packets (host arithmetic, no GPU needed): frame_begin = nflows + 1 frame indices, flow f
    owns the frames frame_begin[f] .. frame_begin[f+1]-1.  Returns (first int64 [F], stride int32 [F]): row j of frame t is packet
    first[t] + j * stride[t] in the order TX_SEGMENTED or TX_ROUND_ROBIN (include/ldpc_erasure_amd_sender_flows.h)."""
    L = load_library()
    fb = np.ascontiguousarray(frame_begin, dtype=np.int64)
    if fb.ndim != 1 or fb.shape[0] < 2:
        raise LdpcAmdError("fec_tx_flows_layout: frame_begin must hold nflows + 1 >= 2 entries")
    F = max(int(fb[-1]), 0)
    first = np.zeros(F, dtype=np.int64)
    stride = np.zeros(F, dtype=np.int32)
    rc = L.ldpc_amd_fec_tx_flows_layout(fb.shape[0] - 1, fb.ctypes.data, n, order, first.ctypes.data, stride.ctypes.data)
    if rc < 0:
        raise LdpcAmdError(f"fec_tx_flows_layout = {rc}: bad nflows / frame_begin / n / order")
    assert rc == F * n
    return first, stride


def fec_tx_ilv_layout(nframes, n, block0, depth):
    """Where the block-interleaved sender puts its packets (host arithmetic, no GPU needed): nframes frames of n packets numbered
    from block0 on, `depth` (1, 2, 4, 8 or 16) consecutive blocks of one group sent one row of each in turn.  Returns (first int64
    [nframes], stride int32 [nframes]): row j of frame f is packet first[f] + j * stride[f] (include/ldpc_erasure_amd_interleave.h)."""
    L = load_library()
    F = max(int(nframes), 0)
    first = np.zeros(F, dtype=np.int64)
    stride = np.zeros(F, dtype=np.int32)
    rc = L.ldpc_amd_fec_tx_ilv_layout(int(nframes), n, block0 & 0xFF, depth, first.ctypes.data, stride.ctypes.data)
    if rc < 0:
        raise LdpcAmdError(f"fec_tx_ilv_layout = {rc}: bad nframes / n / depth")
    assert rc == F * n
    return first, stride


def fec_tx_flows_ilv_layout(frame_begin, n, block0, depth, order):
    """fec_tx_flows_layout with every flow's blocks interleaved to `depth` (host arithmetic, no GPU needed): flow f's frames are
    numbered from block0[f] on (a scalar stands for every flow) and its substream is fec_tx_ilv_layout's.  TX_ROUND_ROBIN with
    depth > 1 needs whole aligned groups, block0[f] % depth == 0 and a frame count that is a multiple of depth for every flow
    (include/ldpc_erasure_amd_interleave_flows.h).  Returns (first int64 [F], stride int32 [F])."""
    L = load_library()
    fb = np.ascontiguousarray(frame_begin, dtype=np.int64)
    if fb.ndim != 1 or fb.shape[0] < 2:
        raise LdpcAmdError("fec_tx_flows_ilv_layout: frame_begin must hold nflows + 1 >= 2 entries")
    nflows = fb.shape[0] - 1
    blk = np.ascontiguousarray(np.broadcast_to(np.asarray(block0, dtype=np.int64) & 0xFF, (nflows,)), dtype=np.uint8)
    F = max(int(fb[-1]), 0)
    first = np.zeros(F, dtype=np.int64)
    stride = np.zeros(F, dtype=np.int32)
    rc = L.ldpc_amd_fec_tx_flows_ilv_layout(nflows, fb.ctypes.data, n, blk.ctypes.data, depth, order, first.ctypes.data, stride.ctypes.data)
    if rc < 0:
        raise LdpcAmdError(f"fec_tx_flows_ilv_layout = {rc}: bad nflows / frame_begin / n / depth / order, or part groups in TX_ROUND_ROBIN")
    assert rc == F * n
    return first, stride


def _dgram_offsets(offsets):
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    if off.ndim != 1 or off.shape[0] < 1:
        raise LdpcAmdError("datagram offsets must be a 1-D array of N + 1 >= 1 entries")
    return off


def fec_datagram_wire_len(offsets, n, k, S):
    """Bytes of every wire packet that have to be transmitted when the datagrams offsets[i] .. offsets[i+1] are packed and sent
    (host arithmetic, no GPU needed; include/ldpc_erasure_amd_datagrams.h): int32 [F*n], 8 + 4 + L for a source row (12 for a
    filler), 8 + S for a repair row.  Every byte of a packet behind that is zero."""
    L = load_library()
    off = _dgram_offsets(offsets)
    N = off.shape[0] - 1
    wl = np.zeros(max(-(-N // max(k, 1)) * max(n, 0), 0), dtype=np.int32)
    rc = L.ldpc_amd_fec_dgram_wire_len(N, off.ctypes.data, n, k, S, wl.ctypes.data)
    if rc < 0:
        raise LdpcAmdError(f"fec_dgram_wire_len = {rc}: bad offsets / n / k / S")
    assert rc == wl.shape[0]
    return wl


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _sender_shape(source, n, k, out):
    """The single-stream senders' shape contract: source a torch uint8 tensor [F][k][S] (or [F][k] for S = 1), out None (allocated
    beside source) or a torch uint8 tensor [F*n][8+S].  Returns (F, S, out)."""
    import torch
    assert _is_torch(source) and source.dtype == torch.uint8 and source.ndim in (2, 3)
    F = source.shape[0]
    S = 1 if source.ndim == 2 else source.shape[2]
    assert source.shape[1] == k
    if out is None:
        out = torch.empty((F * n, 8 + S), dtype=torch.uint8, device=source.device)
    assert tuple(out.shape) == (F * n, 8 + S) and out.dtype == torch.uint8
    return F, S, out


def _ptr(x):
    if x is None:
        return None
    if _is_torch(x):
        assert x.is_contiguous()
        return x.data_ptr()
    assert x.flags["C_CONTIGUOUS"]
    return x.ctypes.data


class Context:
    def __init__(self, device=0):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.ldpc_amd_init(device, C.byref(h))
        if rc != OK:
            raise LdpcAmdError(f"ldpc_amd_init({device}) = {rc}: {self._L.ldpc_amd_last_error(None).decode()}")
        self._h = h
        self.device = device

    # -- life-cycle
    def close(self):
        if getattr(self, "_h", None):
            self._L.ldpc_amd_cleanup(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise LdpcAmdError(f"{what} = {rc}: {self._L.ldpc_amd_last_error(self._h).decode()}")
        return rc

    def _info(self, fn, ctype, keys, paths=None):
        """The ..._info pattern: the leading words of ldpc_amd_<fn>'s four under `keys`; paths: the names of the word "path"."""
        info = (ctype * 4)()
        self._check(getattr(self._L, "ldpc_amd_" + fn)(self._h, info), fn)
        d = {kd: int(v) for kd, v in zip(keys, info)}
        if paths:
            d["path"] = paths[d["path"]]
        return d

    def set_stream(self, stream_handle):
        self._check(self._L.ldpc_amd_set_stream(self._h, C.c_void_p(stream_handle)), "set_stream")

    def synchronize(self):
        self._check(self._L.ldpc_amd_synchronize(self._h), "synchronize")

    def configure(self, key, value=None):
        """Sets a tuning / diagnostic knob of this context ("SCATTER_B", "LDPC_AMD_ML_SOLVE", ...); value None restores the
        default.  The LDPC_AMD_* environment variables are only the initial values, read once when the context is created."""
        v = None if value is None else str(value).encode()
        self._check(self._L.ldpc_amd_configure(self._h, key.encode(), v), "configure")

    def knobs(self):
        """The knobs of this context that are NOT at their shipped default, "NAME=value NAME=value" ('' = all defaults)."""
        buf = C.create_string_buffer(1024)
        self._check(self._L.ldpc_amd_knobs(self._h, buf, 1024), "knobs")
        return buf.value.decode()

    def configure_many(self, knobs):
        """{key: value or None} -> configure() for each."""
        for k, v in knobs.items():
            self.configure(k, v)

    def set_symbol_unit(self, unit):
        """16 (default): S is 1 or a multiple of 16.  4: S is 1 or any multiple of 4 that is at least 16, on every entry point of
        this context that takes a symbol length (include/ldpc_erasure_amd_words.h).  Not a knob: it changes which inputs are
        accepted, never the bytes of an input both units accept.  Any other unit: LdpcAmdError, the context keeps its unit."""
        self._check(self._L.ldpc_amd_set_symbol_unit(self._h, int(unit)), "set_symbol_unit")

    def symbol_unit(self):
        return self._check(self._L.ldpc_amd_get_symbol_unit(self._h), "get_symbol_unit")

    def set_profiling(self, enable):
        """False / 0: off; True / 1: one bracket per kind of a call; 2: + the nested tier-2 and solve-kernel brackets."""
        self._check(self._L.ldpc_amd_set_profiling(self._h, int(enable)), "set_profiling")

    def get_profile(self):
        """{'peel': (ms, launches), 'apply': ..., 'ml': ..., 'apply_tier2': ..., 'ml_solve': ...} since the last call (synchronises)."""
        ms = (C.c_double * len(PROF_KINDS))()
        cnt = (C.c_int64 * len(PROF_KINDS))()
        self._check(self._L.ldpc_amd_get_profile(self._h, ms, cnt), "get_profile")
        return {name: (ms[i], cnt[i]) for i, name in enumerate(PROF_KINDS)}

    def profile_kernel_names(self):
        """{'peel': name, 'apply': name, 'ml': name}: the kernel instantiation the last launch of each kind used."""
        return {name: self._L.ldpc_amd_profile_kernel_name(self._h, i).decode() for i, name in enumerate(PROF_KINDS)}

    def rs_kernel_name(self):
        """The kernel instantiation of the last Reed-Solomon decode launch ('' before the first)."""
        return self._L.ldpc_amd_profile_kernel_name(self._h, NAME_RS).decode()

    def encode_kernel_name(self):
        """The kernel of the last encode launch with S > 1, the gather kernel included ('' before the first)."""
        return self._L.ldpc_amd_profile_kernel_name(self._h, NAME_ENCODE).decode()

    def last_plan(self):
        info = (C.c_int * 8)()
        self._check(self._L.ldpc_amd_last_plan(self._h, info), "last_plan")
        keys = ("frames_per_workgroup", "frames_per_cu", "tables_in_global", "peel_lds_bytes", "peel_lds_per_frame",
                "packet_bytes_per_workgroup", "tier1_cap", "two_tiers")
        return dict(zip(keys, list(info)))

    def ml_stats(self):
        """ML stage of the last decode: residual frames, frames solved through the fast path, frames its consistency test flagged
        (redone exactly), frames whose schedule did not fit the arena.  Synchronises."""
        st = (C.c_longlong * 4)()
        self._check(self._L.ldpc_amd_ml_stats(self._h, st), "ml_stats")
        return dict(zip(("residual_frames", "fast_path_frames", "flagged_frames", "deferred_frames"), [int(x) for x in st]))

    def copy_probe(self, src, dst, reps=10, nbytes=None):
        """Best single-launch device time (ms) of a streaming copy src -> dst (torch CUDA uint8 tensors of equal size;
        nbytes: copy only that many leading bytes), over `reps` launches of each of the probe's launch shapes."""
        ms = C.c_double(0.0)
        nbytes = min(nbytes or (1 << 62), src.numel() * src.element_size())
        self._check(self._L.ldpc_amd_copy_probe(self._h, src.data_ptr(), dst.data_ptr(), nbytes & ~15, reps, C.byref(ms)), "copy_probe")
        return ms.value

    def selftest(self):
        self._check(self._L.ldpc_amd_selftest(self._h), "selftest")

    # -- codes
    def load_builtin_code(self, code_ind, coef_seed):
        return self._check(self._L.ldpc_amd_load_builtin_code(self._h, code_ind, coef_seed), "load_builtin_code")

    def register_code(self, code):
        rp = np.ascontiguousarray(code.row_ptr, dtype=np.uint32)
        cols = np.ascontiguousarray(code.cols, dtype=np.uint16)
        coefs = np.ascontiguousarray(code.coefs, dtype=np.uint8)
        return self._check(self._L.ldpc_amd_register_code(self._h, code.n, code.k, rp.ctypes.data, cols.ctypes.data,
                                                          coefs.ctypes.data), "register_code")

    def code_info(self, code):
        n, k, nnz = C.c_int(), C.c_int(), C.c_int()
        self._check(self._L.ldpc_amd_code_info(self._h, code, C.byref(n), C.byref(k), C.byref(nnz)), "code_info")
        return n.value, k.value, nnz.value

    def code_csr(self, code):
        n, k, nnz = self.code_info(code)
        rp = np.zeros(n - k + 1, dtype=np.uint32)
        cols = np.zeros(nnz, dtype=np.uint16)
        coefs = np.zeros(nnz, dtype=np.uint8)
        self._check(self._L.ldpc_amd_code_csr(self._h, code, rp.ctypes.data, cols.ctypes.data, coefs.ctypes.data), "code_csr")
        return rp, cols, coefs

    # -- hot path
    def decode(self, code, sym, erased, max_sweeps=10, do_ml=1, out=None, sweeps=None, residual=None, status=None,
               inplace=False):
        """sym [F,n,S] (or [F,n] for S=1) uint8, erased [F,n] uint8.
        numpy in -> numpy out (synchronous).  torch CUDA tensors in -> torch out (asynchronous).
        Returns (out, sweeps, residual, status)."""
        n, k, _ = self.code_info(code)
        dev = _is_torch(sym)
        F = sym.shape[0]
        S = 1 if sym.ndim == 2 else sym.shape[2]
        assert sym.shape[1] == n and tuple(erased.shape) == (F, n)
        if dev:
            import torch
            mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=sym.device)  # noqa: E731
            if inplace:
                out = sym
            out = mk(tuple(sym.shape), torch.uint8) if out is None else out
            sweeps = mk((F,), torch.int32) if sweeps is None else sweeps
            residual = mk((F,), torch.int32) if residual is None else residual
            status = mk((F,), torch.int32) if status is None else status
        else:
            sym = np.ascontiguousarray(sym, dtype=np.uint8)
            erased = np.ascontiguousarray(erased, dtype=np.uint8)
            out = np.empty_like(sym) if out is None else out
            sweeps = np.empty(F, dtype=np.int32) if sweeps is None else sweeps
            residual = np.empty(F, dtype=np.int32) if residual is None else residual
            status = np.empty(F, dtype=np.int32) if status is None else status
        self._check(self._L.ldpc_amd_decode_batch(self._h, code, S, F, _ptr(sym), _ptr(erased), max_sweeps, do_ml,
                                                  _ptr(out), _ptr(sweeps), _ptr(residual), _ptr(status),
                                                  (DEVICE_PTRS if dev else 0) | (INPLACE if inplace else 0)), "decode_batch")
        return out, sweeps, residual, status

    def decode_frames(self, code, sym, erased, max_sweeps=10, do_ml=1, inplace=False):
        """decode() plus the frame format on the way out: erased_out [F,n] uint8 is 1 exactly where out holds neither a received
        nor a recovered symbol (all zero for status 0 / 1, the erasures the sweeps left for status 2 / 3), residual_src [F] int32
        counts those among the first k.  numpy in -> numpy out, torch in -> torch out, like decode().
        Returns DecodedFrames(out, sweeps, residual, status, erased_out, residual_src)."""
        n, k, _ = self.code_info(code)
        dev = _is_torch(sym)
        F = sym.shape[0]
        S = 1 if sym.ndim == 2 else sym.shape[2]
        assert sym.shape[1] == n and tuple(erased.shape) == (F, n)
        if dev:
            import torch
            mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=sym.device)  # noqa: E731
            out = sym if inplace else mk(tuple(sym.shape), torch.uint8)
            sweeps, residual, status, residual_src = (mk((F,), torch.int32) for _ in range(4))
            erased_out = mk((F, n), torch.uint8)
        else:
            sym = np.ascontiguousarray(sym, dtype=np.uint8)
            erased = np.ascontiguousarray(erased, dtype=np.uint8)
            out = np.empty_like(sym)
            sweeps, residual, status, residual_src = (np.empty(F, dtype=np.int32) for _ in range(4))
            erased_out = np.empty((F, n), dtype=np.uint8)
        self._check(self._L.ldpc_amd_decode_frames(self._h, code, S, F, _ptr(sym), _ptr(erased), max_sweeps, do_ml,
                                                   _ptr(out), _ptr(sweeps), _ptr(residual), _ptr(status), _ptr(erased_out),
                                                   _ptr(residual_src), (DEVICE_PTRS if dev else 0) | (INPLACE if inplace else 0)),
                    "decode_frames")
        return DecodedFrames(out, sweeps, residual, status, erased_out, residual_src)

    def encode_info(self, code):
        """Static schedules of the code's systematic encoder: levels of the parity triangle, groups of the level-collapsed
        schedule (0: none), accumulators pulled, scatter entries left, longest pull list, and whether the last packet-mode
        encode of this context ran the grouped schedule."""
        info = (C.c_int * 6)()
        self._check(self._L.ldpc_amd_encode_info(self._h, code, info), "encode_info")
        return dict(zip(("levels", "groups", "pull_entries", "scatter_entries", "max_pull", "last_encode_grouped"), list(info)))

    def encode(self, code, source, out=None):
        """source [F,k,S] (or [F,k]) -> codeword [F,n,S] (or [F,n])."""
        n, k, _ = self.code_info(code)
        dev = _is_torch(source)
        F = source.shape[0]
        S = 1 if source.ndim == 2 else source.shape[2]
        assert source.shape[1] == k
        shape = (F, n) if source.ndim == 2 else (F, n, S)
        if dev:
            import torch
            out = torch.empty(shape, dtype=torch.uint8, device=source.device) if out is None else out
        else:
            source = np.ascontiguousarray(source, dtype=np.uint8)
            out = np.empty(shape, dtype=np.uint8) if out is None else out
        self._check(self._L.ldpc_amd_encode_batch(self._h, code, S, F, _ptr(source), _ptr(out), DEVICE_PTRS if dev else 0),
                    "encode_batch")
        return out

    # -- Reed-Solomon
    def rs_create(self, n, k):
        return self._check(self._L.ldpc_amd_rs_create(self._h, n, k), "rs_create")

    def rs_generator(self, rs, n, k):
        g = np.zeros((k, n), dtype=np.uint8)
        self._check(self._L.ldpc_amd_rs_generator(self._h, rs, g.ctypes.data), "rs_generator")
        return g

    def rs_encode(self, rs, n, k, source, out=None):
        """source [B,k,S] or [B,k] -> codewords [B,n,S] or [B,n], into `out` (contiguous, of that shape, where source is) if given."""
        dev = _is_torch(source)
        B = source.shape[0]
        S = 1 if source.ndim == 2 else source.shape[2]
        shape = (B, n) if source.ndim == 2 else (B, n, S)
        if out is not None:
            assert _is_torch(out) == dev and tuple(out.shape) == shape
        if dev:
            import torch
            if out is None:
                out = torch.empty(shape, dtype=torch.uint8, device=source.device)
        else:
            source = np.ascontiguousarray(source, dtype=np.uint8)
            if out is None:
                out = np.empty(shape, dtype=np.uint8)
        self._check(self._L.ldpc_amd_rs_encode_batch(self._h, rs, S, B, _ptr(source), _ptr(out), DEVICE_PTRS if dev else 0),
                    "rs_encode_batch")
        return out

    def rs_decode(self, rs, recv_idx, recv_val, out=None):
        """recv_idx [B,k] uint16 (0-based ascending), recv_val [B,k,S] or [B,k] -> msg like recv_val."""
        dev = _is_torch(recv_val)
        B = recv_val.shape[0]
        S = 1 if recv_val.ndim == 2 else recv_val.shape[2]
        if dev:
            import torch
            msg = torch.empty_like(recv_val) if out is None else out
        else:
            recv_idx = np.ascontiguousarray(recv_idx, dtype=np.uint16)
            recv_val = np.ascontiguousarray(recv_val, dtype=np.uint8)
            msg = np.empty_like(recv_val) if out is None else out
        self._check(self._L.ldpc_amd_rs_decode_batch(self._h, rs, S, B, _ptr(recv_idx), _ptr(recv_val), _ptr(msg),
                                                     DEVICE_PTRS if dev else 0), "rs_decode_batch")
        return msg

    def rs_info(self, rs):
        """(n, k) of an RS handle."""
        n, k = C.c_int(), C.c_int()
        self._check(self._L.ldpc_amd_rs_info(self._h, rs, C.byref(n), C.byref(k)), "rs_info")
        return n.value, k.value

    def rs_decode_frames(self, rs, sym, erased, out=None):
        """sym [B,n,S] (or [B,n] for S=1) uint8, erased [B,n] uint8 -> RsDecodedFrames(msg [B,k,S] or [B,k], received [B] int32,
        status [B] int32).  Per block the first k received symbols are decoded (the rest is not read); a block that received
        fewer than k is all zero with status RS_ST_SHORT.  numpy in -> numpy out, torch in -> torch out; `out`, if given, is the
        (msg, received, status) of those shapes to write into, where sym is."""
        n, k = self.rs_info(rs)
        dev = _is_torch(sym)
        B = sym.shape[0]
        S = 1 if sym.ndim == 2 else sym.shape[2]
        assert sym.shape[1] == n and tuple(erased.shape) == (B, n)
        shape = (B, k) if sym.ndim == 2 else (B, k, S)
        if out is not None:
            msg, received, status = out
            assert all(_is_torch(t) == dev for t in out) and tuple(msg.shape) == shape
            assert tuple(received.shape) == (B,) and tuple(status.shape) == (B,)
            if not dev:
                sym = np.ascontiguousarray(sym, dtype=np.uint8)
                erased = np.ascontiguousarray(erased, dtype=np.uint8)
        elif dev:
            import torch
            msg = torch.empty(shape, dtype=torch.uint8, device=sym.device)
            received, status = (torch.empty((B,), dtype=torch.int32, device=sym.device) for _ in range(2))
        else:
            sym = np.ascontiguousarray(sym, dtype=np.uint8)
            erased = np.ascontiguousarray(erased, dtype=np.uint8)
            msg = np.empty(shape, dtype=np.uint8)
            received, status = (np.empty(B, dtype=np.int32) for _ in range(2))
        self._check(self._L.ldpc_amd_rs_decode_frames(self._h, rs, S, B, _ptr(sym), _ptr(erased), _ptr(msg), _ptr(received),
                                                      _ptr(status), DEVICE_PTRS if dev else 0), "rs_decode_frames")
        return RsDecodedFrames(msg, received, status)

    def rs_decode_rows(self, rs, src, packets=None, stage=None, out=None, erased_out=None):
        """The RS decoder on rows in place (include/ldpc_erasure_amd_rs_rows.h).  src: torch uint32 / int32 [B][n] on this context's
        device, one source word per (block, symbol): p = the payload of packets[p], ROW_STAGED | i = stage[i], ROW_ERASED; packets
        torch uint8 [P][8+S], stage torch uint8 [R][S] (each may be None).  A word that names a packet >= P or a staged row >= R
        counts as erased.  -> RsDecodedFrames(msg [B,k,S], received [B] int32, status [B] int32): what rs_decode_frames returns for
        the frames the words describe.  `out`: the (msg, received, status) to write into; erased_out: torch uint8 [B][n] that
        receives the flags after vetting.  Asynchronous on the context's stream."""
        import torch
        n, k = self.rs_info(rs)
        B = src.shape[0]
        assert _is_torch(src) and src.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and tuple(src.shape) == (B, n) and src.is_contiguous()
        assert packets is not None or stage is not None, "packets or stage: one of them says what S is"
        S = packets.shape[1] - 8 if packets is not None else stage.shape[1]
        for a, width in ((packets, 8 + S), (stage, S)):
            assert a is None or (_is_torch(a) and a.dtype == torch.uint8 and a.ndim == 2 and a.shape[1] == width and a.is_contiguous())
        if out is None:
            out = (torch.empty((B, k, S), dtype=torch.uint8, device=src.device),
                   torch.empty((B,), dtype=torch.int32, device=src.device), torch.empty((B,), dtype=torch.int32, device=src.device))
        msg, received, status = out
        assert tuple(msg.shape) == (B, k, S) and msg.is_contiguous() and tuple(received.shape) == (B,) and tuple(status.shape) == (B,)
        assert erased_out is None or (tuple(erased_out.shape) == (B, n) and erased_out.is_contiguous())
        self._check(self._L.ldpc_amd_rs_decode_rows_dev(self._h, rs, S, B, _ptr(src), _ptr(packets) if packets is not None else None,
                                                        0 if packets is None else packets.shape[0], _ptr(stage) if stage is not None else None,
                                                        0 if stage is None else stage.shape[0], _ptr(msg), _ptr(received), _ptr(status),
                                                        _ptr(erased_out) if erased_out is not None else None), "rs_decode_rows_dev")
        return RsDecodedFrames(msg, received, status)

    def rs_bad_blocks(self):
        """Blocks of the last rs_decode whose positions were malformed (decoded to zeros).  Synchronises."""
        c = C.c_longlong(0)
        self._check(self._L.ldpc_amd_rs_bad_blocks(self._h, C.byref(c)), "rs_bad_blocks")
        return c.value

    # -- synthetic inputs on the device (torch tensors)
    def synth_source(self, seed, frame0, nframes, k, S, out):
        self._check(self._L.ldpc_amd_synth_source(self._h, seed, frame0, nframes, k, S, _ptr(out)), "synth_source")
        return out

    def synth_erasures_uniform(self, seed, frame0, nframes, n, per, out):
        self._check(self._L.ldpc_amd_synth_erasures_uniform(self._h, seed, frame0, nframes, n, float(per), _ptr(out)),
                    "synth_erasures_uniform")
        return out

    def synth_erasures_bursty(self, seed, frame0, nframes, n, alpha, beta, bias, out):
        self._check(self._L.ldpc_amd_synth_erasures_bursty(self._h, seed, frame0, nframes, n, float(alpha), float(beta),
                                                           float(bias), _ptr(out)), "synth_erasures_bursty")
        return out

    # -- FPGA harness trio (OpenCL/host/src/main.cpp:578-626)
    def data_in(self, nldpc, seed, per_numerator_div_64, code_ind, num_frames):
        self._check(self._L.ldpc_amd_data_in(self._h, None, nldpc, seed, per_numerator_div_64, code_ind, num_frames), "data_in")

    def ldpc_erasure_decoder(self, num_iter, code_ind):
        self._check(self._L.ldpc_amd_ldpc_erasure_decoder(self._h, num_iter, code_ind), "ldpc_erasure_decoder")

    def ldpc_erasure_decoder_perf_tests(self, num_iter, code_ind):
        self._check(self._L.ldpc_amd_ldpc_erasure_decoder_perf_tests(self._h, num_iter, code_ind), "ldpc_erasure_decoder_perf_tests")

    def fpga_frame_stats(self, num_frames):
        """(systematic erasures left, iterations) per frame of the last FPGA-style decoder call."""
        left = np.zeros(num_frames, dtype=np.int32)
        its = np.zeros(num_frames, dtype=np.int32)
        self._check(self._L.ldpc_amd_fpga_frame_stats(self._h, num_frames, left.ctypes.data, its.ctypes.data), "fpga_frame_stats")
        return left, its

    def data_out(self, code_ind, num_frames):
        st = ErrorType()
        self._check(self._L.ldpc_amd_data_out(self._h, None, code_ind, num_frames, C.byref(st)), "data_out")
        return st.num_LDPC_errors, st.num_RS_errors

    # -- device-resident wire path (include/ldpc_erasure_amd_wire_dev.h)
    def fec_packetize_device(self, frames, fec_class=1, block0=0, out=None):
        """frames: torch uint8 [F][n][S] on this context's device -> packets [F*n][8+S] (the bytes of fec_packetize).
        Asynchronous on the context's stream."""
        import torch
        assert _is_torch(frames) and frames.dtype == torch.uint8 and frames.ndim == 3
        F, n, S = frames.shape
        if out is None:
            out = torch.empty((F * n, 8 + S), dtype=torch.uint8, device=frames.device)
        assert tuple(out.shape) == (F * n, 8 + S) and out.dtype == torch.uint8
        self._check(self._L.ldpc_amd_fec_packetize_dev(self._h, _ptr(frames), F, n, S, fec_class, block0, _ptr(out)),
                    "fec_packetize_dev")
        return out

    def fec_rx_device(self, n, k, S):
        """A two-buffer reassembler whose packets and blocks stay on this context's device (FecRxDevice)."""
        return FecRxDevice(self, n, k, S)

    # -- the fused sender (include/ldpc_erasure_amd_sender.h)
    def fec_encode_packets_device(self, code, source, fec_class=1, block0=0, out=None):
        """source: torch uint8 [F][k][S] (or [F][k] for S = 1) on this context's device -> packets [F*n][8+S], the bytes of
        fec_packetize_device(encode(code, source)) without the codeword array in between where the encoder can write the
        packets itself (fec_sender_info() says which path ran).  Asynchronous on the context's stream."""
        n, k, _ = self.code_info(code)
        F, S, out = _sender_shape(source, n, k, out)
        self._check(self._L.ldpc_amd_fec_encode_packets_dev(self._h, code, S, F, _ptr(source), fec_class, block0, _ptr(out)),
                    "fec_encode_packets_dev")
        return out

    def fec_sender_info(self):
        """{"path": "none" | "fused" | "composed" of the last fec_encode_packets_device call, "scratch_bytes": codeword scratch the
        context holds for the composed path}."""
        return self._info("fec_sender_info", C.c_int, ("path", "scratch_bytes"), SENDER_PATHS)

    # -- the multi-flow sender (include/ldpc_erasure_amd_sender_flows.h)
    def fec_encode_packets_flows_device(self, code, source, frame_begin, fec_class, block0, order, out=None, want_flow_of=True):
        """source: torch uint8 [F][k][S] (or [F][k] for S = 1) on this context's device, the frames of nflows streams side by side:
        flow f owns the frames frame_begin[f] .. frame_begin[f+1]-1 and sends them with class fec_class[f], numbered from block0[f]
        on (a scalar stands for every flow).  Returns (packets torch uint8 [F*n][8+S], flow_of torch int32 [F*n] or None,
        packet_begin int64 [nflows+1]): every flow's packets as fec_encode_packets_device makes them, flow after flow (order =
        TX_SEGMENTED: FecRxFlows.decode_many's input with packet_begin) or one packet of every flow in turn (TX_ROUND_ROBIN:
        decode_mixed's input with flow_of).  fec_sender_flows_info() says which path ran.  Asynchronous on the context's stream."""
        return self._encode_packets_flows(code, source, frame_begin, fec_class, block0, order, out, want_flow_of, None)

    def _encode_packets_flows(self, code, source, frame_begin, fec_class, block0, order, out, want_flow_of, depth):
        """The two multi-flow senders' common part; depth None: ldpc_amd_fec_encode_packets_flows_dev."""
        import torch
        n, k, _ = self.code_info(code)
        F, S, out = _sender_shape(source, n, k, out)
        fb = np.ascontiguousarray(frame_begin, dtype=np.int64)
        assert fb.ndim == 1 and fb.shape[0] >= 2 and int(fb[-1]) == F
        nflows = fb.shape[0] - 1
        cls = np.ascontiguousarray(np.broadcast_to(np.asarray(fec_class, dtype=np.int64) & 0xFF, (nflows,)), dtype=np.uint8)
        blk = np.ascontiguousarray(np.broadcast_to(np.asarray(block0, dtype=np.int64) & 0xFF, (nflows,)), dtype=np.uint8)
        flow_of = torch.empty(F * n, dtype=torch.int32, device=source.device) if want_flow_of else None
        pb = np.zeros(nflows + 1, dtype=np.int64)
        args = (self._h, code, S, nflows, fb.ctypes.data, _ptr(source) if F else None, cls.ctypes.data, blk.ctypes.data, order,
                _ptr(out) if F else None, _ptr(flow_of) if want_flow_of and F else None, pb.ctypes.data)
        if depth is None:
            self._check(self._L.ldpc_amd_fec_encode_packets_flows_dev(*args), "fec_encode_packets_flows_dev")
        else:
            self._check(self._L.ldpc_amd_fec_encode_packets_flows_ilv_dev(*args, depth), "fec_encode_packets_flows_ilv_dev")
        return out, flow_of, pb

    def fec_sender_flows_info(self):
        """{"path": "none" | "fused" | "composed" of the last fec_encode_packets_flows_device call, "scratch_bytes": codeword scratch
        the context holds for the composed paths, "descriptor_bytes": descriptor memory it holds, "frames": frames of that call}."""
        return self._info("fec_sender_flows_info", C.c_int64, _SENDER_KEYS, SENDER_PATHS)

    # -- ... with every flow interleaved to a depth (include/ldpc_erasure_amd_interleave_flows.h)
    def fec_encode_packets_flows_interleaved_device(self, code, source, frame_begin, fec_class, block0, order, depth, out=None, want_flow_of=True):
        """fec_encode_packets_flows_device with every flow's blocks interleaved to `depth` (1, 2, 4, 8 or 16): flow f's packets are
        those of fec_encode_packets_interleaved_device for its frames, and the flows go back to back (TX_SEGMENTED: the input of
        FecRxWindowFlows(depth=depth).decode_many with packet_begin) or one packet of every flow in turn (TX_ROUND_ROBIN: decode_mixed's
        with flow_of; depth > 1 then needs whole aligned groups, block0[f] % depth == 0 and a multiple of depth frames per flow).  Row j
        of frame t sits at first[t] + j * stride[t] of fec_tx_flows_ilv_layout.  fec_sender_flows_ilv_info() says which path ran."""
        return self._encode_packets_flows(code, source, frame_begin, fec_class, block0, order, out, want_flow_of, depth)

    def fec_sender_flows_ilv_info(self):
        """fec_sender_flows_info() for the last fec_encode_packets_flows_interleaved_device call."""
        return self._info("fec_sender_flows_ilv_info", C.c_int64, _SENDER_KEYS, SENDER_PATHS)

    # -- the block-interleaved sender (include/ldpc_erasure_amd_interleave.h)
    def fec_encode_packets_interleaved_device(self, code, source, depth, fec_class=1, block0=0, out=None):
        """source: torch uint8 [F][k][S] (or [F][k] for S = 1) on this context's device -> packets [F*n][8+S]: the packets of
        fec_encode_packets_device in depth-`depth` order -- row j of frame f at index first[f] + j * stride[f] of
        fec_tx_ilv_layout(F, n, block0, depth).  fec_sender_ilv_info() says which path ran.  Asynchronous on the context's stream."""
        n, k, _ = self.code_info(code)
        F, S, out = _sender_shape(source, n, k, out)
        self._check(self._L.ldpc_amd_fec_encode_packets_ilv_dev(self._h, code, S, F, _ptr(source), fec_class, block0, depth, _ptr(out)),
                    "fec_encode_packets_ilv_dev")
        return out

    def fec_sender_ilv_info(self):
        """{"path": "none" | "fused" | "composed" of the last fec_encode_packets_interleaved_device call, "scratch_bytes": codeword
        scratch the context holds for the composed paths, "descriptor_bytes": descriptor memory it holds, "frames": frames of that
        call}."""
        return self._info("fec_sender_ilv_info", C.c_int64, _SENDER_KEYS, SENDER_PATHS)

    def fec_tx_interleaved(self, code, S, depth, fec_class=1, block0=0):
        """A sender that numbers its blocks across calls and emits them block-interleaved (FecTxInterleaved)."""
        return FecTxInterleaved(self, code, S, depth, fec_class, block0)

    # -- Reed-Solomon on the wire (include/ldpc_erasure_amd_rs_wire.h)
    def fec_rs_encode_packets_device(self, rs, source, depth=1, fec_class=FEC_CLASS_RS, block0=0, out=None):
        """source: torch uint8 [B][k][S] (or [B][k] for S = 1) on this context's device, B blocks of the RS code `rs` -> packets
        [B*n][8+S]: the packets of rs_encode + fec_packetize_device in depth-`depth` order -- row j of block b at index
        first[b] + j * stride[b] of fec_tx_ilv_layout(B, n, block0, depth).  fec_rs_sender_info() says which path ran.
        Asynchronous on the context's stream."""
        n, k = self.rs_info(rs)
        B, S, out = _sender_shape(source, n, k, out)
        self._check(self._L.ldpc_amd_fec_rs_encode_packets_dev(self._h, rs, S, B, _ptr(source), fec_class, block0, depth, _ptr(out)),
                    "fec_rs_encode_packets_dev")
        return out

    def fec_rs_sender_info(self):
        """{"path": "none" | "fused" | "composed" of the last fec_rs_encode_packets_device call, "scratch_bytes": codeword scratch
        the context holds for the composed paths, "descriptor_bytes": descriptor memory it holds, "blocks": blocks of that call}."""
        return self._info("fec_rs_sender_info", C.c_int64, ("path", "scratch_bytes", "descriptor_bytes", "blocks"), SENDER_PATHS)

    def fec_rs_receiver_info(self):
        """{"blocks": blocks RS-decoded by the last FecRxWindow.rs_decode_many / rs_decode_flush of this context, "launches": its RS
        decode launches, "scratch_bytes": the scratch it used (received symbols, or source words and per-block tables), "path": "none" |
        "fused" | "composed"}."""
        return self._info("fec_rs_receiver_info", C.c_int64, ("blocks", "launches", "scratch_bytes", "path"), RECEIVER_PATHS)

    def fec_tx_rs(self, rs, S, depth=1, block0=0):
        """A sender of RS blocks that numbers them across calls and emits them block-interleaved (FecTxRs)."""
        return FecTxRs(self, rs, S, depth, block0)

    # -- datagrams of any length (include/ldpc_erasure_amd_datagrams.h)
    def fec_pack_datagrams(self, data, offsets, k, S, out=None):
        """data: torch uint8 1-D on this context's device (a slice starting at any byte is fine), datagram i = data[offsets[i] :
        offsets[i+1]] (offsets: array-like int64, N + 1 entries, lengths 0 .. S-4; length 0 = a filler) -> source torch uint8
        [F][k][S], F = ceil(N / k): row i = the length as a little-endian uint32, the datagram, zeros.  Every byte of the result is
        written.  Asynchronous on the context's stream."""
        import torch
        off = _dgram_offsets(offsets)
        N = off.shape[0] - 1
        F = -(-N // max(k, 1))
        if out is None:
            dev = data.device if _is_torch(data) else torch.device("cuda", self.device)
            out = torch.empty((F, max(k, 0), max(S, 0)), dtype=torch.uint8, device=dev)
        assert _is_torch(out) and out.dtype == torch.uint8 and tuple(out.shape) == (F, k, S) and out.is_contiguous()
        got = self._check(self._L.ldpc_amd_fec_dgram_pack_dev(self._h, _ptr(data), off.ctypes.data, N, k, S, _ptr(out) if F else None),
                          "fec_dgram_pack_dev")
        assert got == F
        return out

    def fec_unpack_datagrams(self, frames, k, erased=None):
        """frames: torch uint8 [B][n][S] on this context's device, erased: torch uint8 [B][n] or None (nothing erased) -- out and
        erased_out of decode_frames / decode_many / decode_flush_many.  Returns Datagrams(bytes torch uint8 [B*k*(S-4)], offset torch
        int64 [B*k+1], state torch uint8 [B*k]): row r of the source rows is DGRAM_DELIVERED (its datagram is bytes[offset[r] :
        offset[r+1]]), DGRAM_FILLER, DGRAM_LOST (erased) or DGRAM_MALFORMED; offset[-1] is the total, the bytes behind it are not
        written.  Asynchronous on the context's stream, nothing is read back."""
        import torch
        assert _is_torch(frames) and frames.dtype == torch.uint8 and frames.ndim == 3 and frames.is_contiguous()
        B, n, S = frames.shape
        if erased is not None:
            assert _is_torch(erased) and erased.dtype == torch.uint8 and tuple(erased.shape) == (B, n)
        R = B * k
        out = Datagrams(torch.empty(max(R * (S - DGRAM_PREFIX_BYTES), 0), dtype=torch.uint8, device=frames.device),
                        torch.empty(R + 1, dtype=torch.int64, device=frames.device), torch.empty(R, dtype=torch.uint8, device=frames.device))
        self._check(self._L.ldpc_amd_fec_dgram_unpack_dev(self._h, _ptr(frames) if B else None, _ptr(erased) if B else None, B, n, k, S,
                                                          _ptr(out.bytes), out.bytes.shape[0], _ptr(out.offset), _ptr(out.state)),
                    "fec_dgram_unpack_dev")
        if B == 0:
            out.offset.zero_()   # (the library touches nothing for no frames)
        return out

    def fec_dgram_info(self):
        """{"scratch_bytes": device scratch the context holds for pack and unpack, "staging_bytes": pinned staging of pack's offsets,
        "pack_rows": rows of the last pack, "unpack_rows": rows of the last unpack}."""
        return self._info("fec_dgram_info", C.c_int64, ("scratch_bytes", "staging_bytes", "pack_rows", "unpack_rows"))

    # -- the trimmed wire (include/ldpc_erasure_amd_wire_ragged.h)
    def fec_trim_packets(self, packets, k, out=None):
        """packets: torch uint8 [P][8+S] on this context's device (what any sender of the library made of packed datagrams) ->
        Wire(bytes torch uint8 [P*(8+S)], offset torch int64 [P+1]): the bytes of every packet that have to be sent, back to back in
        packet order -- a source row (header symbol below k) with length prefix L <= S - 4 is cut to 8 + 4 + L bytes, every other
        packet is whole.  offset[-1] is the total, the bytes behind it are not written.  `out`, if given, is a Wire of such tensors
        to write into.  Asynchronous on the context's stream, nothing is read back."""
        import torch
        assert _is_torch(packets) and packets.dtype == torch.uint8 and packets.ndim == 2 and packets.is_contiguous()
        P, plen = packets.shape
        if out is None:
            out = Wire(torch.empty(P * plen, dtype=torch.uint8, device=packets.device), torch.empty(P + 1, dtype=torch.int64, device=packets.device))
        out = Wire(*out)
        assert out.bytes.dtype == torch.uint8 and out.bytes.ndim == 1 and out.offset.dtype == torch.int64 and tuple(out.offset.shape) == (P + 1,)
        self._check(self._L.ldpc_amd_fec_wire_trim_dev(self._h, _ptr(packets) if P else None, P, k, plen - 8, _ptr(out.bytes), out.bytes.shape[0],
                                                       _ptr(out.offset)), "fec_wire_trim_dev")
        if P == 0:
            out.offset.zero_()   # (the library touches nothing for no packets)
        return out

    def fec_land_packets(self, data, offset, S, out=None):
        """data: torch uint8 1-D on this context's device (a slice starting at any byte is fine; nbytes = data.numel()), offset: torch
        int64 [P+1] ON THE DEVICE, datagram p = data[offset[p] : offset[p+1]] -> (packets torch uint8 [P][8+S], state torch uint8 [P]):
        slot p is the datagram and zeros (WIRE_LANDED), or -- boundaries outside data, decreasing, a length below 8 or above 8 + S --
        eight bytes 0xFF and zeros, which every receiver drops (WIRE_REJECTED).  Every byte of packets is written.  Asynchronous on
        the context's stream, nothing is read back."""
        import torch
        assert _is_torch(data) and data.dtype == torch.uint8 and data.ndim == 1
        assert _is_torch(offset) and offset.dtype == torch.int64 and offset.ndim == 1 and offset.shape[0] >= 1 and offset.device == data.device
        P, nbytes = offset.shape[0] - 1, data.numel()
        if out is None:
            out = torch.empty((P, 8 + max(S, 0)), dtype=torch.uint8, device=data.device)
        assert _is_torch(out) and out.dtype == torch.uint8 and tuple(out.shape) == (P, 8 + S) and out.is_contiguous()
        state = torch.empty(P, dtype=torch.uint8, device=data.device)
        self._check(self._L.ldpc_amd_fec_wire_land_dev(self._h, _ptr(data) if nbytes else None, nbytes, _ptr(offset), P, S, _ptr(out) if P else None,
                                                       _ptr(state) if P else None), "fec_wire_land_dev")
        return out, state

    def fec_wire_ragged_info(self):
        """{"scratch_bytes": device scratch the context holds for trim, "trim_packets": packets of the last trim, "land_packets":
        packets of the last land}."""
        return self._info("fec_wire_ragged_info", C.c_int64, ("scratch_bytes", "trim_packets", "land_packets"))

    # -- the link emulator (include/ldpc_erasure_amd_link.h)
    def fec_link(self, seed, window=0, dup=0.0, bad_sym=0.0, foreign=0.0, dup_flip=False, first=0):
        """A link between a sender and a receiver of this context's device that re-orders (delays of 0 .. window packet times),
        duplicates and damages what it carries, and continues one stream of draws from call to call (FecLink)."""
        return FecLink(self, seed, window, dup, bad_sym, foreign, dup_flip, first)

    def fec_link_info(self):
        """{"scratch_bytes": device scratch held for the context's link calls, "plan_packets" / "apply_packets" /
        "apply_ragged_packets": packets of the last call of each kind}."""
        return self._info("fec_link_info", C.c_int64, ("scratch_bytes", "plan_packets", "apply_packets", "apply_ragged_packets"))

    def fec_tx_flows(self, code, S, nflows, fec_class=1, block0=0, depth=1):
        """nflows senders that number their blocks across calls and share one wire (FecTxFlows); depth > 1: every flow's blocks
        interleaved to that depth (include/ldpc_erasure_amd_interleave_flows.h)."""
        return FecTxFlows(self, code, S, nflows, fec_class, block0, depth)

    def fec_tx_device(self, code, S, fec_class=1, block0=0):
        """A sender that numbers its blocks across calls (FecTxDevice)."""
        return FecTxDevice(self, code, S, fec_class, block0)

    # -- the fused receiver (include/ldpc_erasure_amd_receiver.h)
    def fec_receiver_info(self):
        """{"path": "none" | "fused" | "composed" of the last FecRxDevice.decode_many call, "scratch_bytes": received-symbol scratch
        the context holds for the composed path, "blocks": blocks that call decoded}."""
        return self._info("fec_receiver_info", C.c_int, ("path", "scratch_bytes", "blocks"), RECEIVER_PATHS)

    # -- the windowed receiver (include/ldpc_erasure_amd_rx_window.h)
    def fec_rx_window(self, n, k, S, window=4, ahead_limit=10, depth=1, rule=None):
        """A device receiver that keeps `window` blocks open and resynchronises after `ahead_limit` packets beyond them (FecRxWindow);
        depth > 1: for a wire interleaved to that depth (include/ldpc_erasure_amd_interleave.h; needs 2 * depth <= window); rule: its
        close rule as a 4-tuple (include/ldpc_erasure_amd_rx_rule.h), None: the default rule."""
        return FecRxWindow(self, n, k, S, window, ahead_limit, depth, rule)

    def fec_rx_window_info(self):
        """{"path": "none" | "fused" | "composed" of the last FecRxWindow.decode_many / decode_flush call, "blocks": the blocks it
        decoded, "launches": its decoder launches, "scratch_bytes": received-symbol scratch it used}."""
        return self._info("fec_rxw_info", C.c_int64, _RXW_KEYS, RX_WINDOW_PATHS)

    # -- ... for many flows (include/ldpc_erasure_amd_rx_window_flows.h)
    def fec_rx_window_flows(self, nflows, n, k, S, window=4, ahead_limit=10, depth=1, rule=None):
        """nflows windowed receivers that are fed, planned, decoded and flushed together (FecRxWindowFlows); depth > 1: every flow's
        wire is interleaved to that depth (include/ldpc_erasure_amd_interleave_flows.h; needs 2 * depth <= window); rule: the close
        rule of every flow as a 4-tuple (include/ldpc_erasure_amd_rx_rule.h), None: the default rule."""
        return FecRxWindowFlows(self, nflows, n, k, S, window, ahead_limit, depth, rule)

    def fec_rx_window_flows_info(self):
        """fec_rx_window_info() for the last FecRxWindowFlows.decode_many / decode_flush_many call."""
        return self._info("fec_rxw_flows_info", C.c_int64, _RXW_KEYS, RX_WINDOW_PATHS)

    # -- the multi-flow receiver (include/ldpc_erasure_amd_flows.h)
    def fec_rx_flows(self, nflows, n, k, S):
        """nflows device receivers that are fed, planned and decoded together, one call for all of them (FecRxFlows)."""
        return FecRxFlows(self, nflows, n, k, S)

    # -- ... its batch flush (include/ldpc_erasure_amd_flows_flush.h)
    def fec_flows_flush_info(self):
        """{"path": "none" | "fused" | "composed" | "push" of the last FecRxFlows.flush_many / decode_flush_many call that closed a
        block, "blocks": the blocks it closed, "scratch_bytes": scratch it used, "launches": its decoder launches}."""
        return self._info("fec_flows_flush_info", C.c_int64, ("path", "blocks", "scratch_bytes", "launches"), FLUSH_PATHS)

    # -- ... fed with interleaved packets (include/ldpc_erasure_amd_flows_mixed.h)
    def fec_flows_demux(self, flow_of, nflows):
        """The stable partition of packet indices by flow, on its own: flow_of torch int32 [P] on this context's device (any value
        outside 0 .. nflows-1: a packet of no flow) -> (order torch int64 [R] on the device: the routed packets' indices flow by flow,
        each flow in arrival order; counts int64 [nflows]).  Synchronous."""
        import torch
        assert _is_torch(flow_of) and flow_of.dtype == torch.int32 and flow_of.ndim == 1
        P = flow_of.shape[0]
        order = torch.empty(max(P, 1), dtype=torch.int32, device=flow_of.device)   # (the library's uint32; an index is below 2^31)
        counts = np.zeros(nflows, dtype=np.int64)
        R = self._check(self._L.ldpc_amd_fec_flows_demux_dev(self._h, _ptr(flow_of) if P else None, P, nflows, _ptr(order), counts.ctypes.data),
                        "fec_flows_demux_dev")
        return order[:R].to(torch.int64), counts

    def fec_flows_demux_info(self):
        """{"tile": tile length in packets of the last partition, "tiles": its tiles, "scratch_bytes": table bytes the context holds}."""
        return self._info("fec_flows_demux_info", C.c_int64, ("tile", "tiles", "scratch_bytes"))


# ---------------------------------------------------------------------------------------------------------
# Host-side wire format (include/ldpc_erasure_amd_wire.h): FEC header, packetiser, two-buffer reassembler.
# ---------------------------------------------------------------------------------------------------------
def fec_header_pack(fec_class, block, symbol):
    return int(load_library().ldpc_amd_fec_header_pack(fec_class, block, symbol))


def fec_header_unpack(word):
    a, b, c = C.c_uint(0), C.c_uint(0), C.c_uint(0)
    load_library().ldpc_amd_fec_header_unpack(C.c_uint64(word), C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def fec_packetize(frames, fec_class=1, block0=0):
    """frames: uint8 [F][n][S] -> packets uint8 [F*n][8+S] in transmission order."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    F, n, S = frames.shape
    packets = np.zeros((F * n, 8 + S), dtype=np.uint8)
    if load_library().ldpc_amd_fec_packetize(frames.ctypes.data, F, n, S, fec_class, block0, packets.ctypes.data) != 0:
        raise LdpcAmdError("fec_packetize: bad arguments")
    return packets


class FecRx:
    """Two-buffer reassembler (OpenCL/device/ldpc_erasure_decoder_with_reordering_logic.cl:44-141,214-243).
    push(packet) / flush() return None or (block number, sym [n][S], erased [n])."""

    def __init__(self, n, k, S):
        self._L = load_library()
        h = C.c_void_p()
        if self._L.ldpc_amd_fec_rx_create(n, k, S, C.byref(h)) != 0:
            raise LdpcAmdError("fec_rx_create: bad arguments")
        self._h, self.n, self.k, self.S = h, n, k, S
        self._sym = np.zeros((n, S), dtype=np.uint8)
        self._er = np.zeros(n, dtype=np.uint8)

    def _ret(self, rc, blk):
        if rc < 0:
            raise LdpcAmdError("fec_rx: bad arguments")
        return (blk.value, self._sym.copy(), self._er.copy()) if rc == 1 else None

    def push(self, packet):
        packet = np.ascontiguousarray(packet, dtype=np.uint8)
        assert packet.size == 8 + self.S
        blk = C.c_int(-1)
        return self._ret(self._L.ldpc_amd_fec_rx_push(self._h, packet.ctypes.data, self._sym.ctypes.data, self._er.ctypes.data, C.byref(blk)), blk)

    def push_many(self, packets, max_blocks):
        """packets: uint8 [P][8+S].  Returns (blocks int32 [B], sym uint8 [B][n][S], erased uint8 [B][n], consumed)."""
        packets = np.ascontiguousarray(packets, dtype=np.uint8)
        assert packets.ndim == 2 and packets.shape[1] == 8 + self.S
        sym = np.zeros((max_blocks, self.n, self.S), dtype=np.uint8)
        er = np.zeros((max_blocks, self.n), dtype=np.uint8)
        blocks = np.zeros(max_blocks, dtype=np.int32)
        used = C.c_long(0)
        nb = self._L.ldpc_amd_fec_rx_push_many(self._h, packets.ctypes.data, packets.shape[0], sym.ctypes.data, er.ctypes.data,
                                               blocks.ctypes.data, max_blocks, C.byref(used))
        if nb < 0:
            raise LdpcAmdError("fec_rx_push_many: bad arguments")
        return blocks[:nb], sym[:nb], er[:nb], used.value

    def flush(self):
        blk = C.c_int(-1)
        return self._ret(self._L.ldpc_amd_fec_rx_flush(self._h, self._sym.ctypes.data, self._er.ctypes.data, C.byref(blk)), blk)

    @property
    def dropped(self):
        return int(self._L.ldpc_amd_fec_rx_dropped(self._h))

    def close(self):
        if self._h:
            self._L.ldpc_amd_fec_rx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Closes:
    """close() through the C destroy call of the object (prefix of its C names in self._pre), once; a context manager; closed when
    collected."""

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._pre + "destroy")(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _OnDevice:
    """What the receivers of packets in GPU memory allocate alike: the device of their context, the result arrays of B frames."""

    def _device(self):
        import torch
        return torch.device("cuda", self._ctx.device)

    def _frames(self, B):
        import torch
        dev = self._device()
        shape = (B, self.n) if self.S == 1 else (B, self.n, self.S)
        i32 = [torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(4)]
        return DecodedFrames(torch.empty(shape, dtype=torch.uint8, device=dev), i32[0], i32[1], i32[2],
                             torch.empty((B, self.n), dtype=torch.uint8, device=dev), i32[3])


class FecRxDevice(_OnDevice, _Closes):
    """FecRx for packets already in GPU memory (include/ldpc_erasure_amd_wire_dev.h): the same blocks, erasure flags,
    consumed and dropped counts, byte for byte.  Payload movement is asynchronous on the context's stream; the returned
    block numbers and counts are final when a call returns.  Close it before its Context."""
    _pre = "ldpc_amd_fec_rx_dev_"

    def __init__(self, ctx, n, k, S):
        self._ctx, self._L = ctx, ctx._L
        h = C.c_void_p()
        ctx._check(self._L.ldpc_amd_fec_rx_dev_create(ctx._h, n, k, S, C.byref(h)), "fec_rx_dev_create")
        self._h, self.n, self.k, self.S = h, n, k, S

    def push_many(self, packets, max_blocks):
        """packets: torch uint8 [P][8+S] on the device.  Returns (blocks int32 [B], sym torch uint8 [B][n][S],
        erased torch uint8 [B][n], consumed)."""
        import torch
        assert _is_torch(packets) and packets.dtype == torch.uint8 and packets.ndim == 2 and packets.shape[1] == 8 + self.S
        sym = torch.empty((max(max_blocks, 1), self.n, self.S), dtype=torch.uint8, device=packets.device)
        er = torch.empty((max(max_blocks, 1), self.n), dtype=torch.uint8, device=packets.device)
        blocks = np.zeros(max(max_blocks, 1), dtype=np.int32)
        used = C.c_int64(0)
        nb = self._ctx._check(self._L.ldpc_amd_fec_rx_dev_push_many(self._h, _ptr(packets) if packets.numel() else None, packets.shape[0],
                                                                    _ptr(sym), _ptr(er), blocks.ctypes.data, max_blocks, C.byref(used)),
                              "fec_rx_dev_push_many")
        return blocks[:nb], sym[:nb], er[:nb], used.value

    def flush(self):
        """None, or (block number, sym torch [n][S], erased torch [n]) of the block the end of the stream closes."""
        import torch
        sym = torch.empty((self.n, self.S), dtype=torch.uint8, device=self._device())
        er = torch.empty(self.n, dtype=torch.uint8, device=self._device())
        blk = C.c_int(-1)
        rc = self._ctx._check(self._L.ldpc_amd_fec_rx_dev_flush(self._h, _ptr(sym), _ptr(er), C.byref(blk)), "fec_rx_dev_flush")
        return (blk.value, sym, er) if rc == 1 else None

    def decode_many(self, code, packets, max_blocks, max_sweeps=10, do_ml=1, out=None):
        """push_many + Context.decode_frames in one call (include/ldpc_erasure_amd_receiver.h): packets torch uint8 [P][8+S] on the
        device -> (blocks int32 [B], DecodedFrames of the B closed blocks, consumed).  Where the decoder can fetch its rows from the
        packets itself no array of received symbols is written (Context.fec_receiver_info() says which path ran).  Keep `packets`
        alive until the context's stream has passed the call.  `out`, if given, is a DecodedFrames of device tensors with room for
        max_blocks frames to write into (the result is its first B frames)."""
        import torch
        assert _is_torch(packets) and packets.dtype == torch.uint8 and packets.ndim == 2 and packets.shape[1] == 8 + self.S
        if out is not None:
            fr = DecodedFrames(*out)
            assert all(t.shape[0] >= max(max_blocks, 1) for t in fr) and tuple(fr.erased_out.shape[1:]) == (self.n,)
            assert tuple(fr.out.shape[1:]) == ((self.n,) if self.S == 1 else (self.n, self.S))
        else:
            fr = self._frames(max(max_blocks, 1))
        blocks = np.zeros(max(max_blocks, 1), dtype=np.int32)
        used = C.c_int64(0)
        nb = self._ctx._check(self._L.ldpc_amd_fec_rx_dev_decode_many(
            self._h, code, _ptr(packets) if packets.numel() else None, packets.shape[0], max_sweeps, do_ml, _ptr(fr.out), _ptr(fr.sweeps),
            _ptr(fr.residual), _ptr(fr.status), _ptr(fr.erased_out), _ptr(fr.residual_src), blocks.ctypes.data, max_blocks, C.byref(used)),
            "fec_rx_dev_decode_many")
        return blocks[:nb], DecodedFrames(*(t[:nb] for t in fr)), used.value

    def decode_flush(self, code, max_sweeps=10, do_ml=1):
        """None, or (block number, DecodedFrames of that one block) for the block the end of the stream closes."""
        fr = self._frames(1)
        blk = C.c_int(-1)
        rc = self._ctx._check(self._L.ldpc_amd_fec_rx_dev_decode_flush(
            self._h, code, max_sweeps, do_ml, _ptr(fr.out), _ptr(fr.sweeps), _ptr(fr.residual), _ptr(fr.status), _ptr(fr.erased_out),
            _ptr(fr.residual_src), C.byref(blk)), "fec_rx_dev_decode_flush")
        return (blk.value, fr) if rc == 1 else None

    @property
    def dropped(self):
        return int(self._L.ldpc_amd_fec_rx_dev_dropped(self._h))


class _RxWindowState(_Closes):
    """What the host and the device object of the windowed receiver report alike (prefix of the C names in self._pre)."""

    def _fn(self, name):
        return getattr(self._L, self._pre + name)

    def stats(self):
        """{"bad_symbol", "late", "ahead_total", "resyncs", "closed"}: the totals since the object was created."""
        t = (C.c_int64 * 5)()
        if self._fn("stats")(self._h, t) != 0:
            raise LdpcAmdError("fec_rxw_stats: bad arguments")
        return dict(zip(RX_WINDOW_TOTALS, (int(v) for v in t)))

    @property
    def dropped(self):
        return int(self._fn("dropped")(self._h))

    def state(self):
        """{"base": block number of slot 0 (-1 before the first packet), "cnt": packets stored per slot, "ahead"}."""
        base, ahead = C.c_int(0), C.c_int64(0)
        cnt = np.zeros(self.window, dtype=np.int32)
        if self._fn("state")(self._h, C.byref(base), cnt.ctypes.data, C.byref(ahead)) != 0:
            raise LdpcAmdError("fec_rxw_state: bad arguments")
        return {"base": base.value, "cnt": cnt.tolist(), "ahead": ahead.value}

    @property
    def depth(self):
        """The interleaving depth the object was created for (include/ldpc_erasure_amd_interleave.h), 1: the plain rule."""
        return int(self._fn("depth")(self._h))

    @property
    def rule(self):
        """The close rule the object follows, (c_hi, later_hi, c_lo, later_lo) (include/ldpc_erasure_amd_rx_rule.h)."""
        r = RxRule()
        if self._fn("get_rule")(self._h, C.byref(r)) != 0:
            raise LdpcAmdError("fec_rxw_get_rule: bad arguments")
        return (r.c_hi, r.later_hi, r.c_lo, r.later_lo)


class FecRxWindowHost(_RxWindowState):
    """The windowed reassembler on the host (include/ldpc_erasure_amd_rx_window.h): `window` blocks open, a resynchronisation after
    `ahead_limit` packets beyond them (0: never).  With window = 2 and ahead_limit = 0 it is FecRx.  depth > 1: the rule for a wire
    interleaved to that depth (include/ldpc_erasure_amd_interleave.h; needs 2 * depth <= window).  rule: the close rule as a 4-tuple
    (include/ldpc_erasure_amd_rx_rule.h; fec_rx_rule_mds(n, k, depth) for Reed-Solomon blocks), None: the default rule."""
    _pre = "ldpc_amd_fec_rxw_"

    def __init__(self, n, k, S, window=4, ahead_limit=10, depth=1, rule=None):
        self._L = load_library()
        h = C.c_void_p()
        if rule is not None:
            rc = self._L.ldpc_amd_fec_rxw_create_rule(n, k, S, window, ahead_limit, depth, C.byref(_rx_rule(rule)), C.byref(h))
        elif depth == 1:   # (the older builds tools/ab_lib.py loads have this call only)
            rc = self._L.ldpc_amd_fec_rxw_create(n, k, S, window, ahead_limit, C.byref(h))
        else:
            rc = self._L.ldpc_amd_fec_rxw_create_depth(n, k, S, window, ahead_limit, depth, C.byref(h))
        if rc != 0:
            raise LdpcAmdError("fec_rxw_create: bad arguments")
        self._h, self.n, self.k, self.S, self.window, self.ahead_limit = h, n, k, S, window, ahead_limit

    def push(self, packet):
        """None, or (block number, sym [n][S], erased [n]) of the block this packet closed."""
        packet = np.ascontiguousarray(packet, dtype=np.uint8)
        assert packet.size == 8 + self.S
        sym, er, blk = np.zeros((self.n, self.S), dtype=np.uint8), np.zeros(self.n, dtype=np.uint8), C.c_int(-1)
        rc = self._L.ldpc_amd_fec_rxw_push(self._h, packet.ctypes.data, sym.ctypes.data, er.ctypes.data, C.byref(blk))
        if rc < 0:
            raise LdpcAmdError("fec_rxw_push: bad arguments")
        return (blk.value, sym, er) if rc == 1 else None

    def push_many(self, packets, max_blocks):
        """packets: uint8 [P][8+S].  Returns (blocks int32 [B], sym uint8 [B][n][S], erased uint8 [B][n], consumed)."""
        packets = np.ascontiguousarray(packets, dtype=np.uint8)
        assert packets.ndim == 2 and packets.shape[1] == 8 + self.S
        mb = max(max_blocks, 1)
        sym = np.zeros((mb, self.n, self.S), dtype=np.uint8)
        er = np.zeros((mb, self.n), dtype=np.uint8)
        blocks = np.zeros(mb, dtype=np.int32)
        used = C.c_long(0)
        nb = self._L.ldpc_amd_fec_rxw_push_many(self._h, packets.ctypes.data if packets.shape[0] else None, packets.shape[0], sym.ctypes.data,
                                                er.ctypes.data, blocks.ctypes.data, max_blocks, C.byref(used))
        if nb < 0:
            raise LdpcAmdError("fec_rxw_push_many: bad arguments")
        return blocks[:nb], sym[:nb], er[:nb], used.value

    def flush(self):
        """(blocks int32 [B], sym [B][n][S], erased [B][n]) of the 0..window blocks the end of the stream closes."""
        sym = np.zeros((self.window, self.n, self.S), dtype=np.uint8)
        er = np.zeros((self.window, self.n), dtype=np.uint8)
        blocks = np.zeros(self.window, dtype=np.int32)
        nb = self._L.ldpc_amd_fec_rxw_flush(self._h, sym.ctypes.data, er.ctypes.data, blocks.ctypes.data)
        if nb < 0:
            raise LdpcAmdError("fec_rxw_flush: bad arguments")
        return blocks[:nb], sym[:nb], er[:nb]


class FecRxWindow(_RxWindowState, _OnDevice):
    """FecRxWindowHost for packets already in GPU memory: the same blocks, erasure flags, consumed, totals and state, byte for byte.
    Shaped on FecRxDevice: payload movement is asynchronous on the context's stream; the returned block numbers and counts are final
    when a call returns.  rule: the close rule as a 4-tuple (include/ldpc_erasure_amd_rx_rule.h), None: the default rule.  Close it
    before its Context."""
    _pre = "ldpc_amd_fec_rxw_dev_"

    def __init__(self, ctx, n, k, S, window=4, ahead_limit=10, depth=1, rule=None):
        self._ctx, self._L = ctx, ctx._L
        h = C.c_void_p()
        if rule is not None:
            ctx._check(self._L.ldpc_amd_fec_rxw_dev_create_rule(ctx._h, n, k, S, window, ahead_limit, depth, C.byref(_rx_rule(rule)), C.byref(h)),
                       "fec_rxw_dev_create")
        elif depth == 1:   # (the older builds tools/ab_lib.py loads have this call only)
            ctx._check(self._L.ldpc_amd_fec_rxw_dev_create(ctx._h, n, k, S, window, ahead_limit, C.byref(h)), "fec_rxw_dev_create")
        else:
            ctx._check(self._L.ldpc_amd_fec_rxw_dev_create_depth(ctx._h, n, k, S, window, ahead_limit, depth, C.byref(h)), "fec_rxw_dev_create")
        self._h, self.n, self.k, self.S, self.window, self.ahead_limit = h, n, k, S, window, ahead_limit

    def push_many(self, packets, max_blocks):
        """packets: torch uint8 [P][8+S] on the device.  Returns (blocks int32 [B], sym torch uint8 [B][n][S],
        erased torch uint8 [B][n], consumed)."""
        import torch
        assert _is_torch(packets) and packets.dtype == torch.uint8 and packets.ndim == 2 and packets.shape[1] == 8 + self.S
        mb = max(max_blocks, 1)
        sym = torch.empty((mb, self.n, self.S), dtype=torch.uint8, device=packets.device)
        er = torch.empty((mb, self.n), dtype=torch.uint8, device=packets.device)
        blocks = np.zeros(mb, dtype=np.int32)
        used = C.c_int64(0)
        nb = self._ctx._check(self._L.ldpc_amd_fec_rxw_dev_push_many(self._h, _ptr(packets) if packets.numel() else None, packets.shape[0],
                                                                     _ptr(sym), _ptr(er), blocks.ctypes.data, max_blocks, C.byref(used)),
                              "fec_rxw_dev_push_many")
        return blocks[:nb], sym[:nb], er[:nb], used.value

    def flush(self):
        """(blocks int32 [B], sym torch [B][n][S], erased torch [B][n]) of the 0..window blocks the end of the stream closes."""
        import torch
        sym = torch.empty((self.window, self.n, self.S), dtype=torch.uint8, device=self._device())
        er = torch.empty((self.window, self.n), dtype=torch.uint8, device=self._device())
        blocks = np.zeros(self.window, dtype=np.int32)
        nb = self._ctx._check(self._L.ldpc_amd_fec_rxw_dev_flush(self._h, _ptr(sym), _ptr(er), blocks.ctypes.data), "fec_rxw_dev_flush")
        return blocks[:nb], sym[:nb], er[:nb]

    def decode_many(self, code, packets, max_blocks, max_sweeps=10, do_ml=1):
        """push_many + Context.decode_frames in one call: packets torch uint8 [P][8+S] on the device -> (blocks int32 [B],
        DecodedFrames of the B closed blocks, consumed).  Context.fec_rx_window_info() says which form ran.  Keep `packets` alive
        until the context's stream has passed the call."""
        import torch
        assert _is_torch(packets) and packets.dtype == torch.uint8 and packets.ndim == 2 and packets.shape[1] == 8 + self.S
        fr = self._frames(max(max_blocks, 1))
        blocks = np.zeros(max(max_blocks, 1), dtype=np.int32)
        used = C.c_int64(0)
        nb = self._ctx._check(self._L.ldpc_amd_fec_rxw_dev_decode_many(
            self._h, code, _ptr(packets) if packets.numel() else None, packets.shape[0], max_sweeps, do_ml, _ptr(fr.out), _ptr(fr.sweeps),
            _ptr(fr.residual), _ptr(fr.status), _ptr(fr.erased_out), _ptr(fr.residual_src), blocks.ctypes.data, max_blocks, C.byref(used)),
            "fec_rxw_dev_decode_many")
        return blocks[:nb], DecodedFrames(*(t[:nb] for t in fr)), used.value

    def decode_flush(self, code, max_sweeps=10, do_ml=1):
        """(blocks int32 [B], DecodedFrames of those B blocks) for the 0..window blocks the end of the stream closes."""
        fr = self._frames(self.window)
        blocks = np.zeros(self.window, dtype=np.int32)
        nb = self._ctx._check(self._L.ldpc_amd_fec_rxw_dev_decode_flush(
            self._h, code, max_sweeps, do_ml, _ptr(fr.out), _ptr(fr.sweeps), _ptr(fr.residual), _ptr(fr.status), _ptr(fr.erased_out),
            _ptr(fr.residual_src), blocks.ctypes.data), "fec_rxw_dev_decode_flush")
        return blocks[:nb], DecodedFrames(*(t[:nb] for t in fr))

    def _rs_out(self, B, out):
        import torch
        dev = self._device()
        if out is None:
            out = (torch.empty((B, self.k, self.S), dtype=torch.uint8, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
                   torch.empty((B,), dtype=torch.int32, device=dev))
        msg, received, status = out
        assert tuple(msg.shape) == (B, self.k, self.S) and msg.dtype == torch.uint8 and msg.is_contiguous()
        assert all(tuple(t.shape) == (B,) and t.dtype == torch.int32 for t in (received, status))
        return msg, received, status

    def rs_decode_many(self, rs, packets, max_blocks, out=None):
        """push_many + Context.rs_decode_frames in one call (include/ldpc_erasure_amd_rs_wire.h): packets torch uint8 [P][8+S] on the
        device -> (blocks int32 [B], msg torch uint8 [B][k][S], received torch int32 [B], status torch int32 [B], consumed).  `out`,
        if given, is the (msg [max_blocks][k][S], received [max_blocks], status [max_blocks]) to write into.  Keep `packets` alive
        until the context's stream has passed the call."""
        import torch
        assert _is_torch(packets) and packets.dtype == torch.uint8 and packets.ndim == 2 and packets.shape[1] == 8 + self.S
        mb = max(max_blocks, 1)
        msg, received, status = self._rs_out(mb, out)
        blocks = np.zeros(mb, dtype=np.int32)
        used = C.c_int64(0)
        nb = self._ctx._check(self._L.ldpc_amd_fec_rxw_dev_rs_decode_many(
            self._h, rs, _ptr(packets) if packets.numel() else None, packets.shape[0], _ptr(msg), _ptr(received), _ptr(status), None,
            blocks.ctypes.data, max_blocks, C.byref(used)), "fec_rxw_dev_rs_decode_many")
        return blocks[:nb], msg[:nb], received[:nb], status[:nb], used.value

    def rs_decode_flush(self, rs):
        """(blocks int32 [B], msg [B][k][S], received [B], status [B]) for the 0..window blocks the end of the stream closes."""
        msg, received, status = self._rs_out(self.window, None)
        blocks = np.zeros(self.window, dtype=np.int32)
        nb = self._ctx._check(self._L.ldpc_amd_fec_rxw_dev_rs_decode_flush(self._h, rs, _ptr(msg), _ptr(received), _ptr(status), None,
                                                                           blocks.ctypes.data), "fec_rxw_dev_rs_decode_flush")
        return blocks[:nb], msg[:nb], received[:nb], status[:nb]


class _RxFlows(_OnDevice, _Closes):
    """What FecRxFlows and FecRxWindowFlows call alike (prefix of the C names in self._pre): the segmented and the mixed push and decode
    calls, `unrouted`, close.  The docstrings are FecRxFlows'; FecRxWindowFlows gives its own where its text differs."""

    def _fn(self, name):
        return getattr(self._L, self._pre + name)

    def _what(self, name):
        return self._pre[len("ldpc_amd_"):] + name

    def _segments(self, packets, flow_begin, max_blocks_per_flow):
        import torch
        assert _is_torch(packets) and packets.dtype == torch.uint8 and packets.ndim == 2 and packets.shape[1] == 8 + self.S
        fb = np.ascontiguousarray(flow_begin, dtype=np.int64)
        assert fb.shape == (self.nflows + 1,) and int(fb[-1]) == packets.shape[0]
        slots = max(self.nflows * max(max_blocks_per_flow, 1), 1)
        return (fb, slots, np.zeros(slots, dtype=np.int32), np.zeros(self.nflows, dtype=np.int32), np.zeros(self.nflows, dtype=np.int64),
                _ptr(packets) if packets.numel() else None)

    def push_many(self, packets, flow_begin, max_blocks_per_flow):
        """packets: torch uint8 [P][8+S] on the device, flow_begin: nflows + 1 packet indices.  Returns (closes int32 [nflows],
        blocks int32 [T], sym torch uint8 [T][n][S], erased torch uint8 [T][n], consumed int64 [nflows])."""
        import torch
        fb, slots, blocks, closes, consumed, pp = self._segments(packets, flow_begin, max_blocks_per_flow)
        sym = torch.empty((slots, self.n, self.S), dtype=torch.uint8, device=packets.device)
        er = torch.empty((slots, self.n), dtype=torch.uint8, device=packets.device)
        T = self._ctx._check(self._fn("push_many")(self._h, pp, fb.ctypes.data, _ptr(sym), _ptr(er), blocks.ctypes.data, closes.ctypes.data,
                                                   max_blocks_per_flow, consumed.ctypes.data), self._what("push_many"))
        return closes, blocks[:T], sym[:T], er[:T], consumed

    def decode_many(self, code, packets, flow_begin, max_blocks_per_flow, max_sweeps=10, do_ml=1):
        """push_many + Context.decode_frames of all flows in one call -> (closes int32 [nflows], blocks int32 [T], DecodedFrames of
        the T closed blocks, consumed int64 [nflows]).  Fused or composed as FecRxDevice.decode_many would be
        (Context.fec_receiver_info() says which path ran).  Keep `packets` alive until the context's stream has passed the call."""
        fb, slots, blocks, closes, consumed, pp = self._segments(packets, flow_begin, max_blocks_per_flow)
        fr = self._frames(slots)
        T = self._ctx._check(self._fn("decode_many")(
            self._h, code, pp, fb.ctypes.data, max_sweeps, do_ml, _ptr(fr.out), _ptr(fr.sweeps), _ptr(fr.residual), _ptr(fr.status),
            _ptr(fr.erased_out), _ptr(fr.residual_src), blocks.ctypes.data, closes.ctypes.data, max_blocks_per_flow, consumed.ctypes.data),
            self._what("decode_many"))
        return closes, blocks[:T], DecodedFrames(*(t[:T] for t in fr)), consumed

    def _mixed(self, packets, flow_of, max_blocks_per_flow, want_left):
        import torch
        assert _is_torch(packets) and packets.dtype == torch.uint8 and packets.ndim == 2 and packets.shape[1] == 8 + self.S
        assert _is_torch(flow_of) and flow_of.dtype == torch.int32 and flow_of.shape == (packets.shape[0],)
        P = packets.shape[0]
        slots = max(self.nflows * max(max_blocks_per_flow, 1), 1)
        left = torch.empty(max(P, 1), dtype=torch.uint8, device=packets.device) if want_left else None
        return (P, slots, np.zeros(slots, dtype=np.int32), np.zeros(self.nflows, dtype=np.int32), np.zeros(self.nflows, dtype=np.int64),
                np.zeros(self.nflows, dtype=np.int64), _ptr(packets) if P else None, _ptr(flow_of) if P else None, left)

    def push_mixed(self, packets, flow_of, max_blocks_per_flow, want_left=False):
        """push_many for packets in arrival order (include/ldpc_erasure_amd_flows_mixed.h): packets torch uint8 [P][8+S], flow_of torch
        int32 [P] on the device, flow_of[p] = the flow of packet p (outside 0 .. nflows-1: no flow, ignored and counted in
        `unrouted`).  Returns push_many's tuple for the per-flow segments, then offered int64 [nflows] (packets of each flow), then --
        want_left -- left torch uint8 [P]: 1 for the packets behind their flow's consumed prefix, to be submitted again."""
        import torch
        P, slots, blocks, closes, consumed, offered, pp, fp, left = self._mixed(packets, flow_of, max_blocks_per_flow, want_left)
        sym = torch.empty((slots, self.n, self.S), dtype=torch.uint8, device=packets.device)
        er = torch.empty((slots, self.n), dtype=torch.uint8, device=packets.device)
        T = self._ctx._check(self._fn("push_mixed")(
            self._h, pp, fp, P, _ptr(sym), _ptr(er), blocks.ctypes.data, closes.ctypes.data, max_blocks_per_flow, consumed.ctypes.data,
            offered.ctypes.data, _ptr(left) if want_left else None), self._what("push_mixed"))
        r = (closes, blocks[:T], sym[:T], er[:T], consumed, offered)
        return r + (left[:P],) if want_left else r

    def decode_mixed(self, code, packets, flow_of, max_blocks_per_flow, max_sweeps=10, do_ml=1, want_left=False):
        """decode_many for packets in arrival order with a flow number each (push_mixed): decode_many's tuple, then offered (and left
        when asked).  No payload byte is copied to sort the packets: only their indices are partitioned by flow."""
        P, slots, blocks, closes, consumed, offered, pp, fp, left = self._mixed(packets, flow_of, max_blocks_per_flow, want_left)
        fr = self._frames(slots)
        T = self._ctx._check(self._fn("decode_mixed")(
            self._h, code, pp, fp, P, max_sweeps, do_ml, _ptr(fr.out), _ptr(fr.sweeps), _ptr(fr.residual), _ptr(fr.status),
            _ptr(fr.erased_out), _ptr(fr.residual_src), blocks.ctypes.data, closes.ctypes.data, max_blocks_per_flow, consumed.ctypes.data,
            offered.ctypes.data, _ptr(left) if want_left else None), self._what("decode_mixed"))
        r = (closes, blocks[:T], DecodedFrames(*(t[:T] for t in fr)), consumed, offered)
        return r + (left[:P],) if want_left else r

    @property
    def unrouted(self):
        """packets of no flow the mixed calls were given so far"""
        return int(self._fn("unrouted")(self._h))


class FecRxFlows(_RxFlows):
    """nflows FecRxDevice in one object (include/ldpc_erasure_amd_flows.h): one packet array segmented by flow -- flow f owns the
    packets flow_begin[f] .. flow_begin[f+1]-1 -- is planned for all flows at once and read back once, and every block that closed, of
    every flow, is decoded in one launch.  Flow f behaves exactly like a FecRxDevice fed its segment with max_blocks =
    max_blocks_per_flow.  The closed blocks come out dense in flow order: flow 0's in closing order, then flow 1's, ...; flow f's
    start at closes[:f].sum().  push_mixed / decode_mixed take the packets in arrival order with a flow number each instead
    (include/ldpc_erasure_amd_flows_mixed.h) and return the same; all four calls mix freely.  Close it before its Context."""
    _pre = "ldpc_amd_fec_rx_flows_"

    def __init__(self, ctx, nflows, n, k, S):
        self._ctx, self._L = ctx, ctx._L
        h = C.c_void_p()
        ctx._check(self._L.ldpc_amd_fec_rx_flows_create(ctx._h, nflows, n, k, S, C.byref(h)), "fec_rx_flows_create")
        self._h, self.nflows, self.n, self.k, self.S = h, nflows, n, k, S

    def flush(self, flow):
        """None, or (block number, sym torch [n][S], erased torch [n]) of the block the end of flow `flow`'s stream closes."""
        import torch
        sym = torch.empty((self.n, self.S), dtype=torch.uint8, device=self._device())
        er = torch.empty(self.n, dtype=torch.uint8, device=self._device())
        blk = C.c_int(-1)
        rc = self._ctx._check(self._L.ldpc_amd_fec_rx_flows_flush(self._h, flow, _ptr(sym), _ptr(er), C.byref(blk)), "fec_rx_flows_flush")
        return (blk.value, sym, er) if rc == 1 else None

    def decode_flush(self, flow, code, max_sweeps=10, do_ml=1):
        """None, or (block number, DecodedFrames of that one block) for the block the end of flow `flow`'s stream closes."""
        fr = self._frames(1)
        blk = C.c_int(-1)
        rc = self._ctx._check(self._L.ldpc_amd_fec_rx_flows_decode_flush(
            self._h, flow, code, max_sweeps, do_ml, _ptr(fr.out), _ptr(fr.sweeps), _ptr(fr.residual), _ptr(fr.status), _ptr(fr.erased_out),
            _ptr(fr.residual_src), C.byref(blk)), "fec_rx_flows_decode_flush")
        return (blk.value, fr) if rc == 1 else None

    # -- the batch flush (include/ldpc_erasure_amd_flows_flush.h)
    def pending(self):
        """FlowsPending(cur_block int32 [nflows] (-1: the flow has not started), cur_cnt, next_cnt int32 [nflows]: packets the
        current / the next block of every flow took so far, blocks: how many blocks a full drain would close now).  Host only."""
        cur, cc, nc = (np.zeros(self.nflows, dtype=np.int32) for _ in range(3))
        total = self._L.ldpc_amd_fec_rx_flows_pending(self._h, cur.ctypes.data, cc.ctypes.data, nc.ctypes.data)
        if total < 0:
            raise LdpcAmdError("fec_rx_flows_pending: the object is closed")
        return FlowsPending(cur, cc, nc, total)

    def _flush_list(self, flows, rounds):
        """(flows int32 [nsel] or None, nsel, slots to allocate: the blocks the call can close at most, from pending())"""
        sel = None if flows is None else np.ascontiguousarray(flows, dtype=np.int32).reshape(-1)
        p = self.pending()
        open_blocks = np.where(p.cur_block < 0, 0, (p.cur_cnt + p.next_cnt > 0).astype(np.int64) + (p.next_cnt > 0))
        pick = open_blocks if sel is None else open_blocks[sel[(sel >= 0) & (sel < self.nflows)]]
        nsel = self.nflows if sel is None else int(sel.shape[0])
        return sel, nsel, max(int(np.minimum(pick, max(rounds, 0)).sum()), 1)

    def flush_many(self, flows=None, rounds=2):
        """flush() of every flow of the list `flows` (None: all flows), up to `rounds` (1 or 2) times each, in one call -> (closes
        int32 [nsel], blocks int32 [T], sym torch uint8 [T][n][S], erased torch uint8 [T][n]).  The blocks come out dense in list
        order, entry j's from closes[:j].sum() on; flows that are not listed are not touched."""
        import torch
        sel, nsel, slots = self._flush_list(flows, rounds)
        sym = torch.empty((slots, self.n, self.S), dtype=torch.uint8, device=self._device())
        er = torch.empty((slots, self.n), dtype=torch.uint8, device=self._device())
        blocks, closes = np.zeros(max(nsel * 2, 1), dtype=np.int32), np.zeros(max(nsel, 1), dtype=np.int32)
        T = self._ctx._check(self._L.ldpc_amd_fec_rx_flows_flush_many(self._h, None if sel is None else sel.ctypes.data, nsel, rounds, _ptr(sym),
                                                                      _ptr(er), blocks.ctypes.data, closes.ctypes.data), "fec_rx_flows_flush_many")
        return closes[:nsel], blocks[:T], sym[:T], er[:T]

    def decode_flush_many(self, code, flows=None, rounds=2, max_sweeps=10, do_ml=1):
        """flush_many + Context.decode_frames in one call: every block closed is decoded by ONE decoder launch, straight from the
        staging planes where the decoder can fetch its rows itself (Context.fec_flows_flush_info() says which path ran) -> (closes
        int32 [nsel], blocks int32 [T], DecodedFrames of the T blocks).  Equal to the loop of decode_flush calls, flow by flow."""
        sel, nsel, slots = self._flush_list(flows, rounds)
        fr = self._frames(slots)
        blocks, closes = np.zeros(max(nsel * 2, 1), dtype=np.int32), np.zeros(max(nsel, 1), dtype=np.int32)
        T = self._ctx._check(self._L.ldpc_amd_fec_rx_flows_decode_flush_many(
            self._h, code, None if sel is None else sel.ctypes.data, nsel, rounds, max_sweeps, do_ml, _ptr(fr.out), _ptr(fr.sweeps),
            _ptr(fr.residual), _ptr(fr.status), _ptr(fr.erased_out), _ptr(fr.residual_src), blocks.ctypes.data, closes.ctypes.data),
            "fec_rx_flows_decode_flush_many")
        return closes[:nsel], blocks[:T], DecodedFrames(*(t[:T] for t in fr))

    @property
    def dropped(self):
        """int64 [nflows]: packets of each flow that went to no block so far"""
        return np.array([self._L.ldpc_amd_fec_rx_flows_dropped(self._h, f) for f in range(self.nflows)], dtype=np.int64)


class FecRxWindowFlows(_RxFlows):
    """nflows FecRxWindow in one object (include/ldpc_erasure_amd_rx_window_flows.h), shaped on FecRxFlows: one packet array segmented
    by flow -- flow f owns the packets flow_begin[f] .. flow_begin[f+1]-1 -- is planned for all flows at once (one wavefront per flow)
    and read back once, and every block that closed, of every flow, is decoded in one launch.  Flow f behaves exactly like a
    FecRxWindowHost fed its segment with max_blocks = max_blocks_per_flow.  The closed blocks come out dense in flow order: flow f's
    start at closes[:f].sum().  push_mixed / decode_mixed take the packets in arrival order with a flow number each instead
    (include/ldpc_erasure_amd_rx_window_flows_mixed.h) and return the same; all calls mix freely.  depth > 1: every flow follows the
    rule for a wire interleaved to that depth, FecRxWindowHost(..., depth=depth) per flow (include/ldpc_erasure_amd_interleave_flows.h;
    needs 2 * depth <= window).  rule: the close rule of every flow as a 4-tuple (include/ldpc_erasure_amd_rx_rule.h), None: the
    default rule.  Close it before its Context."""
    _pre = "ldpc_amd_fec_rxw_flows_"

    def __init__(self, ctx, nflows, n, k, S, window=4, ahead_limit=10, depth=1, rule=None):
        self._ctx, self._L = ctx, ctx._L
        h = C.c_void_p()
        if rule is not None:
            ctx._check(self._L.ldpc_amd_fec_rxw_flows_create_rule(ctx._h, nflows, n, k, S, window, ahead_limit, depth, C.byref(_rx_rule(rule)),
                                                                  C.byref(h)), "fec_rxw_flows_create")
        elif depth == 1:   # (the older builds tools/ab_lib.py loads have this call only)
            ctx._check(self._L.ldpc_amd_fec_rxw_flows_create(ctx._h, nflows, n, k, S, window, ahead_limit, C.byref(h)), "fec_rxw_flows_create")
        else:
            ctx._check(self._L.ldpc_amd_fec_rxw_flows_create_depth(ctx._h, nflows, n, k, S, window, ahead_limit, depth, C.byref(h)),
                       "fec_rxw_flows_create")
        self._h, self.nflows, self.n, self.k, self.S, self.window, self.ahead_limit = h, nflows, n, k, S, window, ahead_limit

    @property
    def depth(self):
        """The interleaving depth the object was created for (include/ldpc_erasure_amd_interleave_flows.h), 1: the plain rule."""
        if not hasattr(self._L, "ldpc_amd_fec_rxw_flows_depth"):   # (the older builds tools/ab_lib.py loads)
            return 1
        return int(self._L.ldpc_amd_fec_rxw_flows_depth(self._h))

    @property
    def rule(self):
        """The close rule every flow follows, (c_hi, later_hi, c_lo, later_lo) (include/ldpc_erasure_amd_rx_rule.h)."""
        r = RxRule()
        self._ctx._check(self._L.ldpc_amd_fec_rxw_flows_get_rule(self._h, C.byref(r)), "fec_rxw_flows_get_rule")
        return (r.c_hi, r.later_hi, r.c_lo, r.later_lo)

    def decode_many(self, code, packets, flow_begin, max_blocks_per_flow, max_sweeps=10, do_ml=1):
        """push_many + Context.decode_frames of all flows in one call -> (closes int32 [nflows], blocks int32 [T], DecodedFrames of
        the T closed blocks, consumed int64 [nflows]).  Context.fec_rx_window_flows_info() says which form ran.  Keep `packets` alive
        until the context's stream has passed the call."""
        return super().decode_many(code, packets, flow_begin, max_blocks_per_flow, max_sweeps, do_ml)

    def push_mixed(self, packets, flow_of, max_blocks_per_flow, want_left=False):
        """push_many for packets in arrival order (include/ldpc_erasure_amd_rx_window_flows_mixed.h): packets torch uint8 [P][8+S],
        flow_of torch int32 [P] on the device, flow_of[p] = the flow of packet p (outside 0 .. nflows-1: no flow, ignored and counted
        in `unrouted`).  Returns push_many's tuple for the per-flow segments, then offered int64 [nflows] (packets of each flow), then
        -- want_left -- left torch uint8 [P]: 1 for the packets behind their flow's consumed prefix, to be submitted again."""
        return super().push_mixed(packets, flow_of, max_blocks_per_flow, want_left)

    def pending(self):
        """WindowFlowsPending(base int32 [nflows] (-1: the flow has not started), cnt int32 [nflows][window]: packets every open slot
        took so far, blocks: how many blocks a flush of all flows would hand out now).  Host only."""
        base = np.zeros(self.nflows, dtype=np.int32)
        cnt = np.zeros((self.nflows, self.window), dtype=np.int32)
        total = self._L.ldpc_amd_fec_rxw_flows_pending(self._h, base.ctypes.data, cnt.ctypes.data)
        if total < 0:
            raise LdpcAmdError("fec_rxw_flows_pending: the object is closed")
        return WindowFlowsPending(base, cnt, total)

    def _flush_list(self, flows):
        sel = None if flows is None else np.ascontiguousarray(flows, dtype=np.int32).reshape(-1)
        nsel = self.nflows if sel is None else int(sel.shape[0])
        return sel, nsel, max(nsel * self.window, 1)

    def flush_many(self, flows=None):
        """FecRxWindow.flush() of every flow of the list `flows` (None: all flows) in one call -> (closes int32 [nsel], blocks int32
        [T], sym torch uint8 [T][n][S], erased torch uint8 [T][n]).  The blocks come out dense in list order, entry j's from
        closes[:j].sum() on; flows that are not listed are not touched."""
        import torch
        sel, nsel, slots = self._flush_list(flows)
        sym = torch.empty((slots, self.n, self.S), dtype=torch.uint8, device=self._device())
        er = torch.empty((slots, self.n), dtype=torch.uint8, device=self._device())
        blocks, closes = np.zeros(slots, dtype=np.int32), np.zeros(max(nsel, 1), dtype=np.int32)
        T = self._ctx._check(self._L.ldpc_amd_fec_rxw_flows_flush_many(self._h, None if sel is None else sel.ctypes.data, nsel, _ptr(sym), _ptr(er),
                                                                       blocks.ctypes.data, closes.ctypes.data), "fec_rxw_flows_flush_many")
        return closes[:nsel], blocks[:T], sym[:T], er[:T]

    def decode_flush_many(self, code, flows=None, max_sweeps=10, do_ml=1):
        """flush_many + Context.decode_frames in one call -> (closes int32 [nsel], blocks int32 [T], DecodedFrames of the T blocks);
        decoded straight from the staging planes where the decoder can fetch its rows itself."""
        sel, nsel, slots = self._flush_list(flows)
        fr = self._frames(slots)
        blocks, closes = np.zeros(slots, dtype=np.int32), np.zeros(max(nsel, 1), dtype=np.int32)
        T = self._ctx._check(self._L.ldpc_amd_fec_rxw_flows_decode_flush_many(
            self._h, code, None if sel is None else sel.ctypes.data, nsel, max_sweeps, do_ml, _ptr(fr.out), _ptr(fr.sweeps), _ptr(fr.residual),
            _ptr(fr.status), _ptr(fr.erased_out), _ptr(fr.residual_src), blocks.ctypes.data, closes.ctypes.data), "fec_rxw_flows_decode_flush_many")
        return closes[:nsel], blocks[:T], DecodedFrames(*(t[:T] for t in fr))

    def stats(self, flow):
        """FecRxWindow.stats() of flow `flow`."""
        t = (C.c_int64 * 5)()
        if self._L.ldpc_amd_fec_rxw_flows_stats(self._h, flow, t) != 0:
            raise LdpcAmdError("fec_rxw_flows_stats: bad arguments")
        return dict(zip(RX_WINDOW_TOTALS, (int(v) for v in t)))

    def state(self, flow):
        """FecRxWindow.state() of flow `flow`."""
        base, ahead = C.c_int(0), C.c_int64(0)
        cnt = np.zeros(self.window, dtype=np.int32)
        if self._L.ldpc_amd_fec_rxw_flows_state(self._h, flow, C.byref(base), cnt.ctypes.data, C.byref(ahead)) != 0:
            raise LdpcAmdError("fec_rxw_flows_state: bad arguments")
        return {"base": base.value, "cnt": cnt.tolist(), "ahead": ahead.value}

    def dropped(self, flow):
        """packets of flow `flow` that went to no block so far (-1: no such flow)"""
        return int(self._L.ldpc_amd_fec_rxw_flows_dropped(self._h, flow))


class _FecTxCounter:
    """The single-stream senders' one piece of state, the block counter: send(source) hands _encode the block number next_block
    and advances it by the frames sent modulo 256."""

    def send(self, source, out=None):
        """source: torch uint8 [F][k][S] (or [F][k] for S = 1) -> packets [F*n][8+S] in transmission order."""
        assert (1 if source.ndim == 2 else source.shape[2]) == self.S
        pk = self._encode(source, self.next_block, out)
        self.next_block = (self.next_block + source.shape[0]) & 0xFF
        return pk

    def send_datagrams_trimmed(self, data, offsets):
        """Pack + encode + trim: datagrams of any length up to S - 4 -> Wire(bytes, offset) of Context.fec_trim_packets, the bytes
        that go on the wire back to back with their boundaries on the device; no per-packet table is made on the host.  Advances
        the block counter by F, as send does."""
        return self._ctx.fec_trim_packets(self.send(self._ctx.fec_pack_datagrams(data, offsets, self.k, self.S)), self.k)


class FecTxDevice(_FecTxCounter):
    """The sender's side of FecRxDevice.  Its one piece of state is the reference's block counter (blockNum += 1 per frame,
    OpenCL/device/ldpc_erasure_encoder_VITA_in_UDP_out.cl:134): send(source) returns the packets of F frames numbered from
    next_block on and advances it by F modulo 256."""

    def __init__(self, ctx, code, S, fec_class=1, block0=0):
        self._ctx, self.code, self.S, self.fec_class = ctx, code, S, fec_class
        self.n, self.k, _ = ctx.code_info(code)
        self.next_block = block0 & 0xFF

    def _encode(self, source, block0, out):
        return self._ctx.fec_encode_packets_device(self.code, source, self.fec_class, block0, out=out)

    def send_datagrams(self, data, offsets):
        """Datagrams of any length up to S - 4 (Context.fec_pack_datagrams) -> (packets [F*n][8+S], wire_len int32 [F*n]): only
        the first wire_len[p] bytes of packet p need to be transmitted, the rest of it is zero.  Advances the block counter by F."""
        wl = fec_datagram_wire_len(offsets, self.n, self.k, self.S)
        return self.send(self._ctx.fec_pack_datagrams(data, offsets, self.k, self.S)), wl


class FecTxInterleaved(_FecTxCounter):
    """FecTxDevice for the block-interleaved wire (include/ldpc_erasure_amd_interleave.h): send(source) returns the packets of F
    frames numbered from next_block on in depth-`depth` order, the input of FecRxWindow(..., depth=depth), and advances the
    counter by F modulo 256.  A call interleaves its own frames only: send whole groups (F a multiple of depth, from a block number
    that is one) to keep every group at full depth.  There is no send_datagrams here: its wire_len table is in straight order."""

    def __init__(self, ctx, code, S, depth, fec_class=1, block0=0):
        if depth not in ILV_DEPTHS:
            raise LdpcAmdError(f"FecTxInterleaved: depth must be one of {ILV_DEPTHS} (got {depth})")
        self._ctx, self.code, self.S, self.depth, self.fec_class = ctx, code, S, depth, fec_class
        self.n, self.k, _ = ctx.code_info(code)
        self.next_block = block0 & 0xFF

    def _encode(self, source, block0, out):
        return self._ctx.fec_encode_packets_interleaved_device(self.code, source, self.depth, self.fec_class, block0, out=out)


class FecTxRs(_FecTxCounter):
    """FecTxInterleaved for the blocks of a Reed-Solomon code (include/ldpc_erasure_amd_rs_wire.h): send(source) returns the packets
    of B blocks numbered from next_block on in depth-`depth` order, class FEC_CLASS_RS, the input of
    FecRxWindow(n, k, S, ..., depth=depth).rs_decode_many, and advances the counter by B modulo 256."""

    def __init__(self, ctx, rs, S, depth=1, block0=0):
        if depth not in ILV_DEPTHS:
            raise LdpcAmdError(f"FecTxRs: depth must be one of {ILV_DEPTHS} (got {depth})")
        self._ctx, self.rs, self.S, self.depth = ctx, rs, S, depth
        self.n, self.k = ctx.rs_info(rs)
        self.next_block = block0 & 0xFF

    def _encode(self, source, block0, out):
        return self._ctx.fec_rs_encode_packets_device(self.rs, source, self.depth, FEC_CLASS_RS, block0, out=out)


class FecLink:
    """The link emulator of include/ldpc_erasure_amd_link.h on one context: every call takes the packets of one burst in send order
    and returns them as they arrive.  `first`, the position of the next packet in the link's life, advances by P per call, so the
    calls continue one stream of draws; packets do not cross a call boundary.  Loss is an input: `lost`, torch uint8 [P] on the
    device (non-zero: the packet is lost), e.g. Context.synth_erasures_uniform / _bursty with n = 1, frame0 = link.first,
    nframes = P.  plan() is asynchronous and reads nothing back; send() and send_wire() read the count back, one 8-byte read --
    the only place that synchronises."""

    def __init__(self, ctx, seed, window=0, dup=0.0, bad_sym=0.0, foreign=0.0, dup_flip=False, first=0):
        self._ctx = ctx
        self.params = LinkParams(seed & 0xFFFFFFFFFFFFFFFF, first & 0xFFFFFFFFFFFFFFFF, window, LINK_DUP_FLIP if dup_flip else 0, float(dup),
                                 float(bad_sym), float(foreign))

    @property
    def first(self):
        return int(self.params.first)

    def _device(self):
        import torch
        return torch.device("cuda", self._ctx.device)

    def plan(self, P, lost=None):
        """(src torch int32 [2P], fate torch int16 [2P] -- the bits of a uint16 --, count torch int64 [1]) on the device: entries
        0 .. count-1 say which packet arrives at each position and with what fate; the rest is not written."""
        import torch
        dev = self._device()
        if lost is not None:
            assert _is_torch(lost) and lost.dtype == torch.uint8 and tuple(lost.shape) == (P,) and lost.is_contiguous()
        cap = 2 * max(P, 0)
        src = torch.empty(cap, dtype=torch.int32, device=dev)
        fate = torch.empty(cap, dtype=torch.int16, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        c = self._ctx
        c._check(c._L.ldpc_amd_fec_link_plan_dev(c._h, C.byref(self.params), P, _ptr(lost) if P > 0 else None, _ptr(src) if cap else None,
                                                 _ptr(fate) if cap else None, cap, _ptr(count)), "fec_link_plan_dev")
        self.params.first = (self.first + P) & 0xFFFFFFFFFFFFFFFF
        return src, fate, count

    def send(self, packets, lost=None, flow_of=None):
        """packets: torch uint8 [P][8+S] on this context's device in send order (flow_of: torch int32 [P], the flow of every packet
        of a mixed wire) -> (packets_out [Q][8+S], flow_of_out [Q] or None, src [Q], fate [Q]): the packets as they arrive."""
        import torch
        assert _is_torch(packets) and packets.dtype == torch.uint8 and packets.ndim == 2 and packets.is_contiguous()
        P, plen = packets.shape
        if flow_of is not None:
            assert _is_torch(flow_of) and flow_of.dtype == torch.int32 and tuple(flow_of.shape) == (P,) and flow_of.is_contiguous()
        src, fate, count = self.plan(P, lost)
        cap = src.shape[0]
        out = torch.empty((cap, plen), dtype=torch.uint8, device=packets.device)
        fo = None if flow_of is None else torch.empty(cap, dtype=torch.int32, device=packets.device)
        c = self._ctx
        c._check(c._L.ldpc_amd_fec_link_apply_dev(c._h, _ptr(packets) if P else None, P, plen - 8, _ptr(src), _ptr(fate), _ptr(count), cap,
                                                  _ptr(out), _ptr(flow_of), _ptr(fo)), "fec_link_apply_dev")
        Q = int(count.item())
        return out[:Q], None if fo is None else fo[:Q], src[:Q], fate[:Q]

    def send_wire(self, wire, lost=None):
        """wire: Wire(bytes torch uint8 1-D, offset torch int64 [P+1]) on this context's device, the datagrams in send order (what
        Context.fec_trim_packets and FecTxDevice.send_datagrams_trimmed make; bytes may be a slice that starts at any byte) ->
        (Wire(bytes_out [total], offset_out [Q+1]), src [Q], fate [Q]): the datagrams as they arrive, back to back."""
        import torch
        wire = Wire(*wire)
        assert _is_torch(wire.bytes) and wire.bytes.dtype == torch.uint8 and wire.bytes.ndim == 1
        assert _is_torch(wire.offset) and wire.offset.dtype == torch.int64 and wire.offset.ndim == 1 and wire.offset.shape[0] >= 1
        P, nbytes = wire.offset.shape[0] - 1, wire.bytes.numel()
        src, fate, count = self.plan(P, lost)
        cap = src.shape[0]
        dev = wire.bytes.device
        out = Wire(torch.empty(2 * nbytes, dtype=torch.uint8, device=dev), torch.empty(cap + 1, dtype=torch.int64, device=dev))
        c = self._ctx
        c._check(c._L.ldpc_amd_fec_link_apply_ragged_dev(c._h, _ptr(wire.bytes) if nbytes else None, nbytes, _ptr(wire.offset), P, _ptr(src) if cap else None,
                                                         _ptr(fate) if cap else None, _ptr(count), cap, _ptr(out.bytes) if nbytes else None,
                                                         2 * nbytes, _ptr(out.offset), None), "fec_link_apply_ragged_dev")
        Q = int(count.item())
        offset = out.offset[:Q + 1]
        return Wire(out.bytes[:int(offset[-1].item())], offset), src[:Q], fate[:Q]


class FecTxFlows:
    """The sender's side of FecRxFlows: nflows FecTxDevice on one wire.  Its state is the reference's block counter, one per flow
    (blockNum += 1 per frame, OpenCL/device/ldpc_erasure_encoder_VITA_in_UDP_out.cl:134): send(source, frame_begin, order) returns
    the packets of every flow's frames numbered from next_block[f] on, in the asked order, and advances each flow's counter by its
    frame count modulo 256.  fec_class and block0: a scalar for all flows or one value per flow.  depth > 1: every flow's blocks
    are interleaved to that depth inside a call (include/ldpc_erasure_amd_interleave_flows.h), the input of
    FecRxWindowFlows(..., depth=depth); TX_ROUND_ROBIN then takes whole aligned groups only -- every flow's next_block and frame
    count a multiple of depth -- and send raises otherwise, with the counters unchanged."""

    def __init__(self, ctx, code, S, nflows, fec_class=1, block0=0, depth=1):
        if depth not in ILV_DEPTHS:
            raise LdpcAmdError(f"FecTxFlows: depth must be one of {ILV_DEPTHS} (got {depth})")
        self.depth = depth
        self._ctx, self.code, self.S, self.nflows = ctx, code, S, nflows
        self.n, self.k, _ = ctx.code_info(code)
        self.fec_class = np.ascontiguousarray(np.broadcast_to(np.asarray(fec_class, dtype=np.int64) & 0xFF, (nflows,)), dtype=np.uint8)
        self.next_block = np.array(np.broadcast_to(np.asarray(block0, dtype=np.int64) & 0xFF, (nflows,)), dtype=np.int64)

    def send(self, source, frame_begin, order=TX_ROUND_ROBIN, out=None, want_flow_of=True):
        """source: torch uint8 [F][k][S] (or [F][k] for S = 1), flow f's frames at frame_begin[f] .. frame_begin[f+1]-1 ->
        (packets, flow_of, packet_begin) of Context.fec_encode_packets_flows_device."""
        assert (1 if source.ndim == 2 else source.shape[2]) == self.S
        fb = np.ascontiguousarray(frame_begin, dtype=np.int64)
        assert fb.shape == (self.nflows + 1,)
        if self.depth == 1:   # (the older builds tools/ab_lib.py loads have this call only)
            r = self._ctx.fec_encode_packets_flows_device(self.code, source, fb, self.fec_class, self.next_block, order, out=out,
                                                          want_flow_of=want_flow_of)
        else:
            r = self._ctx.fec_encode_packets_flows_interleaved_device(self.code, source, fb, self.fec_class, self.next_block, order, self.depth,
                                                                      out=out, want_flow_of=want_flow_of)
        self.next_block = (self.next_block + np.diff(fb)) & 0xFF
        return r


def shard_frames(nframes, nranks, rank):
    """(first, count) of rank's contiguous block: the library's C shard arithmetic (ldpc_amd_shard_frames)."""
    L = load_library()
    f0, cnt = C.c_int64(), C.c_int64()
    L.ldpc_amd_shard_frames(nframes, nranks, rank, C.byref(f0), C.byref(cnt))
    return f0.value, cnt.value


class Group:
    """The C-level multi-device layer (include/ldpc_erasure_amd_multi.h): nranks contexts, one host thread each; devices may
    repeat (several ranks on one device: how the layer is tested on a one-GPU box)."""

    def __init__(self, nranks, devices=None):
        self._L = load_library()
        h = C.c_void_p()
        dv = None if devices is None else (C.c_int * nranks)(*devices)
        rc = self._L.ldpc_amd_group_create(nranks, dv, C.byref(h))
        if rc != OK:
            raise LdpcAmdError(f"ldpc_amd_group_create({nranks}) = {rc}: {self._L.ldpc_amd_last_error(None).decode()}")
        self._h = h
        self.nranks = nranks

    def close(self):
        if getattr(self, "_h", None):
            self._L.ldpc_amd_group_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc < 0:
            raise LdpcAmdError(f"{what} = {rc}: {self._L.ldpc_amd_group_last_error(self._h).decode()}")
        return rc

    def device(self, rank):
        return self._L.ldpc_amd_group_device(self._h, rank)

    def load_builtin_code(self, code_ind, coef_seed):
        return self._check(self._L.ldpc_amd_group_load_builtin_code(self._h, code_ind, coef_seed), "group_load_builtin_code")

    def register_code(self, code):
        rp = np.ascontiguousarray(code.row_ptr, dtype=np.uint32)
        cols = np.ascontiguousarray(code.cols, dtype=np.uint16)
        coefs = np.ascontiguousarray(code.coefs, dtype=np.uint8)
        return self._check(self._L.ldpc_amd_group_register_code(self._h, code.n, code.k, rp.ctypes.data, cols.ctypes.data, coefs.ctypes.data),
                           "group_register_code")

    def decode(self, code, sym, erased, max_sweeps=10, do_ml=1):
        """Host arrays sym [F,n,S] or [F,n], erased [F,n] -> (out, sweeps, residual, status), frames sharded over the ranks."""
        sym = np.ascontiguousarray(sym, dtype=np.uint8)
        erased = np.ascontiguousarray(erased, dtype=np.uint8)
        F = sym.shape[0]
        S = 1 if sym.ndim == 2 else sym.shape[2]
        out = np.empty_like(sym)
        sw, res, st = (np.empty(F, dtype=np.int32) for _ in range(3))
        self._check(self._L.ldpc_amd_group_decode_batch(self._h, code, S, F, sym.ctypes.data, erased.ctypes.data, max_sweeps, do_ml, out.ctypes.data,
                                                        sw.ctypes.data, res.ctypes.data, st.ctypes.data), "group_decode_batch")
        return out, sw, res, st

    def decode_resident(self, code, S, nframes, sym, erased, out, words, gathered_words=None, gathered_out=None, max_sweeps=10, do_ml=1):
        """Per-rank lists of torch CUDA tensors (rank r's shard on its device); gathered_*: tensors on rank 0's device or None.
        Returns (decode_ms, gather_ms)."""
        arr = lambda ts: (C.c_void_p * self.nranks)(*[t.data_ptr() if t is not None else None for t in ts])   # noqa: E731
        dms, gms = C.c_double(0), C.c_double(0)
        self._check(self._L.ldpc_amd_group_decode_resident(self._h, code, S, nframes, arr(sym), arr(erased), max_sweeps, do_ml, arr(out), arr(words),
                                                           None if gathered_words is None else gathered_words.data_ptr(),
                                                           None if gathered_out is None else gathered_out.data_ptr(), C.byref(dms), C.byref(gms)),
                    "group_decode_resident")
        return dms.value, gms.value

    def fpga_run(self, nldpc, seed, per64, code_ind, num_frames, num_iter, perf_tests_body=False):
        st = ErrorType()
        self._check(self._L.ldpc_amd_group_fpga_run(self._h, nldpc, seed, per64, code_ind, num_frames, num_iter, int(perf_tests_body), C.byref(st)),
                    "group_fpga_run")
        return st.num_LDPC_errors, st.num_RS_errors

    def bench_resident(self, code_ind, coef_seed, S, frames_per_rank, per=0.10, max_sweeps=10, steps=5):
        r = (C.c_double * 4)()
        self._check(self._L.ldpc_amd_group_bench_resident(self._h, code_ind, coef_seed, S, frames_per_rank, per, max_sweeps, steps, r), "group_bench_resident")
        return dict(zip(("frames_per_s", "decode_ms_per_step", "gather_ms", "verified"), list(r)))
