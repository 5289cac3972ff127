#!/bin/bash
# Builds libldpc_erasure_amd.so for gfx950 (cross-compiles without a GPU).  Called by __graft_entry__.build().
# Every translation unit is compiled to its own object (in parallel, and only when a source it depends on is newer), then linked:
# kernels.hip -- the one big device TU -- takes minutes, the host TUs seconds.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
python3 "$ROOT/tools/gen_builtin_codes.py" > /dev/null
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-strict-aliasing -Wall -Wno-unused-function ${EXTRA_HIPCC_FLAGS:-}"
OUT="${LDPC_AMD_OUT:-$ROOT/ldpc_erasure_codes_amd/libldpc_erasure_amd.so}"
OBJ="${LDPC_AMD_OBJDIR:-$HERE/obj}"
mkdir -p "$OBJ"
echo "$FLAGS" > "$OBJ/flags.new"
if ! cmp -s "$OBJ/flags.new" "$OBJ/flags" 2>/dev/null; then rm -f "$OBJ"/*.o; mv "$OBJ/flags.new" "$OBJ/flags"; fi
COMMON="$HERE/internal.h $ROOT/include/ldpc_erasure_amd.h $ROOT/include/ldpc_erasure_amd_synth.h $ROOT/include/ldpc_erasure_amd_wire.h $ROOT/include/ldpc_erasure_amd_multi.h $ROOT/include/ldpc_erasure_amd_wire_dev.h $ROOT/include/ldpc_erasure_amd_frames.h $ROOT/include/ldpc_erasure_amd_sender.h $ROOT/include/ldpc_erasure_amd_sender_flows.h $ROOT/include/ldpc_erasure_amd_receiver.h $ROOT/include/ldpc_erasure_amd_words.h $ROOT/include/ldpc_erasure_amd_flows.h $ROOT/include/ldpc_erasure_amd_flows_mixed.h $ROOT/include/ldpc_erasure_amd_flows_flush.h $ROOT/include/ldpc_erasure_amd_datagrams.h $ROOT/include/ldpc_erasure_amd_wire_ragged.h"
declare -A DEPS=(
  [kernels.hip]="$HERE/gf256_dev.h $HERE/fec_header_dev.h $HERE/peel_relax.inc $HERE/ml_kernel.inc $HERE/ml_pi.inc $HERE/rs_kernels.inc $HERE/fpga_kernels.inc"
  [api.cpp]="$HERE/builtin_codes_gen.inc"
  [wire.cpp]=""
  [multi.hip]=""
  [wire_dev.hip]="$HERE/fec_header_dev.h $HERE/rx_host.h $HERE/rx_flows_host.h $HERE/flows_demux_dev.h $ROOT/include/ldpc_erasure_amd_rx_window.h $ROOT/include/ldpc_erasure_amd_interleave.h $ROOT/include/ldpc_erasure_amd_interleave_flows.h $ROOT/include/ldpc_erasure_amd_rx_window_flows.h $ROOT/include/ldpc_erasure_amd_rs_wire.h $ROOT/include/ldpc_erasure_amd_rs_rows.h"
  [rs_wire_dev.hip]="$HERE/fec_header_dev.h $ROOT/include/ldpc_erasure_amd_rs_rows.h"
  [datagram_dev.hip]="$HERE/dgram_scan_dev.h"
  [wire_ragged_dev.hip]="$HERE/dgram_scan_dev.h"
  [link_dev.hip]="$HERE/dgram_scan_dev.h $ROOT/include/ldpc_erasure_amd_link.h"
  [rx_window.cpp]="$ROOT/include/ldpc_erasure_amd_rx_window.h $ROOT/include/ldpc_erasure_amd_rx_rule.h $ROOT/include/ldpc_erasure_amd_interleave.h"
  [rx_window_dev.hip]="$ROOT/include/ldpc_erasure_amd_rx_window.h $ROOT/include/ldpc_erasure_amd_rx_rule.h $ROOT/include/ldpc_erasure_amd_rs_wire.h $ROOT/include/ldpc_erasure_amd_rs_rows.h $ROOT/include/ldpc_erasure_amd_interleave.h $HERE/rx_window_scan_dev.h $HERE/rx_host.h"
  [rx_window_flows_dev.hip]="$ROOT/include/ldpc_erasure_amd_rx_window.h $ROOT/include/ldpc_erasure_amd_rx_rule.h $ROOT/include/ldpc_erasure_amd_interleave.h $ROOT/include/ldpc_erasure_amd_interleave_flows.h $ROOT/include/ldpc_erasure_amd_rx_window_flows.h $ROOT/include/ldpc_erasure_amd_rx_window_flows_mixed.h $HERE/rx_window_scan_dev.h $HERE/rx_host.h $HERE/rx_flows_host.h $HERE/flows_demux_dev.h"
)
pids=()
for src in kernels.hip api.cpp wire.cpp multi.hip wire_dev.hip rs_wire_dev.hip datagram_dev.hip wire_ragged_dev.hip link_dev.hip rx_window.cpp rx_window_dev.hip rx_window_flows_dev.hip; do
  o="$OBJ/${src%.*}.o"
  stale=0
  [ -f "$o" ] || stale=1
  for d in "$HERE/$src" $COMMON ${DEPS[$src]}; do
    if [ "$stale" = 0 ] && [ "$d" -nt "$o" ]; then stale=1; fi
  done
  if [ "$stale" = 1 ]; then
    ( "$HIPCC" $FLAGS -c -o "$o.tmp" "$HERE/$src" && mv "$o.tmp" "$o" ) &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -o "$OUT" "$OBJ/kernels.o" "$OBJ/api.o" "$OBJ/wire.o" "$OBJ/multi.o" "$OBJ/wire_dev.o" "$OBJ/rs_wire_dev.o" "$OBJ/datagram_dev.o" "$OBJ/wire_ragged_dev.o" "$OBJ/link_dev.o" "$OBJ/rx_window.o" "$OBJ/rx_window_dev.o" "$OBJ/rx_window_flows_dev.o"
echo "$OUT"
