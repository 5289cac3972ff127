// fec_header_dev.h -- the FEC packet header on the device, shared by the packetiser (wire_dev.hip) and the packet-output form
// of the encoder (kernels.hip).  Host counterpart: ldpc_amd_fec_header_pack (csrc/wire.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldpc_amd {

__device__ __forceinline__ uint64_t fec_header(unsigned fec_class, unsigned block, unsigned symbol)
{
    // ldpc_amd_fec_header_pack: {class:8 | block:8 | symbol:16} in both halves of a 64-bit word
    const uint64_t d = ((uint64_t)(fec_class & 0xffu) << 24) | ((uint64_t)(block & 0xffu) << 16) | (uint64_t)(symbol & 0xffffu);
    return (d << 32) | d;
}

}  // namespace ldpc_amd
