// host_util.h - the host one-liners every translation unit's C-ABI entries use.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// what an entry returns after its launches: 0, or the HIP error of a launch that was refused
inline int launch_status() { return (int)hipGetLastError(); }
// blocks of `threads` over n items
inline int64_t nblocks(int64_t n, int threads) { return (n + threads - 1) / threads; }
// every part of a carved workspace starts on 256 bytes (tinysplat_amd/_field.py: align256 carves the same way)
inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

}  // namespace
