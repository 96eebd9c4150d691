// waitcnt.hpp -- the vector-memory wait of the LDS-DMA pipelines (device side; fused.hpp, narrow.hip, wide.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace sglm {

// s_waitcnt vmcnt(N) with expcnt / lgkmcnt left open (gfx9 encoding).
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

}  // namespace sglm
