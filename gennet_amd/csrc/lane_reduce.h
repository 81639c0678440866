// Fixed-order all-reduce over aligned sub-groups of the lanes of a wave, shared by the row kernels (csrc/softmax.hip, csrc/layernorm.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace gn {

// The value this lane's partner holds at butterfly step D = 1, 2, 4, ... of a reduction whose steps below D are done, so that the D lanes of
// an aligned group already agree: lane ^ D for D = 1, 2 (quad_perm), 16, 32 (through the LDS crossbar); for D = 4, 8 the mirrored lane of the
// 8 / 16 (row_half_mirror, row_mirror), which lies in the group lane ^ D lies in and so holds its value.  Every lane of the wave is active.
template <int CTRL>
__device__ __forceinline__ float dpp_read(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int D>
__device__ __forceinline__ float partner(float v) {
  if constexpr (D == 1) return dpp_read<0xB1>(v);          // quad_perm [1, 0, 3, 2]
  else if constexpr (D == 2) return dpp_read<0x4E>(v);     // quad_perm [2, 3, 0, 1]
  else if constexpr (D == 4) return dpp_read<0x141>(v);    // row_half_mirror
  else if constexpr (D == 8) return dpp_read<0x140>(v);    // row_mirror
  else return __shfl_xor(v, D, 64);
}
// all-reduce over aligned sub-groups of W lanes, steps D = 1, 2, ..., W / 2: both partners form the same a + b, so every lane ends with the same bits
template <int W, bool MAX, int D = 1>
__device__ __forceinline__ float group_reduce(float v) {
  if constexpr (D < W) {
    const float o = partner<D>(v);
    return group_reduce<W, MAX, 2 * D>(MAX ? fmaxf(v, o) : v + o);
  } else {
    return v;
  }
}

}  // namespace gn
