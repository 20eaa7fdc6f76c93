// Order-preserving integer keys of stack values: a < b  <=>  key(a) < key(b).  Shared by the radix selects of the
// z-shift medians (corrections.hip) and of the stack order statistics (stats.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ia3key {

__device__ __forceinline__ uint32_t fkey(float v) {      // order-preserving key
  uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) {
  uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(u);
}

}  // namespace ia3key
