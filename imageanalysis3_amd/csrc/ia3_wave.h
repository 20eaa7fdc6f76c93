// Two wavefront idioms of ballot compaction, stated once (device code only).
#pragma once

namespace ia3 {

// number of set bits of `mask` below this lane: the lane's place among the lanes that voted true
__device__ __forceinline__ int lane_rank(unsigned long long mask) {
  const int lane = threadIdx.x & 63;
  return __popcll(mask & ((1ull << lane) - 1ull));
}

// Wave-aggregated append: the wave adds its number of hits to *counter with ONE atomic (lane 0 issues it, so the whole
// wave must be here: every caller runs full wavefronts) and each hit lane gets its own position behind the old value, in
// lane order.  The value returned to a lane without a hit means nothing.  Capacity and overflow are the caller's.
template <class T>
__device__ __forceinline__ T wave_append(T* counter, bool hit) {
  const unsigned long long ballot = __ballot(hit);
  if (!ballot) return (T)0;   // wave-uniform
  T base = 0;
  if ((threadIdx.x & 63) == 0) base = atomicAdd(counter, (T)__popcll(ballot));
  return __shfl(base, 0) + (T)lane_rank(ballot);
}

}  // namespace ia3
