// Device-resident batched map lookup, update and delete (xe_mapops.h: the steps and what each one
// decides). One kernel per step; a step works either one batch entry per lane (probes, claims, marks) or
// one entry per sub-group of lanes (value moves, 16 bytes per lane and access where source and
// destination allow it).
//
// 256-thread workgroups. Up to kMoOneTurn of them take one entry (or one sub-group's entry) per lane:
// 65,536 keys in a lane step. A larger batch gets a quarter of the workgroups it would need for that, at
// least kMoOneTurn and at most kMoMaxBlocks, and its lanes stride on: the probes of a large batch are
// latency-bound, and a lane that walks four keys amortises its launch while 4 to 8 workgroups per CU
// stay resident to overlap the round trips.
#include <hip/hip_runtime.h>

#include "xe_mapops.h"

namespace {

constexpr uint32_t kMoThreads = 256, kMoOneTurn = 256, kMoMaxBlocks = 2048;

// The probe of xe_interp.h hash_find for records shorter than a 64-byte group (RW = 2 or 4 words: keys up
// to 8 or 24 bytes): every record from the probe position to the end of its group is loaded in one burst of
// 16-byte loads, then scanned in slot order — first match / stop at the first record that is neither FULL
// nor a tombstone. A chain that stays inside the line costs one round trip. (cap is a multiple of the
// group: it is a power of two >= 16.)
template <uint32_t RW>
__device__ __forceinline__ uint32_t find_grouped(const XeMapOp& o, const uint64_t* kw) {
  constexpr uint32_t G = 8 / RW, KW = RW - 1;
  const uint32_t mask = o.cap - 1;
  uint32_t idx = uint32_t(xe_hash_words(kw, o.kwords, o.key_size)) & mask;
#pragma unroll 1
  for (uint32_t probe = 0; probe < o.cap;) {
    const uint32_t first = idx & (G - 1);
    const uint4* r = reinterpret_cast<const uint4*>(o.recs + uint64_t(idx - first) * RW);
    uint4 a[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) a[j] = r[j];
    uint64_t w[8];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      w[2 * j] = uint64_t(a[j].x) | uint64_t(a[j].y) << 32;
      w[2 * j + 1] = uint64_t(a[j].z) | uint64_t(a[j].w) << 32;
    }
    uint32_t hit = 0, stop = 0;
#pragma unroll
    for (uint32_t g = 0; g < G; g++) {
      const uint32_t st = uint32_t(w[g * RW]);
      const bool full = (st & XE_SLOT_FULL) != 0;
      bool eq = true;
#pragma unroll
      for (uint32_t k = 0; k < KW; k++)
        if (k < o.kwords) eq = eq && w[g * RW + 1 + k] == kw[k];
      hit |= uint32_t(full && eq) << g;
      stop |= uint32_t(!full && !(st & XE_SLOT_TOMB)) << g;
    }
    const uint32_t act = (hit | stop) & (~0u << first);
    if (act) {
      const uint32_t g0 = uint32_t(__builtin_ctz(act));
      return ((hit >> g0) & 1u) ? idx - first + g0 : kMoAbsent;
    }
    probe += G - first;
    idx = (idx - first + G) & mask;
  }
  return kMoAbsent;
}

__device__ __forceinline__ uint32_t find_slot(const XeMapOp& o, uint32_t i) {
  if (o.kind == XE_DM_ARRAY || o.key_size == 0) return mo_slot_of(o, i);
  uint64_t kw[XE_MAX_KEY / 8];
  mo_load_key(o, i, kw);
  if (o.rwords == 2) return find_grouped<2>(o, kw);
  if (o.rwords == 4) return find_grouped<4>(o, kw);
  return mo_find(o, kw);
}

// one entry per lane
__global__ void __launch_bounds__(kMoThreads) xe_mapop_lane_kernel(XeMapOp o, uint32_t step) {
  const uint32_t stride = gridDim.x * kMoThreads;
  // every lane of a wave takes the same number of turns (the ballot below wants the whole wave)
  const uint32_t turns = (o.n + stride - 1) / stride;
  uint32_t i = blockIdx.x * kMoThreads + threadIdx.x;
  for (uint32_t t = 0; t < turns; t++, i += stride) {
    const bool in = i < o.n;  // (n <= 2^32 - 2^17: i does not wrap)
    bool fresh = false;
    if (in) {
      switch (step) {
        case XE_MO_LOOKUP_FIND: mo_find_finish(o, i, find_slot(o, i), true); break;
        case XE_MO_DELETE_FIND: mo_find_finish(o, i, find_slot(o, i), false); break;
        case XE_MO_UPDATE_LOCATE: fresh = mo_update_locate_item(o, i); break;
        case XE_MO_UPDATE_UNDO: mo_update_undo_item(o, i); break;
        case XE_MO_UPDATE_MARK: mo_update_mark_item(o, i); break;
        case XE_MO_DELETE_CLAIM: mo_delete_claim_item(o, i); break;
        default: break;
      }
    }
    if (step == XE_MO_UPDATE_LOCATE) {  // the claims, counted once per wave
      const unsigned long long b = __ballot(fresh);
      if (b && (threadIdx.x & 63) == uint32_t(__builtin_ctzll(b))) mo_add32(o.ctr + kMoNew, uint32_t(__popcll(b)));
    }
  }
}

// one entry per LANES consecutive lanes
template <uint32_t LANES>
__global__ void __launch_bounds__(kMoThreads) xe_mapop_value_kernel(XeMapOp o, uint32_t step) {
  const uint32_t sub = threadIdx.x % LANES, per = kMoThreads / LANES;
  const uint64_t stride = uint64_t(gridDim.x) * per;
  for (uint64_t i = uint64_t(blockIdx.x) * per + threadIdx.x / LANES; i < o.n; i += stride) {
    switch (step) {
      case XE_MO_LOOKUP_VALUE: mo_lookup_value_item(o, uint32_t(i), sub, LANES); break;
      case XE_MO_UPDATE_COPY: mo_update_copy_item(o, uint32_t(i), sub, LANES); break;
      case XE_MO_DELETE_ZERO: mo_delete_zero_item(o, uint32_t(i), sub, LANES); break;
      default: break;
    }
  }
}

}  // namespace

extern "C" int xe_launch_mapop(const XeMapOp* op, uint32_t step, void* stream) {
  if (!op->n) return 0;
  hipStream_t s = hipStream_t(stream);
  const bool value = step == XE_MO_LOOKUP_VALUE || step == XE_MO_UPDATE_COPY || step == XE_MO_DELETE_ZERO;
  const uint32_t lanes = value ? xe_mo_lanes(op->value_size) : 1, per = kMoThreads / lanes;
  const uint64_t want = (uint64_t(op->n) + per - 1) / per;
  const uint64_t blocks = want <= kMoOneTurn ? want : want / 4 < kMoOneTurn ? kMoOneTurn : want / 4 < kMoMaxBlocks ? want / 4 : kMoMaxBlocks;
  const dim3 grid{uint32_t(blocks)}, block(kMoThreads);
  if (!value) hipLaunchKernelGGL(xe_mapop_lane_kernel, grid, block, 0, s, *op, step);
  else if (lanes == 1) hipLaunchKernelGGL(xe_mapop_value_kernel<1>, grid, block, 0, s, *op, step);
  else if (lanes == 4) hipLaunchKernelGGL(xe_mapop_value_kernel<4>, grid, block, 0, s, *op, step);
  else if (lanes == 16) hipLaunchKernelGGL(xe_mapop_value_kernel<16>, grid, block, 0, s, *op, step);
  else hipLaunchKernelGGL(xe_mapop_value_kernel<64>, grid, block, 0, s, *op, step);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
