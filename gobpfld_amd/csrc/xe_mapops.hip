// Device-resident batched map lookup, update and delete, scan / expire, top / evict / stats, group, compact, modify, join (xe_mapops.h:
// the steps and what each one decides). One kernel per step; a step works either one batch entry per lane
// (probes, claims, marks) or one entry per sub-group of lanes (value moves, 16 bytes per lane and access where source and
// destination allow it). Scan and expire add one wave per tile of slots (SELECT, SCATTER) and a
// one-workgroup prefix sum of the tile counts (SCAN); their COPY and EXPIRE are value kernels.
//
// The xe_lru_* calls run the same kernels over an LRU view and add four lane steps (TOUCH, CLAIM, ERASE, RANK) and
// SORT, the library's device radix sort over the r selected (rank key, slot) pairs.
//
// 256-thread workgroups. Up to kMoOneTurn of them take one entry (or one sub-group's entry) per lane:
// 65,536 keys in a lane step. A larger batch gets a quarter of the workgroups it would need for that, at
// least kMoOneTurn and at most kMoMaxBlocks, and its lanes stride on: the probes of a large batch are
// latency-bound, and a lane that walks four keys amortises its launch while 4 to 8 workgroups per CU
// stay resident to overlap the round trips.
#include <hip/hip_runtime.h>
#include <hipcub/device/device_radix_sort.hpp>

#include "xe_mapops.h"

namespace {

constexpr uint32_t kMoThreads = 256, kMoOneTurn = 256, kMoMaxBlocks = 2048;

// The probe of xe_interp.h hash_find for records shorter than a 64-byte group (RW = 2 or 4 words: keys up
// to 8 or 24 bytes): every record from the probe position to the end of its group is loaded in one burst of
// 16-byte loads, then scanned in slot order — first match / stop at the first record that is neither FULL
// nor a tombstone. A chain that stays inside the line costs one round trip. (cap is a multiple of the
// group: it is a power of two >= 16.)
template <uint32_t RW>
__device__ __forceinline__ uint32_t find_grouped(const XeMapView& o, const uint64_t* kw) {
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

// The kernels' read-only probe of HASH table v (the Find of mo_slot_of and mg_slot_of); the empty key's rwords is 1.
__device__ __forceinline__ uint32_t find_slot(const XeMapView& v, const uint64_t* kw) {
  if (v.rwords == 2) return find_grouped<2>(v, kw);
  if (v.rwords == 4) return find_grouped<4>(v, kw);
  return mo_find(v, kw);
}

// `mine` counted into *ctr once per wave (every lane of the wave is here).
__device__ __forceinline__ void count_once_per_wave(uint32_t* ctr, bool mine) {
  const unsigned long long b = __ballot(mine);
  if (b && (threadIdx.x & 63) == uint32_t(__builtin_ctzll(b))) mo_add32(ctr, uint32_t(__popcll(b)));
}

// one entry per lane
__global__ void __launch_bounds__(kMoThreads) xe_mapop_lane_kernel(XeMapOp o, uint32_t step) {
  const uint32_t stride = gridDim.x * kMoThreads;
  // every lane of a wave takes the same number of turns (the ballot below wants the whole wave)
  const uint32_t turns = (o.n + stride - 1) / stride;
  uint32_t i = blockIdx.x * kMoThreads + threadIdx.x;
  for (uint32_t t = 0; t < turns; t++, i += stride) {
    const bool in = i < o.n;  // (n <= 2^32 - 2^17: i does not wrap)
    bool fresh = false, gone = false;
    if (in) {
      switch (step) {
        case XE_MO_LRU_TOUCH: ml_touch_item(o, i); break;
        case XE_MO_LRU_CLAIM: gone = ml_claim_item(o, i); break;
        case XE_MO_LRU_ERASE: ml_erase_item(o, i); break;
        case XE_MO_LRU_RANK: ml_rank_item(o, i); break;
        case XE_MO_LOOKUP_FIND: mo_find_finish(o, i, mo_slot_of(o, i, find_slot), true); break;
        case XE_MO_DELETE_FIND: mo_find_finish(o, i, mo_slot_of(o, i, find_slot), false); break;
        case XE_MO_UPDATE_LOCATE: fresh = mo_update_locate_item(o, i); break;
        case XE_MO_UPDATE_UNDO: mo_update_undo_item(o, i); break;
        case XE_MO_UPDATE_MARK: mo_update_mark_item(o, i); break;
        case XE_MO_DELETE_CLAIM: mo_delete_claim_item(o, i); break;
        case XE_MO_MODIFY_MARK: mm_mark_item(o, i); break;
        default: break;
      }
    }
    if (step == XE_MO_UPDATE_LOCATE) count_once_per_wave(o.ctr + kMoNew, fresh);  // the claims
    if (step == XE_MO_LRU_CLAIM) count_once_per_wave(o.ctr + kMoGone, gone);      // the winners
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
      case XE_MO_SCAN_COPY: ms_copy_item(o, uint32_t(i), sub, LANES); break;
      case XE_MO_SCAN_EXPIRE: ms_expire_item(o, uint32_t(i), sub, LANES); break;
      case XE_MO_MODIFY_EDIT: mm_modify_item(o, o.slot[i], sub, LANES, false); break;
      case XE_MO_MODIFY_KEYED: mm_keyed_item(o, uint32_t(i), sub, LANES); break;
      default: break;
    }
  }
}

// ---- scan / expire. SELECT and SCATTER: one wave per tile of kMsTile consecutive slots, kMsRounds rounds
// of one slot per lane; the waves stride over the tiles. A wave's round reads word 0 of 64 consecutive
// records (512 to 4,096 contiguous bytes) and, for the FULL ones, the field's bytes of 64 consecutive
// values; the rounds are independent, so their loads are in flight together.
template <class F>
__device__ __forceinline__ void tile_walk(uint32_t tiles, F f) {  // f(t, lane)
  const uint32_t lane = threadIdx.x & 63, waves = gridDim.x * (kMoThreads / 64);
  for (uint32_t t = blockIdx.x * (kMoThreads / 64) + (threadIdx.x >> 6); t < tiles; t += waves) f(t, lane);
}
__device__ __forceinline__ uint32_t tile_slot(uint32_t t, uint32_t r, uint32_t lane) { return t * kMsTile + r * 64 + lane; }
__device__ __forceinline__ void tile_words(const uint64_t* bitmap, uint32_t t, uint64_t (&word)[kMsRounds]) {
#pragma unroll
  for (uint32_t r = 0; r < kMsRounds; r++) word[r] = bitmap[uint64_t(t) * kMsRounds + r];
}

__global__ void __launch_bounds__(kMoThreads) xe_mapscan_select_kernel(XeMapOp o, uint32_t tiles) {
  tile_walk(tiles, [&](uint32_t t, uint32_t lane) {
    bool hit[kMsRounds];
#pragma unroll
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const uint32_t s = tile_slot(t, r, lane);
      hit[r] = s < o.nslots && ms_select_item(o, s);
    }
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const unsigned long long b = __ballot(hit[r]);
      if (lane == 0) o.bitmap[uint64_t(t) * kMsRounds + r] = b;
      cnt += uint32_t(__popcll(b));
    }
    if (lane == 0) o.tile[t] = cnt;
  });
}

// The exclusive sum of x over the workgroup's kThreads threads, and the sum of all: an inclusive scan across
// each wave, the waves' sums through LDS (wsum: a word per wave; a barrier before it is written again).
template <uint32_t kThreads>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t x, uint32_t* wsum, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = x;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(inc, d, 64);
    if (lane >= d) inc += y;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t before = inc - x, all = 0;
#pragma unroll
  for (uint32_t k = 0; k < kThreads / 64; k++) {
    const uint32_t s = wsum[k];
    before += k < w ? s : 0;
    all += s;
  }
  *total = all;
  return before;
}

// Exclusive sums of the tile counts in place, by one workgroup: four counts per lane, a carry from pass to pass.
__global__ void __launch_bounds__(kMsScanThreads) xe_mapscan_scan_kernel(XeMapOp o, uint32_t tiles) {
  __shared__ uint32_t wsum[kMsScanThreads / 64];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < tiles; base += kMsScanPass) {
    const uint32_t at = base + threadIdx.x * 4;
    uint32_t x[4], all;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) x[j] = at + j < tiles ? o.tile[at + j] : 0;
    uint32_t e = carry + block_exclusive_scan<kMsScanThreads>(x[0] + x[1] + x[2] + x[3], wsum, &all);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      if (at + j < tiles) o.tile[at + j] = e;
      e += x[j];
    }
    carry += all;
    __syncthreads();  // (wsum is written again in the next pass)
  }
  if (threadIdx.x == 0) o.ctr[kMoMatched] = carry;
}

__global__ void __launch_bounds__(kMoThreads) xe_mapscan_scatter_kernel(XeMapOp o, uint32_t tiles) {
  tile_walk(tiles, [&](uint32_t t, uint32_t lane) {
    uint32_t before = o.tile[t];
    if (before >= o.n) return;  // every entry to report lies in front of this tile
    uint64_t word[kMsRounds];
    tile_words(o.bitmap, t, word);
#pragma unroll
    for (uint32_t r = 0; r < kMsRounds; r++) {
      ms_scatter_item(o, t, r, lane, word[r], before);
      before += uint32_t(__popcll(word[r]));
    }
  });
}

// ---- top / evict / stats. PREFIX, CUT, TRIM and STATS keep SELECT's shape (a wave per tile, four
// independent rounds, the waves striding over the tiles).
//
// PREFIX: the workgroup's 256 bins live in LDS. A flow table's counters leave most of a wide field's high
// bytes zero, so a round's keys usually share one bin: the first eligible lane's bin is counted once for
// the wave (one LDS atomic instead of 64 to one address), the lanes in other bins add on their own.
__global__ void __launch_bounds__(kMoThreads) xe_maptop_prefix_kernel(XeMapOp o, uint32_t tiles) {
  __shared__ uint32_t hist[kMtBins];
  static_assert(kMtBins == kMoThreads, "one bin per thread");
  hist[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t prefix = mt_prefix(o);
  tile_walk(tiles, [&](uint32_t t, uint32_t lane) {
    uint64_t key[kMsRounds];
    bool in[kMsRounds];
#pragma unroll
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const uint32_t s = tile_slot(t, r, lane);
      key[r] = 0;
      in[r] = s < o.nslots && mt_key_item(o, s, &key[r]) && mt_in_prefix(o, key[r], prefix);
    }
#pragma unroll
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const unsigned long long act = __ballot(in[r]);
      if (!act) continue;
      const uint32_t bin = mt_bin(o, key[r]);
      const uint32_t lead = uint32_t(__builtin_ctzll(act)), lbin = uint32_t(__shfl(int(bin), int(lead), 64));
      const unsigned long long same = __ballot(in[r] && bin == lbin);
      if (lane == lead) atomicAdd(&hist[lbin], uint32_t(__popcll(same)));
      else if (in[r] && bin != lbin) atomicAdd(&hist[bin], 1u);
    }
  });
  __syncthreads();
  const uint32_t c = hist[threadIdx.x];
  if (c) mo_add32(o.bins + threadIdx.x, c);
}

// PICK: one bin per thread and the exclusive sums of the bins.
__global__ void __launch_bounds__(kMtBins) xe_maptop_pick_kernel(XeMapOp o, uint32_t) {
  __shared__ uint32_t wsum[kMtBins / 64];
  const uint32_t t = threadIdx.x, c = o.bins[t];
  uint32_t need = o.ctr[kMtNeed], total;
  // (the scan's barrier also: every thread has read the counters before one of them writes)
  const uint32_t before = block_exclusive_scan<kMtBins>(c, wsum, &total);
  if (o.t_pass == 0) {
    need = total < o.t_k ? total : o.t_k;
    if (t == 0) o.ctr[kMtMatched] = total;
  }
  if (mt_pick_here(need, before, c)) mt_pick_write(o, t, need, before);
  o.bins[t] = 0;
}

// CUT and MARK: one pass over the source's slots that sorts them into two classes. cls(s) of a slot below
// nslots: 1, 2 or neither; one ballot a round into the first bitmap with the bit "class 1", one into the second
// with the bit "class 2"; lane 0 then gets the tile's two counts: done(t, c1, c2).
template <class Cls, class Done>
__device__ __forceinline__ void two_class_pass(const XeMapOp& o, uint32_t tiles, Cls cls, Done done) {
  tile_walk(tiles, [&](uint32_t t, uint32_t lane) {
    uint32_t c[kMsRounds];
#pragma unroll
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const uint32_t s = tile_slot(t, r, lane);
      c[r] = s < o.nslots ? cls(s) : 0;
    }
    uint32_t c1 = 0, c2 = 0;
#pragma unroll
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const unsigned long long b1 = __ballot(c[r] == 1), b2 = __ballot(c[r] == 2);
      if (lane == 0) {
        o.bitmap[uint64_t(t) * kMsRounds + r] = b1;
        o.bitmap2[uint64_t(t) * kMsRounds + r] = b2;
      }
      c1 += uint32_t(__popcll(b1));
      c2 += uint32_t(__popcll(b2));
    }
    if (lane == 0) done(t, c1, c2);
  });
}

__global__ void __launch_bounds__(kMoThreads) xe_maptop_cut_kernel(XeMapOp o, uint32_t tiles) {
  const uint64_t cut = mt_prefix(o);
  const uint32_t need = o.ctr[kMtNeed];
  two_class_pass(o, tiles, [&](uint32_t s) { return mt_cut_item(o, s, cut, need); }, [&](uint32_t t, uint32_t c1, uint32_t c2) {
    o.tile[t] = c1;
    o.tile2[t] = c2;
  });
}

__global__ void __launch_bounds__(kMoThreads) xe_maptop_trim_kernel(XeMapOp o, uint32_t tiles) {
  const uint32_t need = o.ctr[kMtNeed];
  tile_walk(tiles, [&](uint32_t t, uint32_t lane) {
    uint32_t before = o.tile2[t];
    if (before >= need) return;  // every equal to keep lies in front of this tile
    uint64_t word[kMsRounds];
    tile_words(o.bitmap2, t, word);
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const unsigned long long kept = __ballot(mt_trim_item(lane, word[r], before, need));
      if (lane == 0 && kept) o.bitmap[uint64_t(t) * kMsRounds + r] |= kept;
      cnt += uint32_t(__popcll(kept));
      before += uint32_t(__popcll(word[r]));
    }
    if (lane == 0 && cnt) o.tile[t] += cnt;
  });
}

__global__ void __launch_bounds__(kMoThreads) xe_maptop_stats_kernel(XeMapOp o, uint32_t tiles) {
  XeMtStats a{};
  tile_walk(tiles, [&](uint32_t t, uint32_t lane) {
#pragma unroll
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const uint32_t s = tile_slot(t, r, lane);
      if (s < o.nslots) mt_stats_item(o, s, &a);
    }
  });
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) {
    const uint64_t cn = __shfl_xor((unsigned long long)a.count, int(d), 64), sm = __shfl_xor((unsigned long long)a.sum, int(d), 64);
    const uint64_t mn = __shfl_xor((unsigned long long)a.nmin, int(d), 64), mx = __shfl_xor((unsigned long long)a.max, int(d), 64);
    a.count += cn;
    a.sum += sm;
    a.nmin = a.nmin > mn ? a.nmin : mn;
    a.max = a.max > mx ? a.max : mx;
  }
  // the waves of a workgroup meet in LDS: the atomics all go to the same four words, so fewer is faster
  __shared__ XeMtStats part[kMoThreads / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t w = 1; w < kMoThreads / 64; w++) {
      a.count += part[w].count;
      a.sum += part[w].sum;
      a.nmin = a.nmin > part[w].nmin ? a.nmin : part[w].nmin;
      a.max = a.max > part[w].max ? a.max : part[w].max;
    }
    mt_stats_flush(o, a);
  }
}

// ---- group. LOCATE and ADD read the source bitmap a wave per tile (SCATTER's shape); UNDO and PUBLISH walk the
// destination table a wave per tile (SELECT's shape). A lane's work is a probe of the destination, so the
// rounds of a tile run one after another.
__global__ void __launch_bounds__(kMoThreads) xe_mapgroup_locate_kernel(XeMapOp o, uint32_t tiles) {
  tile_walk(tiles, [&](uint32_t t, uint32_t lane) {
    uint64_t word[kMsRounds];
    tile_words(o.bitmap, t, word);
#pragma unroll 1
    for (uint32_t r = 0; r < kMsRounds; r++) {
      if (!word[r]) continue;
      count_once_per_wave(o.ctr + kMoNew, ((word[r] >> lane) & 1) && mg_locate_item(o, tile_slot(t, r, lane)));  // the claims
    }
  });
}

// ADD. A low-cardinality group-by sends most of a round's lanes to one or two destination slots, and many
// adders on one address serialise in the L2. So, as xe_maptop_prefix_kernel does for its leader's bin, the
// wave combines first: the first remaining lane leads, the lanes with its slot are balloted, their count is a
// popcount and their measures a wave sum, the leader adds once for all of them; kMgLeaders times a round, the
// lanes still left add singly.
__global__ void __launch_bounds__(kMoThreads) xe_mapgroup_add_kernel(XeMapOp o, uint32_t tiles) {
  const bool measured = o.g_sum_off != kMgNone;
  tile_walk(tiles, [&](uint32_t t, uint32_t lane) {
    uint64_t word[kMsRounds];
    tile_words(o.bitmap, t, word);
#pragma unroll 1
    for (uint32_t r = 0; r < kMsRounds; r++) {
      if (!word[r]) continue;
      const uint32_t s = tile_slot(t, r, lane);
      uint32_t ds = kMoAbsent;
      uint64_t m = 0;
      if ((word[r] >> lane) & 1) {
        ds = mg_slot_of(o, s, find_slot);
        if (measured) m = mg_measure(o, o.sbase + s);
      }
      bool left = ds != kMoAbsent;
#pragma unroll 1
      for (uint32_t l = 0; l < kMgLeaders; l++) {
        const unsigned long long act = __ballot(left);
        if (!act) break;
        const uint32_t lead = uint32_t(__builtin_ctzll(act)), lds = uint32_t(__shfl(int(ds), int(lead), 64));
        const bool mine = left && ds == lds;
        const unsigned long long same = __ballot(mine);
        uint64_t sum = mine ? m : 0;
        if (measured) {
#pragma unroll
          for (uint32_t d = 32; d; d >>= 1) sum += __shfl_xor((unsigned long long)sum, int(d), 64);
        }
        if (lane == lead) mg_add_item(o, lds, uint64_t(__popcll(same)), sum);
        left = left && !mine;
      }
      if (left) mg_add_item(o, ds, 1, m);
    }
  });
}

// UNDO / PUBLISH over the destination table. PUBLISH: a value of up to kMoInline bytes is zeroed by its record's
// lane; a larger one by the whole wave, one claimed record of the round after another.
__global__ void __launch_bounds__(kMoThreads) xe_mapgroup_dst_kernel(XeMapOp o, uint32_t step) {
  if (step == XE_MO_GROUP_PUBLISH && blockIdx.x == 0 && threadIdx.x == 0) mg_publish_count(o);
  tile_walk(xe_ms_tiles(o.dst.cap), [&](uint32_t t, uint32_t lane) {
#pragma unroll 1
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const uint32_t ds = tile_slot(t, r, lane);
      const bool in = ds < o.dst.cap;
      if (step == XE_MO_GROUP_UNDO) {
        if (in) mg_undo_item(o, ds);
        continue;
      }
      const bool claimed = in && mg_claimed(o, ds);
      if (o.dst.value_size <= kMoInline) {
        if (claimed) mg_publish_item(o, ds, 0, 1);
        continue;
      }
      unsigned long long todo = __ballot(claimed);
      while (todo) {
        const uint32_t l = uint32_t(__builtin_ctzll(todo));
        todo &= todo - 1;
        mg_publish_item(o, tile_slot(t, r, l), lane, 64);
      }
    }
  });
}

// ---- compact. MARK has SELECT's shape and reads word 0 of every record once: two ballots a round, the tile's
// tombstones for SCAN, the tile's free records in one atomic.
__global__ void __launch_bounds__(kMoThreads) xe_mapcompact_mark_kernel(XeMapOp o, uint32_t tiles) {
  two_class_pass(o, tiles, [&](uint32_t s) { return mc_mark_item(o, s); }, [&](uint32_t t, uint32_t frees, uint32_t tombs) {
    o.tile[t] = tombs;
    if (frees) mo_add32(o.ctr + kMcFree, frees);
  });
}

// REBUILD: a lane whose slot starts a run measures it from the bitmaps. Values of up to kMoInline bytes: the lane
// walks its run alone. Larger values: the wave takes the runs of the round one after another, as PUBLISH takes
// its records: lane 0 decides where each record goes, every lane moves its share of the value.
__global__ void __launch_bounds__(kMoThreads) xe_mapcompact_rebuild_kernel(XeMapOp o, uint32_t tiles) {
  tile_walk(tiles, [&](uint32_t t, uint32_t lane) {
#pragma unroll 1
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const uint32_t s = tile_slot(t, r, lane);
      uint32_t len = 0, first = 0, moved = 0;
      bool mine = false;
      if (s < o.nslots && mc_run_start(o, s)) {
        len = mc_run_scan(o, s, &first);
        mine = mc_run_counts(o, len, first);
      }
      unsigned long long todo = __ballot(mine);
      if (!todo) continue;
      if (o.value_size <= kMoInline) {
        if (mine) {
          for (uint32_t j = first; j < len; j++) {
            const uint32_t q = mc_target(o, s, j);
            moved += q < j;
            mc_apply(o, s, j, q, 0, 1);
          }
        }
      } else {
        while (todo) {
          const int l = __builtin_ctzll(todo);
          todo &= todo - 1;
          const uint32_t rs = uint32_t(__shfl(int(s), l, 64)), rlen = uint32_t(__shfl(int(len), l, 64));
#pragma unroll 1
          for (uint32_t j = uint32_t(__shfl(int(first), l, 64)); j < rlen; j++) {
            const uint32_t q = uint32_t(__shfl(int(lane == 0 ? mc_target(o, rs, j) : 0u), 0, 64));
            moved += lane == 0 && q < j;
            mc_apply(o, rs, j, q, lane, 64);
          }
        }
      }
      // the entries moved, counted once per wave
#pragma unroll
      for (uint32_t d = 32; d; d >>= 1) moved += uint32_t(__shfl_xor(int(moved), int(d), 64));
      if (lane == 0 && moved) mo_add32(o.ctr + kMcMoved, moved);
    }
  });
}

// ---- modify. TILE has SELECT's shape: the filter of the four rounds first (their loads are in flight
// together), then a selected slot's lane edits its value where it lies (mm_modify_item with the lane alone: no
// store of one lane meets another's). The ballot takes the whole wave: a lane whose slot lies past the table
// votes "not selected". The wave's matches are counted once, after its last tile.
__global__ void __launch_bounds__(kMoThreads) xe_mapmodify_tile_kernel(XeMapOp o, uint32_t tiles) {
  uint32_t cnt = 0;
  tile_walk(tiles, [&](uint32_t t, uint32_t lane) {
    uint32_t hit = 0;  // bit r: the slot of round r is selected
#pragma unroll
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const uint32_t s = tile_slot(t, r, lane);
      hit |= uint32_t(s < o.nslots && ms_select_item(o, s)) << r;
    }
#pragma unroll 1  // (one copy of the edit's code)
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const bool mine = (hit >> r) & 1;
      cnt += uint32_t(__popcll(__ballot(mine)));
      if (mine) mm_modify_item(o, o.sbase + tile_slot(t, r, lane), 0, 1, false);
    }
  });
  if ((threadIdx.x & 63) == 0 && cnt) mo_add32(o.ctr + kMoMatched, cnt);
}

// ---- join. JOIN_SELECT is SELECT with a probe behind the filter: the filter of the four rounds first (their
// loads are in flight together), then a candidate's lane builds its join key and probes the other table, one
// round after another (a probe is a dependent chain of loads: what overlaps it is the other waves of the CU).
// The probes diverge, lane by lane and in the number of groups they read; the ballots stand in a loop of their
// own behind them, where every lane of the wave arrives (the tile loop's bound is the same for the whole wave),
// and a lane whose slot lies past the table or is no candidate votes "not kept". The wave's candidates are
// counted once, after its last tile.
__global__ void __launch_bounds__(kMoThreads) xe_mapjoin_select_kernel(XeMapOp o, uint32_t tiles) {
  uint32_t cands = 0;
  tile_walk(tiles, [&](uint32_t t, uint32_t lane) {
    uint32_t hit = 0, kept = 0;  // bit r: the slot of round r is a candidate / is kept
#pragma unroll
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const uint32_t s = tile_slot(t, r, lane);
      hit |= uint32_t(s < o.nslots && ms_select_item(o, s)) << r;
    }
#pragma unroll 1  // (one copy of the probe's code)
    for (uint32_t r = 0; r < kMsRounds; r++)
      if (((hit >> r) & 1) && mj_kept_item(o, tile_slot(t, r, lane), find_slot)) kept |= 1u << r;
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t r = 0; r < kMsRounds; r++) {
      const unsigned long long b = __ballot((kept >> r) & 1);
      cands += uint32_t(__popcll(__ballot((hit >> r) & 1)));
      if (lane == 0) o.bitmap[uint64_t(t) * kMsRounds + r] = b;
      cnt += uint32_t(__popcll(b));
    }
    if (lane == 0) o.tile[t] = cnt;
  });
  if ((threadIdx.x & 63) == 0 && cands) mo_add32(o.ctr + kMjSelected, cands);
}

// JOIN_VALUE: one reported entry per LANES consecutive lanes, LANES by the OTHER map's value size. Every lane of
// a sub-group probes for the same key (the same addresses: one request) and moves its share of the value.
template <uint32_t LANES>
__global__ void __launch_bounds__(kMoThreads) xe_mapjoin_value_kernel(XeMapOp o, uint32_t) {
  const uint32_t sub = threadIdx.x % LANES, per = kMoThreads / LANES;
  const uint64_t stride = uint64_t(gridDim.x) * per;
  for (uint64_t j = uint64_t(blockIdx.x) * per + threadIdx.x / LANES; j < o.n; j += stride)
    mj_value_item(o, uint32_t(j), sub, LANES, find_slot);
}

// The steps: how each is launched, and its kernel. kLane / kValue: one batch entry per lane / per sub-group of
// xe_mo_lanes lanes (the kernel's second argument is the step; a value step's kernel is the instantiation for
// those lanes; kValueDst: the join's value kernel, the lanes by the other map's value size). kTileSrc /
// kTileDst: a wave per tile of the source's slots (the second argument is their number) / of the group's
// destination table, a HASH one (the step). kOneGroup: one workgroup, once the source has a tile. kSort: no kernel
// of this file's, the device radix sort over the n pairs.
enum MoShape : uint32_t { kNoShape = 0, kLane, kValue, kValueDst, kTileSrc, kTileDst, kOneGroup, kSort };
using MoKernel = void (*)(XeMapOp, uint32_t);
struct MoStep {
  MoShape shape;
  MoKernel kernel;
};
struct MoTable {
  MoStep row[XE_MO_STEPS];
};
constexpr MoTable mo_table() {
  MoTable t{};
  for (uint32_t s : {XE_MO_LOOKUP_FIND, XE_MO_UPDATE_LOCATE, XE_MO_UPDATE_UNDO, XE_MO_UPDATE_MARK, XE_MO_DELETE_FIND, XE_MO_DELETE_CLAIM,
                     XE_MO_MODIFY_MARK, XE_MO_LRU_TOUCH, XE_MO_LRU_CLAIM, XE_MO_LRU_ERASE, XE_MO_LRU_RANK})
    t.row[s] = {kLane, xe_mapop_lane_kernel};
  for (uint32_t s : {XE_MO_LOOKUP_VALUE, XE_MO_UPDATE_COPY, XE_MO_DELETE_ZERO, XE_MO_SCAN_COPY, XE_MO_SCAN_EXPIRE, XE_MO_MODIFY_EDIT,
                     XE_MO_MODIFY_KEYED})
    t.row[s] = {kValue, nullptr};
  t.row[XE_MO_SCAN_SELECT] = {kTileSrc, xe_mapscan_select_kernel};
  t.row[XE_MO_SCAN_SCAN] = {kOneGroup, xe_mapscan_scan_kernel};
  t.row[XE_MO_SCAN_SCATTER] = {kTileSrc, xe_mapscan_scatter_kernel};
  t.row[XE_MO_TOP_PREFIX] = {kTileSrc, xe_maptop_prefix_kernel};
  t.row[XE_MO_TOP_PICK] = {kOneGroup, xe_maptop_pick_kernel};
  t.row[XE_MO_TOP_CUT] = {kTileSrc, xe_maptop_cut_kernel};
  t.row[XE_MO_TOP_TRIM] = {kTileSrc, xe_maptop_trim_kernel};
  t.row[XE_MO_TOP_STATS] = {kTileSrc, xe_maptop_stats_kernel};
  t.row[XE_MO_GROUP_LOCATE] = {kTileSrc, xe_mapgroup_locate_kernel};
  t.row[XE_MO_GROUP_UNDO] = t.row[XE_MO_GROUP_PUBLISH] = {kTileDst, xe_mapgroup_dst_kernel};
  t.row[XE_MO_GROUP_ADD] = {kTileSrc, xe_mapgroup_add_kernel};
  t.row[XE_MO_COMPACT_MARK] = {kTileSrc, xe_mapcompact_mark_kernel};
  t.row[XE_MO_COMPACT_REBUILD] = {kTileSrc, xe_mapcompact_rebuild_kernel};
  t.row[XE_MO_MODIFY_TILE] = {kTileSrc, xe_mapmodify_tile_kernel};
  t.row[XE_MO_JOIN_SELECT] = {kTileSrc, xe_mapjoin_select_kernel};
  t.row[XE_MO_JOIN_VALUE] = {kValueDst, nullptr};
  t.row[XE_MO_LRU_SORT] = {kSort, nullptr};
  return t;
}
constexpr MoTable kMoSteps = mo_table();
constexpr bool mo_steps_filled() {
  for (const MoStep& r : kMoSteps.row)
    if (r.shape == kNoShape || (r.kernel == nullptr) != (r.shape == kValue || r.shape == kValueDst || r.shape == kSort)) return false;
  return true;
}
static_assert(sizeof kMoSteps.row / sizeof kMoSteps.row[0] == XE_MO_STEPS && mo_steps_filled(), "one filled row per step");
static_assert(kMsScanThreads == kMoThreads && kMtBins == kMoThreads, "every step's workgroup has kMoThreads threads");

// The grid of `want` workgroups' worth of work (the head of this file).
uint32_t mo_blocks(uint64_t want) {
  return uint32_t(want <= kMoOneTurn ? want : want / 4 < kMoOneTurn ? kMoOneTurn : want / 4 < kMoMaxBlocks ? want / 4 : kMoMaxBlocks);
}

// SORT: (l_keys, slot) -> (l_keys2, l_slot2) by rank key, ascending. The LSD radix sort is stable, so equal keys
// keep the slot order SCATTER left them in.
int mo_sort(const XeMapOp& o, hipStream_t s) {
  size_t tmp = o.l_tmp_bytes;
  return hipcub::DeviceRadixSort::SortPairs(o.l_tmp, tmp, (const unsigned long long*)o.l_keys, (unsigned long long*)o.l_keys2,
                                            (const uint32_t*)o.slot, o.l_slot2, int(o.n), 0, 64, s) == hipSuccess ? 0 : -1;
}

}  // namespace

extern "C" int xe_mapop_sort_bytes(uint32_t n, size_t* bytes) {
  size_t tmp = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                         (const uint32_t*)nullptr, (uint32_t*)nullptr, int(n), 0, 64, nullptr) != hipSuccess)
    return -1;
  *bytes = tmp ? tmp : 8;
  return 0;
}

extern "C" int xe_launch_mapop(const XeMapOp* op, uint32_t step, void* stream) {
  if (step >= XE_MO_STEPS) return -1;
  const MoShape shape = kMoSteps.row[step].shape;
  MoKernel kernel = kMoSteps.row[step].kernel;
  uint32_t blocks = 1, arg = step;
  if (shape == kSort) return op->n ? mo_sort(*op, hipStream_t(stream)) : 0;
  if (shape == kLane || shape == kValue || shape == kValueDst) {
    if (!op->n) return 0;
    const uint32_t lanes = shape == kValue ? xe_mo_lanes(op->value_size) : shape == kValueDst ? xe_mo_lanes(op->dst.value_size) : 1;
    const uint32_t per = kMoThreads / lanes;
    blocks = mo_blocks((uint64_t(op->n) + per - 1) / per);
    if (shape == kValue)
      kernel = lanes == 1 ? xe_mapop_value_kernel<1> : lanes == 4 ? xe_mapop_value_kernel<4> : lanes == 16 ? xe_mapop_value_kernel<16> : xe_mapop_value_kernel<64>;
    if (shape == kValueDst)
      kernel = lanes == 1 ? xe_mapjoin_value_kernel<1> : lanes == 4 ? xe_mapjoin_value_kernel<4> : lanes == 16 ? xe_mapjoin_value_kernel<16> : xe_mapjoin_value_kernel<64>;
  } else {
    if (shape == kTileDst && op->dst.kind != XE_DM_HASH) return 0;
    const uint32_t tiles = xe_ms_tiles(shape == kTileDst ? op->dst.cap : op->nslots);
    if (!tiles) return 0;
    if (shape != kOneGroup) blocks = mo_blocks((tiles + kMoThreads / 64 - 1) / (kMoThreads / 64));
    if (shape != kTileDst) arg = tiles;
  }
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kMoThreads), 0, hipStream_t(stream), *op, arg);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
