// Verdict dispatch on the device (include/xdpemu_io.h, output side): a stable partition of a batch's
// descriptors by XDP action in three launches (count, scan, scatter), and the gather of one class's
// packets into caller-chosen frames.
//
// No kernel here waits on another workgroup: the per-tile counts go through memory between launches, and
// the scatter re-reads the verdicts (4 B per packet) instead of looking back at its neighbours.
//
// Tile layout (count and scatter agree on it): a 256-thread workgroup takes XE_DISPATCH_TILE consecutive
// packets, wave w the kDspWaveSpan consecutive ones from w * kDspWaveSpan on, 64 at a time. Packet order
// is therefore (tile, wave, round, lane), and a packet's rank within its class is: the class's global
// base of the tile (scan) + the waves before it (LDS) + the rounds before it (a running wave-uniform
// count) + the lanes before it (ballot).
#include <hip/hip_runtime.h>

#include "xe_dispatch.h"

namespace {

constexpr uint32_t kDspThreads = 256, kDspWaves = kDspThreads / 64;
constexpr uint32_t kDspWaveSpan = XE_DISPATCH_TILE / kDspWaves, kDspRounds = kDspWaveSpan / 64;
static_assert(kDspRounds * 64 * kDspWaves == XE_DISPATCH_TILE, "a tile is a whole number of 64-packet rounds per wave");
constexpr uint32_t kScanThreads = 1024, kScanQ = 4, kScanPass = kScanThreads * 4 * kScanQ;

__device__ inline uint32_t lanes_before(unsigned long long b) {  // set bits of b below this lane
  return __builtin_amdgcn_mbcnt_hi(uint32_t(b >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(b), 0));
}

// The rows (xe_dsp_row) of this lane's kDspRounds packets; kDspNone past the end of the batch.
// Only the status byte of a 16-byte xe_result is read.
__device__ inline void load_rows(const uint32_t* __restrict__ ver, const uint8_t* __restrict__ res, uint32_t n,
                                 uint32_t first, uint32_t (&row)[kDspRounds]) {
  uint32_t v[kDspRounds], st[kDspRounds];
#pragma unroll
  for (uint32_t r = 0; r < kDspRounds; r++) {
    const uint32_t i = first + r * 64;  // first <= 2^32 - 64 * kDspRounds: no wrap
    const bool in = i < n;
    v[r] = in ? ver[i] : 0;
    st[r] = in && res ? res[uint64_t(i) * sizeof(xe_result)] : 0;
  }
#pragma unroll
  for (uint32_t r = 0; r < kDspRounds; r++) row[r] = first + r * 64 < n ? xe_dsp_row(v[r], st[r]) : kDspNone;
}

// The same for counting, where the order within the tile does not matter: thread t takes four consecutive
// packets from 4 t on in each quarter of the tile's kDspRounds / 4 spans of 1024, so that the verdicts
// come in as 16-byte loads (when the array is 16-byte aligned and the four lie inside the batch).
static_assert(kDspRounds % 4 == 0 && kDspThreads * kDspRounds == XE_DISPATCH_TILE, "the tile splits into 16-byte loads");
__device__ inline void load_rows_packed(const uint32_t* __restrict__ ver, const uint8_t* __restrict__ res, uint32_t n,
                                        uint32_t tile, uint32_t (&row)[kDspRounds]) {
  const bool vec = (uintptr_t(ver) & 15) == 0;
  uint32_t v[kDspRounds], st[kDspRounds];
#pragma unroll
  for (uint32_t q = 0; q < kDspRounds / 4; q++) {
    const uint32_t i = tile * XE_DISPATCH_TILE + q * (kDspThreads * 4) + threadIdx.x * 4;  // i + 3 <= 2^32 - 1: no wrap
    if (vec && i + 3 < n) {
      const uint4 x = *reinterpret_cast<const uint4*>(ver + i);
      v[q * 4] = x.x, v[q * 4 + 1] = x.y, v[q * 4 + 2] = x.z, v[q * 4 + 3] = x.w;
    } else {
#pragma unroll
      for (uint32_t j = 0; j < 4; j++) v[q * 4 + j] = i + j < n ? ver[i + j] : 0;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) st[q * 4 + j] = i + j < n && res ? res[uint64_t(i + j) * sizeof(xe_result)] : 0;
  }
#pragma unroll
  for (uint32_t q = 0; q < kDspRounds / 4; q++) {
    const uint32_t i = tile * XE_DISPATCH_TILE + q * (kDspThreads * 4) + threadIdx.x * 4;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) row[q * 4 + j] = i + j < n ? xe_dsp_row(v[q * 4 + j], st[q * 4 + j]) : kDspNone;
  }
}

__device__ inline uint32_t tile_first(uint32_t tile) {  // this lane's first packet
  return tile * XE_DISPATCH_TILE + (threadIdx.x >> 6) * kDspWaveSpan + (threadIdx.x & 63);
}

}  // namespace

// counts[row * tiles + tile] = packets of that row in the tile (row 0: the whole class 0).
extern "C" __global__ void __launch_bounds__(256) xe_dispatch_count_kernel(const uint32_t* __restrict__ ver,
                                                                           const uint8_t* __restrict__ res, uint32_t n,
                                                                           uint32_t tiles, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wcnt[kDspWaves][kDspRows];
  uint32_t row[kDspRounds];
  load_rows_packed(ver, res, n, blockIdx.x, row);
  uint32_t c[kDspRows] = {};
#pragma unroll
  for (uint32_t r = 0; r < kDspRounds; r++) {
#pragma unroll
    for (uint32_t k = 1; k < kDspRows; k++) c[k] += __popcll(__ballot(row[r] == k));
    c[0] += __popcll(__ballot(row[r] == 0 || row[r] == kDspInvalid || row[r] == kDspFailed));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (uint32_t k = 0; k < kDspRows; k++) wcnt[threadIdx.x >> 6][k] = c[k];
  }
  __syncthreads();
  if (threadIdx.x < kDspRows) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t w = 0; w < kDspWaves; w++) s += wcnt[w][threadIdx.x];
    counts[uint64_t(threadIdx.x) * tiles + blockIdx.x] = s;
  }
}

// In-place exclusive scan of a[0 .. total) by one workgroup, kScanPass elements per pass with a carry,
// so any total is handled. A pass is kScanQ quarters of 4096 elements; in each, thread t holds the four
// elements from 4 t on (one 16-byte load: a is 16-byte aligned), so a pass costs one load latency and one
// barrier pair for all quarters. The value in front of each row's first element is a segment bound of
// xe_dispatch_counts; rows 5 and 6 only give the invalid and failed totals (sums wrap mod 2^32 above
// n, the differences are exact).
extern "C" __global__ void __launch_bounds__(1024) xe_dispatch_scan_kernel(uint32_t* a, uint32_t tiles,
                                                                           xe_dispatch_counts* out) {
  constexpr uint32_t kWaves = kScanThreads / 64;
  __shared__ uint32_t wsum[kScanQ][kWaves];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint64_t total = uint64_t(tiles) * kDspRows;
  uint32_t carry = 0;
  for (uint64_t base = 0; base < total; base += kScanPass) {
    uint32_t x[kScanQ][4], sum[kScanQ], inc[kScanQ];
#pragma unroll
    for (uint32_t q = 0; q < kScanQ; q++) {
      const uint64_t at = base + q * (kScanThreads * 4) + t * 4;
      if (at + 3 < total) {
        const uint4 v = *reinterpret_cast<const uint4*>(a + at);
        x[q][0] = v.x, x[q][1] = v.y, x[q][2] = v.z, x[q][3] = v.w;
      } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) x[q][j] = at + j < total ? a[at + j] : 0;
      }
      sum[q] = inc[q] = x[q][0] + x[q][1] + x[q][2] + x[q][3];
    }
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {  // inclusive scans across the wave, the quarters side by side
#pragma unroll
      for (uint32_t q = 0; q < kScanQ; q++) {
        const uint32_t y = __shfl_up(inc[q], d, 64);
        if (lane >= d) inc[q] += y;
      }
    }
    if (lane == 63) {
#pragma unroll
      for (uint32_t q = 0; q < kScanQ; q++) wsum[q][w] = inc[q];
    }
    __syncthreads();
    uint32_t before = carry;  // the sum of everything in front of quarter q's wave w
#pragma unroll
    for (uint32_t q = 0; q < kScanQ; q++) {
      uint32_t mine = 0, all = 0;
#pragma unroll
      for (uint32_t k = 0; k < kWaves; k++) {
        const uint32_t s = wsum[q][k];
        mine += k < w ? s : 0;
        all += s;
      }
      const uint64_t at = base + q * (kScanThreads * 4) + t * 4;
      uint32_t e[4];
      e[0] = before + mine + inc[q] - sum[q];
#pragma unroll
      for (uint32_t j = 1; j < 4; j++) e[j] = e[j - 1] + x[q][j - 1];
      if (at + 3 < total) {
        *reinterpret_cast<uint4*>(a + at) = make_uint4(e[0], e[1], e[2], e[3]);
      } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
          if (at + j < total) a[at + j] = e[j];
      }
      before += all;
    }
    carry = before;
    __syncthreads();  // wsum is rewritten by the next pass; the stores to a are visible to the workgroup
  }
  // carry = the sum of everything, the same in every thread; a[row * tiles] = the sum in front of the row
  if (t < XE_ACT_COUNT + 1) out->offset[t] = a[uint64_t(t) * tiles];  // row 5 starts at n
  if (t == 6) out->invalid = a[uint64_t(kDspFailed) * tiles] - a[uint64_t(kDspInvalid) * tiles];
  if (t == 7) out->failed = carry - a[uint64_t(kDspFailed) * tiles];
}

// out_desc / out_index at (class base of the tile + rank within the tile) = packet i's descriptor / i.
extern "C" __global__ void __launch_bounds__(256) xe_dispatch_scatter_kernel(
    const uint4* __restrict__ desc, const uint32_t* __restrict__ ver, const uint8_t* __restrict__ res, uint32_t n,
    uint32_t tiles, const uint32_t* __restrict__ bases, uint4* __restrict__ out_desc, uint32_t* __restrict__ out_index) {
  __shared__ uint32_t wcnt[kDspWaves][XE_ACT_COUNT], tbase[XE_ACT_COUNT];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, first = tile_first(blockIdx.x);
  uint32_t cls[kDspRounds];
  load_rows(ver, res, n, first, cls);
  uint32_t c[XE_ACT_COUNT] = {};
#pragma unroll
  for (uint32_t r = 0; r < kDspRounds; r++) {
    if (cls[r] != kDspNone) cls[r] = xe_dsp_class(cls[r]);
#pragma unroll
    for (uint32_t k = 0; k < XE_ACT_COUNT; k++) c[k] += __popcll(__ballot(cls[r] == k));
  }
  if (lane == 0) {
#pragma unroll
    for (uint32_t k = 0; k < XE_ACT_COUNT; k++) wcnt[w][k] = c[k];
  }
  if (threadIdx.x < XE_ACT_COUNT) tbase[threadIdx.x] = bases[uint64_t(threadIdx.x) * tiles + blockIdx.x];
  __syncthreads();
  uint32_t at[XE_ACT_COUNT];  // wave-uniform: where this wave's next packet of each class goes
#pragma unroll
  for (uint32_t k = 0; k < XE_ACT_COUNT; k++) {
    at[k] = tbase[k];
    for (uint32_t v = 0; v < kDspWaves; v++) at[k] += v < w ? wcnt[v][k] : 0;
  }
#pragma unroll
  for (uint32_t r = 0; r < kDspRounds; r++) {
    const uint32_t i = first + r * 64;
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t k = 0; k < XE_ACT_COUNT; k++) {
      const unsigned long long b = __ballot(cls[r] == k);
      if (cls[r] == k) pos = at[k] + lanes_before(b);
      at[k] += __popcll(b);
    }
    // pos < n: the bases are an exclusive scan of counts that sum to n, the rank is below the class's count
    if (cls[r] != kDspNone && pos < n) {
      out_desc[pos] = desc[i];
      if (out_index) out_index[pos] = i;
    }
  }
}

// One group of LANES lanes per packet, 16 bytes per lane and step: 16 lanes (four packets per wave: a
// 1514-byte packet takes six steps of 256 bytes; a wave per packet would leave most lanes idle on short
// ones), or 4 lanes (sixteen packets per wave) when no packet can be longer than 256 bytes. A group's
// packets are a chain of dependent loads (descriptor, then bytes), so the next packet's descriptor and
// frame are loaded before the current one's bytes move.
template <uint32_t LANES>
__global__ void __launch_bounds__(256) xe_gather_kernel(
    const uint8_t* __restrict__ src, uint64_t src_len, const xe_desc* __restrict__ sorted, const xe_dispatch_counts* __restrict__ counts,
    uint32_t cls, uint32_t max_count, const uint64_t* __restrict__ frames, uint32_t frame_room, uint8_t* __restrict__ dst,
    uint64_t dst_len, xe_desc* __restrict__ out_desc, uint32_t* __restrict__ rejected) {
  const uint32_t lo = counts->offset[cls], hi = counts->offset[cls + 1], n = counts->offset[XE_ACT_COUNT];
  if (lo > hi || hi > n) return;  // not a record the dispatch wrote: select nothing
  const uint32_t cnt = hi - lo < max_count ? hi - lo : max_count;
  const uint32_t sub = threadIdx.x % LANES, groups = gridDim.x * (blockDim.x / LANES);
  uint64_t k = blockIdx.x * (blockDim.x / LANES) + threadIdx.x / LANES;
  if (k >= cnt) return;
  xe_desc d = sorted[lo + k];
  uint64_t f = frames[k];
  while (true) {
    const uint64_t k_next = k + groups;
    const bool more = k_next < cnt;
    xe_desc d_next = d;
    uint64_t f_next = f;
    if (more) {
      d_next = sorted[lo + k_next];
      f_next = frames[k_next];
    }
    const bool ok = xe_gather_ok(d.addr, d.len, src_len, frame_room, f, dst_len);
    if (sub == 0) {
      out_desc[k] = xe_desc{f, ok ? d.len : 0, 0};
      if (!ok) atomicAdd(rejected, 1u);
    }
    if (ok) {
      const uint8_t* s = src + d.addr;
      uint8_t* t = dst + f;
      const uint32_t len = d.len;
      if (((uintptr_t(s) ^ uintptr_t(t)) & 15) == 0) {  // co-aligned: bytes up to the 16-byte line, vectors, bytes
        uint32_t head = uint32_t(-uintptr_t(t)) & 15;
        head = head < len ? head : len;
        for (uint32_t j = sub; j < head; j += LANES) t[j] = s[j];
        const uint32_t vecs = (len - head) / 16;
        const uint4* sv = reinterpret_cast<const uint4*>(s + head);
        uint4* tv = reinterpret_cast<uint4*>(t + head);
        for (uint32_t j = sub; j < vecs; j += LANES) tv[j] = sv[j];
        for (uint32_t j = head + vecs * 16 + sub; j < len; j += LANES) t[j] = s[j];
      } else {
        for (uint32_t j = sub; j < len; j += LANES) t[j] = s[j];
      }
    }
    if (!more) break;
    k = k_next, d = d_next, f = f_next;
  }
}

namespace {
constexpr uint32_t kGatherShort = 256;  // frame_room up to this: the 4-lane gather (at most four steps per packet)
inline bool launched() { return hipGetLastError() == hipSuccess; }
}  // namespace

extern "C" int xe_launch_dispatch(const void* desc, const void* verdicts, const void* results, uint32_t n, void* out_desc,
                                  void* out_index, void* counts, void* scratch, void* stream) {
  hipStream_t s = hipStream_t(stream);
  if (!n) return hipMemsetAsync(counts, 0, sizeof(xe_dispatch_counts), s) == hipSuccess ? 0 : -1;
  const uint32_t tiles = xe_dsp_tiles(n);
  hipLaunchKernelGGL(xe_dispatch_count_kernel, dim3(tiles), dim3(kDspThreads), 0, s, (const uint32_t*)verdicts,
                     (const uint8_t*)results, n, tiles, (uint32_t*)scratch);
  if (!launched()) return -1;
  hipLaunchKernelGGL(xe_dispatch_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, (uint32_t*)scratch, tiles,
                     (xe_dispatch_counts*)counts);
  if (!launched()) return -1;
  hipLaunchKernelGGL(xe_dispatch_scatter_kernel, dim3(tiles), dim3(kDspThreads), 0, s, (const uint4*)desc,
                     (const uint32_t*)verdicts, (const uint8_t*)results, n, tiles, (const uint32_t*)scratch, (uint4*)out_desc,
                     (uint32_t*)out_index);
  return launched() ? 0 : -1;
}

extern "C" int xe_launch_gather(const void* src, uint64_t src_len, const void* sorted_desc, const void* counts, uint32_t cls,
                                uint32_t max_count, const void* frames, uint32_t frame_room, void* dst, uint64_t dst_len,
                                void* out_desc, void* rejected, void* stream) {
  hipStream_t s = hipStream_t(stream);
  if (hipMemsetAsync(rejected, 0, 4, s) != hipSuccess) return -1;
  if (!max_count) return 0;
  const uint32_t lanes = frame_room <= kGatherShort ? 4 : 16, per = kDspThreads / lanes, want = max_count / per + 1;
  const dim3 grid(want < 8192 ? want : 8192), block(kDspThreads);
  if (lanes == 4)
    hipLaunchKernelGGL(xe_gather_kernel<4>, grid, block, 0, s, (const uint8_t*)src, src_len, (const xe_desc*)sorted_desc,
                       (const xe_dispatch_counts*)counts, cls, max_count, (const uint64_t*)frames, frame_room, (uint8_t*)dst,
                       dst_len, (xe_desc*)out_desc, (uint32_t*)rejected);
  else
    hipLaunchKernelGGL(xe_gather_kernel<16>, grid, block, 0, s, (const uint8_t*)src, src_len, (const xe_desc*)sorted_desc,
                       (const xe_dispatch_counts*)counts, cls, max_count, (const uint64_t*)frames, frame_room, (uint8_t*)dst,
                       dst_len, (xe_desc*)out_desc, (uint32_t*)rejected);
  return launched() ? 0 : -1;
}
