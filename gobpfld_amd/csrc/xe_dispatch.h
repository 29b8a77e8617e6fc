// Verdict dispatch (include/xdpemu_io.h, output side): what the kernels (xe_dispatch.hip), the API
// functions and the host-simulation loops (xe_io.cpp) share. Not part of the per-program kernel sources.
#ifndef XE_DISPATCH_H
#define XE_DISPATCH_H

#include "../../include/xdpemu_io.h"

#if defined(__HIPCC__)
#define XE_DSP_HD __host__ __device__
#else
#define XE_DSP_HD
#endif

// Rows of the per-tile count array in the scratch, row-major (row r, tile t at r * tiles + t): the five
// classes' rows, then two more that ride the same scan only for their totals (invalid, failed). A packet
// of rows 5 and 6 is also counted in row 0, so rows 0..4 sum to n.
constexpr uint32_t kDspRows = 7;
constexpr uint32_t kDspInvalid = 5, kDspFailed = 6, kDspNone = 7;

// The row of a packet: its class 0..4, or why it went to class 0.
XE_DSP_HD inline uint32_t xe_dsp_row(uint32_t verdict, uint32_t status) {
  return status != XE_ST_OK ? kDspFailed : verdict > 4 ? kDspInvalid : verdict;
}
XE_DSP_HD inline uint32_t xe_dsp_class(uint32_t row) { return row > 4 ? 0 : row; }

inline uint32_t xe_dsp_tiles(uint32_t n) { return uint32_t((uint64_t(n) + XE_DISPATCH_TILE - 1) / XE_DISPATCH_TILE); }
inline uint64_t xe_dsp_scratch(uint32_t n) { return (uint64_t(xe_dsp_tiles(n)) * kDspRows * 4 + 255) & ~uint64_t(255); }

// A gather packet is copied only when all of its source and destination bytes lie inside the buffers.
XE_DSP_HD inline bool xe_gather_ok(uint64_t addr, uint32_t len, uint64_t src_len, uint32_t frame_room, uint64_t frame,
                                   uint64_t dst_len) {
  return addr <= src_len && len <= src_len - addr && len <= frame_room && frame <= dst_len && len <= dst_len - frame;
}

#ifndef XE_HOSTSIM
extern "C" int xe_launch_dispatch(const void* desc, const void* verdicts, const void* results, uint32_t n, void* out_desc,
                                  void* out_index, void* counts, void* scratch, void* stream);
extern "C" int xe_launch_gather(const void* src, uint64_t src_len, const void* sorted_desc, const void* counts, uint32_t cls,
                                uint32_t max_count, const void* frames, uint32_t frame_room, void* dst, uint64_t dst_len,
                                void* out_desc, void* rejected, void* stream);
#endif
#endif  // XE_DISPATCH_H
