/*
 * xdpemu_io.h — packet ingestion for the end-to-end path: capture files into
 * AF_XDP-shaped UMEM frames and 16-byte descriptors (the layout xe_run_batch_* consume).
 *
 * The reference's host input format is the AF_XDP UMEM of FrameCount x FrameSize bytes plus
 * `struct xdp_desc {u64 addr; u32 len; u32 options;}` descriptors (xsk.go:695-701, XSKSettings
 * xsk.go:720-757); its rx path hands the program a frame at `addr` (frame start + headroom). These
 * calls fill exactly that layout from a classic libpcap capture (magic 0xa1b2c3d4 microsecond or
 * 0xa1b23c4d nanosecond timestamps, either byte order) held in memory (e.g. an mmap of the file).
 * Host-only code: no device calls, usable without a GPU.
 */
#ifndef XDPEMU_IO_H
#define XDPEMU_IO_H

#include "xdpemu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XE_ERR_FORMAT (-103) /* not a classic pcap capture / truncated header */

typedef struct xe_pcap_info {
    uint32_t linktype;     /* LINKTYPE_* (1 = Ethernet, the only one an XDP program sees)   */
    uint32_t snaplen;
    uint32_t nanosecond;   /* 1: timestamps are ns, 0: us                                   */
    uint32_t swapped;      /* 1: the file was written big-endian                            */
    uint64_t first_record; /* byte offset of the first record header (24)                   */
} xe_pcap_info;

/* Validate the global header. Returns XE_OK or XE_ERR_FORMAT. */
int xe_pcap_header(const uint8_t* file, uint64_t file_len, xe_pcap_info* info);

/* Count the complete records from *offset on (a truncated final record is not counted); *bytes
 * receives the captured bytes of the counted records. Returns XE_OK. */
int xe_pcap_count(const uint8_t* file, uint64_t file_len, const xe_pcap_info* info, uint64_t offset,
                  uint64_t* records, uint64_t* bytes);

/* Copy up to `max` records, from *offset on, into UMEM frames: record k goes to the frame starting at
 * UMEM byte address frame_addr[k] (frame_addr NULL: the frames first_frame, first_frame + 1, ...
 * in order), its bytes at frame start + headroom, cut to frame_size - headroom.
 * desc[k] = {frame start + headroom, copied bytes, 0} (the rx descriptor the kernel would post);
 * orig_len[k] (optional) = the record's wire length, ts_ns[k] (optional) = its timestamp in ns.
 * *offset advances past the copied records; *filled = records copied. A truncated final record
 * stops the copy (it stays unread). Returns XE_OK, XE_ERR_INVAL (a frame outside the UMEM,
 * frame_size <= headroom). */
int xe_pcap_fill(const uint8_t* file, uint64_t file_len, const xe_pcap_info* info, uint64_t* offset,
                 uint8_t* umem, uint64_t umem_len, uint32_t frame_size, uint32_t headroom,
                 const uint64_t* frame_addr, uint64_t first_frame, uint32_t max, xe_desc* desc,
                 uint32_t* orig_len, uint64_t* ts_ns, uint32_t* filled);

/* Staging form for the device path: copy up to `max` records, from *offset on, back to back into
 * buf, each starting at a multiple of `align` (a power of two, >= 16), cut to `max_len` bytes
 * (0: no cut); desc[k] = {offset in buf, copied bytes, 0}. Only the packet bytes cross PCIe, not
 * whole frames. Stops before a record that does not fit in buf_len. *used = bytes of buf used.
 * Same offset / filled / orig_len / ts_ns contract as xe_pcap_fill. */
int xe_pcap_pack(const uint8_t* file, uint64_t file_len, const xe_pcap_info* info, uint64_t* offset,
                 uint8_t* buf, uint64_t buf_len, uint32_t align, uint32_t max_len, uint32_t max,
                 xe_desc* desc, uint32_t* orig_len, uint64_t* ts_ns, uint32_t* filled, uint64_t* used);

/*
 * Output side: device-side verdict dispatch. A batch leaves xe_run_batch_device as one uint32 verdict
 * per packet; an AF_XDP forwarder works with lists: frames to recycle to the fill ring (drop,
 * aborted), descriptors to post on the tx ring (tx), descriptors to hand up (pass, redirect). These
 * calls build the lists on the device: a stable partition of the batch's descriptors by XDP action
 * with its counts, and a gather of one action's packets into frames the caller chose. Both are
 * stream-ordered and stateless (no xe_vm); every pointer named d_* is a device address (a host
 * address in the host-simulation build).
 */
#define XE_ACT_ABORTED 0  /* also: verdict > 4, and (when results are given) status != XE_ST_OK */
#define XE_ACT_DROP 1
#define XE_ACT_PASS 2
#define XE_ACT_TX 3
#define XE_ACT_REDIRECT 4
#define XE_ACT_COUNT 5
#define XE_DISPATCH_TILE 2048 /* packets per workgroup tile of the kernels; tests size their cases by it */

typedef struct xe_dispatch_counts { /* 32 bytes, written on the device */
    uint32_t offset[6]; /* class c occupies out[offset[c] .. offset[c+1]); offset[5] == n */
    uint32_t invalid;   /* status OK (or no results given) and verdict > 4: sent to class 0 */
    uint32_t failed;    /* status != XE_ST_OK: sent to class 0 (0 when d_results is NULL) */
} xe_dispatch_counts;

/* Workspace, in bytes, that the dispatch call below needs for a batch of n packets (0 for n == 0). */
int xe_dispatch_scratch_bytes(uint32_t n, uint64_t* bytes);

/* Stable partition of a batch by action. Packet i belongs to class verdicts[i] if that is <= 4, else
 * to class 0; when d_results (n xe_result) is given and results[i].status != XE_ST_OK it belongs to
 * class 0 whatever the verdict holds. d_out_desc (n xe_desc) receives the input descriptors ordered
 * by class and, within a class, in packet order (a ring must keep a flow's order); d_out_index
 * (n uint32, may be NULL) the packet index of each output slot; d_counts one xe_dispatch_counts.
 * d_scratch / scratch_bytes: at least what the query above reports for n.
 * Verdicts are final once xe_run_batch_device has returned or, for a pipelined batch, once its stats
 * are filled and its mode is not XE_MODE_CANCELLED: a replay at xe_sync rewrites the verdicts, so a
 * dispatch enqueued behind a pipelined batch that is later replayed has partitioned stale values.
 * n == 0 launches nothing, writes zero counts and needs only d_counts.
 * Returns XE_OK, XE_ERR_INVAL (a required pointer NULL; d_desc, d_out_desc or d_scratch not 16-byte
 * aligned, a uint32 array not 4-byte aligned; scratch_bytes too small; d_out_desc overlapping d_desc),
 * XE_ERR_DEVICE (a launch failed). */
int xe_dispatch_device(const void* d_desc, const void* d_verdicts, const void* d_results, uint32_t n,
                       void* d_out_desc, void* d_out_index, void* d_counts, void* d_scratch,
                       uint64_t scratch_bytes, void* stream);

/* Copy one class's packets into caller-chosen frames: the device form of a tx-ring post, and the way
 * to collect bounced packets into a dense region that one contiguous copy brings back. The class's
 * segment bounds are read on the device from d_counts (as the dispatch wrote it; no host round trip
 * in between). For k < min(offset[cls + 1] - offset[cls], max_count): d = sorted_desc[offset[cls] + k];
 * d.len bytes go from d_src + d.addr to d_dst + frames[k]; out_desc[k] = {frames[k], d.len, 0}.
 * A packet is not copied, out_desc[k] = {frames[k], 0, 0} and *d_rejected (one uint32, zeroed by the
 * call) counts it, when d.addr + d.len exceeds src_len (checked without wraparound), d.len exceeds
 * frame_room, or frames[k] + d.len exceeds dst_len. Bounds that do not satisfy
 * offset[cls] <= offset[cls + 1] <= offset[5] select nothing. d_frames (uint64) and d_out_desc hold
 * min(segment, max_count) entries. The caller keeps the source ranges, the destination ranges and
 * the frames of different packets from overlapping one another.
 * Returns XE_OK, XE_ERR_INVAL (a required pointer NULL or misaligned as above, cls >= XE_ACT_COUNT),
 * XE_ERR_DEVICE. */
int xe_gather_device(const void* d_src, uint64_t src_len, const void* d_sorted_desc, const void* d_counts,
                     uint32_t cls, uint32_t max_count, const void* d_frames, uint32_t frame_room,
                     void* d_dst, uint64_t dst_len, void* d_out_desc, void* d_rejected, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XDPEMU_IO_H */
