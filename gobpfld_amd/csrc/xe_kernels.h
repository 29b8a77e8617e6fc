// xe_kernels.h — the C-linkage seams between the translation units of the library, each declared once:
// the launchers of xe_kernel.hip, the kernel generator and loader of xe_jit.cpp, and the hooks
// xe_multi.cpp calls into the runtime. The defining unit and every caller include this header, so a
// signature that drifts between definition and use fails to compile. Not part of include/xdpemu.h.
#ifndef XE_KERNELS_H_
#define XE_KERNELS_H_

#include "xe_internal.h"

#ifndef XE_HOSTSIM
#include <hip/hip_runtime_api.h>
#endif

extern "C" {

// the kernel generator (xe_jit.cpp; in the host simulation too: sources only, no compiles)
int xe_jit_may_write_entries(const XeUop* prog, size_t n);
size_t xe_jit_source_for(const XeUop* const* progs, const uint32_t* lens, uint32_t nprogs, int32_t entry,
                         const XeDevMap* maps, uint32_t nmaps, int variant, char* buf, size_t buflen);

#ifndef XE_HOSTSIM
// per-program kernels (xe_jit.cpp)
void* xe_jit_get(const XeUop* const* progs, const uint32_t* lens, uint32_t nprogs, int32_t entry, int device,
                 const XeDevMap* maps, uint32_t nmaps, bool* cyclic, bool* general, const char** err, int variant,
                 uint64_t* maxpath);
int xe_jit_launch(void* fn, const XeParams* P, uint32_t blocks, uint32_t threads, hipStream_t s);
int xe_jit_occupancy(void* fn, uint32_t nmaps);

// xe_kernel.hip
int xe_launch_interp(const XeParams* P, uint32_t blocks, uint32_t threads, hipStream_t s);
int xe_interp_occupancy(uint32_t nmaps);
int xe_launch_delta(const void* cur, const void* snap, void* out, uint64_t bytes, uint32_t lane, hipStream_t s);
int xe_launch_apply_delta(void* cur, const void* snap, const void* delta, uint64_t bytes, uint32_t lane, hipStream_t s);
int xe_launch_delta_sum(void* acc, const void* in, uint64_t bytes, uint32_t lane, hipStream_t s);
int xe_launch_rep_fold(void* vals, void* rep, uint64_t stride_words, uint32_t nrep, uint64_t nwords, const void* recs,
                       uint32_t rwords, uint32_t vsize, uint32_t cap, const void* lim, hipStream_t s);
int xe_launch_prologue(const void* const* src, void* const* dst, const uint64_t* words, uint32_t nseg, void* zero,
                       uint64_t zero_words, hipStream_t s);
int xe_launch_tail(const XeTailArgs* A, hipStream_t s);
int xe_launch_desc_overlap(const void* desc, uint32_t n, uint64_t umem_len, void* scratch, size_t* scratch_bytes,
                           uint32_t* flag, hipStream_t s);
int xe_launch_keyed(const XeKeyed* K, const XeDevMap* maps, uint8_t* skip, uint32_t step, uint32_t items, hipStream_t s);
int xe_launch_keyed_sort(const XeKeyed* K, uint32_t n, uint32_t end_bit, void* scratch, size_t* bytes, hipStream_t s);
int xe_launch_keyed_esort(const XeKeyed* K, void* scratch, size_t* bytes, hipStream_t s);
int xe_launch_keyed_scan(const XeKeyed* K, uint32_t n, void* scratch, size_t* bytes, hipStream_t s);
int xe_launch_append(const XeAppendArgs* A, uint32_t end_bit, void* scratch, size_t* bytes, hipStream_t s);
int xe_launch_pop(const uint32_t* src, uint32_t* dst, uint32_t n, uint32_t mode, uint32_t arg, XePopSlots sl, uint32_t* flag,
                  hipStream_t s);
int xe_launch_lru_relink(uint64_t* tag, uint32_t pool, uint32_t cnt, uint32_t* link, uint64_t* hdr, void* scratch,
                         size_t* bytes, int renumber, hipStream_t s);
int xe_launch_lru_tag_fold(uint64_t* tag, uint64_t* rep, uint32_t pool, uint32_t r, const uint64_t* hdr, hipStream_t s);
int xe_launch_lru_log(const uint64_t* tag, uint32_t pool, const uint32_t* order, const uint64_t* hdr, uint64_t* log,
                      hipStream_t s);
#endif

// hooks for xe_multi.cpp (defined in xe_runtime.cpp)
int xe_internal_vm_device(const xe_vm* vm);
void* xe_internal_vm_stream(xe_vm* vm);
int xe_internal_nmaps(const xe_vm* vm);
int xe_internal_may_write_packet(const xe_vm* vm);
int xe_internal_delta_sum(xe_vm* vm, void* acc, const void* in, uint64_t bytes, uint32_t lane);
int xe_internal_alloc(xe_vm* vm, void** p, uint64_t bytes);
void xe_internal_free(xe_vm* vm, void* p);
int xe_internal_copy(xe_vm* vm, void* dst, const void* src, uint64_t bytes);

}  // extern "C"

#endif  // XE_KERNELS_H_
