// Device-resident batched map operations (include/xdpemu.h: xe_map_lookup_batch_device,
// xe_map_update_batch_device, xe_map_delete_batch_device, xe_map_scan_device, xe_map_expire_device,
// xe_map_top_device, xe_map_evict_device, xe_map_stats, xe_map_group, xe_map_compact, xe_map_modify_device,
// xe_map_modify_batch_device, xe_map_join_device; xe_lru_lookup_batch_device, xe_lru_delete_batch_device,
// xe_lru_order_device, xe_lru_evict_device): the per-key and per-slot decision logic that the kernels
// (xe_mapops.hip) and the host simulation (the loops at the end of this file) share, and the launch
// declaration. ARRAY and HASH maps; LRU_HASH maps through the xe_lru_* calls only. Not part of the per-program
// kernel sources.
//
// A batch is a sequence of steps, one launch each (a step's writes are the next step's reads: the
// phases are kernel boundaries, no workgroup waits on another):
//
//   lookup   FIND    one key per lane: probe (read-only), found[i], slot[i]; values of up to
//                    kMoInline bytes are written by the same lane
//            VALUE   larger values: a sub-group of lanes copies value i (or zero-fills it)
//   update   LOCATE  one key per lane: the key's record, or a record claimed for it. A claim is one CAS
//                    on the record's word 0 that also names the claiming batch entry (BUSY | (i+1) << 32),
//                    so a repetition of the key that meets the claim compares its key with batch entry
//                    i's — input bytes, complete before the launch — and never waits for the claimer.
//                    The claims are counted: the distinct absent keys of the batch.
//            UNDO    (the batch does not fit, or an ARRAY index is out of range) every claim is put back:
//                    the table is bit for bit what it was
//            MARK    the claimer writes the key words; every entry raises the record's "last writer"
//                    word to its batch index + 1 (atomic max): the last repetition wins, decided here,
//                    before any value byte moves
//            COPY    a sub-group per entry; the winner copies its value into the map and into the delta
//                    base, then publishes the record as FULL (clearing VLEN0 and the last-writer word)
//   delete   FIND    as the lookup's (found[i] is "present before the call" for every repetition)
//            CLAIM   one CAS FULL -> TOMB | (i+1) << 32 per present key: one entry per distinct key wins
//            ZERO    the winner's sub-group zeroes the value (map and delta base), the record becomes a
//                    plain tombstone and the count drops
//   scan /   SELECT  one slot per lane over tiles of kMsTile consecutive slots (HASH: table slots; ARRAY:
//   expire           indices), one wave per tile in kMsRounds rounds: a FULL record's field is assembled from
//                    its value bytes and the filter evaluated, once; one 64-bit ballot per round goes to a
//                    bitmap, one match count per tile to the tile counts
//            SCAN    one workgroup turns the tile counts into their exclusive sums, kMsScanPass counts a
//                    pass with a carry; the total lands in the counters (kMoMatched) and the host reads it
//            SCATTER reads the bitmap and the tile bases only: a set bit's rank is its tile's base + the
//                    bits of the rounds before + the bits of the lanes before; rank < r: slot[rank] = slot.
//                    Ascending slot order, a function of the map's state alone
//            COPY    a sub-group per selected entry: its key (HASH: the record's key words; ARRAY: the
//                    index) and its value (zeros under VLEN0) to entry j of the outputs
//            EXPIRE  (expire only, after COPY) the same sub-groups leave their records as DELETE ZERO
//                    leaves one: value zeroed in the map and the delta base, a plain tombstone with its
//                    key words kept; the count drops by r
//   top /    PREFIX  the SELECT shape, one pass per byte of the order field, most significant first: a lane
//   evict            evaluates the filter and reads the order field once; the rank key is the field, or its
//                    complement within the width when the largest ranks first, so the smallest key always
//                    ranks first. Keys that share the prefix fixed so far add to a 256-bin histogram of
//                    their next byte (LDS per workgroup, one atomic per non-empty bin to the global bins)
//            PICK    one workgroup: the bin in which the number still needed runs out is the next prefix
//                    byte, the bins in front of it lower that number, the bins are cleared. Pass 0's bins sum
//                    to the eligible entries (kMtMatched); the number needed starts as min(k, that). The
//                    state lives in the counters: no host readback between the passes
//            CUT     one more tile pass, two bitmaps with a count per tile each: key < cut ("beyond") and
//                    key == cut ("equal"); nothing at all when nothing is needed
//            SCAN    (the scan's, over the equal counts)
//            TRIM    an equal bit's rank among the equals is its tile's base + the bits of the rounds before
//                    + the bits of the lanes before, SCATTER's arithmetic; rank < the number still needed:
//                    the bit joins the first bitmap and its tile's count. Ties are so taken in slot order
//            SCAN, SCATTER, COPY, EXPIRE   unchanged: the first bitmap now holds exactly the r selected
//   stats    STATS   one tile pass: count, sum, min and max of the field per lane, reduced across the wave and
//                    the workgroup, one 64-bit atomic each per workgroup (integers: the order of arrival
//                    does not matter)
//   group    SELECT, SCAN   (the scan's, on the source: the bitmap, matched)
//            LOCATE  a tile pass over the source bitmap: a selected slot assembles its group key (some bytes of
//                    its key or value, zero-padded as mo_load_key pads a key) and finds or claims the
//                    destination record with update LOCATE's protocol; the claim names the claiming SOURCE
//                    slot (BUSY | (slot + 1) << 32), so a lane that meets a claim compares its group key with
//                    that slot's — the source is only read during the call — and never waits. A FULL
//                    nil-backed (VLEN0) record of the group is claimed too, so that it can be zeroed. Claims
//                    of free and tombstone records are counted (kMoNew). No per-entry scratch: the later
//                    passes probe again
//            UNDO    (the groups do not fit, or an ARRAY index is out of range) a tile pass over the
//                    destination table: every BUSY record is what it was
//            PUBLISH a tile pass over the destination table: a BUSY record gets its key words (rebuilt from
//                    the source slot it names; a tombstone holds them), a zero value in the map and the delta
//                    base, and becomes plain FULL; the count rises by the counted claims
//            ADD     a tile pass over the source bitmap again: a read-only probe (every record is FULL now),
//                    then 64-bit atomic adds of the count and the measure into the map and the delta base.
//                    The kernel combines the lanes of a wave that share a destination slot first, for up to
//                    kMgLeaders distinct slots a round
//   compact  MARK    the SELECT shape over the table's slots, word 0 of each record only: one ballot a round into
//                    the first bitmap with the bit "free" (neither FULL nor a tombstone; the bits of slots past
//                    the table are "not free"), one into the second with the bit "tombstone"; the tile counts
//                    are the tombstones, the free records are counted in the counters (kMcFree)
//            SCAN    (the scan's: the tombstones of the table, kMoMatched)
//            REBUILD a tile pass: a run is a maximal sequence of consecutive non-free slots modulo cap; linear
//                    probing never carries an entry across a free record, so every entry's home lies in its run
//                    and the runs are independent. The lane whose slot is not free while its predecessor is (slot
//                    0's is slot cap - 1) takes the run: its end and its first tombstone come from the two
//                    bitmaps by word operations, no record of a clean run is read. A run with a tombstone is
//                    rebuilt in place, front to back: the entry at run offset j probes from its home offset over
//                    the records that are FULL now and stops at the first that is not, or at j; a target q < j
//                    takes the record (VLEN0 kept, the high half zero) and the value (map and delta base), and
//                    slot j is zeroed; a tombstone is zeroed, key words and values included. (home <= q <= j, and
//                    the slots in front of j already hold the new layout: each of them was filled by an entry
//                    that came earlier in run order, exactly the records an insertion in run order would have
//                    met.) No atomics on the table: a run's writes stay inside it. A run with a tombstone that
//                    is longer than kMcMaxRun is left alone and flagged (kMcLong): the runtime then compacts
//                    through the host. The longest run with a tombstone is an atomic max; with c_only the pass
//                    only measures
//   modify   TILE    (the silent, uncapped walk of values up to kMmTileMax bytes: every match is edited and none
//                    reported) one tile pass in the SELECT shape: a lane evaluates the filter on its slot and
//                    edits the value where it lies: a nil-backed (VLEN0) value is zeroed first, the edits run in
//                    list order on the value as it stands, the whole value goes to the delta base and the
//                    record becomes plain FULL. The matches are counted by ballot (kMoMatched). No bitmap, no
//                    SCAN, no SCATTER, no per-entry scratch
//            SELECT, SCAN, SCATTER, COPY   (the general walk: the scan's; COPY reports the values from before)
//            EDIT    a sub-group per reported entry j < r over slot[j]: TILE's edit of one slot, the value shared
//                    by the sub-group's lanes (mm_modify_item says what orders their stores)
//   modify   FIND    the lookup's FIND and VALUE when the old values are wanted, the delete's FIND otherwise:
//   (keyed)          found[i], slot[i] and the values from before, complete before any edit
//            MARK    every present entry raises its slot's last-writer word to i + 1 (update MARK's atomic max):
//                    one of a key's repetitions is named, decided before any value byte moves
//            KEYED   a sub-group per entry; the one whose i + 1 is still there edits the slot as EDIT does and
//                    clears the word: each distinct present key is edited exactly once
//   join     SELECT  (JOIN_SELECT, in place of the scan's) the SELECT shape over the source's slots: a lane evaluates
//                    the filter on its slot, the four rounds' loads in flight together; a candidate then assembles
//                    its join key (the group's rule: some bytes of its key or value) and probes the other map
//                    read-only (an ARRAY: the index against max_entries). The bit that goes to the bitmap and the
//                    tile counts is "kept": present under mode 0, absent under mode 1. The probes diverge, the
//                    ballots stand behind them where the wave is whole again. The candidates are counted once per
//                    wave (kMjSelected). Nothing per entry is written: one bit
//            SCAN, SCATTER, COPY   (the scan's: matched, slot[j], the kept entries' keys and values)
//            VALUE   (JOIN_VALUE, when the other map's values are wanted) a sub-group per reported entry j < r, as
//                    wide as the OTHER map's value asks: the join key is rebuilt from slot[j] and probed again (no
//                    per-entry scratch beyond slot), the value found (zeros when nil-backed, and always under mode
//                    1) goes to entry j of the third output. Behind COPY and in front of EXPIRE: a join of a map
//                    with itself reads everything before anything is removed
//            EXPIRE  (the scan's, under XE_MJ_REMOVE)
//   lru      FIND, VALUE   the lookup's, over an LRU view (below): the probe is mo_find unchanged, the value of a
//   lookup           slot is the pool value its record names, nil-backed when that value's length is 0
//            TOUCH   (without XE_LRU_PEEK) one key per lane: a found entry raises its value's stamp to
//                    epoch << 48 | (i + 1) (a 64-bit atomic max), the epoch a fresh one as every batch run takes:
//                    above every stamp in the map, and the last repetition of a key wins by construction. The
//                    links are not touched: the runtime marks them stale and lru_relink rebuilds them from the
//                    stamps when a replay or a host read asks
//   lru      FIND    the delete's
//   delete   CLAIM   one CAS on word 0 from FULL | vid << 32 to TOMB | vid << 32 per present key (the high half
//                    holds the value id and cannot name the claimer): the entry that wins marks itself in its own
//                    slot[i] (kMoFresh); the winners are counted (kMoGone)
//            ERASE   a winner leaves its entry as xe_interp.h lru_erase leaves one: stamp 0 (out of the usage
//                    order), the record a plain tombstone with its key words kept; the header's count drops by the
//                    winners once. The value bytes and the value's length stay as they are, as lru_erase leaves
//                    them: nothing reads the pool entry of a value whose stamp is 0 and which no record names
//                    (ordered_download walks the links, which lru_relink builds from the non-zero stamps), and
//                    whoever hands the id out again (lru_insert) sets its length and writes its value first
//   lru      PREFIX, PICK, CUT, SCAN, TRIM, SCAN, SCATTER   (the top's) over the table's slots and the nil key's
//   order /          record behind them. The eligible entries are the FULL records with a non-zero stamp whose
//   evict            value passes the filter; the rank key is the stamp (width 8), complemented when the most
//                    recent ranks first. Equal stamps are taken in slot order (TRIM)
//            RANK    entry j < r: the rank key of slot[j] into the sort's keys
//            SORT    the r (rank key, slot) pairs by rank key, ascending and stable (SCATTER left them in slot
//                    order, so equal stamps stay in slot order): the device radix sort the library links for
//                    lru_relink; a std::stable_sort in the host simulation. COPY then reports in rank order
//            COPY    (the scan's; the nil key's record reports key_size zero bytes)
//            ERASE   (evict only) the delete's, every one of the r entries a winner
//
// The last-writer word is the high half of a HASH record's word 0 (a HASH map keeps nothing there;
// an LRU record keeps its value id there, and the calls that mark are not served for LRU maps) and, for an ARRAY map, a word per
// index in a buffer of the map's own that is zero between calls. Both are zero again when a call returns.
//
// A deleted record keeps its key words. A tombstone holding key words is what the keyed path calls a
// reservation for that key (xe_interp.h hash_reserve / hash_claim): a later insert of the same key, by a
// keyed batch or by LOCATE, takes that record again, so a flow that is expired and learned again and again
// keeps using one record instead of a fresh one each time; its value bytes are zero, as a reservation's are.
// Clearing the words would turn every deleted record into a reservation for the all-zero key instead.
// Tombstones of keys that never come back stay until xe_map_compact removes them on the device (MARK, REBUILD)
// or the map next visits the host (drop_tombstones: the same layout for every run that does not wrap the
// table's end); when they have used up a probe chain's free records LOCATE says so (kMoErrFull) and the
// runtime compacts the table through the host once.
#ifndef XE_MAPOPS_H
#define XE_MAPOPS_H

#include "xe_internal.h"

enum : uint32_t {
  XE_MO_LOOKUP_FIND = 0, XE_MO_LOOKUP_VALUE,
  XE_MO_UPDATE_LOCATE, XE_MO_UPDATE_UNDO, XE_MO_UPDATE_MARK, XE_MO_UPDATE_COPY,
  XE_MO_DELETE_FIND, XE_MO_DELETE_CLAIM, XE_MO_DELETE_ZERO,
  XE_MO_SCAN_SELECT, XE_MO_SCAN_SCAN, XE_MO_SCAN_SCATTER, XE_MO_SCAN_COPY, XE_MO_SCAN_EXPIRE,
  XE_MO_TOP_PREFIX, XE_MO_TOP_PICK, XE_MO_TOP_CUT, XE_MO_TOP_TRIM, XE_MO_TOP_STATS,
  XE_MO_GROUP_LOCATE, XE_MO_GROUP_UNDO, XE_MO_GROUP_PUBLISH, XE_MO_GROUP_ADD,
  XE_MO_COMPACT_MARK, XE_MO_COMPACT_REBUILD,
  XE_MO_MODIFY_TILE, XE_MO_MODIFY_EDIT, XE_MO_MODIFY_MARK, XE_MO_MODIFY_KEYED,
  XE_MO_JOIN_SELECT, XE_MO_JOIN_VALUE,
  XE_MO_LRU_TOUCH, XE_MO_LRU_CLAIM, XE_MO_LRU_ERASE, XE_MO_LRU_RANK, XE_MO_LRU_SORT,
  XE_MO_STEPS
};

constexpr uint32_t kMoInline = 16;           // values up to this many bytes move on their key's lane
constexpr uint32_t kMoFresh = 0x80000000u;   // slot[i]: this entry claimed the record (update, LRU delete)
constexpr uint32_t kMoVlen0 = 0x40000000u;   // slot[i]: the record's value reads as zeros (lookup)
constexpr uint32_t kMoSlotMask = 0x3fffffffu;  // (cap <= 2^27, ARRAY indices are checked against it)
constexpr uint32_t kMoAbsent = kMoSlotMask;
// counters of a batch (u32 words of the scratch)
constexpr uint32_t kMoNew = 0, kMoErr = 1, kMoGone = 2, kMoMatched = 3, kMoCounters = 16;
// top / evict: the eligible entries, the number still needed, the rank-key prefix fixed so far (two words);
// stats: four 64-bit words (count, sum, ~min, max) from word kMtStats on
constexpr uint32_t kMtMatched = 4, kMtNeed = 5, kMtPrefix = 6, kMtStats = 8, kMtBins = 256;
constexpr uint32_t kMoErrRange = 1, kMoErrFull = 2;  // an ARRAY index out of range; no free record in the table
// scan / expire: a tile is kMsTile consecutive slots, one wave's work in kMsRounds rounds of 64; the SCAN
// step sums kMsScanPass tile counts a pass (262,144 slots: a table of 2^20 slots takes four passes)
constexpr uint32_t kMsRounds = 4, kMsTile = 64 * kMsRounds, kMsScanThreads = 256, kMsScanPass = kMsScanThreads * 4;
// group: GROUP_ADD combines the lanes of a wave that share a destination slot for this many distinct slots a
// round (the first remaining lane leads each time), the lanes left over add singly. 0: every lane adds singly
// (a -D of the tuning build, for the profile's comparison)
#ifndef XE_MG_LEADERS
#define XE_MG_LEADERS 4
#endif
constexpr uint32_t kMgLeaders = XE_MG_LEADERS, kMgNone = 0xffffffffu;
// compact: the free records, the entries moved, the longest run with a tombstone, "a run with a tombstone is
// longer than kMcMaxRun" (counters); kMcMaxRun bounds the records one lane walks alone (DESIGN.md has the walk's
// measured time); kMcDead: the record at a run offset is no entry
constexpr uint32_t kMcFree = 4, kMcMoved = 5, kMcLongest = 6, kMcLong = 7, kMcMaxRun = 4096, kMcDead = 0xffffffffu;
// modify: the edit's ops (include/xdpemu.h XE_MM_*); the silent uncapped walk edits values of up to kMmTileMax
// bytes on their slot's lane (MODIFY_TILE), larger ones go the general way where a sub-group shares a value
enum : uint32_t { kMmSet = 0, kMmAdd, kMmSub, kMmAddSat, kMmSubSat, kMmAnd, kMmOr, kMmXor, kMmMin, kMmMax, kMmShr, kMmOps };
constexpr uint32_t kMmTileMax = 64;
// join: the candidates (the entries the filter selects, kept or not), a counter word
constexpr uint32_t kMjSelected = 4;
static_assert(kMmTileMax >= kMoInline, "the single pass serves at least the values that move on one lane");
// the filter's ops (include/xdpemu.h XE_MF_*)
enum : uint32_t { kMfAll = 0, kMfEq, kMfNe, kMfLt, kMfLe, kMfGt, kMfGe, kMfAnyBits, kMfNoBits, kMfOps };

// One table: what a probe reads. A call's source map is the XeMapOp itself, the group's destination its `dst`.
// An LRU view (kind XE_DM_LRU): recs, cap and rwords as for HASH (word 0 of a FULL record: XE_SLOT_FULL | value id
// << 32; the nil key's record sits at slot cap); vals is the value pool, indexed by value id.
struct XeMapView {
  uint32_t kind;  // XE_DM_ARRAY / XE_DM_HASH / XE_DM_LRU
  uint32_t key_size, value_size, max_entries, cap, kwords, rwords;
  uint64_t* recs;         // HASH, LRU: slot records
  uint8_t* vals;
  uint8_t* snap;          // the delta base (HostMap::d_snap): kept equal to vals on the slots a call writes
  uint32_t* count;        // HASH: entry count
  // LRU
  uint32_t pool_cap;      // value ids are below it
  uint32_t* elen;         // [pool_cap] a value's length: 0 is a nil backing
  uint64_t* tag;          // [pool_cap] a value's stamp (xe_interp.h lru_stamp): 0 is "not in the usage order"
  uint64_t* hdr;          // the map's header words (word 2: the entry count)
};
struct XeMapOp : XeMapView {
  uint32_t n;             // batch entries
  uint32_t* win;          // ARRAY: last-writer word per index
  const uint8_t* keys;    // n x key_size (ARRAY: n x 4)
  const uint8_t* values_in;
  uint8_t* values_out;
  uint8_t* found;         // may be null
  uint32_t* slot;         // [n] scratch
  uint32_t* ctr;          // [kMoCounters] scratch, zero at the batch's start
  // scan / expire (n is then r, the entries reported)
  uint32_t f_op, f_off, f_width;  // the filter: kMf*, the field's byte offset in the value and its width
  uint32_t nslots, sbase;         // the slots looked at: sbase .. sbase + nslots (the empty key: the record past the table)
  uint64_t f_operand;
  uint64_t* bitmap;       // [tiles x kMsRounds] one bit per slot: selected
  uint32_t* tile;         // [tiles] matches per tile (SELECT), then the matches in front of the tile (SCAN)
  uint8_t* keys_out;      // may be null (so may values_out)
  // top / evict / stats
  uint32_t t_off, t_width, t_desc;  // the order field's byte offset and width; 1: the largest ranks first
  uint32_t t_pass, t_k;             // PREFIX / PICK: the pass (0: the most significant byte); min(k, 2^32 - 1)
  uint32_t* bins;         // [kMtBins] zero between the passes
  uint64_t* bitmap2;      // [tiles x kMsRounds] key == cut
  uint32_t* tile2;        // [tiles] equals per tile (CUT), then the equals in front of the tile (SCAN)
  // group: the destination map beside the source above; join: the other map, only read
  XeMapView dst;
  uint32_t g_from, g_off, g_len;     // the group / join bytes: 0 the source key / 1 the source value, first byte, number
  uint32_t g_moff, g_mwidth;         // the measure in the source value (width 0: none)
  uint32_t g_count_off, g_sum_off;   // the accumulators in the destination value (kMgNone: none)
  // compact
  uint32_t c_only;        // 1: REBUILD measures and changes nothing
  // join
  uint32_t j_mode;        // 0: the entries whose join key is an entry of dst are kept; 1: those whose key is not
  uint8_t* j_values;      // n x dst.value_size: the joined entries' values (JOIN_VALUE)
  // modify
  uint32_t m_n;           // the edits in use
  xe_map_edit m_edits[XE_MM_MAX_EDITS];  // checked by the runtime: op, width, the field and an operand field inside the value
  // lru
  uint64_t l_stamp;       // TOUCH: the call's epoch << 48
  uint32_t l_all;         // ERASE: 1: every one of the n entries is a winner (evict), the count drops by n
  uint64_t* l_keys;       // [n] RANK: the rank keys of slot[0 .. n); SORT: sorted into l_keys2, the slots into l_slot2
  uint64_t* l_keys2;
  uint32_t* l_slot2;
  void* l_tmp;            // SORT: the radix sort's own storage (xe_mapop_sort_bytes)
  uint64_t l_tmp_bytes;
};
// The whole struct is a kernel argument. The edits add 200 bytes; it stays far below the 4 KiB a HIP kernel's
// arguments may take.
static_assert(sizeof(XeMapOp) <= 1024, "XeMapOp is passed by value to every map-operation kernel");
XE_HD uint32_t xe_ms_tiles(uint32_t nslots) { return (nslots + kMsTile - 1) / kMsTile; }

// lanes that share one value (a power of two <= 64)
inline uint32_t xe_mo_lanes(uint32_t value_size) {
  return value_size <= kMoInline ? 1u : value_size <= 64 ? 4u : value_size <= 1024 ? 16u : 64u;
}

// ---------------------------------------------------------------- atomics (plain on the host: one thread)
XE_HD uint64_t mo_load64(uint64_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load((unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
XE_HD uint64_t mo_cas64(uint64_t* p, uint64_t expect, uint64_t v) {  // the value found
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned long long c = expect;
  __hip_atomic_compare_exchange_strong((unsigned long long*)p, &c, (unsigned long long)v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  return c;
#else
  const uint64_t c = *p;
  if (c == expect) *p = v;
  return c;
#endif
}
XE_HD void mo_max32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  if (*p < v) *p = v;
#endif
}
XE_HD void mo_add32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *p += v;
#endif
}
XE_HD void mo_or32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *p |= v;
#endif
}

// ---------------------------------------------------------------- keys
// Batch entry i's key as zero-padded words (HASH), as HostMap::pack_key makes them.
XE_HD void mo_load_key(const XeMapOp& o, uint32_t i, uint64_t* kw) {
  const uint8_t* k = o.keys + uint64_t(i) * o.key_size;
  if (!(o.key_size & 7) && !(uintptr_t(o.keys) & 7)) {
    for (uint32_t w = 0; w < XE_MAX_KEY / 8; w++) kw[w] = w < o.kwords ? ((const uint64_t*)k)[w] : 0;
    return;
  }
  for (uint32_t w = 0; w < XE_MAX_KEY / 8; w++) {
    uint64_t v = 0;
    for (uint32_t b = 0; b < 8; b++)
      if (w * 8 + b < o.key_size) v |= uint64_t(k[w * 8 + b]) << (8 * b);
    kw[w] = v;
  }
}
XE_HD uint32_t mo_load_index(const XeMapOp& o, uint32_t i) {
  const uint8_t* k = o.keys + uint64_t(i) * 4;
  return uint32_t(k[0]) | uint32_t(k[1]) << 8 | uint32_t(k[2]) << 16 | uint32_t(k[3]) << 24;
}
XE_HD bool mo_key_eq(const XeMapView& o, const uint64_t* r, const uint64_t* kw) {
  bool eq = true;
  for (uint32_t k = 0; k < XE_MAX_KEY / 8; k++)
    if (k < o.kwords) eq = eq && r[1 + k] == kw[k];
  return eq;
}
XE_HD bool mo_words_eq(const uint64_t* a, const uint64_t* b) {  // two keys as mo_load_key pads them
  bool eq = true;
  for (uint32_t k = 0; k < XE_MAX_KEY / 8; k++) eq = eq && a[k] == b[k];
  return eq;
}
// The last-writer word of a slot: the high half of a HASH record's word 0 (little endian), an ARRAY map's
// word per index. The host build goes through the 64-bit word (one type per object).
XE_HD uint32_t mo_hi_get(const XeMapOp& o, uint32_t slot) {
  if (o.kind == XE_DM_ARRAY) return o.win[slot];
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(reinterpret_cast<uint32_t*>(o.recs + uint64_t(slot) * o.rwords) + 1, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
#else
  return uint32_t(o.recs[uint64_t(slot) * o.rwords] >> 32);
#endif
}
XE_HD void mo_hi_max(const XeMapOp& o, uint32_t slot, uint32_t v) {
  if (o.kind == XE_DM_ARRAY) { mo_max32(o.win + slot, v); return; }
#if defined(__HIP_DEVICE_COMPILE__)
  mo_max32(reinterpret_cast<uint32_t*>(o.recs + uint64_t(slot) * o.rwords) + 1, v);
#else
  uint64_t* r = o.recs + uint64_t(slot) * o.rwords;
  if (uint32_t(*r >> 32) < v) *r = (*r & 0xffffffffull) | (uint64_t(v) << 32);
#endif
}

// The walk of xe_interp.h hash_find, one record at a time: first record that is FULL and holds the key;
// the chain ends at a record that is neither FULL nor a tombstone. kMoAbsent: not there.
XE_HD uint32_t mo_find(const XeMapView& o, const uint64_t* kw) {
  if (o.key_size == 0) return (uint32_t(o.recs[uint64_t(o.cap) * o.rwords]) & XE_SLOT_FULL) ? o.cap : kMoAbsent;
  const uint32_t mask = o.cap - 1;
  uint32_t idx = uint32_t(xe_hash_words(kw, o.kwords, o.key_size)) & mask;
  for (uint32_t probe = 0; probe < o.cap; probe++) {
    const uint64_t* r = o.recs + uint64_t(idx) * o.rwords;
    const uint32_t st = uint32_t(r[0]);
    if (st & XE_SLOT_FULL) {
      if (mo_key_eq(o, r, kw)) return idx;
    } else if (!(st & XE_SLOT_TOMB)) {
      return kMoAbsent;
    }
    idx = (idx + 1) & mask;
  }
  return kMoAbsent;
}

// ---------------------------------------------------------------- cooperative value moves
// Lane `sub` of `lanes` moves its share of len bytes: in units of the widest of 16, 8 or 4 bytes at which
// source and destination are aligned alike (bytes up to the first aligned address, units, bytes), else
// bytes. src null: zero fill.
template <class U>
XE_HD void mo_move_units(uint8_t* t, const uint8_t* s, uint32_t len, uint32_t sub, uint32_t lanes) {
  uint32_t head = uint32_t(-uintptr_t(t)) & uint32_t(sizeof(U) - 1);
  head = head < len ? head : len;
  for (uint32_t j = sub; j < head; j += lanes) t[j] = s ? s[j] : uint8_t(0);
  const uint32_t units = (len - head) / uint32_t(sizeof(U));
  U* tv = reinterpret_cast<U*>(t + head);
  const U* sv = s ? reinterpret_cast<const U*>(s + head) : nullptr;
  for (uint32_t j = sub; j < units; j += lanes) tv[j] = s ? sv[j] : U{};
  for (uint32_t j = head + units * uint32_t(sizeof(U)) + sub; j < len; j += lanes) t[j] = s ? s[j] : uint8_t(0);
}
struct alignas(16) XeMo16 { uint64_t a, b; };
XE_HD void mo_move(uint8_t* t, const uint8_t* s, uint32_t len, uint32_t sub, uint32_t lanes) {
  const uintptr_t x = s ? (uintptr_t(s) ^ uintptr_t(t)) : 0;
  if (len >= 16 && !(x & 15)) mo_move_units<XeMo16>(t, s, len, sub, lanes);
  else if (len >= 8 && !(x & 7)) mo_move_units<uint64_t>(t, s, len, sub, lanes);
  else if (len >= 4 && !(x & 3)) mo_move_units<uint32_t>(t, s, len, sub, lanes);
  else
    for (uint32_t j = sub; j < len; j += lanes) t[j] = s ? s[j] : uint8_t(0);
}

// ---------------------------------------------------------------- where a slot's value lies
// The pair every value access of a map that may be an LRU one goes through, given word 0 of the slot's record
// (ARRAY: anything): is the value nil-backed (it then reads as zeros), and its address. HASH and ARRAY: the VLEN0
// bit and vals + slot x value_size, as before; LRU: the length and the pool entry of the value id in word 0's high
// half (an id at or past pool_cap, which no record of a sound map holds, reads as nil and is never dereferenced).
XE_HD uint32_t ml_vid(uint64_t w0) { return uint32_t(w0 >> 32); }
XE_HD bool mo_val_nil(const XeMapView& v, uint64_t w0) {
  if (v.kind == XE_DM_LRU) return ml_vid(w0) >= v.pool_cap || v.elen[ml_vid(w0)] == 0;
  return v.kind == XE_DM_HASH && (uint32_t(w0) & XE_SLOT_VLEN0) != 0;
}
XE_HD uint8_t* mo_val_at(const XeMapView& v, uint32_t slot, uint64_t w0) {
  return v.vals + uint64_t(v.kind == XE_DM_LRU ? ml_vid(w0) : slot) * v.value_size;
}
XE_HD uint64_t mo_word0(const XeMapView& v, uint32_t slot) { return v.kind == XE_DM_ARRAY ? 0 : v.recs[uint64_t(slot) * v.rwords]; }

// ---------------------------------------------------------------- lookup / delete: find
// Entry i's slot, read-only (kMoAbsent: absent or out of range). find: mo_find, or the kernels' faster probe.
template <class Find>
XE_HD uint32_t mo_slot_of(const XeMapOp& o, uint32_t i, Find find) {
  if (o.kind == XE_DM_ARRAY) {
    const uint32_t idx = mo_load_index(o, i);
    return idx < o.max_entries ? idx : kMoAbsent;
  }
  uint64_t kw[XE_MAX_KEY / 8];
  mo_load_key(o, i, kw);
  return find(o, kw);
}
// ... and what follows from it: found[i], slot[i], and a small value on the same lane.
XE_HD void mo_find_finish(const XeMapOp& o, uint32_t i, uint32_t s, bool with_value) {
  uint32_t w = s;
  const uint64_t w0 = s != kMoAbsent ? mo_word0(o, s) : 0;
  if (s != kMoAbsent && mo_val_nil(o, w0)) w |= kMoVlen0;
  o.slot[i] = w;
  if (o.found) o.found[i] = s != kMoAbsent ? 1 : 0;
  if (with_value && o.value_size <= kMoInline && o.value_size) {
    const bool zero = s == kMoAbsent || (w & kMoVlen0);
    mo_move(o.values_out + uint64_t(i) * o.value_size, zero ? nullptr : mo_val_at(o, s, w0), o.value_size, 0, 1);
  }
}
XE_HD void mo_lookup_value_item(const XeMapOp& o, uint32_t i, uint32_t sub, uint32_t lanes) {
  const uint32_t w = o.slot[i], s = w & kMoSlotMask;
  const bool zero = s == kMoAbsent || (w & kMoVlen0);
  mo_move(o.values_out + uint64_t(i) * o.value_size, zero ? nullptr : mo_val_at(o, s, o.kind == XE_DM_LRU ? mo_word0(o, s) : 0),
          o.value_size, sub, lanes);
}

// ---------------------------------------------------------------- update
// The claim walk of update LOCATE and group LOCATE over HASH table v (see the head of this file): the record
// that holds the key kw, or one claimed for it with word 0 `own` (BUSY | the claimer's name << 32). A record
// claimed in this launch names its claimer j = (w0 >> 32) - 1: same(j) says whether j is a claimer with this
// key. kEmptyKey: the table may be the empty key's one record past cap. kNilBacked: a FULL nil-backed record of
// the key is claimed too, so that it can be zeroed. The slot, with kMoFresh when a free or a tombstone record
// was claimed; kMoAbsent: no free record in the chain.
template <bool kEmptyKey, bool kNilBacked, class Same>
XE_HD uint32_t mo_claim_walk(const XeMapView& v, const uint64_t* kw, uint64_t own, Same same) {
  const bool single = kEmptyKey && v.key_size == 0;
  const uint32_t mask = v.cap - 1;
  uint32_t idx = single ? v.cap : uint32_t(xe_hash_words(kw, v.kwords, v.key_size)) & mask;
  for (uint32_t probe = 0; probe < v.cap;) {
    uint64_t* r = v.recs + uint64_t(idx) * v.rwords;
    const uint64_t w0 = mo_load64(r);
    const uint32_t st = uint32_t(w0);
    if (st & XE_SLOT_FULL) {
      if (mo_key_eq(v, r, kw)) {
        if (!kNilBacked || !(st & XE_SLOT_VLEN0) || (st & XE_SLOT_BUSY)) return idx;
        if (mo_cas64(r, w0, uint64_t(st) | own) == w0) return idx;
        continue;  // lost it (to another claimer of this key): look again
      }
    } else if (st & XE_SLOT_TOMB) {  // holds key words: a deleted entry or an unused reservation
      if (mo_key_eq(v, r, kw)) {
        if (st & XE_SLOT_BUSY) return idx;  // a repetition of this key claimed it
        if (mo_cas64(r, w0, uint64_t(st) | own) == w0) return idx | kMoFresh;
        continue;  // lost it (to a repetition of this key): look again
      }
    } else if (st & XE_SLOT_BUSY) {  // claimed in this launch by the claimer it names
      if (same(uint32_t(w0 >> 32) - 1)) return idx;
    } else {  // free
      if (mo_cas64(r, w0, own) == w0) return idx | kMoFresh;
      continue;  // lost it: look again
    }
    if (single) break;
    idx = (idx + 1) & mask;
    probe++;
  }
  return kMoAbsent;
}
// Entry i's record: the one holding its key, or one claimed for it. True: this entry made the claim (the
// caller counts them). No free record: kMoErrFull.
XE_HD bool mo_update_locate_item(const XeMapOp& o, uint32_t i) {
  if (o.kind == XE_DM_ARRAY) {
    const uint32_t idx = mo_load_index(o, i);
    if (idx >= o.max_entries) mo_or32(o.ctr + kMoErr, kMoErrRange);
    o.slot[i] = idx < o.max_entries ? idx : kMoAbsent;
    return false;
  }
  uint64_t kw[XE_MAX_KEY / 8];
  mo_load_key(o, i, kw);
  const uint32_t c = mo_claim_walk<true, false>(o, kw, XE_SLOT_BUSY | ((uint64_t(i) + 1) << 32), [&](uint32_t j) {
    uint64_t kj[XE_MAX_KEY / 8];
    if (j >= o.n) return false;
    mo_load_key(o, j, kj);
    return mo_words_eq(kj, kw);
  });
  if (c == kMoAbsent) mo_or32(o.ctr + kMoErr, kMoErrFull);
  o.slot[i] = c;
  return (c & kMoFresh) != 0;
}
// The claim of entry i put back: a free record is free again (its key words were never written), a
// tombstone is the tombstone it was.
XE_HD void mo_update_undo_item(const XeMapOp& o, uint32_t i) {
  const uint32_t w = o.slot[i];
  if (o.kind != XE_DM_HASH || !(w & kMoFresh)) return;
  uint64_t* r = o.recs + uint64_t(w & kMoSlotMask) * o.rwords;
  r[0] = uint64_t(uint32_t(r[0]) & ~XE_SLOT_BUSY);
}
XE_HD void mo_update_mark_item(const XeMapOp& o, uint32_t i) {
  const uint32_t w = o.slot[i], s = w & kMoSlotMask;
  if (o.kind == XE_DM_HASH && (w & kMoFresh)) {
    uint64_t* r = o.recs + uint64_t(s) * o.rwords;
    if (!(uint32_t(r[0]) & XE_SLOT_TOMB)) {  // claimed free: the key words are this entry's to write
      uint64_t kw[XE_MAX_KEY / 8];
      mo_load_key(o, i, kw);
      for (uint32_t k = 0; k < XE_MAX_KEY / 8; k++)
        if (k < o.kwords) r[1 + k] = kw[k];
    }
  }
  mo_hi_max(o, s, i + 1);
  if (i == 0 && o.kind == XE_DM_HASH) *o.count += o.ctr[kMoNew];
}
XE_HD void mo_update_copy_item(const XeMapOp& o, uint32_t i, uint32_t sub, uint32_t lanes) {
  const uint32_t s = o.slot[i] & kMoSlotMask;
  if (mo_hi_get(o, s) != i + 1) return;  // a later repetition of the key writes the value (or has written it)
  const uint8_t* v = o.values_in + uint64_t(i) * o.value_size;
  mo_move(o.vals + uint64_t(s) * o.value_size, v, o.value_size, sub, lanes);
  mo_move(o.snap + uint64_t(s) * o.value_size, v, o.value_size, sub, lanes);
  if (sub == 0) {
    if (o.kind == XE_DM_HASH) o.recs[uint64_t(s) * o.rwords] = XE_SLOT_FULL;
    else o.win[s] = 0;
  }
}

// ---------------------------------------------------------------- delete
XE_HD void mo_delete_claim_item(const XeMapOp& o, uint32_t i) {
  const uint32_t s = o.slot[i] & kMoSlotMask;
  if (s == kMoAbsent) return;
  uint64_t* r = o.recs + uint64_t(s) * o.rwords;
  const uint64_t w0 = mo_load64(r);
  if (!(uint32_t(w0) & XE_SLOT_FULL)) return;  // a repetition of the key has it
  if (mo_cas64(r, w0, XE_SLOT_TOMB | ((uint64_t(i) + 1) << 32)) == w0) mo_add32(o.ctr + kMoGone, 1);
}
XE_HD void mo_delete_zero_item(const XeMapOp& o, uint32_t i, uint32_t sub, uint32_t lanes) {
  if (i == 0 && sub == 0) *o.count -= o.ctr[kMoGone];
  const uint32_t s = o.slot[i] & kMoSlotMask;
  if (s == kMoAbsent) return;
  if (mo_hi_get(o, s) != i + 1) return;
  mo_move(o.vals + uint64_t(s) * o.value_size, nullptr, o.value_size, sub, lanes);
  mo_move(o.snap + uint64_t(s) * o.value_size, nullptr, o.value_size, sub, lanes);
  if (sub == 0) o.recs[uint64_t(s) * o.rwords] = XE_SLOT_TOMB;  // a plain tombstone, its key words kept
}

// ---------------------------------------------------------------- scan / expire
XE_HD bool ms_filter(uint32_t op, uint64_t field, uint64_t operand) {
  switch (op) {
    case kMfAll: return true;
    case kMfEq: return field == operand;
    case kMfNe: return field != operand;
    case kMfLt: return field < operand;
    case kMfLe: return field <= operand;
    case kMfGt: return field > operand;
    case kMfGe: return field >= operand;
    case kMfAnyBits: return (field & operand) != 0;
    case kMfNoBits: return (field & operand) == 0;
    default: return false;
  }
}
// The field of the value at v, little endian, zero-extended: one load where the address allows it.
XE_HD uint64_t ms_field(const uint8_t* v, uint32_t width) {
  if (!(uintptr_t(v) & (width - 1))) {
    if (width == 8) return *reinterpret_cast<const uint64_t*>(v);
    if (width == 4) return *reinterpret_cast<const uint32_t*>(v);
    if (width == 2) return *reinterpret_cast<const uint16_t*>(v);
    return *v;
  }
  uint64_t f = 0;
  for (uint32_t b = 0; b < 8; b++)
    if (b < width) f |= uint64_t(v[b]) << (8 * b);
  return f;
}
// Is slot sbase + s (s < nslots) selected? HASH: FULL records only (a tombstone keeps key words and a zero
// value and never matches); a nil-backed value reads as zeros, as it does for xe_map_lookup.
XE_HD bool ms_select_item(const XeMapOp& o, uint32_t s) {
  const uint32_t at = o.sbase + s;
  const uint64_t w0 = mo_word0(o, at);
  if (o.kind != XE_DM_ARRAY && !(uint32_t(w0) & XE_SLOT_FULL)) return false;
  if (o.f_op == kMfAll) return true;
  return ms_filter(o.f_op, mo_val_nil(o, w0) ? 0 : ms_field(mo_val_at(o, at, w0) + o.f_off, o.f_width), o.f_operand);
}
// Lane `lane` of round `round` of tile t, given the round's bitmap word and the matches in front of the
// round: a selected slot's rank; below n it is reported.
XE_HD void ms_scatter_item(const XeMapOp& o, uint32_t t, uint32_t round, uint32_t lane, uint64_t word, uint32_t before) {
  if (!((word >> lane) & 1)) return;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t rank = before + __builtin_amdgcn_mbcnt_hi(uint32_t(word >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(word), 0));
#else
  const uint32_t rank = before + uint32_t(__builtin_popcountll(word & ((uint64_t(1) << lane) - 1)));
#endif
  if (rank < o.n) o.slot[rank] = o.sbase + t * kMsTile + round * 64 + lane;
}
XE_HD void ms_copy_item(const XeMapOp& o, uint32_t j, uint32_t sub, uint32_t lanes) {
  const uint32_t s = o.slot[j];
  if (o.keys_out) {
    if (o.kind == XE_DM_ARRAY) {
      uint8_t* k = o.keys_out + uint64_t(j) * 4;
      if (sub == 0) k[0] = uint8_t(s), k[1] = uint8_t(s >> 8), k[2] = uint8_t(s >> 16), k[3] = uint8_t(s >> 24);
    } else if (o.key_size) {  // (an LRU map's nil key, the record past the table: key_size zero bytes)
      const bool nil_key = o.kind == XE_DM_LRU && s == o.cap;
      mo_move(o.keys_out + uint64_t(j) * o.key_size, nil_key ? nullptr : reinterpret_cast<const uint8_t*>(o.recs + uint64_t(s) * o.rwords + 1),
              o.key_size, sub, lanes);
    }
  }
  if (o.values_out) {
    const uint64_t w0 = mo_word0(o, s);
    mo_move(o.values_out + uint64_t(j) * o.value_size, mo_val_nil(o, w0) ? nullptr : mo_val_at(o, s, w0), o.value_size, sub, lanes);
  }
}
XE_HD void ms_expire_item(const XeMapOp& o, uint32_t j, uint32_t sub, uint32_t lanes) {
  if (j == 0 && sub == 0) *o.count -= o.n;
  const uint32_t s = o.slot[j];
  mo_move(o.vals + uint64_t(s) * o.value_size, nullptr, o.value_size, sub, lanes);
  mo_move(o.snap + uint64_t(s) * o.value_size, nullptr, o.value_size, sub, lanes);
  if (sub == 0) o.recs[uint64_t(s) * o.rwords] = XE_SLOT_TOMB;  // a plain tombstone, its key words kept
}


// ---------------------------------------------------------------- top / evict / stats
XE_HD void mo_add64(uint64_t* p, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_fetch_add((unsigned long long*)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *p += v;
#endif
}
XE_HD void mo_max64(uint64_t* p, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_fetch_max((unsigned long long*)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  if (*p < v) *p = v;
#endif
}
XE_HD uint64_t mt_mask(uint32_t width) { return width >= 8 ? ~uint64_t(0) : (uint64_t(1) << (8 * width)) - 1; }
// Is slot sbase + s eligible (ms_select_item's answer), and if so its rank key: the order field (0 under
// VLEN0), complemented within the width when the largest ranks first.
XE_HD bool mt_key_item(const XeMapOp& o, uint32_t s, uint64_t* key) {
  const uint32_t at = o.sbase + s;
  const uint64_t w0 = mo_word0(o, at);
  if (o.kind != XE_DM_ARRAY && !(uint32_t(w0) & XE_SLOT_FULL)) return false;
  // an LRU entry ranks by its stamp (t_width is 8), and one whose stamp is 0 is in no usage order
  const uint64_t stamp = o.kind == XE_DM_LRU && ml_vid(w0) < o.pool_cap ? o.tag[ml_vid(w0)] : 0;
  if (o.kind == XE_DM_LRU && !stamp) return false;
  const bool zero = mo_val_nil(o, w0);
  const uint8_t* v = mo_val_at(o, at, w0);
  if (o.f_op != kMfAll && !ms_filter(o.f_op, zero ? 0 : ms_field(v + o.f_off, o.f_width), o.f_operand)) return false;
  const uint64_t f = o.kind == XE_DM_LRU ? stamp : zero ? 0 : ms_field(v + o.t_off, o.t_width);
  *key = o.t_desc ? ~f & mt_mask(o.t_width) : f;
  return true;
}
XE_HD uint64_t mt_prefix(const XeMapOp& o) { return uint64_t(o.ctr[kMtPrefix]) | uint64_t(o.ctr[kMtPrefix + 1]) << 32; }
// PREFIX, pass t_pass: does the key share the bytes fixed so far, and the bin of its next byte.
XE_HD bool mt_in_prefix(const XeMapOp& o, uint64_t key, uint64_t prefix) {
  return o.t_pass == 0 || (key >> (8 * (o.t_width - o.t_pass))) == prefix;
}
XE_HD uint32_t mt_bin(const XeMapOp& o, uint64_t key) { return uint32_t(key >> (8 * (o.t_width - 1 - o.t_pass))) & 255u; }
// PICK, bin b holding c keys with `before` keys in the bins in front of it: does the number needed run out here?
XE_HD bool mt_pick_here(uint32_t need, uint32_t before, uint32_t c) { return need > before && need - before <= c; }
XE_HD void mt_pick_write(const XeMapOp& o, uint32_t b, uint32_t need, uint32_t before) {
  const uint64_t p = (o.t_pass ? mt_prefix(o) << 8 : 0) | b;
  o.ctr[kMtPrefix] = uint32_t(p);
  o.ctr[kMtPrefix + 1] = uint32_t(p >> 32);
  o.ctr[kMtNeed] = need - before;
}
// CUT: 1: the key ranks in front of the cut; 2: it equals the cut; 0: neither, or nothing is needed.
XE_HD uint32_t mt_cut_item(const XeMapOp& o, uint32_t s, uint64_t cut, uint32_t need) {
  uint64_t key;
  if (!need || !mt_key_item(o, s, &key)) return 0;
  return key < cut ? 1u : key == cut ? 2u : 0u;
}
// TRIM: lane `lane` of a round whose equal bits are `word`, with `before` equals in front of the round.
XE_HD bool mt_trim_item(uint32_t lane, uint64_t word, uint32_t before, uint32_t need) {
  if (!((word >> lane) & 1)) return false;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t rank = before + __builtin_amdgcn_mbcnt_hi(uint32_t(word >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(word), 0));
#else
  const uint32_t rank = before + uint32_t(__builtin_popcountll(word & ((uint64_t(1) << lane) - 1)));
#endif
  return rank < need;
}
// STATS: one lane's running count, sum, ~min and max; and their way into the counters.
struct XeMtStats { uint64_t count, sum, nmin, max; };
XE_HD void mt_stats_item(const XeMapOp& o, uint32_t s, XeMtStats* a) {
  uint64_t f;
  if (!mt_key_item(o, s, &f)) return;  // (t_desc is 0: the key is the field)
  a->count++;
  a->sum += f;
  a->nmin = a->nmin > ~f ? a->nmin : ~f;
  a->max = a->max > f ? a->max : f;
}
XE_HD void mt_stats_flush(const XeMapOp& o, const XeMtStats& a) {
  if (!a.count) return;
  uint64_t* w = reinterpret_cast<uint64_t*>(o.ctr + kMtStats);
  mo_add64(w, a.count);
  mo_add64(w + 1, a.sum);
  mo_max64(w + 2, a.nmin);
  mo_max64(w + 3, a.max);
}

// ---------------------------------------------------------------- group
// Is the value of source slot `at` nil-backed (it then reads as zeros)?
XE_HD bool mg_src_zero(const XeMapOp& o, uint32_t at) {
  return o.kind == XE_DM_HASH && (uint32_t(o.recs[uint64_t(at) * o.rwords]) & XE_SLOT_VLEN0) != 0;
}
// The group key of source slot `at` (sbase included) as zero-padded words, as mo_load_key makes a key's: g_len
// bytes at g_off of the slot's key (ARRAY: its index as a u32) or of its value. An ARRAY destination's index
// is word 0 (g_len <= 4: zero-extended).
XE_HD void mg_group_key(const XeMapOp& o, uint32_t at, uint64_t* kw) {
  for (uint32_t w = 0; w < XE_MAX_KEY / 8; w++) kw[w] = 0;
  if (o.g_from == 0 && o.kind == XE_DM_ARRAY) {  // (g_off + g_len <= 4)
    kw[0] = (uint64_t(at) >> (8 * o.g_off)) & mt_mask(o.g_len);
    return;
  }
  if (o.g_from != 0 && mg_src_zero(o, at)) return;
  const uint8_t* p = (o.g_from == 0 ? reinterpret_cast<const uint8_t*>(o.recs + uint64_t(at) * o.rwords + 1)
                                    : o.vals + uint64_t(at) * o.value_size) + o.g_off;
  if (!(o.g_len & 7) && !(uintptr_t(p) & 7)) {
    for (uint32_t w = 0; w < XE_MAX_KEY / 8; w++)
      if (w * 8 < o.g_len) kw[w] = reinterpret_cast<const uint64_t*>(p)[w];
    return;
  }
  for (uint32_t w = 0; w < XE_MAX_KEY / 8; w++) {
    uint64_t v = 0;
    for (uint32_t b = 0; b < 8; b++)
      if (w * 8 + b < o.g_len) v |= uint64_t(p[w * 8 + b]) << (8 * b);
    kw[w] = v;
  }
}
XE_HD uint64_t mg_measure(const XeMapOp& o, uint32_t at) {
  if (!o.g_mwidth || mg_src_zero(o, at)) return 0;
  return ms_field(o.vals + uint64_t(at) * o.value_size + o.g_moff, o.g_mwidth);
}
// LOCATE: the destination record of source slot sbase + s's group, or one claimed for it: mo_claim_walk over the
// destination with the claim naming the source slot. True: this slot claimed a free or a tombstone record (the
// caller counts them). An ARRAY destination only has its index checked.
XE_HD bool mg_locate_item(const XeMapOp& o, uint32_t s) {
  const uint32_t at = o.sbase + s;
  uint64_t kw[XE_MAX_KEY / 8];
  mg_group_key(o, at, kw);
  if (o.dst.kind == XE_DM_ARRAY) {
    if (kw[0] >= o.dst.max_entries) mo_or32(o.ctr + kMoErr, kMoErrRange);
    return false;
  }
  const uint32_t c = mo_claim_walk<false, true>(o.dst, kw, XE_SLOT_BUSY | ((uint64_t(at) + 1) << 32), [&](uint32_t j) {
    uint64_t kj[XE_MAX_KEY / 8];
    if (j < o.sbase || j - o.sbase >= o.nslots) return false;
    mg_group_key(o, j, kj);
    return mo_words_eq(kj, kw);
  });
  if (c == kMoAbsent) mo_or32(o.ctr + kMoErr, kMoErrFull);
  return (c & kMoFresh) != 0;
}
// UNDO, destination slot ds: a claimed record is what it was (the high half of word 0 was zero).
XE_HD void mg_undo_item(const XeMapOp& o, uint32_t ds) {
  uint64_t* r = o.dst.recs + uint64_t(ds) * o.dst.rwords;
  const uint32_t st = uint32_t(r[0]);
  if (st & XE_SLOT_BUSY) r[0] = uint64_t(st & ~XE_SLOT_BUSY);
}
// PUBLISH, destination slot ds, lane `sub` of the `lanes` that share it: nothing unless the record is claimed.
XE_HD bool mg_claimed(const XeMapOp& o, uint32_t ds) { return (uint32_t(o.dst.recs[uint64_t(ds) * o.dst.rwords]) & XE_SLOT_BUSY) != 0; }
XE_HD void mg_publish_item(const XeMapOp& o, uint32_t ds, uint32_t sub, uint32_t lanes) {
  uint64_t* r = o.dst.recs + uint64_t(ds) * o.dst.rwords;
  const uint64_t w0 = r[0];
  const uint32_t st = uint32_t(w0);
  // the value: zero in the map and in the delta base (a tombstone's usually is, a nil-backed record's is not)
  mo_move(o.dst.vals + uint64_t(ds) * o.dst.value_size, nullptr, o.dst.value_size, sub, lanes);
  mo_move(o.dst.snap + uint64_t(ds) * o.dst.value_size, nullptr, o.dst.value_size, sub, lanes);
  if (sub != 0) return;
  if (!(st & (XE_SLOT_FULL | XE_SLOT_TOMB))) {  // claimed free: the key words are the claiming slot's group key
    uint64_t kw[XE_MAX_KEY / 8];
    mg_group_key(o, uint32_t(w0 >> 32) - 1, kw);
    for (uint32_t k = 0; k < XE_MAX_KEY / 8; k++)
      if (k < o.dst.kwords) r[1 + k] = kw[k];
  }
  r[0] = XE_SLOT_FULL;
}
XE_HD void mg_publish_count(const XeMapOp& o) { *o.dst.count += o.ctr[kMoNew]; }
// ADD: the destination slot of source slot sbase + s's group, read-only (find: as mo_slot_of's); kMoAbsent
// cannot happen after LOCATE and PUBLISH and is skipped.
template <class Find>
XE_HD uint32_t mg_slot_of(const XeMapOp& o, uint32_t s, Find find) {
  uint64_t kw[XE_MAX_KEY / 8];
  mg_group_key(o, o.sbase + s, kw);
  if (o.dst.kind == XE_DM_ARRAY) return kw[0] < o.dst.max_entries ? uint32_t(kw[0]) : kMoAbsent;
  return find(o.dst, kw);
}
// ... and `count` entries with measures summing to `sum` added to destination slot ds, in the map and in the
// delta base alike (so xe_map_delta sees no packet adds).
XE_HD void mg_add_item(const XeMapOp& o, uint32_t ds, uint64_t count, uint64_t sum) {
  uint8_t* v = o.dst.vals + uint64_t(ds) * o.dst.value_size;
  uint8_t* b = o.dst.snap + uint64_t(ds) * o.dst.value_size;
  if (o.g_count_off != kMgNone) {
    mo_add64(reinterpret_cast<uint64_t*>(v + o.g_count_off), count);
    mo_add64(reinterpret_cast<uint64_t*>(b + o.g_count_off), count);
  }
  if (o.g_sum_off != kMgNone) {
    mo_add64(reinterpret_cast<uint64_t*>(v + o.g_sum_off), sum);
    mo_add64(reinterpret_cast<uint64_t*>(b + o.g_sum_off), sum);
  }
}

// ---------------------------------------------------------------- compact
// MARK, slot s (< cap): 1 free, 2 a tombstone, 0 an entry (the classes of the two bitmaps, as mt_cut_item's).
XE_HD uint32_t mc_mark_item(const XeMapOp& o, uint32_t s) {
  const uint32_t st = uint32_t(o.recs[uint64_t(s) * o.rwords]);
  return (st & XE_SLOT_FULL) ? 0u : (st & XE_SLOT_TOMB) ? 2u : 1u;
}
// One bit of a bitmap: slot s sits in word s / 64 (tile s / kMsTile, round s / 64 % kMsRounds).
XE_HD bool mc_bit(const uint64_t* bm, uint32_t s) { return (bm[s >> 6] >> (s & 63)) & 1; }
// REBUILD: does slot s (< cap) start a run? It is not free and its predecessor modulo cap is.
XE_HD bool mc_run_start(const XeMapOp& o, uint32_t s) {
  return !mc_bit(o.bitmap, s) && mc_bit(o.bitmap, (s - 1) & (o.cap - 1));
}
// ... and the run that starts there: its slots up to the next free one (through the table's end), and the
// offset of its first tombstone (>= the length: none). Word operations on the two bitmaps; a run has a start
// only when the table has a free record, so the walk ends.
XE_HD uint32_t mc_run_scan(const XeMapOp& o, uint32_t s, uint32_t* first_tomb) {
  uint32_t len = 0, first = 0xffffffffu, p = s;
  while (len < o.cap) {
    const uint32_t bit = p & 63, left = o.cap - p;
    const uint32_t valid = 64 - bit < left ? 64 - bit : left;  // slots of this word from p on, inside the table
    const uint64_t in = valid == 64 ? ~uint64_t(0) : (uint64_t(1) << valid) - 1;
    const uint64_t fr = (o.bitmap[p >> 6] >> bit) & in;
    uint64_t tb = (o.bitmap2[p >> 6] >> bit) & in;
    const uint32_t upto = fr ? uint32_t(__builtin_ctzll(fr)) : valid;
    if (upto < 64) tb &= (uint64_t(1) << upto) - 1;
    if (tb && first == 0xffffffffu) first = len + uint32_t(__builtin_ctzll(tb));
    len += upto;
    if (fr) break;
    p = (p + valid) & (o.cap - 1);
  }
  *first_tomb = first;
  return len;
}
// The walk, run offset j of the run that starts at slot s (every slot in front of j holds the new layout):
// the offset the entry there belongs at (j: it stays), kMcDead when the record is no entry. An entry whose home
// lay outside the slots in front of it (no table the map's calls make) stays.
XE_HD uint32_t mc_target(const XeMapOp& o, uint32_t s, uint32_t j) {
  const uint32_t mask = o.cap - 1;
  const uint64_t* r = o.recs + uint64_t((s + j) & mask) * o.rwords;
  if (!(uint32_t(r[0]) & XE_SLOT_FULL)) return kMcDead;
  uint32_t q = (uint32_t(xe_hash_words(r + 1, o.kwords, o.key_size)) - s) & mask;
  if (q > j) return j;
  while (q < j && (uint32_t(o.recs[uint64_t((s + q) & mask) * o.rwords]) & XE_SLOT_FULL)) q++;
  return q;
}
// ... and what follows from it, by lane `sub` of the `lanes` that share the record: the record and the value
// (map and delta base) move to offset q < j and slot j is zeroed; a record that is no entry is zeroed.
XE_HD void mc_apply(const XeMapOp& o, uint32_t s, uint32_t j, uint32_t q, uint32_t sub, uint32_t lanes) {
  if (q == j) return;
  const uint32_t mask = o.cap - 1, at = (s + j) & mask;
  uint64_t* r = o.recs + uint64_t(at) * o.rwords;
  uint8_t* v = o.vals + uint64_t(at) * o.value_size;
  uint8_t* b = o.snap + uint64_t(at) * o.value_size;
  if (q != kMcDead) {
    const uint32_t to = (s + q) & mask;
    mo_move(o.vals + uint64_t(to) * o.value_size, v, o.value_size, sub, lanes);
    mo_move(o.snap + uint64_t(to) * o.value_size, b, o.value_size, sub, lanes);
    if (sub == 0) {
      uint64_t* t = o.recs + uint64_t(to) * o.rwords;
      for (uint32_t k = 0; k < XE_MAX_KEY / 8; k++)
        if (k < o.kwords) t[1 + k] = r[1 + k];
      t[0] = uint64_t(uint32_t(r[0]) & (XE_SLOT_FULL | XE_SLOT_VLEN0));
    }
  }
  mo_move(v, nullptr, o.value_size, sub, lanes);
  mo_move(b, nullptr, o.value_size, sub, lanes);
  if (sub == 0) {
    for (uint32_t k = 0; k < XE_MAX_KEY / 8; k++)
      if (k < o.kwords) r[1 + k] = 0;
    r[0] = 0;
  }
}
// What a run of len slots whose first tombstone is at offset `first` adds to the counters; true: it is to be
// rebuilt (the walk starts at `first`: the entries in front of the first tombstone never move).
XE_HD bool mc_run_counts(const XeMapOp& o, uint32_t len, uint32_t first) {
  if (first >= len) return false;
  mo_max32(o.ctr + kMcLongest, len);
  if (len > kMcMaxRun) { mo_or32(o.ctr + kMcLong, 1); return false; }
  return !o.c_only;
}

// ---------------------------------------------------------------- modify
// One edit's arithmetic on the zero-extended field (include/xdpemu.h XE_MM_*): the new field, within the width.
XE_HD uint64_t mm_apply(uint32_t op, uint64_t field, uint64_t operand, uint32_t width) {
  const uint64_t mask = mt_mask(width);
  const uint64_t sat = operand > mask ? mask : operand;  // an operand the field cannot hold acts as the largest it can
  switch (op) {
    case kMmSet: return operand & mask;
    case kMmAdd: return (field + operand) & mask;
    case kMmSub: return (field - operand) & mask;
    case kMmAddSat: return sat > mask - field ? mask : field + sat;
    case kMmSubSat: return field > sat ? field - sat : 0;
    case kMmAnd: return field & operand;
    case kMmOr: return (field | operand) & mask;
    case kMmXor: return (field ^ operand) & mask;
    case kMmMin: return field < sat ? field : sat;
    case kMmMax: return field > sat ? field : sat;
    case kMmShr: return operand >= 8 * width ? 0 : field >> operand;
    default: return field;
  }
}
// The field at v set to x: one store where the address allows it (ms_field's counterpart), else bytes.
XE_HD void mm_store(uint8_t* v, uint32_t width, uint64_t x) {
  if (!(uintptr_t(v) & (width - 1))) {
    if (width == 8) *reinterpret_cast<uint64_t*>(v) = x;
    else if (width == 4) *reinterpret_cast<uint32_t*>(v) = uint32_t(x);
    else if (width == 2) *reinterpret_cast<uint16_t*>(v) = uint16_t(x);
    else *v = uint8_t(x);
    return;
  }
  for (uint32_t b = 0; b < 8; b++)
    if (b < width) v[b] = uint8_t(x >> (8 * b));
}
// The edit list applied to the value at v, by one lane, in list order on the value as it stands (zero: it reads
// as zeros, so it is zeroed first). An operand field is read when its edit runs.
XE_HD void mm_edit_value(const XeMapOp& o, uint8_t* v, bool zero) {
  if (zero) mo_move(v, nullptr, o.value_size, 0, 1);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1  // (an edit's words are read when its turn comes: the list is not held in registers)
#endif
  for (uint32_t e = 0; e < o.m_n; e++) {
    const xe_map_edit& d = o.m_edits[e];
    const uint64_t operand = (d.flags & XE_MM_OPERAND_FIELD) ? ms_field(v + d.operand, d.width) : d.operand;
    mm_store(v + d.offset, d.width, mm_apply(d.op, ms_field(v + d.offset, d.width), operand, d.width));
  }
}
// What orders the stores of one lane before the loads and stores of the other lanes of its sub-group. A
// sub-group never spans waves (xe_mo_lanes <= 64 divides the wave), and a wave's vector memory instructions
// reach the memory pipeline in program order: release and acquire fences at wavefront scope keep the compiler
// from moving accesses across this point and are all the AMDGPU memory model asks for between the lanes of one
// wave. Nothing here depends on the lanes running in lockstep.
XE_HD void mm_subgroup_order() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
}
// Slot `slot` (sbase included) edited by lane `sub` of the `lanes` that share it: a nil-backed value is zeroed,
// the edits run, the whole value goes to the delta base (so xe_map_delta sees no packet adds on it, and adds
// still pending are dropped, as an update drops them), the record is left plain FULL (HASH: VLEN0 and the
// last-writer word cleared; keyed, ARRAY: the index's last-writer word cleared).
// Lane 0 alone zeroes and edits the value in the map: one thread's stores and loads to one address keep their
// order. The copy to the delta base is shared, so the other lanes read bytes lane 0 wrote: mm_subgroup_order
// stands between the two. The record's word 0 is written by lane 0 after every lane of the sub-group has read
// it (the read below is in front of the ordering point, the write behind it).
XE_HD void mm_modify_item(const XeMapOp& o, uint32_t slot, uint32_t sub, uint32_t lanes, bool keyed) {
  uint64_t* r = o.kind == XE_DM_HASH ? o.recs + uint64_t(slot) * o.rwords : nullptr;
  const uint64_t w0 = r ? r[0] : 0;
  uint8_t* v = o.vals + uint64_t(slot) * o.value_size;
  if (sub == 0) mm_edit_value(o, v, (uint32_t(w0) & XE_SLOT_VLEN0) != 0);
  if (lanes > 1) mm_subgroup_order();
  mo_move(o.snap + uint64_t(slot) * o.value_size, v, o.value_size, sub, lanes);
  if (sub != 0) return;
  if (r) {
    if (w0 != XE_SLOT_FULL) r[0] = XE_SLOT_FULL;
  } else if (keyed) {
    o.win[slot] = 0;
  }
}
// MARK: a present entry names itself on its slot; KEYED: the entry still named there edits the slot.
XE_HD void mm_mark_item(const XeMapOp& o, uint32_t i) {
  const uint32_t s = o.slot[i] & kMoSlotMask;
  if (s != kMoAbsent) mo_hi_max(o, s, i + 1);
}
XE_HD void mm_keyed_item(const XeMapOp& o, uint32_t i, uint32_t sub, uint32_t lanes) {
  const uint32_t s = o.slot[i] & kMoSlotMask;
  if (s == kMoAbsent || mo_hi_get(o, s) != i + 1) return;  // absent, or another repetition of the key edits
  mm_modify_item(o, s, sub, lanes, true);
}

// ---------------------------------------------------------------- join
// JOIN_SELECT: is the candidate in source slot sbase + s (ms_select_item said yes) kept? Its join key is the
// group's (mg_group_key), the probe of the other map read-only (find: as mo_slot_of's): a FULL record that
// holds the key, nil-backed or not, is present, a tombstone is not; an ARRAY index at or beyond max_entries is absent.
template <class Find>
XE_HD bool mj_kept_item(const XeMapOp& o, uint32_t s, Find find) {
  return (mg_slot_of(o, s, find) != kMoAbsent) != (o.j_mode != 0);
}
// JOIN_VALUE, reported entry j by lane `sub` of the `lanes` that share it: the value of the entry that slot[j]
// joined with, found again from slot[j] alone; zeros when it is nil-backed, and always under mode 1 (no probe).
template <class Find>
XE_HD void mj_value_item(const XeMapOp& o, uint32_t j, uint32_t sub, uint32_t lanes, Find find) {
  const uint32_t ds = o.j_mode ? kMoAbsent : mg_slot_of(o, o.slot[j] - o.sbase, find);
  const bool zero = ds == kMoAbsent ||
                    (o.dst.kind == XE_DM_HASH && (uint32_t(o.dst.recs[uint64_t(ds) * o.dst.rwords]) & XE_SLOT_VLEN0));
  mo_move(o.j_values + uint64_t(j) * o.dst.value_size, zero ? nullptr : o.dst.vals + uint64_t(ds) * o.dst.value_size,
          o.dst.value_size, sub, lanes);
}

// ---------------------------------------------------------------- lru
// TOUCH, entry i: a found entry's value gets the call's stamp for it. A later repetition of the key carries a
// larger one, so the maximum is the last occurrence's.
XE_HD void ml_touch_item(const XeMapOp& o, uint32_t i) {
  const uint32_t s = o.slot[i] & kMoSlotMask;
  if (s == kMoAbsent) return;
  const uint32_t vid = ml_vid(o.recs[uint64_t(s) * o.rwords]);
  if (vid < o.pool_cap) mo_max64(o.tag + vid, o.l_stamp | (uint64_t(i) + 1));
}
// CLAIM, entry i: true when this entry took the record (the caller counts the winners).
XE_HD bool ml_claim_item(const XeMapOp& o, uint32_t i) {
  const uint32_t s = o.slot[i] & kMoSlotMask;
  if (s == kMoAbsent) return false;
  uint64_t* r = o.recs + uint64_t(s) * o.rwords;
  const uint64_t w0 = mo_load64(r);
  if (!(uint32_t(w0) & XE_SLOT_FULL)) return false;  // a repetition of the key has it
  if (mo_cas64(r, w0, (w0 & ~uint64_t(0xffffffffu)) | XE_SLOT_TOMB) != w0) return false;
  o.slot[i] |= kMoFresh;
  return true;
}
// ERASE, entry i: what lru_erase leaves (the head of this file says why the value bytes stay).
XE_HD void ml_erase_item(const XeMapOp& o, uint32_t i) {
  if (i == 0) o.hdr[2] -= o.l_all ? o.n : o.ctr[kMoGone];
  const uint32_t w = o.slot[i];
  if (!o.l_all && !(w & kMoFresh)) return;
  uint64_t* r = o.recs + uint64_t(w & kMoSlotMask) * o.rwords;
  const uint32_t vid = ml_vid(r[0]);
  if (vid < o.pool_cap) o.tag[vid] = 0;
  r[0] = XE_SLOT_TOMB;  // a plain tombstone, its key words kept
}
// RANK, entry j: the rank key of slot[j] (SCATTER selected it: it is eligible).
XE_HD void ml_rank_item(const XeMapOp& o, uint32_t j) {
  uint64_t key = 0;
  mt_key_item(o, o.slot[j] - o.sbase, &key);
  o.l_keys[j] = key;
}

#ifndef XE_HOSTSIM
extern "C" int xe_launch_mapop(const XeMapOp* op, uint32_t step, void* stream);
extern "C" int xe_mapop_sort_bytes(uint32_t n, size_t* bytes);  // SORT's l_tmp for n pairs
#else
#include <algorithm>
#include <vector>
static inline int xe_mapop_sort_bytes(uint32_t, size_t* bytes) { *bytes = 8; return 0; }
// The host simulation: the same items, one after another. A pass that ballots: for every tile, round and lane
// cls(t, r, lane) gives the slot's class; done(t, w1, w2, c1, c2) gets the tile's words of class 1 and class 2,
// one per round, and their counts.
template <class Cls, class Done>
static inline void sim_tile_words(uint32_t tiles, Cls cls, Done done) {
  for (uint32_t t = 0; t < tiles; t++) {
    uint64_t w1[kMsRounds] = {}, w2[kMsRounds] = {};
    uint32_t c1 = 0, c2 = 0;
    for (uint32_t r = 0; r < kMsRounds; r++)
      for (uint32_t lane = 0; lane < 64; lane++) {
        const uint32_t c = cls(t, r, lane);
        if (c == 1) w1[r] |= uint64_t(1) << lane, c1++;
        if (c == 2) w2[r] |= uint64_t(1) << lane, c2++;
      }
    done(t, w1, w2, c1, c2);
  }
}
static inline int xe_launch_mapop(const XeMapOp* op, uint32_t step, void*) {
  const XeMapOp& o = *op;
  const uint32_t tiles = xe_ms_tiles(o.nslots);
  // a class per slot of the source (slots past nslots: none), and the two bitmaps and tile counts from the words
  const auto slots = [&](auto item) {
    return [&o, item](uint32_t t, uint32_t r, uint32_t lane) {
      const uint32_t s = t * kMsTile + r * 64 + lane;
      return s < o.nslots ? uint32_t(item(s)) : 0u;
    };
  };
  const auto put = [&](uint32_t t, const uint64_t* w1, const uint64_t* w2, uint32_t count) {  // (w2 null: one bitmap)
    for (uint32_t r = 0; r < kMsRounds; r++) {
      o.bitmap[uint64_t(t) * kMsRounds + r] = w1[r];
      if (w2) o.bitmap2[uint64_t(t) * kMsRounds + r] = w2[r];
    }
    o.tile[t] = count;
  };
  using Words = const uint64_t*;
  if (step == XE_MO_SCAN_SELECT) {
    sim_tile_words(tiles, slots([&](uint32_t s) { return ms_select_item(o, s); }),
                   [&](uint32_t t, Words w1, Words, uint32_t c1, uint32_t) { put(t, w1, nullptr, c1); });
    return 0;
  }
  if (step == XE_MO_JOIN_SELECT) {  // the candidates go to the counters, the kept ones to the bitmap
    sim_tile_words(tiles, slots([&](uint32_t s) {
                     if (!ms_select_item(o, s)) return false;
                     o.ctr[kMjSelected]++;
                     return mj_kept_item(o, s, mo_find);
                   }),
                   [&](uint32_t t, Words w1, Words, uint32_t c1, uint32_t) { put(t, w1, nullptr, c1); });
    return 0;
  }
  if (step == XE_MO_SCAN_SCAN) {
    uint32_t carry = 0;
    for (uint32_t t = 0; t < tiles; t++) {
      const uint32_t c = o.tile[t];
      o.tile[t] = carry;
      carry += c;
    }
    o.ctr[kMoMatched] = carry;
    return 0;
  }
  if (step == XE_MO_SCAN_SCATTER) {
    for (uint32_t t = 0; t < tiles; t++) {
      uint32_t before = o.tile[t];
      for (uint32_t r = 0; r < kMsRounds; r++) {
        const uint64_t word = o.bitmap[uint64_t(t) * kMsRounds + r];
        for (uint32_t lane = 0; lane < 64; lane++) ms_scatter_item(o, t, r, lane, word, before);
        before += uint32_t(__builtin_popcountll(word));
      }
    }
    return 0;
  }
  if (step == XE_MO_TOP_PREFIX) {
    const uint64_t prefix = mt_prefix(o);
    for (uint32_t s = 0; s < o.nslots; s++) {
      uint64_t key;
      if (mt_key_item(o, s, &key) && mt_in_prefix(o, key, prefix)) o.bins[mt_bin(o, key)]++;
    }
    return 0;
  }
  if (step == XE_MO_TOP_PICK) {
    uint32_t need = o.ctr[kMtNeed];
    if (o.t_pass == 0) {
      uint32_t total = 0;
      for (uint32_t b = 0; b < kMtBins; b++) total += o.bins[b];
      o.ctr[kMtMatched] = total;
      need = total < o.t_k ? total : o.t_k;
    }
    uint32_t before = 0;
    for (uint32_t b = 0; b < kMtBins; b++) {
      const uint32_t c = o.bins[b];
      if (mt_pick_here(need, before, c)) mt_pick_write(o, b, need, before);
      before += c;
      o.bins[b] = 0;
    }
    return 0;
  }
  if (step == XE_MO_TOP_CUT) {
    const uint64_t cut = mt_prefix(o);
    const uint32_t need = o.ctr[kMtNeed];
    sim_tile_words(tiles, slots([&](uint32_t s) { return mt_cut_item(o, s, cut, need); }),
                   [&](uint32_t t, Words w1, Words w2, uint32_t c1, uint32_t c2) { put(t, w1, w2, c1), o.tile2[t] = c2; });
    return 0;
  }
  if (step == XE_MO_TOP_TRIM) {  // the equals kept join the first bitmap and its tile's count
    const uint32_t need = o.ctr[kMtNeed];
    const auto kept = [&](uint32_t t, uint32_t r, uint32_t lane) {
      uint32_t before = o.tile2[t];
      for (uint32_t q = 0; q < r; q++) before += uint32_t(__builtin_popcountll(o.bitmap2[uint64_t(t) * kMsRounds + q]));
      return uint32_t(mt_trim_item(lane, o.bitmap2[uint64_t(t) * kMsRounds + r], before, need));
    };
    sim_tile_words(tiles, kept, [&](uint32_t t, Words w1, Words, uint32_t c1, uint32_t) {
      for (uint32_t r = 0; r < kMsRounds; r++) o.bitmap[uint64_t(t) * kMsRounds + r] |= w1[r];
      o.tile[t] += c1;
    });
    return 0;
  }
  if (step == XE_MO_TOP_STATS) {
    XeMtStats a{};
    for (uint32_t s = 0; s < o.nslots; s++) mt_stats_item(o, s, &a);
    mt_stats_flush(o, a);
    return 0;
  }
  if (step == XE_MO_GROUP_LOCATE || step == XE_MO_GROUP_ADD) {  // over the source bitmap
    for (uint32_t t = 0; t < tiles; t++)
      for (uint32_t r = 0; r < kMsRounds; r++) {
        const uint64_t word = o.bitmap[uint64_t(t) * kMsRounds + r];
        for (uint32_t lane = 0; lane < 64; lane++) {
          if (!((word >> lane) & 1)) continue;
          const uint32_t s = t * kMsTile + r * 64 + lane;
          if (step == XE_MO_GROUP_LOCATE) {
            if (mg_locate_item(o, s)) o.ctr[kMoNew]++;
          } else {
            const uint32_t ds = mg_slot_of(o, s, mo_find);
            if (ds != kMoAbsent) mg_add_item(o, ds, 1, mg_measure(o, o.sbase + s));
          }
        }
      }
    return 0;
  }
  if (step == XE_MO_GROUP_UNDO || step == XE_MO_GROUP_PUBLISH) {  // over the destination table
    if (o.dst.kind != XE_DM_HASH) return 0;
    for (uint32_t ds = 0; ds < o.dst.cap; ds++) {
      if (step == XE_MO_GROUP_UNDO) mg_undo_item(o, ds);
      else if (mg_claimed(o, ds)) mg_publish_item(o, ds, 0, 1);
    }
    if (step == XE_MO_GROUP_PUBLISH) mg_publish_count(o);
    return 0;
  }
  if (step == XE_MO_COMPACT_MARK) {  // the tile counts are the tombstones, the free records go to the counters
    sim_tile_words(tiles, slots([&](uint32_t s) { return mc_mark_item(o, s); }),
                   [&](uint32_t t, Words w1, Words w2, uint32_t c1, uint32_t c2) { put(t, w1, w2, c2), o.ctr[kMcFree] += c1; });
    return 0;
  }
  if (step == XE_MO_COMPACT_REBUILD) {
    for (uint32_t s = 0; s < o.nslots; s++) {
      if (!mc_run_start(o, s)) continue;
      uint32_t first = 0;
      const uint32_t len = mc_run_scan(o, s, &first);
      if (!mc_run_counts(o, len, first)) continue;
      for (uint32_t j = first; j < len; j++) {
        const uint32_t q = mc_target(o, s, j);
        if (q < j) o.ctr[kMcMoved]++;
        mc_apply(o, s, j, q, 0, 1);
      }
    }
    return 0;
  }
  if (step == XE_MO_LRU_SORT) {
    std::vector<uint32_t> idx(o.n);
    for (uint32_t j = 0; j < o.n; j++) idx[j] = j;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return o.l_keys[a] < o.l_keys[b]; });
    for (uint32_t j = 0; j < o.n; j++) o.l_keys2[j] = o.l_keys[idx[j]], o.l_slot2[j] = o.slot[idx[j]];
    return 0;
  }
  if (step == XE_MO_MODIFY_TILE) {
    for (uint32_t s = 0; s < o.nslots; s++)
      if (ms_select_item(o, s)) mm_modify_item(o, o.sbase + s, 0, 1, false), o.ctr[kMoMatched]++;
    return 0;
  }
  for (uint32_t i = 0; i < o.n; i++) {
    switch (step) {
      case XE_MO_LOOKUP_FIND: mo_find_finish(o, i, mo_slot_of(o, i, mo_find), true); break;
      case XE_MO_LOOKUP_VALUE: mo_lookup_value_item(o, i, 0, 1); break;
      case XE_MO_UPDATE_LOCATE: if (mo_update_locate_item(o, i)) o.ctr[kMoNew]++; break;
      case XE_MO_UPDATE_UNDO: mo_update_undo_item(o, i); break;
      case XE_MO_UPDATE_MARK: mo_update_mark_item(o, i); break;
      case XE_MO_UPDATE_COPY: mo_update_copy_item(o, i, 0, 1); break;
      case XE_MO_DELETE_FIND: mo_find_finish(o, i, mo_slot_of(o, i, mo_find), false); break;
      case XE_MO_DELETE_CLAIM: mo_delete_claim_item(o, i); break;
      case XE_MO_DELETE_ZERO: mo_delete_zero_item(o, i, 0, 1); break;
      case XE_MO_SCAN_COPY: ms_copy_item(o, i, 0, 1); break;
      case XE_MO_SCAN_EXPIRE: ms_expire_item(o, i, 0, 1); break;
      case XE_MO_MODIFY_EDIT: mm_modify_item(o, o.slot[i], 0, 1, false); break;
      case XE_MO_MODIFY_MARK: mm_mark_item(o, i); break;
      case XE_MO_MODIFY_KEYED: mm_keyed_item(o, i, 0, 1); break;
      case XE_MO_JOIN_VALUE: mj_value_item(o, i, 0, 1, mo_find); break;
      case XE_MO_LRU_TOUCH: ml_touch_item(o, i); break;
      case XE_MO_LRU_CLAIM: if (ml_claim_item(o, i)) o.ctr[kMoGone]++; break;
      case XE_MO_LRU_ERASE: ml_erase_item(o, i); break;
      case XE_MO_LRU_RANK: ml_rank_item(o, i); break;
      default: return -1;
    }
  }
  return 0;
}
#endif
#endif  // XE_MAPOPS_H
