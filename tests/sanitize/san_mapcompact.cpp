// san_mapcompact.cpp — TEST INFRASTRUCTURE: a stand-alone program that drives the host-simulation loops of the
// device-side tombstone compaction (gobpfld_amd/csrc/xe_mapops.h: COMPACT_MARK, the scan's SCAN,
// COMPACT_REBUILD) in a library built with -fsanitize=address,undefined: runs placed by hand in tables of 16, 64,
// 128 and 512 slots (across a bitmap word, across a tile, through the table's end with the tombstone on either
// side of it, from slot 0, with the tombstone first and last), small and large values, and runs of exactly
// kMcMaxRun slots, of one more (through the host) and a table without a free record. The image a call leaves
// (xe_map_state_export; device addresses are host addresses in this library) is compared byte for byte with a
// rebuild computed here: every run that holds a tombstone cleared and its entries inserted again in run order.
// A sanitizer report aborts the process.
//
//   san_mapcompact <hostsim.so> <kMcMaxRun>
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/xdpemu.h"

namespace {

#define NEED(name) \
  decltype(&xe_##name) name = reinterpret_cast<decltype(&xe_##name)>(dlsym(h, "xe_" #name)); \
  if (!name) { fprintf(stderr, "missing symbol xe_%s\n", #name); return 3; }

int g_bad = 0;
void check(bool ok, const char* what, int line) {
  if (!ok) { fprintf(stderr, "FAILED line %d: %s\n", line, what); g_bad++; }
}
#define CHECK(x) check((x), #x, __LINE__)

using Bytes = std::vector<uint8_t>;
constexpr uint32_t kFull = 1, kVlen0 = 2, kTomb = 4;  // word 0 of a record

decltype(&xe_map_state_bytes) g_bytes;
decltype(&xe_map_state_export) g_export;
decltype(&xe_map_state_import) g_import;
decltype(&xe_map_compact) g_compact;
decltype(&xe_map_update_batch_staged) g_update;
decltype(&xe_map_delete_batch) g_delete;
decltype(&xe_debug_map_traffic) g_traffic;

// the hash of a key's zero-padded words, restated (8-byte keys here: one word)
uint64_t hash8(uint64_t key) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t(8) * 0xC2B2AE3D27D4EB4Full);
  h ^= key;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 32;
  h ^= h >> 29;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 32;
  return h;
}
uint32_t home(uint64_t key, uint32_t cap) { return uint32_t(hash8(key)) & (cap - 1); }

// An 8-byte-key HASH map's image: [values][cap + 1 records of 2 words][count u32, pad]
struct Table {
  uint32_t cap, vs;
  uint64_t vals_alloc;
  Bytes img;
  uint64_t* rec(uint32_t s) { return reinterpret_cast<uint64_t*>(img.data() + vals_alloc) + uint64_t(s) * 2; }
  uint8_t* val(uint32_t s) { return img.data() + uint64_t(s) * vs; }
};
Table image(xe_vm* vm, int32_t m, uint32_t vs) {
  Table t{};
  uint64_t bytes = 0;
  CHECK(g_bytes(vm, m, &bytes) == 0);
  t.vs = vs;
  for (t.cap = 16;; t.cap <<= 1) {
    t.vals_alloc = ((uint64_t(t.cap) + 1) * vs + 7) & ~uint64_t(7);
    if (t.vals_alloc < 8) t.vals_alloc = 8;
    if (t.vals_alloc + (uint64_t(t.cap) + 1) * 16 + 8 >= bytes) break;
  }
  CHECK(t.vals_alloc + (uint64_t(t.cap) + 1) * 16 + 8 == bytes);
  t.img.assign(bytes, 0);
  CHECK(g_export(vm, m, t.img.data(), nullptr) == 0);
  return t;
}

// `n` slots from slot `first` on (modulo cap) cleared, their entries inserted again in that order. Returns
// the entries that changed slot.
uint64_t rebuild(Table& t, uint32_t first, uint32_t n) {
  struct E { uint32_t slot; uint64_t w0, key; Bytes v; };
  std::vector<E> full;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t s = (first + i) & (t.cap - 1);
    if (t.rec(s)[0] & kFull) full.push_back({s, t.rec(s)[0], t.rec(s)[1], Bytes(t.val(s), t.val(s) + t.vs)});
    t.rec(s)[0] = t.rec(s)[1] = 0;
    memset(t.val(s), 0, t.vs);
  }
  uint64_t moved = 0;
  for (const E& e : full) {
    uint32_t at = home(e.key, t.cap);
    while (t.rec(at)[0] & kFull) at = (at + 1) & (t.cap - 1);
    t.rec(at)[0] = e.w0 & (kFull | kVlen0);
    t.rec(at)[1] = e.key;
    memcpy(t.val(at), e.v.data(), t.vs);
    moved += at != e.slot;
  }
  return moved;
}

// The definition over the image before the call: the image after it and the info.
xe_map_compact_info expect(Table& t, uint32_t max_run) {
  xe_map_compact_info want{};
  std::vector<uint8_t> st(t.cap);  // 0 free, 1 a tombstone, 2 an entry
  uint32_t frees = 0;
  for (uint32_t s = 0; s < t.cap; s++) {
    const uint64_t w0 = t.rec(s)[0];
    st[s] = (w0 & kFull) ? 2 : (w0 & kTomb) ? 1 : 0;
    want.tombstones += st[s] == 1;
    frees += st[s] == 0;
  }
  if (!want.tombstones) return want;
  if (!frees) {
    rebuild(t, 0, t.cap);
    want.longest_run = t.cap;
    want.via_host = 1;
    return want;
  }
  bool long_run = false;
  for (uint32_t s = 0; s < t.cap; s++) {
    if (st[s] == 0 || st[(s - 1) & (t.cap - 1)] != 0) continue;
    uint32_t n = 0;
    bool tomb = false;
    for (; st[(s + n) & (t.cap - 1)] != 0; n++) tomb = tomb || st[(s + n) & (t.cap - 1)] == 1;
    if (!tomb) continue;
    if (n > want.longest_run) want.longest_run = n;
    if (n > max_run) long_run = true;
    else want.moved += rebuild(t, s, n);
  }
  if (long_run) {
    rebuild(t, 0, t.cap);
    want.moved = 0;
    want.via_host = 1;
  }
  return want;
}

// COUNT_ONLY, then the call, against the definition.
void compact_and_compare(xe_vm* vm, int32_t m, uint32_t vs, uint32_t max_run, const xe_map_compact_info* must = nullptr) {
  Table before = image(vm, m, vs), model = before;
  const xe_map_compact_info want = expect(model, max_run);
  if (must) CHECK(want.tombstones == must->tombstones && want.moved == must->moved && want.longest_run == must->longest_run && want.via_host == must->via_host);
  uint64_t up0 = 0, down0 = 0, up1 = 0, down1 = 0;
  CHECK(g_traffic(vm, m, &up0, &down0) == 0);
  xe_map_compact_info got;
  memset(&got, 0xEE, sizeof got);
  CHECK(g_compact(vm, m, XE_MC_COUNT_ONLY, &got, nullptr) == 0);
  CHECK(got.tombstones == want.tombstones && got.moved == 0 && got.longest_run == want.longest_run && got.via_host == 0);
  CHECK(image(vm, m, vs).img == before.img);
  memset(&got, 0xEE, sizeof got);
  CHECK(g_compact(vm, m, 0, &got, nullptr) == 0);
  CHECK(got.tombstones == want.tombstones && got.moved == want.moved && got.longest_run == want.longest_run && got.via_host == want.via_host);
  CHECK(g_traffic(vm, m, &up1, &down1) == 0);
  CHECK(up1 == up0 + want.via_host && down1 == down0 + want.via_host);
  CHECK(image(vm, m, vs).img == model.img);
  memset(&got, 0xEE, sizeof got);
  CHECK(g_compact(vm, m, 0, &got, nullptr) == 0);
  CHECK(got.tombstones == 0 && got.moved == 0 && got.longest_run == 0 && got.via_host == 0);
}

// The next key (a counter) whose home in a table of cap slots is `want`.
uint64_t g_counter = 1;
uint64_t key_at(uint32_t cap, uint32_t want) {
  while (home(g_counter, cap) != want) g_counter++;
  return g_counter++;
}

// A run placed by hand: entry i has its home at offset hoff[i] <= i of the run and is installed alone, after the
// entries in front of it: it lands at offset i. The entries listed in `dead` are deleted again.
struct Run { uint32_t first; std::vector<uint32_t> hoff, dead; };
void place(xe_vm* vm, int32_t m, uint32_t cap, uint32_t vs, const std::vector<Run>& runs) {
  std::vector<uint64_t> gone;
  for (const Run& r : runs) {
    for (size_t i = 0; i < r.hoff.size(); i++) {
      const uint64_t k = key_at(cap, (r.first + r.hoff[i]) & (cap - 1));
      Bytes v(vs);  // a heap block of exactly the value's size
      for (uint32_t b = 0; b < vs; b++) v[b] = uint8_t(1 + (k * 31 + b) % 255);
      CHECK(g_update(vm, m, &k, v.data(), 1) == 0);
      for (uint32_t d : r.dead)
        if (d == i) gone.push_back(k);
    }
  }
  CHECK(g_delete(vm, m, gone.data(), gone.size(), nullptr) == 0);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s hostsim.so kMcMaxRun\n", argv[0]); return 2; }
  const uint32_t max_run = uint32_t(atoi(argv[2]));
  void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "dlopen %s: %s\n", argv[1], dlerror()); return 3; }
  NEED(default_settings) NEED(create) NEED(destroy) NEED(add_map) NEED(map_state_bytes) NEED(map_state_export) NEED(map_state_import)
  NEED(map_compact) NEED(map_update_batch_staged) NEED(map_delete_batch) NEED(debug_map_traffic)
  g_bytes = map_state_bytes, g_export = map_state_export, g_import = map_state_import, g_compact = map_compact;
  g_update = map_update_batch_staged, g_delete = map_delete_batch, g_traffic = debug_map_traffic;

  xe_settings s;
  memset(&s, 0, sizeof s);
  default_settings(&s);
  s.engine = 1;
  xe_vm* vm = nullptr;
  if (create(&s, &vm)) return 3;

  // ---- geometry: tables of 16, 64, 128 and 512 slots, values moved by the run's lane (8 bytes) and by sub-groups
  // of lanes (17 and 1025 bytes leave the map's values at every alignment)
  for (uint32_t max_entries : {8u, 32u, 33u, 256u}) {
    const uint32_t cap = max_entries == 8 ? 16 : max_entries == 32 ? 64 : max_entries == 33 ? 128 : 512;
    for (uint32_t vs : {8u, 17u, 1025u}) {
      for (int which = 0; which < 3; which++) {
        xe_map_def def{XE_MAP_HASH, 8, vs, max_entries, 0};
        int32_t m = 0;
        CHECK(add_map(vm, &def, nullptr, 0, &m) == 0);
        std::vector<Run> runs;
        if (which == 0) runs.push_back({cap - 2, {0, 0, 1, 2}, {1}});       // through the end, the tombstone in slot cap - 1
        else if (which == 1) runs.push_back({cap - 2, {0, 0, 1, 2}, {2}});  // ... in slot 0
        else runs.push_back({0, {0, 0, 0}, {0}});                           // from slot 0, slot cap - 1 free
        runs.push_back({5, {0, 0}, {0}});  // the tombstone first
        runs.push_back({9, {0, 0}, {1}});  // ... last
        if (cap >= 128) runs.push_back({61, {0, 0, 1, 1, 3}, {1}});   // across slot 63 -> 64
        if (cap >= 512) runs.push_back({253, {0, 0, 1, 1, 3}, {2}});  // across slot 255 -> 256
        place(vm, m, cap, vs, runs);
        xe_map_compact_info must{};
        must.tombstones = runs.size();
        must.moved = (which == 1 ? 1 : 2) + 1 + (cap >= 128 ? 3 : 0) + (cap >= 512 ? 2 : 0);
        must.longest_run = cap >= 128 ? 5 : which == 2 ? 3 : 4;
        compact_and_compare(vm, m, vs, max_run, &must);
      }
    }
  }

  // ---- tombstones only, and none
  {
    xe_map_def def{XE_MAP_HASH, 8, 24, 64, 0};
    int32_t m = 0;
    CHECK(add_map(vm, &def, nullptr, 0, &m) == 0);
    place(vm, m, 128, 24, {{30, {0, 0, 0, 2, 2}, {}}, {90, {0, 1, 1}, {}}});
    xe_map_compact_info none{};
    compact_and_compare(vm, m, 24, max_run, &none);
    CHECK(add_map(vm, &def, nullptr, 0, &m) == 0);
    place(vm, m, 128, 24, {{30, {0, 0, 0, 2, 2}, {0, 1, 2, 3, 4}}, {90, {0, 1, 1}, {0, 1, 2}}});
    xe_map_compact_info all{};
    all.tombstones = 8, all.longest_run = 5;
    compact_and_compare(vm, m, 24, max_run, &all);
    const Table t = image(vm, m, 24);
    bool zero = true;
    for (uint8_t b : t.img) zero = zero && !b;
    CHECK(zero);
  }

  // ---- long runs in 16,384 slots, written into an image and imported: the first entry at home, every other
  // one slot behind its home, the second one a tombstone: every entry behind it moves up by one
  for (uint32_t vs : {8u, 24u}) {
    for (uint32_t slots : {max_run, max_run + 1}) {
      if (slots + 1 > 8192) continue;
      xe_map_def def{XE_MAP_HASH, 8, vs, 8192, 0};
      int32_t m = 0;
      CHECK(add_map(vm, &def, nullptr, 0, &m) == 0);
      Table t = image(vm, m, vs);
      CHECK(t.cap == 16384);
      const uint32_t first = 1000;
      for (uint32_t j = 0; j < slots; j++) {
        const uint64_t k = key_at(t.cap, first + (j ? j - 1 : 0));
        t.rec(first + j)[0] = j == 1 ? kTomb : kFull;
        t.rec(first + j)[1] = k;
        if (j != 1)
          for (uint32_t b = 0; b < vs; b++) t.val(first + j)[b] = uint8_t(1 + (k + b) % 255);
      }
      const uint32_t count = slots - 1;
      memcpy(t.img.data() + t.img.size() - 8, &count, 4);
      CHECK(g_import(vm, m, t.img.data(), nullptr) == 0);
      xe_map_compact_info must{};
      must.tombstones = 1, must.longest_run = slots, must.via_host = slots > max_run, must.moved = must.via_host ? 0 : slots - 2;
      compact_and_compare(vm, m, vs, max_run, &must);
    }
  }

  // ---- no free record: three entries and 125 tombstones in 128 slots
  {
    xe_map_def def{XE_MAP_HASH, 8, 8, 64, 0};
    int32_t m = 0;
    CHECK(add_map(vm, &def, nullptr, 0, &m) == 0);
    uint64_t k = 1000000;
    for (uint32_t round : {3u, 61u, 61u, 3u}) {
      std::vector<uint64_t> keys(round), vals(round);
      for (uint32_t i = 0; i < round; i++) keys[i] = k++, vals[i] = keys[i] * 7 + 1;
      CHECK(g_update(vm, m, keys.data(), vals.data(), round) == 0);
      if (round != 3 || k > 1000100) CHECK(g_delete(vm, m, keys.data(), round, nullptr) == 0);
    }
    xe_map_compact_info must{};
    must.tombstones = 125, must.longest_run = 128, must.via_host = 1;
    compact_and_compare(vm, m, 8, max_run, &must);
  }

  destroy(vm);
  printf("san_mapcompact: %d failed checks\n", g_bad);
  return g_bad ? 1 : 0;
}
