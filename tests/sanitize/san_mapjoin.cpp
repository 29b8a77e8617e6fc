// san_mapjoin.cpp — TEST INFRASTRUCTURE: a stand-alone program that drives the host-simulation loops of the
// device-side join (gobpfld_amd/csrc/xe_mapops.h: JOIN_SELECT, then the scan's SCAN, SCATTER and COPY, JOIN_VALUE
// and EXPIRE) in a library built with -fsanitize=address,undefined: join bytes at odd offsets of keys and
// odd-sized values, other maps of every record size and value sub-group width, outputs in heap blocks of exactly
// r entries with cap_entries below, at and above matched, removal, and a map joined with itself. Every answer is
// compared with a join of the two maps' scanned entries computed here. A sanitizer report aborts the process.
//
//   san_mapjoin <hostsim.so>
#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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

decltype(&xe_map_scan_device) g_scan;
decltype(&xe_map_join_device) g_join;

struct Map {
  int32_t idx;
  bool array;
  uint32_t ks, vs, max_entries;  // (ks: 4 for an ARRAY)
};

// Every entry of map m in scan order, in heap blocks of exactly their size.
uint64_t scan_all(xe_vm* vm, const Map& m, Bytes& k, Bytes& v) {
  uint64_t n = 0;
  CHECK(g_scan(vm, m.idx, nullptr, nullptr, nullptr, 0, &n, nullptr) == 0);
  k.assign(n * m.ks, 0);
  v.assign(n * m.vs, 0);
  CHECK(g_scan(vm, m.idx, nullptr, n ? k.data() : nullptr, n ? v.data() : nullptr, n, &n, nullptr) == 0);
  return n;
}

// One join of src against other, checked against the two maps' scanned entries; the outputs are heap blocks of
// exactly r entries (one byte for r = 0), so a byte written past entry r is a heap overflow. Returns matched.
uint64_t join(xe_vm* vm, const Map& src, const Map& other, xe_map_join_spec j, uint64_t cap, bool outputs = true) {
  Bytes sk, sv, ok, ov;
  const uint64_t n = scan_all(vm, src, sk, sv);
  std::map<Bytes, Bytes> have;  // the other map: key bytes -> value
  if (!other.array) {
    const uint64_t on = scan_all(vm, other, ok, ov);
    for (uint64_t i = 0; i < on; i++) have[Bytes(&ok[i * other.ks], &ok[i * other.ks] + other.ks)] = Bytes(&ov[i * other.vs], &ov[i * other.vs] + other.vs);
  } else {
    scan_all(vm, other, ok, ov);
  }
  Bytes wk, wv, wo;
  uint64_t want = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t* from = (j.from == XE_MG_KEY ? &sk[i * src.ks] : &sv[i * src.vs]) + j.offset;
    const uint8_t* hit = nullptr;
    if (other.array) {
      uint64_t index = 0;
      for (uint32_t b = 0; b < j.len; b++) index |= uint64_t(from[b]) << (8 * b);
      if (index < other.max_entries) hit = &ov[index * other.vs];
    } else {
      const auto it = have.find(Bytes(from, from + j.len));
      if (it != have.end()) hit = it->second.data();
    }
    if ((hit != nullptr) != (j.mode == XE_MJ_PRESENT)) continue;
    want++;
    if (want > cap) continue;
    wk.insert(wk.end(), &sk[i * src.ks], &sk[i * src.ks] + src.ks);
    wv.insert(wv.end(), &sv[i * src.vs], &sv[i * src.vs] + src.vs);
    Bytes o(other.vs, 0);
    if (hit) memcpy(o.data(), hit, other.vs);
    wo.insert(wo.end(), o.begin(), o.end());
  }
  const uint64_t r = std::min(want, cap);
  Bytes gk(std::max<size_t>(r * src.ks, 1)), gv(std::max<size_t>(r * src.vs, 1)), go(std::max<size_t>(r * other.vs, 1));
  uint64_t matched = 7, selected = 7;
  CHECK(g_join(vm, src.idx, nullptr, &j, other.idx, outputs ? gk.data() : nullptr, outputs ? gv.data() : nullptr,
               outputs ? go.data() : nullptr, cap, &matched, &selected, nullptr) == 0);
  CHECK(matched == want);
  CHECK(selected == n);
  if (outputs && r) {
    CHECK(!memcmp(gk.data(), wk.data(), r * src.ks));
    CHECK(!memcmp(gv.data(), wv.data(), r * src.vs));
    CHECK(!memcmp(go.data(), wo.data(), r * other.vs));
  }
  if (j.flags & XE_MJ_REMOVE) {  // exactly the r reported entries are gone
    Bytes ak, av;
    CHECK(scan_all(vm, src, ak, av) == n - r);
    uint64_t p = 0;
    for (uint64_t i = 0, q = 0; i < n; i++) {
      const bool gone = q < r && !memcmp(&sk[i * src.ks], &wk[q * src.ks], src.ks);
      if (gone) { q++; continue; }
      CHECK(p < n - r && !memcmp(&ak[p * src.ks], &sk[i * src.ks], src.ks) && !memcmp(&av[p * src.vs], &sv[i * src.vs], src.vs));
      p++;
    }
  }
  return matched;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s hostsim.so\n", argv[0]); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "dlopen %s: %s\n", argv[1], dlerror()); return 3; }
  NEED(default_settings) NEED(create) NEED(destroy) NEED(add_map) NEED(map_update) NEED(map_delete_batch) NEED(map_scan_device)
  NEED(map_join_device) NEED(map_join)
  g_scan = map_scan_device;
  g_join = map_join_device;

  xe_settings s;
  memset(&s, 0, sizeof s);
  default_settings(&s);
  s.engine = 1;
  xe_vm* vm = nullptr;
  if (create(&s, &vm)) return 3;
  uint32_t seed = 24680;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return uint8_t(seed >> 24); };
  auto add = [&](uint32_t type, uint32_t ks, uint32_t vs, uint32_t entries) {
    xe_map_def def{type, ks, vs, entries, 0};
    int32_t idx = -1;
    CHECK(add_map(vm, &def, nullptr, 0, &idx) == 0);
    return Map{idx, type == XE_MAP_ARRAY, type == XE_MAP_ARRAY ? 4u : ks, vs, entries};
  };

  // ---- join shapes: a 64-byte key and a 73-byte value; other maps of every record size and sub-group width
  {
    const uint32_t sks = 64, svs = 73, n = 330;  // more than a tile of live entries
    const Map src = add(XE_MAP_HASH, sks, svs, 512);
    Bytes gone, all_k, all_v;
    for (uint32_t i = 0; i < n; i++) {
      Bytes k(sks), v(svs);
      for (auto& b : k) b = uint8_t(rnd() % 3);  // few values per byte: the short shapes repeat, the long ones do not
      for (auto& b : v) b = uint8_t(rnd() % 3);
      memcpy(&k[40], &i, 4);  // distinct keys (outside the join bytes of the short shapes)
      CHECK(map_update(vm, src.idx, k.data(), v.data()) == 0);
      if (i % 5 == 0) gone.insert(gone.end(), k.begin(), k.end());
      else all_k.insert(all_k.end(), k.begin(), k.end()), all_v.insert(all_v.end(), v.begin(), v.end());
    }
    CHECK(map_delete_batch(vm, src.idx, gone.data(), gone.size() / sks, nullptr) == 0);  // live tombstones
    const uint32_t live = uint32_t(all_k.size() / sks);
    struct Shape { uint32_t from, off, len; };
    const Shape shapes[] = {{XE_MG_KEY, 0, 4}, {XE_MG_KEY, 1, 3}, {XE_MG_KEY, 3, 13}, {XE_MG_KEY, 0, 64}, {XE_MG_VALUE, 2, 8},
                            {XE_MG_VALUE, 1, 3}, {XE_MG_VALUE, 5, 4}, {XE_MG_VALUE, 3, 13}, {XE_MG_VALUE, 7, 24}, {XE_MG_VALUE, 1, 64}};
    const uint32_t ovss[] = {8, 24, 100, 1100};
    uint32_t turn = 0;
    for (const Shape& sh : shapes) {
      const uint32_t ovs = ovss[turn++ % 4];
      const Map other = add(XE_MAP_HASH, sh.len, ovs, 512);
      // every second live entry's join bytes become a key of the other map, and every seventh of those is deleted again
      Bytes dead;
      for (uint32_t i = 0; i < live; i += 2) {
        const uint8_t* from = (sh.from == XE_MG_KEY ? &all_k[i * sks] : &all_v[i * svs]) + sh.off;
        Bytes v(ovs);
        for (auto& b : v) b = uint8_t(rnd() | 1);
        CHECK(map_update(vm, other.idx, from, v.data()) == 0);
        if (i % 14 == 0) dead.insert(dead.end(), from, from + sh.len);
      }
      CHECK(map_delete_batch(vm, other.idx, dead.data(), dead.size() / sh.len, nullptr) == 0);
      for (uint32_t mode : {uint32_t(XE_MJ_PRESENT), uint32_t(XE_MJ_ABSENT)}) {
        const xe_map_join_spec j{sh.from, sh.off, sh.len, mode, 0, 0};
        const uint64_t m = join(vm, src, other, j, ~uint64_t(0), false);  // count only
        CHECK(m <= live);
        for (uint64_t cap : {uint64_t(0), uint64_t(1), m - 1, m, m + 9}) CHECK(join(vm, src, other, j, cap) == m);
      }
    }
    // an ARRAY other map by one, two and four odd bytes; an index at or beyond max_entries is absent
    const Map a1 = add(XE_MAP_ARRAY, 4, 9, 2), a2 = add(XE_MAP_ARRAY, 4, 17, 514), a4 = add(XE_MAP_ARRAY, 4, 8, 1u << 16);
    for (uint32_t i = 0; i < 514; i++) {
      Bytes v(17);
      for (auto& b : v) b = rnd();
      CHECK(map_update(vm, a2.idx, &i, v.data()) == 0);
      if (i < 2) CHECK(map_update(vm, a1.idx, &i, v.data()) == 0);
    }
    for (uint32_t mode : {uint32_t(XE_MJ_PRESENT), uint32_t(XE_MJ_ABSENT)}) {
      CHECK(join(vm, src, a1, xe_map_join_spec{XE_MG_VALUE, 11, 1, mode, 0, 0}, 40) > 0);
      CHECK(join(vm, src, a2, xe_map_join_spec{XE_MG_VALUE, 11, 2, mode, 0, 0}, 40) > 0);
      join(vm, src, a4, xe_map_join_spec{XE_MG_KEY, 41, 4, mode, 0, 0}, 40);
      // an ARRAY source's index bytes
      CHECK(join(vm, a2, a1, xe_map_join_spec{XE_MG_KEY, 0, 2, mode, 0, 0}, 600) == (mode == XE_MJ_PRESENT ? 2u : 512u));
      CHECK(join(vm, a2, a1, xe_map_join_spec{XE_MG_KEY, 1, 1, mode, 0, 0}, 3) == (mode == XE_MJ_PRESENT ? 512u : 2u));
    }
  }

  // ---- removal and the self-join: sessions that name a parent of the same map at an odd offset of their value
  {
    const uint32_t ks = 8, vs = 21, n = 700;
    const Map m = add(XE_MAP_HASH, ks, vs, 1024), block = add(XE_MAP_HASH, 3, 5, 64);
    Bytes gone;
    for (uint32_t i = 0; i < n; i++) {
      const uint64_t key = 0x9E3779B97F4A7C15ull * (i + 1), parent = 0x9E3779B97F4A7C15ull * ((i * 7 + 3) % n + 1);
      uint8_t v[vs];
      for (auto& b : v) b = rnd();
      memcpy(v + 5, &parent, 8);
      v[1] = uint8_t(i % 50), v[2] = 0, v[3] = 1;
      CHECK(map_update(vm, m.idx, &key, v) == 0);
      if (i % 9 == 0) gone.insert(gone.end(), (const uint8_t*)&key, (const uint8_t*)&key + 8);
    }
    CHECK(map_delete_batch(vm, m.idx, gone.data(), gone.size() / ks, nullptr) == 0);
    for (uint8_t b : {uint8_t(3), uint8_t(17), uint8_t(49)}) {
      const uint8_t k[3] = {b, 0, 1}, v[5] = {1, 2, 3, 4, 5};
      CHECK(map_update(vm, block.idx, k, v) == 0);
    }
    const xe_map_join_spec parent_gone{XE_MG_VALUE, 5, 8, XE_MJ_ABSENT, 0, 0}, parent_there{XE_MG_VALUE, 5, 8, XE_MJ_PRESENT, 0, 0};
    const uint64_t orphans = join(vm, m, m, parent_gone, 10);
    CHECK(orphans > 0 && join(vm, m, m, parent_there, ~uint64_t(0)) + orphans == n - gone.size() / ks);
    // a blocklist: the first five, then silently three more, then the rest
    xe_map_join_spec blocked{XE_MG_VALUE, 1, 3, XE_MJ_PRESENT, XE_MJ_REMOVE, 0};
    const uint64_t b0 = join(vm, m, block, blocked, 5);
    CHECK(b0 > 8 && join(vm, m, block, blocked, 3, false) == b0 - 5);
    CHECK(join(vm, m, block, blocked, ~uint64_t(0)) == b0 - 8);
    CHECK(join(vm, m, block, blocked, ~uint64_t(0)) == 0);
    // the orphans removed from the map they are looked up in, until none is left
    xe_map_join_spec collect = parent_gone;
    collect.flags = XE_MJ_REMOVE;
    for (int round = 0; round < 100 && join(vm, m, m, collect, ~uint64_t(0)); round++) {}
    CHECK(join(vm, m, m, parent_gone, 0) == 0);
    // the host-pointer form takes the same arguments
    uint64_t matched = 0, selected = 0;
    Bytes k(8), v(vs), o(vs);
    CHECK(map_join(vm, m.idx, nullptr, &parent_there, m.idx, k.data(), v.data(), o.data(), 1, &matched, &selected) == 0);
    CHECK(matched == selected);
  }
  destroy(vm);
  printf("san_mapjoin: %d failed checks\n", g_bad);
  return g_bad ? 1 : 0;
}
