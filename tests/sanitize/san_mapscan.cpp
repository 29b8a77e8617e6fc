// san_mapscan.cpp — TEST INFRASTRUCTURE: a stand-alone program that drives the host-simulation loops of the
// map scan and expire (gobpfld_amd/csrc/xe_mapops.h: SELECT, SCAN, SCATTER, COPY, EXPIRE) in a library built
// with -fsanitize=address,undefined. Every output buffer is a heap block of exactly the bytes the call may
// write, placed at an odd address inside it where the case says so, so a byte too many is a sanitizer
// report; the field of the filter sits at an odd offset of an odd-sized value. What the calls report is
// compared with xe_map_dump filtered here. A sanitizer report aborts the process.
//
//   san_mapscan <hostsim.so>
#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
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

uint64_t field(const uint8_t* v, uint32_t off, uint32_t width) {
  uint64_t f = 0;
  for (uint32_t b = 0; b < width; b++) f |= uint64_t(v[off + b]) << (8 * b);
  return f;
}
bool selects(const xe_map_filter& f, const uint8_t* v) {
  const uint64_t x = f.op == XE_MF_ALL ? 0 : field(v, f.offset, f.width), o = f.operand;
  switch (f.op) {
    case XE_MF_ALL: return true;
    case XE_MF_EQ: return x == o;
    case XE_MF_NE: return x != o;
    case XE_MF_LT: return x < o;
    case XE_MF_LE: return x <= o;
    case XE_MF_GT: return x > o;
    case XE_MF_GE: return x >= o;
    case XE_MF_ANYBITS: return (x & o) != 0;
    default: return (x & o) == 0;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s hostsim.so\n", argv[0]); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "dlopen %s: %s\n", argv[1], dlerror()); return 3; }
  NEED(default_settings) NEED(create) NEED(destroy) NEED(add_map) NEED(map_update) NEED(map_dump)
  NEED(map_delete_batch) NEED(map_scan_device) NEED(map_expire_device) NEED(map_scan) NEED(map_expire) NEED(map_count)

  xe_settings s;
  memset(&s, 0, sizeof s);
  default_settings(&s);
  s.engine = 1;
  xe_vm* vm = nullptr;
  if (create(&s, &vm)) return 3;

  struct Geo { uint32_t type, ks, vs, max, n; };
  // key and value sizes on both sides of the record and sub-group cuts; 300 entries: two tiles of a 1,024-slot table
  const Geo geos[] = {{XE_MAP_HASH, 13, 13, 300, 300}, {XE_MAP_HASH, 8, 17, 64, 40}, {XE_MAP_HASH, 25, 65, 64, 40},
                      {XE_MAP_HASH, 0, 24, 8, 1},      {XE_MAP_ARRAY, 4, 13, 300, 150}, {XE_MAP_HASH, 64, 1025, 16, 9}};
  uint32_t seed = 12345;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return uint8_t(seed >> 24); };
  for (const Geo& g : geos) {
    const bool array = g.type == XE_MAP_ARRAY;
    xe_map_def def{g.type, g.ks, g.vs, g.max, 0};
    int32_t m = 0;
    CHECK(add_map(vm, &def, nullptr, 0, &m) == 0);
    const uint32_t ks = array ? 4 : g.ks;
    std::vector<Bytes> keys;
    for (uint32_t i = 0; i < g.n; i++) {
      Bytes k(std::max<uint32_t>(ks, 4), 0), v(g.vs);
      if (array) { const uint32_t idx = i * 2; memcpy(k.data(), &idx, 4); }
      else for (uint32_t b = 0; b < ks; b++) k[b] = b < 4 ? uint8_t(i >> (8 * b)) : rnd();
      for (auto& b : v) b = rnd();
      CHECK(map_update(vm, m, k.data(), v.data()) == 0);
      keys.push_back(Bytes(k.begin(), k.begin() + ks));
    }
    if (!array && g.ks && g.n >= 9) {  // every third entry deleted on the device copy: live tombstones
      Bytes dk;
      for (uint32_t i = 0; i < g.n; i += 3) dk.insert(dk.end(), keys[i].begin(), keys[i].end());
      CHECK(map_delete_batch(vm, m, dk.data(), dk.size() / ks, nullptr) == 0);
    }
    const uint32_t width = g.vs >= 12 ? 8 : 4, off = g.vs >= 12 ? 3 : 1;  // an odd offset: never aligned for every slot
    const xe_map_filter filters[] = {{XE_MF_ALL, 0, 0, 0, 0},
                                     {XE_MF_ANYBITS, off, width, 0, 0x0101},
                                     {XE_MF_LT, g.vs - 1, 1, 0, 0x80},
                                     {XE_MF_GE, g.vs - width, width, 0, uint64_t(1) << (8 * width - 1)}};
    for (int round = 0; round < 2; round++) {  // a scan of every filter; then an expire of every filter
      for (const xe_map_filter& f : filters) {
        // the truth: xe_map_dump, filtered here
        uint64_t cnt = 0;
        CHECK(map_dump(vm, m, nullptr, nullptr, 0, &cnt) == 0);
        std::map<Bytes, Bytes> want;
        if (array) {
          Bytes raw(size_t(g.vs) * g.max + 1);
          CHECK(map_dump(vm, m, raw.data(), nullptr, cnt, &cnt) == 0);
          for (uint32_t i = 0; i < g.max; i++)
            if (selects(f, &raw[size_t(i) * g.vs])) {
              Bytes k(4);
              memcpy(k.data(), &i, 4);
              want[k] = Bytes(&raw[size_t(i) * g.vs], &raw[size_t(i + 1) * g.vs]);
            }
        } else {
          Bytes dk(cnt * ks + 1), dv(cnt * g.vs + 1);
          CHECK(map_dump(vm, m, dk.data(), dv.data(), cnt, &cnt) == 0);
          for (uint64_t i = 0; i < cnt; i++)
            if (selects(f, &dv[i * g.vs])) want[Bytes(&dk[i * ks], &dk[i * ks] + ks)] = Bytes(&dv[i * g.vs], &dv[(i + 1) * g.vs]);
        }
        const bool expire = round == 1 && !array;
        uint64_t matched = 0;
        bool expired = false;
        CHECK(map_scan_device(vm, m, &f, nullptr, nullptr, 0, &matched, nullptr) == 0);  // count only
        CHECK(matched == want.size());
        for (uint64_t cap : {uint64_t(1), uint64_t(want.size() / 2), uint64_t(want.size()) + 5}) {
          const uint64_t r = std::min<uint64_t>(cap, want.size());
          for (uint32_t shift : {0u, 1u}) {
            if (expire && (expired || cap != want.size() / 2)) continue;  // one expire per filter: half of its matches
            expired = expire;
            // exactly r entries of room, `shift` bytes into the block
            uint8_t* kb = static_cast<uint8_t*>(malloc(std::max<size_t>(r * ks + shift, 1)));
            uint8_t* vb = static_cast<uint8_t*>(malloc(std::max<size_t>(r * g.vs + shift, 1)));
            uint64_t got = 0;
            int rc;
            if (expire && (cap & 1)) rc = map_expire(vm, m, &f, kb + shift, vb + shift, cap, &got);
            else if (expire) rc = map_expire_device(vm, m, &f, kb + shift, vb + shift, cap, &got, nullptr);
            else if (shift) rc = map_scan(vm, m, &f, kb + shift, vb + shift, cap, &got);
            else rc = map_scan_device(vm, m, &f, kb + shift, vb + shift, cap, &got, nullptr);
            CHECK(rc == 0);
            CHECK(got == want.size());
            std::map<Bytes, Bytes> seen;
            for (uint64_t i = 0; i < r; i++)
              seen[Bytes(kb + shift + i * ks, kb + shift + (i + 1) * ks)] = Bytes(vb + shift + i * g.vs, vb + shift + (i + 1) * g.vs);
            CHECK(seen.size() == r || ks == 0);
            for (auto& e : seen) {
              auto it = want.find(e.first);
              CHECK(it != want.end() && it->second == e.second);
            }
            free(kb);
            free(vb);
            if (expire) {
              uint64_t left = 0, live = 0;
              CHECK(map_scan_device(vm, m, &f, nullptr, nullptr, 0, &left, nullptr) == 0);
              CHECK(left == want.size() - r);
              CHECK(map_count(vm, m, &live) == 0 && live == cnt - r);
            }
          }
        }
      }
    }
  }
  destroy(vm);
  printf("san_mapscan: %d failed checks\n", g_bad);
  return g_bad ? 1 : 0;
}
