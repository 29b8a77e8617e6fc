// san_maptop.cpp — TEST INFRASTRUCTURE: a stand-alone program that drives the host-simulation loops of the
// map top-K, evict and statistics (gobpfld_amd/csrc/xe_mapops.h: PREFIX, PICK, CUT, TRIM, STATS and the scan's
// steps) in a library built with -fsanitize=address,undefined. Every output buffer is a heap block of exactly
// the r entries the call may write, placed at an odd address inside it where the case says so, so a byte too
// many is a sanitizer report; the order field and the filter's field sit at odd offsets of odd-sized values.
// What the calls report is compared with xe_map_scan_device's entries (slot order) ranked here. A sanitizer
// report aborts the process.
//
//   san_maptop <hostsim.so>
#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
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

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s hostsim.so\n", argv[0]); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "dlopen %s: %s\n", argv[1], dlerror()); return 3; }
  NEED(default_settings) NEED(create) NEED(destroy) NEED(add_map) NEED(map_update) NEED(map_delete_batch) NEED(map_scan_device)
  NEED(map_top_device) NEED(map_evict_device) NEED(map_top) NEED(map_evict) NEED(map_stats) NEED(map_count)

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
  uint32_t seed = 54321;
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
      v[3] &= 3;  // the 1-byte order field: runs of ties
      CHECK(map_update(vm, m, k.data(), v.data()) == 0);
      keys.push_back(Bytes(k.begin(), k.begin() + ks));
    }
    if (!array && g.ks && g.n >= 9) {  // every third entry deleted on the device copy: live tombstones
      Bytes dk;
      for (uint32_t i = 0; i < g.n; i += 3) dk.insert(dk.end(), keys[i].begin(), keys[i].end());
      CHECK(map_delete_batch(vm, m, dk.data(), dk.size() / ks, nullptr) == 0);
    }
    const xe_map_filter filters[] = {{XE_MF_ALL, 0, 0, 0, 0}, {XE_MF_ANYBITS, 1, 4, 0, 0x01010101}, {XE_MF_GT, 0, 1, 0, 0xfff}};
    const xe_map_order orders[] = {{3, 1, 1, 0}, {3, 1, 0, 0}, {1, 2, 0, 0}, {5, 4, 1, 0}, {g.vs - 8, 8, 1, 0}, {3, 8, 0, 0}};
    for (int round = 0; round < 2; round++) {  // a top of every filter and order; then an evict of each
      for (const xe_map_filter& f : filters) {
        for (const xe_map_order& o : orders) {
          // the truth: the scan's entries (slot order), ranked here by a stable sort
          uint64_t n = 0;
          CHECK(map_scan_device(vm, m, &f, nullptr, nullptr, 0, &n, nullptr) == 0);
          Bytes sk(n * ks + 1), sv(n * g.vs + 1);
          CHECK(map_scan_device(vm, m, &f, sk.data(), sv.data(), n, &n, nullptr) == 0);
          std::vector<uint64_t> fld(n);
          for (uint64_t i = 0; i < n; i++) fld[i] = field(&sv[i * g.vs], o.offset, o.width);
          std::vector<uint32_t> rank(n);
          std::iota(rank.begin(), rank.end(), 0u);
          std::stable_sort(rank.begin(), rank.end(), [&](uint32_t a, uint32_t b) { return o.descending ? fld[a] > fld[b] : fld[a] < fld[b]; });
          struct xe_map_stats st;
          CHECK(map_stats(vm, m, &f, &o, &st, nullptr) == 0);
          uint64_t sum = 0, mn = ~uint64_t(0), mx = 0;
          for (uint64_t x : fld) sum += x, mn = std::min(mn, x), mx = std::max(mx, x);
          CHECK(st.count == n && st.sum == sum && st.min == mn && st.max == mx);
          const bool evict = round == 1 && !array;
          bool evicted = false;
          for (uint64_t k : {uint64_t(0), uint64_t(1), n / 2, n + 5}) {
            const uint64_t r = std::min(k, n);
            for (uint32_t shift : {0u, 1u}) {
              if (evict && (evicted || k != n / 2)) continue;  // one evict per filter and order: half of the matches
              evicted = evict;
              std::vector<uint32_t> want(rank.begin(), rank.begin() + r);
              std::sort(want.begin(), want.end());
              // exactly r entries of room, `shift` bytes into the block
              uint8_t* kb = static_cast<uint8_t*>(malloc(std::max<size_t>(r * ks + shift, 1)));
              uint8_t* vb = static_cast<uint8_t*>(malloc(std::max<size_t>(r * g.vs + shift, 1)));
              uint64_t got = 0, cut = 77;
              int rc;
              if (evict && (k & 1)) rc = map_evict(vm, m, &f, &o, kb + shift, vb + shift, k, &got, &cut);
              else if (evict) rc = map_evict_device(vm, m, &f, &o, kb + shift, vb + shift, k, &got, &cut, nullptr);
              else if (shift) rc = map_top(vm, m, &f, &o, kb + shift, vb + shift, k, &got, &cut);
              else rc = map_top_device(vm, m, &f, &o, kb + shift, vb + shift, k, &got, &cut, nullptr);
              CHECK(rc == 0);
              CHECK(got == n);
              CHECK(cut == (r ? fld[rank[r - 1]] : 0));
              for (uint64_t i = 0; i < r; i++) {
                CHECK(!ks || !memcmp(kb + shift + i * ks, &sk[size_t(want[i]) * ks], ks));
                CHECK(!memcmp(vb + shift + i * g.vs, &sv[size_t(want[i]) * g.vs], g.vs));
              }
              free(kb);
              free(vb);
              if (evict) {
                uint64_t left = 0, live = 0;
                CHECK(map_scan_device(vm, m, &f, nullptr, nullptr, 0, &left, nullptr) == 0);
                CHECK(left == n - r);
                CHECK(map_count(vm, m, &live) == 0);
              }
            }
          }
        }
      }
    }
  }
  destroy(vm);
  printf("san_maptop: %d failed checks\n", g_bad);
  return g_bad ? 1 : 0;
}
