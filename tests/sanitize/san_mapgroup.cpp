// san_mapgroup.cpp — TEST INFRASTRUCTURE: a stand-alone program that drives the host-simulation loops of the
// device-side group-by (gobpfld_amd/csrc/xe_mapops.h: GROUP_LOCATE, UNDO, PUBLISH, ADD after the scan's SELECT
// and SCAN) in a library built with -fsanitize=address,undefined: group bytes and measures at odd offsets of
// keys and odd-sized values (the key-shape cases), and destinations with exactly enough room, and one entry too
// little, for the groups that are new (the claim cases). What a call leaves in the destination is read back
// with xe_map_scan_device and compared with an aggregate of the source's scanned entries computed here. A
// sanitizer report aborts the process.
//
//   san_mapgroup <hostsim.so>
#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
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
using Sums = std::map<Bytes, std::pair<uint64_t, uint64_t>>;  // group bytes -> (entries, sum of measures)

uint64_t field(const uint8_t* v, uint32_t off, uint32_t width) {
  uint64_t f = 0;
  for (uint32_t b = 0; b < width; b++) f |= uint64_t(v[off + b]) << (8 * b);
  return f;
}

decltype(&xe_map_scan_device) g_scan;
decltype(&xe_map_group) g_group;

// Every entry of map m, in heap blocks of exactly their size.
uint64_t scan_all(xe_vm* vm, int32_t m, uint32_t ks, uint32_t vs, Bytes& k, Bytes& v) {
  uint64_t n = 0;
  CHECK(g_scan(vm, m, nullptr, nullptr, nullptr, 0, &n, nullptr) == 0);
  k.assign(n * ks + 1, 0);
  v.assign(n * vs + 1, 0);
  CHECK(g_scan(vm, m, nullptr, k.data(), v.data(), n, &n, nullptr) == 0);
  return n;
}

// One group call; `acc` (what the destination's accumulators hold so far) gains the source's aggregate and the
// destination must then hold exactly acc. HASH destinations of value size dvs that only these calls write.
void fold(xe_vm* vm, int32_t src, uint32_t sks, uint32_t svs, int32_t dst, uint32_t dvs, const xe_map_group_spec& g, Sums& acc) {
  Bytes sk, sv, dk, dv;
  const uint64_t n = scan_all(vm, src, sks, svs, sk, sv);
  const size_t had = acc.size();
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t* from = g.from == XE_MG_KEY ? &sk[i * sks] : &sv[i * svs];
    auto& a = acc[Bytes(from + g.offset, from + g.offset + g.len)];
    a.first += g.count_off != XE_MG_NONE;
    if (g.sum_off != XE_MG_NONE) a.second += field(&sv[i * svs], g.measure_off, g.measure_width);
  }
  uint64_t matched = 7, created = 7;
  CHECK(g_group(vm, src, nullptr, &g, dst, &matched, &created, nullptr) == 0);
  CHECK(matched == n);
  CHECK(created == acc.size() - had);
  const uint64_t got = scan_all(vm, dst, g.len, dvs, dk, dv);
  CHECK(got == acc.size());
  for (uint64_t i = 0; i < got; i++) {
    const auto it = acc.find(Bytes(&dk[i * g.len], &dk[i * g.len] + g.len));
    CHECK(it != acc.end());
    if (it == acc.end()) continue;
    Bytes want(dvs, 0);
    // (one destination keeps one layout: the accumulators of every call lie at the same offsets)
    if (g.count_off != XE_MG_NONE) memcpy(&want[g.count_off], &it->second.first, 8);
    if (g.sum_off != XE_MG_NONE) memcpy(&want[g.sum_off], &it->second.second, 8);
    CHECK(!memcmp(&dv[i * dvs], want.data(), dvs));
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s hostsim.so\n", argv[0]); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "dlopen %s: %s\n", argv[1], dlerror()); return 3; }
  NEED(default_settings) NEED(create) NEED(destroy) NEED(add_map) NEED(map_update) NEED(map_delete_batch) NEED(map_scan_device)
  NEED(map_group)
  g_scan = map_scan_device;
  g_group = map_group;

  xe_settings s;
  memset(&s, 0, sizeof s);
  default_settings(&s);
  s.engine = 1;
  xe_vm* vm = nullptr;
  if (create(&s, &vm)) return 3;
  uint32_t seed = 97531;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return uint8_t(seed >> 24); };

  // ---- key shapes: a 64-byte key and a 73-byte value, about a dozen groups under every shape
  {
    const uint32_t sks = 64, svs = 73, n = 45;
    xe_map_def def{XE_MAP_HASH, sks, svs, 64, 0};
    int32_t src = 0;
    CHECK(add_map(vm, &def, nullptr, 0, &src) == 0);
    Bytes gone;
    for (uint32_t i = 0; i < n; i++) {
      Bytes k(sks), v(svs);
      for (auto& b : k) b = uint8_t(rnd() % 3);  // few values per byte: the short shapes repeat, the long ones do not
      for (auto& b : v) b = uint8_t(rnd() % 3);
      memcpy(&k[40], &i, 4);  // distinct keys (outside the grouped bytes of the short shapes)
      for (uint32_t b = svs - 9; b < svs; b++) v[b] = rnd();  // the measures
      CHECK(map_update(vm, src, k.data(), v.data()) == 0);
      if (i % 3 == 0) gone.insert(gone.end(), k.begin(), k.end());
    }
    CHECK(map_delete_batch(vm, src, gone.data(), gone.size() / sks, nullptr) == 0);  // live tombstones
    struct Shape { uint32_t from, off, len; };
    const Shape shapes[] = {{XE_MG_KEY, 0, 4}, {XE_MG_KEY, 1, 3}, {XE_MG_KEY, 3, 13}, {XE_MG_KEY, 0, 64},
                            {XE_MG_VALUE, 1, 3}, {XE_MG_VALUE, 5, 4}, {XE_MG_VALUE, 3, 13}, {XE_MG_VALUE, 7, 24}, {XE_MG_VALUE, 1, 64}};
    struct Acc { uint32_t dvs, count_off, sum_off; };
    const Acc accs[] = {{8, 0, XE_MG_NONE}, {16, 8, 0}, {32, XE_MG_NONE, 24}, {4096, 16, 4080}};
    for (const Shape& sh : shapes) {
      for (const Acc& a : accs) {
        xe_map_def ddef{XE_MAP_HASH, sh.len, a.dvs, 64, 0};
        int32_t dst = 0;
        CHECK(add_map(vm, &ddef, nullptr, 0, &dst) == 0);
        Sums acc;
        for (uint32_t width : {1u, 2u, 4u, 8u})
          for (uint32_t moff : {1u, 3u, svs - width}) {
            const bool sum = a.sum_off != XE_MG_NONE;
            fold(vm, src, sks, svs, dst, a.dvs, xe_map_group_spec{sh.from, sh.off, sh.len, moff, sum ? width : 0, a.count_off, a.sum_off, 0}, acc);
          }
      }
    }
  }

  // ---- claims: 3,000 distinct groups and repetitions of them; room for all of them, then for one too few
  {
    const uint32_t sks = 8, svs = 13, groups = 3000, n = 3700;
    xe_map_def def{XE_MAP_HASH, sks, svs, 4096, 0};
    int32_t src = 0;
    CHECK(add_map(vm, &def, nullptr, 0, &src) == 0);
    for (uint32_t i = 0; i < n; i++) {
      uint8_t k[8], v[svs];
      const uint64_t key = 0x9E3779B97F4A7C15ull * (i + 1);
      const uint32_t grp = (i % groups) * 2654435761u;
      memcpy(k, &key, 8);
      for (auto& b : v) b = rnd();
      memcpy(v + 5, &grp, 4);  // the group bytes at an odd offset
      CHECK(map_update(vm, src, k, v) == 0);
    }
    const xe_map_group_spec g{XE_MG_VALUE, 5, 4, 1, 4, 8, 0, 0};
    xe_map_def fits{XE_MAP_HASH, 4, 16, groups, 0}, tight{XE_MAP_HASH, 4, 16, groups - 1, 0};
    int32_t dst = 0, small = 0;
    CHECK(add_map(vm, &fits, nullptr, 0, &dst) == 0);
    CHECK(add_map(vm, &tight, nullptr, 0, &small) == 0);
    Sums acc;
    fold(vm, src, sks, svs, dst, 16, g, acc);
    CHECK(acc.size() == groups);
    fold(vm, src, sks, svs, dst, 16, g, acc);  // every group is there now
    uint64_t matched = 0, created = 0, left = 7;
    CHECK(map_group(vm, src, nullptr, &g, small, &matched, &created, nullptr) == XE_ERR_NOMEM);
    CHECK(map_scan_device(vm, small, nullptr, nullptr, nullptr, 0, &left, nullptr) == 0);
    CHECK(left == 0);
    // an ARRAY source by the odd bytes of its index, into an ARRAY: out of range first, then a map that holds them
    xe_map_def adef{XE_MAP_ARRAY, 4, 9, 700, 0}, hist{XE_MAP_ARRAY, 4, 8, 3, 0}, low{XE_MAP_ARRAY, 4, 8, 2, 0};
    int32_t asrc = 0, ahist = 0, alow = 0;
    CHECK(add_map(vm, &adef, nullptr, 0, &asrc) == 0);
    CHECK(add_map(vm, &hist, nullptr, 0, &ahist) == 0);
    CHECK(add_map(vm, &low, nullptr, 0, &alow) == 0);
    const xe_map_group_spec byte1{XE_MG_KEY, 1, 1, 0, 0, 0, XE_MG_NONE, 0};  // index >> 8: 0, 1, 2
    CHECK(map_group(vm, asrc, nullptr, &byte1, alow, &matched, nullptr, nullptr) == XE_ERR_INVAL);
    CHECK(map_group(vm, asrc, nullptr, &byte1, ahist, &matched, &created, nullptr) == 0);
    CHECK(matched == 700 && created == 0);
    Bytes hk, hv;
    CHECK(scan_all(vm, ahist, 4, 8, hk, hv) == 3);
    CHECK(field(&hv[0], 0, 8) == 256 && field(&hv[8], 0, 8) == 256 && field(&hv[16], 0, 8) == 700 - 512);
  }
  destroy(vm);
  printf("san_mapgroup: %d failed checks\n", g_bad);
  return g_bad ? 1 : 0;
}
