// san_maplru.cpp — TEST INFRASTRUCTURE: a stand-alone program that drives the host-simulation loops of the
// device-side LRU_HASH calls (gobpfld_amd/csrc/xe_mapops.h: FIND, VALUE, TOUCH; CLAIM, ERASE; the top's selection
// over the stamps, RANK, SORT, COPY) in a library built with -fsanitize=address,undefined: keys of 4, 13 and 64
// bytes, values of every sub-group width, key and value batches in heap blocks of exactly their size, outputs in
// heap blocks of exactly r entries with k below, at and above matched, filters on odd fields, deletes with
// repetitions and evictions. Every answer is compared with a model of the usage list kept here (a vector of keys,
// most recent first, moved as xe_map_lookup and xe_map_delete move it) and with xe_map_lru_order / xe_map_dump.
// A sanitizer report aborts the process.
//
//   san_maplru <hostsim.so>
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

decltype(&xe_lru_lookup_batch_device) g_lookup;
decltype(&xe_lru_delete_batch_device) g_delete;
decltype(&xe_lru_order_device) g_order;
decltype(&xe_lru_evict_device) g_evict;
decltype(&xe_map_lru_order) g_host_order;

// The model: the usage list (most recent first) and every key's value.
struct Model {
  int32_t idx;
  uint32_t ks, vs;
  std::vector<Bytes> usage;
  std::map<Bytes, Bytes> vals;
  size_t at(const Bytes& k) const { return size_t(std::find(usage.begin(), usage.end(), k) - usage.begin()); }
};

uint64_t field(const Bytes& v, uint32_t off, uint32_t width) {
  uint64_t f = 0;
  for (uint32_t b = 0; b < width; b++) f |= uint64_t(v[off + b]) << (8 * b);
  return f;
}
bool passes(const xe_map_filter* f, const Bytes& v) {
  if (!f || f->op == XE_MF_ALL) return true;
  const uint64_t x = field(v, f->offset, f->width), y = f->operand;
  switch (f->op) {
    case XE_MF_EQ: return x == y;
    case XE_MF_NE: return x != y;
    case XE_MF_LT: return x < y;
    case XE_MF_LE: return x <= y;
    case XE_MF_GT: return x > y;
    case XE_MF_GE: return x >= y;
    case XE_MF_ANYBITS: return (x & y) != 0;
    default: return (x & y) == 0;
  }
}

// The device copy's usage order is the model's (through the host mirror: a download, which relinks from the stamps).
void same_order(xe_vm* vm, const Model& m) {
  uint64_t n = 0;
  CHECK(g_host_order(vm, m.idx, nullptr, 0, &n) == 0);
  CHECK(n == m.usage.size());
  Bytes k(std::max<size_t>(n * m.ks, 1));
  CHECK(g_host_order(vm, m.idx, k.data(), n, &n) == 0);
  for (uint64_t i = 0; i < n && i < m.usage.size(); i++) CHECK(!memcmp(&k[i * m.ks], m.usage[i].data(), m.ks));
}

// A lookup of `keys` (a heap block of exactly count keys) into heap blocks of exactly count values / flags.
void lookup(xe_vm* vm, Model& m, const std::vector<Bytes>& keys, uint32_t flags) {
  const size_t n = keys.size();
  Bytes kb(std::max<size_t>(n * m.ks, 1)), vb(std::max<size_t>(n * m.vs, 1)), fb(std::max<size_t>(n, 1));
  for (size_t i = 0; i < n; i++) memcpy(&kb[i * m.ks], keys[i].data(), m.ks);
  CHECK(g_lookup(vm, m.idx, kb.data(), n, vb.data(), fb.data(), flags, nullptr) == 0);
  for (size_t i = 0; i < n; i++) {
    const auto it = m.vals.find(keys[i]);
    CHECK(fb[i] == (it != m.vals.end() ? 1 : 0));
    const Bytes want = it != m.vals.end() ? it->second : Bytes(m.vs, 0);
    CHECK(!memcmp(&vb[i * m.vs], want.data(), m.vs));
    if (it != m.vals.end() && !(flags & XE_LRU_PEEK)) {  // promote
      const size_t p = m.at(keys[i]);
      std::rotate(m.usage.begin(), m.usage.begin() + long(p), m.usage.begin() + long(p) + 1);
    }
  }
}

void remove(Model& m, const Bytes& k) {
  if (!m.vals.erase(k)) return;
  m.usage.erase(m.usage.begin() + long(m.at(k)));
}

void erase(xe_vm* vm, Model& m, const std::vector<Bytes>& keys) {
  const size_t n = keys.size();
  Bytes kb(std::max<size_t>(n * m.ks, 1)), fb(std::max<size_t>(n, 1));
  for (size_t i = 0; i < n; i++) memcpy(&kb[i * m.ks], keys[i].data(), m.ks);
  CHECK(g_delete(vm, m.idx, kb.data(), n, fb.data(), nullptr) == 0);
  for (size_t i = 0; i < n; i++) CHECK(fb[i] == (m.vals.count(keys[i]) ? 1 : 0));  // present before the call
  for (const Bytes& k : keys) remove(m, k);
}

// One order or evict into heap blocks of exactly r entries (one byte for r = 0): a byte past entry r is a heap
// overflow. Returns matched.
uint64_t order(xe_vm* vm, Model& m, const xe_map_filter* f, uint32_t flags, uint64_t k, bool evict, bool outputs = true) {
  std::vector<Bytes> want;
  uint64_t eligible = 0;
  const size_t n = m.usage.size();
  for (size_t i = 0; i < n; i++) {
    const Bytes& key = m.usage[(flags & XE_LRU_OLDEST_FIRST) ? n - 1 - i : i];
    if (!passes(f, m.vals[key])) continue;
    if (eligible++ < k) want.push_back(key);
  }
  const uint64_t r = want.size();
  Bytes gk(std::max<size_t>(r * m.ks, 1)), gv(std::max<size_t>(r * m.vs, 1));
  uint64_t matched = 7;
  CHECK((evict ? g_evict : g_order)(vm, m.idx, f, flags, outputs ? gk.data() : nullptr, outputs ? gv.data() : nullptr, k, &matched,
                                   nullptr) == 0);
  CHECK(matched == eligible);
  for (uint64_t i = 0; outputs && i < r; i++) {
    CHECK(!memcmp(&gk[i * m.ks], want[i].data(), m.ks));
    CHECK(!memcmp(&gv[i * m.vs], m.vals[want[i]].data(), m.vs));
  }
  if (evict)
    for (const Bytes& key : want) remove(m, key);
  return matched;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s hostsim.so\n", argv[0]); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "dlopen %s: %s\n", argv[1], dlerror()); return 3; }
  NEED(default_settings) NEED(create) NEED(destroy) NEED(add_map) NEED(map_update) NEED(map_lru_order) NEED(map_count)
  NEED(lru_lookup_batch_device) NEED(lru_delete_batch_device) NEED(lru_order_device) NEED(lru_evict_device)
  NEED(lru_lookup_batch) NEED(lru_delete_batch) NEED(lru_order) NEED(lru_evict)
  g_lookup = lru_lookup_batch_device;
  g_delete = lru_delete_batch_device;
  g_order = lru_order_device;
  g_evict = lru_evict_device;
  g_host_order = map_lru_order;

  xe_settings s;
  memset(&s, 0, sizeof s);
  default_settings(&s);
  s.engine = 1;
  xe_vm* vm = nullptr;
  if (create(&s, &vm)) return 3;
  uint32_t seed = 13579;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return uint8_t(seed >> 24); };

  struct Shape { uint32_t ks, vs, max_entries, live; };
  // every key size and value sub-group width; 0, 1 and more than a tile of live entries
  const Shape shapes[] = {{4, 8, 16, 16}, {13, 24, 300, 257}, {64, 100, 512, 300}, {4, 1100, 300, 70}, {13, 8, 16, 0}, {64, 24, 16, 1}};
  for (const Shape& sh : shapes) {
    xe_map_def def{XE_MAP_LRU_HASH, sh.ks, sh.vs, sh.max_entries, 0};
    Model m{-1, sh.ks, sh.vs, {}, {}};
    CHECK(add_map(vm, &def, nullptr, 0, &m.idx) == 0);
    std::vector<Bytes> keys, absent;
    for (uint32_t i = 0; i < sh.live + 5; i++) {
      Bytes k(sh.ks), v(sh.vs);
      for (auto& b : k) b = rnd();
      for (auto& b : v) b = uint8_t(rnd() % 5);  // few values per byte: every filter op selects some and not all
      memcpy(k.data(), &i, std::min<size_t>(4, sh.ks));  // distinct keys
      if (i >= sh.live) { absent.push_back(k); continue; }
      CHECK(map_update(vm, m.idx, k.data(), v.data()) == 0);
      keys.push_back(k);
      m.vals[k] = v;
      m.usage.insert(m.usage.begin(), k);
    }
    auto some = [&](size_t count) {
      std::vector<Bytes> out;
      for (size_t i = 0; i < count; i++) out.push_back(keys.empty() || rnd() % 8 == 0 ? absent[rnd() % absent.size()] : keys[(rnd() * 256u + rnd()) % keys.size()]);
      return out;
    };
    for (size_t count : {size_t(0), size_t(1), size_t(63), size_t(64), size_t(65), size_t(257)}) {
      lookup(vm, m, some(count), 0);
      lookup(vm, m, some(count), XE_LRU_PEEK);
    }
    if (!keys.empty()) lookup(vm, m, std::vector<Bytes>(257, keys[0]), 0);  // one key 257 times
    same_order(vm, m);
    // filters on an 8-byte field (where the value has one) and on an unaligned 2-byte field, both directions
    std::vector<xe_map_filter> fs;
    for (uint32_t op = XE_MF_ALL; op <= XE_MF_NOBITS; op++) {
      fs.push_back(xe_map_filter{op, 3, 2, 0, 0x0201});
      if (sh.vs >= 16) fs.push_back(xe_map_filter{op, 8, 8, 0, 0x0202020202020202ull});
    }
    for (const xe_map_filter& f : fs)
      for (uint32_t flags : {0u, uint32_t(XE_LRU_OLDEST_FIRST)}) {
        const uint64_t matched = order(vm, m, &f, flags, ~uint64_t(0), false, false);  // count only
        for (uint64_t k : {uint64_t(0), uint64_t(1), matched ? matched - 1 : 0, matched, matched + 9}) CHECK(order(vm, m, &f, flags, k, false) == matched);
      }
    CHECK(order(vm, m, nullptr, 0, sh.max_entries, false) == m.usage.size());
    // deletes with repetitions and absent keys, an eviction, lookups from the stamps the removals left, and again
    for (size_t count : {size_t(1), size_t(65)}) {
      const std::vector<Bytes> once = some(count);
      std::vector<Bytes> d = once;
      d.insert(d.end(), once.begin(), once.end());
      erase(vm, m, d);
      order(vm, m, nullptr, XE_LRU_OLDEST_FIRST, 3, true);
      const xe_map_filter f{XE_MF_NE, 3, 2, 0, 0x0201};
      order(vm, m, &f, 0, 2, true);
      lookup(vm, m, some(70), 0);
      CHECK(order(vm, m, nullptr, XE_LRU_OLDEST_FIRST, ~uint64_t(0), false) == m.usage.size());
    }
    same_order(vm, m);
    uint64_t cnt = 0;
    CHECK(map_count(vm, m.idx, &cnt) == 0 && cnt == m.usage.size());
    // the host-pointer forms take the same arguments
    if (!m.usage.empty()) {
      Bytes k = m.usage.back(), v(sh.vs), gk(sh.ks), gv(sh.vs);
      uint8_t found = 7;
      uint64_t matched = 0;
      CHECK(lru_lookup_batch(vm, m.idx, k.data(), 1, v.data(), &found, XE_LRU_PEEK) == 0 && found == 1 && v == m.vals[k]);
      CHECK(lru_order(vm, m.idx, nullptr, XE_LRU_OLDEST_FIRST, gk.data(), gv.data(), 1, &matched) == 0 && matched == m.usage.size() && gk == k);
      CHECK(lru_evict(vm, m.idx, nullptr, XE_LRU_OLDEST_FIRST, gk.data(), gv.data(), 1, &matched) == 0 && gk == k && gv == v);
      remove(m, k);
      CHECK(lru_delete_batch(vm, m.idx, k.data(), 1, &found) == 0 && found == 0);
      same_order(vm, m);
    }
    // delete everything
    erase(vm, m, std::vector<Bytes>(m.usage));
    CHECK(m.usage.empty() && order(vm, m, nullptr, 0, 4, false) == 0);
    same_order(vm, m);
  }
  destroy(vm);
  printf("san_maplru: %d failed checks\n", g_bad);
  return g_bad ? 1 : 0;
}
