// san_mapmodify.cpp — TEST INFRASTRUCTURE: a stand-alone program that drives the host-simulation loops of the
// in-place map edits (gobpfld_amd/csrc/xe_mapops.h: MODIFY_TILE, MODIFY_EDIT, MODIFY_MARK, MODIFY_KEYED) in a
// library built with -fsanitize=address,undefined. Every output buffer is a heap block of exactly the bytes
// the call may write, placed at an odd address inside it where the case says so, so a byte too many is a
// sanitizer report; the edited fields sit at odd offsets of odd-sized values and at the value's last bytes,
// so a store past a value of the last slot is one too. What the calls leave is compared with xe_map_dump
// edited here by a restatement of the ops over 128-bit integers. A sanitizer report aborts the process.
//
//   san_mapmodify <hostsim.so>
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
using Wide = unsigned __int128;

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
    case XE_MF_ANYBITS: return (x & o) != 0;
    case XE_MF_LT: return x < o;
    default: return (x & o) == 0;  // XE_MF_NOBITS
  }
}
// the ops over integers that cannot overflow
uint64_t apply(uint32_t op, uint32_t width, uint64_t f, uint64_t o) {
  const Wide top = (Wide(1) << (8 * width)) - 1, F = f, O = o;
  Wide r = 0;
  switch (op) {
    case XE_MM_SET: r = O & top; break;
    case XE_MM_ADD: r = (F + O) & top; break;
    case XE_MM_SUB: r = (F + (top + 1) * 2 - (O & top)) & top; break;
    case XE_MM_ADD_SAT: r = std::min(F + O, top); break;
    case XE_MM_SUB_SAT: r = F > O ? F - O : 0; break;
    case XE_MM_AND: r = F & O; break;
    case XE_MM_OR: r = (F | O) & top; break;
    case XE_MM_XOR: r = (F ^ O) & top; break;
    case XE_MM_MIN: r = std::min(F, O); break;
    case XE_MM_MAX: r = std::min(std::max(F, O), top); break;
    default: r = o >= 8 * width ? 0 : F >> o; break;  // XE_MM_SHR
  }
  return uint64_t(r);
}
void edit(uint8_t* v, const std::vector<xe_map_edit>& edits) {
  for (const xe_map_edit& e : edits) {
    const uint64_t o = (e.flags & XE_MM_OPERAND_FIELD) ? field(v, uint32_t(e.operand), e.width) : e.operand;
    const uint64_t r = apply(e.op, e.width, field(v, e.offset, e.width), o);
    for (uint32_t b = 0; b < e.width; b++) v[e.offset + b] = uint8_t(r >> (8 * b));
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s hostsim.so\n", argv[0]); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "dlopen %s: %s\n", argv[1], dlerror()); return 3; }
  NEED(default_settings) NEED(create) NEED(destroy) NEED(add_map) NEED(map_update) NEED(map_dump) NEED(map_delete_batch)
  NEED(map_modify_device) NEED(map_modify) NEED(map_modify_batch_device) NEED(map_modify_batch) NEED(map_count)

  xe_settings s;
  memset(&s, 0, sizeof s);
  default_settings(&s);
  s.engine = 1;
  xe_vm* vm = nullptr;
  if (create(&s, &vm)) return 3;

  struct Geo { uint32_t type, ks, vs, max, n; };
  // value sizes on both sides of the single pass's limit and of the sub-group cuts; 300 entries: two tiles of a 1,024-slot table
  const Geo geos[] = {{XE_MAP_HASH, 13, 13, 300, 300}, {XE_MAP_HASH, 8, 17, 64, 40},   {XE_MAP_HASH, 25, 65, 64, 40},
                      {XE_MAP_HASH, 0, 24, 8, 1},      {XE_MAP_ARRAY, 4, 13, 300, 150}, {XE_MAP_HASH, 64, 1025, 16, 9},
                      {XE_MAP_ARRAY, 4, 9, 257, 257},  {XE_MAP_HASH, 8, 64, 64, 50}};
  uint32_t seed = 4242;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return uint8_t(seed >> 24); };
  for (const Geo& g : geos) {
    const bool array = g.type == XE_MAP_ARRAY;
    xe_map_def def{g.type, g.ks, g.vs, g.max, 0};
    int32_t m = 0;
    CHECK(add_map(vm, &def, nullptr, 0, &m) == 0);
    const uint32_t ks = array ? 4 : g.ks, vs = g.vs;
    std::vector<Bytes> keys;
    for (uint32_t i = 0; i < g.n; i++) {
      Bytes k(std::max<uint32_t>(ks, 4), 0), v(vs);
      if (array) { const uint32_t idx = g.n == g.max ? i : i * 2; memcpy(k.data(), &idx, 4); }
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
    // the map as key -> value, from xe_map_dump
    auto dump = [&]() {
      std::map<Bytes, Bytes> all;
      uint64_t cnt = 0;
      CHECK(map_dump(vm, m, nullptr, nullptr, 0, &cnt) == 0);
      if (array) {
        Bytes raw(size_t(vs) * g.max + 1);
        CHECK(map_dump(vm, m, raw.data(), nullptr, cnt, &cnt) == 0);
        for (uint32_t i = 0; i < g.max; i++) {
          Bytes k(4);
          memcpy(k.data(), &i, 4);
          all[k] = Bytes(&raw[size_t(i) * vs], &raw[size_t(i + 1) * vs]);
        }
      } else {
        Bytes dk(cnt * ks + 1), dv(cnt * vs + 1);
        CHECK(map_dump(vm, m, dk.data(), dv.data(), cnt, &cnt) == 0);
        for (uint64_t i = 0; i < cnt; i++) all[Bytes(&dk[i * ks], &dk[i * ks] + ks)] = Bytes(&dv[i * vs], &dv[(i + 1) * vs]);
      }
      return all;
    };
    const uint32_t w = vs >= 12 ? 8 : 4;
    const std::vector<std::vector<xe_map_edit>> lists = {
        {{XE_MM_ADD, vs - w, w, 0, 0xf1f2f3f4f5f6f7f8ull}},                              // the value's last bytes
        {{XE_MM_SET, 1, w, 0, 0x1122334455667788ull}, {XE_MM_SHR, 3, 4, 0, 5}, {XE_MM_XOR, vs - 1, 1, 0, 0xff}},
        {{XE_MM_ADD_SAT, 1, 4, XE_MM_OPERAND_FIELD, vs - 4}, {XE_MM_MIN, 1, 4, XE_MM_OPERAND_FIELD, 5}, {XE_MM_SUB_SAT, vs - 2, 2, 0, 0x8000},
         {XE_MM_MAX, 0, 1, 0, 0x1ff}, {XE_MM_SUB, 2, 2, 0, 3}, {XE_MM_AND, 0, 2, 0, 0xf0f0}, {XE_MM_OR, vs - w, w, 0, 1}, {XE_MM_ADD, 0, 1, 0, 255}},
    };
    const xe_map_filter filters[] = {{XE_MF_ALL, 0, 0, 0, 0}, {XE_MF_ANYBITS, 0, 1, 0, 0x5}, {XE_MF_LT, vs - 1, 1, 0, 0x60}};
    int variant = 0;
    for (const auto& edits : lists) {
      for (const xe_map_filter& f : filters) {
        std::map<Bytes, Bytes> before = dump();
        std::map<Bytes, Bytes> want;  // the matches
        for (auto& e : before)
          if (selects(f, e.second.data())) want[e.first] = e.second;
        for (uint64_t cap : {uint64_t(0), uint64_t(want.size() / 2), uint64_t(g.max), ~uint64_t(0)}) {
          before = dump();
          want.clear();
          for (auto& e : before)
            if (selects(f, e.second.data())) want[e.first] = e.second;
          const uint64_t r = std::min<uint64_t>(cap, want.size());
          const uint32_t shift = variant & 1;
          const bool silent = (variant % 3) == 0, host = (variant & 2) != 0;
          variant++;
          // exactly r entries of room, `shift` bytes into the block
          uint8_t* kb = static_cast<uint8_t*>(malloc(std::max<size_t>(r * ks + shift, 1)));
          uint8_t* vb = static_cast<uint8_t*>(malloc(std::max<size_t>(r * vs + shift, 1)));
          uint64_t got = 0;
          int rc;
          if (host) rc = map_modify(vm, m, &f, edits.data(), uint32_t(edits.size()), silent ? nullptr : kb + shift, silent ? nullptr : vb + shift, cap, &got);
          else rc = map_modify_device(vm, m, &f, edits.data(), uint32_t(edits.size()), silent ? nullptr : kb + shift, silent ? nullptr : vb + shift, cap, &got, nullptr);
          CHECK(rc == 0);
          CHECK(got == want.size());
          std::map<Bytes, Bytes> seen;
          if (!silent) {
            for (uint64_t i = 0; i < r; i++)
              seen[Bytes(kb + shift + i * ks, kb + shift + (i + 1) * ks)] = Bytes(vb + shift + i * vs, vb + shift + (i + 1) * vs);
            CHECK(seen.size() == r || ks == 0);
            for (auto& e : seen) {
              auto it = want.find(e.first);
              CHECK(it != want.end() && it->second == e.second);  // the value from before the edits
            }
          }
          free(kb);
          free(vb);
          // exactly r of the matches are edited, once; every other entry is what it was
          std::map<Bytes, Bytes> after = dump();
          CHECK(after.size() == before.size());
          uint64_t edited = 0, idle = 0;  // matches that changed; matches that the edits leave as they are
          for (auto& e : before) {
            Bytes v = e.second;
            edit(v.data(), edits);
            const Bytes& now = after[e.first];
            const bool was = want.count(e.first) != 0;
            CHECK(now == e.second || (was && now == v));
            if (was && v == e.second) idle++;
            else if (was && now == v) edited++;
            if (!silent && was && v != e.second) CHECK((seen.count(e.first) != 0) == (now == v));  // the reported are the edited
          }
          CHECK(edited <= r && r <= edited + idle);
        }
      }
    }
    // keyed: every key three times, spread over the batch, and absent keys in between; exact-size outputs
    {
      std::map<Bytes, Bytes> before = dump();
      const std::vector<xe_map_edit> inc = {{XE_MM_ADD, vs - 4, 4, 0, 1}, {XE_MM_ADD, 0, 1, 0, 1}};
      std::vector<Bytes> batch;
      for (int rep = 0; rep < 3; rep++)
        for (size_t i = rep; i < keys.size(); i += 2) batch.push_back(keys[i]);
      Bytes absent(std::max<uint32_t>(ks, 4), 0xfe);
      if (ks) batch.insert(batch.begin() + batch.size() / 2, Bytes(absent.begin(), absent.begin() + ks));
      for (int form = 0; form < 2; form++) {
        before = dump();
        const size_t n = batch.size(), shift = form;
        uint8_t* kb = static_cast<uint8_t*>(malloc(std::max<size_t>(n * ks + shift, 1)));
        uint8_t* vb = static_cast<uint8_t*>(malloc(n * vs + shift));
        uint8_t* fb = static_cast<uint8_t*>(malloc(n + shift));
        for (size_t i = 0; i < n && ks; i++) memcpy(kb + shift + i * ks, batch[i].data(), ks);
        int rc;
        if (form) rc = map_modify_batch(vm, m, kb + shift, n, inc.data(), 2, vb + shift, fb + shift);
        else rc = map_modify_batch_device(vm, m, kb + shift, n, inc.data(), 2, vb + shift, fb + shift, nullptr);
        CHECK(rc == 0);
        for (size_t i = 0; i < n; i++) {
          auto it = before.find(batch[i]);
          CHECK((fb[shift + i] != 0) == (it != before.end()));
          const Bytes old(vb + shift + i * vs, vb + shift + (i + 1) * vs);
          CHECK(it != before.end() ? old == it->second : old == Bytes(vs, 0));
        }
        free(kb);
        free(vb);
        free(fb);
        std::map<Bytes, Bytes> after = dump();
        CHECK(after.size() == before.size());
        for (auto& e : before) {
          Bytes v = e.second;
          if (std::find(batch.begin(), batch.end(), e.first) != batch.end()) edit(v.data(), inc);  // once, however often it is repeated
          CHECK(after[e.first] == v);
        }
      }
      // refused: nothing is read through the edits or written anywhere
      before = dump();
      uint64_t got = 0;
      const xe_map_edit bad[] = {{XE_MM_ADD, vs - 3, 4, 0, 1}, {XE_MM_ADD, 0, 4, XE_MM_OPERAND_FIELD, vs - 3}, {11, 0, 1, 0, 0}, {XE_MM_ADD, 0, 1, 2, 0}};
      for (const xe_map_edit& e : bad) {
        CHECK(map_modify_device(vm, m, nullptr, &e, 1, nullptr, nullptr, 5, &got, nullptr) == XE_ERR_INVAL);
        CHECK(map_modify_batch(vm, m, keys[0].data(), 1, &e, 1, nullptr, nullptr) == XE_ERR_INVAL);
      }
      CHECK(map_modify(vm, m, nullptr, inc.data(), XE_MM_MAX_EDITS + 1, nullptr, nullptr, 5, &got) == XE_ERR_INVAL);
      CHECK(map_modify(vm, m, nullptr, nullptr, 1, nullptr, nullptr, 5, &got) == XE_ERR_INVAL);
      CHECK(before == dump());
    }
  }
  destroy(vm);
  printf("san_mapmodify: %d failed checks\n", g_bad);
  return g_bad ? 1 : 0;
}
