// Host-only check of the context workspace's bookkeeping (multi_party_ecdsa_amd/csrc/mpe_ws.h) over a malloc device: alignment, chaining,
// settling into one block, Keep / Hold, the sticky failure flag, and 1 000 random steps.  Every allocation is filled with a pattern of
// its own and read again whenever it must still be intact.  Built with `hipcc --cuda-host-only` by tests/test_ws_arena_cpu.py, once
// plain and once with the address and undefined-behaviour sanitizers (no GPU needed).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "../../multi_party_ecdsa_amd/csrc/mpe_ws.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct HostDev {
  std::map<char*, size_t> owned;
  size_t allocs = 0, frees = 0, syncs = 0;
  bool refuse = false, freed_dirty = false;
  void* alloc(size_t n) {
    if (refuse) return nullptr;
    char* p = (char*)std::aligned_alloc(256, (n + 255) & ~(size_t)255);
    std::memset(p, 0xA5, n);                                   // a block never starts out zero: only zero() makes it so
    owned[p] = n; ++allocs;
    return p;
  }
  void free(void* p) {
    const char* c = (const char*)p;
    for (size_t i = 0, n = owned.at((char*)p); i < n; ++i) if (c[i]) { freed_dirty = true; break; }
    owned.erase((char*)p); ++frees;
    std::free(p);
  }
  void zero(void* p, size_t n, void*) { std::memset(p, 0, n); }
  void sync(void*) { ++syncs; }
};
using Arena = mpe::WsArena<HostDev>;
using Keep = Arena::Keep;
using Hold = Arena::Hold;

struct Live { char* p; size_t n; uint8_t pat; int depth; };
static std::vector<Live> live;
static uint8_t next_pat = 1;

// allocates, checks alignment, that the range lies in ONE block of the arena and overlaps no live range, and fills it
static char* take(Arena& a, size_t n, int depth = 0) {
  char* p = (char*)a.alloc(n);
  if (!p) return nullptr;
  if ((uintptr_t)p % 256) { std::printf("FAILED: %p is not 256-byte aligned\n", (void*)p); std::exit(1); }
  bool inside = false;
  for (const auto& b : a.blocks) inside = inside || (p >= b.p && p + n <= b.p + b.bytes);
  if (!inside) { std::printf("FAILED: an allocation of %zu bytes is not inside a block\n", n); std::exit(1); }
  for (const Live& l : live)
    if (p < l.p + l.n && l.p < p + n) { std::printf("FAILED: an allocation of %zu bytes overlaps a live one\n", n); std::exit(1); }
  std::memset(p, next_pat, n);
  live.push_back(Live{p, n, next_pat, depth});
  next_pat = next_pat == 255 ? 1 : next_pat + 1;
  return p;
}
static bool intact() {
  for (const Live& l : live) for (size_t i = 0; i < l.n; ++i) if ((uint8_t)l.p[i] != l.pat) return false;
  return true;
}
static void drop(int depth) { std::vector<Live> keep; for (const Live& l : live) if (l.depth < depth) keep.push_back(l); live.swap(keep); }

int main() {
  const size_t KB = 1024, MB = 1024 * 1024;
  {  // chaining, settling into one block, zero before free
    Arena a;
    CHECK(a.begin(nullptr) && a.blocks.empty());
    for (int i = 0; i < 4; ++i) CHECK(take(a, 300 * KB + 7));
    CHECK(a.blocks.size() == 1);
    CHECK(take(a, 300 * KB) && take(a, 3 * MB) && take(a, 0));             // does not fit: chains; earlier pointers stay
    CHECK(a.blocks.size() > 1 && intact());
    const size_t high = a.high, chained = a.blocks.size();
    CHECK(high >= 5 * 300 * KB + 3 * MB && high <= a.capacity());
    live.clear();
    CHECK(a.begin(nullptr));
    CHECK(a.blocks.size() == 1 && a.blocks[0].bytes >= high && a.blocks[0].bytes == high + high / 4 + MB);
    CHECK(a.dev.frees == chained && !a.dev.freed_dirty && a.dev.syncs >= 1);
    // the same sequence again: one block, no allocation, nothing freed
    const size_t allocs = a.dev.allocs;
    for (int i = 0; i < 4; ++i) CHECK(take(a, 300 * KB + 7));
    CHECK(take(a, 300 * KB) && take(a, 3 * MB) && take(a, 0));
    CHECK(a.blocks.size() == 1 && a.dev.allocs == allocs && a.high == high && intact());
    live.clear();
    CHECK(a.begin(nullptr) && a.dev.allocs == allocs && a.dev.frees == chained);
    a.release(nullptr);
    CHECK(a.blocks.empty() && a.dev.owned.empty() && !a.dev.freed_dirty);
  }
  {  // keep: a nested begin returns to the mark, the kept arrays stay; afterwards a begin returns to the start
    Arena a;
    CHECK(a.begin(nullptr));
    char* own = take(a, 100 * KB);
    CHECK(own);
    {
      Keep k(a);
      CHECK(a.begin(nullptr));
      char* x = take(a, 200 * KB, 1);
      CHECK(x && x != own);
      drop(1);
      CHECK(a.begin(nullptr));
      CHECK(take(a, 200 * KB, 1) == x && intact());                          // the space above the mark is reused
      CHECK(take(a, 4 * MB, 1) && a.blocks.size() > 1);                      // ... and grows under the keep
      const size_t blocks = a.blocks.size(), frees = a.dev.frees;
      drop(1);
      CHECK(a.begin(nullptr) && a.blocks.size() == blocks && a.dev.frees == frees);      // chained under a keep: no coalescing
      CHECK(take(a, 200 * KB, 1) == x && take(a, 4 * MB, 1) && a.blocks.size() == blocks && intact());
      {
        Keep inner(a);                                                       // keeps nest: the inner mark lies behind the 4 MB array
        CHECK(a.begin(nullptr));
        CHECK(take(a, 64 * KB, 2) && intact());
        drop(2);
      }
      drop(1);
      CHECK(a.begin(nullptr) && take(a, 200 * KB, 1) == x && intact());      // the outer mark is back
      drop(1);
    }
    CHECK(intact());
    live.clear();
    CHECK(a.begin(nullptr) && a.blocks.size() == 1 && !a.dev.freed_dirty);
    CHECK(take(a, 100 * KB) == a.blocks[0].p);                               // from the start
    live.clear();
    a.release(nullptr);
  }
  {  // hold: a nested begin changes nothing, chained or not
    Arena a;
    CHECK(a.begin(nullptr));
    {
      Hold off(a, false);
      CHECK(a.hold == 0);
    }
    {
      Hold h(a, true);
      CHECK(a.hold == 1 && take(a, 500 * KB));
      const Arena::Pos at = a.pos;
      CHECK(a.begin(nullptr) && a.pos.blk == at.blk && a.pos.off == at.off);
      CHECK(take(a, 500 * KB) && take(a, 2 * MB) && a.blocks.size() > 1);
      const size_t blocks = a.blocks.size();
      CHECK(a.begin(nullptr) && a.blocks.size() == blocks && a.dev.frees == 0 && intact());
      CHECK(take(a, 100 * KB) && intact());
    }
    CHECK(a.hold == 0);
    live.clear();
    CHECK(a.begin(nullptr) && a.blocks.size() == 1 && a.blocks[0].bytes >= a.high);
    a.release(nullptr);
  }
  {  // a failing device allocation: nullptr, the flag stays up until a top-level begin
    Arena a;
    CHECK(a.begin(nullptr) && take(a, 100 * KB));
    a.dev.refuse = true;
    CHECK(a.alloc(8 * MB) == nullptr && a.failed);
    { Hold h(a, true); CHECK(!a.begin(nullptr) && a.failed); }
    { Keep k(a); CHECK(!a.begin(nullptr) && a.failed); }
    CHECK(intact());
    a.dev.refuse = false;
    live.clear();
    CHECK(a.begin(nullptr) && !a.failed && take(a, 8 * MB));
    live.clear();
    a.dev.refuse = true;                                                     // ... and a begin that cannot get its one block says so
    CHECK(!a.begin(nullptr) && a.failed && a.blocks.empty());
    a.dev.refuse = false;
    CHECK(a.begin(nullptr) && !a.failed && take(a, 1 * KB));
    live.clear();
    a.release(nullptr);
    CHECK(a.dev.owned.empty() && !a.dev.freed_dirty);
  }
  {  // 1 000 random steps: no overlapping live ranges, every survivor intact, one block behind every top-level begin
    Arena a;
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint64_t n) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (s >> 33) % n; };
    std::vector<std::unique_ptr<Keep>> keeps;
    std::unique_ptr<Hold> hold;
    long begins = 0, tops = 0;
    CHECK(a.begin(nullptr));
    for (int step = 0; step < 1000; ++step) {
      const int depth = (int)keeps.size();
      const uint64_t r = rnd(100);
      if (r < 70) {
        const size_t n = r < 3 ? 2 * MB + rnd(MB) : (r < 10 ? rnd(600 * KB) : rnd(40 * KB));
        CHECK(take(a, n, depth));
      } else if (r < 85) {
        ++begins;
        if (!hold) drop(depth);                                              // what a begin gives up: everything above the innermost mark
        CHECK(a.begin(nullptr) && intact());
        if (!hold && !depth) { ++tops; CHECK(a.blocks.size() <= 1 && (a.blocks.empty() || a.blocks[0].bytes >= a.high)); }
      } else if (r < 90) {
        if (depth < 3 && !hold) keeps.push_back(std::make_unique<Keep>(a));
      } else if (r < 95) {
        if (depth && !hold) { keeps.pop_back(); for (Live& l : live) if (l.depth == depth) l.depth = depth - 1; }
      } else if (hold) {
        hold.reset();
      } else {
        hold = std::make_unique<Hold>(a, true);
      }
    }
    CHECK(intact() && !a.failed && !a.dev.freed_dirty && tops > 10);
    hold.reset();
    while (!keeps.empty()) keeps.pop_back();
    live.clear();
    CHECK(a.begin(nullptr) && a.blocks.size() <= 1);
    a.release(nullptr);
    CHECK(a.dev.owned.empty() && a.dev.allocs == a.dev.frees && !a.dev.freed_dirty);
    std::printf("OK %ld begins (%ld top-level), %zu device allocations, high-water mark %zu bytes\n", begins, tops, a.dev.allocs, a.high);
  }
  return 0;
}
