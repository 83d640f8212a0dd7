// The context workspace: device memory for the intermediates of composite operations (Paillier, proofs, rounds), bump-allocated.
// Nobody states a size in advance.  A composite calls begin(), then takes what it needs; when the current block has no room the arena
// chains another one — earlier blocks are not touched, so pointers already handed to queued kernels stay valid — and the next top-level
// begin() replaces the chain by ONE block of the recorded high-water mark (+ 1/4 + 1 MB).  In steady state the workspace is one block
// that is reset and bumped, with no allocation.  An allocation fails only when the device has no memory: nullptr, and `failed` stays
// raised until the next top-level begin() (ws_ok), so a composite checks once behind its allocations instead of every pointer.
//   Hold   several composites run side by side out of one begin(): their begin() does nothing
//   Keep   a composite's own arrays, allocated before the Keep: the begin() of the composites it calls returns to that mark, not to
//          the start, so that they reuse the space above it one after the other
// The bookkeeping calls no HIP: Dev supplies alloc / free / zero / sync (WsHip in mpe_internal.h, malloc in tests/cpp/test_ws_arena.cpp).
#pragma once
#include <stddef.h>
#include <vector>

namespace mpe {

template <class Dev>
struct WsArena {
  struct Block { char* p; size_t bytes, used; };            // used: where the bump position stood when it moved on to the next block
  struct Pos { size_t blk = 0, off = 0; };
  Dev dev;
  std::vector<Block> blocks;
  Pos pos, mark;
  bool kept = false;       // a Keep is alive: begin() returns to `mark`
  int hold = 0;            // Holds alive: begin() does nothing
  size_t high = 0;         // the most bytes ever in use at once, as one block would hold them
  bool failed = false;

  static size_t up(size_t x) { return (x + 255) & ~(size_t)255; }
  size_t capacity() const { size_t s = 0; for (const Block& b : blocks) s += b.bytes; return s; }

  // false: an allocation has failed since the last top-level begin (or the one block could not be allocated just now)
  bool begin(void* stream) {
    if (hold) return !failed;
    if (kept) { pos = mark; return !failed; }
    pos = Pos{};
    failed = false;
    if (blocks.size() > 1) {                                 // the last use chained: settle into one block (queued work may still read the old ones)
      release(stream);
      failed = !grow(high + high / 4 + ((size_t)1 << 20));
    }
    return !failed;
  }
  void* alloc(size_t bytes) {
    for (;;) {
      if (pos.blk == blocks.size() && !grow((bytes > capacity() ? bytes : capacity()) + ((size_t)1 << 20))) { failed = true; return nullptr; }
      Block& b = blocks[pos.blk];
      const size_t off = up(pos.off);
      if (off + bytes <= b.bytes) {
        pos.off = off + bytes;
        size_t lin = pos.off;
        for (size_t i = 0; i < pos.blk; ++i) lin += up(blocks[i].used);
        if (lin > high) high = lin;
        return b.p + off;
      }
      b.used = pos.off;
      pos.blk++;
      pos.off = 0;
    }
  }
  // zeroes and frees every block (the workspace holds nonce-derived values); the caller's stream is drained first
  void release(void* stream) {
    dev.sync(stream);
    for (const Block& b : blocks) dev.zero(b.p, b.bytes, stream);
    dev.sync(stream);
    for (const Block& b : blocks) dev.free(b.p);
    blocks.clear();
    pos = mark = Pos{};
  }

  struct Hold {
    WsArena* a;
    Hold(WsArena& arena, bool on) : a(on ? &arena : nullptr) { if (a) a->hold++; }
    ~Hold() { if (a) a->hold--; }
    Hold(const Hold&) = delete;
  };
  struct Keep {
    WsArena& a; Pos mark; bool kept;
    explicit Keep(WsArena& arena) : a(arena), mark(arena.mark), kept(arena.kept) { a.mark = a.pos; a.kept = true; }
    ~Keep() { a.mark = mark; a.kept = kept; }
    Keep(const Keep&) = delete;
  };

 private:
  bool grow(size_t bytes) {
    char* p = (char*)dev.alloc(bytes);
    if (p) blocks.push_back(Block{p, bytes, 0});
    return p != nullptr;
  }
};

}  // namespace mpe
