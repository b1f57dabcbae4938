// Host harness for csrc/workspace.h: pa::Carver itself, compiled for the host with -fsanitize=address,undefined.
// For a set of take sequences -- block-aligned, packed, mixed alignments, zero-length blocks, with and without slack
// for an unaligned base -- it checks that the sizing pass and the carving pass report the same bytes(), that every
// pointer is aligned as asked, that the blocks are disjoint, in order and inside [base, base + bytes()), and writes
// every block end to end in a buffer of exactly bytes() bytes, which the sanitizer watches.
// usage: harness  ->  exit code 0 iff every check held (the first failure is printed).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "workspace.h"

struct Pair16 {
  double a, b;
};
struct Take {
  int elem;  // sizeof(T): 1 char, 4 int, 8 double, 16 Pair16
  size_t count, align;
};
struct Block {
  unsigned char* p;
  size_t bytes, align;
};

static Block take(pa::Carver& c, const Take& t) {
  unsigned char* p = nullptr;
  switch (t.elem) {
    case 1: p = (unsigned char*)c.take<char>(t.count, t.align); break;
    case 4: p = (unsigned char*)c.take<int>(t.count, t.align); break;
    case 8: p = (unsigned char*)c.take<double>(t.count, t.align); break;
    default: p = (unsigned char*)c.take<Pair16>(t.count, t.align); break;
  }
  return Block{p, t.count * (size_t)t.elem, t.align};
}

#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      fprintf(stderr, "sequence %d, slack %zu, shift %zu: ", id, slack, shift); \
      fprintf(stderr, __VA_ARGS__);         \
      fprintf(stderr, "\n");                \
      return false;                         \
    }                                       \
  } while (0)

// `shift`: bytes by which the base handed to the carver is moved off the allocation's alignment (needs slack)
static bool run(int id, const std::vector<Take>& seq, size_t slack, size_t shift, size_t expect_bytes) {
  pa::Carver sizing(nullptr, slack);
  for (const Take& t : seq) take(sizing, t);
  const size_t bytes = sizing.bytes();
  if (expect_bytes != (size_t)-1) CHECK(bytes == expect_bytes, "bytes() = %zu, %zu expected", bytes, expect_bytes);
  // a buffer of exactly shift + bytes bytes; without slack the caller owes the strictest alignment of the sequence
  void* raw = nullptr;
  if (posix_memalign(&raw, 256, shift + bytes + (shift + bytes == 0)) != 0) return false;
  unsigned char* base = (unsigned char*)raw + shift;
  pa::Carver carver(base, slack);
  std::vector<Block> blocks;
  for (const Take& t : seq) blocks.push_back(take(carver, t));
  CHECK(carver.bytes() == bytes, "carving pass reports %zu bytes, sizing pass %zu", carver.bytes(), bytes);
  unsigned char* at = base;
  for (size_t i = 0; i < blocks.size(); ++i) {
    const Block& b = blocks[i];
    CHECK((uintptr_t)b.p % b.align == 0, "block %zu is not aligned to %zu", i, b.align);
    CHECK(b.p >= at, "block %zu starts %td bytes inside the block before it", i, at - b.p);
    CHECK(b.p + b.bytes <= base + bytes, "block %zu ends %td bytes past bytes()", i, b.p + b.bytes - (base + bytes));
    memset(b.p, 0xA5, b.bytes);
    at = b.p + b.bytes;
  }
  // every byte written belongs to exactly one block: writing them all again, block by block, finds each still whole
  for (size_t i = 0; i < blocks.size(); ++i)
    for (size_t k = 0; k < blocks[i].bytes; ++k) CHECK(blocks[i].p[k] == 0xA5, "block %zu lost byte %zu", i, k);
  free(raw);
  return true;
}

int main() {
  const size_t any = (size_t)-1;
  struct Case {
    std::vector<Take> seq;
    size_t slack, expect;
  };
  const std::vector<Case> cases = {
      // block-aligned: every block rounded up to 256 bytes (kmeans, the VBx batch, the linkage family, regions, det)
      {{{8, 3, 256}, {8, 33, 256}, {4, 1, 256}, {4, 65, 256}}, 0, 256 + 512 + 256 + 512},
      // ... with zero-length blocks in front, in the middle and at the end
      {{{8, 0, 256}, {4, 7, 256}, {16, 0, 256}, {8, 0, 256}, {4, 64, 256}, {4, 0, 256}}, 0, 512},
      // the linkage tail: 128 bytes of counters behind 256-byte blocks whose last one is not full
      {{{4, 2, 256}, {8, 2, 256}, {8, 16, 128}}, 0, 256 + 256 + 128},
      // packed doubles and 64 spare bytes (pa_vbx_iteration)
      {{{8, 5, 8}, {8, 1, 8}, {8, 0, 8}, {8, 7, 8}, {1, 64, 8}}, 0, 8 * 13 + 64},
      // packed arrays behind 256 bytes of slack for an unaligned base (the annotation counts)
      {{{8, 3, 8}, {8, 3, 8}, {8, 3, 8}, {8, 3, 8}, {8, 3, 8}, {4, 3, 4}}, 256, 256 + 3 * 44},
      {{{8, 0, 8}, {4, 0, 4}}, 256, 256},
      // mixed alignments, rising and falling
      {{{1, 3, 1}, {4, 5, 4}, {8, 1, 64}, {1, 1, 1}, {16, 2, 256}, {4, 3, 4}, {8, 2, 8}}, 0, any},
      {{{4, 3, 4}, {8, 2, 8}, {1, 5, 1}, {16, 1, 16}, {1, 0, 1}, {4, 1, 128}}, 256, any},
      // nothing taken
      {{}, 0, 0},
      {{}, 256, 256},
  };
  int id = 0;
  for (const Case& c : cases) {
    // without slack the base carries the strictest alignment; with slack it may sit anywhere
    const std::vector<size_t> shifts = c.slack ? std::vector<size_t>{0, 1, 8, 255} : std::vector<size_t>{0};
    for (size_t shift : shifts)
      if (!run(id, c.seq, c.slack, shift, c.expect)) return 1;
    ++id;
  }
  printf("%d sequences held\n", id);
  return 0;
}
