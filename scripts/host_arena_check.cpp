// Developer check on the host alone (no GPU, nothing of the library linked): the book-keeping of Arena (common.h) --
// requested / peak / excess, reset(), guard placement, the guard comparison and the poison fill -- over a block of HOST memory.
// The three hooks that api.cpp implements on the stream are restated here with memset / memcpy; everything else is the library's own
// inline code.  Under the address and undefined-behaviour sanitizers a guard placed outside the block is reported.
//   hipcc -std=c++17 -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined -Wno-unused-value -I keras_ocr_amd/csrc \
//         scripts/host_arena_check.cpp -o host_arena_check && ./host_arena_check
#include "common.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHECK(c)                                      \
  do {                                                \
    if (!(c)) {                                       \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
      exit(1);                                        \
    }                                                 \
  } while (0)

// ---- the hooks of api.cpp, restated on host memory ----
void arena_guard_fill(Arena& a, size_t at, size_t len) { memset(a.base + at, ARENA_GUARD_FILL, len); }
void arena_poison_fill(Arena& a, void* p, size_t bytes) { memset(p, a.pbyte, bytes); }
void arena_guard_check(Arena& a) {
  kocr_ctx* ctx = a.gctx;
  std::vector<ArenaGuard> list;
  list.swap(a.guards);
  std::vector<unsigned char> copy;
  for (const ArenaGuard& g : list) {
    copy.assign((const unsigned char*)a.base + g.at, (const unsigned char*)a.base + g.at + g.len);
    const long bad = arena_guard_damage(copy.data(), g.len);
    if (bad < 0) continue;
    if (ctx->guard_damage.count++ == 0) {
      ctx->guard_damage.arena = 0;
      ctx->guard_damage.offset = g.buf;
      ctx->guard_damage.byte = g.at + (size_t)bad;
    }
  }
}
// arena_reserve's book-keeping over a block of exactly `cap` bytes: one byte more is the sanitizer's
static void reserve(Arena& a, size_t requested, size_t cap) {
  free(a.base);
  a.base = (char*)malloc(cap);
  a.cap = cap;
  a.requested = requested;
  a.peak = 0;
  a.reset();
}

int main() {
  static kocr_ctx ctx;
  Arena& a = ctx.ws;
  CHECK(kocr_ctx::N_ARENAS == 8 && ctx.arena_at(0) == &ctx.ws && ctx.arena_at(7) == &ctx.chr && !ctx.arena_at(8) && !ctx.arena_at(-1));
  CHECK(!strcmp(kocr_ctx::arena_name(0), "ws") && !strcmp(kocr_ctx::arena_name(7), "chr") && !kocr_ctx::arena_name(8));

  // (1) a sequence that stays inside `requested`
  reserve(a, 1000, 1000 + 125 + 4096);
  char* p0 = (char*)arena_alloc(a, 100);
  char* p1 = (char*)arena_alloc(a, 300);
  char* p2 = (char*)arena_alloc(a, 232);
  CHECK(p0 == a.base && p1 == a.base + 256 && p2 == a.base + 768);
  CHECK(a.off == 1000 && a.peak == 1000 && a.excess == 0 && a.requested == 1000);
  // (2) past `requested`, inside `cap`: the overshoot is the excess, and the buffer is real
  char* p3 = (char*)arena_alloc(a, 500);
  CHECK(p3 == a.base + 1024 && a.peak == 1524 && a.excess == 524);
  memset(p3, 1, 500);
  // ... past `cap`: refused, nothing moves but the statistics, which say how far the plan was short
  CHECK(!arena_alloc(a, 8000) && a.off == 1524 && a.peak == 1536 + 8000 && a.excess == 1536 + 8000 - 1000);
  // (3) reset() and a second epoch: excess is sticky, peak restarts at the next reservation
  const size_t sticky = a.excess;
  reserve(a, 2000, 2000 + 250 + 4096);
  CHECK(a.off == 0 && a.peak == 0 && a.excess == sticky);
  CHECK(arena_alloc(a, 1999) && a.peak == 1999 && a.excess == sticky);
  a.reset();
  CHECK(a.off == 0 && a.peak == 1999 && arena_alloc(a, 10) && a.peak == 1999 && a.excess == sticky);
  a.excess = 0;

  // (4) guard placement: behind an odd-sized buffer the guard starts at its first byte and ends 256 bytes behind the next
  // 256-byte boundary; the guards move the buffers but count neither in off nor in peak / excess
  a.gctx = &ctx;
  reserve(a, 1000, 1000 + 125 + 4096 + 3 * (256 + 255));
  char* g0 = (char*)arena_alloc(a, 100);
  char* g1 = (char*)arena_alloc(a, 300);
  char* g2 = (char*)arena_alloc(a, 256);
  CHECK(g0 == a.base && g1 == a.base + 256 + 256 && g2 == a.base + 768 + 512);
  CHECK(a.off == 1024 && a.peak == 1024 && a.excess == 24 && a.gextra == 768 && a.guards.size() == 3);
  a.excess = 0;
  CHECK(a.guards[0].buf == 0 && a.guards[0].at == 100 && a.guards[0].len == 156 + 256);
  CHECK(a.guards[1].buf == 512 && a.guards[1].at == 812 && a.guards[1].len == 212 + 256);
  CHECK(a.guards[2].buf == 1280 && a.guards[2].at == 1536 && a.guards[2].len == 256);  // an aligned end: 256 bytes
  for (const ArenaGuard& g : a.guards)
    for (size_t i = 0; i < g.len; ++i) CHECK((unsigned char)a.base[g.at + i] == ARENA_GUARD_FILL);
  // every byte of a buffer may be written; the byte before a guard is the buffer's last
  memset(g0, 0, 100);
  memset(g1, 0, 300);
  memset(g2, 0, 256);
  // an allocation that does not fit with its guard is refused
  CHECK(!arena_alloc(a, a.cap));

  // (5) the comparison of a copied-back guard: clean, then the first, a middle and the last byte changed
  std::vector<unsigned char> copy(412, ARENA_GUARD_FILL);
  CHECK(arena_guard_damage(copy.data(), copy.size()) == -1);
  for (size_t at : {(size_t)0, (size_t)200, (size_t)411}) {
    copy[at] ^= 0xFF;
    CHECK(arena_guard_damage(copy.data(), copy.size()) == (long)at);
    copy[at] = ARENA_GUARD_FILL;
  }
  copy[411] = 0;
  copy[7] = 0;
  CHECK(arena_guard_damage(copy.data(), copy.size()) == 7);  // the first of several

  // (6) reset() compares, latches the first damaged guard and forgets the list
  a.reset();
  CHECK(a.guards.empty() && a.off == 0 && a.gextra == 0 && ctx.guard_damage.count == 0);
  g0 = (char*)arena_alloc(a, 100);
  g1 = (char*)arena_alloc(a, 300);
  g1[300] = 0;                 // one byte past the second buffer
  g1[300 + 212 + 255] = 0x5A;  // and the last byte of the same guard: one damaged guard, its first byte named
  a.reset();
  CHECK(ctx.guard_damage.count == 1 && ctx.guard_damage.arena == 0 && ctx.guard_damage.offset == 512 && ctx.guard_damage.byte == 812);
  g0 = (char*)arena_alloc(a, 100);
  g0[100 + 155] = 0;  // the last byte before the next boundary
  a.reset();
  CHECK(ctx.guard_damage.count == 2 && ctx.guard_damage.offset == 512);  // the first stays latched
  // guards off: the plain layout again
  a.gctx = nullptr;
  CHECK(arena_alloc(a, 100) == a.base && arena_alloc(a, 1) == a.base + 256 && a.guards.empty());

  // (7) poison mode: exactly the buffer's bytes are filled -- not the alignment gap behind it, not a guard -- with and
  // without guards, and the layout and the statistics are those of the mode off
  reserve(a, 1000, 1000 + 125 + 4096 + 2 * (256 + 255));
  memset(a.base, 0x11, a.cap);
  a.pctx = &ctx;
  a.pbyte = 0xFF;
  p0 = (char*)arena_alloc(a, 100);
  p1 = (char*)arena_alloc(a, 300);
  CHECK(p0 == a.base && p1 == a.base + 256 && a.off == 556 && a.peak == 556 && a.guards.empty());
  for (size_t i = 0; i < 556; ++i) CHECK((unsigned char)a.base[i] == ((i < 100 || i >= 256) ? 0xFF : 0x11));
  CHECK((unsigned char)a.base[556] == 0x11);
  a.reset();
  a.gctx = &ctx;
  a.pbyte = 0x00;
  memset(a.base, 0x11, a.cap);
  g0 = (char*)arena_alloc(a, 100);
  g1 = (char*)arena_alloc(a, 300);
  CHECK(g0 == a.base && g1 == a.base + 512 && a.off == 556 && a.guards.size() == 2);
  for (size_t i = 0; i < 100; ++i) CHECK(g0[i] == 0);
  for (size_t i = 100; i < 512; ++i) CHECK((unsigned char)a.base[i] == ARENA_GUARD_FILL);
  for (size_t i = 0; i < 300; ++i) CHECK(g1[i] == 0);
  CHECK((unsigned char)g1[300] == ARENA_GUARD_FILL);
  const int before = ctx.guard_damage.count;
  a.reset();
  CHECK(ctx.guard_damage.count == before);  // the fill damaged no guard
  a.gctx = a.pctx = nullptr;
  CHECK(arena_alloc(a, 100) == a.base && (unsigned char)a.base[0] == 0);  // off: nothing is filled
  free(a.base);
  a.base = nullptr;
  printf("host_arena_check ok\n");
  return 0;
}
