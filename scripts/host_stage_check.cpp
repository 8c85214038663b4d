// Developer check on the host alone (no GPU, nothing of the library linked): the recogniser stage of abi.h (RecStage with
// staging_bytes / staging_take) and the resident-result states of kocr_ctx, over arenas of HOST memory, with a crnn_forward
// that fills every row it is handed with that buffer's own byte.  Under the address and undefined-behaviour sanitizers a row
// past its buffer or past the arena is reported; rows of two buffers that overlap fail the pattern check.
//   hipcc -std=c++17 -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined -Wno-unused-value -I keras_ocr_amd/csrc \
//         scripts/host_stage_check.cpp -o host_stage_check && ./host_stage_check
#include "abi.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);                 \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

// ---- what the helpers call in the library, restated on host memory ----
static const int LW = 48;
int arena_reserve(kocr_ctx* ctx, Arena& a, size_t bytes) {
  ctx->invalidate_results();
  if (bytes <= a.cap) return KOCR_OK;
  free(a.base);
  a.base = (char*)malloc(bytes);  // exactly what was asked for: one byte more is the sanitizer's
  a.cap = bytes;
  a.off = 0;
  return KOCR_OK;
}
int kocr_ctx::ws_reserve(size_t bytes) { return arena_reserve(this, ws, bytes); }
void arena_guard_fill(Arena&, size_t, size_t) {}  // guard mode stays off here (scripts/host_arena_check.cpp drives it)
void arena_guard_check(Arena&) {}
int crnn_label_width(kocr_ctx*) { return LW; }
int crnn_classes(kocr_ctx*) { return 37; }
size_t crnn_workspace_bytes(int M, int) { return (size_t)M * 64; }
size_t lexicon_workspace_bytes(kocr_ctx*, int M, bool) { return (size_t)M * 16; }
size_t pattern_workspace_bytes(kocr_ctx*, int M, const CrnnPattern&) { return (size_t)M * 8; }
int craft_micro_batch(int micro_batch, int N, int, int) { return std::min(micro_batch > 0 ? micro_batch : 32, N); }

static long crops_seen;
int crnn_forward(kocr_ctx*, const float* d_crops, int M, int* d_labels, float*, CrnnStop, float*, const float**, const CrnnScores* sc,
                 const CrnnBeam* bm, const CrnnLexicon* lx, const CharMask&, const CrnnPattern*) {
  const size_t m = (size_t)M;
  for (size_t i = 0; i < m * CRNN_CROP_PIXELS; ++i) CHECK(d_crops[i] == 0.f);
  memset(d_labels, 1, m * LW * 4);
  if (sc) memset(sc->d_logw, 2, m * 4), memset(sc->d_chars, 3, m * LW * 4);
  if (bm) memset(bm->d_labels, 4, m * bm->top_paths * LW * 4), memset(bm->d_logp, 5, m * bm->top_paths * 4);
  if (lx) memset(lx->d_index, 6, m * lx->top_words * 4), memset(lx->d_logp, 7, m * lx->top_words * 4);
  crops_seen += M;
  return KOCR_OK;
}

static void filled(const void* p, int byte, size_t n) {
  for (size_t i = 0; i < n; ++i) CHECK(((const unsigned char*)p)[i] == byte);
}

int main() {
  kocr_ctx ctx;
  int stages = 0;
  for (long M : {1L, 7L, 1023L, 1024L, 1025L, 2500L})
    for (int sw = 0; sw < 16; ++sw) {
      ctx.scores_on = sw & 1;
      ctx.beam_width = sw & 2 ? 4 : 0;
      ctx.beam_top_paths = sw & 2 ? 3 : 1;
      ctx.lex_top = sw & 4 ? 5 : 0;
      const bool force = sw & 8;
      RecStage rec(&ctx, M, force);
      const size_t m = (size_t)M, crop_b = m * CRNN_CROP_PIXELS * sizeof(float);
      Staging st{&ctx, ctx.io, "host_stage_check"};
      CHECK(st.reserve(0, {}, {crop_b, rec.bytes()}) == KOCR_OK);
      float* crops;
      CHECK(st.scratch(crop_b, crops) == KOCR_OK);
      memset(crops, 0, crop_b);
      CHECK(rec.take(st) == KOCR_OK && ctx.io.off <= ctx.io.cap);
      crops_seen = 0;
      CHECK(rec.run(crops) == KOCR_OK && crops_seen == M);
      const bool scores = ctx.scores_on || force;
      filled(rec.lab, 1, m * LW * 4);
      if (scores) filled(rec.sc.d_logw, 2, m * 4), filled(rec.sc.d_chars, 3, m * LW * 4);
      if (ctx.beam_width) filled(rec.bm.d_labels, 4, m * 3 * LW * 4), filled(rec.bm.d_logp, 5, m * 3 * 4);
      if (ctx.lex_top) filled(rec.lx.d_index, 6, m * 5 * 4), filled(rec.lx.d_logp, 7, m * 5 * 4);
      CHECK(scores || (!rec.sc.d_logw && !rec.sc.d_chars));
      // what stays resident: every record with the state of its switch, and all of them forgotten by the next sizing
      rec.keep();
      CHECK(ctx.last_sc.rec == resident(ctx.scores_on) && ctx.last_sc.M == M && ctx.last_sc.lw == LW);
      CHECK(ctx.last_beam.state == resident(ctx.beam_width > 0) && ctx.last_beam.K == ctx.beam_top_paths);
      CHECK(ctx.last_lex.state == resident(ctx.lex_top > 0) && ctx.last_or.state == Resident::OFF);
      ctx.orient_mode = KOCR_ORIENT_ANY;
      OrientWinners won;
      won.words = M / 2;
      rec.keep(&won);
      CHECK(ctx.last_or.state == Resident::VALID && ctx.last_or.M == M / 2 && ctx.last_sc.M == M / 2);
      ctx.orient_mode = KOCR_ORIENT_OFF;
      CHECK(arena_reserve(&ctx, ctx.pl, 1) == KOCR_OK);
      CHECK(ctx.last_sc.rec == Resident::NONE && ctx.last_sc.det == Resident::NONE && ctx.last_beam.state == Resident::NONE &&
            ctx.last_lex.state == Resident::NONE && ctx.last_or.state == Resident::NONE && ctx.last_ch.state == Resident::NONE &&
            ctx.last_pl.state == Resident::NONE);
      ++stages;
    }
  // no crops: nothing taken, nothing run, "nothing resident, M = 0"
  ctx.scores_on = true;
  ctx.beam_width = 0;
  RecStage(&ctx, 0).keep();
  CHECK(ctx.last_sc.rec == Resident::VALID && ctx.last_sc.M == 0 && !ctx.last_sc.d_logw && ctx.last_beam.state == Resident::OFF);
  // the detector's batch loop covers [0, N) once, in order
  int next = 0;
  CHECK(craft_batches(&ctx, 3, 10, 0, 0, [&](int s, int nb) {
          CHECK(s == next && nb >= 1 && nb <= 3 && ctx.ws.off == 0);
          next += nb;
          return KOCR_OK;
        }) == KOCR_OK && next == 10);
  for (Arena* a : {&ctx.ws, &ctx.io, &ctx.pl}) free(a->base);
  printf("host_stage_check ok: %d stages\n", stages);
  return 0;
}
