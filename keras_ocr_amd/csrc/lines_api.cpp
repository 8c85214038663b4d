// lines_api.cpp — kocr_group_lines (include/kocr.h, "lines"): argument checks, staging, the two launches of lines.hip; with
// flags == KOCR_LINES_BLOCKS the first launch is blocks.hip's instead (the same checks, buffers and staging plan); with
// KOCR_LINES_DESKEW beside it the cut runs on the quads in their page's own frame and the boxes are mapped back before the pack;
// with flags == KOCR_LINES_TABLE the first launch is table.hip's, and the box scratch holds two bands a quad.
#include "abi.h"
#include <cmath>

namespace {

int lines_run(kocr_ctx* ctx, int N, const float* quads, const int32_t* offsets, const LinesRule& rule, int32_t* line_of, int32_t* order,
              int32_t* line_counts, float* line_boxes, int64_t cap_lines, int64_t* true_lines, int flags) {
  const std::string fn("kocr_group_lines");
  if (N < 0 || cap_lines < 0) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": bad sizes");
  if (flags == KOCR_LINES_DESKEW)
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": flags " + std::to_string(flags) + ": KOCR_LINES_DESKEW needs KOCR_LINES_BLOCKS (lines do not depend on the page's rotation)");
  if ((flags & KOCR_LINES_TABLE) && flags != KOCR_LINES_TABLE)
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": flags " + std::to_string(flags) + ": KOCR_LINES_TABLE stands alone (the table rule is axis-aligned and has no blocks)");
  if (flags != 0 && flags != KOCR_LINES_BLOCKS && flags != (KOCR_LINES_BLOCKS | KOCR_LINES_DESKEW) && flags != KOCR_LINES_TABLE)
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": flags " + std::to_string(flags) + " is neither 0 nor KOCR_LINES_BLOCKS, with or without KOCR_LINES_DESKEW, nor KOCR_LINES_TABLE");
  const bool table = flags == KOCR_LINES_TABLE;  // max_offset is min_gap_x, max_gap is min_gap_y, min_height_ratio is min_support
  const bool blocks = (flags & KOCR_LINES_BLOCKS) != 0;  // max_offset is then read as min_gap_x, max_gap as min_gap_y
  const bool deskew = (flags & KOCR_LINES_DESKEW) != 0;  // the cut runs in the page's own frame
  if (!line_boxes && cap_lines != 0) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null line_boxes with cap_lines " + std::to_string((long long)cap_lines));
  // !(a <= x) also refuses a NaN
  if (!(rule.cos_max > 0 && rule.cos_max <= 1))
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": cos_max " + std::to_string(rule.cos_max) + " outside (0, 1] (max_angle must lie in [0, 90) degrees)");
  if (!(rule.min_height_ratio >= 0 && rule.min_height_ratio <= 1))
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": min_height_ratio " + std::to_string(rule.min_height_ratio) + " outside [0, 1]");
  if (!(rule.max_offset >= 0 && std::isfinite(rule.max_offset)))
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": max_offset " + std::to_string(rule.max_offset) + " is not a finite number >= 0");
  if (!(rule.max_gap >= 0 && std::isfinite(rule.max_gap)))
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": max_gap " + std::to_string(rule.max_gap) + " is not a finite number >= 0");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  if (true_lines) *true_lines = 0;
  if (N == 0) return KOCR_OK;
  if (!offsets || !line_counts) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null offsets or line_counts");
  if (offsets[0] != 0) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": offsets must start at 0");
  int max_words = 0;
  for (int i = 0; i < N; ++i) {
    if (offsets[i + 1] < offsets[i]) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": offsets decreases at entry " + std::to_string(i + 1));
    const int words = offsets[i + 1] - offsets[i];
    if (words > KOCR_LINES_MAX_WORDS)
      KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": page " + std::to_string(i) + " holds " + std::to_string(words) +
                                      " words, more than KOCR_LINES_MAX_WORDS = " + std::to_string(KOCR_LINES_MAX_WORDS));
    max_words = std::max(max_words, words);
  }
  const size_t total = (size_t)offsets[N];
  if (total && (!quads || !line_of || !order)) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null buffer");
  if (table && total >= ((size_t)1 << 30)) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": " + std::to_string(total) + " quads, table mode takes fewer than 2^30 in a call");
  for (int i = 0; i < N; ++i)
    for (int j = offsets[i]; j < offsets[i + 1]; ++j)
      for (int c = 0; c < 8; ++c)
        if (!std::isfinite(quads[(size_t)j * 8 + c]))
          KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": page " + std::to_string(i) + ", word " + std::to_string(j - offsets[i]) + ": non-finite coordinate");
  if (total == 0) {
    std::fill(line_counts, line_counts + N, 0);
    return KOCR_OK;
  }

  std::vector<long long> line_off((size_t)N + 1, 0);
  std::vector<int32_t> band_off;  // table mode: where a page's bands stand in the scratch, twice its quad offset
  // line_off is uploaded asynchronously: the stream is drained on every return path before the vector goes
  struct Drain {
    hipStream_t stream;
    ~Drain() { (void)hipStreamSynchronize(stream); }
  } drain{ctx->stream};
  const size_t quads_b = total * 8 * sizeof(float), off_b = ((size_t)N + 1) * sizeof(int32_t), words_b = total * sizeof(int32_t);
  const size_t counts_b = (size_t)N * sizeof(int32_t), line_off_b = ((size_t)N + 1) * sizeof(long long);
  // a page has at most as many lines (or blocks) as words; a table of n words at most 2 n bands (n rows, n columns)
  const size_t boxes_b = line_boxes ? (table ? 2 * quads_b : quads_b) : 0;
  const size_t band_off_b = table && line_boxes ? off_b + 256 : 0;  // the doubled offsets, in table mode only
  // deskew only: the quads in their page's frame and the axes, counted as arena_alloc places them; nothing in the other modes
  const size_t axes_b = (size_t)N * 2 * sizeof(double), frame_b = deskew ? quads_b + 256 + axes_b + 256 : 0;
  Staging st{ctx, ctx->io, "kocr_group_lines", false};
  KOCR_TRY(st.reserve(frame_b + band_off_b, {quads_b, off_b, words_b, words_b, counts_b}, {boxes_b, boxes_b, line_off_b}));
  const float* d_quads;
  const int32_t* d_off;
  int32_t *d_line_of, *d_order, *d_counts;
  float *d_scratch = nullptr, *d_boxes = nullptr;
  KOCR_TRY(st.in(quads, quads_b, d_quads));
  KOCR_TRY(st.in(offsets, off_b, d_off));
  KOCR_TRY(st.out(line_of, words_b, d_line_of));
  KOCR_TRY(st.out(order, words_b, d_order));
  KOCR_TRY(st.out(line_counts, counts_b, d_counts));
  if (line_boxes) KOCR_TRY(st.scratch(boxes_b, d_scratch));
  if (deskew) {
    float* d_frame;
    double* d_axes;
    KOCR_TRY(st.scratch(quads_b, d_frame));
    KOCR_TRY(st.scratch(axes_b, d_axes));
    KOCR_TRY(launch_blocks_axis(ctx, d_quads, d_off, N, max_words, d_axes));
    KOCR_TRY(launch_blocks_frame(ctx, d_quads, d_off, d_axes, N, max_words, d_frame));
    KOCR_TRY(launch_blocks_cut(ctx, d_frame, d_off, N, max_words, rule.max_offset, rule.max_gap, d_line_of, d_order, d_counts, d_scratch));
    if (d_scratch) KOCR_TRY(launch_blocks_unframe(ctx, d_scratch, d_off, d_counts, d_axes, N));
  } else if (table)
    KOCR_TRY(launch_table_grid(ctx, d_quads, d_off, N, max_words, rule.max_offset, rule.max_gap, rule.min_height_ratio, d_line_of, d_order,
                               d_counts, d_scratch));
  else if (blocks)
    KOCR_TRY(launch_blocks_cut(ctx, d_quads, d_off, N, max_words, rule.max_offset, rule.max_gap, d_line_of, d_order, d_counts, d_scratch));
  else
    KOCR_TRY(launch_lines_group(ctx, d_quads, d_off, N, max_words, rule, d_line_of, d_order, d_counts, d_scratch));
  KOCR_TRY(st.back(line_of, d_line_of, words_b));
  KOCR_TRY(st.back(order, d_order, words_b));
  KOCR_TRY(st.back(line_counts, d_counts, counts_b));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the counts size the packed boxes; a failure is reported
  for (int i = 0; i < N; ++i) line_off[i + 1] = line_off[i] + line_counts[i];
  const long long lines = line_off[N];
  if (true_lines) *true_lines = lines;
  if (!line_boxes) return KOCR_OK;
  if (lines > cap_lines)
    KOCR_FAIL(ctx, KOCR_ECAPACITY, fn + ": " + std::to_string(lines) + (table ? " bands" : blocks ? " blocks" : " lines") + ", line_boxes holds " + std::to_string((long long)cap_lines));
  const size_t packed_b = (size_t)lines * 8 * sizeof(float);
  const long long* d_line_off;
  KOCR_TRY(st.upload((const long long*)line_off.data(), line_off_b, d_line_off));
  KOCR_TRY(st.scratch(packed_b, d_boxes));
  const int32_t* d_from = d_off;  // where a page's boxes stand in the scratch
  if (table) {
    band_off.resize((size_t)N + 1);
    for (int i = 0; i <= N; ++i) band_off[i] = 2 * offsets[i];  // total < 2^30: checked above
    KOCR_TRY(st.upload((const int32_t*)band_off.data(), off_b, d_from));
  }
  KOCR_TRY(launch_lines_pack(ctx, d_scratch, d_from, d_line_off, N, d_boxes));
  KOCR_TRY(st.download(line_boxes, (const float*)d_boxes, packed_b));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // results are complete on return; a failure is reported
  return KOCR_OK;
}

}  // namespace

extern "C" {

int kocr_group_lines(kocr_ctx* ctx, int N, const float* quads, const int32_t* offsets, double cos_max, double min_height_ratio,
                     double max_offset, double max_gap, int32_t* line_of, int32_t* order, int32_t* line_counts, float* line_boxes,
                     int64_t cap_lines, int64_t* true_lines, int flags) {
  if (!ctx) return KOCR_EINVAL;
  const LinesRule rule{cos_max, min_height_ratio, max_offset, max_gap};
  return lines_run(ctx, N, quads, offsets, rule, line_of, order, line_counts, line_boxes, cap_lines, true_lines, flags);
}

}  // extern "C"
