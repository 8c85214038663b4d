/* kocr_windows.h -- long words: the calls that read a box too wide for one crop in overlapping windows.  Part of the C ABI of
 * libkocr.so; include it beside kocr.h, which states the rule ("long words"; DESIGN.md section 4, "Long words"; in numpy:
 * tests/windows_statement.py).  tests/test_windows_abi_cpu.py holds this header to what the suite holds kocr.h to: every
 * function exported, with a ctypes signature of the declared length, and on the workspace table of tests/windows_cases.py. */
#ifndef KOCR_WINDOWS_H
#define KOCR_WINDOWS_H

#include "kocr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KOCR_WINDOW_FRAMES_MAX 2048

/* The whole route.  Arguments as kocr_recognize_boxes (boxes [M][4][2] and counts [N] are HOST arrays; on_device: img_rgb is
 * a device pointer) plus aspect and overlap.  The results are RAGGED and stay resident on the context, the two-call pattern of
 * kocr_pipeline_results_shape / kocr_pipeline_results: kocr_windowed_results_shape gives the number of words M and the row
 * width Lmax = the longest T' of the call (no boxes: 0 words of the recogniser's label width); kocr_windowed_results copies
 * labels [M][width] int32 (-1 padded), log_word [M], char_scores [M][width] (0 padded), frames [M] int32 = T' and windows [M]
 * int32 = K into HOST buffers of max_words rows of `width` columns (any pointer may be NULL: not copied); KOCR_ECAPACITY when
 * max_words < M or width < Lmax.  Valid until the next call on the context that sizes a workspace arena; KOCR_EINVAL when
 * nothing is resident.  Profiler rows of its own launches: window_plan, window_stitch, ctc_scores_ragged. */
int kocr_recognize_boxes_windowed(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                                  const int32_t* counts, double aspect, int overlap, int on_device);
int kocr_windowed_results_shape(kocr_ctx* ctx, int32_t* n_words, int32_t* width);
int kocr_windowed_results(kocr_ctx* ctx, int32_t* labels, float* log_word, float* char_scores, int32_t* frames, int32_t* windows,
                          int max_words, int width);

/* The stages alone (unit-test seams; HOST pointers).  d is the context's rnn_steps_to_discard.
 * kocr_window_plan: M boxes [M][4][2] -> windows [M] = K and *n_windows = sum K (both always written once the arguments are
 * valid), and, computed on the device, quads [sum K][4][2] float32 = q_k and ranges [sum K][2] int32 = (lo_k, hi_k);
 * KOCR_ECAPACITY when max_windows < sum K (call it with max_windows = 0 first to learn the size).
 * kocr_warp_crops_windowed: kocr_warp_crops' arguments plus aspect and overlap -> crops [sum K][31][200] and the plan as
 * above (image-major box order).
 * kocr_ctc_stitch_decode: the caller's logits [sum K][50][C] (C = kocr_crnn_classes), windows [M] = K per word and overlap ->
 * labels [M][width], log_word [M], char_scores [M][width], frames [M]; width >= the longest T' (else KOCR_ECAPACITY).  Leaves
 * no result resident. */
int kocr_window_plan(kocr_ctx* ctx, int M, const float* boxes, double aspect, int overlap, int32_t* windows, float* quads,
                     int32_t* ranges, int max_windows, int32_t* n_windows);
int kocr_warp_crops_windowed(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes, const int32_t* counts,
                             double aspect, int overlap, float* crops, int32_t* windows, float* quads, int32_t* ranges,
                             int max_windows, int32_t* n_windows);
int kocr_ctc_stitch_decode(kocr_ctx* ctx, const float* logits, int M, const int32_t* windows, int overlap, int32_t* labels,
                           float* log_word, float* char_scores, int32_t* frames, int width);

#ifdef __cplusplus
}
#endif
#endif /* KOCR_WINDOWS_H */
