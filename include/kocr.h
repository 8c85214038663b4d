/* kocr.h — C-ABI of libkocr.so: the MI355X (gfx950) hot path of
 * keras_ocr.pipeline.Pipeline.recognize().
 *
 * The reference (faustomorales/keras-ocr) is pure Python and has NO FFI; the seams this
 * library replaces are the two Keras `predict` calls and the OpenCV/shapely host loops
 * between them.  Every entry point cites the reference interface it replaces
 * (file:line relative to the reference checkout).
 *
 * Conventions
 *   - every call returns 0 on success, a negative KOCR_E* code on failure;
 *     kocr_last_error() gives the message of the last failure on that ctx.  After a non-zero
 *     return the contents of every OUTPUT buffer of that call are undefined (partial results may
 *     have been written); only documented exceptions hold (KOCR_ECAPACITY: the counts).  When
 *     several failures apply, a data error the reference would raise (KOCR_EEMPTYCONTOUR,
 *     KOCR_EZERODIV) takes precedence over KOCR_ECAPACITY.
 *   - the caller owns every buffer passed in or out; the library owns weights and
 *     workspace.  `on_device` != 0 means the pointers are HIP device pointers on the
 *     ctx's device (e.g. torch.Tensor.data_ptr()); 0 means host pointers (numpy).
 *   - one ctx per device; calls on a ctx are serialised on its HIP stream and are not
 *     re-entrant.  A ctx (its stream, workspace arenas and profiler) belongs to ONE host thread
 *     at a time: the library takes no locks, exactly as the reference documents nothing as
 *     thread-safe (single caller thread, synchronous).  Use one ctx per thread, or serialise
 *     the calls yourself; separate contexts (also on one device) are independent.  Device-pointer calls are asynchronous on that stream unless they
 *     return host-side counts (documented per call).
 *   - tensors are dense, row-major, channels-last (NHWC), exactly the layouts the
 *     reference hands to / receives from Keras.
 */
#ifndef KOCR_H
#define KOCR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kocr_ctx kocr_ctx;

enum {
  KOCR_OK = 0,
  KOCR_EINVAL = -1,   /* bad argument (the reference would raise AssertionError/ValueError) */
  KOCR_EHIP = -2,     /* HIP runtime error */
  KOCR_ENOWEIGHTS = -3, /* forward called before kocr_load_* */
  KOCR_ECAPACITY = -4,  /* caller-provided output capacity too small */
  KOCR_ENOMEM = -5,
  KOCR_EEMPTYCONTOUR = -6, /* reference: IndexError at detection.py:272 */
  KOCR_EZERODIV = -7       /* reference: ZeroDivisionError at tools.py:95 */
};

enum { KOCR_U8 = 0, KOCR_F32 = 1 };

/* ---- context ------------------------------------------------------------------------ */
int kocr_create(kocr_ctx** out, int hip_device);
void kocr_destroy(kocr_ctx* ctx);
const char* kocr_last_error(const kocr_ctx* ctx);
/* Run on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream of a NON-default torch stream).  The
 * call first synchronises the stream the ctx was on, so work queued there is complete when it returns.
 * Handle 0 / NULL selects the ctx's own stream, created with hipStreamNonBlocking.  That includes torch's default stream,
 * whose handle is 0: the library never runs on the legacy default stream.  The ctx's own stream is NOT ordered against the
 * legacy default stream in either direction, so a caller whose device buffers are produced or consumed on the default stream
 * synchronises on both sides -- the device (torch.cuda.synchronize()) before the call, kocr_synchronize() after it -- or
 * works on a non-default stream and hands that one over. */
int kocr_set_stream(kocr_ctx* ctx, void* hip_stream);
int kocr_synchronize(kocr_ctx* ctx);
/* Device-buffer helpers so a host without torch can still keep data resident. */
int kocr_device_alloc(kocr_ctx* ctx, void** out, uint64_t bytes);
int kocr_device_free(kocr_ctx* ctx, void* p);
int kocr_memcpy_h2d(kocr_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int kocr_memcpy_d2h(kocr_ctx* ctx, void* dst, const void* src, uint64_t bytes);

/* ---- weights ------------------------------------------------------------------------ */
/* Both loaders may be called again on a context that already holds weights, and both keep one contract:
 *  - Validate first, change afterwards.  Every required tensor is looked up by name and checked for its size before the
 *    context is touched.  A refused set returns KOCR_EINVAL, kocr_last_error naming the first tensor that is missing
 *    ("missing tensor <name>") or of another size ("tensor <name> has wrong size"), and leaves everything as it was: the
 *    weights and whether they are loaded, the class count, the label width, the lexicon, character sets and patterns, and
 *    the device memory the context holds.  On a context without weights every forward then still returns KOCR_ENOWEIGHTS.
 *  - A reload replaces.  After a successful load the context computes what a new context with that set computes, bit for
 *    bit, and holds the same persistent device memory: every device copy derived from the previous set has been freed (the
 *    stream is drained first).  A recogniser set without the stn_* tensors replaces one with them by a network without the
 *    transformer, whose four layers are freed too.  The stn_* tensors come all eight or not at all: a set with some of them
 *    is refused naming the first that is missing.
 *  - A recogniser of another class count (the length of "fc_12/bias") unloads the lexicon, the character sets and the
 *    patterns, which were validated against the previous count, and gives back the workspace arenas, which were sized for it.
 *    The label width (kocr_crnn_set_rnn_steps_to_discard) is no part of a weight set and stays.
 *  - Should a load fail after its validation (a device allocation or a copy), the network is left NOT loaded
 *    (KOCR_ENOWEIGHTS until a load succeeds), never a mixture of two sets. */
/* CRAFT detector weights.  Replaces detection.build_keras_model(weights_path) +
 * load_torch_weights (detection.py:353-424, 428-468).  `names[i]` are the PyTorch
 * state-dict keys minus the "module." prefix (the naming load_torch_weights uses,
 * detection.py:432-461), e.g. "basenet.slice1.0.weight" (OIHW), "...bias",
 * BN "...weight/bias/running_mean/running_var".  shapes is n x 4 (unused dims = 1). */
int kocr_load_craft(kocr_ctx* ctx, int n, const char* const* names,
                    const float* const* data, const int64_t* shapes, const int* ranks);
/* CRNN recogniser weights.  Replaces recognition.build_model + Recognizer.__init__
 * load_weights (recognition.py:187-350, 365-404).  Names are Keras layer/variable
 * names: "conv_1/kernel" (HWIO) "conv_1/bias" ... "conv_7/...", "bn_3|5|7/gamma|beta|
 * moving_mean|moving_variance", STN localisation net "stn_conv_1/...", "stn_conv_2/...",
 * "stn_dense_1/kernel|bias", "stn_dense_2/...", "fc_9/...", "lstm_10|lstm_10_back|
 * lstm_11|lstm_11_back/kernel|recurrent_kernel|bias", "fc_12/kernel|bias". */
int kocr_load_crnn(kocr_ctx* ctx, int n, const char* const* names,
                   const float* const* data, const int64_t* shapes, const int* ranks);

/* ---- inner seam #1: detector.model.predict (detection.py:779) ------------------------ */
/* img: N x H x W x 3.  dtype KOCR_U8 = raw RGB bytes, normalised in the first conv's
 * loader exactly as detection.compute_input (detection.py:34-42); KOCR_F32 = already
 * normalised.  heat: N x (H/2) x (W/2) x 2 float32 (ch0 text, ch1 link), linear output
 * (detection.py:408-413).  micro_batch <= 0 selects the default (Keras predict's
 * batch_size=32 analogue, detection.py:779). */
int kocr_craft_forward(kocr_ctx* ctx, const void* img, int dtype, int N, int H, int W,
                       float* heat, int micro_batch, int on_device);

/* ---- taps of the detector forward (test seam: one layer at a time against a float64 reference) --------------
 * kocr_craft_set_taps selects launches of kocr_craft_forward by name: the layer names (basenet.slice1.3,
 * basenet.slice5#fold, upconv2.conv.0#y, upconv2.conv.0#skip, conv_cls.4, ...) and maxpool3x3s1, resize:upconv2
 * .. resize:upconv4 (the unfolded decoder's bilinear resize) and head_tail (conv_cls.6 + conv_cls.8); "*" selects
 * every launch, n = 0 turns taps off.  Which launches run depends on the shapes, the arithmetic mode and the
 * schedule.  Every kocr_craft_forward call with taps on restarts the record; for each selected launch it copies to
 * context-owned host memory, ordered on the ctx stream, three parts, each accumulated over all micro-batches:
 *   which = 0  the input view as the launch read it (absent for a uint8 image),
 *   which = 1  the full output after the launch (absent where only the pooled tensor is written; for
 *              resize:upconvN the whole concat buffer, for head_tail the heat-map),
 *   which = 2  the pooled output,
 * each as the logical N x H x W x C float32 tensor (channel slices gathered) with the tensor's per-image max-|x|
 * slots as they stood at that moment (-1: the tensor has no slots).  Taps change no kernel and no result.
 * kocr_craft_tap_count: launches recorded by the last call.  kocr_craft_tap_info: the i-th in launch order --
 * name (64 bytes), kernel (256 bytes: the profiler rows of what the launch ran, '+'-joined, e.g.
 * "conv_w4hr_256x64_pool"), dims[3][4] = N, H, W, C per part (all 0 = absent).  kocr_craft_get_tap synchronises the
 * ctx stream and copies one part: dst N*H*W*C floats, amax_dst N floats (either may be NULL). */
int kocr_craft_set_taps(kocr_ctx* ctx, int n, const char* const* names);
int kocr_craft_tap_count(kocr_ctx* ctx);
int kocr_craft_tap_info(kocr_ctx* ctx, int i, char* name, char* kernel, int32_t* dims);
int kocr_craft_get_tap(kocr_ctx* ctx, const char* name, int which, float* dst, float* amax_dst);

/* ---- taps of the recogniser forward (the same recorder; its readers are the three above) ------------------------
 * kocr_crnn_set_taps selects launches of kocr_crnn_forward by name, replacing any detector taps (one network is
 * recorded at a time; the other network's forward records nothing): conv_1 .. conv_7 (conv_3 / conv_5 on the cell
 * grid: pooled output only, which = 2), pool_3 / pool_5 (the separate pooling of the dense crop batch), cells_to_keras
 * or crnn_to_keras, stn_conv_1, stn_conv_2, stn_dense_1 (input viewed as M x 1 x 1 x 11200), stn_dense_2,
 * stn_sample.theta (no launch: theta as the sampler reads it), stn_sample, fc_9, lstm_10_xproj, lstm_10, lstm_11_xproj,
 * lstm_11 (input xp = [M][50][1][1024]; output [M][50][1][forward | backward], the backward half in processing order),
 * fc_12 and ctc (fc_12's logits in; the probabilities M x 1 x 48 x C out, when kocr_crnn_forward is given them).
 * Tensors in the cell grid (KOCR_CELLS) are recorded one crop per image: the crop's whole cell, H x cellW x C, zero
 * gutters included, with that cell's max-|x| slot. */
int kocr_crnn_set_taps(kocr_ctx* ctx, int n, const char* const* names);

/* ---- detection.getBoxes (detection.py:207-287) ---------------------------------------- */
/* heat: N x h x w x 2 float32.  Thresholds as Detector.detect's keyword arguments
 * (detection.py:748-751).  boxes: N x cap x 4 x 2 float32, corner order and x2 scaling as the
 * reference (clockwise from the min(x+y) corner, or l,t,r,b for near-square boxes); counts:
 * HOST int32[N] (the call synchronises).  Box order inside an image = connected-component
 * label order of cv2.connectedComponentsWithStats (raster order of the first pixel).
 * KOCR_ECAPACITY if an image has more than cap boxes (counts still hold the true numbers);
 * KOCR_EEMPTYCONTOUR where the reference would raise IndexError (a component whose
 * segmentation map is empty after removing text AND link pixels, detection.py:246, 272). */
int kocr_get_boxes(kocr_ctx* ctx, const float* heat, int N, int h, int w, float detection_threshold,
                   float text_threshold, float link_threshold, int size_threshold, float* boxes,
                   int32_t* counts, int cap, int on_device);

/* ---- crops: recognize_from_boxes' cvtColor + tools.warpBox loop (recognition.py:506-526,
 * tools.py:61-117) ---------------------------------------------------------------------- */
/* img_rgb: N x H x W x 3 uint8 (device if on_device).  boxes: HOST float32 [M][4][2], the
 * images' boxes concatenated in image order; counts: HOST int32[N], sum = M.  crops:
 * M x target_h x target_w float32 = gray/255, zero outside the warped region (device if
 * on_device).  KOCR_EZERODIV where the reference raises ZeroDivisionError (box with integer
 * width or height 0, tools.py:95).  The call synchronises, on_device too: the warp parameters
 * come from the HOST boxes, and the crops are complete on return. */
int kocr_warp_crops(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                    const int32_t* counts, int target_h, int target_w, float* crops, int on_device);

/* ---- float images (round 5) --------------------------------------------------------------------------------------------
 * The reference hands cv2 whatever dtype it is given: a float image is resized, converted to gray and warped IN FLOAT
 * (tools.py:394, recognition.py:507-526).  These are the float forms of kocr_resize_pad / kocr_warp_crops: bilinear with
 * half-pixel centres and replicated border, float32 arithmetic (horizontal then vertical pass); gray = 0.299 R + 0.587 G +
 * 0.114 B, perspective warp with 1/32-pixel source coordinates, float weights and constant-0 border, the crop NOT divided by
 * 255 (the caller's, recognition.py:524).  channels = 3 (RGB) or 1 (gray) for the warp, any for the resize.  Host pointers. */
int kocr_resize_pad_f32(kocr_ctx* ctx, const float* src, int n, int sh, int sw, int channels, int dh, int dw, int Hmax, int Wmax,
                        float cval, float* dst);
int kocr_warp_crops_f32(kocr_ctx* ctx, const float* img, int N, int H, int W, int channels, const float* boxes,
                        const int32_t* counts, int target_h, int target_w, float* crops);

/* The general form of tools.warpBox (tools.py:61-117: margin, skip_rotate, target size taken from the box,
 * return_transform): the caller states the ordered source quad and the destination quad of each of the M crops;
 * cv2.getPerspectiveTransform (8x8 float64 LU, on the device) + cv2.warpPerspective as above.  All buffers are HOST
 * arrays: src_quads / dst_quads float32 [M][4][2]; image_index int32[M] (which of the N images); crop_w / crop_h
 * int32[M] = dsize of the warp (clipped to the target); crops M x target_h x target_w float32 gray/255, zero
 * outside the crop; transforms (optional) float64 [M][3][3] = the matrices M the reference returns. */
int kocr_warp_quads(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, int M, const float* src_quads,
                    const float* dst_quads, const int32_t* image_index, const int32_t* crop_w, const int32_t* crop_h,
                    int target_h, int target_w, float* crops, double* transforms);

/* ---- inner seam #2: recognizer.prediction_model.predict (recognition.py:535) ------------ */
/* crops: M x 31 x 200 float32 in [0,1] (the (M,31,200,1) array recognize_from_boxes builds,
 * recognition.py:524-526).  labels: M x 48 int32, the CTCDecoder output: greedy decode,
 * repeats merged, blank (= n_classes-1) removed, -1 padded (recognition.py:169-184).
 * probs (may be NULL): M x 48 x n_classes float32 = recognizer.model.predict, the softmax
 * after dropping the first 2 steps (recognition.py:322-328). */
int kocr_crnn_forward(kocr_ctx* ctx, const float* crops, int M, int32_t* labels, float* probs,
                      int on_device);
/* len(alphabet) + 1 of the loaded recogniser (recognition.py:323), 0 if none is loaded. */
int kocr_crnn_classes(kocr_ctx* ctx);
/* Non-default recogniser builds (recognition.py:187-198 build_params; round 6).  `stn=False` (recognition.py:243) needs no call:
 * kocr_load_crnn on a weight set WITHOUT the stn_* tensors builds the model without the spatial transformer.
 * `rnn_steps_to_discard` (recognition.py:328; default 2): every "48" in this header -- the label rows of kocr_crnn_forward,
 * kocr_recognize_boxes, kocr_pipeline and the probability rows -- is kocr_crnn_label_width() = 50 - steps columns. */
int kocr_crnn_set_rnn_steps_to_discard(kocr_ctx* ctx, int steps);
int kocr_crnn_label_width(kocr_ctx* ctx);

/* ---- the recogniser's other two models: recognizer.backbone and recognizer.training_model (recognition.py:319-349) ---- */
/* keras.backend.ctc_batch_cost(y_true, y_pred, input_length, label_length) (recognition.py:340-347), forward only; the rule
 * is DESIGN.md section 4: q_t = (y_t + 1e-7) / sum (y_t + 1e-7), blank = C - 1, loss = -log of the summed probability of
 * every alignment of labels[m][0 .. label_lengths[m]) to the first input_lengths[m] frames.  y_pred: M x T x C float32
 * probabilities; labels: HOST int32 rows of label_stride entries (entries from label_lengths[m] on are ignored; the
 * reference pads with -1); label_lengths / input_lengths: HOST int32[M]; loss: float32[M].  y_pred and loss are device
 * pointers when on_device is set.  KOCR_EINVAL, naming the sample, before anything is launched: input_lengths[m] outside
 * [1, T], label_lengths[m] outside [0, min(input_lengths[m], label_stride)], a label outside [0, C - 2].  A label that
 * fits in length but not with a blank between its repeats ("aa" in 2 frames) has loss +inf.
 * The call SYNCHRONISES the ctx stream before it returns, on_device too: the labels and lengths are packed into a host
 * staging buffer of the call and copied from there on the stream, and the call waits for the stream at its end so that the
 * buffer may go.  The loss is therefore complete on return. */
int kocr_ctc_batch_cost(kocr_ctx* ctx, const float* y_pred, int M, int T, int C, const int32_t* labels, int label_stride,
                        const int32_t* label_lengths, const int32_t* input_lengths, float* loss, int on_device);
/* recognizer.training_model.predict([crops, labels, input_length, label_length]) (recognition.py:334-349): the recogniser
 * up to fc_12, then kocr_ctc_batch_cost's rule on fc_12's softmax, with T = kocr_crnn_label_width() (the frames after
 * rnn_steps_to_discard).  The probabilities never leave HBM and are bit for bit those kocr_crnn_forward returns, so the
 * loss equals kocr_ctc_batch_cost on them bit for bit.  crops: M x 31 x 200 float32 (device when on_device), loss:
 * float32[M] (device when on_device); labels and lengths as kocr_ctc_batch_cost (HOST arrays), and for the same reason the
 * call SYNCHRONISES the ctx stream at the end of every batch of 1024 crops, on_device too: the loss is complete on return. */
int kocr_crnn_ctc_loss(kocr_ctx* ctx, const float* crops, int M, const int32_t* labels, int label_stride,
                       const int32_t* label_lengths, const int32_t* input_lengths, float* loss, int on_device);
/* recognizer.backbone.predict (recognition.py:319-320): feats M x 50 x 256 float32, the Concatenate output
 * [lstm_11 | lstm_11_back] of every RNN step (rnn_steps_to_discard does not apply).  Buffers are device pointers when
 * on_device is set. */
int kocr_crnn_features(kocr_ctx* ctx, const float* crops, int M, float* feats, int on_device);

/* ---- the detector's training data and validation loss (detection.py:106-198, :696, :698-743) ---- */
/* detection.compute_maps for N pages of H x W (both even) with one uint8 heat-map (hh x hw, detection.get_gaussian_heatmap):
 * maps N x H/2 x W/2 x 2 float32, text then link, equal bit for bit to the full-map statement tests/maps_statement.py
 * (DESIGN.md section 4).  The characters of all pages, line after line: char_quads n_chars x 4 x 2 float32 (the points as
 * given; the rotated box is taken here), is_space uint8[n_chars] (a " " character: resets the link chain, draws nothing),
 * line_offsets int32[n_lines + 1] (line l = characters [line_offsets[l], line_offsets[l + 1]), a non-empty range),
 * image_line_offsets int32[N + 1] (page i = lines [image_line_offsets[i], image_line_offsets[i + 1])).  All buffers are device
 * pointers when on_device is set; host offsets are checked (KOCR_EINVAL), device ones are only clamped to the buffers.
 * KOCR_EINVAL for an odd H or W (the reference's AssertionError). */
int kocr_compute_maps(kocr_ctx* ctx, const uint8_t* heatmap, int hh, int hw, int N, int H, int W, int n_chars,
                      const float* char_quads, const uint8_t* is_space, int n_lines, const int32_t* line_offsets,
                      const int32_t* image_line_offsets, float* maps, int on_device);
/* The per-image half of Keras' compiled "mse" (detection.py:696) on N maps of h x w x 2: sums[n] = sum over the pixels of
 * the mean over the two channels of (y_true - y_pred)^2, float64, in a fixed order.  model.evaluate's loss is
 * sum_n weight_n sums[n] / (N h w).  All buffers are device pointers when on_device is set. */
int kocr_heat_mse(kocr_ctx* ctx, const float* y_true, const float* y_pred, int N, int h, int w, double* sums, int on_device);
/* kocr_craft_forward (arguments as there) and kocr_heat_mse against y_true (N x H/2 x W/2 x 2) in one call: the heat-maps
 * stay in HBM and are bit for bit those kocr_craft_forward returns, so sums equal kocr_heat_mse on them bit for bit. */
int kocr_craft_mse(kocr_ctx* ctx, const void* img, int dtype, int N, int H, int W, const float* y_true, int micro_batch,
                   double* sums, int on_device);

/* ---- evaluation: scoring predictions against labelled pages (evaluation.py:13-53 iou_score, :56-147 score) ----------------
 * The rule is tests/evaluation_statement.py ("Evaluation"): a box is four int32 corners (the caller
 * expands a 2-point box and truncates to int32 as evaluation.py:31-38 does); each quad is put into counter-clockwise order and
 * cut into two triangles by ear clipping, the intersection is the sum over the 2 x 2 triangle pairs of the Sutherland-Hodgman
 * clip, all in float64 in the statement's operation order -- the IoUs equal the statement's bit for bit.
 * N images; truth_quads int32 [nt][4][2] with truth_offsets int32 [N + 1] (image i = truths [truth_offsets[i],
 * truth_offsets[i + 1])), pred_quads / pred_offsets likewise.  Pairs are numbered image-major, truth-major inside an image:
 * P = sum_i nt_i * np_i.  `P` is the capacity, in pairs, of the caller's per-pair buffers; when it is too small the call
 * returns KOCR_ECAPACITY.  *P_true (may be NULL) receives the true P whenever the offsets were accepted.
 * kocr_iou_table (evaluation.py:13-53 for every pair): iou float64 [P]; a box of zero area gives 0.
 * kocr_score (evaluation.py:56-147): ignore uint8 [nt]; truth_text / pred_text: the texts (translator already applied) as
 * concatenated int32 code points with truth_text_offsets int32 [nt + 1] / pred_text_offsets int32 [np + 1], at most
 * KOCR_SCORE_MAX_TEXT code points each.  Outputs: pair_class uint8 [P] -- 0 iou < iou_threshold; 1 true positive; 2 near true
 * positive (text similarity 1 - levenshtein / longest < similarity_threshold, float64; two empty texts: 1); 3 overlap with an
 * ignored truth --, truth_missed uint8 [nt] (not ignored and no pair of class != 0), pred_unclaimed uint8 [np] (no pair of
 * class != 0, ignored truths included), counts int64 [3] = {truths with a class-1 pair, unclaimed predictions, missed truths}
 * (precision = counts[0] / (counts[0] + counts[1]), recall = counts[0] / (counts[0] + counts[2])), iou float64 [P] or NULL.
 * Three launches (profiler rows eval_iou, eval_text, eval_reduce); the Levenshtein distance is computed only for the pairs of
 * class 1 / 2.  An image's results do not depend on what else is in the batch.  N = 0, images without truths or without
 * predictions and P = 0 are valid.
 * on_device: every buffer except P_true is then a device pointer.  The four offset arrays are read back to the host (the call
 * synchronises for that) and checked either way: they start at 0, never decrease, and no text is longer than
 * KOCR_SCORE_MAX_TEXT -- KOCR_EINVAL naming the image or annotation, before anything is launched; host quads are also checked
 * for |coordinate| < 2^24 (KOCR_EINVAL naming image and annotation); device quads are not looked at: larger coordinates
 * lose exactness, nothing else.  The results are complete on return, also on_device.  Workspace comes from the context's staging arena: like every other call that processes
 * images, the two end the validity of resident pipeline results, scores, beams and lexicon matches. */
#define KOCR_SCORE_MAX_TEXT 256
int kocr_iou_table(kocr_ctx* ctx, int N, const int32_t* truth_quads, const int32_t* truth_offsets, const int32_t* pred_quads,
                   const int32_t* pred_offsets, double* iou, int64_t P, int64_t* P_true, int on_device);
int kocr_score(kocr_ctx* ctx, int N, const int32_t* truth_quads, const int32_t* truth_offsets, const int32_t* pred_quads,
               const int32_t* pred_offsets, const uint8_t* ignore, const int32_t* truth_text, const int32_t* truth_text_offsets,
               const int32_t* pred_text, const int32_t* pred_text_offsets, double iou_threshold, double similarity_threshold,
               uint8_t* pair_class, uint8_t* truth_missed, uint8_t* pred_unclaimed, int64_t* counts, double* iou, int64_t P,
               int64_t* P_true, int on_device);

/* ---- lines: recognised words grouped into text lines, in reading order (no reference counterpart) ---------------------------
 * The rule is tests/lines_statement.py ("Lines"), float64 in the statement's operation order: the
 * integers equal the statement's and the line boxes carry its float32 bits.  A word is a quad [tl, tr, br, bl] as
 * kocr_get_boxes returns it.  Two words link when their directions differ by at most max_angle (cos_max = cos(max_angle), a
 * double the caller computes once; max_angle in [0, 90) degrees, so cos_max in (0, 1]), the smaller height is at least
 * min_height_ratio (in [0, 1]) of the larger, their centres lie at most max_offset (>= 0) smaller heights apart across the
 * joint axis, and the gap between them along it is at most max_gap (>= 0) larger heights.  Lines are the connected
 * components; a word without width or height is a line of its own.  Inside a line the words are ordered along the summed
 * direction of its members; the line box is the bounding rectangle ALONG that axis (not a min-area rectangle); lines are
 * ordered by the y, then the x of the box centre, then the smallest member.  Columns are not detected.
 * N pages; quads float32 [total][4][2] with offsets int32 [N + 1] (page i = words [offsets[i], offsets[i + 1])), at most
 * KOCR_LINES_MAX_WORDS words on a page.  Outputs: line_of int32 [total], the index of word j's line among its page's lines;
 * order int32 [total], per page (at the page's offset) the page-local word indices in reading order, line 0's words, then
 * line 1's, ...; line_counts int32 [N]; line_boxes float32 [cap_lines][4][2], all lines of all pages in that order
 * (tl, tr, br, bl along the line).  cap_lines is the capacity of line_boxes in lines: with more lines the call returns
 * KOCR_ECAPACITY; *true_lines (may be NULL) receives the number of lines whenever the kernel ran, and line_of / order /
 * line_counts are complete then too (total is always enough).  line_boxes == NULL with cap_lines == 0 skips the boxes.
 * KOCR_EINVAL with a message, before anything is launched: offsets that do not start at 0 or decrease, a page above
 * KOCR_LINES_MAX_WORDS (naming the page and its count), a non-finite coordinate (naming page and word), a rule parameter out of
 * range.  N == 0 and pages without words are valid.  All buffers are HOST arrays; flags is 0, KOCR_LINES_BLOCKS,
 * KOCR_LINES_BLOCKS | KOCR_LINES_DESKEW or KOCR_LINES_TABLE (all below), anything else KOCR_EINVAL with a message that names flags.  Two launches on the ctx stream (profiler rows lines_group,
 * lines_pack), one workgroup per page; a page's results do not depend on what else is in the batch.  The results are
 * complete on return.  Workspace comes from the staging arena: like every other call that processes images it ends the
 * validity of resident pipeline results.
 *
 * flags == KOCR_LINES_BLOCKS: the quads of a page -- any quads, in practice the line boxes of a call with flags == 0 -- are cut
 * into BLOCKS (columns, paragraphs) by a recursive XY-cut and returned in reading order.  The rule is tests/blocks_statement.py
 * ("Blocks"): a quad counts as its axis-aligned box; H is the mean height of the boxes that have one;
 * along an axis the gap in front of a box is its start minus the largest end of the boxes of its set that start before it,
 * and it is valid when it is > 0 and >= min_gap H.  A set with valid gaps along x is cut at ALL of them (columns, gutters,
 * sidebars), the parts taken left to right; otherwise, with valid gaps along y, at ONE, the widest (the topmost of equal
 * ones), the upper part first; otherwise it is a block.  Inside a block the quads are ordered by (top, left, index); a block's
 * box is the axis-aligned box of its members.  The cut is axis-aligned -- a rotated page needs KOCR_LINES_DESKEW (below) --
 * and whitespace is its only cue: a paragraph gap wider than the heading's and the footer's is cut first.
 * How the arguments are read: max_offset is min_gap_x and max_gap is min_gap_y, both finite and >= 0 (the same check and
 * message); cos_max and min_height_ratio are validated as ever and not read.  What the outputs hold: line_of[j] is the block
 * of quad j among its page's blocks; order holds, per page, the page-local indices block after block; line_counts the
 * blocks per page; line_boxes / cap_lines / true_lines the block boxes [tl, tr, br, bl], with the same KOCR_ECAPACITY
 * contract.  Every other check and its message is the one above; a page has at most as many blocks as quads, so the
 * workspace is the same.  Profiler rows blocks_cut, lines_pack.  A call with flags == 0 launches and returns exactly what
 * it did before this flag existed.
 *
 * flags == KOCR_LINES_BLOCKS | KOCR_LINES_DESKEW (5): block mode for ROTATED pages -- a skewed scan, a photo, a page fed in
 * sideways or upside down.  The rule is tests/deskew_statement.py ("Rotated pages"), float64 in the
 * statement's operation order.  Every quad has a direction u = a / |a| with a = (tr + br) / 2 - (tl + bl) / 2 and the weight
 * w = |a| (the per-word arithmetic of line mode); a quad with w == 0 has none.  The page's axis A is the weighted medoid of
 * the directions: the u_k with the smallest sum over j of w_j |u_k - u_j|, the smallest k among equal ones; (1, 0) on a page
 * without any direction.  The chord |u_k - u_j| grows with the angle up to 180 degrees, so an upside-down page has its own
 * axis, and a medoid is a median: a minority of short quads turned by 90 degrees does not pull it.  Every corner is
 * expressed in the frame (A, V), V = (-A.y, A.x), and rounded to float32; the cut above runs on those quads unchanged; the
 * block boxes come back as ROTATED rectangles in page coordinates, tl = X0 A + Y0 V, tr = X1 A + Y0 V, br = X1 A + Y1 V,
 * bl = X0 A + Y1 V of the cut's frame box, so tl -> tr is the page's text direction, as for line boxes.  On a page whose
 * directions are all exactly (1, 0) the results equal plain block mode's as numbers.  Inputs, outputs, the capacity
 * protocol, every check and its message are block mode's.  The workspace grows by the frame quads (total x 8 floats) and
 * the axes (N x 2 doubles), planned in the same single request and in this mode only.  Profiler rows blocks_axis (one
 * workgroup per page, n^2 chords), blocks_frame, blocks_cut, blocks_unframe (only with line_boxes), lines_pack; nothing waits
 * on the host between them.  KOCR_LINES_DESKEW without KOCR_LINES_BLOCKS (4) is KOCR_EINVAL naming flags: lines do not depend
 * on the page's rotation, and re-ordering them by a page axis is not built.  Not covered: a page whose text runs in several
 * directions, and a page turned by 90 or 180 degrees whose quads do not run tl -> tr along the text (read such words with
 * an orientation mode first).  Calls with flags == 0 and flags == KOCR_LINES_BLOCKS launch, reserve and return exactly what
 * they did before this flag existed.
 *
 * flags == KOCR_LINES_TABLE (16): the quads of a page -- any quads, in practice the word boxes of ONE table: a whole page, or the
 * words of one block -- are put into ROWS, COLUMNS and spanning cells by the white space between them.  The rule is
 * tests/table_statement.py ("Tables"): a quad counts as its axis-aligned box; H is the mean height as in
 * block mode, tx = min_gap_x H, ty = min_gap_y H.  Rows: the page by (top, index) is cut at ALL gaps along y that are > 0 and
 * >= ty (a gap is a box's top minus the largest bottom before it); nothing recurses.  A row's white intervals are its gaps
 * along x that are > 0 and >= tx, and its two margins up to the page's extent, whatever their width: a short row does not
 * vote against the columns it does not reach.  Where at least K = max(1, ceil(min_support R)) of the R rows are white, over
 * a maximal stretch (a, b) with b - a >= tx that ends before the page's right edge, stands a separator; S separators make
 * S + 1 columns.  Quad j lies in the columns col0 = #{b_s <= its left} to col1 = max(col0, #{b_s < its right}); col1 > col0
 * is a spanning cell (a title row, a merged header).
 * How the arguments are read: max_offset is min_gap_x and max_gap is min_gap_y, both finite and >= 0 (block mode's check and
 * message); min_height_ratio is min_support, under its [0, 1] check; cos_max is validated as ever and not read.  What the
 * outputs hold: line_of[j] is the row of quad j; order[j] is col0 | col1 << 16; line_counts[i] = R_i + S_i + 1, the page's
 * bands (0 for a page without quads; R_i = 1 + the largest line_of of the page, every row has a member); line_boxes holds,
 * per page, its R_i row bands (the page's width, the row's members' height) and then its S_i + 1 column bands (from the page's
 * left edge or b_{k-1} to a_k or the right edge, the page's height), [tl, tr, br, bl], under the same cap_lines / true_lines /
 * KOCR_ECAPACITY contract.  A page of n quads has at most 2 n bands (S <= n - 1: every b_s is the left edge of a box other
 * than the leftmost), so the box workspace is planned for 2 total quads, in the same single request and in this mode only.
 * Every other check and its message is the one above.  Profiler rows table_grid (one workgroup per page), lines_pack.
 * KOCR_LINES_TABLE stands alone: every other value that contains it (17, 20, 21, 48, ...) is KOCR_EINVAL naming flags, before
 * anything is launched -- the rule is axis-aligned, so there is no deskewed table.  Not covered: several tables in one call
 * (pass each table's words as a page of its own), ruling lines (whitespace is the only cue), a cell whose text wraps (two
 * rows unless min_gap_y is raised).  Calls with flags 0, 1 and 5 launch, reserve and return exactly what they did before this
 * flag existed. */
#define KOCR_LINES_MAX_WORDS 2048
#define KOCR_LINES_BLOCKS 1
#define KOCR_LINES_DESKEW 4
#define KOCR_LINES_TABLE 16
int kocr_group_lines(kocr_ctx* ctx, int N, const float* quads, const int32_t* offsets, double cos_max, double min_height_ratio,
                     double max_offset, double max_gap, int32_t* line_of, int32_t* order, int32_t* line_counts, float* line_boxes,
                     int64_t cap_lines, int64_t* true_lines, int flags);

/* ---- characters: the character boxes of word boxes, read off the detector's region map (no reference counterpart) ----------
 * The rule is tests/chars_statement.py ("Characters"), float64 in the statement's operation order: the
 * counts equal the statement's and the quads and scores carry its float32 bits.  Channel 0 of a heat-map is a per-character
 * Gaussian score.  A word is a quad [tl, tr, br, bl] in detector-input pixels as kocr_get_boxes returns it (heat-map pixels
 * x 2).  Its region is sampled bilinearly (pixels outside the map count as 0) on a grid of n_cols = min(KOCR_CHARS_MAX_COLS,
 * ceil(width)) by n_rows = min(KOCR_CHARS_MAX_ROWS, ceil(height)) cells, width and height in heat-map pixels; the profile
 * is the maximum over the rows per column.  Columns below extent_threshold at either end are trimmed; a column is a peak
 * candidate when it reaches peak_threshold, exceeds its left and is not below its right neighbour; scanning from the left,
 * a candidate starts a new character when the profile's minimum since the current peak is at most valley_ratio x the lower
 * of the two peaks (the cut is that minimum's first column), and otherwise replaces the current peak when it is higher.
 * Every character is a slice of the word quad between two cuts, at the word's full height; its score is the profile at
 * its peak.  The profile runs along tl -> tr whatever the text's direction; characters whose blobs merge above
 * valley_ratio come out as one box; a word without width or height, or without a peak, has no characters.
 * heat N x h x w x 2 float32 (a device pointer when on_device is set); quads float32 [total][4][2] with offsets int32
 * [N + 1] (page i = words [offsets[i], offsets[i + 1])), both HOST arrays.  Outputs, all HOST: char_counts int32 [total];
 * char_quads float32 [cap_chars][4][2] and char_scores float32 [cap_chars], all characters of all words in word order.
 * cap_chars is their capacity in characters: with more the call returns KOCR_ECAPACITY; *true_chars (may be NULL) receives
 * the number of characters whenever the kernel ran, and char_counts is complete then too.  char_quads == NULL with cap_chars
 * == 0 skips the boxes and scores.  KOCR_EINVAL with a message, before anything is launched: offsets that do not start at 0
 * or decrease, a non-finite coordinate (naming page and word), a parameter out of range -- all finite, 0 < peak_threshold,
 * 0 <= valley_ratio <= 1, 0 <= extent_threshold <= peak_threshold.  N == 0 and pages without words are valid; flags is
 * reserved and must be 0.  Two launches on the ctx stream (profiler rows chars_split, chars_pack), one wave per word; a
 * word's results do not depend on what else is in the batch.  The results are complete on return.  Like every other call that
 * processes images it ends the validity of resident results.
 * kocr_set_char_boxes(ctx, 1, ...) (default off; kocr_get_char_boxes returns the switch and the parameters, any pointer may
 * be NULL) makes kocr_get_boxes / kocr_detect / kocr_pipeline run the same two launches on the heat-maps and boxes they have
 * in HBM, after the post-processing that succeeded, and leave the characters resident; with on == 0 the parameters are
 * ignored and kept, and the calls launch and allocate what they always did.  kocr_detection_char_boxes fetches them:
 * char_counts N x cap int32 (row i holds counts[i] values in box order, the rest 0), cap >= the cap the results were produced
 * with (as kocr_detection_scores); char_quads / char_scores / cap_chars / true_chars as above (KOCR_ECAPACITY with
 * *true_chars and char_counts complete; NULL with 0 skips them).  Valid and refused like kocr_detection_scores: until the next
 * call on the context that processes images, KOCR_EINVAL when nothing is resident or when the results were produced with the
 * switch off; after KOCR_ECAPACITY from kocr_pipeline they are resident together with kocr_pipeline_results'. */
#define KOCR_CHARS_MAX_COLS 512
#define KOCR_CHARS_MAX_ROWS 32
int kocr_char_boxes(kocr_ctx* ctx, const float* heat, int N, int h, int w, const float* quads, const int32_t* offsets,
                    double peak_threshold, double valley_ratio, double extent_threshold, int32_t* char_counts, float* char_quads,
                    float* char_scores, int64_t cap_chars, int64_t* true_chars, int on_device, int flags);
int kocr_set_char_boxes(kocr_ctx* ctx, int on, double peak_threshold, double valley_ratio, double extent_threshold);
int kocr_get_char_boxes(const kocr_ctx* ctx, int* on, double* peak_threshold, double* valley_ratio, double* extent_threshold);
int kocr_detection_char_boxes(kocr_ctx* ctx, int32_t* char_counts, float* char_quads, float* char_scores, int cap, int64_t cap_chars,
                              int64_t* true_chars);

/* ---- Detector.detect (detection.py:745-785): compute_input + predict + getBoxes in one call; the
 * heat-maps stay in HBM.  Arguments as kocr_craft_forward + kocr_get_boxes; counts is a HOST array. */
int kocr_detect(kocr_ctx* ctx, const void* img, int dtype, int N, int H, int W,
                float detection_threshold, float text_threshold, float link_threshold,
                int size_threshold, int micro_batch, float* boxes, int32_t* counts, int cap,
                int on_device);

/* ---- Recognizer.recognize_from_boxes (recognition.py:491-537) for N same-sized images: gray
 * conversion + warpBox crops + prediction_model.predict without leaving HBM.  boxes [M][4][2],
 * counts [N] and labels [M][48] are HOST buffers; img_rgb is a device pointer if on_device. */
int kocr_recognize_boxes(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W,
                         const float* boxes, const int32_t* counts, int32_t* labels, int on_device);

/* ---- tools.resize_image + tools.pad (tools.py:356-398; pipeline.py:44-57) -------------- */
/* src: n x sh x sw x 3 uint8 (n images of one size); each is resized to dh x dw exactly as
 * cv2.resize(image, dsize=(dw, dh)) (INTER_LINEAR, uint8 fixed point) and written to the
 * top-left of an Hmax x Wmax canvas filled with cval (255 for tools.pad, tools.py:356; 0 for the
 * letterbox of Recognizer.recognize, tools.py:442, recognition.py:473-478).  dst: n x Hmax x Wmax x 3.
 * The interpolation tables of the two axes are built in a host vector local to the call and copied to the device on the
 * stream; the call SYNCHRONISES the ctx stream right after that copy, on_device too, so that the vector may go.  The resize
 * launch behind it is asynchronous: on return everything queued ahead of the call has finished, dst has not. */
int kocr_resize_pad(kocr_ctx* ctx, const uint8_t* src, int n, int sh, int sw, int dh, int dw,
                    int Hmax, int Wmax, int cval, uint8_t* dst, int on_device);

/* ---- the fused path of Pipeline.recognize (pipeline.py:28-75) ---------------------------- */
/* imgs[i]: RGB uint8 image i of size hs[i] x ws[i] (device pointers if on_device); dhs/dws:
 * its size after tools.resize_image (the caller applies the scale rule of tools.py:387-397,
 * int(h*scale), int(w*scale)); Hmax/Wmax: the batch's padded size (pipeline.py:48-57).
 * Runs resize+pad -> CRAFT -> getBoxes -> warp crops -> CRNN -> CTC decode without leaving HBM.
 * Outputs (HOST): boxes N x cap x 4 x 2 in detector-input pixels (the caller divides by its
 * scale, tools.adjust_boxes / pipeline.py:66-71), counts[N], labels [sum(counts)] x 48 (-1
 * padded, image-major, box order), n_crops = sum(counts).  KOCR_ECAPACITY if an image has more
 * than cap boxes or sum(counts) > max_crops (counts / n_crops hold the true numbers). */
int kocr_pipeline(kocr_ctx* ctx, int N, const uint8_t* const* imgs, const int32_t* hs,
                  const int32_t* ws, const int32_t* dhs, const int32_t* dws, int Hmax, int Wmax,
                  float detection_threshold, float text_threshold, float link_threshold,
                  int size_threshold, int micro_batch, float* boxes, int32_t* counts, int cap,
                  int32_t* labels, int max_crops, int32_t* n_crops, int on_device);

/* The same results where kocr_pipeline left them in HBM (round 5): d_boxes [N][cap][4][2] float32 (rows >= counts[i] of an
 * image undefined), d_counts [N] int32, d_labels [M][label width] int32 (M = sum of the counts; NULL when M == 0; the width: see below).  Valid only until
 * the next libkocr call on this context that processes images (the buffers live in the context's arenas); KOCR_EINVAL when
 * no result is resident.  For callers that hand the results to another device-side consumer -- keras_ocr_amd.dist packs
 * them on the device and all-gathers them over RCCL without a host round trip. */
/* Capacity without recomputation (round 6).  cap / max_crops size the CALLER's buffers only: when an image has more boxes than
 * cap, or there are more crops than max_crops, kocr_pipeline still runs the whole chain once (a larger device box buffer, the
 * post-processing alone repeated on the resident heat-maps), leaves the results in HBM and returns KOCR_ECAPACITY with the
 * true counts / n_crops.  This call copies them into buffers sized from those numbers: boxes N x cap x 4 x 2 (cap >= the
 * largest count), labels n_crops x label width.  Valid until the next libkocr call on this context that processes images.
 *
 * The width contract: resident label rows keep the width they were PRODUCED with.  kocr_crnn_set_rnn_steps_to_discard between
 * kocr_pipeline and a fetch changes kocr_crnn_label_width() but neither the rows nor their pitch: kocr_pipeline_results copies
 * n_crops rows of the produced width, densely, and writes nothing behind them; d_labels of kocr_pipeline_device_results is
 * [M][produced width].  kocr_pipeline_results_shape reports that width (and M) -- *n_crops / *label_width, either may be NULL;
 * KOCR_EINVAL when no result is resident -- as kocr_recognition_scores / _beams report the width of their rows.  Size the label
 * buffer from it, not from kocr_crnn_label_width(), whenever the build parameter may have changed since the call. */
int kocr_pipeline_results(kocr_ctx* ctx, float* boxes, int cap, int32_t* labels, int max_crops);

int kocr_pipeline_device_results(kocr_ctx* ctx, const float** d_boxes, const int32_t** d_counts, const int32_t** d_labels,
                                 int32_t* N, int32_t* cap, int32_t* M);
int kocr_pipeline_results_shape(kocr_ctx* ctx, int32_t* n_crops, int32_t* label_width);

/* ---- tiled pages: a page larger than the detector takes in one image, read in overlapping tiles (DESIGN.md section 4,
 * "Tiled pages"; statement: tests/tiling_statement.py) ------------------------------------------------------------------------
 * The detector addresses one image with 32-bit byte offsets, which ends below one A4 page at 300 dpi.  It is fully
 * convolutional, so a page is read as tiles with a halo: the resized page lies in the top-left corner of a canvas padded with
 * 255 (tools.pad), tile_gather copies the overlapping tiles into one batch, the detector runs on that batch, and heat_stitch
 * copies every pixel of the page's heat-map, bit for bit, from the one tile whose core contains it (no blending).  Everything
 * behind the heat-map runs unchanged on the stitched map.
 *
 * The plan, with tile T and overlap O in detector-input pixels: T a multiple of 32, T >= 64; O a multiple of 16, O >= 0; the
 * stride S = T - 2 O >= 32.  Per axis of length d >= 1: n = 1 tiles if d <= T, else ceil((d - T) / S) + 1; tile k starts at
 * k S; the canvas is (n - 1) S + T long; the core of tile k is [k S + (O if k > 0 else 0), k S + T - (O if k < n - 1 else 0)).
 * The cores partition the canvas; a tile's 2-D core is the product of its axis cores; tiles are numbered row-major.  Every
 * origin and core bound is a multiple of 16, so a tile's pooling grid is the page's.  kocr_tile_plan writes
 * out[6] = {ny, nx, Hc, Wc, S, nT = ny nx} for an H x W page; KOCR_EINVAL names a refused argument.
 *
 * A halo of O pixels does not reproduce a whole-page pass: pixels nearer than the detector's receptive field to a tile edge
 * see the tile's zero padding instead of the page (DESIGN.md states how much).
 *
 * kocr_gather_tiles / kocr_stitch_heat: the two copies alone (test seams; host or, with on_device, 16-byte aligned device
 * pointers).  canvas: N x Hc x Wc x 3 uint8, Hc x Wc a canvas of (tile, overlap) -- KOCR_EINVAL otherwise; tiles: N x nT x T x T
 * x 3 uint8; tile_heat: N x nT x T/2 x T/2 x 2 float32; heat: N x Hc/2 x Wc/2 x 2 float32.
 * kocr_craft_forward_tiled: gather -> kocr_craft_forward's forward over the N nT tiles, micro_batch TILES at a time -> stitch.
 * kocr_detect_tiled: kocr_detect with that in place of the forward; the canvases are uint8.
 * kocr_pipeline_tiled: kocr_pipeline's arguments with (tile, overlap) in place of (Hmax, Wmax): the batch is padded to the
 * canvas of the largest dhs x the largest dws, the detector runs tiled, and the REST OF THE CALL IS kocr_pipeline's own code.
 * So every context switch (scores, beam, lexicon match, orientation, character boxes, min-area-rect rule) acts on it, and every
 * getter of resident results (kocr_pipeline_results, kocr_detection_scores, kocr_recognition_scores / _beams / _lexicon /
 * _orientation, kocr_detection_char_boxes, kocr_pipeline_device_results) answers after it, exactly as after kocr_pipeline;
 * boxes are in canvas = detector-input pixels.
 * Limit of the last three: a canvas side of 8192 (the post-processing takes heat-map sides up to 4096, the first bound a
 * growing canvas meets); beyond it KOCR_EINVAL names the limit. */
int kocr_tile_plan(kocr_ctx* ctx, int H, int W, int tile, int overlap, int32_t* out);
int kocr_gather_tiles(kocr_ctx* ctx, const uint8_t* canvas, int N, int Hc, int Wc, int tile, int overlap, uint8_t* tiles,
                      int on_device);
int kocr_stitch_heat(kocr_ctx* ctx, const float* tile_heat, int N, int Hc, int Wc, int tile, int overlap, float* heat,
                     int on_device);
int kocr_craft_forward_tiled(kocr_ctx* ctx, const uint8_t* canvas, int N, int Hc, int Wc, int tile, int overlap, float* heat,
                             int micro_batch, int on_device);
int kocr_detect_tiled(kocr_ctx* ctx, const uint8_t* canvas, int N, int Hc, int Wc, int tile, int overlap,
                      float detection_threshold, float text_threshold, float link_threshold, int size_threshold,
                      int micro_batch, float* boxes, int32_t* counts, int cap, int on_device);
int kocr_pipeline_tiled(kocr_ctx* ctx, int N, const uint8_t* const* imgs, const int32_t* hs, const int32_t* ws,
                        const int32_t* dhs, const int32_t* dws, int tile, int overlap, float detection_threshold,
                        float text_threshold, float link_threshold, int size_threshold, int micro_batch, float* boxes,
                        int32_t* counts, int cap, int32_t* labels, int max_crops, int32_t* n_crops, int on_device);

/* ---- single fused-epilogue convolution (unit-test seam for the MFMA kernel) ---------- */
/* out = post_a * act(pre_a * conv(in, w) + pre_b) + post_b, NHWC, stride 1, 'same'
 * padding; w is HWIO (the Keras kernel layout, detection.py:461).  pre_a/pre_b/post_a/
 * post_b are per-Cout vectors or NULL (identity).  Host pointers only. */
int kocr_conv2d_nhwc(kocr_ctx* ctx, const float* in, int N, int H, int W, int Cin,
                     const float* w_hwio, int KH, int KW, int dilation, int Cout,
                     const float* pre_a, const float* pre_b, int relu,
                     const float* post_a, const float* post_b, float* out);

/* The same seam for a CELL GRID (round 5; the layout the recogniser's conv stack runs in, keras_ocr_amd/csrc/crnn.cpp): every
 * image is one row of W / cellW cells of cellW columns, each holding an independent crop in its columns [0, cellWv) and rows
 * [1, H); row 0 and the columns behind cellWv are zero gutters (the caller passes zeros there, the result has zeros there).
 * 3x3, dilation 1, Cin % 32 == 0, Cout > 64, H % 4 == 0, W % 64 == 0, fp16 arithmetic modes only.  pool != 0: the 2x2 max
 * pooling of cell rows (2 i, 2 i + 1) -- crop rows (2 i - 1, 2 i): the flipped 'valid' pooling of recognition.py:228, 238 -- is
 * fused and pool_out [N][H/2][W/2][Cout] (cells of cellW / 2) is written instead of out (out may be NULL).  amax_out (or NULL):
 * the per-cell max |x| the kernel tracked for what it wrote, N * (W / cellW) floats.  Host pointers only. */
int kocr_conv2d_cells(kocr_ctx* ctx, const float* in, int N, int H, int W, int Cin, const float* w_hwio, int Cout,
                      const float* pre_a, const float* pre_b, int relu, const float* post_a, const float* post_b,
                      int cellW, int cellWv, int pool, float* out, float* pool_out, float* amax_out);

/* ---- the decode launches on the caller's logits (unit-test seam for the CTC kernels) ---------- */
/* Everything kocr_crnn_forward[_scores], kocr_crnn_beam, kocr_crnn_lexicon and kocr_crnn_ctc_loss launch BEHIND fc_12, on
 * logits the caller made: the same launch functions with the same arguments, so a test decides what the kernels see
 * (saturated frames, exact ties) instead of whatever a network produces.  Bound to the loaded recogniser: C =
 * kocr_crnn_classes(), LW = kocr_crnn_label_width() (rows 50 - LW .. 49 of a crop's logits are decoded), the lexicon is the
 * context's.  logits: M x 50 x C float32, M <= 1024 (one recogniser batch; more is KOCR_EINVAL).  Always: labels [M][LW],
 * probs [M][LW][C] or NULL -- kocr_crnn_forward's.  Each further part is off when its switch is 0 / NULL:
 *   log_word [M] and char_scores [M][LW], both or neither: kocr_crnn_forward_scores' launch instead of the plain decode;
 *   beam_width != 0: beam_labels [M][top_paths][LW], beam_log_prob [M][top_paths] as kocr_crnn_beam (same refusals);
 *   top_words != 0: lex_index / lex_log_prob [M][top_words], lex_values [M][V] or NULL as kocr_crnn_lexicon (same refusals);
 *   loss_labels != NULL: loss [M] as kocr_crnn_ctc_loss for these labels and lengths (same refusals).
 * KOCR_ENOWEIGHTS without a recogniser.  Host pointers only.  Runs on the ctx stream and is complete on return.  Records no
 * taps and leaves the resident pipeline results alone. */
int kocr_crnn_decode_logits(kocr_ctx* ctx, const float* logits, int M, int32_t* labels, float* probs, float* log_word,
                            float* char_scores, int beam_width, int top_paths, int32_t* beam_labels, float* beam_log_prob,
                            int top_words, int32_t* lex_index, float* lex_log_prob, float* lex_values, const int32_t* loss_labels,
                            int label_stride, const int32_t* label_lengths, const int32_t* input_lengths, float* loss);
/* The same with character sets ("Character sets" below): set_of int32 [M] (HOST), each in [-1, kocr_charset_count()) else
 * KOCR_EINVAL naming the crop; NULL: the context's kocr_set_charset switch, which kocr_crnn_decode_logits follows too.  The
 * decode, the scores, the beam and the lexicon parts run under the sets; the loss part stays unmasked. */
int kocr_crnn_decode_logits_charsets(kocr_ctx* ctx, const float* logits, int M, int32_t* labels, float* probs, float* log_word,
                                     float* char_scores, int beam_width, int top_paths, int32_t* beam_labels, float* beam_log_prob,
                                     int top_words, int32_t* lex_index, float* lex_log_prob, float* lex_values,
                                     const int32_t* loss_labels, int label_stride, const int32_t* label_lengths,
                                     const int32_t* input_lengths, float* loss, const int32_t* set_of);

/* ---- arithmetic of the wide convolutions --------------------------------------------- */
/* The 3x3 / 1x1 / dilated convolutions with Cout > 32 run on the 16-bit matrix cores with fp32 operands split into
 * 16-bit pieces and fp32 accumulation:
 *   KOCR_SPLIT_BF16X3: 3 bf16 pieces, exact split, 6 products everywhere (dropped terms < 2^-21 |ab| worst case,
 *                      2^-25 |ab| rms; no operand bit is dropped);
 *   KOCR_SPLIT_F16X2:  the Winograd F(4,3) layers whose images tile as 4 x 64 or 8 x 32 pixels (the bulk of CRAFT) run on
 *                      the fp16 cores instead: 2 fp16 pieces per operand (round to nearest, <= 2^-22 |a| worst case, 2^-24
 *                      rms, while the low piece is a normal fp16), 3 products, operands scaled by exact powers of two --
 *                      per IMAGE from the max |x| its producer tracked, per output channel for the weights -- so a result
 *                      never depends on the rest of the batch.  Same measured error against fp64 as bf16x3; half the
 *                      matrix-core work of those layers.  Every other layer runs as in KOCR_SPLIT_BF16X3;
 *   KOCR_SPLIT_F16X1:  REDUCED PRECISION fast mode (opt-in, never a default): the same layers with ONE fp16 piece per
 *                      operand and one product (relative operand error 2^-12); tolerance stated in DESIGN.md section 3.
 * The environment variable KOCR_SPLIT=bf16|f16|f16x1 sets the initial mode of new contexts.  There is no reference
 * counterpart (the reference computes in TensorFlow fp32). */
#define KOCR_SPLIT_BF16X3 0
#define KOCR_SPLIT_F16X2 1
#define KOCR_SPLIT_F16X1 2
int kocr_set_split_mode(kocr_ctx* ctx, int mode);
int kocr_get_split_mode(const kocr_ctx* ctx);

/* CRAFT schedule (every arithmetic mode): two chains of convolutions without a non-linearity between them are evaluated in
 * their algebraically identical shorter form ("Folded linear layers"):
 * fold_linear_chain -- slice5.1 -> slice5.2 -> upconv1.conv.0 (detection.py:349-353, :106-108) as one composed
 * dilated 3x3 + a 1x1 over s4; fold_upsample -- conv1x1(concat(resize(y), skip)) (detection.py:106-115, 380-389)
 * as resize(conv1x1_y(y)) + conv1x1_skip(skip).  Both default to on (KOCR_LINFOLD=0 / KOCR_UPFOLD=0 in the
 * environment of kocr_create turn them off for new contexts); results differ by fp32 round-off only. */
int kocr_set_schedule(kocr_ctx* ctx, int fold_linear_chain, int fold_upsample);
/* The switches as they stand (1 = on): the environment's choice until kocr_set_schedule changes it. */
int kocr_get_schedule(kocr_ctx* ctx, int* fold_linear_chain, int* fold_upsample);

/* ---- minAreaRect rule of getBoxes ----------------------------------------------------------------------------------------
 * Which enclosing rectangle kocr_get_boxes, kocr_detect and kocr_pipeline give a word (detection.py:273,
 * cv2.boxPoints(cv2.minAreaRect(contour))); the diamond test, the roll and the x2 that follow are the same under both:
 *   KOCR_RECT_EXACT   (default): the min-area rectangle over the hull's edges compared in exact integer arithmetic, equal
 *                     areas going to the first edge; corners from exact integer numerators and one float64 division
 *                     (oracle/postproc.py::min_area_box).  Geometrically exact; differs from cv2 by float32 round-off, and
 *                     where cv2's float32 areas break a tie or a near-tie the other way, by the rectangle chosen;
 *   KOCR_RECT_OPENCV: OpenCV's own arithmetic: float32 rotating calipers over the hull in cv2.convexHull's order with
 *                     the last of equal areas kept, the corner solve in float32, the angle through float64 atan2 and
 *                     degrees, RotatedRect::points with float32 cos / sin (oracle/postproc.py::min_area_box_cv32).
 * A per-context setting; any other value is KOCR_EINVAL.  kocr_get_min_area_rect returns the rule in force. */
#define KOCR_RECT_EXACT 0
#define KOCR_RECT_OPENCV 1
int kocr_set_min_area_rect(kocr_ctx* ctx, int rule);
int kocr_get_min_area_rect(const kocr_ctx* ctx);

/* ---- scores: how sure the two networks were ("Scores") ----------------------------------------------
 * The reference returns none; they are the numbers it computes on the way and drops:
 *   detection score of a box   the maximum of the text map over the pixels of the box's connected component, the number
 *                              detection.py:240 compares with detection_threshold (float32, no arithmetic);
 *   word log-probability       -ctc_batch_cost (the rule of kocr_ctc_batch_cost: epsilon, renormalisation) of the crop's own
 *                              greedy decode over all kocr_crnn_label_width() frames of fc_12's softmax: the log of the summed
 *                              probability of every alignment that collapses to the returned text; bit for bit
 *                              -kocr_crnn_ctc_loss of the crop with its decoded labels.  An empty decode: the all-blank path;
 *   character scores           for the k-th decoded label the maximum, over the frames of the run of arg-maxes that emitted it,
 *                              of that label's probability -- each value bit for bit an entry of kocr_crnn_forward's probs;
 *                              0 in the -1 padded tail.
 * kocr_set_scores(ctx, 1) (default 0; kocr_get_scores returns the switch) makes kocr_get_boxes / kocr_detect leave the
 * detection scores, kocr_recognize_boxes the recogniser's two, kocr_pipeline all three resident in HBM next to their
 * results: the recogniser's decode then runs as ONE launch that also produces the scores (profiler row ctc_scores instead of
 * ctc_greedy; the decoded labels never visit the host); the label rows, boxes and counts are the same bits either way.  With
 * the switch off the calls launch what they always launched.
 * kocr_detection_scores: scores N x cap float32 (HOST; row i holds counts[i] values in box order, the rest undefined), cap >=
 * the cap the results were produced with -- after KOCR_ECAPACITY from kocr_pipeline that is the largest count, as for
 * kocr_pipeline_results.  kocr_recognition_scores: log_word [n_crops], char_scores [n_crops][label width] (HOST, image-major,
 * box order as the label rows); *n_crops / *label_width (either may be NULL) receive the number of crops and the label width
 * the rows were PRODUCED with, also when the call fails with KOCR_ECAPACITY (max_crops too small).  Both are valid until the
 * next libkocr call on the context that processes images, and fail with KOCR_EINVAL and a message when nothing is resident
 * (also after a failed call; kocr_get_boxes / kocr_detect returning KOCR_ECAPACITY leave nothing) or when the results were
 * produced with the switch off. */
int kocr_set_scores(kocr_ctx* ctx, int on);
int kocr_get_scores(const kocr_ctx* ctx);
int kocr_detection_scores(kocr_ctx* ctx, float* scores, int cap);
int kocr_recognition_scores(kocr_ctx* ctx, float* log_word, float* char_scores, int max_crops, int32_t* n_crops,
                            int32_t* label_width);
/* kocr_crnn_forward (arguments as there; probs may be NULL) that also returns log_word [M] and char_scores
 * [M][kocr_crnn_label_width()] (device pointers when on_device), whatever the switch says.  labels and probs are bit for bit
 * kocr_crnn_forward's. */
int kocr_crnn_forward_scores(kocr_ctx* ctx, const float* crops, int M, int32_t* labels, float* probs, float* log_word,
                             float* char_scores, int on_device);

/* ---- beam search: the other readings of a word ("Beam search") ---------------------------------------
 * keras.backend.ctc_decode(greedy=False, beam_width, top_paths), which the reference never exposes: CTC prefix beam search
 * without a language model on the frame probabilities of kocr_ctc_batch_cost (q_t: fc_12's softmax + epsilon, renormalised;
 * frames rnn_steps_to_discard .. 49).  Per frame a prefix is extended by the min(beam_width, classes - 1) non-blank classes
 * of the largest logit only; candidates spelling the same prefix are merged; the best beam_width by total probability
 * survive.  Order everywhere: the higher value first, then the lexicographically smaller label row, -1 sorting after every
 * label.  Of the final beam the top_paths best are RESCORED with the CTC forward algorithm: log_prob is, bit for bit,
 * -kocr_crnn_ctc_loss of the crop with that label row (the exact sum over all its alignments, not the beam's running sum),
 * and the rows come sorted by it.  labels: M x top_paths x kocr_crnn_label_width() int32, -1 padded as kocr_crnn_forward's;
 * log_prob: M x top_paths float32.  When fewer than top_paths prefixes survive, the remaining rows are all -1 with
 * log_prob = -inf.  1 <= beam_width <= 64, 1 <= top_paths <= beam_width, else KOCR_EINVAL naming the argument.
 * beam_width = 1 is NOT the greedy decode (one prefix per frame is not one arg-max per frame).  A crop's result does not
 * depend on M or on its place in the batch.  on_device as for kocr_crnn_forward. */
int kocr_crnn_beam(kocr_ctx* ctx, const float* crops, int M, int beam_width, int top_paths, int32_t* labels, float* log_prob,
                   int on_device);
/* kocr_set_beam(ctx, beam_width, top_paths) (beam_width = 0, the default: off) makes kocr_recognize_boxes / kocr_pipeline run
 * the beam search on every crop AFTER their unchanged greedy decode (one more launch per batch, profiler row ctc_beam) and
 * leave the alternatives resident in HBM; the label rows, boxes, counts and scores they return are the same bits either way.
 * kocr_recognition_beams copies them out: labels [n_crops][top_paths][label width], log_prob [n_crops][top_paths] (HOST,
 * image-major, box order as the label rows); *n_crops / *label_width / *top_paths (each may be NULL) receive what the rows
 * were PRODUCED with, also when the call fails with KOCR_ECAPACITY (max_crops too small).  Validity and errors as for
 * kocr_recognition_scores. */
int kocr_set_beam(kocr_ctx* ctx, int beam_width, int top_paths);
int kocr_get_beam(const kocr_ctx* ctx, int* beam_width, int* top_paths);
int kocr_recognition_beams(kocr_ctx* ctx, int32_t* labels, float* log_prob, int max_crops, int32_t* n_crops,
                           int32_t* label_width, int32_t* top_paths);

/* ---- lexicon: which of the caller's words is this crop ("Lexicon") -----------------------------------
 * value[m][v] = the exact CTC log-probability of word v given crop m: -kocr_crnn_ctc_loss of the crop with the word's labels
 * over all kocr_crnn_label_width() frames (q_t: fc_12's softmax + epsilon, renormalised, as kocr_ctc_batch_cost); -inf for
 * a word that has no alignment (it needs more frames than there are once every repeated label has its blank).
 * A lexicon is loaded once and stays resident on the context like weights.  kocr_set_lexicon: words = V label rows, int32
 * [V][stride], lengths int32 [V] (HOST); every label in [0, classes - 2] of the LOADED recogniser (KOCR_ENOWEIGHTS without
 * one), 1 <= length <= min(KOCR_LEXICON_MAX_WORD, stride), else KOCR_EINVAL naming the argument and the word.  Equal words
 * may repeat (the tie rule orders them).  V = 0 unloads.  A call replaces the previous lexicon; a refused one changes nothing.
 * Loading another recogniser with a DIFFERENT class count unloads the lexicon and switches the match off (the labels were
 * checked against the old alphabet); calls that need one then fail with KOCR_EINVAL saying so.  kocr_lexicon_size: V (0: none).
 *
 * kocr_crnn_lexicon: crops as kocr_crnn_forward.  Per crop the top_words best words: index M x top_words int32 (the word's
 * row in the CALLER's order), log_prob M x top_words float32.  Order: the higher value first, then the smaller index.  The
 * best are found on the values of the scoring kernel, then each is RESCORED with the loss's own forward recursion:
 * log_prob is, bit for bit, -kocr_crnn_ctc_loss of the crop with that word, and the rows come sorted by it (same tie rule).
 * Where fewer than top_words words have an alignment the remaining entries are index -1, log_prob -inf.  all_values
 * (nullable): M x V float32, the scoring kernel's own value of every pair (within the CTC loss's float32 error of the
 * definition above, -inf exactly where it is).  1 <= top_words <= 64 (more than V is allowed), else KOCR_EINVAL naming the
 * argument; no lexicon loaded: KOCR_EINVAL.  M = 0 is valid.  A crop's result does not depend on M, on its place in the
 * batch or on the scratch chunking.  on_device as for kocr_crnn_forward (all buffers then device pointers).
 *
 * kocr_set_lexicon_match(ctx, top_words) (0, the default: off; needs a loaded lexicon otherwise) makes kocr_recognize_boxes /
 * kocr_pipeline run the match on every crop AFTER their unchanged decode (three more launches per chunk of crops: profiler
 * rows lexicon_logq, lexicon_score, lexicon_select) and leave index / log_prob resident in HBM; label rows, boxes, counts,
 * scores and beam rows are the same bits either way.  kocr_recognition_lexicon copies them out: index / log_prob
 * [n_crops][top_words] (HOST, image-major, box order as the label rows); *n_crops / *top_words (each may be NULL) receive
 * what the rows were PRODUCED with, also when the call fails with KOCR_ECAPACITY (max_crops too small).  Validity and errors
 * as for kocr_recognition_beams.
 * kocr_set_lexicon_scratch: the M x V values of a batch live in workspace scratch of at most `bytes` (0: the default,
 * 256 MiB); a batch whose values exceed it is processed in chunks of max(1, bytes / (4 V)) crops.  Results do not depend on it. */
#define KOCR_LEXICON_MAX_WORD 32
int kocr_set_lexicon(kocr_ctx* ctx, const int32_t* words, int stride, const int32_t* lengths, int V);
int kocr_lexicon_size(const kocr_ctx* ctx);
int kocr_crnn_lexicon(kocr_ctx* ctx, const float* crops, int M, int top_words, int32_t* index, float* log_prob, float* all_values,
                      int on_device);
int kocr_set_lexicon_match(kocr_ctx* ctx, int top_words);
int kocr_get_lexicon_match(const kocr_ctx* ctx, int* top_words);
int kocr_recognition_lexicon(kocr_ctx* ctx, int32_t* index, float* log_prob, int max_crops, int32_t* n_crops, int32_t* top_words);
int kocr_set_lexicon_scratch(kocr_ctx* ctx, uint64_t bytes);

/* ---- character sets: which characters may this crop hold ("Character sets") ---------------------------
 * A character set A is a non-empty subset of the non-blank classes [0, classes - 2] of the loaded recogniser; the blank is
 * always allowed.  A crop decoded under A is decoded as if fc_12 had written -inf for every class outside A and the blank,
 * and everything behind that is the unchanged rule on the masked row: the arg-max (ties to the smaller class), the softmax
 * (masked classes exactly 0), q_t = (p + 1e-7) / sum over ALL classes, the word log-probability, the character scores, the
 * lexicon values (a word with a masked character keeps a finite, very small value: it is not removed) and the beam search,
 * whose prefixes are extended only by classes of A -- per frame the min(beam_width, |A|) of them with the largest logit.
 * The mask is applied where the decode kernels read the row: no launch is added, the logits, the taps (fc_12, ctc input),
 * kocr_ctc_batch_cost, kocr_crnn_ctc_loss and kocr_crnn_features are never masked.
 * kocr_set_charsets: allowed = S rows of classes - 1 bytes (HOST; non-zero: the class is in the set); classes must equal
 * kocr_crnn_classes() (KOCR_ENOWEIGHTS without a recogniser), 0 <= S <= KOCR_CHARSETS_MAX and every set non-empty, else
 * KOCR_EINVAL naming the argument and the set.  The table stays resident on the context like a lexicon.  S = 0 unloads and
 * switches off.  A call replaces the previous table (and switches off); a refused one changes nothing.  Loading another
 * recogniser with a DIFFERENT class count unloads the table and switches off.  kocr_charset_count: S (0: none).
 * kocr_set_charset(ctx, set): -1 (the default) is off -- the calls launch the kernels they always launched and return the
 * same bits; set in [0, S) makes every decode of kocr_crnn_forward[_scores], kocr_crnn_beam, kocr_crnn_lexicon,
 * kocr_recognize_boxes and kocr_pipeline[_tiled] run under that set, with every other switch (scores, beam, lexicon match,
 * orientation, character boxes) as before and every resident-result getter answering as before; anything else KOCR_EINVAL.
 * kocr_recognize_boxes_charsets: kocr_recognize_boxes with one set per box, set_of int32 [sum of counts] (HOST, image-major,
 * box order), each in [-1, S) (-1: unconstrained); anything else is KOCR_EINVAL naming the box, before any launch.  The
 * context's uniform switch is not consulted.  With orientation on, both candidates of box m are read under set_of[m]. */
#define KOCR_CHARSETS_MAX 256
int kocr_set_charsets(kocr_ctx* ctx, const uint8_t* allowed, int S, int classes);
int kocr_charset_count(const kocr_ctx* ctx);
int kocr_set_charset(kocr_ctx* ctx, int set);
int kocr_get_charset(const kocr_ctx* ctx, int* set);
int kocr_recognize_boxes_charsets(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                                  const int32_t* counts, int32_t* labels, int on_device, const int32_t* set_of);

/* ---- patterns: decode a crop under a regular expression ("Patterns") -----------------------------------
 * A pattern is a trimmed deterministic automaton over the non-blank classes [0, classes - 2] of the loaded recogniser: start
 * state 0, delta[s][c] the next state or -1, accept[s]; every state reachable from 0 and able to reach an accepting one.  A
 * crop decoded under it gets the best single CTC alignment of its crnn_label_width() frames whose collapsed text the
 * automaton accepts -- a Viterbi pass over (frame x state x last label) on the loss's float32 log q_t, exact, with a fixed
 * tie rule -- as labels [LW] (-1 padded), log_path (that alignment's log-probability) and log_prob, the CTC
 * log-probability of the text over ALL its alignments: bit for bit -kocr_crnn_ctc_loss of the row, as for the beam and the
 * lexicon.  When the greedy text satisfies the pattern it is the greedy text.  Where no accepted text fits the frames, and
 * for a crop without a pattern (-1), the row is all -1 and both values are -inf.  The decode itself is untouched: the
 * pattern launches run behind it on the same logits (never masked by a character set).
 * kocr_set_patterns: P automata, pattern p with n_states[p] states; delta = the patterns' rows one after another, each of
 * classes - 1 int32; accept = one byte per row (HOST).  classes must equal kocr_crnn_classes() (KOCR_ENOWEIGHTS without a
 * recogniser); 0 <= P <= KOCR_PATTERNS_MAX, 1 <= n_states <= KOCR_PATTERN_MAX_STATES, at most KOCR_PATTERN_MAX_NODES pairs
 * (state, class entering it) per pattern, every move in [-1, n_states), trimmed (so the language is not empty): else
 * KOCR_EINVAL naming the argument, the pattern and the count.  The tables stay resident on the context like a lexicon.  P = 0
 * unloads and switches off; a call replaces the previous tables (and switches off); a refused one changes nothing.  Loading
 * another recogniser with a DIFFERENT class count unloads them and switches off.  kocr_pattern_count: P (0: none).
 * kocr_set_pattern(ctx, index): -1 (the default) is off -- the calls launch what they always launched and return the same
 * bits; index in [0, P) makes the recogniser stage of kocr_recognize_boxes and kocr_pipeline[_tiled] also run the pattern
 * launches on every batch's logits and leave the rows resident beside the label rows for kocr_recognition_patterns (the
 * resident-result protocol of kocr_recognition_lexicon).  Scores, the beam and the lexicon match run as before beside it;
 * orientation and an active character set (kocr_set_charset) are KOCR_EINVAL.
 * kocr_crnn_pattern: the forward to the logits, then the pattern launches alone; pattern_of int32 [M] (HOST, each in
 * [-1, P), else KOCR_EINVAL naming the crop) or NULL for the context's switch; crops and results as kocr_crnn_lexicon's.
 * kocr_recognize_boxes_patterns: kocr_recognize_boxes with one pattern per box, pattern_of int32 [sum of counts] (HOST),
 * each in [-1, P) else KOCR_EINVAL naming the box, before any launch; the context's switch is not consulted.
 * kocr_crnn_decode_logits_patterns (development): the pattern launches on the caller's logits (HOST, M <= 1024), as
 * kocr_crnn_decode_logits.  The back-pointers of a large pattern leave LDS for workspace scratch, a crop's table lies there
 * too, and both are chunked under the byte budget of kocr_set_lexicon_scratch; no result depends on the chunking. */
#define KOCR_PATTERNS_MAX 64
#define KOCR_PATTERN_MAX_STATES 256
#define KOCR_PATTERN_MAX_NODES 4096
int kocr_set_patterns(kocr_ctx* ctx, const int32_t* delta, const uint8_t* accept, const int32_t* n_states, int P, int classes);
int kocr_pattern_count(const kocr_ctx* ctx);
int kocr_set_pattern(kocr_ctx* ctx, int index);
int kocr_get_pattern(const kocr_ctx* ctx, int* index);
int kocr_recognition_patterns(kocr_ctx* ctx, int32_t* labels, float* log_path, float* log_prob, int max_crops, int32_t* n_crops);
int kocr_crnn_pattern(kocr_ctx* ctx, const float* crops, int M, const int32_t* pattern_of, int32_t* labels, float* log_path,
                      float* log_prob, int on_device);
int kocr_recognize_boxes_patterns(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                                  const int32_t* counts, int32_t* labels, int on_device, const int32_t* pattern_of);
int kocr_crnn_decode_logits_patterns(kocr_ctx* ctx, const float* logits, int M, const int32_t* pattern_of, int32_t* labels,
                                     float* log_path, float* log_prob);

/* ---- orientation: read each box both ways and keep the better reading ("Orientation") ----------------
 * The reference's get_rotated_box always names the upper of the two leftmost corners tl, so an upside-down word is warped
 * upside down and a vertical one into a sliver.  With the switch on, every box is read in two orientations: its ordered box
 * ob = get_rotated_box(box) with (w, h) = get_rotated_width_height(ob) has the base turn b = 1 when mode is KOCR_ORIENT_ANY
 * and float(h) >= tall_ratio * float(w) (float64), else 0; candidate c = 0, 1 has t_c = b + 2 c quarter turns and the source
 * quad q_c[i] = ob[(i + t_c) % 4] -- the same four float32 corners renamed: turn 1 reads text running down the page, turn 3
 * up the page, turn 2 upside down.  Everything behind that is the crop stage's arithmetic on q_c in place of ob (width and
 * height come from q_c and swap for odd turns; a zero width or height stays KOCR_EZERODIV), the unchanged warp, and the
 * unchanged recogniser with its scores on the 2 M crops, a word's two crops side by side.  Candidate 1 wins iff
 * (n_1 > 0 and n_0 == 0) or ((n_1 > 0) == (n_0 > 0) and v_1 > v_0), n_c the number of decoded labels and v_c the word
 * log-probability ("Scores") of candidate c: an empty decode loses to a non-empty one, otherwise the larger exact
 * log-probability wins, a tie or a NaN keeps candidate 0.  Two candidates per box, never four.
 * kocr_set_orientation(ctx, mode, tall_ratio): mode KOCR_ORIENT_OFF (default), KOCR_ORIENT_FLIP (turns 0 / 2 for every box)
 * or KOCR_ORIENT_ANY; KOCR_EINVAL for another mode, for a tall_ratio that is not finite and positive, and while a beam, a
 * lexicon match or character boxes are switched on -- kocr_recognize_boxes / kocr_pipeline refuse those combinations as well.
 * With the switch on the two calls return the WINNERS' label rows, leave the winners' scores resident (with scores on) and
 * kocr_pipeline_results / kocr_pipeline_device_results carry the winners' rows, M of them as ever; two more launches per call
 * (profiler rows warp_prepare_turned in kocr_pipeline, orient_select in both) and ctc_scores in place of ctc_greedy.  The box
 * buffers keep getBoxes' boxes, bit for bit.  With the switch off the calls launch what they always launched.
 * kocr_recognition_orientation: turns [n_crops] int32, quads [n_crops][4][2] float32 -- the winner's q, [tl, tr, br, bl] of the
 * text AS READ, so quads[m][0] -> quads[m][1] is the reading direction --, log_words [n_crops][2] float32 = (v_0, v_1) (HOST,
 * image-major, box order as the label rows); *n_crops (may be NULL) receives the number of crops, also when the call fails
 * with KOCR_ECAPACITY (max_crops too small).  Validity and errors as for kocr_recognition_scores. */
#define KOCR_ORIENT_OFF 0
#define KOCR_ORIENT_FLIP 1
#define KOCR_ORIENT_ANY 2
int kocr_set_orientation(kocr_ctx* ctx, int mode, double tall_ratio);
int kocr_get_orientation(const kocr_ctx* ctx, int* mode, double* tall_ratio);
int kocr_recognition_orientation(kocr_ctx* ctx, int32_t* turns, float* quads, float* log_words, int max_crops, int32_t* n_crops);
/* The two stages alone (unit-test seams).  kocr_warp_crops_turned: kocr_warp_crops' arguments (HOST) plus mode (FLIP / ANY) and
 * tall_ratio; the set-up runs on the device as in kocr_pipeline.  crops [2 M][target_h][target_w], turns [2 M], quads
 * [2 M][4][2], crop 2 m + c = candidate c of box m.  kocr_orient_select: the choice on the caller's rows (HOST): labels
 * [M][2][L] int32, log_word [M][2], char_scores [M][2][L], turns [M][2], quads [M][2][4][2] -> out_labels [M][L], out_log_word
 * [M], out_char_scores [M][L], out_turns [M], out_quads [M][4][2], out_log_words [M][2]; L >= 1. */
int kocr_warp_crops_turned(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes, const int32_t* counts,
                           int mode, double tall_ratio, int target_h, int target_w, float* crops, int32_t* turns, float* quads);
int kocr_orient_select(kocr_ctx* ctx, int M, int L, const int32_t* labels, const float* log_word, const float* char_scores,
                       const int32_t* turns, const float* quads, int32_t* out_labels, float* out_log_word, float* out_char_scores,
                       int32_t* out_turns, float* out_quads, float* out_log_words);

/* ---- long words ---------------------------------------------------------------------- */
/* The opt-in calls that read a box wider than 200 : 31 in overlapping windows -- the whole route, its results and its
 * unit-test seams -- are declared in kocr_windows.h beside this file; they are part of this ABI and of libkocr.so.  The rule:
 *
 * Every other recognition route fits a box into ONE 31 x 200 crop with scale = min(200 / w, 31 / h), so a box wider than
 * 200 : 31 is shrunk in both directions and at 20 : 1 its text reaches the recogniser 10 pixels high.  Those calls cut such
 * a box into K windows along its long side, read every window as an ordinary crop, stitch the windows' fc_12 logit rows
 * into ONE frame sequence per word and decode that sequence.  Opt-in: no other call launches or returns anything else.
 *
 * Constants: the crop is 31 x 200, T = 50 frames of 4 pixels, d = the recogniser's rnn_steps_to_discard.
 * Parameters: aspect A (float64, finite, >= 200 / 31; 10.0 is a good default), overlap O (a multiple of 8 in [16, 96]; 40),
 * S = 200 - O, f = O / 8.  KOCR_EINVAL when they are out of range or when d >= 50 - f.
 *
 * Per box: ob = get_rotated_box(box) = [tl, tr, br, bl], (w, h) the integers of get_rotated_width_height(ob); a zero w or h
 * stays KOCR_EZERODIV.
 *   1. The box is LONG iff (double)w > A * (double)h.  Not long: K = 1 and q_0 = ob, the ordinary crop operation for operation.
 *   2. Long: K = ceil((31 w - 200 h) / (S h)) + 1 in exact 64-bit integers (the numerator is positive since A >= 200 / 31).
 *   3. Window k spans the fractions [a_k, b_k] of the top edge tl -> tr and of the bottom edge bl -> br:
 *      a_k = (double)(k S h) / (double)(31 w), b_k = min(1, (double)((k S + 200) h) / (double)(31 w)), products in int64.
 *   4. The point at fraction a of an edge p -> q is (float)((double)p + ((double)q - (double)p) * a) per component, in this
 *      order, never fused; a == 0 takes p's own float32 numbers and a == 1 takes q's.
 *   5. q_k = [top(a_k), top(b_k), bottom(b_k), bottom(a_k)]; everything behind it is the ordinary set-up of an ordered quad for
 *      a 31 x 200 crop and the unchanged warp.  The last window is shorter: its crop is narrower and zero-padded on the right.
 *   6. Frames kept of window k: [lo_k, hi_k) with lo_k = d for k = 0, else f; hi_k = 50 for k = K - 1, else 50 - f.  The seam
 *      is the middle of the overlap: frame 50 - f of window k and frame f of window k + 1 lie at the same nominal crop x.
 *   7. The word's sequence has T' = (K - 1) S / 4 + 50 - d frames (K = 1: frames d .. 49, the ordinary ones).
 *   8. A call is refused with KOCR_EINVAL before any launch when some T' exceeds KOCR_WINDOW_FRAMES_MAX, naming the image and
 *      the box.
 * A window's own quad goes through the ordinary set-up, so a window whose integer width or height comes out zero (only boxes a
 * pixel or two high have such windows) is KOCR_EZERODIV as well.
 * Window k of box m (image-major box order) is crop offset(m) + k, offset = the exclusive prefix sum of K.  The recogniser
 * runs on all sum K crops in its usual batches of at most 1024; a word's windows may straddle two batches.  One difference:
 * a last batch of fewer than 82 crops behind a full one takes crops from it (1040 crops run as 958 + 82).  Below 82 crops the
 * recogniser's per-frame 1x1 layers run on another GEMM kernel, whose sums round differently in the last bits; this way the
 * last windows of a call do not depend on how many windows came before them.
 *
 * Stitch and decode: row j of word m's sequence is the fc_12 logit row of (window k, frame t), k upwards and t from lo_k to
 * hi_k - 1 -- copied, never recomputed.  On that sequence: the greedy labels (first maximum on ties, repeats merged ACROSS
 * seams too, blank dropped), per emitted label the largest arg-max probability of its run, and log_word = minus the exact CTC
 * loss of the decode over all T' frames -- the rules and the device functions of "Scores" above.  One wave per word, every
 * reduction in a fixed order, nothing shared between words: on the same logits a K = 1 word comes out bit for bit as
 * kocr_recognize_boxes with scores gives it, and a word's bits do not depend on the other words of the call.  The logits are
 * the recogniser's, and the recogniser picks its GEMM kernels by the size of the batch (the 1x1 layers at 82 crops, stn_conv_2
 * at 12): the two statements hold for whole calls whenever both calls' batches lie on the same side of
 * those sizes -- always from 82 crops on --, as they do between any two calls of kocr_recognize_boxes itself.
 *
 * Not combinable: a beam, a lexicon match, a character set, a pattern, orientation and character boxes switched on on the
 * context are refused with KOCR_EINVAL naming both sides, by every one of those calls.  uint8 images only.
 *
 * Limits.  With the spatial transformer on, the frame <-> x correspondence the seam relies on is nominal, not exact.  The edges
 * of a trapezoid are cut by linear fractions, not perspective-correct ones.  What windowing does for the reading of real long
 * words has not been measured (it needs pretrained weights): these calls establish the statement, not an accuracy figure. */

/* ---- measurement -------------------------------------------------------------------- */
/* When enabled, every kernel launch on the ctx is bracketed by hipEvents on the ctx
 * stream; kocr_profile_report fills parallel arrays (up to cap rows) with per-kernel-name
 * launch count, total milliseconds and algorithmic FLOPs / bytes.  Returns the number of
 * rows available. */
int kocr_profile_enable(kocr_ctx* ctx, int on);
int kocr_profile_reset(kocr_ctx* ctx);
int kocr_profile_report(kocr_ctx* ctx, int cap, char* names /* cap x 64 */, int64_t* launches,
                        double* total_ms, double* flops, double* bytes);

/* ---- range statistics of the fp16x2 arithmetic (developer instrumentation; off = no cost) ------------- */
/* KOCR_SPLIT_F16X2 keeps fp32's 24 bits of an element only while its magnitude lies within 2^16 of its image's maximum
 * (DESIGN.md section 3).  With the statistics enabled, every fp16-arithmetic convolution first counts, over its INPUT tensor
 * and with the per-image scale 2^e it is about to use, the non-zero elements with |x| 2^e < 2^-4 (two-piece precision worse
 * than 2^-21 relative to the element) and < 2^-14 (the high piece is an fp16 subnormal: worse than 2^-11), and the share
 * of the tensor's sum |x| they carry -- one synchronising side launch per layer, so timing runs keep it off.
 * kocr_range_stats_report fills parallel arrays (up to cap rows, one per layer name, accumulated since the last enable):
 * values[i * 7 + k] = launches, elements, non-zero elements, elements below 2^-4, below 2^-14, sum |x|, sum |x| of the
 * elements below 2^-4.  Returns the number of rows. */
int kocr_range_stats_enable(kocr_ctx* ctx, int on);
int kocr_range_stats_report(kocr_ctx* ctx, int cap, char* names /* cap x 64 */, double* values /* cap x 7 */);

/* ---- workspace arenas (FOR TESTS ONLY: not for callers, and no part of the stable surface) ------------ */
/* Every entry point sizes the context's bump arenas from a plan -- the bytes it hands the reservation -- and then allocates
 * from them.  These calls let the suite see whether the plans hold ("Arena book-keeping").
 * For tests: kocr_debug_arena_count() arenas, kocr_debug_arena_name(i) the name of arena i (NULL outside the range). */
int kocr_debug_arena_count(void);
const char* kocr_debug_arena_name(int i);
/* For tests: arena i's capacity, the bytes its last reservation asked for, the largest offset an allocation reached (or, when
 * refused for want of room, would have reached) since then, and the largest peak - requested over the arena's life (0 when
 * every plan held).  Any pointer may be NULL.  KOCR_EINVAL outside the range. */
int kocr_debug_arena_stats(kocr_ctx* ctx, int i, uint64_t* cap, uint64_t* requested, uint64_t* peak, uint64_t* excess);
/* For tests: synchronises, frees every arena and zeroes its statistics, forgets every resident result and the latched guard
 * damage -- the context is as cold as a new one, but keeps its networks, lexicon, patterns, character sets and switches. */
int kocr_debug_release_arenas(kocr_ctx* ctx);
/* For tests: guard mode (off by default; off costs nothing and changes no launch).  On, every arena allocation is followed by
 * a guard -- from the first byte behind the buffer to the next 256-byte boundary plus 256 bytes -- filled with 0xA5 on the
 * context's stream when the buffer is allocated, and compared whenever the arena is emptied (so for every batch of a call) and
 * by kocr_debug_check_arena_guards.  A reservation takes 256 KiB more for the guards; they do not count in the statistics. */
int kocr_debug_set_arena_guards(kocr_ctx* ctx, int on);
/* For tests: compares the guards still recorded and returns the number of damaged guards since the last check or release
 * (negative: a KOCR_* code); *arena, *offset, *byte (nullable) name the first: its arena, the offset of the buffer it follows,
 * and the offset of its first damaged byte.  The count starts again at 0. */
int kocr_debug_check_arena_guards(kocr_ctx* ctx, int* arena, uint64_t* offset, uint64_t* byte);
/* For tests: poison mode (byte = -1: off, the default; off costs one test per allocation and changes no launch).  With byte in
 * [0, 255], every allocation from an arena -- and every tensor the detector's lifetime pool hands out inside the ws arena --
 * is filled with that byte over exactly its bytes, on the context's stream when it is allocated: behind the previous user of
 * those bytes, before its own first writer.  A kernel that reads what this call has not written then reads the byte instead of
 * whatever the memory last held, so a call whose results differ between byte 0x00 and byte 0xFF (NaN as a float, -1 as an
 * integer) depends on stale workspace.  Results that stay resident are not touched by their getters.  Works together with
 * guard mode.  KOCR_EINVAL for another byte.  ("Poison mode".) */
int kocr_debug_set_arena_poison(kocr_ctx* ctx, int byte);
/* For tests: the device memory the library holds ("What a context owns and when it lets go").
 * *persistent_count / *persistent_bytes: the context's persistent allocations -- weights with their derived copies, lexicon,
 * character sets, patterns, the lazily allocated buffers -- and their sizes as asked for; *arena_bytes: the sum of its arenas'
 * capacities.  *process_count / *process_bytes: every allocation the library has made and not yet freed in this process, all
 * contexts' and kocr_device_alloc's included (counted where the memory is taken and given back, never read from the device,
 * whose free memory moves with other processes' work).  ctx may be NULL: the context's three figures are then 0.  Any pointer
 * may be NULL. */
int kocr_debug_memory_stats(kocr_ctx* ctx, uint64_t* persistent_count, uint64_t* persistent_bytes, uint64_t* arena_bytes,
                            uint64_t* process_count, uint64_t* process_bytes);

#ifdef __cplusplus
}
#endif
#endif /* KOCR_H */
