// crnn.cpp — the CRNN recogniser graph (default build parameters, recognition.py:13-23).
//
// Follows recognition.build_model (recognition.py:187-333) layer for layer; names are the Keras
// layer names ("conv_1".."conv_7", "bn_3/5/7", "fc_9", "lstm_10[_back]", "lstm_11[_back]",
// "fc_12"; the unnamed STN localisation layers are "stn_conv_1/2", "stn_dense_1/2").
//   - every Conv2D / Dense runs on the MFMA implicit-GEMM kernel; conv bias + ReLU, and the
//     BatchNorm that FOLLOWS the ReLU at conv_3/5/7 (Keras default eps = 1e-3,
//     recognition.py:226-242), are the kernel's pre/post affine epilogue;
//   - conv_1..conv_7 and the two poolings run in the crop's NATURAL orientation [M,31,200,C]: the
//     reference first permutes to (200,31) and flips the 31-axis (recognition.py:215-216), i.e.
//     x'[w][j] = x[30-j][w]; a 3x3 convolution on x' with kernel K[a][b] equals one on x with
//     Knat[p][q] = K[q][2-p], and 'valid' 2x2 pooling of the flipped odd axis (31 -> 15 -> 7, last
//     row dropped) equals pooling rows (2i+1, 2i+2) of the natural tensor (first row dropped).
//     W = 200 / 100 / 50 is even, so the whole stack takes the Winograd F(2,3) kernel; one small
//     transpose+flip kernel after bn_7 restores the Keras layout for the STN and the recurrent part;
//   - Flatten / Reshape are free re-interpretations of the NHWC buffers;
//   - the forward and backward LSTM input projections of a layer are one GEMM (N = 2*4*128);
//     Add (recognition.py:305) is folded into the next projection by stacking its kernel over
//     the [forward | backward] channel halves; Concatenate (:319) is the same buffer.
#include "common.h"
#include "load_check.h"
#include "taps.h"
#include <algorithm>
#include <cmath>

int launch_crnn_input(kocr_ctx* ctx, const float* d_crops, float* d_x, int M, int Hc, int Wc);
int launch_crnn_to_keras(kocr_ctx* ctx, const Tensor& in, const Tensor& out);
int launch_crnn_conv1_cells(kocr_ctx* ctx, const ConvLayer& L, const float* d_crops, int M, int Hc, int Wc, const Tensor& out);
int launch_crnn_cells_to_keras(kocr_ctx* ctx, const Tensor& in, const Tensor& out);
int launch_stn_sample(kocr_ctx* ctx, const Tensor& x, const float* d_theta, const Tensor& out);
int launch_lstm(kocr_ctx* ctx, const float* d_xp, const float* d_Uf, const float* d_Ub, float* d_out, int M, int T);
size_t dense_splitk_workspace(int M, int K);
int launch_dense_splitk(kocr_ctx* ctx, const ConvLayer& L, const float* d_in, float* d_out, float* d_partial, int M);
int launch_ctc(kocr_ctx* ctx, const float* d_logits, int M, int T, int C, int discard, int* d_labels, float* d_probs,
               const CharMask& cm);
int launch_ctc_scores(kocr_ctx* ctx, const float* d_logits, int M, int T, int C, int discard, int* d_labels, float* d_probs,
                      float* d_logw, float* d_chars, const CharMask& cm);
int launch_ctc_beam(kocr_ctx* ctx, const float* d_logits, int M, int T, int C, int discard, int beam_width, int top_paths,
                    int* d_labels, float* d_logp, const CharMask& cm);

int launch_lexicon_logq(kocr_ctx* ctx, const float* d_logits, int M, int T, int C, int discard, float* d_lq, const CharMask& cm);
int launch_lexicon_score(kocr_ctx* ctx, const float* d_lq, int M, int To, int C, const int* d_words, int wstride, const int* d_lens,
                         const int* d_order, int V, int Lmax, float* d_values);
int launch_lexicon_select(kocr_ctx* ctx, const float* d_logits, int M, int T, int C, int discard, const float* d_values, int V,
                          const int* d_words, int wstride, const int* d_lens, int top_words, int* d_index, float* d_logp,
                          const CharMask& cm);

struct CrnnNet {
  std::map<std::string, ConvLayer> L;
  float* U[4] = {nullptr, nullptr, nullptr, nullptr};  // recurrent kernels 10, 10_back, 11, 11_back
  int n_classes = 0;
  bool loaded = false;
  bool stn = true;   // build_params["stn"] (recognition.py:243-281): false when the weight set carries no stn_* tensors
  int discard = 2;   // build_params["rnn_steps_to_discard"] (recognition.py:328)
};

namespace {
constexpr int HC = CRNN_CROP_H, WC = CRNN_CROP_W, UNITS = CRNN_FEAT / 2, T = CRNN_STEPS, DISCARD = 2;
// the crop batch as a cell grid (Tensor::cellW): CN crops side by side per image; cell = (HC + 1) x 208 at full resolution
// (one zero row on top, eight zero columns behind the crop), 16 x 104 and 8 x 52 after the two poolings.  208 CN, 104 CN and
// 52 CN are multiples of 64: the grid tiles as 4 rows x 64 columns at every level.
// CN = 16 cells per row; batches of at most 8 crops (Recognizer.recognize, a page with a few words) take 8 -- 208 * 8, 104 * 8 and
// 52 * 8 are multiples of 64 / 64 / 32 as well -- so that a single crop convolves 8 cells, not 16.  A crop's result
// does not depend on its cell or its neighbours (tests/test_cells_gpu.py), hence not on this choice.
constexpr int CN = 16, CELL_W = 208;
static inline int cells_per_row(int M) { return M <= 8 ? 8 : CN; }
const int kFilters[7] = {64, 128, 256, 256, 512, 512, 512};

struct Blob {
  const float* p;
  size_t numel;
};
}  // namespace

int crnn_classes(kocr_ctx* ctx) { return ctx->crnn && ctx->crnn->loaded ? ctx->crnn->n_classes : 0; }
int crnn_label_width(kocr_ctx* ctx) { return T - (ctx->crnn ? ctx->crnn->discard : DISCARD); }
// The smallest batch whose per-frame 1x1 layers (fc_9, the LSTM projections, fc_12: T pixels a crop) launch_conv sends to
// conv_ds; a smaller batch runs them on the fp32 MFMA kernel, whose sums round differently.  0: conv_ds is switched off on this
// context (KOCR_DSPLIT=0), every batch takes the same kernel.
int crnn_small_batch(const kocr_ctx* ctx) { return ctx->sw.dsplit ? (int)((DSPLIT_MIN_PIXELS + T - 1) / T) : 0; }
int crnn_set_discard(kocr_ctx* ctx, int d) {
  if (d < 0 || d >= T) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_crnn_set_rnn_steps_to_discard: 0 <= steps < 50 (recognition.py:328)");
  if (!ctx->crnn) ctx->crnn = new CrnnNet();
  ctx->crnn->discard = d;
  return KOCR_OK;
}

int crnn_load(kocr_ctx* ctx, int n, const char* const* names, const float* const* data, const int64_t* shapes,
              const int* ranks) {
  std::map<std::string, Blob> blobs;
  BlobSizes sizes;
  for (int i = 0; i < n; ++i) {
    size_t ne = 1;
    for (int d = 0; d < ranks[i]; ++d) ne *= (size_t)shapes[i * 4 + d];
    blobs[names[i]] = Blob{data[i], ne};
    sizes[names[i]] = ne;
  }
  // Validate first, change afterwards (include/kocr.h): a refused set leaves the context as it was -- weights, loaded, class
  // count, label width, tables and device memory.  Nothing below this check can fail for a reason the caller's set gives.
  int n_classes = 0;
  bool stn = false;
  const std::string bad = crnn_check_blobs(sizes, &n_classes, &stn);
  if (!bad.empty()) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_load_crnn: " + bad);
  auto need = [&](const std::string& k, size_t numel, const float** out) -> int {
    auto it = blobs.find(k);
    if (it == blobs.end()) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_load_crnn: missing tensor " + k);
    if (numel && it->second.numel != numel) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_load_crnn: tensor " + k + " has wrong size");
    *out = it->second.p;
    return KOCR_OK;
  };
  if (!ctx->crnn) ctx->crnn = new CrnnNet();
  CrnnNet* net = ctx->crnn;
  // The changing phase: from here to its end the network counts as not loaded, so that a failure on the way (an allocation or a
  // copy -- nothing else is left) leaves KOCR_ENOWEIGHTS behind and never a network of two weight sets.
  net->loaded = false;
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // no launch still reads what is released below
  for (float*& u : net->U) {
    ctx->release(u);
    u = nullptr;
  }
  if (!stn)  // a recogniser without the transformer replaces one with it: its four layers and their device copies go
    for (auto it = net->L.begin(); it != net->L.end();) {
      if (it->first.rfind("stn_", 0) == 0) {
        KOCR_TRY(release_layer(ctx, it->second));
        it = net->L.erase(it);
      } else {
        ++it;
      }
    }
  auto add = [&](const std::string& name, const float* w, int cin, int cout, int k, const float* bias, int relu,
                 const float* post_a, const float* post_b) -> int {
    ConvLayer& L = net->L[name];
    L.name = name;
    return prepare_conv(ctx, L, w, /*oihw=*/false, cin, cout, k, k, 1, nullptr, bias, relu, post_a, post_b);
  };
  int cin = 1;
  for (int i = 1; i <= 7; ++i) {
    const int cout = kFilters[i - 1];
    const std::string nm = "conv_" + std::to_string(i);
    const float *w, *b;
    KOCR_TRY(need(nm + "/kernel", (size_t)9 * cin * cout, &w));
    KOCR_TRY(need(nm + "/bias", cout, &b));
    // natural-orientation kernel: Knat[p][q][c][o] = K[q][2-p][c][o]  (HWIO)
    std::vector<float> wn((size_t)9 * cin * cout);
    for (int pp = 0; pp < 3; ++pp)
      for (int q = 0; q < 3; ++q)
        memcpy(&wn[((size_t)pp * 3 + q) * cin * cout], &w[((size_t)q * 3 + (2 - pp)) * cin * cout],
               sizeof(float) * cin * cout);
    w = wn.data();
    std::vector<float> qa, qb;
    if (i == 3 || i == 5 || i == 7) {
      const std::string bn = "bn_" + std::to_string(i);
      const float *g, *be, *mu, *var;
      KOCR_TRY(need(bn + "/gamma", cout, &g));
      KOCR_TRY(need(bn + "/beta", cout, &be));
      KOCR_TRY(need(bn + "/moving_mean", cout, &mu));
      KOCR_TRY(need(bn + "/moving_variance", cout, &var));
      qa.resize(cout);
      qb.resize(cout);
      for (int o = 0; o < cout; ++o) {
        qa[o] = g[o] / std::sqrt(var[o] + 1e-3f);
        qb[o] = be[o] - mu[o] * qa[o];
      }
    }
    KOCR_TRY(add(nm, w, cin, cout, 3, b, 1, qa.empty() ? nullptr : qa.data(), qb.empty() ? nullptr : qb.data()));
    cin = cout;
  }
  // build_params["stn"] = False (recognition.py:243): a weight set without the localisation network -> no transformer
  net->stn = stn;
  if (net->stn) {
    const float *w, *b;
    KOCR_TRY(need("stn_conv_1/kernel", (size_t)25 * 512 * 16, &w));
    KOCR_TRY(need("stn_conv_1/bias", 16, &b));
    KOCR_TRY(add("stn_conv_1", w, 512, 16, 5, b, 1, nullptr, nullptr));
    KOCR_TRY(need("stn_conv_2/kernel", (size_t)25 * 16 * 32, &w));
    KOCR_TRY(need("stn_conv_2/bias", 32, &b));
    KOCR_TRY(add("stn_conv_2", w, 16, 32, 5, b, 1, nullptr, nullptr));
    KOCR_TRY(need("stn_dense_1/kernel", (size_t)11200 * 64, &w));
    KOCR_TRY(need("stn_dense_1/bias", 64, &b));
    KOCR_TRY(add("stn_dense_1", w, 11200, 64, 1, b, 1, nullptr, nullptr));
    KOCR_TRY(need("stn_dense_2/kernel", (size_t)64 * 6, &w));
    KOCR_TRY(need("stn_dense_2/bias", 6, &b));
    KOCR_TRY(add("stn_dense_2", w, 64, 6, 1, b, 0, nullptr, nullptr));
  }
  {
    const float *w, *b;
    KOCR_TRY(need("fc_9/kernel", (size_t)3584 * UNITS, &w));
    KOCR_TRY(need("fc_9/bias", UNITS, &b));
    KOCR_TRY(add("fc_9", w, 3584, UNITS, 1, b, 1, nullptr, nullptr));
  }
  // LSTM layers: merged [fwd | back] input projection; layer 2 reads [f | b] = 256 channels and
  // its kernel is stacked twice so that (f + b) @ W == [f | b] @ [W; W]   (recognition.py:305)
  const char* lname[4] = {"lstm_10", "lstm_10_back", "lstm_11", "lstm_11_back"};
  for (int layer = 0; layer < 2; ++layer) {
    const float *wf, *wb, *bf, *bb;
    KOCR_TRY(need(std::string(lname[2 * layer]) + "/kernel", (size_t)UNITS * 4 * UNITS, &wf));
    KOCR_TRY(need(std::string(lname[2 * layer + 1]) + "/kernel", (size_t)UNITS * 4 * UNITS, &wb));
    KOCR_TRY(need(std::string(lname[2 * layer]) + "/bias", 4 * UNITS, &bf));
    KOCR_TRY(need(std::string(lname[2 * layer + 1]) + "/bias", 4 * UNITS, &bb));
    const int kin = layer == 0 ? UNITS : 2 * UNITS;
    std::vector<float> w((size_t)kin * 8 * UNITS), b(8 * UNITS);
    for (int k = 0; k < kin; ++k)
      for (int o = 0; o < 4 * UNITS; ++o) {
        w[(size_t)k * 8 * UNITS + o] = wf[(size_t)(k % UNITS) * 4 * UNITS + o];
        w[(size_t)k * 8 * UNITS + 4 * UNITS + o] = wb[(size_t)(k % UNITS) * 4 * UNITS + o];
      }
    for (int o = 0; o < 4 * UNITS; ++o) {
      b[o] = bf[o];
      b[4 * UNITS + o] = bb[o];
    }
    KOCR_TRY(add(layer == 0 ? "lstm_10_xproj" : "lstm_11_xproj", w.data(), kin, 8 * UNITS, 1, b.data(), 0, nullptr, nullptr));
    for (int d = 0; d < 2; ++d) {
      const float* u;
      KOCR_TRY(need(std::string(lname[2 * layer + d]) + "/recurrent_kernel", (size_t)UNITS * 4 * UNITS, &u));
      KOCR_TRY(ctx->upload(&net->U[2 * layer + d], std::vector<float>(u, u + (size_t)UNITS * 4 * UNITS)));
    }
  }
  {
    net->n_classes = n_classes;
    const float *w, *b;
    KOCR_TRY(need("fc_12/kernel", (size_t)2 * UNITS * net->n_classes, &w));
    KOCR_TRY(need("fc_12/bias", net->n_classes, &b));
    KOCR_TRY(add("fc_12", w, 2 * UNITS, net->n_classes, 1, b, 0, nullptr, nullptr));
  }
  net->loaded = true;
  return KOCR_OK;
}

void crnn_free(kocr_ctx* ctx) {
  delete ctx->crnn;
  ctx->crnn = nullptr;
}

size_t crnn_workspace_bytes(int M, int n_classes) {
  const size_t m = (size_t)M, f = sizeof(float);
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  size_t t = 0;
  {  // the cell-grid schedule instead of the dense conv stack below (whichever is larger): whole rows of CN cells
    const size_t mc = (m + CN - 1) / CN * CN;
    const size_t cells = al(mc * (HC + 1) * CELL_W * 64 * f) + al(mc * (HC + 1) * CELL_W * 128 * f) +
                         al(mc * 16 * (CELL_W / 2) * 256 * f) * 2 + al(mc * 8 * (CELL_W / 4) * 512 * f) * 3;
    const size_t dense = al(m * WC * HC * 64 * f) + al(m * WC * HC * 128 * f) + al(m * WC * HC * 256 * f) +
                         al(m * 100 * 15 * 256 * f) * 2 + al(m * 100 * 15 * 512 * f) + al(m * 52 * 7 * 512 * f) * 3;
    if (cells > dense) t += cells - dense;
  }
  t += al(m * WC * HC * 64 * f) + al(m * WC * HC * 128 * f) + al(m * WC * HC * 256 * f);
  t += al(m * 100 * 15 * 256 * f) * 2 + al(m * 100 * 15 * 512 * f);
  t += al(m * 52 * 7 * 512 * f) * 5;                              // p5, c6, c7 (both layouts; width padded to 52), stn
  t += al(m * 50 * 7 * 16 * f) + al(m * 50 * 7 * 32 * f) + al(m * 64 * f) + al(m * 6 * f);
  t += al(dense_splitk_workspace(M, 50 * 7 * 32));
  t += al(m * T * UNITS * f) + al(m * T * 8 * UNITS * f) + al(m * T * 2 * UNITS * f) * 2;
  t += al(m * T * (size_t)n_classes * f);
  return t + 8192;
}

// The chunking rule of the lexicon launches (common.h): a chunk's crops share one table / value scratch; a crop's result does
// not depend on the chunk it falls into (nothing is shared between crops).
int lexicon_chunk(const kocr_ctx* ctx, int M) {
  const size_t per_crop = (size_t)std::max(ctx->lex.V, 1) * sizeof(float);
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(M, 1), ctx->lex_scratch / per_crop));
}

size_t lexicon_workspace_bytes(kocr_ctx* ctx, int M, bool own_values) {
  const size_t chunk = (size_t)lexicon_chunk(ctx, M);
  return chunk * T * (size_t)std::max(crnn_classes(ctx), 1) * sizeof(float) + (own_values ? chunk * ctx->lex.V * sizeof(float) : 0) + 1024;
}

// lexicon_logq, lexicon_score, lexicon_select on the logits [M][T][C] of a batch, chunk by chunk; cm: the batch's character
// sets, advanced to each chunk's first crop
static int lexicon_run(kocr_ctx* ctx, const float* d_lg, int M, const CrnnLexicon& lx, const CharMask& cm) {
  const auto& lex = ctx->lex;
  const int C = ctx->crnn->n_classes, discard = ctx->crnn->discard, To = T - discard, V = lex.V;
  if (V <= 0 || lex.classes != C) KOCR_FAIL(ctx, KOCR_EINVAL, "lexicon: no lexicon loaded for this recogniser's class count");
  const int chunk = lexicon_chunk(ctx, M);
  float* d_lq = (float*)ctx->ws_alloc((size_t)chunk * To * C * sizeof(float));
  float* d_vals = lx.d_all ? nullptr : (float*)ctx->ws_alloc((size_t)chunk * V * sizeof(float));
  if (!d_lq || (!lx.d_all && !d_vals)) KOCR_FAIL(ctx, KOCR_ENOMEM, "lexicon: workspace exhausted");
  for (int c0 = 0; c0 < M; c0 += chunk) {
    const int nc = std::min(chunk, M - c0);
    const float* lg = d_lg + (size_t)c0 * T * C;
    float* vals = lx.d_all ? lx.d_all + (size_t)c0 * V : d_vals;
    const CharMask cc = cm.from(c0);
    KOCR_TRY(launch_lexicon_logq(ctx, lg, nc, T, C, discard, d_lq, cc));
    KOCR_TRY(launch_lexicon_score(ctx, d_lq, nc, To, C, lex.d_words, lex.Lmax, lex.d_lens, lex.d_order, V, lex.Lmax, vals));
    KOCR_TRY(launch_lexicon_select(ctx, lg, nc, T, C, discard, vals, V, lex.d_words, lex.Lmax, lex.d_lens, lx.top_words,
                                   lx.d_index + (size_t)c0 * lx.top_words, lx.d_logp + (size_t)c0 * lx.top_words, cc));
  }
  return KOCR_OK;
}

// The largest node and state counts among the patterns that crops [pt.first, pt.first + M) run under (0: none of them has one)
static void pattern_extent(const kocr_ctx* ctx, int M, const CrnnPattern& pt, int* NTmax, int* Smax) {
  const auto& pats = ctx->patterns;
  *NTmax = *Smax = 0;
  auto take = [&](int p) {
    if (p < 0 || p >= pats.P) return;
    *NTmax = std::max(*NTmax, pats.NT[p]);
    *Smax = std::max(*Smax, pats.S[p]);
  };
  if (!pt.of) take(pt.uniform);
  else
    for (int m = 0; m < M; ++m) take(pt.of[pt.first + m]);
}

static size_t pattern_crop_bytes(kocr_ctx* ctx, int M, const CrnnPattern& pt) {
  int NTmax, Smax;
  pattern_extent(ctx, M, pt, &NTmax, &Smax);
  const int C = std::max(crnn_classes(ctx), 2), To = std::max(crnn_label_width(ctx), 1);
  // as pattern_run launches: a batch of -1 rows runs with one node and one state, and its table may take the LDS that their
  // back-pointers would have had
  const size_t bp = (pattern_bp_bytes(To, C, std::max(NTmax, 1), std::max(Smax, 1)) + 255) & ~(size_t)255;
  return (size_t)To * C * sizeof(float) + bp;
}

int pattern_chunk(kocr_ctx* ctx, int M, const CrnnPattern& pt) {
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(M, 1), ctx->lex_scratch / pattern_crop_bytes(ctx, M, pt)));
}

// A batch's chunk times what its crops take is at most max(one crop, min(the budget, the batch)) of the whole call's extent.
size_t pattern_workspace_bytes(kocr_ctx* ctx, int M, const CrnnPattern& pt) {
  const size_t cb = pattern_crop_bytes(ctx, M, pt), mb = (size_t)std::min(std::max(M, 1), 1024);
  return std::max(cb, std::min(ctx->lex_scratch, mb * cb)) + 1024;
}

// lexicon_logq (unmasked), pattern_viterbi, pattern_rescore on the logits [M][T][C] of a batch, chunk by chunk.  The chunk and
// the launch's extent follow the patterns of the whole batch: a crop's rows do not depend on either.
static int pattern_run(kocr_ctx* ctx, const float* d_lg, int M, const CrnnPattern& pt) {
  if (M <= 0) return KOCR_OK;
  const auto& pats = ctx->patterns;
  const int C = ctx->crnn->n_classes, discard = ctx->crnn->discard, To = T - discard;
  if (pats.P <= 0 || pats.classes != C) KOCR_FAIL(ctx, KOCR_EINVAL, "patterns: no patterns loaded for this recogniser's class count");
  int NTmax, Smax;
  pattern_extent(ctx, M, pt, &NTmax, &Smax);
  NTmax = std::max(NTmax, 1);  // a batch of -1 rows
  Smax = std::max(Smax, 1);
  const int chunk = pattern_chunk(ctx, M, pt);
  const size_t bpb = (pattern_bp_bytes(To, C, NTmax, Smax) + 255) & ~(size_t)255;
  float* d_lq = (float*)ctx->ws_alloc((size_t)chunk * To * C * sizeof(float));
  void* d_bp = bpb ? ctx->ws_alloc((size_t)chunk * bpb) : nullptr;
  if (!d_lq || (bpb && !d_bp)) KOCR_FAIL(ctx, KOCR_ENOMEM, "patterns: workspace exhausted");
  for (int c0 = 0; c0 < M; c0 += chunk) {
    const int nc = std::min(chunk, M - c0);
    const float* lg = d_lg + (size_t)c0 * T * C;
    KOCR_TRY(launch_lexicon_logq(ctx, lg, nc, T, C, discard, d_lq, CharMask{}));
    KOCR_TRY(launch_pattern(ctx, lg, d_lq, nc, T, C, discard, pats.tables(), pt.d_of, pt.uniform, pt.first + c0, NTmax, Smax, d_bp,
                            pt.d_labels + (size_t)c0 * To, pt.d_logpath + c0, pt.d_logp + c0));
  }
  return KOCR_OK;
}

// The launches behind fc_12 on the logits [M][T][C] of a batch, for crnn_forward (`lg`: the logits as the "ctc" tap's input) and
// crnn_decode_logits (no taps): the greedy decode (with the scores when asked for), then the beam search, the lexicon match
// and the pattern decode, each where `rq` asks for it
static int decode_run(kocr_ctx* ctx, const float* d_lg, int M, const CrnnDecode& rq, const Tensor* lg = nullptr) {
  const CrnnNet* net = ctx->crnn;
  const int C = net->n_classes, discard = net->discard;
  if (rq.greedy) {
    auto greedy = [&]() {
      if (rq.sc.on) return launch_ctc_scores(ctx, d_lg, M, T, C, discard, rq.d_labels, rq.d_probs, rq.sc.d_logw, rq.sc.d_chars, rq.cm);
      return launch_ctc(ctx, d_lg, M, T, C, discard, rq.d_labels, rq.d_probs, rq.cm);
    };
    if (lg) {
      Tensor probs;  // tap view [M][1][LW][C] (not recorded without d_probs)
      probs.N = M;
      probs.H = 1;
      probs.W = T - discard;
      probs.C = probs.cs = C;
      probs.p = rq.d_probs;
      KOCR_TRY(tapped(ctx, "ctc", lg, &probs, nullptr, greedy));
    } else {
      KOCR_TRY(greedy());
    }
  }
  if (rq.bm.beam_width)
    KOCR_TRY(launch_ctc_beam(ctx, d_lg, M, T, C, discard, rq.bm.beam_width, rq.bm.top_paths, rq.bm.d_labels, rq.bm.d_logp, rq.cm));
  if (rq.lx.top_words) KOCR_TRY(lexicon_run(ctx, d_lg, M, rq.lx, rq.cm));
  if (rq.pt.on) KOCR_TRY(pattern_run(ctx, d_lg, M, rq.pt));
  return KOCR_OK;
}

// The one body of crnn_features / crnn_logits / crnn_forward (common.h): exactly one of d_feats, d_logits and rq is given.
// d_crops: device [M][31][200]
static int crnn_run(kocr_ctx* ctx, const float* d_crops, int M, float* d_feats, const float** d_logits, const CrnnDecode* rq) {
  CrnnNet* net = ctx->crnn;
  if (!net || !net->loaded) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_crnn_forward: call kocr_load_crnn first");
  if (M <= 0) return KOCR_OK;
  KOCR_TRY(ctx->amax_begin());
  // Arithmetic: conv_2 ... conv_5 take the flattened-pixel F(4,3) kernel in the context's mode -- fp16x2 with one input scale
  // per CROP (the "images" of this batch), so a crop's result does not depend on its neighbours in the batch; the
  // reduced-precision KOCR_SPLIT_F16X1 is a detector-only mode: the recogniser then runs fp16x2 (its decoded strings hang on
  // top-1 margins).  conv_6 / conv_7 (width 50) stay on the exact bf16x3 F(2,3) kernel.
  struct ModeGuard {
    kocr_ctx* c;
    int old;
    explicit ModeGuard(kocr_ctx* ctx) : c(ctx), old(ctx->split_mode) {
      if (c->split_mode == KOCR_SPLIT_F16X1) c->split_mode = KOCR_SPLIT_F16X2;
    }
    ~ModeGuard() { c->split_mode = old; }
  } mode_guard(ctx);
  auto mk = [&](int n, int h, int w, int c, Tensor* t) -> int {
    t->amax = nullptr;
    t->N = n;
    t->H = h;
    t->W = w;
    t->C = c;
    t->cs = c;
    t->co = 0;
    t->p = (float*)ctx->ws_alloc((size_t)n * h * w * c * sizeof(float));
    if (!t->p) KOCR_FAIL(ctx, KOCR_ENOMEM, "kocr_crnn_forward: workspace exhausted");
    return KOCR_OK;
  };
  auto view = [](const Tensor& t, int n, int h, int w, int c) {
    Tensor v = t;
    v.N = n;
    v.H = h;
    v.W = w;
    v.C = c;
    v.cs = c;
    v.co = 0;
    return v;
  };
  // every launch with its taps (kocr_crnn_set_taps, taps.h); with taps off the launch alone
  auto conv = [&](const char* name, const Tensor& in, const Tensor& out) -> int {
    return tapped(ctx, name, &in, &out, nullptr, [&]() { return launch_conv(ctx, net->L[name], in, nullptr, nullptr, out); });
  };
  auto pool = [&](const char* name, const Tensor& in, const Tensor& out) -> int {
    return tapped(ctx, name, &in, &out, nullptr, [&]() { return launch_maxpool2x2(ctx, in, out, /*row_off=*/1); });
  };
  Tensor crops;  // the crop batch as a tap view [M][31][200][1]
  crops.N = M;
  crops.H = HC;
  crops.W = WC;
  crops.C = crops.cs = 1;
  crops.p = const_cast<float*>(d_crops);
  Tensor x0, c1, c2, c3, p3, c4, c5, p5, c6, c7n, c7, s1, s2, d1, th, st, f9, xp, r1, r2, lg;
  // Round 5: in the fp16 arithmetic the conv stack runs on a CELL GRID (Tensor::cellW): the crops side by side, CN per image,
  // with zero gutters, so that conv_2 ... conv_7 take the vertical-reuse F(4,3) kernel (conv_w43vh_kernel MODE 2) with both
  // poolings fused into conv_3 / conv_5 (whose full-resolution outputs are never written) and the max-|x| slots maintained
  // per cell by every producer.  One path for every M (a crop's result must not depend on the batch it comes in).
  bool cells = true;
  for (int i = 2; i <= 7; ++i) cells = cells && w43_cells_ok(ctx, net->L["conv_" + std::to_string(i)]);
  if (cells) {
    const int cn = cells_per_row(M);
    const int R = (M + cn - 1) / cn;
    auto mkc = [&](int hc, int wc, int wv, int c, bool alloc, Tensor* t) -> int {
      t->N = R;
      t->H = hc;
      t->W = cn * wc;
      t->C = t->cs = c;
      t->co = 0;
      t->cellW = wc;
      t->cellWv = wv;
      t->amax = ctx->amax_slots(R * cn);
      if (!t->amax) KOCR_FAIL(ctx, KOCR_ECAPACITY, "kocr_crnn_forward: out of max-|x| slots");
      t->p = alloc ? (float*)ctx->ws_alloc((size_t)R * hc * cn * wc * c * sizeof(float)) : nullptr;
      if (alloc && !t->p) KOCR_FAIL(ctx, KOCR_ENOMEM, "kocr_crnn_forward: workspace exhausted");
      return KOCR_OK;
    };
    KOCR_TRY(mkc(HC + 1, CELL_W, WC, 64, true, &c1));
    KOCR_TRY(tapped(ctx, "conv_1", &crops, &c1, nullptr,
                    [&]() { return launch_crnn_conv1_cells(ctx, net->L["conv_1"], d_crops, M, HC, WC, c1); }));
    KOCR_TRY(mkc(HC + 1, CELL_W, WC, 128, true, &c2));
    KOCR_TRY(conv("conv_2", c1, c2));
    KOCR_TRY(mkc(HC + 1, CELL_W, WC, 256, false, &c3));  // conv_3's full-resolution output is only ever pooled
    KOCR_TRY(mkc(16, CELL_W / 2, WC / 2, 256, true, &p3));
    KOCR_TRY(tapped(ctx, "conv_3", &c2, nullptr, &p3, [&]() {  // ReLU, bn_3, pool
      return launch_conv_pool(ctx, net->L["conv_3"], c2, nullptr, nullptr, c3, &p3, /*need_full=*/false);
    }));
    KOCR_TRY(mkc(16, CELL_W / 2, WC / 2, 256, true, &c4));
    KOCR_TRY(conv("conv_4", p3, c4));
    KOCR_TRY(mkc(16, CELL_W / 2, WC / 2, 512, false, &c5));
    KOCR_TRY(mkc(8, CELL_W / 4, WC / 4, 512, true, &p5));
    KOCR_TRY(tapped(ctx, "conv_5", &c4, nullptr, &p5, [&]() {
      return launch_conv_pool(ctx, net->L["conv_5"], c4, nullptr, nullptr, c5, &p5, /*need_full=*/false);
    }));
    KOCR_TRY(mkc(8, CELL_W / 4, WC / 4, 512, true, &c6));
    KOCR_TRY(conv("conv_6", p5, c6));
    KOCR_TRY(mkc(8, CELL_W / 4, WC / 4, 512, true, &c7n));
    c7n.amax = nullptr;  // nothing downstream reads its scale
    KOCR_TRY(conv("conv_7", c6, c7n));
    KOCR_TRY(mk(M, WC / 4, HC / 4, 512, &c7));
    KOCR_TRY(tapped(ctx, "cells_to_keras", &c7n, &c7, nullptr, [&]() { return launch_crnn_cells_to_keras(ctx, c7n, c7); }));
  } else {
  // conv stack in the crop's natural orientation (see the header): [M,31,200,C]
  x0.N = M;
  x0.H = HC;
  x0.W = WC;
  x0.C = x0.cs = 1;
  x0.co = 0;
  x0.p = const_cast<float*>(d_crops);
  KOCR_TRY(mk(M, HC, WC, 64, &c1));
  c1.amax = ctx->amax_slots(M);  // per-crop max |x| for the fp16 consumer (conv_2); nullptr in bf16x3 mode
  KOCR_TRY(conv("conv_1", x0, c1));
  KOCR_TRY(mk(M, HC, WC, 128, &c2));
  c2.amax = ctx->amax_slots(M);
  KOCR_TRY(conv("conv_2", c1, c2));
  KOCR_TRY(mk(M, HC, WC, 256, &c3));
  c3.amax = ctx->amax_slots(M);
  KOCR_TRY(conv("conv_3", c2, c3));  // ReLU then bn_3
  KOCR_TRY(mk(M, HC / 2, WC / 2, 256, &p3));
  p3.amax = ctx->amax_slots(M);
  KOCR_TRY(pool("pool_3", c3, p3));
  KOCR_TRY(mk(M, HC / 2, WC / 2, 256, &c4));
  c4.amax = ctx->amax_slots(M);
  KOCR_TRY(conv("conv_4", p3, c4));
  KOCR_TRY(mk(M, HC / 2, WC / 2, 512, &c5));
  // conv_6 / conv_7 work on 7 x 50 maps: 50 is not a multiple of 4, so the F(4,3) kernels do not take them as they are.
  // In the fp16 modes the three tensors around them are stored 52 wide with two zero columns (Tensor::Wv = 50): the pooling
  // kernel and the flattened fp16 F(4,3) kernel write the zeros, which are exactly the 'same' padding of column 49's right
  // neighbours -- 4 % more pixels on a kernel 1.4x faster than the F(2,3) bf16x3 one that takes the 50-wide tensors.
  // (the same predicate the dispatcher uses: a 52-wide tensor through any other kernel would get convolution values written
  //  into its padding columns -- launch_conv now refuses that)
  const bool pad52 = w43_flat_h_ok(ctx, net->L["conv_6"]) && w43_flat_h_ok(ctx, net->L["conv_7"]);
  const int W6 = pad52 ? 52 : WC / 4;
  if (pad52) c5.amax = ctx->amax_slots(M);
  KOCR_TRY(conv("conv_5", c4, c5));
  KOCR_TRY(mk(M, HC / 4, W6, 512, &p5));
  p5.Wv = WC / 4;
  if (pad52) p5.amax = ctx->amax_slots(M);
  KOCR_TRY(pool("pool_5", c5, p5));
  KOCR_TRY(mk(M, HC / 4, W6, 512, &c6));
  c6.Wv = WC / 4;
  if (pad52) c6.amax = ctx->amax_slots(M);
  KOCR_TRY(conv("conv_6", p5, c6));
  KOCR_TRY(mk(M, HC / 4, W6, 512, &c7n));
  c7n.Wv = WC / 4;
  KOCR_TRY(conv("conv_7", c6, c7n));
  // back to the Keras layout (M, 50, 7, 512) for the STN and everything after it
  KOCR_TRY(mk(M, WC / 4, HC / 4, 512, &c7));
  KOCR_TRY(tapped(ctx, "crnn_to_keras", &c7n, &c7, nullptr, [&]() { return launch_crnn_to_keras(ctx, c7n, c7); }));
  }
  // STN (recognition.py:268-281)
  if (!net->stn) {
    st = c7;
  } else {
  KOCR_TRY(mk(M, WC / 4, HC / 4, 16, &s1));
  KOCR_TRY(conv("stn_conv_1", c7, s1));
  KOCR_TRY(mk(M, WC / 4, HC / 4, 32, &s2));
  KOCR_TRY(conv("stn_conv_2", s1, s2));
  KOCR_TRY(mk(M, 1, 1, 64, &d1));
  {
    // Dense(64) over 11 200 features: split-K (crnn_kernels.hip); the weight rows must be in plain k order
    const ConvLayer& Ld = net->L["stn_dense_1"];
    const bool sk = ctx->sw.dense_splitk && Ld.Cout == 64 && Ld.Cin == 11200;
    float* part = sk ? (float*)ctx->ws_alloc(dense_splitk_workspace(M, 11200)) : nullptr;
    if (sk && !part) KOCR_FAIL(ctx, KOCR_ENOMEM, "kocr_crnn_forward: workspace exhausted");
    const Tensor flat = view(s2, M, 1, 1, 11200);
    if (sk)
      KOCR_TRY(tapped(ctx, "stn_dense_1", &flat, &d1, nullptr, [&]() { return launch_dense_splitk(ctx, Ld, s2.p, d1.p, part, M); }));
    else
      KOCR_TRY(conv("stn_dense_1", view(s2, M, 1, 1, 11200), d1));
  }
  KOCR_TRY(mk(M, 1, 1, 6, &th));
  KOCR_TRY(conv("stn_dense_2", d1, th));
  KOCR_TRY(mk(M, WC / 4, HC / 4, 512, &st));
  KOCR_TRY(tapped(ctx, "stn_sample.theta", &th, nullptr, nullptr, []() { return KOCR_OK; }));  // theta as the sampler reads it
  KOCR_TRY(tapped(ctx, "stn_sample", &c7, &st, nullptr, [&]() { return launch_stn_sample(ctx, c7, th.p, st); }));
  }
  // Reshape + fc_9 (recognition.py:282-290)
  KOCR_TRY(mk(M, T, 1, UNITS, &f9));
  KOCR_TRY(conv("fc_9", view(st, M, T, 1, 7 * 512), f9));
  // BiLSTM x2 (recognition.py:292-319)
  KOCR_TRY(mk(M, T, 1, 8 * UNITS, &xp));
  KOCR_TRY(mk(M, T, 1, 2 * UNITS, &r1));
  KOCR_TRY(mk(M, T, 1, 2 * UNITS, &r2));
  if (d_feats) r2.p = d_feats;  // the backbone's output (recognition.py:319-320) goes straight to the caller
  KOCR_TRY(conv("lstm_10_xproj", f9, xp));
  KOCR_TRY(tapped(ctx, "lstm_10", &xp, &r1, nullptr, [&]() { return launch_lstm(ctx, xp.p, net->U[0], net->U[1], r1.p, M, T); }));
  KOCR_TRY(conv("lstm_11_xproj", r1, xp));
  KOCR_TRY(tapped(ctx, "lstm_11", &xp, &r2, nullptr, [&]() { return launch_lstm(ctx, xp.p, net->U[2], net->U[3], r2.p, M, T); }));
  if (d_feats) return KOCR_OK;
  // fc_12 + softmax + decode (recognition.py:321-328, 169-184)
  KOCR_TRY(mk(M, T, 1, net->n_classes, &lg));
  KOCR_TRY(conv("fc_12", r2, lg));
  if (d_logits) {
    *d_logits = lg.p;
    return KOCR_OK;
  }
  return decode_run(ctx, lg.p, M, *rq, &lg);
}

int crnn_features(kocr_ctx* ctx, const float* d_crops, int M, float* d_feats) {
  return crnn_run(ctx, d_crops, M, d_feats, nullptr, nullptr);
}
int crnn_logits(kocr_ctx* ctx, const float* d_crops, int M, const float** d_logits) {
  return crnn_run(ctx, d_crops, M, nullptr, d_logits, nullptr);
}
int crnn_forward(kocr_ctx* ctx, const float* d_crops, int M, const CrnnDecode& rq) {
  return crnn_run(ctx, d_crops, M, nullptr, nullptr, &rq);
}

int crnn_decode_logits(kocr_ctx* ctx, const float* d_lg, int M, const CrnnDecode& rq) {
  if (!ctx->crnn || !ctx->crnn->loaded) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_crnn_decode_logits: call kocr_load_crnn first");
  if (M <= 0) return KOCR_OK;
  return decode_run(ctx, d_lg, M, rq);
}

void patterns_unload(kocr_ctx* ctx) {
  hipStreamSynchronize(ctx->stream);  // no launch still reads the tables
  ctx->release(ctx->patterns.d_hdr);
  ctx->release(ctx->patterns.d_nodes);
  ctx->release(ctx->patterns.d_states);
  ctx->release(ctx->patterns.d_pred);
  ctx->patterns = kocr_ctx::Patterns{};
  ctx->pattern = -1;
}

int patterns_validate(kocr_ctx* ctx, const char* fn, const int32_t* pattern_of, long M, const char* what) {
  const int P = ctx->patterns.P;
  for (long m = 0; m < M; ++m)
    if (pattern_of[m] < -1 || pattern_of[m] >= P)
      KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": pattern_of: " + what + " " + std::to_string(m) + " has pattern " +
                                      std::to_string(pattern_of[m]) + " outside [-1, " + std::to_string(P) + ") (" + std::to_string(P) +
                                      " patterns are loaded: kocr_set_patterns)");
  return KOCR_OK;
}

int pattern_refusal(kocr_ctx* ctx, const char* fn) {
  if (ctx->charset >= 0)
    KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": a pattern cannot be combined with an active character set (kocr_set_charset): the "
                                                  "pattern states the characters itself");
  if (ctx->orient_mode != KOCR_ORIENT_OFF)
    KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": orientation cannot be combined with a pattern (kocr_set_pattern)");
  return KOCR_OK;
}

int lexicon_validate(kocr_ctx* ctx, const char* fn, int top_words) {
  if (top_words < 1 || top_words > 64)
    KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": top_words " + std::to_string(top_words) + " outside [1, 64]");
  if (ctx->lex.V == 0 && ctx->lex.dropped_classes)
    KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": the lexicon was loaded for a recogniser of " +
                                    std::to_string(ctx->lex.dropped_classes) + " classes and was unloaded when one of " +
                                    std::to_string(crnn_classes(ctx)) + " classes was loaded (class count mismatch): call "
                                    "kocr_set_lexicon again");
  if (ctx->lex.V == 0) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": no lexicon is loaded (kocr_set_lexicon first)");
  return KOCR_OK;
}

void charsets_unload(kocr_ctx* ctx) {
  hipStreamSynchronize(ctx->stream);  // no launch still reads the table
  ctx->release(ctx->charsets.d_bits);
  ctx->charsets = kocr_ctx::Charsets{};
  ctx->charset = -1;
}

int charsets_validate(kocr_ctx* ctx, const char* fn, const int32_t* set_of, long M, const char* what) {
  const int S = ctx->charsets.S;
  for (long m = 0; m < M; ++m)
    if (set_of[m] < -1 || set_of[m] >= S)
      KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": set_of: " + what + " " + std::to_string(m) + " has set " +
                                      std::to_string(set_of[m]) + " outside [-1, " + std::to_string(S) + ") (" + std::to_string(S) +
                                      " sets are loaded: kocr_set_charsets)");
  return KOCR_OK;
}

void lexicon_unload(kocr_ctx* ctx, int dropped_classes) {
  hipStreamSynchronize(ctx->stream);  // no launch still reads the words
  ctx->release(ctx->lex.d_words);
  ctx->release(ctx->lex.d_lens);
  ctx->release(ctx->lex.d_order);
  ctx->lex = kocr_ctx::Lexicon{};
  ctx->lex.dropped_classes = dropped_classes;
  ctx->lex_top = 0;
}

int beam_validate(kocr_ctx* ctx, const char* fn, int beam_width, int top_paths) {
  if (beam_width < 1 || beam_width > 64)
    KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": beam_width " + std::to_string(beam_width) + " outside [1, 64]");
  if (top_paths < 1 || top_paths > beam_width)
    KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": top_paths " + std::to_string(top_paths) + " outside [1, beam_width = " +
                                    std::to_string(beam_width) + "]");
  return KOCR_OK;
}

int crnn_ctc_loss(kocr_ctx* ctx, const float* d_crops, int M, const CtcLabels& lab, float* d_loss) {
  const float* d_lg = nullptr;
  KOCR_TRY(crnn_logits(ctx, d_crops, M, &d_lg));
  return crnn_logits_loss(ctx, d_lg, M, lab, d_loss);
}

int crnn_logits_loss(kocr_ctx* ctx, const float* d_lg, int M, const CtcLabels& lab, float* d_loss) {
  if (!ctx->crnn || !ctx->crnn->loaded) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "ctc loss: call kocr_load_crnn first");
  if (M <= 0) return KOCR_OK;
  return launch_ctc_loss(ctx, /*logits=*/true, d_lg, M, T, ctx->crnn->n_classes, ctx->crnn->discard, lab.d_lab, lab.lstride, lab.d_len,
                         lab.d_in_len, d_loss, lab.Lmax);
}

int ctc_validate(kocr_ctx* ctx, const char* fn, int M, int T, int C, const int32_t* labels, int label_stride,
                 const int32_t* label_lengths, const int32_t* input_lengths, int* Lmax) {
  const std::string f = fn;
  *Lmax = 0;
  for (int m = 0; m < M; ++m) {
    const std::string sm = "sample " + std::to_string(m);
    const int Tm = input_lengths[m], L = label_lengths[m];
    if (Tm < 1 || Tm > T)
      KOCR_FAIL(ctx, KOCR_EINVAL, f + ": " + sm + ": input_length " + std::to_string(Tm) + " outside [1, " + std::to_string(T) + "]");
    if (L < 0 || L > Tm)
      KOCR_FAIL(ctx, KOCR_EINVAL, f + ": " + sm + ": label_length " + std::to_string(L) + " outside [0, input_length = " +
                                      std::to_string(Tm) + "] (not enough time for the target transition sequence)");
    if (L > label_stride)
      KOCR_FAIL(ctx, KOCR_EINVAL, f + ": " + sm + ": label_length " + std::to_string(L) + " exceeds the label row width " +
                                      std::to_string(label_stride));
    for (int i = 0; i < L; ++i) {
      const int c = labels[(size_t)m * label_stride + i];
      if (c < 0 || c > C - 2)
        KOCR_FAIL(ctx, KOCR_EINVAL, f + ": " + sm + ": label " + std::to_string(c) + " at position " + std::to_string(i) +
                                        " outside [0, " + std::to_string(C - 2) + "] (the blank is " + std::to_string(C - 1) + ")");
    }
    *Lmax = std::max(*Lmax, L);
  }
  return KOCR_OK;
}
