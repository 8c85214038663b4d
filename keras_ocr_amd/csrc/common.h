// common.h — internal (non-ABI) declarations shared by the libkocr translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <map>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include "../../include/kocr.h"
#include "../../include/kocr_windows.h"

// ---------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------
#define KOCR_HIP(ctx, expr)                                                         \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess) {                                                         \
      (ctx)->set_err(std::string(#expr) + ": " + hipGetErrorString(_e) + " at " +   \
                     __FILE__ + ":" + std::to_string(__LINE__));                    \
      return KOCR_EHIP;                                                             \
    }                                                                               \
  } while (0)

#define KOCR_TRY(expr)            \
  do {                            \
    int _rc = (expr);             \
    if (_rc != KOCR_OK) return _rc; \
  } while (0)

#define KOCR_FAIL(ctx, code, msg) \
  do {                            \
    (ctx)->set_err(msg);          \
    return (code);                \
  } while (0)

// ---------------------------------------------------------------------------------------
// device tensors (NHWC fp32, optionally a channel slice of a wider buffer)
// ---------------------------------------------------------------------------------------
struct Tensor {
  float* p = nullptr;  // base of the (wider) buffer
  int N = 0, H = 0, W = 0, C = 0;
  int cs = 0;  // channel stride of the underlying buffer (floats per pixel)
  int co = 0;  // channel offset of this view inside the buffer
  // Optional device slots, ONE PER IMAGE (amax[n], n < N), each holding (as uint bits of a non-negative float) an UPPER
  // BOUND of max |x| over everything written into image n of the underlying buffer during this forward; every producer
  // kernel atomicMax-es into them.  The fp16 F(4,3) convolutions (conv_w43h.hip) derive the exact power-of-two input scale
  // of an image from its slot -- per image, so that a result never depends on the rest of the batch; a tensor without
  // slots is reduced on demand (launch_absmax).  Slices / views share the buffer's slots.
  unsigned* amax = nullptr;
  // Valid width (0 = W): columns [Wv, W) of every row are ZERO padding that belongs to the tensor -- its producer writes
  // zeros there, a convolution reading it sees exactly the 'same' padding it would see at the image edge.  Lets a tensor
  // whose width is not a multiple of 4 (the recogniser's 50-wide conv_6 / conv_7) run on the F(4,3) kernels at width 52.
  int Wv = 0;
  int wv() const { return Wv ? Wv : W; }
  // Cell grid (0 = none; round 5, the recogniser's crop batch): every image is ONE ROW of W / cellW cells of cellW columns,
  // each holding an independent crop in its columns [0, cellWv) and rows [1, H); row 0 and the columns [cellWv, cellW) of a
  // cell are ZERO gutters that belong to the tensor (its producer writes them) -- the 'same' padding between neighbouring
  // crops.  amax then holds one slot per CELL (image * cells() + cell).  Only conv_w43vh_kernel<.., MODE 2> takes and
  // writes such tensors; launch_conv fails loudly for anything else.
  int cellW = 0, cellWv = 0;
  int cells() const { return cellW ? W / cellW : 0; }
  size_t pixels() const { return (size_t)N * H * W; }
  Tensor slice(int off, int c) const {
    Tensor t = *this;
    t.co = co + off;
    t.C = c;
    return t;
  }
};

// ---------------------------------------------------------------------------------------
// a prepared convolution / dense layer
// ---------------------------------------------------------------------------------------
struct ConvLayer {
  std::string name;
  int Cin = 0, Cout = 0, KH = 1, KW = 1, dil = 1;
  int Kreal = 0, Kpad = 0, Cout_pad = 0, BN = 0;
  float* d_w = nullptr;       // [Kpad][Cout_pad], k = (ky*KW + kx)*Cin + c
  float* d_pre_a = nullptr;   // [Cout_pad]  v = acc*pre_a + pre_b
  float* d_pre_b = nullptr;
  float* d_post_a = nullptr;  // [Cout_pad] or nullptr: out = relu?(v)*post_a + post_b
  float* d_post_b = nullptr;
  int relu = 0;
  float* d_w_rgb4 = nullptr;  // first layer on raw uint8: [9 taps][R,G,B,0][Cout_pad] (48 rows)
  unsigned short* d_ws = nullptr;  // Winograd F(2,3) weights, 3-way bf16 split, conv_wsplit.hip order (Cout > 32)
  int ws_cout_pad = 0;
  unsigned short* d_w4 = nullptr;  // Winograd F(4,3) weights, 3-way bf16 split, conv_w43.hip order (Cout > 64, Cin % 32 == 0)
  int w4_cout_pad = 0;
  // the same weights for the fp16 kernels (conv_w43h.hip): U * 2^wexp[o] split into two fp16 pieces (round to nearest), the
  // per-cout exponent chosen so that max |U 2^wexp| over the cout's weights lies in [2^14, 2^15); d_pre_a_h[o] =
  // pre_a[o] * 2^-wexp[o] undoes it in the epilogue
  unsigned short* d_w4h = nullptr;
  float* d_pre_a_h = nullptr;
  unsigned short* d_ds = nullptr;  // direct-conv weights, 3-way bf16 split, conv_dsplit.hip order
  int ds_cout_pad = 0;
  unsigned short* d_first = nullptr;  // 3 -> <= 64 first layer on raw uint8, im2col K = 27 -> 32, conv_hsplit.hip order
  float first_bound = 0.f;            // ... an upper bound of |output| over every uint8 image (prepare_conv)
  unsigned short* d_hs = nullptr;  // 3x3, <= 32 couts: 3-way bf16 split, conv_hsplit.hip order
  unsigned short* d_hs16 = nullptr;  // the same for <= 16 couts: tap pairs on the 16x16x32 MFMA (conv_hs16_kernel)
  unsigned short* d_hsh = nullptr;   // conv_hsh_kernel: the <= 32-cout weights scaled per cout and split into two fp16 pieces
  std::vector<int> hs_wexp;          // ... their exponents (d_pre_a_h = pre_a 2^-wexp is uploaded by prepare_conv)
  unsigned short* d_k5 = nullptr;  // 5x5, 16 couts, small images: 3-way bf16 split, conv_k5.hip order
  bool tap_inner = false;  // K order [16-channel group][tap][16] (Cin % 16 == 0) instead of [tap][Cin]
  bool ready() const { return d_w != nullptr; }
};

// ---------------------------------------------------------------------------------------
// profiler: per kernel name, HIP-event bracketed launches on the ctx stream
// ---------------------------------------------------------------------------------------
struct ProfRow {
  int64_t launches = 0;
  double ms = 0, flops = 0, bytes = 0;
};

// range statistics of the fp16x2 arithmetic per convolution layer (elementwise.hip: launch_range_stats)
struct RangeRow {
  double launches = 0, elements = 0, nonzero = 0, below_m4 = 0, below_m14 = 0, sum_abs = 0, sum_abs_below_m4 = 0;
};

// A bump arena.  requested / peak / excess state how well the entry point's plan (the bytes it gave arena_reserve) covers what
// it then took: peak is the largest offset an allocation reached (or, refused for want of room, would have reached) since the
// last arena_reserve, excess the largest peak - requested over the arena's life -- the part of a plan's shortfall that the
// slack of arena_reserve hides (kocr_debug_arena_stats).  Guard mode (kocr_debug_set_arena_guards; gctx
// set): every allocation is followed by ARENA_GUARD_BYTES more, and the bytes from its end to the end of those are filled with
// ARENA_GUARD_FILL on the stream at allocation time and compared by reset() and kocr_debug_check_arena_guards.  off stays the
// offset the allocations would have reached without guards (gextra: what the guards have added), so the stats are the same.
// Poison mode (kocr_debug_set_arena_poison; pctx set): every allocation is filled with `pbyte` over exactly its bytes on the
// stream at allocation time -- behind the previous user of those bytes, like a guard's fill -- so that a kernel which reads
// what this call has not written reads the same loud value wherever the bytes came from ("Poison mode").
constexpr size_t ARENA_GUARD_BYTES = 256, ARENA_GUARD_RESERVE = (size_t)256 << 10;
constexpr unsigned char ARENA_GUARD_FILL = 0xA5;
struct ArenaGuard {
  size_t buf, at, len;  // the buffer's offset in the arena; the guard's first byte behind it and its length
};
struct kocr_ctx;
struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0;
  size_t requested = 0, peak = 0, excess = 0;
  kocr_ctx* gctx = nullptr;  // guard mode: the context whose stream fills and whose record latches the damage
  size_t gextra = 0;
  std::vector<ArenaGuard> guards;  // of the allocations since the last check
  kocr_ctx* pctx = nullptr;  // poison mode: the context whose stream fills
  unsigned char pbyte = 0;
  inline void reset();
  void note(size_t end) {  // an allocation that reaches (or would reach) `end`
    if (end > peak) peak = end;
    if (peak > requested && peak - requested > excess) excess = peak - requested;
  }
};
// the first byte of a copied-back guard that is not ARENA_GUARD_FILL, or -1
inline long arena_guard_damage(const unsigned char* copy, size_t len) {
  for (size_t i = 0; i < len; ++i)
    if (copy[i] != ARENA_GUARD_FILL) return (long)i;
  return -1;
}

struct CraftNet;
struct CrnnNet;
struct Taps;

// What a resident-result record of kocr_ctx holds: nothing (never produced, or an arena has been sized since), only the fact
// that the results were produced with the record's switch off, or rows that a getter may copy.
enum class Resident { NONE, OFF, VALID };
inline Resident resident(bool on) { return on ? Resident::VALID : Resident::OFF; }

// the rule of chars.hip (tests/chars_statement.py: check_rule)
struct CharsRule {
  double peak_threshold, valley_ratio, extent_threshold;
};

// Character sets (kocr_set_charsets; DESIGN.md section 4, "Character sets"): what the decode kernels of crnn_kernels.hip take
// by value.  bits: the device table [S][ceil(C / 32)], bit c of set s = class c is allowed (the blank's bit is always set,
// the bits from C on are clear).  Crop m of a launch decodes under set set_of[(first + m) >> shift] (device, one entry per
// crop; shift = 1: per box of an oriented run's candidate pairs), or under `uniform` when set_of is null; set -1 allows
// every class.  first: the place of the launch's crop 0 in the whole call's crops (the batch and chunk loops advance it).
// Off (no table, or neither a per-crop list nor a uniform set): the launchers take the unmasked instantiations.
struct CharMask {
  const uint32_t* bits = nullptr;
  const int32_t* set_of = nullptr;
  int uniform = -1;
  int shift = 0;
  int first = 0;
  bool on() const { return bits && (set_of || uniform >= 0); }
  CharMask from(int crop) const {
    CharMask c = *this;
    c.first += crop;
    return c;
  }
};

// Patterns (kocr_set_patterns; DESIGN.md section 4, "Patterns"): the device tables pattern_viterbi_kernel takes by value, all
// patterns in one buffer each.  hdr: [P][8] = {states S, nodes NT, first node, first state, first pred, 0, 0, 0}; nodes:
// per node (label | state << 16, first pred), label 0xffff for a blank node, one entry behind a pattern's last; states: per
// state (its blank node, accept), one entry behind the last; pred: the predecessor states of the label nodes.
struct PatternTables {
  const int* hdr = nullptr;
  const int2* nodes = nullptr;
  const int2* states = nullptr;
  const int* pred = nullptr;
};

struct kocr_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  void set_err(const std::string& s) { err = s; }

  int split_mode = KOCR_SPLIT_F16X2;  // KOCR_SPLIT_BF16X3 / KOCR_SPLIT_F16X2 (default since round 4) / KOCR_SPLIT_F16X1
  // CRAFT schedule options (craft.cpp: folded linear layers); read ONCE from KOCR_LINFOLD / KOCR_UPFOLD when the
  // context is created, changed through kocr_set_schedule
  bool opt_linfold = true, opt_upfold = true;
  // min-area rectangle rule of getBoxes (postproc.hip K13), changed through kocr_set_min_area_rect
  int min_area_rect = KOCR_RECT_EXACT;
  // kernel selection switches, read ONCE per context in kocr_create from the environment variable of the same name in
  // upper case with the KOCR_ prefix (KOCR_LSTM16=0 ...): the fallback kernels can be exercised per context, inside
  // one process
  struct Switches {
    bool dense_splitk = true;  // stn_dense_1 on the split-K kernel
    bool lstm16 = true;        // round-3 LSTM kernel (16 crops per workgroup, U resident in registers)
    bool hs16 = true;          // <= 16-cout 3x3 layers on the 16x16x32 MFMA
    bool k5 = true;            // 5x5 / 16-cout kernel (stn_conv_1)
    bool up2x = true;          // shared-tap epilogue for exact 2x up-sampling in the decoder 1x1s
    bool w43h = true;          // fp16 F(4,3) kernels in the fp16 arithmetic modes
    bool w43 = true;           // F(4,3) kernels altogether (wide 3x3 layers then on conv_ws / conv_ds)
    bool w43r = true;          // row-reuse arrangement of the 64-cout layers (then conv_w43n)
    bool w43v = true;          // vertical-reuse arrangement of the wider layers (then conv_w43_kernel)
    bool w43rag = true;        // ragged tile grids (images that do not tile exactly: flattened / F(2,3) / fp32 kernels)
    bool w43dilh = true;       // fp16 F(4,3) comb tiles of dilated layers (then bf16x3)
    bool cells = true;         // cell grids of the recogniser's crop batch (then round 4's dense crop batch)
    bool wsplit = true;        // conv_ws_kernel, Winograd F(2,3) on bf16x3
    bool dsplit = true;        // conv_ds_kernel, direct convolution on bf16x3
    bool hsplit = true;        // <= 32-cout 3x3 split kernels (then the fp32 MFMA kernel)
    bool first = true;         // split first-layer kernel on raw uint8 (then the fp32 MFMA kernel)
  } sw;
  bool prof_layers = false;  // KOCR_PROF_LAYERS (developer): one profiler row per layer (prof_name)
  int n_cu = 0;              // compute units of the device (the grid of the persistent kernels)

  // max-|x| slots of the tensors of the current forward (see Tensor::amax): zeroed by amax_begin()
  unsigned* d_amax = nullptr;
  int amax_used = 0;
  static constexpr int AMAX_SLOTS = 1 << 16;
  int amax_begin();            // (re)start slot allocation, zero the slots on the ctx stream
  unsigned* amax_slots(int n); // the next n slots (one per image; nullptr when exhausted or when the arithmetic in use never
                               // reads them: the consumer then reduces on demand)

  // workspace arenas (bump allocated per call, grown on demand): ws = network activations,
  // pp = post-processing per-pixel scratch, pp2 = post-processing canvases, io = staging,
  // pl = buffers that live for a whole kocr_pipeline call (padded batch, heat-maps, boxes)
  Arena ws, pp, pp2, io, pl;
  Arena bx;  // kocr_pipeline: the box buffer of a page with more boxes than the caller's cap (the pl arena holds the heat-maps)
  // every arena by index, with its name (kocr_debug_arena_*; chw / chr are declared with the character boxes below)
  static constexpr int N_ARENAS = 8;
  inline Arena* arena_at(int i);
  static const char* arena_name(int i) {
    static const char* const names[N_ARENAS] = {"ws", "pp", "pp2", "io", "pl", "bx", "chw", "chr"};
    return i >= 0 && i < N_ARENAS ? names[i] : nullptr;
  }
  // guard mode (tests): the damaged guards since the last kocr_debug_check_arena_guards, and the first of them
  struct GuardDamage {
    int count = 0, arena = -1;
    size_t offset = 0, byte = 0;  // the buffer the guard follows; the first damaged byte (both offsets in the arena)
  } guard_damage;
  int ws_reserve(size_t bytes);
  void ws_reset() { ws.reset(); }
  void* ws_alloc(size_t bytes);

  // persistent allocations (weights, tables, the lazy buffers of DESIGN.md section 2), each with its size
  // (kocr_debug_memory_stats)
  struct Owned {
    void* p;
    size_t bytes;
  };
  std::vector<Owned> owned;
  inline int dev_alloc(void** out, size_t bytes);
  int upload(float** out, const std::vector<float>& host);
  inline void release(void* p);            // frees one persistent allocation (a re-prepared layer's previous weights); nullptr is ignored
  inline void release_since(size_t mark);  // frees every allocation behind the first `mark` (TempLayer, abi.h)
  float* d_div255 = nullptr;  // [256] float32 v / 255 of kocr_compute_maps, uploaded by its first call on the context

  CraftNet* craft = nullptr;
  CrnnNet* crnn = nullptr;
  // kocr_craft_set_taps / kocr_crnn_set_taps (taps.h): the tensors recorded during kocr_craft_forward or kocr_crnn_forward;
  // nullptr = no taps.  While a tapped launch runs, tap_rows collects the profiler row names of what it launched
  // (ProfScope), i.e. its kernel family.
  Taps* taps = nullptr;
  std::vector<std::string>* tap_rows = nullptr;

  // the device-resident results of the last successful kocr_pipeline call (kocr_pipeline_device_results): boxes in the pl
  // arena, counts in the post-processing scratch, label rows in the io arena -- all valid until the next call that uses
  // those arenas, which resets `state` first (arena_reserve).  lw: the label width the rows were produced with, which is
  // their pitch whatever kocr_crnn_set_rnn_steps_to_discard says afterwards (kocr_pipeline_results_shape reports it)
  struct LastPipeline {
    const float* d_boxes = nullptr;
    const int32_t* d_counts = nullptr;
    const int32_t* d_labels = nullptr;  // [M][lw]
    int N = 0, cap = 0, M = 0, lw = 0;
    Resident state = Resident::NONE;  // never OFF: the call has no switch
  } last_pl;

  // scores (kocr_set_scores; DESIGN.md section 4, "Scores"): with the switch on, kocr_get_boxes / kocr_detect /
  // kocr_recognize_boxes / kocr_pipeline leave what they have of the three scores resident for kocr_detection_scores /
  // kocr_recognition_scores -- detection scores in the post-processing scratch, the recogniser's beside its label rows.
  // lw: the label width the rows were produced with.  Valid like last_pl: until the next call that sizes an arena.
  bool scores_on = false;
  struct LastScores {
    const float* d_det = nullptr;  // [N][cap]
    int N = 0, cap = 0;
    Resident det = Resident::NONE;
    const float* d_logw = nullptr;   // [M]
    const float* d_chars = nullptr;  // [M][lw]
    int M = 0, lw = 0;
    Resident rec = Resident::NONE;
  } last_sc;
  // beam search (kocr_set_beam; DESIGN.md section 4, "Beam search"): with beam_width > 0, kocr_recognize_boxes /
  // kocr_pipeline also run ctc_beam_kernel on every batch's logits and leave the alternatives resident beside the label
  // rows for kocr_recognition_beams.  Valid like last_sc; lw / K: the label width and top_paths they were produced with.
  int beam_width = 0, beam_top_paths = 1;
  struct LastBeam {
    const int* d_labels = nullptr;  // [M][K][lw]
    const float* d_logp = nullptr;  // [M][K]
    int M = 0, lw = 0, K = 0;
    Resident state = Resident::NONE;
  } last_beam;
  void keep_beams(const int* d_labels, const float* d_logp, int M, int lw) {
    last_beam = {d_labels, d_logp, M, lw, beam_top_paths, resident(beam_width > 0)};
  }
  // lexicon (kocr_set_lexicon / kocr_set_lexicon_match; DESIGN.md section 4, "Lexicon"): the caller's words, resident like
  // weights -- label rows and lengths in the caller's order, `order` the words by ascending length (what a wave of
  // lexicon_score_kernel walks).  classes: the recogniser's class count the labels were validated against; dropped_classes:
  // that count of a lexicon that loading another recogniser unloaded (for the refusal's text).  With lex_top > 0 (only
  // while a lexicon is loaded) kocr_recognize_boxes / kocr_pipeline also run the three lexicon launches on every batch's
  // logits and leave index / log_prob resident beside the label rows for kocr_recognition_lexicon.  Valid like last_beam.
  // lex_scratch: the bytes of the M x V value scratch one chunk of crops may take (kocr_set_lexicon_scratch).
  struct Lexicon {
    int* d_words = nullptr;  // [V][Lmax]
    int* d_lens = nullptr;   // [V]
    int* d_order = nullptr;  // [V]
    int V = 0, Lmax = 0, classes = 0, dropped_classes = 0;
  } lex;
  int lex_top = 0;
  static constexpr size_t LEX_SCRATCH_DEFAULT = (size_t)256 << 20;
  size_t lex_scratch = LEX_SCRATCH_DEFAULT;
  struct LastLexicon {
    const int* d_index = nullptr;   // [M][K]
    const float* d_logp = nullptr;  // [M][K]
    int M = 0, K = 0;
    Resident state = Resident::NONE;
  } last_lex;
  void keep_lexicon(const int* d_index, const float* d_logp, int M) {
    last_lex = {d_index, d_logp, M, lex_top, resident(lex_top > 0)};
  }
  // character sets (kocr_set_charsets / kocr_set_charset; DESIGN.md section 4, "Character sets"): the caller's S sets as a
  // bit table, resident like the lexicon; classes: the recogniser's class count it was built for.  charset: the set every
  // decode of the context runs under (-1: none -- the unmasked kernels); only ever >= 0 while a table is loaded.
  struct Charsets {
    uint32_t* d_bits = nullptr;  // [S][ceil(classes / 32)]
    int S = 0, classes = 0;
  } charsets;
  int charset = -1;
  CharMask charmask() const { return CharMask{charsets.d_bits, nullptr, charsets.d_bits ? charset : -1, 0, 0}; }
  // ... with a per-crop list (device) in place of the uniform set
  CharMask charmask(const int32_t* d_set_of, int shift) const {
    return d_set_of ? CharMask{charsets.d_bits, d_set_of, -1, shift, 0} : charmask();
  }
  // patterns (kocr_set_patterns / kocr_set_pattern; DESIGN.md section 4, "Patterns"): the caller's P automata as node tables,
  // resident like the lexicon; S / NT: every pattern's state and node count (host); classes: the recogniser's class count
  // they were built for.  pattern: the one every crop of kocr_recognize_boxes / kocr_pipeline is also decoded under (-1:
  // none); only ever >= 0 while a table is loaded.  The rows stay resident beside the label rows for
  // kocr_recognition_patterns.  Valid like last_beam.
  struct Patterns {
    int* d_hdr = nullptr;
    int2* d_nodes = nullptr;
    int2* d_states = nullptr;
    int* d_pred = nullptr;
    int P = 0, classes = 0;
    std::vector<int> S, NT;
    PatternTables tables() const { return PatternTables{d_hdr, d_nodes, d_states, d_pred}; }
  } patterns;
  int pattern = -1;
  struct LastPattern {
    const int* d_labels = nullptr;    // [M][lw]
    const float* d_logpath = nullptr;  // [M]
    const float* d_logp = nullptr;     // [M]
    int M = 0, lw = 0;
    Resident state = Resident::NONE;
  } last_pat;
  void keep_patterns(const int* d_labels, const float* d_logpath, const float* d_logp, int M, int lw, bool on) {
    last_pat = {d_labels, d_logpath, d_logp, M, lw, resident(on)};
  }
  // character boxes (kocr_set_char_boxes; DESIGN.md section 4, "Characters"): with the switch on, kocr_get_boxes /
  // kocr_detect / kocr_pipeline run the two launches of chars.hip on the heat-maps and boxes in HBM (chars_resident) and leave
  // the packed quads and scores resident for kocr_detection_char_boxes.  Workspace and results live in two arenas of their
  // own (chw, chr: never allocated while the switch stays off and kocr_char_boxes is not called), because the callers' arenas
  // are spoken for.  counts / off are host copies: the per-word counts in packed word order and the pages' word offsets.  Valid
  // like last_sc.
  bool chars_on = false;
  CharsRule chars_rule{0.4, 0.7, 0.2};
  Arena chw, chr;
  struct LastChars {
    const float* d_quads = nullptr;   // [total][4][2]
    const float* d_scores = nullptr;  // [total]
    std::vector<int32_t> counts, off;
    int N = 0, cap = 0;
    long long total = 0;
    Resident state = Resident::NONE;
  } last_ch;
  // orientation (kocr_set_orientation; DESIGN.md section 4, "Orientation"): with orient_mode != KOCR_ORIENT_OFF,
  // kocr_recognize_boxes / kocr_pipeline warp and read every box in two orientations (2 M crops, candidate-interleaved), and
  // orient_select_kernel leaves the winners' rows in compact [M] buffers beside them: the label rows (what last_pl.d_labels
  // and the callers' labels get), the scores, and the turns, quads and log_word pairs for kocr_recognition_orientation.
  // Valid like last_sc.
  int orient_mode = KOCR_ORIENT_OFF;
  double orient_ratio = 1.5;
  struct LastOrient {
    const int* d_turns = nullptr;    // [M]
    const float* d_quads = nullptr;  // [M][4][2]
    const float* d_pairs = nullptr;  // [M][2]
    int M = 0;
    Resident state = Resident::NONE;
  } last_or;
  void keep_orientation(const int* d_turns, const float* d_quads, const float* d_pairs, int M) {
    last_or = {d_turns, d_quads, d_pairs, M, resident(orient_mode != KOCR_ORIENT_OFF)};
  }
  // long words (include/kocr_windows.h; DESIGN.md section 4, "Long words"): kocr_recognize_boxes_windowed leaves its ragged rows
  // in the io arena for kocr_windowed_results_shape / kocr_windowed_results.  lw: the row width, the longest T' of the call.
  // Valid like last_pl; never OFF: the call has no switch.
  struct LastWindowed {
    const int32_t* d_labels = nullptr;   // [M][lw]
    const float* d_logw = nullptr;       // [M]
    const float* d_chars = nullptr;      // [M][lw]
    const int32_t* d_frames = nullptr;   // [M]
    const int32_t* d_windows = nullptr;  // [M]
    int M = 0, lw = 0;
    Resident state = Resident::NONE;
  } last_win;
  // Whoever sizes an arena is about to overwrite what the records point at: arena_reserve calls this, and so does an entry
  // point that replaces the results without sizing one.  The one list of what there is to forget.
  void invalidate_results() {
    last_pl.state = last_sc.det = last_sc.rec = last_beam.state = last_lex.state = last_ch.state = last_or.state = last_pat.state =
        last_win.state = Resident::NONE;
  }
  // what an entry point leaves resident at its end (with the switch off: only the fact that it was off)
  void keep_det_scores(const float* d, int N, int cap) {
    last_sc.d_det = d;
    last_sc.N = N;
    last_sc.cap = cap;
    last_sc.det = resident(scores_on);
    // ... and the character boxes that chars_resident has put beside them
    last_ch.N = N;
    last_ch.cap = cap;
    last_ch.state = resident(chars_on);
  }
  void keep_rec_scores(const float* d_logw, const float* d_chars, int M, int lw) {
    last_sc.d_logw = d_logw;
    last_sc.d_chars = d_chars;
    last_sc.M = M;
    last_sc.lw = lw;
    last_sc.rec = resident(scores_on);
  }

  // developer instrumentation of the fp16x2 range assumption (kocr_range_stats_enable): off = no cost
  bool range_on = false;
  void* d_range = nullptr;
  std::map<std::string, RangeRow> range;

  // profiler
  bool prof_on = false;
  std::map<std::string, ProfRow> prof;
  struct Pending {
    std::string name;
    hipEvent_t a, b;
  };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> ev_pool;
  hipEvent_t get_event();
  void prof_begin(const char* name, double flops, double bytes);
  void prof_end();
  int prof_flush();
};

// The one pair of calls through which the library takes device memory and gives it back (api.cpp): they keep the process-wide
// figures of kocr_debug_memory_stats.  tests/test_lifecycle_cpu.py asserts that the runtime's allocator is called nowhere else.
hipError_t kocr_counted_malloc(void** p, size_t bytes);
hipError_t kocr_counted_free(void* p);  // nullptr is ignored

inline int kocr_ctx::dev_alloc(void** out, size_t bytes) {
  void* p = nullptr;
  const size_t want = bytes ? bytes : 4;
  hipError_t e = kocr_counted_malloc(&p, want);
  if (e != hipSuccess) {
    set_err(std::string("device allocation failed: ") + hipGetErrorString(e));
    return KOCR_ENOMEM;
  }
  owned.push_back(Owned{p, want});
  *out = p;
  return KOCR_OK;
}
inline void kocr_ctx::release(void* p) {
  if (!p) return;
  for (size_t i = owned.size(); i-- > 0;)
    if (owned[i].p == p) {
      owned.erase(owned.begin() + (long)i);
      kocr_counted_free(p);
      return;
    }
}
inline void kocr_ctx::release_since(size_t mark) {
  while (owned.size() > mark) {
    kocr_counted_free(owned.back().p);
    owned.pop_back();
  }
}

int arena_reserve(kocr_ctx* ctx, Arena& a, size_t bytes);
// guard mode only (api.cpp): the fill of one guard on the stream; the comparison of the recorded guards, which latches the
// first damaged one in ctx->guard_damage and forgets the list
void arena_guard_fill(Arena& a, size_t at, size_t len);
void arena_guard_check(Arena& a);
// poison mode only (api.cpp): the fill of one allocation on the stream.  The sub-allocators that carve a reserved block
// themselves (craft.cpp: LivePool) call it for every hand-out.
void arena_poison_fill(Arena& a, void* p, size_t bytes);
inline void Arena::reset() {
  if (!guards.empty()) arena_guard_check(*this);
  off = gextra = 0;
}
inline void* arena_alloc(Arena& a, size_t bytes) {
  const size_t o = (a.off + 255) & ~(size_t)255;
  a.note(o + bytes);
  if (!a.gctx) {
    if (o + bytes > a.cap) return nullptr;
    a.off = o + bytes;
    if (a.pctx) arena_poison_fill(a, a.base + o, bytes);
    return a.base + o;
  }
  const size_t at = o + a.gextra, end = at + bytes, glen = ((end + 255) & ~(size_t)255) + ARENA_GUARD_BYTES - end;
  if (end + glen > a.cap) return nullptr;
  a.off = o + bytes;
  a.gextra += ARENA_GUARD_BYTES;
  a.guards.push_back(ArenaGuard{at, end, glen});
  arena_guard_fill(a, end, glen);
  if (a.pctx) arena_poison_fill(a, a.base + at, bytes);
  return a.base + at;
}
inline void* kocr_ctx::ws_alloc(size_t bytes) { return arena_alloc(ws, bytes); }
inline Arena* kocr_ctx::arena_at(int i) {
  Arena* const all[N_ARENAS] = {&ws, &pp, &pp2, &io, &pl, &bx, &chw, &chr};
  return i >= 0 && i < N_ARENAS ? all[i] : nullptr;
}

// RAII-less helper used around launches
struct ProfScope {
  kocr_ctx* c;
  ProfScope(kocr_ctx* ctx, const char* name, double flops, double bytes) : c(ctx) {
    if (c->tap_rows) c->tap_rows->push_back(name);
    if (c->prof_on) c->prof_begin(name, flops, bytes);
  }
  ~ProfScope() {
    if (c->prof_on) c->prof_end();
  }
};

// the profiler row of one launch: `row`, or with KOCR_PROF_LAYERS (developer) one row per layer, `layer_row` + ":" + layer
inline std::string prof_name(const kocr_ctx* ctx, const ConvLayer& L, const std::string& row, const std::string& layer_row) {
  return ctx->prof_layers ? layer_row + ":" + L.name : row;
}

// Launch of a persistent kernel K: min(total_tiles, n_cu * occ) blocks of `block` threads with `lds` bytes of dynamic LDS.
// The kernel's LDS limit is raised to `attr_lds` (>= lds: a launch whose coefficient area depends on the layer may use less
// than the maximum) once per device -- one process may hold contexts on several GPUs; a race only repeats the call.
template <auto K, typename P>
int launch_persistent(kocr_ctx* ctx, const P& p, int total_tiles, int block, int lds, int attr_lds, int occ = 1,
                      int* grid_out = nullptr) {
  static std::atomic<bool> attr_done[64];
  const int dev = ctx->device & 63;
  if (!attr_done[dev]) {
    KOCR_HIP(ctx, hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, attr_lds));
    attr_done[dev] = true;
  }
  const int slots = ctx->n_cu * occ;
  const int grid = total_tiles < slots ? total_tiles : slots;
  if (grid_out) *grid_out = grid;
  hipLaunchKernelGGL(K, dim3(grid), dim3(block), lds, ctx->stream, p);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// wave-level max |x| into a Tensor::amax slot (device code; values are non-negative, so uint order = float order)
#if defined(__HIPCC__)
// max over the wave of a value that is >= 0 (not NaN) in every lane, as its bits, wave-uniform.  Non-negative floats order
// like their bit patterns, so the cross-row step is four v_readlane + scalar max; the in-row steps are DPP modifiers.  No
// lane-index operand anywhere: the __shfl_xor version kept six (lane ^ o) * 4 addresses alive across a persistent kernel's
// K loop -- spilled there, and reloaded one by one (each a full memory round trip) in every tile's epilogue.
__device__ __forceinline__ unsigned kocr_wave_max_bits(float m) {
  int v = __float_as_int(m);
  int t;
  t = __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);  // quad_perm [1, 0, 3, 2]
  v = v > t ? v : t;
  t = __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);  // quad_perm [2, 3, 0, 1]
  v = v > t ? v : t;
  t = __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);  // row_half_mirror
  v = v > t ? v : t;
  t = __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);  // row_mirror: every lane holds its row's maximum
  v = v > t ? v : t;
  const unsigned a = (unsigned)__builtin_amdgcn_readlane(v, 0), b = (unsigned)__builtin_amdgcn_readlane(v, 16),
                 c = (unsigned)__builtin_amdgcn_readlane(v, 32), d = (unsigned)__builtin_amdgcn_readlane(v, 48);
  const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}
__device__ __forceinline__ unsigned kocr_amax_peek(const unsigned* slot) {
  // a relaxed agent-scope atomic load: read at L2 like a volatile read, but without the s_waitcnt vmcnt(0) hipcc puts
  // behind every volatile access
  return __hip_atomic_load(const_cast<unsigned*>(slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The slot's value as the caller read it beforehand (kocr_amax_peek at the start of its epilogue, consumed here after the
// epilogue's arithmetic): the read's latency is hidden instead of being waited for tile after tile.
// One address for a whole image: the atomic is issued only when it can still raise the slot (a stale read merely costs a
// redundant atomic).  Unconditional atomics from every tile serialise in L2 -- measured 4x on the first layer.
__device__ __forceinline__ void kocr_amax_update_known(unsigned* slot, float m, unsigned seen) {
  const unsigned bits = kocr_wave_max_bits(m);
  if (bits > seen) {  // uniform
    int l = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(l));  // not a loop invariant to hoist (and spill) out of the caller's tile loop
    if (l == 0) atomicMax(slot, bits);
  }
}
__device__ __forceinline__ void kocr_amax_update(unsigned* slot, float m) { kocr_amax_update_known(slot, m, kocr_amax_peek(slot)); }
#endif

// ---------------------------------------------------------------------------------------
// kernels (launchers)
// ---------------------------------------------------------------------------------------
// conv_mfma.hip
int prepare_conv(kocr_ctx* ctx, ConvLayer& L, const float* w, bool w_is_oihw, int Cin, int Cout,
                 int KH, int KW, int dil, const float* pre_a, const float* pre_b, int relu,
                 const float* post_a, const float* post_b);
int release_layer(kocr_ctx* ctx, ConvLayer& L);  // every device copy of L given back; L is then not ready()
// in_u8 != nullptr: first-layer mode, raw RGB bytes + LUT normalisation.
// developer instrumentation (KOCR_DISPATCH_LOG=<file>): one line per distinct (kernel family, layer, input shape) the dispatcher
// of launch_conv_pool chose in this process -- the table of DESIGN.md section 3 "which shapes reach which family" comes from it
void kocr_note_dispatch(const char* family, const ConvLayer& L, const Tensor& in);
int launch_conv(kocr_ctx* ctx, const ConvLayer& L, const Tensor& in, const uint8_t* in_u8,
                const float* lut, const Tensor& out);
int launch_conv_pool(kocr_ctx* ctx, const ConvLayer& L, const Tensor& in, const uint8_t* in_u8,
                     const float* lut, const Tensor& out, const Tensor* pool, bool need_full = true);
// Split arithmetic of conv_wsplit.hip / conv_dsplit.hip: 0 = bf16 x 3 pieces / 6 products (exact split),
// 1 = fp16 x 2 pieces / 3 products (RNE split at 2^-24, exact power-of-two scaling from Tensor::amax).
// kocr_ctx::split_mode; KOCR_SPLIT=bf16|f16 sets the initial value, kocr_set_split_mode changes it.
// conv_wsplit.hip
int prepare_wsplit(kocr_ctx* ctx, ConvLayer& L, const float* w, bool w_is_oihw);
bool wsplit_applicable(const kocr_ctx* ctx, const ConvLayer& L, const Tensor& in);
int launch_conv_wsplit(kocr_ctx* ctx, const ConvLayer& L, const Tensor& in, const Tensor& out, const Tensor* pool,
                       bool need_full);
// conv_w43.hip: Winograd F(4,3) on the bf16 cores (bf16x3 mode; 3.0 issued FLOPs per algorithmic FLOP instead of 4.0)
int prepare_w43(kocr_ctx* ctx, ConvLayer& L, const float* w, bool w_is_oihw);
// conv_w43h.hip: the same algebra on the fp16 cores, operands scaled by exact powers of two (per image / per cout) and
// split into two fp16 pieces, three products (KOCR_SPLIT_F16X2: 1.5 issued FLOPs per algorithmic FLOP) or cut to ONE
// fp16 piece, one product (KOCR_SPLIT_F16X1, the reduced-precision fast mode: 0.5).  launch_conv_w43 dispatches to it.
struct W4Params;
int prepare_w43h(kocr_ctx* ctx, ConvLayer& L, const float* w, bool w_is_oihw, const float* pre_a);
// mode: 0 = the image tiles exactly, 1 = ragged (any H, W), 2 = cell grid (launch_w43vh, geo 1 only)
int launch_w43vh(kocr_ctx* ctx, W4Params& p, bool fuse, int geo, int pieces, int mode = 0);
int launch_w43rh(kocr_ctx* ctx, W4Params& p, bool fuse, int pieces, int mode = 0);
int launch_w43fh(kocr_ctx* ctx, W4Params& p, int pieces);
bool w43_applicable(const kocr_ctx* ctx, const ConvLayer& L, const Tensor& in);
bool w43_cells_ok(const kocr_ctx* ctx, const ConvLayer& L);   // a cell-grid tensor (Tensor::cellW) can run through layer L
bool w43_flat_h_ok(const kocr_ctx* ctx, const ConvLayer& L);  // a width-padded tensor (Tensor::Wv) can
int launch_conv_w43(kocr_ctx* ctx, const ConvLayer& L, const Tensor& in, const Tensor& out, const Tensor* pool,
                    bool need_full);
// conv_dsplit.hip
int prepare_dsplit(kocr_ctx* ctx, ConvLayer& L, const float* w, bool w_is_oihw);
bool dsplit_applicable(const kocr_ctx* ctx, const ConvLayer& L, const Tensor& in);
bool dsplit_usable(const kocr_ctx* ctx, const ConvLayer& L, const Tensor& in);
// launch_conv prefers conv_ds from this many pixels on; below it a layer stays on the fp32 MFMA kernel, whose sums round
// differently.  The recogniser's per-frame 1x1 layers (50 pixels a crop) cross it at 82 crops.
constexpr size_t DSPLIT_MIN_PIXELS = 4096;
// conv_hsplit.hip
int prepare_hsplit(kocr_ctx* ctx, ConvLayer& L, const float* w, bool w_is_oihw);
bool hsplit_applicable(kocr_ctx* ctx, const ConvLayer& L, const Tensor& in);
int launch_conv_hsplit(kocr_ctx* ctx, const ConvLayer& L, const Tensor& in, const Tensor& out);
int prepare_first(kocr_ctx* ctx, ConvLayer& L, const float* w, bool w_is_oihw);
bool first_applicable(kocr_ctx* ctx, const ConvLayer& L, const Tensor& in);
int launch_conv_first(kocr_ctx* ctx, const ConvLayer& L, const Tensor& in, const uint8_t* in_u8, const float* lut, const Tensor& out);
int launch_conv_dsplit(kocr_ctx* ctx, const ConvLayer& L, const Tensor& in, const Tensor& out, const Tensor* up = nullptr);
// conv_k5.hip
int prepare_k5(kocr_ctx* ctx, ConvLayer& L, const float* w, bool w_is_oihw);
bool k5_applicable(kocr_ctx* ctx, const ConvLayer& L, const Tensor& in, const Tensor& out);
int launch_conv_k5(kocr_ctx* ctx, const ConvLayer& L, const Tensor& in, const Tensor& out);
// elementwise.hip
// row_off: input row that starts output row 0 (0 = keras 'valid' pooling; 1 = the same pooling seen
// through a vertical flip of an odd-height tensor, as in the CRNN's natural-orientation conv stack)
int launch_maxpool2x2(kocr_ctx* ctx, const Tensor& in, const Tensor& out, int row_off = 0);
int launch_maxpool3x3s1(kocr_ctx* ctx, const Tensor& in, const Tensor& out);
int launch_resize_bilinear(kocr_ctx* ctx, const Tensor& in, const Tensor& out);
int launch_copy_channels(kocr_ctx* ctx, const Tensor& in, const Tensor& out);
// per-image max |x| of a tensor into t.N slots (atomicMax; the slots are NOT cleared), and slot-to-slot propagation
int launch_absmax(kocr_ctx* ctx, const Tensor& t, unsigned* slots);
int launch_amax_copy(kocr_ctx* ctx, const unsigned* from, unsigned* to, int n);
int launch_range_stats(kocr_ctx* ctx, const std::string& name, const Tensor& t, const unsigned* slots, int top);
// conv_cls.6 + conv_cls.8 of the CRAFT head in one pass (16 -> 16 ReLU -> 2), heat-map written densely
int launch_head_tail(kocr_ctx* ctx, const ConvLayer& L6, const ConvLayer& L8, const Tensor& in, float* d_heat);

// craft.cpp
int craft_load(kocr_ctx* ctx, int n, const char* const* names, const float* const* data,
               const int64_t* shapes, const int* ranks);
int craft_forward(kocr_ctx* ctx, const void* d_img, int dtype, int N, int H, int W, float* d_heat);
// a complete detector is loaded (not: none yet, a refused first load, a load that failed on its way).  The entry points ask
// this ahead of any work; craft_forward asks again.
bool craft_loaded(const kocr_ctx* ctx);
size_t craft_workspace_bytes(int N, int H, int W);
void craft_free(kocr_ctx* ctx);
void taps_free(kocr_ctx* ctx);  // taps.cpp

// crnn.cpp
// the recogniser's geometry: crops of CRNN_CROP_H x CRNN_CROP_W, CRNN_STEPS time steps of CRNN_FEAT features (the backbone's
// [lstm_11 | lstm_11_back] concatenation); a label row has crnn_label_width() = CRNN_STEPS - rnn_steps_to_discard columns
constexpr int CRNN_CROP_H = 31, CRNN_CROP_W = 200, CRNN_STEPS = 50, CRNN_FEAT = 256;
constexpr size_t CRNN_CROP_PIXELS = (size_t)CRNN_CROP_H * CRNN_CROP_W;
void crnn_free(kocr_ctx* ctx);
int crnn_load(kocr_ctx* ctx, int n, const char* const* names, const float* const* data, const int64_t* shapes,
              const int* ranks);
int crnn_classes(kocr_ctx* ctx);
int crnn_label_width(kocr_ctx* ctx);  // 50 - rnn_steps_to_discard (48)
int crnn_set_discard(kocr_ctx* ctx, int d);
size_t crnn_workspace_bytes(int M, int n_classes);
// What runs behind fc_12 on a batch's logits, and where its results go: one request for crnn_forward, crnn_decode_logits,
// the recogniser stage (abi.h) and the staged calls of api.cpp.  Each member carries its own "off".
// sc: the greedy decode's launch also writes the word log-probabilities [M] and the character scores [M][crnn_label_width()]
// (ctc_scores_kernel instead of ctc_kernel; the label rows and probabilities are the same bits).
struct CrnnScores {
  bool on = false;
  float* d_logw = nullptr;
  float* d_chars = nullptr;
};
// bm (beam_width > 0): ctc_beam_kernel on the same logits: d_labels [M][top_paths][crnn_label_width()], d_logp [M][top_paths].
struct CrnnBeam {
  int beam_width = 0, top_paths = 0;
  int* d_labels = nullptr;
  float* d_logp = nullptr;
};
// lx (top_words > 0): after the beam, the three lexicon launches on the same logits: d_index / d_logp [M][top_words]; d_all
// (nullable) [M][V]: lexicon_score_kernel's own values, else they live in workspace scratch.
struct CrnnLexicon {
  int top_words = 0;
  int* d_index = nullptr;
  float* d_logp = nullptr;
  float* d_all = nullptr;
};
// pt (on): after the lexicon match, lexicon_logq_kernel<false> and the two pattern launches on the same logits, never masked:
// crop m under pattern of[first + m] (HOST list; d_of its device copy), or under `uniform` when `of` is null; -1: none (a -1 /
// -inf row: a run like any other, so "off" is a flag of its own).  d_labels [M][crnn_label_width()], d_logpath / d_logp [M].
struct CrnnPattern {
  bool on = false;
  const int32_t* of = nullptr;
  const int32_t* d_of = nullptr;
  int uniform = -1;
  int first = 0;
  int* d_labels = nullptr;
  float* d_logpath = nullptr;
  float* d_logp = nullptr;
};
// greedy: the decode launch itself, d_labels [M][crnn_label_width()] and (nullable) d_probs [M][crnn_label_width()][C]; off,
// nothing is launched for it (kocr_crnn_beam / _lexicon / _pattern).  The switches are flags rather than null pointers because
// the recogniser stage lists its buffers before they have addresses.
// cm: the character sets of the batch's crops (CharMask above; off by default).  Every decode launch behind fc_12 but the
// patterns' reads its rows through it; the logits themselves, the taps, the loss and the features are never masked.
struct CrnnDecode {
  bool greedy = false;
  int* d_labels = nullptr;
  float* d_probs = nullptr;
  CrnnScores sc;
  CrnnBeam bm;
  CrnnLexicon lx;
  CrnnPattern pt;
  CharMask cm;
  static constexpr int MAX_OUTPUTS = 12;
  // THE list of the outputs: f(pointer&, bytes per crop) for every one the request produces, for label rows of LW columns, C
  // classes and a lexicon of V words; stops at the first failure
  template <class F> int each(int LW, int C, int V, F f) {
    const size_t lw = (size_t)LW, i4 = sizeof(int32_t), f4 = sizeof(float);
    if (greedy) {
      KOCR_TRY(f(d_labels, lw * i4));
      if (d_probs) KOCR_TRY(f(d_probs, lw * C * f4));
    }
    if (sc.on) {
      KOCR_TRY(f(sc.d_logw, f4));
      KOCR_TRY(f(sc.d_chars, lw * f4));
    }
    if (bm.beam_width) {
      KOCR_TRY(f(bm.d_labels, bm.top_paths * lw * i4));
      KOCR_TRY(f(bm.d_logp, bm.top_paths * f4));
    }
    if (lx.top_words) {
      KOCR_TRY(f(lx.d_index, lx.top_words * i4));
      KOCR_TRY(f(lx.d_logp, lx.top_words * f4));
      if (lx.d_all) KOCR_TRY(f(lx.d_all, (size_t)V * f4));
    }
    if (pt.on) {
      KOCR_TRY(f(pt.d_labels, lw * i4));
      KOCR_TRY(f(pt.d_logpath, f4));
      KOCR_TRY(f(pt.d_logp, f4));
    }
    return KOCR_OK;
  }
  // the same request for the crops from `s` on: every output at its row s, the per-crop lists read from entry s
  CrnnDecode from(long s, int LW, int C, int V) const {
    CrnnDecode r = *this;
    r.each(LW, C, V, [s](auto*& p, size_t b) {
      p = (std::remove_reference_t<decltype(p)>)((char*)p + (size_t)s * b);
      return KOCR_OK;
    });
    r.cm = cm.from((int)s);
    r.pt.first += (int)s;
    return r;
  }
};
// The recogniser on d_crops [M][31][200] (device), three ways over one body -- the launches up to the stop are the same in all
// three: up to the Concatenate output, written to d_feats [M][50][256] (kocr_crnn_features); up to fc_12's logits, *d_logits =
// [M][50][n_classes] in the workspace (crnn_ctc_loss); the whole recogniser with what `rq` asks for behind fc_12.
// crops of the smallest batch that takes the large-batch kernels for the per-frame 1x1 layers (crnn.cpp); 0: no such size
int crnn_small_batch(const kocr_ctx* ctx);
int crnn_features(kocr_ctx* ctx, const float* d_crops, int M, float* d_feats);
int crnn_logits(kocr_ctx* ctx, const float* d_crops, int M, const float** d_logits);
int crnn_forward(kocr_ctx* ctx, const float* d_crops, int M, const CrnnDecode& rq);
// crnn_forward's launches behind fc_12 alone, on the caller's logits [M][50][n_classes] (device): the same launch functions with
// the same arguments.  No taps, nothing resident changes.
int crnn_decode_logits(kocr_ctx* ctx, const float* d_lg, int M, const CrnnDecode& rq);
// Crops per chunk of the pattern launches: as many as lex_scratch bytes (kocr_set_lexicon_scratch) hold of what a crop takes
// -- its To x C table and, when they leave LDS, its back-pointers -- clamp(lex_scratch / per crop, 1, M), for the patterns the
// M crops from pt.first on run under; and the workspace bytes that the launches of any recogniser batch (at most 1024 crops)
// of a call's M crops take on top of crnn_workspace_bytes.
int pattern_chunk(kocr_ctx* ctx, int M, const CrnnPattern& pt);
size_t pattern_workspace_bytes(kocr_ctx* ctx, int M, const CrnnPattern& pt);
// the tables freed, P = 0, the switch off
void patterns_unload(kocr_ctx* ctx);
// KOCR_EINVAL naming the entry unless each of pattern_of[0 .. M) (HOST) lies in [-1, P); `what`: what an entry belongs to
int patterns_validate(kocr_ctx* ctx, const char* fn, const int32_t* pattern_of, long M, const char* what);
// KOCR_EINVAL when a pattern cannot run here: an active character set (kocr_set_charset), or orientation
int pattern_refusal(kocr_ctx* ctx, const char* fn);
// Crops per chunk of the lexicon launches: as many as lex_scratch bytes of values hold, clamp(lex_scratch / (4 V), 1, M);
// and the workspace bytes the launches take on top of crnn_workspace_bytes(M) (own_values: no d_all buffer is given)
int lexicon_chunk(const kocr_ctx* ctx, int M);
size_t lexicon_workspace_bytes(kocr_ctx* ctx, int M, bool own_values);
// KOCR_EINVAL naming the argument unless 1 <= top_words <= 64; and unless a lexicon is loaded (saying why not)
int lexicon_validate(kocr_ctx* ctx, const char* fn, int top_words);
// the device copies freed, V = 0, the match switched off; dropped_classes as given
void lexicon_unload(kocr_ctx* ctx, int dropped_classes);
// the character-set table freed, S = 0, the uniform switch off
void charsets_unload(kocr_ctx* ctx);
// KOCR_EINVAL naming the entry unless each of set_of[0 .. M) (HOST) lies in [-1, S); `what`: what an entry belongs to ("box")
int charsets_validate(kocr_ctx* ctx, const char* fn, const int32_t* set_of, long M, const char* what);
// KOCR_EINVAL naming the argument unless 1 <= beam_width <= 64 and 1 <= top_paths <= beam_width
int beam_validate(kocr_ctx* ctx, const char* fn, int beam_width, int top_paths);
// training_model (recognition.py:334-349): crnn_logits, then ctc_loss_kernel on fc_12's softmax of frames
// rnn_steps_to_discard .. + input_length - 1; labels / lengths already validated (ctc_validate) and on the device
struct CtcLabels {  // device: label rows [M][lstride], their lengths [M] (at most Lmax), the input lengths [M]
  const int* d_lab = nullptr;
  int lstride = 0;
  const int* d_len = nullptr;
  const int* d_in_len = nullptr;
  int Lmax = 0;
};
int crnn_ctc_loss(kocr_ctx* ctx, const float* d_crops, int M, const CtcLabels& lab, float* d_loss);
// the same loss launch on logits [M][50][n_classes] that are already on the device (crnn_ctc_loss's tail; kocr_crnn_decode_logits)
int crnn_logits_loss(kocr_ctx* ctx, const float* d_lg, int M, const CtcLabels& lab, float* d_loss);
// keras.backend.ctc_batch_cost's refusals on host arrays, before anything is launched: T_m in [1, T],
// L_m in [0, min(T_m, label_stride)], labels[m][0 .. L_m) in [0, C - 2]; KOCR_EINVAL naming the sample.  *Lmax = max L_m.
int ctc_validate(kocr_ctx* ctx, const char* fn, int M, int T, int C, const int32_t* labels, int label_stride,
                 const int32_t* label_lengths, const int32_t* input_lengths, int* Lmax);

// crnn_kernels.hip
// the bytes of 16-bit back-pointers one crop takes in the workspace under patterns of at most NTmax nodes / Smax states (0:
// they fit the launch's LDS), and the two pattern launches on the table d_lq of launch_lexicon_logq
size_t pattern_bp_bytes(int To, int C, int NTmax, int Smax);
int launch_pattern(kocr_ctx* ctx, const float* d_logits, const float* d_lq, int M, int T, int C, int discard, const PatternTables& pt,
                   const int32_t* d_pat_of, int uniform, int first, int NTmax, int Smax, void* d_bp, int* d_labels, float* d_logpath,
                   float* d_logp);
int launch_ctc_loss(kocr_ctx* ctx, bool logits, const float* d_y, int M, int T, int C, int t0, const int* d_lab, int lstride,
                    const int* d_len, const int* d_in_len, float* d_loss, int Lmax);

// postproc.hip
// dev (optional): device-side results for a caller that keeps going on the stream -- the per-image counts and the
// totals block (totals[2] = components whose contour list is empty); with dev set, the final synchronisation that
// fetches n_empty is skipped and the caller reads totals[2] itself.  Both pointers live until the next call.
// d_scores: [N][cap] float32, the detection score (the text map's maximum over the component) of the box in the same slot.
struct PPDeviceOut {
  int* d_counts = nullptr;
  int* d_totals = nullptr;
  float* d_scores = nullptr;
};
int postproc_get_boxes(kocr_ctx* ctx, const float* d_heat, int N, int h, int w, float det_thr,
                       float text_thr, float link_thr, int size_thr, float* d_boxes, int cap,
                       int* h_counts, int* n_empty_out, PPDeviceOut* dev = nullptr, const float** d_scores = nullptr);

// warp.hip
struct WarpParam {
  double mi[9];  // inverse homography (crop px -> image px)
  int img;       // image index
  int cw, ch;    // crop size (<= target); outside -> 0
  int pad;
};
int warp_prepare(const float* box, int target_h, int target_w, WarpParam* out, float* ordered_box);
int launch_warp(kocr_ctx* ctx, const uint8_t* d_img, int H, int W, const WarpParam* d_prm, int M, int th,
                int tw, float* d_crops);
// the same set-up on the device, one thread per box slot of d_boxes[N][cap][4][2] (d_counts[N] on the device);
// *d_status = max return code of warp_prepare over all boxes (caller zeroes it)
int launch_warp_prepare(kocr_ctx* ctx, const float* d_boxes, const int* d_counts, int N, int cap, int th, int tw,
                        WarpParam* d_prm, int* d_status);
int launch_warp_quads(kocr_ctx* ctx, const float* d_src, const float* d_dst, const int* d_img, const int* d_cw,
                      const int* d_ch, int M, WarpParam* d_prm, double* d_mfwd, int* d_status);
// Orientation: candidate c (0 / 1) of a box in mode KOCR_ORIENT_FLIP / KOCR_ORIENT_ANY -- its quarter turns, its source quad
// (8 floats: the ordered box's corners renamed) and the warp parameters of that quad; return code as warp_prepare.  The
// launch does the same on the device, one thread per (box slot, candidate), for crop 2 (offset + b) + c.
int warp_prepare_turned(const float* box, int mode, double tall_ratio, int c, int target_h, int target_w, WarpParam* out, int* turn,
                        float* quad);
int launch_warp_prepare_turned(kocr_ctx* ctx, const float* d_boxes, const int* d_counts, int N, int cap, int mode, double tall_ratio,
                               int th, int tw, WarpParam* d_prm, int* d_turns, float* d_quads, int* d_status);
// orient.hip: per word the winner of its two candidates (rows [M][2][..]) into compact [M] buffers
int launch_orient_select(kocr_ctx* ctx, const int* d_lab, const float* d_logw, const float* d_chars, const int* d_turns,
                         const float* d_quads, long M, int LW, int* o_lab, float* o_logw, float* o_chars, int* o_turn, float* o_quad,
                         float* o_pair);

// windows.hip: long words (include/kocr_windows.h).  A window of the call: its word, the frames [lo, hi) kept of its crop and the
// row of the call's ragged sequence buffer [sum T'][C] that frame lo goes to.
struct WindowRec {
  int word, lo, hi, pad;
  long long row;
};
// The plan on the device for M boxes d_boxes [M][4][2] of images d_img_of [M]: d_K [M] windows and d_T [M] frames per word, their
// ordered boxes d_ob [M][4][2], the
// exclusive prefix sums d_woff / d_roff [M + 1], and per window (total = sum K of them, known to the host from the same
// function) its source quad, warp parameters and record.  *d_status: max return code as warp_prepare (the caller zeroes it).
int launch_window_plan(kocr_ctx* ctx, const float* d_boxes, const int* d_img_of, int M, double aspect, int overlap, int discard,
                       long total, int* d_K, int* d_T, float* d_ob, long long* d_woff, long long* d_roff, WarpParam* d_prm,
                       float* d_quads, WindowRec* d_rec, int* d_status);
// The kept logit rows of windows [0, n) of d_rec, whose logits are d_logits [n][50][C], into the ragged buffer d_seq
int launch_window_stitch(kocr_ctx* ctx, const float* d_logits, const WindowRec* d_rec, int n, int C, float* d_seq);
// crnn_kernels.hip: ctc_scores_kernel's two passes on word m's frames d_seq[d_roff[m] .. + d_T[m]) of C classes: labels / chars
// [M][LW] (-1 / 0 behind the decode), logw [M]; LW >= every d_T[m] (the host knows: it sizes the LDS)
int launch_ctc_scores_ragged(kocr_ctx* ctx, const float* d_seq, const long long* d_roff, const int* d_T, int M, int C, int LW,
                             int* d_labels, float* d_logw, float* d_chars);

// warp.hip: detection.compute_maps for a batch of pages (kocr_compute_maps).  A slot is one quad drawn into one plane (0 text,
// 1 link) of one page: the inverse homography and the pixel box [x0, x1] x [y0, y1] it may touch (x1 < x0: nothing).
struct MapSlot {
  double mi[9];
  int x0, y0, x1, y1;
  int img, plane;
};
// device work buffers of launch_compute_maps for n characters of N pages of h x w map pixels
struct MapsWork {
  float* rbox;     // [n][8] rotated boxes
  float* ctr;      // [n][2] centres
  int* permx;      // [n] reading order by x, per line
  int* permy;      // [n] by y
  MapSlot* slots;  // [2n]: ordered character k of a line -> its quad, the link ending at it
  int* planes;     // [N][2][h][w] integer sums
  const float* table;  // [256] float32 v / 255
};
int launch_compute_maps(kocr_ctx* ctx, const uint8_t* d_heat, int hh, int hw, int N, int h, int w, int n_chars,
                        const float* d_quads, const uint8_t* d_space, int n_lines, const int* d_line_off, const int* d_img_off,
                        const MapsWork& wk, float* d_maps);
// Keras' mse on the maps: per-image float64 sums d_sums[N] of the channel-mean squared error over h w pixels
int launch_heat_mse(kocr_ctx* ctx, const float* d_true, const float* d_pred, int N, int hw_px, double* d_sums);

// evaluate.hip: evaluation.score on the device (kocr_iou_table / kocr_score).  The device view of a batch of N images: quads
// int32 [n][4][2] with offsets [N + 1], pair_off[i] = the flat index of image i's first (truth, prediction) pair (truth-major),
// P = pair_off[N], words = truths + predictions of the batch; ignore / texts only for kocr_score (code-point rows with
// offsets [n + 1]).
struct EvalBatch {
  int N = 0;
  long long P = 0, words = 0;
  const int32_t *d_tq = nullptr, *d_toff = nullptr, *d_pq = nullptr, *d_poff = nullptr;
  const long long* d_pair_off = nullptr;
  const uint8_t* d_ignore = nullptr;
  const int32_t *d_ttext = nullptr, *d_ttoff = nullptr, *d_ptext = nullptr, *d_ptoff = nullptr;
};
// a pair whose texts eval_text_kernel compares: flat pair index, truth and prediction index in the batch
struct EvalWork {
  long long k;
  int t, p;
};
// d_iou / d_class may be null (kocr_score without the table / kocr_iou_table); d_work holds P entries, *d_work_count is zero
int launch_eval_iou(kocr_ctx* ctx, const EvalBatch& b, double* d_iou, double iou_threshold, uint8_t* d_class, EvalWork* d_work,
                    unsigned* d_work_count);
int launch_eval_text(kocr_ctx* ctx, const EvalBatch& b, const EvalWork* d_work, const unsigned* d_work_count, double similarity_threshold,
                     uint8_t* d_class);
// d_counts: int64[3], zeroed by the caller
int launch_eval_reduce(kocr_ctx* ctx, const EvalBatch& b, const uint8_t* d_class, uint8_t* d_missed, uint8_t* d_unclaimed, int64_t* d_counts);

// lines.hip: recognised words grouped into text lines (kocr_group_lines; DESIGN.md section 4, "Lines").  d_quads float32
// [total][4][2] with d_off [N + 1]; max_words: the largest page (at most KOCR_LINES_MAX_WORDS; it sizes the LDS).  d_boxes
// (nullable) [total][4][2]: the lines of page i at its WORD offset d_off[i], in page order; launch_lines_pack moves them to
// d_line_off[i] of the packed buffer once the host has the counts.
struct LinesRule {
  double cos_max, min_height_ratio, max_offset, max_gap;
};
size_t lines_lds_bytes(int max_words);
int launch_lines_group(kocr_ctx* ctx, const float* d_quads, const int32_t* d_off, int N, int max_words, const LinesRule& rule,
                       int32_t* d_line_of, int32_t* d_order, int32_t* d_line_counts, float* d_boxes);
int launch_lines_pack(kocr_ctx* ctx, const float* d_scratch, const int32_t* d_off, const long long* d_line_off, int N, float* d_boxes);

// blocks.hip: the quads of a page cut into blocks in reading order (kocr_group_lines with KOCR_LINES_BLOCKS; DESIGN.md section
// 4, "Blocks").  The buffers are launch_lines_group's: d_block_of [total] the block of every quad, d_order [total] per page the
// page-local indices block after block, d_block_counts [N], d_boxes (nullable) [total][4][2] the blocks of page i at its QUAD
// offset d_off[i], which launch_lines_pack packs.  min_gap_x / min_gap_y: the smallest cut in mean line heights.
int launch_blocks_cut(kocr_ctx* ctx, const float* d_quads, const int32_t* d_off, int N, int max_quads, double min_gap_x, double min_gap_y,
                      int32_t* d_block_of, int32_t* d_order, int32_t* d_block_counts, float* d_boxes);
// KOCR_LINES_DESKEW ("Rotated pages"; the rule is tests/deskew_statement.py): d_axes [N][2] float64, every page's text direction,
// the weighted medoid of its quads' directions; d_frame [total][4][2] the quads in their page's frame, which launch_blocks_cut
// then reads; launch_blocks_unframe maps the first d_block_counts[i] boxes at page i's quad offset back onto the page in
// place, before launch_lines_pack.
int launch_blocks_axis(kocr_ctx* ctx, const float* d_quads, const int32_t* d_off, int N, int max_quads, double* d_axes);
int launch_blocks_frame(kocr_ctx* ctx, const float* d_quads, const int32_t* d_off, const double* d_axes, int N, int max_quads, float* d_frame);
int launch_blocks_unframe(kocr_ctx* ctx, float* d_boxes, const int32_t* d_off, const int32_t* d_counts, const double* d_axes, int N);

// table.hip: the word boxes of a table put into rows, columns and spanning cells (kocr_group_lines with KOCR_LINES_TABLE;
// DESIGN.md section 4, "Tables").  d_row_of [total] the row of every quad, d_cols [total] col0 | col1 << 16, d_band_counts [N]
// rows + columns, d_boxes (nullable) [2 total][4][2] the row bands, then the column bands of page i at TWICE its quad offset
// (a page of n quads has at most 2 n bands): launch_lines_pack packs them when it is given the doubled offsets.
int launch_table_grid(kocr_ctx* ctx, const float* d_quads, const int32_t* d_off, int N, int max_quads, double min_gap_x, double min_gap_y,
                      double min_support, int32_t* d_row_of, int32_t* d_cols, int32_t* d_band_counts, float* d_boxes);

// chars.hip: the characters of word boxes from the region map (kocr_char_boxes; DESIGN.md section 4, "Characters").  d_heat
// [N][h][w][2]; M words in packed word order with d_off [N + 1]; word j of page i is quad d_off[i] + j of d_quads with
// stride == 0, quad i * stride + j otherwise.  launch_chars_split fills the workspace rows of every word, launch_chars_pack
// writes the characters of all words in word order: d_char_quads [sum of counts][4][2], d_char_scores [sum of counts].
constexpr int KOCR_CHARS_MAX_PER_WORD = KOCR_CHARS_MAX_COLS / 2;        // two neighbouring columns are never both peaks
constexpr int KOCR_CHARS_BOUNDS_STRIDE = KOCR_CHARS_MAX_PER_WORD + 2;  // K + 1 bounds, rows kept 4-byte aligned
struct CharsWork {
  int32_t *counts = nullptr, *ncols = nullptr;  // [M]
  uint16_t* bounds = nullptr;                   // [M][KOCR_CHARS_BOUNDS_STRIDE] column bounds of the characters
  float* scores = nullptr;                      // [M][KOCR_CHARS_MAX_PER_WORD] profile at the peaks
};
size_t chars_workspace_bytes(int N, long M);
int launch_chars_split(kocr_ctx* ctx, const float* d_heat, int N, int h, int w, const float* d_quads, const int32_t* d_off, int stride,
                       int M, const CharsRule& rule, const CharsWork& wk);
int launch_chars_pack(kocr_ctx* ctx, const float* d_quads, const int32_t* d_off, int N, int stride, int M, const CharsWork& wk,
                      float* d_char_quads, float* d_char_scores);
// chars_api.cpp: the two launches on heat-maps and boxes that an entry point has in HBM (boxes [N][cap][4][2], h_counts the
// host's per-page counts); the results go to ctx->last_ch, which the entry point's keep_det_scores validates.  Nothing happens
// with the switch off.
int chars_resident(kocr_ctx* ctx, const char* fn, const float* d_heat, int N, int h, int w, const float* d_boxes, int cap,
                   const int32_t* h_counts);

// tiles.hip: a page read in overlapping detector tiles ("Tiled pages"; kocr_tile_plan in include/kocr.h
// states the plan).  T = tile, O = overlap, S = T - 2 O the stride, ny x nx tiles (nT of them, row-major) over a canvas of
// Hc x Wc detector-input pixels.
struct TilePlan {
  int T, O, S, ny, nx, Hc, Wc, nT;
};
// The plan of an H x W page, or KOCR_EINVAL naming the refused argument (`fn`: the entry point)
int tile_plan(kocr_ctx* ctx, const char* fn, int H, int W, int tile, int overlap, TilePlan& p);
int launch_tile_gather(kocr_ctx* ctx, const uint8_t* d_canvas, int N, const TilePlan& p, uint8_t* d_tiles);
int launch_heat_stitch(kocr_ctx* ctx, const float* d_tile_heat, int N, const TilePlan& p, float* d_heat);

// imgproc.hip
int launch_resize_pad_f32(kocr_ctx* ctx, const float* d_src, int n, int sh, int sw, int C, float* d_dst, int dh, int dw, int Hmax,
                          int Wmax, float cval, Arena& tab_arena);
int launch_warp_f32(kocr_ctx* ctx, const float* d_img, int H, int W, int C, const WarpParam* d_prm, int M, int th, int tw, float* d_crops);
int launch_resize_pad(kocr_ctx* ctx, const uint8_t* d_src, int n, int sh, int sw, uint8_t* d_dst, int dh, int dw,
                      int Hmax, int Wmax, int cval, Arena& tab_arena);
