// taps.h — the launch recorder behind kocr_craft_set_taps / kocr_crnn_set_taps (test seam, include/kocr.h).
// A tapped launch enqueues, on ctx->stream, a device-to-host copy of the input view it reads and of its slots just
// before it, and of what it wrote (full and / or pooled output, with their slots) just after it -- LivePool and the
// workspace reuse every buffer, so nothing can be read back later.  Nothing else changes: no kernel, no launch order, no
// buffer; with taps off tapped() is the launch alone.
#pragma once
#include "common.h"

enum TapNet { TAPS_CRAFT = 0, TAPS_CRNN = 1 };

struct Taps {
  struct Part {
    int N = 0, H = 0, W = 0, C = 0;  // N = 0: not recorded
    std::vector<float> data;          // [N][H][W][C] of the whole call (every micro-batch)
    std::vector<float> amax;          // [N] slot values as floats, -1 = the tensor had no slots
  };
  struct Tap {
    std::string name;
    std::vector<std::string> rows;  // profiler rows of the launch (ProfScope)
    Part part[3];                   // input, full output, pooled output
  };
  TapNet net = TAPS_CRAFT;  // the forward whose launches are recorded (the other network's forward records nothing)
  bool all = false;
  std::vector<std::string> sel;
  std::vector<Tap> rec;  // launch order; reserved up front so that pointers into it stay valid during the call
  // images (crops) of the forward call, first image of its current micro-batch (-1: none running) and its image count
  int N = 0, n0 = -1, nb = 0;
  Tap* find(const std::string& nm) {
    for (Tap& t : rec)
      if (t.name == nm) return &t;
    return nullptr;
  }
};

// a forward call of `net` over N images starts: restart the record if taps of that network are on
int taps_begin(kocr_ctx* ctx, TapNet net, int N);
// ... its next micro-batch holds images n0 .. n0 + nb - 1 (n0 = -1: the call is over)
void taps_batch(kocr_ctx* ctx, TapNet net, int n0, int nb);
// the end of a forward call of `net`, also on an error return: no later launch records into this call's taps
struct TapsEnd {
  kocr_ctx* c;
  TapNet net;
  ~TapsEnd() { taps_batch(c, net, -1, 0); }
};
// before the launch of `name`: *out = nullptr if it is not tapped, else its record, the input copy enqueued
int tap_begin(kocr_ctx* ctx, const std::string& name, const Tensor* in, Taps::Tap** out);
// after it: what it wrote
int tap_end(kocr_ctx* ctx, Taps::Tap* t, const Tensor* full, const Tensor* pool);

// a launch with its taps: `in` as read, then `full` / `pool` as written.  A cell-grid tensor (Tensor::cellW) is recorded
// per image: image i's cell as [H][cellW][C], gutters included, with its cell's slot.
template <class Launch>
int tapped(kocr_ctx* ctx, const std::string& name, const Tensor* in, const Tensor* full, const Tensor* pool, Launch&& launch) {
  struct RowsOff {  // the launch's row collection ends with it, also when it fails
    kocr_ctx* c;
    ~RowsOff() { c->tap_rows = nullptr; }
  } rows_off{ctx};
  Taps::Tap* t = nullptr;
  KOCR_TRY(tap_begin(ctx, name, in, &t));
  KOCR_TRY(launch());
  return tap_end(ctx, t, full, pool);
}
