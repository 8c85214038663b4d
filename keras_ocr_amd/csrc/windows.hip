// windows.hip — long words: a box too wide for one crop read in overlapping windows (include/kocr_windows.h states the rule;
// DESIGN.md section 4, "Long words"; in numpy: tests/windows_statement.py).
//
// The rule is written ONCE, as the host/device functions below (the way warp_geom.h holds the crop set-up; float64, fixed
// operation order, -ffp-contract=off): the host runs them on the caller's boxes to size the call and to refuse it before any
// launch, the device runs them to make the plan.
//   window_count_kernel   one thread per box: K and T'
//   window_scan_kernel    one workgroup: the exclusive prefix sums of K (crop offsets) and of T' (row offsets), int64
//   window_plan_kernel    one thread per window: its source quad q_k, the WarpParam of that quad (warp_prepare_quad, the set-up
//                         every crop gets) and its record (word, lo, hi, first row); status by atomicMax as warp_prepare_kernel
//   window_stitch_kernel  one workgroup per window: its kept logit rows, one contiguous run of (hi - lo) C floats, into the
//                         word's sequence -- copied, never recomputed
// launch_warp makes the crops from the plan's WarpParams, the recogniser reads them in its usual batches, and
// ctc_scores_ragged_kernel (crnn_kernels.hip, beside the ctc_loss_wave it shares with ctc_scores_kernel) decodes the sequences.
// The entry points of include/kocr_windows.h are at the end of the file.
#include "abi.h"
#include "warp_geom.h"
#include <cfloat>
#include <climits>

#define HD __host__ __device__

namespace {

constexpr int WIN_T = CRNN_STEPS;  // frames per crop, 4 crop pixels each

// aspect finite and >= 200 / 31, overlap a multiple of 8 in [16, 96], 0 <= d < 50 - overlap / 8
HD bool window_args_ok(double aspect, int overlap, int discard) {
  if (!(aspect >= (double)CRNN_CROP_W / (double)CRNN_CROP_H) || !(aspect <= DBL_MAX)) return false;
  if (overlap < 16 || overlap > 96 || overlap % 8 != 0) return false;
  return discard >= 0 && discard < WIN_T - overlap / 8;
}

// get_rotated_width_height of an ordered box: warp_prepare_quad's own two expressions
HD void window_wh(const float* ob, int* w, int* h) {
  *w = (int)((dist2(ob + 0, ob + 2) + dist2(ob + 4, ob + 6)) / 2);
  *h = (int)((dist2(ob + 0, ob + 6) + dist2(ob + 2, ob + 4)) / 2);
}

// K of a box of w x h (both positive): 1 unless (double)w > A (double)h, else ceil((31 w - 200 h) / (S h)) + 1
HD long long window_count(int w, int h, double aspect, int overlap) {
  if (!((double)w > aspect * (double)h)) return 1;
  const long long S = CRNN_CROP_W - overlap;
  const long long num = (long long)CRNN_CROP_H * w - (long long)CRNN_CROP_W * h, den = S * h;
  if (num <= 0) return 1;  // aspect * h rounded below 200 h / 31: one window holds the box
  return (num + den - 1) / den + 1;
}

// T' of a word of K windows
HD long long window_frames(long long K, int overlap, int discard) {
  return (K - 1) * ((CRNN_CROP_W - overlap) / 4) + WIN_T - discard;
}

// window k of K: the frames [lo, hi) kept of its crop and the row of the word's sequence that frame lo goes to
HD void window_range(long long k, long long K, int overlap, int discard, int* lo, int* hi, long long* first) {
  const int f = overlap / 8;
  *lo = k == 0 ? discard : f;
  *hi = k == K - 1 ? WIN_T : WIN_T - f;
  *first = k == 0 ? 0 : (long long)(WIN_T - f - discard) + (k - 1) * (WIN_T - 2 * f);
}

// the point at fraction a of the edge p -> q, one component
HD float window_edge(float p, float q, double a) {
  if (a == 0.0) return p;
  if (a == 1.0) return q;
  return (float)((double)p + ((double)q - (double)p) * a);
}

// q_k of a LONG box: ob = [tl, tr, br, bl] cut at the fractions [a_k, b_k] of its top and bottom edges
HD void window_quad(const float* ob, int w, int h, long long k, int overlap, float* q) {
  const long long S = CRNN_CROP_W - overlap;
  const double den = (double)((long long)CRNN_CROP_H * w);
  const double a = (double)(k * S * h) / den;
  double b = (double)((k * S + CRNN_CROP_W) * h) / den;
  if (b > 1.0) b = 1.0;
  for (int c = 0; c < 2; ++c) {
    q[0 + c] = window_edge(ob[0 + c], ob[2 + c], a);  // top(a)
    q[2 + c] = window_edge(ob[0 + c], ob[2 + c], b);  // top(b)
    q[4 + c] = window_edge(ob[6 + c], ob[4 + c], b);  // bottom(b)
    q[6 + c] = window_edge(ob[6 + c], ob[4 + c], a);  // bottom(a)
  }
}

// One box: its ordered box, K and T'.  rc 1: zero width or height (K = 1, T' as one window's, so that the slot stays harmless).
HD int window_box(const float* box, double aspect, int overlap, int discard, float* ob, int* w, int* h, long long* K, long long* T,
                  BoxWork& wk) {
  rotated_box(box, ob, wk);
  window_wh(ob, w, h);
  const bool zero = *w == 0 || *h == 0;
  *K = zero ? 1 : window_count(*w, *h, aspect, overlap);
  *T = window_frames(*K, overlap, discard);
  return zero ? 1 : 0;
}

HD int window_box(const float* box, double aspect, int overlap, int discard, float* ob, int* w, int* h, long long* K, long long* T) {
  BoxWork wk;
  return window_box(box, aspect, overlap, discard, ob, w, h, K, T, wk);
}

constexpr int PLAN_THREADS = 64;  // lanes of a plan workgroup: each has its slice of LDS for the set-up's arrays

}  // namespace

// The arrays get_rotated_box indexes at run time (the hull) lie in a per-lane LDS slice, 592 bytes a lane: no scratch.
__global__ __launch_bounds__(PLAN_THREADS) void window_count_kernel(const float* __restrict__ boxes, int M, double aspect, int overlap, int discard, int* __restrict__ Kn,
                                    int* __restrict__ Tn, float* __restrict__ obs, int* __restrict__ status) {
  __shared__ BoxWork work[PLAN_THREADS];
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;  // no barrier below
  float ob[8];
  int w, h;
  long long K, T;
  const int rc = window_box(boxes + (size_t)m * 8, aspect, overlap, discard, ob, &w, &h, &K, &T, work[threadIdx.x]);
  for (int j = 0; j < 8; ++j) obs[(size_t)m * 8 + j] = ob[j];
  if (rc != 0) atomicMax(status, rc);
  // the host has refused every call with a T' beyond KOCR_WINDOW_FRAMES_MAX; the clamp keeps the buffers' sizes whatever comes
  const long long Kmax = (KOCR_WINDOW_FRAMES_MAX - (WIN_T - discard)) / ((CRNN_CROP_W - overlap) / 4) + 1;
  if (K > Kmax) {
    K = Kmax;
    T = window_frames(K, overlap, discard);
  }
  Kn[m] = (int)K;
  Tn[m] = (int)T;
}

constexpr int SCAN_THREADS = 256;

// woff / roff [M + 1]: exclusive prefix sums of Kn / Tn.  Each thread owns a contiguous run of boxes; thread 0 scans the runs' sums.
__global__ __launch_bounds__(SCAN_THREADS) void window_scan_kernel(const int* __restrict__ Kn, const int* __restrict__ Tn, int M,
                                                                   long long* __restrict__ woff, long long* __restrict__ roff) {
  __shared__ long long sk[SCAN_THREADS], st[SCAN_THREADS];
  const int per = (M + SCAN_THREADS - 1) / SCAN_THREADS;
  const long b0 = (long)threadIdx.x * per;
  const int b = (int)(b0 < M ? b0 : M), e = (int)(b0 + per < M ? b0 + per : M);
  long long ak = 0, at = 0;
  for (int i = b; i < e; ++i) {
    ak += Kn[i];
    at += Tn[i];
  }
  sk[threadIdx.x] = ak;
  st[threadIdx.x] = at;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long rk = 0, rt = 0;
    for (int i = 0; i < SCAN_THREADS; ++i) {
      const long long vk = sk[i], vt = st[i];
      sk[i] = rk;
      st[i] = rt;
      rk += vk;
      rt += vt;
    }
    woff[M] = rk;
    roff[M] = rt;
  }
  __syncthreads();
  ak = sk[threadIdx.x];
  at = st[threadIdx.x];
  for (int i = b; i < e; ++i) {
    woff[i] = ak;
    roff[i] = at;
    ak += Kn[i];
    at += Tn[i];
  }
}

// One thread per window i < total: its word m is the last one with woff[m] <= i, k = i - woff[m].  obs: the ordered boxes
// window_count_kernel left.  The 8 x 8 system of the homography lies in a per-lane LDS slice, 640 bytes a lane: no scratch.
__global__ __launch_bounds__(PLAN_THREADS) void window_plan_kernel(const float* __restrict__ obs, const int* __restrict__ img_of, int M, double aspect, int overlap,
                                   int discard, long total, const int* __restrict__ Kn, const long long* __restrict__ woff,
                                   const long long* __restrict__ roff, WarpParam* __restrict__ prm, float* __restrict__ quads,
                                   WindowRec* __restrict__ rec, int* __restrict__ status) {
  __shared__ SolveWork work[PLAN_THREADS];
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total || i >= woff[M]) return;  // no barrier below
  int lo = 0, hi = M;
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (woff[mid] <= i) lo = mid; else hi = mid;
  }
  const int m = lo;
  const long long k = i - woff[m], K = Kn[m];
  float ob[8], q[8];
  int w, h;
  for (int j = 0; j < 8; ++j) ob[j] = obs[(size_t)m * 8 + j];
  window_wh(ob, &w, &h);
  int rc = (w == 0 || h == 0) ? 1 : 0;
  if (rc == 0 && K > 1) window_quad(ob, w, h, k, overlap, q);
  else
    for (int j = 0; j < 8; ++j) q[j] = ob[j];
  WarpParam p;
  if (rc == 0) rc = warp_prepare_quad(q, CRNN_CROP_H, CRNN_CROP_W, &p, work[threadIdx.x]);
  if (rc != 0) {
    // keep the slot harmless: an empty crop
    for (int j = 0; j < 9; ++j) p.mi[j] = 0.0;
    p.cw = p.ch = 0;
    p.pad = 0;
    atomicMax(status, rc);
  }
  p.img = img_of[m];
  prm[i] = p;
  for (int j = 0; j < 8; ++j) quads[(size_t)i * 8 + j] = q[j];
  WindowRec r;
  long long first;
  window_range(k, K, overlap, discard, &r.lo, &r.hi, &first);
  r.word = m;
  r.pad = 0;
  r.row = roff[m] + first;
  rec[i] = r;
}

int launch_window_plan(kocr_ctx* ctx, const float* d_boxes, const int* d_img_of, int M, double aspect, int overlap, int discard,
                       long total, int* d_K, int* d_T, float* d_ob, long long* d_woff, long long* d_roff, WarpParam* d_prm,
                       float* d_quads, WindowRec* d_rec, int* d_status) {
  if (M <= 0) return KOCR_OK;
  ProfScope ps(ctx, "window_plan", 0, (double)M * 48.0 + (double)total * (sizeof(WarpParam) + 32.0 + sizeof(WindowRec)));
  hipLaunchKernelGGL(window_count_kernel, dim3((M + PLAN_THREADS - 1) / PLAN_THREADS), dim3(PLAN_THREADS), 0, ctx->stream, d_boxes, M,
                     aspect, overlap, discard, d_K, d_T, d_ob, d_status);
  hipLaunchKernelGGL(window_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, d_K, d_T, M, d_woff, d_roff);
  hipLaunchKernelGGL(window_plan_kernel, dim3((unsigned)((total + PLAN_THREADS - 1) / PLAN_THREADS)), dim3(PLAN_THREADS), 0, ctx->stream,
                     d_ob, d_img_of, M, aspect, overlap, discard, total, d_K, d_woff, d_roff, d_prm, d_quads, d_rec, d_status);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// Window blockIdx.x of the launch: rows [lo, hi) of its logits [50][C] are ONE run of (hi - lo) C floats, and so is their place
// in the sequence buffer.  16-byte accesses when both runs start on a 16-byte boundary (always so when C is a multiple of 4:
// both buffers are 256-byte aligned) and for the whole multiples of 4 floats; scalar accesses otherwise and for the tail.
__global__ __launch_bounds__(256) void window_stitch_kernel(const float* __restrict__ logits, const WindowRec* __restrict__ rec, int C,
                                                            float* __restrict__ seq) {
  const WindowRec r = rec[blockIdx.x];
  const int lo = min(max(r.lo, 0), WIN_T), hi = min(max(r.hi, lo), WIN_T);
  const size_t n = (size_t)(hi - lo) * C;
  const float* src = logits + ((size_t)blockIdx.x * WIN_T + lo) * C;
  float* dst = seq + (size_t)r.row * C;
  size_t done = 0;
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const size_t n4 = n / 4;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (size_t i = threadIdx.x; i < n4; i += blockDim.x) d4[i] = s4[i];
    done = n4 * 4;
  }
  for (size_t i = done + threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

int launch_window_stitch(kocr_ctx* ctx, const float* d_logits, const WindowRec* d_rec, int n, int C, float* d_seq) {
  if (n <= 0) return KOCR_OK;
  ProfScope ps(ctx, "window_stitch", 0, (double)n * WIN_T * C * 8.0);
  hipLaunchKernelGGL(window_stitch_kernel, dim3(n), dim3(256), 0, ctx->stream, d_logits, d_rec, C, d_seq);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// entry points (include/kocr_windows.h)
// ---------------------------------------------------------------------------------------------------------------------
namespace {

// what the host learns of a call from its boxes (or, for the decode seam, from its window counts) before anything is launched
struct WindowSizes {
  std::vector<int32_t> K, T;  // per word
  long total = 0, rows = 0;   // sum K, sum T'
  int Lmax = 0;               // the longest T'
};

int window_refusal(kocr_ctx* ctx, const char* fn, double aspect, int overlap) {
  const std::string f(fn);
  const char* why = nullptr;
  if (ctx->beam_width) why = "a beam (kocr_set_beam)";
  else if (ctx->lex_top) why = "a lexicon match (kocr_set_lexicon_match)";
  else if (ctx->charset >= 0) why = "a character set (kocr_set_charset)";
  else if (ctx->pattern >= 0) why = "a pattern (kocr_set_pattern)";
  else if (ctx->orient_mode != KOCR_ORIENT_OFF) why = "orientation (kocr_set_orientation)";
  else if (ctx->chars_on) why = "character boxes (kocr_set_char_boxes)";
  if (why) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": long words (windowed reading) cannot be combined with " + why);
  const int d = WIN_T - crnn_label_width(ctx);
  if (!window_args_ok(aspect, overlap, 0))
    KOCR_FAIL(ctx, KOCR_EINVAL, f + ": aspect must be finite and >= 200 / 31, overlap a multiple of 8 in [16, 96] (got aspect " +
                                    std::to_string(aspect) + ", overlap " + std::to_string(overlap) + ")");
  if (!window_args_ok(aspect, overlap, d))
    KOCR_FAIL(ctx, KOCR_EINVAL, f + ": rnn_steps_to_discard " + std::to_string(d) + " leaves no frame of the first window at overlap " +
                                    std::to_string(overlap) + " (it must be below 50 - overlap / 8 = " + std::to_string(WIN_T - overlap / 8) + ")");
  return KOCR_OK;
}

int window_cap_error(kocr_ctx* ctx, const char* fn, int image, long box, long long K, long long T) {
  KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": box " + std::to_string(box) + " of image " + std::to_string(image) + " takes " +
                                  std::to_string(K) + " windows and " + std::to_string(T) + " frames, more than KOCR_WINDOW_FRAMES_MAX = " +
                                  std::to_string(KOCR_WINDOW_FRAMES_MAX) + " (raise aspect or split the box)");
}

// The sizes of the boxes [M][4][2] of N images (counts; image-major), img_of [M] the image of every box.  Refusals before any
// launch: a zero width or height KOCR_EZERODIV, a T' beyond the cap KOCR_EINVAL naming image and box.
int window_sizes(kocr_ctx* ctx, const char* fn, int N, const float* boxes, const int32_t* counts, double aspect, int overlap,
                 WindowSizes& z, std::vector<int32_t>& img_of) {
  const int d = WIN_T - crnn_label_width(ctx);
  long m = 0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < counts[i]; ++j, ++m) {
      float ob[8];
      int w, h;
      long long K, T;
      KOCR_TRY(warp_status_error(ctx, fn, window_box(boxes + m * 8, aspect, overlap, d, ob, &w, &h, &K, &T)));
      if (T > KOCR_WINDOW_FRAMES_MAX) return window_cap_error(ctx, fn, i, j, K, T);
      z.K.push_back((int32_t)K);
      z.T.push_back((int32_t)T);
      img_of.push_back(i);
      z.total += (long)K;
      z.rows += (long)T;
      z.Lmax = std::max(z.Lmax, (int)T);
      if (z.total > INT32_MAX / 2)  // crop counts, grids and *n_windows are 32-bit
        KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": more than " + std::to_string(INT32_MAX / 2) + " windows in one call");
    }
  return KOCR_OK;
}

long window_words(kocr_ctx* ctx, const char* fn, int N, const int32_t* counts) {
  long M = 0;
  for (int i = 0; i < N; ++i) {
    if (counts[i] < 0) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": negative count");
    M += counts[i];
  }
  if (M > INT32_MAX / 64) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": too many boxes");
  return M;
}

// the device buffers of a plan over M words and `total` windows
struct WindowPlanBufs {
  long M = 0, total = 0;
  float* boxes = nullptr;
  int32_t* img_of = nullptr;
  int32_t *K = nullptr, *T = nullptr;
  float* ob = nullptr;  // [M][8] the ordered boxes, from the count kernel to the plan kernel
  long long *woff = nullptr, *roff = nullptr;
  WarpParam* prm = nullptr;
  float* quads = nullptr;
  WindowRec* rec = nullptr;
  int* status = nullptr;
  template <class F> int each(F f) {
    const size_t m = (size_t)M, t = (size_t)total;
    KOCR_TRY(f(boxes, m * 8 * sizeof(float)));
    KOCR_TRY(f(img_of, m * sizeof(int32_t)));
    KOCR_TRY(f(K, m * sizeof(int32_t)));
    KOCR_TRY(f(T, m * sizeof(int32_t)));
    KOCR_TRY(f(ob, m * 8 * sizeof(float)));
    KOCR_TRY(f(woff, (m + 1) * sizeof(long long)));
    KOCR_TRY(f(roff, (m + 1) * sizeof(long long)));
    KOCR_TRY(f(prm, t * sizeof(WarpParam)));
    KOCR_TRY(f(quads, t * 8 * sizeof(float)));
    KOCR_TRY(f(rec, t * sizeof(WindowRec)));
    return f(status, 256);
  }
};

// the plan on the device from the host's boxes; the host vectors must outlive the copies (the callers synchronise)
int window_plan_run(kocr_ctx* ctx, Staging& st, WindowPlanBufs& p, const float* boxes, const std::vector<int32_t>& img_of, long rows,
                    double aspect, int overlap) {
  KOCR_TRY(st.put(p.boxes, boxes, (size_t)p.M * 8 * sizeof(float)));
  KOCR_TRY(st.put(p.img_of, img_of.data(), (size_t)p.M * sizeof(int32_t)));
  KOCR_HIP(ctx, hipMemsetAsync(p.status, 0, sizeof(int), ctx->stream));
  KOCR_TRY(launch_window_plan(ctx, p.boxes, p.img_of, (int)p.M, aspect, overlap, WIN_T - crnn_label_width(ctx), p.total, p.K, p.T, p.ob,
                              p.woff, p.roff, p.prm, p.quads, p.rec, p.status));
  // The buffers behind the plan are sized from the host's run of the same functions: the device's totals must be the host's
  // before anything is written through the records (16 bytes and a synchronisation; the boxes are host arrays anyway).
  long long got[2] = {-1, -1};
  KOCR_HIP(ctx, hipMemcpyAsync(&got[0], p.woff + p.M, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipMemcpyAsync(&got[1], p.roff + p.M, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (got[0] != p.total || got[1] != rows)
    KOCR_FAIL(ctx, KOCR_EINVAL, std::string(st.fn) + ": the device's window plan (" + std::to_string(got[0]) + " windows, " +
                                    std::to_string(got[1]) + " frames) differs from the host's (" + std::to_string(p.total) + ", " +
                                    std::to_string(rows) + ")");
  return KOCR_OK;
}

// kocr_window_plan (img_rgb == nullptr: no crops) and kocr_warp_crops_windowed
int window_plan_call(kocr_ctx* ctx, const char* fn, const uint8_t* img_rgb, int N, int H, int W, const float* boxes, const int32_t* counts,
                     double aspect, int overlap, float* crops, int32_t* windows, float* quads, int32_t* ranges, int max_windows,
                     int32_t* n_windows) {
  const std::string f(fn);
  KOCR_TRY(window_refusal(ctx, fn, aspect, overlap));
  if (n_windows) *n_windows = 0;
  const long M = window_words(ctx, fn, N, counts);
  if (M < 0) return (int)M;
  if (M == 0) return KOCR_OK;
  if (!boxes || !windows) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null buffer");
  WindowSizes z;
  std::vector<int32_t> img_of;
  KOCR_TRY(window_sizes(ctx, fn, N, boxes, counts, aspect, overlap, z, img_of));
  for (long m = 0; m < M; ++m) windows[m] = z.K[m];
  if (n_windows) *n_windows = (int32_t)z.total;
  if (max_windows < z.total)
    KOCR_FAIL(ctx, KOCR_ECAPACITY, f + ": max_windows " + std::to_string(max_windows) + " is below the " + std::to_string(z.total) +
                                       " windows of the call");
  if (!quads || !ranges || (img_rgb && !crops)) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null buffer");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t ib = img_rgb ? (size_t)N * H * W * 3 : 0, cb = img_rgb ? (size_t)z.total * CRNN_CROP_PIXELS * sizeof(float) : 0;
  WindowPlanBufs p;
  p.M = M;
  p.total = z.total;
  Staging st{ctx, ctx->io, fn};
  KOCR_TRY(st.reserve(0, {ib, cb}, {staging_bytes(p)}));
  KOCR_TRY(staging_take(st, p));
  KOCR_TRY(window_plan_run(ctx, st, p, boxes, img_of, z.rows, aspect, overlap));
  float* d_crops = nullptr;
  if (img_rgb) {
    const uint8_t* d_img;
    KOCR_TRY(st.in(img_rgb, ib, d_img));
    KOCR_TRY(st.scratch(cb, d_crops));
    KOCR_TRY(launch_warp(ctx, d_img, H, W, p.prm, (int)z.total, CRNN_CROP_H, CRNN_CROP_W, d_crops));
    KOCR_TRY(st.download(crops, (const float*)d_crops, cb));
  }
  std::vector<WindowRec> rec((size_t)z.total);
  int status = 0;
  KOCR_TRY(st.download(windows, (const int32_t*)p.K, (size_t)M * sizeof(int32_t)));  // the device's counts
  KOCR_TRY(st.download(quads, (const float*)p.quads, (size_t)z.total * 8 * sizeof(float)));
  KOCR_TRY(st.download(rec.data(), (const WindowRec*)p.rec, rec.size() * sizeof(WindowRec)));
  KOCR_TRY(st.download(&status, (const int*)p.status, sizeof(int)));
  KOCR_TRY(st.finish());
  for (size_t i = 0; i < rec.size(); ++i) {
    ranges[2 * i] = rec[i].lo;
    ranges[2 * i + 1] = rec[i].hi;
  }
  return warp_status_error(ctx, fn, status);
}

}  // namespace

extern "C" int kocr_window_plan(kocr_ctx* ctx, int M, const float* boxes, double aspect, int overlap, int32_t* windows, float* quads,
                                int32_t* ranges, int max_windows, int32_t* n_windows) {
  if (!ctx) return KOCR_EINVAL;
  if (M < 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_window_plan: bad sizes");
  const int32_t counts[1] = {M};
  return window_plan_call(ctx, "kocr_window_plan", nullptr, 1, 0, 0, boxes, counts, aspect, overlap, nullptr, windows, quads, ranges,
                          max_windows, n_windows);
}

extern "C" int kocr_warp_crops_windowed(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                                        const int32_t* counts, double aspect, int overlap, float* crops, int32_t* windows, float* quads,
                                        int32_t* ranges, int max_windows, int32_t* n_windows) {
  if (!ctx) return KOCR_EINVAL;
  if (N < 0 || H <= 0 || W <= 0 || (N > 0 && (!img_rgb || !counts))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_warp_crops_windowed: bad argument");
  return window_plan_call(ctx, "kocr_warp_crops_windowed", img_rgb, N, H, W, boxes, counts, aspect, overlap, crops, windows, quads, ranges,
                          max_windows, n_windows);
}

// The decode seam: the records come from window_range on the host (there are no boxes here), the launches are the route's.
extern "C" int kocr_ctc_stitch_decode(kocr_ctx* ctx, const float* logits, int M, const int32_t* windows, int overlap, int32_t* labels,
                                      float* log_word, float* char_scores, int32_t* frames, int width) {
  if (!ctx) return KOCR_EINVAL;
  const char* fn = "kocr_ctc_stitch_decode";
  const std::string f(fn);
  KOCR_TRY(window_refusal(ctx, fn, (double)CRNN_CROP_W / (double)CRNN_CROP_H, overlap));
  const int C = crnn_classes(ctx), d = WIN_T - crnn_label_width(ctx);
  if (C == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, f + ": call kocr_load_crnn first");
  if (M < 0 || width < 0 || M > INT32_MAX / 64) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": bad sizes");
  if (M == 0) return KOCR_OK;
  if (!logits || !windows || !labels || !log_word || !char_scores || !frames) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null buffer");
  WindowSizes z;
  std::vector<long long> roff((size_t)M + 1, 0);
  for (int m = 0; m < M; ++m) {
    if (windows[m] < 1) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": word " + std::to_string(m) + " has " + std::to_string(windows[m]) + " windows");
    const long long T = window_frames(windows[m], overlap, d);
    if (T > KOCR_WINDOW_FRAMES_MAX) return window_cap_error(ctx, fn, 0, m, windows[m], T);
    z.K.push_back(windows[m]);
    z.T.push_back((int32_t)T);
    z.total += windows[m];
    roff[m] = z.rows;
    z.rows += (long)T;
    z.Lmax = std::max(z.Lmax, (int)T);
  }
  roff[M] = z.rows;
  for (int m = 0; m < M; ++m) frames[m] = z.T[m];
  if (width < z.Lmax)
    KOCR_FAIL(ctx, KOCR_ECAPACITY, f + ": width " + std::to_string(width) + " is below the longest sequence of the call, " +
                                       std::to_string(z.Lmax) + " frames");
  std::vector<WindowRec> rec;
  rec.reserve((size_t)z.total);
  for (int m = 0; m < M; ++m)
    for (int k = 0; k < z.K[m]; ++k) {
      WindowRec r;
      long long first;
      window_range(k, z.K[m], overlap, d, &r.lo, &r.hi, &first);
      r.word = m;
      r.pad = 0;
      r.row = roff[m] + first;
      rec.push_back(r);
    }
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t m = (size_t)M, lw = (size_t)z.Lmax, f4 = sizeof(float), i4 = sizeof(int32_t);
  const size_t lb = (size_t)z.total * WIN_T * C * f4, sb = (size_t)z.rows * C * f4, rb = rec.size() * sizeof(WindowRec);
  Staging st{ctx, ctx->io, fn};
  KOCR_TRY(st.reserve(0, {lb, rb, (m + 1) * sizeof(long long), m * i4, sb, m * lw * i4, m * f4, m * lw * f4}));
  const float* d_lg;
  const WindowRec* d_rec;
  const long long* d_roff;
  const int32_t* d_T;
  float *d_seq, *d_logw, *d_chars;
  int32_t* d_lab;
  KOCR_TRY(st.in(logits, lb, d_lg));
  KOCR_TRY(st.upload((const WindowRec*)rec.data(), rb, d_rec));
  KOCR_TRY(st.upload((const long long*)roff.data(), (m + 1) * sizeof(long long), d_roff));
  KOCR_TRY(st.upload((const int32_t*)z.T.data(), m * i4, d_T));
  KOCR_TRY(st.scratch(sb, d_seq));
  KOCR_TRY(st.scratch(m * lw * i4, d_lab));
  KOCR_TRY(st.scratch(m * f4, d_logw));
  KOCR_TRY(st.scratch(m * lw * f4, d_chars));
  KOCR_TRY(launch_window_stitch(ctx, d_lg, d_rec, (int)z.total, C, d_seq));
  KOCR_TRY(launch_ctc_scores_ragged(ctx, d_seq, d_roff, d_T, M, C, z.Lmax, d_lab, d_logw, d_chars));
  for (size_t r = 0; r < m; ++r)
    for (size_t c = lw; c < (size_t)width; ++c) {
      labels[r * width + c] = -1;
      char_scores[r * width + c] = 0.f;
    }
  KOCR_HIP(ctx, hipMemcpy2DAsync(labels, (size_t)width * i4, d_lab, lw * i4, lw * i4, m, hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipMemcpy2DAsync(char_scores, (size_t)width * f4, d_chars, lw * f4, lw * f4, m, hipMemcpyDeviceToHost, ctx->stream));
  KOCR_TRY(st.download(log_word, (const float*)d_logw, m * f4));
  return st.finish();  // also: the host vectors' copies are done
}

// The whole route: plan, crops, the recogniser up to fc_12 batch by batch with every batch's windows stitched into the
// sequence buffer before the workspace is reused, then one ragged decode.  The rows stay in the io arena (ctx->last_win).
extern "C" int kocr_recognize_boxes_windowed(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                                             const int32_t* counts, double aspect, int overlap, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  const char* fn = "kocr_recognize_boxes_windowed";
  const std::string f(fn);
  if (N < 0 || (N > 0 && (!img_rgb || !counts || H <= 0 || W <= 0))) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": bad argument");
  const int C = crnn_classes(ctx);
  if (C == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, f + ": call kocr_load_crnn first");
  KOCR_TRY(window_refusal(ctx, fn, aspect, overlap));
  const long M = window_words(ctx, fn, N, counts);
  if (M < 0) return (int)M;
  if (M == 0) {
    ctx->invalidate_results();
    ctx->last_win = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, crnn_label_width(ctx), Resident::VALID};
    return KOCR_OK;
  }
  if (!boxes) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null buffer");
  WindowSizes z;
  std::vector<int32_t> img_of;
  KOCR_TRY(window_sizes(ctx, fn, N, boxes, counts, aspect, overlap, z, img_of));
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t m = (size_t)M, lw = (size_t)z.Lmax, f4 = sizeof(float), i4 = sizeof(int32_t);
  const size_t ib = (size_t)N * H * W * 3, cb = (size_t)z.total * CRNN_CROP_PIXELS * f4, sb = (size_t)z.rows * C * f4;
  WindowPlanBufs p;
  p.M = M;
  p.total = z.total;
  Staging st{ctx, ctx->io, fn, on_device != 0};
  KOCR_TRY(st.reserve(0, {ib}, {staging_bytes(p), cb, sb, m * lw * i4, m * f4, m * lw * f4}));
  KOCR_TRY(staging_take(st, p));
  float *d_crops, *d_seq, *d_logw, *d_chars;
  int32_t* d_lab;
  const uint8_t* d_img;
  KOCR_TRY(st.scratch(cb, d_crops));
  KOCR_TRY(st.scratch(sb, d_seq));
  KOCR_TRY(st.scratch(m * lw * i4, d_lab));
  KOCR_TRY(st.scratch(m * f4, d_logw));
  KOCR_TRY(st.scratch(m * lw * f4, d_chars));
  KOCR_TRY(st.in(img_rgb, ib, d_img));
  KOCR_TRY(window_plan_run(ctx, st, p, boxes, img_of, z.rows, aspect, overlap));
  KOCR_TRY(launch_warp(ctx, d_img, H, W, p.prm, (int)z.total, CRNN_CROP_H, CRNN_CROP_W, d_crops));
  KOCR_TRY(ctx->ws_reserve(crnn_workspace_bytes(crnn_batch(z.total), C)));
  // The recogniser's usual batches of at most CRNN_BATCH crops, with one difference: a last batch of fewer than `small` crops
  // behind a full one takes crops from it.  Below `small` crops (crnn_small_batch) the per-frame 1x1 layers leave conv_ds for the
  // fp32 MFMA kernel, whose sums round differently: without this the last windows of a call's last word would depend on
  // how many windows the boxes before it have.  A call of fewer than `small` crops is one batch, as in kocr_recognize_boxes.
  const long small = crnn_small_batch(ctx);
  for (long s = 0; s < z.total;) {
    long nb = std::min<long>(CRNN_BATCH, z.total - s);
    const long rest = z.total - s - nb;
    if (rest > 0 && rest < small) nb -= small - rest;
    ctx->ws_reset();
    const float* d_lg = nullptr;
    KOCR_TRY(crnn_logits(ctx, d_crops + (size_t)s * CRNN_CROP_PIXELS, (int)nb, &d_lg));
    KOCR_TRY(launch_window_stitch(ctx, d_lg, p.rec + s, (int)nb, C, d_seq));
    s += nb;
  }
  KOCR_TRY(launch_ctc_scores_ragged(ctx, d_seq, p.roff, p.T, (int)M, C, z.Lmax, d_lab, d_logw, d_chars));
  int status = 0;
  KOCR_TRY(st.download(&status, (const int*)p.status, sizeof(int)));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // also: the host vectors' copies are done
  KOCR_TRY(warp_status_error(ctx, fn, status));
  ctx->last_win = {d_lab, d_logw, d_chars, p.T, p.K, (int)M, z.Lmax, Resident::VALID};
  return KOCR_OK;
}

extern "C" int kocr_windowed_results_shape(kocr_ctx* ctx, int32_t* n_words, int32_t* width) {
  if (!ctx) return KOCR_EINVAL;
  if (ctx->last_win.state != Resident::VALID)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_windowed_results_shape: no windowed result is resident (call it right after kocr_recognize_boxes_windowed)");
  if (n_words) *n_words = ctx->last_win.M;
  if (width) *width = ctx->last_win.lw;
  return KOCR_OK;
}

extern "C" int kocr_windowed_results(kocr_ctx* ctx, int32_t* labels, float* log_word, float* char_scores, int32_t* frames,
                                     int32_t* windows, int max_words, int width) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_win;
  if (r.state != Resident::VALID)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_windowed_results: no windowed result is resident (call it right after kocr_recognize_boxes_windowed)");
  if (max_words < r.M || (r.M > 0 && width < r.lw))
    KOCR_FAIL(ctx, KOCR_ECAPACITY, "kocr_windowed_results: buffers smaller than the resident rows (max_words >= " + std::to_string(r.M) +
                                       ", width >= " + std::to_string(r.lw) + ")");
  if (r.M == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t m = (size_t)r.M, lw = (size_t)r.lw, wd = (size_t)width, f4 = sizeof(float), i4 = sizeof(int32_t);
  for (size_t row = 0; row < m; ++row)
    for (size_t c = lw; c < wd; ++c) {
      if (labels) labels[row * wd + c] = -1;
      if (char_scores) char_scores[row * wd + c] = 0.f;
    }
  if (labels) KOCR_HIP(ctx, hipMemcpy2DAsync(labels, wd * i4, r.d_labels, lw * i4, lw * i4, m, hipMemcpyDeviceToHost, ctx->stream));
  if (char_scores) KOCR_HIP(ctx, hipMemcpy2DAsync(char_scores, wd * f4, r.d_chars, lw * f4, lw * f4, m, hipMemcpyDeviceToHost, ctx->stream));
  if (log_word) KOCR_HIP(ctx, hipMemcpyAsync(log_word, r.d_logw, m * f4, hipMemcpyDeviceToHost, ctx->stream));
  if (frames) KOCR_HIP(ctx, hipMemcpyAsync(frames, r.d_frames, m * i4, hipMemcpyDeviceToHost, ctx->stream));
  if (windows) KOCR_HIP(ctx, hipMemcpyAsync(windows, r.d_windows, m * i4, hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}
