// chars.hip — the characters of word boxes read off the detector's region map (kocr_char_boxes; the reference has no
// counterpart).  The rule is tests/chars_statement.py ("Characters"): every float64 operation below is
// one of the statement's, in its order; this file is compiled with -ffp-contract=off so that none is fused.
#include "common.h"

namespace {

constexpr int CH_THREADS = 64;  // one wave per word: a word of w heat-map pixels has w columns, rarely more than 64
constexpr int CH_PACK_THREADS = 256;

__device__ inline double ch_length(double dx, double dy) { return __dsqrt_rn(dx * dx + dy * dy); }
__device__ inline double ch_lerp(double p, double q, double t) { return p + (q - p) * t; }

// statement: half_quad
struct ChQuad {
  double tlx, tly, trx, try_, brx, bry, blx, bly;
};

// word m of the batch: its page (off[page] <= m < off[page + 1]; empty pages are stepped over) and its quad -- packed word
// order with stride == 0, else page-major rows of `stride` quads (the resident boxes of kocr_get_boxes and its kin)
__device__ inline int ch_page_of(const int32_t* __restrict__ off, int N, int m) {
  int lo = 0, hi = N;  // the first page whose end lies beyond m
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid + 1] > m)
      hi = mid;
    else
      lo = mid + 1;
  }
  return min(lo, N - 1);  // off[N] == M: reached by no word
}

__device__ inline ChQuad ch_quad(const float* __restrict__ quads, const int32_t* __restrict__ off, int stride, int page, int m) {
  const size_t at = stride ? (size_t)page * stride + (m - off[page]) : (size_t)m;
  const float4 q01 = ((const float4*)quads)[2 * at], q23 = ((const float4*)quads)[2 * at + 1];
  ChQuad q;
  q.tlx = (double)q01.x / 2.0;
  q.tly = (double)q01.y / 2.0;
  q.trx = (double)q01.z / 2.0;
  q.try_ = (double)q01.w / 2.0;
  q.brx = (double)q23.x / 2.0;
  q.bry = (double)q23.y / 2.0;
  q.blx = (double)q23.z / 2.0;
  q.bly = (double)q23.w / 2.0;
  return q;
}

// statement: sample.  T is the page's heat-map, two interleaved channels; the text map is channel 0.
__device__ inline double ch_sample(const float* __restrict__ T, int h, int w, double px, double py) {
  const double x0 = floor(px), y0 = floor(py);
  if (!(x0 >= -1.0 && x0 <= (double)(w - 1) && y0 >= -1.0 && y0 <= (double)(h - 1))) return 0.0;
  const int ix = (int)x0, iy = (int)y0;
  const double fx = px - x0, fy = py - y0;
  const bool xa = ix >= 0, xb = ix + 1 < w, ya = iy >= 0, yb = iy + 1 < h;  // ix <= w - 1 and iy <= h - 1 already hold
  const size_t row0 = (size_t)(ya ? iy : 0) * w, row1 = (size_t)(yb ? iy + 1 : 0) * w;
  const size_t col0 = xa ? ix : 0, col1 = xb ? ix + 1 : 0;
  const double t00 = xa && ya ? (double)T[(row0 + col0) * 2] : 0.0;
  const double t01 = xb && ya ? (double)T[(row0 + col1) * 2] : 0.0;
  const double t10 = xa && yb ? (double)T[(row1 + col0) * 2] : 0.0;
  const double t11 = xb && yb ? (double)T[(row1 + col1) * 2] : 0.0;
  const double top = t00 + (t01 - t00) * fx;
  const double bottom = t10 + (t11 - t10) * fx;
  return top + (bottom - top) * fy;
}

}  // namespace

// One workgroup of one wave per word.  Phases, a __syncthreads between them:
//   profile   the columns spread over the lanes, a loop over the rows: the statement's profile into LDS
//   split     lane 0: the statement's split, one pass from the left over at most KOCR_CHARS_MAX_COLS columns in LDS; count,
//             column bounds and peak values go to the word's workspace rows
__global__ __launch_bounds__(CH_THREADS) void chars_split_kernel(const float* __restrict__ heat, int N, int h, int w,
                                                                  const float* __restrict__ quads, const int32_t* __restrict__ off,
                                                                  int stride, double peak_threshold, double valley_ratio,
                                                                  double extent_threshold, int32_t* __restrict__ counts,
                                                                  int32_t* __restrict__ ncols, uint16_t* __restrict__ bounds,
                                                                  float* __restrict__ peak_scores) {
  __shared__ double prof[KOCR_CHARS_MAX_COLS];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int page = ch_page_of(off, N, m);
  const ChQuad q = ch_quad(quads, off, stride, page, m);
  // statement: grid
  const double wq = (ch_length(q.trx - q.tlx, q.try_ - q.tly) + ch_length(q.brx - q.blx, q.bry - q.bly)) * 0.5;
  const double hq = (ch_length(q.blx - q.tlx, q.bly - q.tly) + ch_length(q.brx - q.trx, q.bry - q.try_)) * 0.5;
  if (!(wq > 0.0) || !(hq > 0.0)) {
    if (tid == 0) {
      counts[m] = 0;
      ncols[m] = 1;
    }
    return;
  }
  const int n_cols = (int)fmin((double)KOCR_CHARS_MAX_COLS, fmax(1.0, ceil(wq)));
  const int n_rows = (int)fmin((double)KOCR_CHARS_MAX_ROWS, fmax(1.0, ceil(hq)));
  const float* T = heat + (size_t)page * h * w * 2;

  // profile
  for (int i = tid; i < n_cols; i += CH_THREADS) {
    const double u = ((double)i + 0.5) / (double)n_cols;
    const double ax = ch_lerp(q.tlx, q.trx, u), ay = ch_lerp(q.tly, q.try_, u);
    const double bx = ch_lerp(q.blx, q.brx, u), by = ch_lerp(q.bly, q.bry, u);
    double best = 0.0;
    for (int j = 0; j < n_rows; ++j) {
      const double v = ((double)j + 0.5) / (double)n_rows;
      const double s = ch_sample(T, h, w, ch_lerp(ax, bx, v), ch_lerp(ay, by, v));
      if (j == 0 || s > best) best = s;
    }
    prof[i] = best;
  }
  __syncthreads();
  if (tid != 0) return;

  // split
  int first = -1, last = -1;
  for (int i = 0; i < n_cols; ++i)
    if (prof[i] >= extent_threshold) {
      if (first < 0) first = i;
      last = i;
    }
  uint16_t* wb = bounds + (size_t)m * KOCR_CHARS_BOUNDS_STRIDE;
  float* ws = peak_scores + (size_t)m * KOCR_CHARS_MAX_PER_WORD;
  int k = 0;  // characters emitted; two neighbouring columns are never both candidates, so k <= KOCR_CHARS_MAX_PER_WORD
  if (first >= 0) {
    int c = -1, low_at = -1;
    double low = 0.0, at_c = 0.0;
    double left = first > 0 ? prof[first - 1] : -1.0, here = prof[first];
    for (int i = first; i <= last; ++i) {
      const double right = i + 1 < n_cols ? prof[i + 1] : -1.0;
      if (c >= 0 && here < low) {
        low = here;
        low_at = i;
      }
      if (here >= peak_threshold && here > left && here >= right) {
        bool take = false;
        if (c < 0) {
          take = true;
        } else if (low <= valley_ratio * fmin(at_c, here)) {
          if (k < KOCR_CHARS_MAX_PER_WORD) {
            ws[k] = (float)at_c;
            wb[k + 1] = (uint16_t)low_at;
            ++k;
          }
          take = true;
        } else if (here > at_c) {
          take = true;
        }
        if (take) {
          c = i;
          at_c = here;
          low = here;
          low_at = i;
        }
      }
      left = here;
      here = right;
    }
    if (c >= 0 && k < KOCR_CHARS_MAX_PER_WORD) {
      ws[k] = (float)at_c;
      wb[0] = (uint16_t)first;
      wb[k + 1] = (uint16_t)(last + 1);
      ++k;
    } else {
      k = 0;
    }
  }
  counts[m] = k;
  ncols[m] = n_cols;
}

// The characters of all words in word order.  A block takes CH_PACK_THREADS consecutive words: the exclusive scan of the
// counts -- the characters before the block's first word summed in a fixed order, then a scan of the block's own counts in
// LDS -- and then one character per lane: its word by bisection of the scan, its quad from the word's quad and bounds
// (statement: word_chars).
__global__ __launch_bounds__(CH_PACK_THREADS) void chars_pack_kernel(const float* __restrict__ quads, const int32_t* __restrict__ off, int N,
                                                                      int stride, int M, const int32_t* __restrict__ counts,
                                                                      const int32_t* __restrict__ ncols, const uint16_t* __restrict__ bounds,
                                                                      const float* __restrict__ peak_scores, float* __restrict__ char_quads,
                                                                      float* __restrict__ char_scores) {
  __shared__ long long before[CH_PACK_THREADS];
  __shared__ int scan[CH_PACK_THREADS];
  const int tid = threadIdx.x, word0 = blockIdx.x * CH_PACK_THREADS;
  long long part = 0;
  for (int j = tid; j < word0; j += CH_PACK_THREADS) part += counts[j];
  before[tid] = part;
  const int own = word0 + tid < M ? counts[word0 + tid] : 0;
  scan[tid] = own;
  __syncthreads();
  for (int step = CH_PACK_THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) before[tid] += before[tid + step];
    __syncthreads();
  }
  for (int step = 1; step < CH_PACK_THREADS; step <<= 1) {  // inclusive scan
    const int add = tid >= step ? scan[tid - step] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const long long base = before[0];
  const int chars = scan[CH_PACK_THREADS - 1];
  for (int ch = tid; ch < chars; ch += CH_PACK_THREADS) {
    int lo = 0, hi = CH_PACK_THREADS - 1;  // the first word whose inclusive sum lies beyond ch
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (scan[mid] > ch)
        hi = mid;
      else
        lo = mid + 1;
    }
    const int m = word0 + lo;
    const int k = ch - (lo ? scan[lo - 1] : 0);
    const int page = ch_page_of(off, N, m);
    const ChQuad q = ch_quad(quads, off, stride, page, m);
    const double n_cols = (double)ncols[m];
    const uint16_t* wb = bounds + (size_t)m * KOCR_CHARS_BOUNDS_STRIDE;
    const double u0 = (double)wb[k] / n_cols, u1 = (double)wb[k + 1] / n_cols;
    float4* dst = (float4*)char_quads + (size_t)(base + ch) * 2;
    dst[0] = make_float4((float)(ch_lerp(q.tlx, q.trx, u0) * 2.0), (float)(ch_lerp(q.tly, q.try_, u0) * 2.0),
                         (float)(ch_lerp(q.tlx, q.trx, u1) * 2.0), (float)(ch_lerp(q.tly, q.try_, u1) * 2.0));
    dst[1] = make_float4((float)(ch_lerp(q.blx, q.brx, u1) * 2.0), (float)(ch_lerp(q.bly, q.bry, u1) * 2.0),
                         (float)(ch_lerp(q.blx, q.brx, u0) * 2.0), (float)(ch_lerp(q.bly, q.bry, u0) * 2.0));
    char_scores[base + ch] = peak_scores[(size_t)m * KOCR_CHARS_MAX_PER_WORD + k];
  }
}

size_t chars_workspace_bytes(int N, long M) {
  const size_t m = (size_t)M;
  return ((size_t)N + 1) * sizeof(int32_t) + 2 * m * sizeof(int32_t) + m * KOCR_CHARS_BOUNDS_STRIDE * sizeof(uint16_t) +
         m * KOCR_CHARS_MAX_PER_WORD * sizeof(float) + 5 * 256;
}

int launch_chars_split(kocr_ctx* ctx, const float* d_heat, int N, int h, int w, const float* d_quads, const int32_t* d_off, int stride,
                       int M, const CharsRule& rule, const CharsWork& wk) {
  if (M == 0) return KOCR_OK;
  ProfScope ps(ctx, "chars_split", 0, 0);
  hipLaunchKernelGGL(chars_split_kernel, dim3(M), dim3(CH_THREADS), 0, ctx->stream, d_heat, N, h, w, d_quads, d_off, stride,
                     rule.peak_threshold, rule.valley_ratio, rule.extent_threshold, wk.counts, wk.ncols, wk.bounds, wk.scores);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

int launch_chars_pack(kocr_ctx* ctx, const float* d_quads, const int32_t* d_off, int N, int stride, int M, const CharsWork& wk,
                      float* d_char_quads, float* d_char_scores) {
  if (M == 0) return KOCR_OK;
  ProfScope ps(ctx, "chars_pack", 0, 0);
  hipLaunchKernelGGL(chars_pack_kernel, dim3((M + CH_PACK_THREADS - 1) / CH_PACK_THREADS), dim3(CH_PACK_THREADS), 0, ctx->stream, d_quads,
                     d_off, N, stride, M, wk.counts, wk.ncols, wk.bounds, wk.scores, d_char_quads, d_char_scores);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}
