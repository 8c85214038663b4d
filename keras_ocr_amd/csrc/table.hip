// table.hip — the word boxes of one table put into rows, columns and spanning cells by the white space between them, on the
// device (kocr_group_lines with flags == KOCR_LINES_TABLE; the reference has no counterpart).  The rule is
// tests/table_statement.py ("Tables"): a gap is one float64 subtraction of two float32 values, a
// threshold one float64 product, the mean height one sum in ascending index; this file is compiled with -ffp-contract=off
// like lines.hip and blocks.hip.
#include "common.h"
#include <algorithm>

namespace {

constexpr int TB_MAX_THREADS = 1024;
static_assert(2 * TB_MAX_THREADS >= KOCR_LINES_MAX_WORDS, "a lane owns two quads of a page");

// The LDS of one page of at most `cap` quads (cap = 2 x the lanes of the block).  A SLOT is one white interval (a, b) or none
// (a == b == 0, which no comparison below counts).  Of the n + R slots of a page, slot x < n is quad x's: the gap in front of
// it in its row, or the row's left margin where x is the row's first by (x0, index); slot n + r is the right margin of row r.
// The slots that hold something lie close together, so the lanes of a wave have the same work or none.
struct TbPage {
  float *x0, *x1, *y0, *y1;  // [quad] the axis-aligned box
  int *vy;                   // [quad] 1: a valid gap along y lies in front of it, a row starts here
  int *row;                  // [quad]
  float *ia, *ib;            // [slot] the white interval
  int *flag;                 // [slot] TB_START: ia is where a run starts; TB_END: ib is where one ends; TB_SEP: that run is a separator
  float *ra;                 // [slot] for a TB_END slot: where its run starts
  float *sa, *sb;            // [separator] from the left
};
constexpr int TB_START = 1, TB_END = 2, TB_SEP = 4;
constexpr size_t TB_BYTES_PER_QUAD = 4 * sizeof(float) + 2 * sizeof(int) + 2 * (2 * sizeof(float) + sizeof(int) + sizeof(float)) + 2 * sizeof(float);
static_assert(TB_BYTES_PER_QUAD == 64, "the layout above");
static_assert((size_t)KOCR_LINES_MAX_WORDS * TB_BYTES_PER_QUAD + 1024 <= 160 * 1024, "a page of KOCR_LINES_MAX_WORDS quads must fit the 160 KB LDS of a CU");

struct TbShared {
  double tx, ty;
  int rows, separators;
};

// `first` before `second` in the order (key, index)
__device__ inline bool tb_before(float ka, int a, float kb, int b) { return ka < kb || (ka == kb && a < b); }

}  // namespace

// One workgroup per page, blockDim.x = cap / 2: lane t owns the quads t and t + blockDim.x and the slots t + k blockDim.x.  Every
// step is a count, a max or a min over the page that each lane takes for its own quads or slots in a loop whose reads are
// the same address in every lane (an LDS broadcast): nothing is sorted or scanned, and no result depends on which lane
// gets where first.
//   boxes       one quad per lane: x0, x1, y0, y1
//   rows        lane 0: the mean height in ascending index, tx and ty.  Every quad: the largest y1 of the quads before it by
//               (y0, index) and with it the gap in front of it; then its row, the valid gaps in front of it and of the quads
//               before it, counted
//   intervals   every quad over its row: the largest x1 of the quads before it by (x0, index) -> its interior gap; the row's
//               first quad also takes the row's extent -> both margins and the row band
//   runs        c just right of a value v is #{a <= v < b} over the white intervals, just left of it #{a < v <= b} (the white
//               intervals of one row do not overlap: rows and intervals count alike).  A run of c >= K starts at v where the
//               left count is below K and the right one is not; it can only start at some interval's a, and ends at some b.
//               Of equal values the smallest slot speaks.
//   separators  every run end finds its start, the largest start below it; the run is a separator when it is wide enough
//               and ends before X1; its number is the count of separators that end before it
//   cells       every quad: col0 = #{b_s <= x0}, col1 = max(col0, #{b_s < x1})
//   output      line_of = row, order = col0 | col1 << 16, counts = R + S + 1; the bands to `boxes` at TWICE the page's quad
//               offset (a page has at most 2 n bands), rows first, packed by lines_pack_kernel
__global__ __launch_bounds__(TB_MAX_THREADS) void table_grid_kernel(const float* __restrict__ quads, const int32_t* __restrict__ off, int cap,
                                                                     double min_gap_x, double min_gap_y, double min_support,
                                                                     int32_t* __restrict__ row_of, int32_t* __restrict__ cols,
                                                                     int32_t* __restrict__ band_counts, float* __restrict__ boxes) {
  extern __shared__ float tb_lds[];
  __shared__ TbShared sh;
  const int page = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int o = off[page];
  const int n = min(min(off[page + 1] - o, cap), 2 * T);  // the host has checked the offsets; nothing is written past `cap` whatever they say
  if (n <= 0) {
    if (tid == 0) band_counts[page] = 0;
    return;
  }
  TbPage s;
  s.x0 = tb_lds;
  s.x1 = s.x0 + cap;
  s.y0 = s.x1 + cap;
  s.y1 = s.y0 + cap;
  s.vy = (int*)(s.y1 + cap);
  s.row = s.vy + cap;
  s.ia = (float*)(s.row + cap);
  s.ib = s.ia + 2 * cap;
  s.flag = (int*)(s.ib + 2 * cap);
  s.ra = (float*)(s.flag + 2 * cap);
  s.sa = s.ra + 2 * cap;
  s.sb = s.sa + cap;
  const float4* q4 = (const float4*)quads + (size_t)o * 2;

  // boxes
  for (int x = tid; x < n; x += T) {
    const float4 q01 = q4[2 * x], q23 = q4[2 * x + 1];
    s.x0[x] = fminf(fminf(q01.x, q01.z), fminf(q23.x, q23.z));
    s.x1[x] = fmaxf(fmaxf(q01.x, q01.z), fmaxf(q23.x, q23.z));
    s.y0[x] = fminf(fminf(q01.y, q01.w), fminf(q23.y, q23.w));
    s.y1[x] = fmaxf(fmaxf(q01.y, q01.w), fmaxf(q23.y, q23.w));
  }
  if (tid == 0) sh.separators = 0;
  __syncthreads();

  // rows
  if (tid == 0) {
    double hsum = 0.0;
    int count = 0;
    for (int x = 0; x < n; ++x)
      if (s.y1[x] > s.y0[x]) {
        hsum = hsum + ((double)s.y1[x] - (double)s.y0[x]);
        ++count;
      }
    const double H = count ? hsum / (double)count : 0.0;
    sh.tx = min_gap_x * H;
    sh.ty = min_gap_y * H;
  }
  // the page's extent: every lane takes it for itself (min and max are exact in any order)
  float X0 = s.x0[0], X1 = s.x1[0], Y0 = s.y0[0], Y1 = s.y1[0];
  for (int y = 1; y < n; ++y) {
    X0 = fminf(X0, s.x0[y]);
    X1 = fmaxf(X1, s.x1[y]);
    Y0 = fminf(Y0, s.y0[y]);
    Y1 = fmaxf(Y1, s.y1[y]);
  }
  // the gap along y in front of quad x; -1 where nothing lies before it
  auto gap_y = [&](int x) {
    if (x >= n) return -1.0;
    const float ys = s.y0[x];
    float top = 0.f;
    int before = 0;
    for (int y = 0; y < n; ++y) {
      const float yo = s.y0[y], ye = s.y1[y];
      if (tb_before(yo, y, ys, x)) {
        top = before ? fmaxf(top, ye) : ye;
        ++before;
      }
    }
    return before ? (double)ys - (double)top : -1.0;
  };
  const double gy0 = gap_y(tid), gy1 = gap_y(tid + T);
  __syncthreads();
  const double tx = sh.tx, ty = sh.ty;
  if (tid < n) s.vy[tid] = (gy0 > 0 && gy0 >= ty) ? 1 : 0;
  if (tid + T < n) s.vy[tid + T] = (gy1 > 0 && gy1 >= ty) ? 1 : 0;
  __syncthreads();
  for (int k = 0; k < 2; ++k) {
    const int x = tid + k * T;
    if (x >= n) break;
    const float ys = s.y0[x];
    int r = s.vy[x], after = 0;
    for (int y = 0; y < n; ++y) {
      const float yo = s.y0[y];
      r += tb_before(yo, y, ys, x) ? s.vy[y] : 0;
      after += tb_before(ys, x, yo, y) ? 1 : 0;
    }
    s.row[x] = r;
    row_of[o + x] = r;
    if (after == 0) sh.rows = r + 1;  // the last quad by (y0, index) stands in the last row
  }
  __syncthreads();
  const int R = sh.rows;
  const int slots = n + R;  // R <= n: at most 2 cap, four a lane

  // intervals
  for (int k = 0; k < 2; ++k) {
    const int x = tid + k * T;
    if (x >= n) break;
    const int r = s.row[x];
    const float xs = s.x0[x];
    float reach = 0.f, left = xs, right = s.x1[x], top = s.y0[x], bottom = s.y1[x];
    int before = 0;
    for (int y = 0; y < n; ++y) {
      if (s.row[y] != r) continue;  // the same y in every lane, but not the same r: a divergent skip, no barrier inside
      const float xo = s.x0[y], xe = s.x1[y];
      left = fminf(left, xo);
      right = fmaxf(right, xe);
      top = fminf(top, s.y0[y]);
      bottom = fmaxf(bottom, s.y1[y]);
      if (tb_before(xo, y, xs, x)) {
        reach = before ? fmaxf(reach, xe) : xe;
        ++before;
      }
    }
    float a0 = 0.f, b0 = 0.f, a1 = 0.f, b1 = 0.f;
    if (before) {
      const double w = (double)xs - (double)reach;
      if (w > 0 && w >= tx) a0 = reach, b0 = xs;
    } else {
      if (left > X0) a0 = X0, b0 = left;
      if (right < X1) a1 = right, b1 = X1;
      if (boxes) {
        float4* dst = (float4*)boxes + ((size_t)2 * o + r) * 2;
        dst[0] = make_float4(X0, top, X1, top);
        dst[1] = make_float4(X1, bottom, X0, bottom);
      }
    }
    s.ia[x] = a0;
    s.ib[x] = b0;
    if (!before) {  // one quad a row: every slot from n to n + R - 1 is written
      s.ia[n + r] = a1;
      s.ib[n + r] = b1;
    }
  }
  __syncthreads();

  // runs
  const double kd = ceil(min_support * (double)R);
  const int K = kd < 1.0 ? 1 : (int)kd;
  for (int k = 0; k < 4; ++k) {
    const int e = tid + k * T;
    if (e >= slots) break;
    const float va = s.ia[e], vb = s.ib[e];
    int f = 0;
    if (va < vb) {
      int a_right = 0, a_left = 0, b_right = 0, b_left = 0;
      bool a_first = true, b_first = true;
      for (int j = 0; j < slots; ++j) {
        const float a = s.ia[j], b = s.ib[j];
        if (!(a < b)) continue;  // the same j in every lane
        a_right += (a <= va && va < b) ? 1 : 0;
        a_left += (a < va && va <= b) ? 1 : 0;
        b_right += (a <= vb && vb < b) ? 1 : 0;
        b_left += (a < vb && vb <= b) ? 1 : 0;
        a_first = a_first && !(j < e && a == va);
        b_first = b_first && !(j < e && b == vb);
      }
      if (a_first && a_left < K && a_right >= K) f |= TB_START;
      if (b_first && b_left >= K && b_right < K) f |= TB_END;
    }
    s.flag[e] = f;
  }
  __syncthreads();

  // separators
  for (int k = 0; k < 4; ++k) {
    const int e = tid + k * T;
    if (e >= slots) break;
    if (!(s.flag[e] & TB_END)) continue;
    const float vb = s.ib[e];
    float start = X0;  // every end has a start below it, and no start lies left of X0
    for (int j = 0; j < slots; ++j) {
      const float a = s.ia[j];
      if ((s.flag[j] & TB_START) && a < vb) start = fmaxf(start, a);
    }
    s.ra[e] = start;
  }
  __syncthreads();
  // TB_SEP is set behind the barrier: the loop above reads the flags of other slots
  for (int k = 0; k < 4; ++k) {
    const int e = tid + k * T;
    if (e >= slots) break;
    if (!(s.flag[e] & TB_END)) continue;
    const float vb = s.ib[e];
    if ((double)vb - (double)s.ra[e] >= tx && vb < X1) s.flag[e] |= TB_SEP;
  }
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    const int e = tid + k * T;
    if (e >= slots) break;
    if (!(s.flag[e] & TB_SEP)) continue;
    const float vb = s.ib[e];
    int rank = 0;
    for (int j = 0; j < slots; ++j) rank += ((s.flag[j] & TB_SEP) && s.ib[j] < vb) ? 1 : 0;
    if (rank < cap) {  // always: a separator ends at the x0 of a box that is not the leftmost, and they are distinct
      s.sa[rank] = s.ra[e];
      s.sb[rank] = vb;
    }
    atomicAdd(&sh.separators, 1);  // an integer count: the same in any order
  }
  __syncthreads();
  const int S = min(sh.separators, n - 1);

  // cells
  for (int k = 0; k < 2; ++k) {
    const int x = tid + k * T;
    if (x >= n) break;
    const float xs = s.x0[x], xe = s.x1[x];
    int c0 = 0, c1 = 0;
    for (int j = 0; j < S; ++j) {
      const float b = s.sb[j];
      c0 += b <= xs ? 1 : 0;
      c1 += b < xe ? 1 : 0;
    }
    cols[o + x] = c0 | (max(c0, c1) << 16);
  }
  if (boxes)
    for (int c = tid; c <= S; c += T) {
      if (R + c >= 2 * n) break;  // never: R <= n and S <= n - 1
      const float left = c == 0 ? X0 : s.sb[c - 1], right = c == S ? X1 : s.sa[c];
      float4* dst = (float4*)boxes + ((size_t)2 * o + R + c) * 2;
      dst[0] = make_float4(left, Y0, right, Y0);
      dst[1] = make_float4(right, Y1, left, Y1);
    }
  if (tid == 0) band_counts[page] = R + S + 1;
}

namespace {
int table_cap(int max_quads) { return (std::max(max_quads, 1) + 127) / 128 * 128; }  // two quads per lane, whole waves
size_t table_lds_bytes(int max_quads) { return (size_t)table_cap(max_quads) * TB_BYTES_PER_QUAD; }
}  // namespace

int launch_table_grid(kocr_ctx* ctx, const float* d_quads, const int32_t* d_off, int N, int max_quads, double min_gap_x, double min_gap_y,
                      double min_support, int32_t* d_row_of, int32_t* d_cols, int32_t* d_band_counts, float* d_boxes) {
  if (N == 0) return KOCR_OK;
  if (max_quads > KOCR_LINES_MAX_WORDS) KOCR_FAIL(ctx, KOCR_EINVAL, "launch_table_grid: a page above KOCR_LINES_MAX_WORDS");
  static std::atomic<bool> attr_done[64];
  const int dev = ctx->device & 63;
  if (!attr_done[dev]) {
    KOCR_HIP(ctx, hipFuncSetAttribute((const void*)table_grid_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)table_lds_bytes(KOCR_LINES_MAX_WORDS)));
    attr_done[dev] = true;
  }
  const int cap = table_cap(max_quads);
  ProfScope ps(ctx, "table_grid", 0, 0);
  hipLaunchKernelGGL(table_grid_kernel, dim3(N), dim3(cap / 2), table_lds_bytes(max_quads), ctx->stream, d_quads, d_off, cap, min_gap_x,
                     min_gap_y, min_support, d_row_of, d_cols, d_band_counts, d_boxes);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}
