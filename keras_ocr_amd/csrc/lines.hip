// lines.hip — recognised words grouped into text lines on the device (kocr_group_lines; the reference has no counterpart).
// The rule is tests/lines_statement.py ("Lines"): every float64 operation below is one of the
// statement's, in its order; this file is compiled with -ffp-contract=off so that none is fused.
#include "common.h"
#include <algorithm>

namespace {

constexpr int LN_MAX_THREADS = 1024;

// The LDS of one page of at most `cap` words: seven double rows and five int rows of cap entries each.  What a row holds
// changes from phase to phase (a __syncthreads between any write and a read by another thread):
//   row    records .. links        axis            words                    boxes                  line order
//   d0     c.x                     c.x             min p.A of the word      tl of the line (2 x float32 bits, at the root)
//   d1     c.y                     c.y             max p.A                  tr
//   d2     u.x                     u.x             min p.V                  br
//   d3     u.y                     u.y             max p.V                  bl
//   d4     w                       A.x at the root A.x                      centre y at the root   centre y
//   d5     h                       A.y at the root A.y                      centre x at the root   centre x
//   d6     -                       -               t = c.A                  t
//   parent union-find parent       -               -                        -                      rank of the line at the root
//   label  -                       root of the word's line (its smallest word index)
//   rank   -                       -               -                        rank of the word in its line
//   count  -                       members at the root
//   start  -                       -               -                        -                      first slot of the line at the root
struct LnRows {
  double *d0, *d1, *d2, *d3, *d4, *d5, *d6;
  int *parent, *label, *rank, *count, *start;
};
constexpr size_t LN_BYTES_PER_WORD = 7 * sizeof(double) + 5 * sizeof(int);
static_assert((size_t)KOCR_LINES_MAX_WORDS * LN_BYTES_PER_WORD + 64 <= 160 * 1024, "a page of KOCR_LINES_MAX_WORDS words must fit the 160 KB LDS of a CU");

__device__ inline double ln_norm(double x, double y) { return __dsqrt_rn(x * x + y * y); }

// statement: link_matrix, for words a < b.  The four conditions in an order that puts the square root and the divisions
// last; which of them fails first does not change the conjunction.
__device__ inline bool ln_link(const LnRows& s, int a, int b, double cos_max, double min_height_ratio, double max_offset, double max_gap) {
  const double wa = s.d4[a], ha = s.d5[a], wb = s.d4[b], hb = s.d5[b];
  if (wa == 0 || ha == 0 || wb == 0 || hb == 0) return false;  // degenerate: links to nothing
  const double hmin = fmin(ha, hb), hmax = fmax(ha, hb);
  if (!(hmin >= min_height_ratio * hmax)) return false;
  const double uax = s.d2[a], uay = s.d3[a], ubx = s.d2[b], uby = s.d3[b];
  const double dot = uax * ubx + uay * uby;
  if (!(dot >= cos_max)) return false;
  const double sx = uax + ubx, sy = uay + uby;
  const double sn = ln_norm(sx, sy);  // > 0: the two unit vectors are less than a right angle apart
  const double mx = sx / sn, my = sy / sn;
  const double dx = s.d0[b] - s.d0[a], dy = s.d1[b] - s.d1[a];
  const double along = fabs(dx * mx + dy * my);
  const double across = fabs(dx * my - dy * mx);
  if (!(across <= max_offset * hmin)) return false;
  const double gap = along - 0.5 * (wa + wb);
  return gap <= max_gap * hmax;
}

// Union-find in LDS.  A parent is never larger than its child and a root only ever gets a smaller parent, so the forest has
// no cycles, the root of a finished component is its smallest word and the result does not depend on the schedule.  Path
// halving writes only to words that are no longer roots, the compare-and-swap only succeeds on roots: the two never meet.
__device__ inline int ln_find(int* parent, int x) {
  volatile int* p = parent;
  for (;;) {
    const int y = p[x];
    if (y == x) return x;
    const int z = p[y];
    if (z != y) p[x] = z;
    x = z;
  }
}

__device__ inline void ln_union(int* parent, int a, int b) {
  for (;;) {
    a = ln_find(parent, a);
    b = ln_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(&parent[a], a, b) == a) return;
  }
}

__device__ inline double ln_pack(float x, float y) { return __hiloint2double(__float_as_int(y), __float_as_int(x)); }

}  // namespace

// One workgroup per page.  Phases, a __syncthreads between them:
//   records   one word per lane: the statement's word_records into LDS
//   links     the n (n - 1) / 2 pairs spread over the lanes, each tested ONCE and united at once: n^2 work whatever the
//             shape of the graph (no sweep is repeated until labels settle, so a long chain costs what a short one does)
//   labels    label = root of every word
//   axis      one lane per root: the sum of its members' u in ascending word index (members are never below the root)
//   words     one word per lane: t along its line's axis and the extent of its four corners along and across it
//   order     one word per lane: its rank in its line by (t, index), by counting; one lane per root: the line's box from the
//             members' extents (min / max do not depend on the order they are taken in) and the key of the line's centre
//   lines     one lane per root: the rank of the line by (centre y, centre x, root), by counting, and the slot of its first word
//   output    line_of, order, line_counts; the boxes go to `boxes` at the PAGE's word offset (a page has at most as many lines
//             as words), packed by lines_pack_kernel once the host knows every page's count
__global__ __launch_bounds__(LN_MAX_THREADS) void lines_group_kernel(const float* __restrict__ quads, const int32_t* __restrict__ off, int cap,
                                                                      double cos_max, double min_height_ratio, double max_offset, double max_gap,
                                                                      int32_t* __restrict__ line_of, int32_t* __restrict__ order,
                                                                      int32_t* __restrict__ line_counts, float* __restrict__ boxes) {
  extern __shared__ double ln_lds[];
  __shared__ int n_lines;
  const int page = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int o = off[page];
  const int n = min(off[page + 1] - o, cap);  // the host has checked the offsets; nothing is written past `cap` whatever they say
  if (n <= 0) {
    if (tid == 0) line_counts[page] = 0;
    return;
  }
  LnRows s;
  s.d0 = ln_lds;
  s.d1 = s.d0 + cap;
  s.d2 = s.d1 + cap;
  s.d3 = s.d2 + cap;
  s.d4 = s.d3 + cap;
  s.d5 = s.d4 + cap;
  s.d6 = s.d5 + cap;
  s.parent = (int*)(s.d6 + cap);
  s.label = s.parent + cap;
  s.rank = s.label + cap;
  s.count = s.rank + cap;
  s.start = s.count + cap;
  const float4* q4 = (const float4*)quads + (size_t)o * 2;
  if (tid == 0) n_lines = 0;

  // records
  for (int x = tid; x < n; x += T) {
    const float4 q01 = q4[2 * x], q23 = q4[2 * x + 1];
    const double p0x = q01.x, p0y = q01.y, p1x = q01.z, p1y = q01.w, p2x = q23.x, p2y = q23.y, p3x = q23.z, p3y = q23.w;
    const double lx = (p0x + p3x) * 0.5, ly = (p0y + p3y) * 0.5;
    const double rx = (p1x + p2x) * 0.5, ry = (p1y + p2y) * 0.5;
    const double ax = rx - lx, ay = ry - ly;
    const double w = ln_norm(ax, ay);
    const double h = 0.5 * (ln_norm(p3x - p0x, p3y - p0y) + ln_norm(p2x - p1x, p2y - p1y));
    const bool degenerate = w == 0 || h == 0;
    s.d0[x] = (lx + rx) * 0.5;
    s.d1[x] = (ly + ry) * 0.5;
    s.d2[x] = degenerate ? 1.0 : ax / w;
    s.d3[x] = degenerate ? 0.0 : ay / w;
    s.d4[x] = w;
    s.d5[x] = h;
    s.parent[x] = x;
  }
  __syncthreads();

  // links: pair (i, (i + d) mod n) for d = 1 .. n / 2 is every unordered pair once (for an even n the distance n / 2 from
  // the first half of the words only); consecutive lanes take consecutive i
  const int half = n / 2, pairs = n * half;
  for (int k = tid; k < pairs; k += T) {
    const int d = k / n + 1, i = k - (d - 1) * n;
    if ((n & 1) == 0 && d == half && i >= half) continue;
    int j = i + d;
    if (j >= n) j -= n;
    const int a = min(i, j), b = max(i, j);
    if (ln_link(s, a, b, cos_max, min_height_ratio, max_offset, max_gap)) ln_union(s.parent, a, b);
  }
  __syncthreads();

  // labels
  for (int x = tid; x < n; x += T) s.label[x] = ln_find(s.parent, x);
  __syncthreads();

  // axis (statement: line_axis)
  for (int r = tid; r < n; r += T) {
    if (s.label[r] != r) continue;
    double ax = 0.0, ay = 0.0;
    int members = 0;
    for (int y = r; y < n; ++y)
      if (s.label[y] == r) {
        ax = ax + s.d2[y];
        ay = ay + s.d3[y];
        ++members;
      }
    const double norm = ln_norm(ax, ay);
    s.d4[r] = norm == 0 ? 1.0 : ax / norm;
    s.d5[r] = norm == 0 ? 0.0 : ay / norm;
    s.count[r] = members;
    atomicAdd(&n_lines, 1);
  }
  __syncthreads();

  // words
  for (int x = tid; x < n; x += T) {
    const int r = s.label[x];
    const double ax = s.d4[r], ay = s.d5[r];
    const double vx = -ay, vy = ax;
    const float4 q01 = q4[2 * x], q23 = q4[2 * x + 1];
    const double px[4] = {q01.x, q01.z, q23.x, q23.z}, py[4] = {q01.y, q01.w, q23.y, q23.w};
    double t0 = px[0] * ax + py[0] * ay, t1 = t0, s0 = px[0] * vx + py[0] * vy, s1 = s0;
#pragma unroll
    for (int c = 1; c < 4; ++c) {
      const double t = px[c] * ax + py[c] * ay, v = px[c] * vx + py[c] * vy;
      t0 = fmin(t0, t);
      t1 = fmax(t1, t);
      s0 = fmin(s0, v);
      s1 = fmax(s1, v);
    }
    s.d6[x] = s.d0[x] * ax + s.d1[x] * ay;
    s.d0[x] = t0;
    s.d1[x] = t1;
    s.d2[x] = s0;
    s.d3[x] = s1;
  }
  __syncthreads();

  // order (statement: word_order) ...
  for (int x = tid; x < n; x += T) {
    const int r = s.label[x];
    const double tx = s.d6[x];
    int before = 0;
    for (int y = r; y < n; ++y)
      if (s.label[y] == r) {
        const double ty = s.d6[y];
        before += (ty < tx || (ty == tx && y < x)) ? 1 : 0;
      }
    s.rank[x] = before;
  }
  // ... and boxes (statement: line_box).  d0 .. d3 of the root are read by this lane alone, which then overwrites them
  for (int r = tid; r < n; r += T) {
    if (s.label[r] != r) continue;
    double t0 = s.d0[r], t1 = s.d1[r], s0 = s.d2[r], s1 = s.d3[r];
    for (int y = r + 1; y < n; ++y)
      if (s.label[y] == r) {
        t0 = fmin(t0, s.d0[y]);
        t1 = fmax(t1, s.d1[y]);
        s0 = fmin(s0, s.d2[y]);
        s1 = fmax(s1, s.d3[y]);
      }
    const double ax = s.d4[r], ay = s.d5[r];
    const double vx = -ay, vy = ax;
    const double tlx = t0 * ax + s0 * vx, tly = t0 * ay + s0 * vy;
    const double trx = t1 * ax + s0 * vx, try_ = t1 * ay + s0 * vy;
    const double brx = t1 * ax + s1 * vx, bry = t1 * ay + s1 * vy;
    const double blx = t0 * ax + s1 * vx, bly = t0 * ay + s1 * vy;
    s.d0[r] = ln_pack((float)tlx, (float)tly);
    s.d1[r] = ln_pack((float)trx, (float)try_);
    s.d2[r] = ln_pack((float)brx, (float)bry);
    s.d3[r] = ln_pack((float)blx, (float)bly);
    s.d4[r] = (tly + bry) * 0.5;
    s.d5[r] = (tlx + brx) * 0.5;
  }
  __syncthreads();

  // lines
  for (int r = tid; r < n; r += T) {
    if (s.label[r] != r) continue;
    const double ky = s.d4[r], kx = s.d5[r];
    int before = 0, first = 0;
    for (int q = 0; q < n; ++q) {
      if (s.label[q] != q) continue;
      const double qy = s.d4[q], qx = s.d5[q];
      if (qy < ky || (qy == ky && (qx < kx || (qx == kx && q < r)))) {
        ++before;
        first += s.count[q];
      }
    }
    s.parent[r] = before;
    s.start[r] = first;
    if (boxes) {
      float4* dst = (float4*)boxes + (size_t)(o + before) * 2;
      const double a = s.d0[r], b = s.d1[r], c = s.d2[r], d = s.d3[r];
      dst[0] = make_float4(__int_as_float(__double2loint(a)), __int_as_float(__double2hiint(a)), __int_as_float(__double2loint(b)),
                           __int_as_float(__double2hiint(b)));
      dst[1] = make_float4(__int_as_float(__double2loint(c)), __int_as_float(__double2hiint(c)), __int_as_float(__double2loint(d)),
                           __int_as_float(__double2hiint(d)));
    }
  }
  __syncthreads();

  // output
  for (int x = tid; x < n; x += T) {
    const int r = s.label[x];
    line_of[o + x] = s.parent[r];
    order[o + s.start[r] + s.rank[x]] = x;
  }
  if (tid == 0) line_counts[page] = n_lines;
}

// The boxes of page i from their place at the page's word offset to the batch's packed order: lines [line_off[i], line_off[i + 1]).
__global__ __launch_bounds__(256) void lines_pack_kernel(const float* __restrict__ scratch, const int32_t* __restrict__ off,
                                                          const long long* __restrict__ line_off, float* __restrict__ boxes) {
  const int page = blockIdx.x;
  const long long first = line_off[page], lines = line_off[page + 1] - first;
  const float4* src = (const float4*)scratch + (size_t)off[page] * 2;
  float4* dst = (float4*)boxes + (size_t)first * 2;
  for (long long k = threadIdx.x; k < 2 * lines; k += blockDim.x) dst[k] = src[k];
}

size_t lines_lds_bytes(int max_words) {
  const size_t cap = ((size_t)std::max(max_words, 1) + 63) / 64 * 64;
  return cap * LN_BYTES_PER_WORD;
}

int launch_lines_group(kocr_ctx* ctx, const float* d_quads, const int32_t* d_off, int N, int max_words, const LinesRule& rule,
                       int32_t* d_line_of, int32_t* d_order, int32_t* d_line_counts, float* d_boxes) {
  if (N == 0) return KOCR_OK;
  if (max_words > KOCR_LINES_MAX_WORDS) KOCR_FAIL(ctx, KOCR_EINVAL, "launch_lines_group: a page above KOCR_LINES_MAX_WORDS");
  static std::atomic<bool> attr_done[64];
  const int dev = ctx->device & 63;
  if (!attr_done[dev]) {
    KOCR_HIP(ctx, hipFuncSetAttribute((const void*)lines_group_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lines_lds_bytes(KOCR_LINES_MAX_WORDS)));
    attr_done[dev] = true;
  }
  const int cap = (std::max(max_words, 1) + 63) / 64 * 64;
  // a small page leaves most lanes of a large block idle at every barrier: 256 lanes up to 256 words, 1024 above
  const int threads = cap <= 256 ? 256 : LN_MAX_THREADS;
  ProfScope ps(ctx, "lines_group", 0, 0);
  hipLaunchKernelGGL(lines_group_kernel, dim3(N), dim3(threads), lines_lds_bytes(max_words), ctx->stream, d_quads, d_off, cap, rule.cos_max,
                     rule.min_height_ratio, rule.max_offset, rule.max_gap, d_line_of, d_order, d_line_counts, d_boxes);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

int launch_lines_pack(kocr_ctx* ctx, const float* d_scratch, const int32_t* d_off, const long long* d_line_off, int N, float* d_boxes) {
  if (N == 0) return KOCR_OK;
  ProfScope ps(ctx, "lines_pack", 0, 0);
  hipLaunchKernelGGL(lines_pack_kernel, dim3(N), dim3(256), 0, ctx->stream, d_scratch, d_off, d_line_off, d_boxes);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}
