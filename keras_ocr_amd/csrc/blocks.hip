// blocks.hip — the lines of a page cut into blocks (columns, paragraphs) in reading order by a recursive XY-cut on the device
// (kocr_group_lines with flags == KOCR_LINES_BLOCKS; the reference has no counterpart).  The rule is tests/blocks_statement.py
// ("Blocks"): a gap is one float64 subtraction of two float32 values, a threshold one float64 product,
// the mean height one sum in ascending index; this file is compiled with -ffp-contract=off like lines.hip.
// With KOCR_LINES_DESKEW the cut runs in the page's own frame (tests/deskew_statement.py, "Rotated pages" in the same section):
// blocks_axis_kernel, blocks_frame_kernel and blocks_unframe_kernel at the end of this file, around an unchanged cut.
#include "common.h"
#include <algorithm>

namespace {

constexpr int BK_MAX_THREADS = 1024, BK_WAVES = BK_MAX_THREADS / 64;
static_assert(2 * BK_MAX_THREADS >= KOCR_LINES_MAX_WORDS, "a lane owns two positions of a page");

// The LDS of one page of at most `cap` quads (cap = 2 x the lanes of the block).  A SEGMENT is a set of quads that the cuts
// made so far have not separated; segments are numbered in reading order (their RANK).  Both orders keep every segment in
// one slice [start[r], start[r + 1]), the same slice in both, so a segment-wide scan is a segmented scan over positions.
struct BkRows {
  float *x0, *x1, *y0, *y1;  // [quad] the axis-aligned box
  int *ordx, *ordy;          // [position] -> quad: by (rank, x0, index) and by (rank, y0, x0, index)
  int *sp;                   // [position] the rank of the segment at that position (the same in both orders)
  int *side;                 // [quad] 1: behind this round's cut of its segment
  int *cnt, *cutpos, *cutaxis;  // [rank] valid x-gaps; the position the cut falls before; 0 an x-cut, 1 a y-cut, -1 none
  int *start;                // [rank], cap + 1 entries
};
constexpr size_t BK_BYTES_PER_QUAD = 4 * sizeof(float) + 8 * sizeof(int);
constexpr size_t BK_BYTES_FIXED = 64;  // the last entry of `start`, rounded up

struct BkBest {
  double g;  // a gap; -1 where there is none
  int p;     // the position it lies before
};

// what the waves of a block hand each other in a scan; two sets taken in turns, so that one barrier per scan is enough (a
// wave that is still reading set 0 of scan k cannot meet a writer before scan k + 2, which lies behind scan k + 1's barrier)
struct BkScratch {
  alignas(16) unsigned char v[2][BK_WAVES][16];
  int f[2][BK_WAVES];
};

__device__ inline float bk_up(float v, int d) { return __shfl_up(v, d); }
__device__ inline int bk_up(int v, int d) { return __shfl_up(v, d); }
__device__ inline BkBest bk_up(BkBest v, int d) { return BkBest{__shfl_up(v.g, d), __shfl_up(v.p, d)}; }

struct BkMax {
  __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct BkSum {
  __device__ int operator()(int a, int b) const { return a + b; }
};
// the wider gap; of two equal ones the earlier (the left operand is always the earlier position)
struct BkWidest {
  __device__ BkBest operator()(BkBest a, BkBest b) const { return b.g > a.g ? b : a; }
};

// Segmented scan over the 2 x blockDim.x positions of a block, lane t owning positions 2 t (value a, head flag ha) and
// 2 t + 1 (b, hb); a head starts a segment, and position 0 must be one.  ea / eb: op over the values of the same segment
// BEFORE the position, in position order (meaningless at a head, which has none).  The operands are always combined
// earlier-on-the-left, and what is combined with what depends on the positions alone: the result is that of a sequential
// left-to-right pass for max and integer sums, and for BkWidest by its tie rule.  Every lane of the block must call it.
template <class V, class Op>
__device__ inline void bk_scan(V a, bool ha, V b, bool hb, Op op, BkScratch* sc, int& turn, V& ea, V& eb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  V v = hb ? b : op(a, b);
  int f = (ha || hb) ? 1 : 0;
  for (int d = 1; d < 64; d <<= 1) {  // inclusive over the lanes of the wave: (of, ov) o (f, v) = (of | f, f ? v : op(ov, v))
    const V ov = bk_up(v, d);
    const int of = __shfl_up(f, d);
    if (lane >= d) {
      if (!f) v = op(ov, v);
      f |= of;
    }
  }
  if (lane == 63) {
    *(V*)sc->v[turn][wave] = v;
    sc->f[turn][wave] = f;
  }
  const V lv = bk_up(v, 1);  // the lanes before this one in its wave
  const int lf = __shfl_up(f, 1);
  __syncthreads();
  V wv = a;  // the waves before this one
  bool whave = false;
  for (int k = 0; k < wave; ++k) {
    const V kv = *(const V*)sc->v[turn][k];
    wv = (whave && !sc->f[turn][k]) ? op(wv, kv) : kv;
    whave = true;
  }
  V before = a;
  if (lane > 0)
    before = (whave && !lf) ? op(wv, lv) : lv;
  else if (whave)
    before = wv;
  ea = before;
  eb = ha ? a : op(before, a);
  turn ^= 1;
}

}  // namespace

// One workgroup per page, lane t owning positions 2 t and 2 t + 1 of both orders.
//   boxes    one quad per lane: x0, x1, y0, y1
//   setup    lane 0: the mean height in ascending index, tx and ty; every lane: the rank of its quads by (x0, index) and by
//            (y0, x0, index), by counting, ONCE.  (The statement orders a segment by (y0, index) for its y-gaps.  Quads of equal
//            y0 follow each other in either order, only the first of them can have a positive gap -- the others come after
//            a quad whose y1 >= their y0 --, and that gap is y0 minus the largest y1 of the quads of smaller y0 either way:
//            the same gaps between the same sets.  (y0, x0, index) is the order of the lines inside a block, so the y-order
//            IS the output.)
//   rounds   every segment looks for a cut: the exclusive running max of x1 along its slice of the x-order gives every gap
//            along x, likewise y1 along y.  With valid x-gaps it is cut at the MIDDLE one of them, otherwise at the widest
//            valid y-gap (the first of equals), otherwise it is final -- a final segment finds nothing again in later
//            rounds, which costs no more than skipping it.  One x-gap per round gives the statement's blocks: a quad that
//            has a predecessor in its part keeps its running max (everything left of the part ends before the part's first
//            quad starts, which ends no earlier than it starts), so the other valid x-gaps stay valid, no new one appears,
//            and a part is cut along y only when none is left -- the parts the statement gets by cutting all at once, in
//            the same left-to-right order; the middle one makes that log2 (parts) rounds.  The quads behind the cut are
//            moved behind the others by a stable partition of both slices (a segmented sum), the ranks renumbered by a sum
//            over the new heads.  A round costs seven scans whatever the page looks like; the loop ends with the first round
//            that cuts nothing, after at most n rounds.
//   output   block_of, order (the y-order), block_counts; one lane per block: its box, to `boxes` at the PAGE's quad offset
//            (packed by lines_pack_kernel)
__global__ __launch_bounds__(BK_MAX_THREADS) void blocks_cut_kernel(const float* __restrict__ quads, const int32_t* __restrict__ off, int cap,
                                                                     double min_gap_x, double min_gap_y, int32_t* __restrict__ block_of,
                                                                     int32_t* __restrict__ order, int32_t* __restrict__ block_counts,
                                                                     float* __restrict__ boxes) {
  extern __shared__ float bk_lds[];
  __shared__ BkScratch scratch;
  __shared__ double gap_min[2];
  __shared__ int n_segments;
  const int page = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int o = off[page];
  const int n = min(min(off[page + 1] - o, cap), 2 * T);  // the host has checked the offsets; nothing is written past `cap` whatever they say
  if (n <= 0) {
    if (tid == 0) block_counts[page] = 0;
    return;
  }
  BkRows s;
  s.x0 = bk_lds;
  s.x1 = s.x0 + cap;
  s.y0 = s.x1 + cap;
  s.y1 = s.y0 + cap;
  s.ordx = (int*)(s.y1 + cap);
  s.ordy = s.ordx + cap;
  s.sp = s.ordy + cap;
  s.side = s.sp + cap;
  s.cnt = s.side + cap;
  s.cutpos = s.cnt + cap;
  s.cutaxis = s.cutpos + cap;
  s.start = s.cutaxis + cap;
  const float4* q4 = (const float4*)quads + (size_t)o * 2;

  // boxes
  for (int x = tid; x < n; x += T) {
    const float4 q01 = q4[2 * x], q23 = q4[2 * x + 1];
    s.x0[x] = fminf(fminf(q01.x, q01.z), fminf(q23.x, q23.z));
    s.x1[x] = fmaxf(fmaxf(q01.x, q01.z), fmaxf(q23.x, q23.z));
    s.y0[x] = fminf(fminf(q01.y, q01.w), fminf(q23.y, q23.w));
    s.y1[x] = fmaxf(fmaxf(q01.y, q01.w), fmaxf(q23.y, q23.w));
  }
  __syncthreads();

  // setup
  if (tid == 0) {
    double hsum = 0.0;
    int count = 0;
    for (int x = 0; x < n; ++x)
      if (s.y1[x] > s.y0[x]) {
        hsum = hsum + ((double)s.y1[x] - (double)s.y0[x]);
        ++count;
      }
    const double H = count ? hsum / (double)count : 0.0;
    gap_min[0] = min_gap_x * H;
    gap_min[1] = min_gap_y * H;
    s.start[0] = 0;
    s.start[1] = n;
  }
  for (int x = tid; x < n; x += T) {
    const float xs = s.x0[x], ys = s.y0[x];
    int bx = 0, by = 0;
    for (int y = 0; y < n; ++y) {
      const float xo = s.x0[y], yo = s.y0[y];
      const bool x_first = xo < xs || (xo == xs && y < x);
      bx += x_first ? 1 : 0;
      by += (yo < ys || (yo == ys && x_first)) ? 1 : 0;
    }
    s.ordx[bx] = x;
    s.ordy[by] = x;
    s.sp[x] = 0;
  }
  __syncthreads();
  const double tx = gap_min[0], ty = gap_min[1];

  // rounds
  const int p0 = 2 * tid, p1 = p0 + 1;
  const bool in0 = p0 < n, in1 = p1 < n;
  int segments = 1, turn = 0;
  for (int round = 0; round < n; ++round) {
    const int r0 = in0 ? s.sp[p0] : -1, r1 = in1 ? s.sp[p1] : -1;
    const bool h0 = !in0 || p0 == 0 || s.sp[p0 - 1] != r0, h1 = !in1 || r1 != r0;
    const bool last0 = in0 && (!in1 || r1 != r0), last1 = in1 && (p1 == n - 1 || s.sp[p1 + 1] != r1);
    const int ex0 = in0 ? s.ordx[p0] : 0, ex1 = in1 ? s.ordx[p1] : 0, ey0 = in0 ? s.ordy[p0] : 0, ey1 = in1 ? s.ordy[p1] : 0;

    // the gaps along x, and the valid ones of every segment counted
    float m0, m1;
    bk_scan(in0 ? s.x1[ex0] : 0.f, h0, in1 ? s.x1[ex1] : 0.f, h1, BkMax(), &scratch, turn, m0, m1);
    double g0 = h0 ? -1.0 : (double)s.x0[ex0] - (double)m0, g1 = h1 ? -1.0 : (double)s.x0[ex1] - (double)m1;
    const int vx0 = (g0 > 0 && g0 >= tx) ? 1 : 0, vx1 = (g1 > 0 && g1 >= tx) ? 1 : 0;
    int c0, c1;
    bk_scan(vx0, h0, vx1, h1, BkSum(), &scratch, turn, c0, c1);
    c0 = (h0 ? 0 : c0) + vx0;
    c1 = (h1 ? 0 : c1) + vx1;
    if (last0) s.cnt[r0] = c0;
    if (last1) s.cnt[r1] = c1;
    __syncthreads();
    if (vx0 && c0 == (s.cnt[r0] + 1) / 2) s.cutpos[r0] = p0;
    if (vx1 && c1 == (s.cnt[r1] + 1) / 2) s.cutpos[r1] = p1;

    // the gaps along y, and the widest valid one of every segment
    bk_scan(in0 ? s.y1[ey0] : 0.f, h0, in1 ? s.y1[ey1] : 0.f, h1, BkMax(), &scratch, turn, m0, m1);
    g0 = h0 ? -1.0 : (double)s.y0[ey0] - (double)m0;
    g1 = h1 ? -1.0 : (double)s.y0[ey1] - (double)m1;
    const BkBest b0{(g0 > 0 && g0 >= ty) ? g0 : -1.0, p0}, b1{(g1 > 0 && g1 >= ty) ? g1 : -1.0, p1};
    BkBest w0, w1;
    bk_scan(b0, h0, b1, h1, BkWidest(), &scratch, turn, w0, w1);
    w0 = h0 ? b0 : BkWidest()(w0, b0);
    w1 = h1 ? b1 : BkWidest()(w1, b1);
    if (last0) {
      const bool along_x = s.cnt[r0] > 0;
      s.cutaxis[r0] = along_x ? 0 : (w0.g > 0 ? 1 : -1);
      if (!along_x && w0.g > 0) s.cutpos[r0] = w0.p;
    }
    if (last1) {
      const bool along_x = s.cnt[r1] > 0;
      s.cutaxis[r1] = along_x ? 0 : (w1.g > 0 ? 1 : -1);
      if (!along_x && w1.g > 0) s.cutpos[r1] = w1.p;
    }
    __syncthreads();

    // which quads lie behind the cut of their segment
    const int a0 = in0 ? s.cutaxis[r0] : -1, a1 = in1 ? s.cutaxis[r1] : -1;
    const int k0 = a0 >= 0 ? s.cutpos[r0] : 0, k1 = a1 >= 0 ? s.cutpos[r1] : 0;
    if (in0) s.side[a0 == 1 ? ey0 : ex0] = (a0 >= 0 && p0 >= k0) ? 1 : 0;
    if (in1) s.side[a1 == 1 ? ey1 : ex1] = (a1 >= 0 && p1 >= k1) ? 1 : 0;
    __syncthreads();

    // the stable partition of both slices: the quads before the cut keep their order at the front, the others behind them
    const int st0 = in0 ? s.start[r0] : 0, en0 = in0 ? s.start[r0 + 1] : 0, st1 = in1 ? s.start[r1] : 0, en1 = in1 ? s.start[r1 + 1] : 0;
    const int front0 = a0 >= 0 ? k0 - st0 : en0 - st0, front1 = a1 >= 0 ? k1 - st1 : en1 - st1;  // quads before the cut
    const int sx0 = in0 ? s.side[ex0] : 0, sx1 = in1 ? s.side[ex1] : 0, sy0 = in0 ? s.side[ey0] : 0, sy1 = in1 ? s.side[ey1] : 0;
    int bx0, bx1, by0, by1;  // quads behind the cut before this position, in each order
    bk_scan(sx0, h0, sx1, h1, BkSum(), &scratch, turn, bx0, bx1);
    bk_scan(sy0, h0, sy1, h1, BkSum(), &scratch, turn, by0, by1);
    bx0 = h0 ? 0 : bx0;
    bx1 = h1 ? 0 : bx1;
    by0 = h0 ? 0 : by0;
    by1 = h1 ? 0 : by1;
    const int nx0 = sx0 ? st0 + front0 + bx0 : p0 - bx0, nx1 = sx1 ? st1 + front1 + bx1 : p1 - bx1;
    const int ny0 = sy0 ? st0 + front0 + by0 : p0 - by0, ny1 = sy1 ? st1 + front1 + by1 : p1 - by1;

    // the new ranks: a segment starts where one started before and at every cut
    const int nh0 = (in0 && (h0 || (a0 >= 0 && p0 == k0))) ? 1 : 0, nh1 = (in1 && (h1 || (a1 >= 0 && p1 == k1))) ? 1 : 0;
    int nr0, nr1;
    bk_scan(nh0, p0 == 0, nh1, false, BkSum(), &scratch, turn, nr0, nr1);
    nr0 = (p0 == 0 ? 0 : nr0) + nh0 - 1;  // heads up to and including this position, less one
    nr1 = nr1 + nh1 - 1;
    // every lane is past the scan's barrier: all reads of this round's orders, ranks, starts and cuts are done
    if (in0) {
      s.ordx[nx0] = ex0;
      s.ordy[ny0] = ey0;
      s.sp[p0] = nr0;
      if (nh0) s.start[nr0] = p0;
      if (p0 == n - 1) {
        s.start[nr0 + 1] = n;
        n_segments = nr0 + 1;
      }
    }
    if (in1) {
      s.ordx[nx1] = ex1;
      s.ordy[ny1] = ey1;
      s.sp[p1] = nr1;
      if (nh1) s.start[nr1] = p1;
      if (p1 == n - 1) {
        s.start[nr1 + 1] = n;
        n_segments = nr1 + 1;
      }
    }
    __syncthreads();
    const int now = n_segments;  // the next write to it lies behind the next round's barriers
    if (now == segments) break;
    segments = now;
  }

  // output
  for (int k = 0; k < 2; ++k) {
    const int p = p0 + k;
    if (p >= n) break;
    const int r = s.sp[p];
    block_of[o + s.ordx[p]] = r;
    order[o + p] = s.ordy[p];
    if (boxes && s.start[r] == p) {
      float bx0 = s.x0[s.ordy[p]], bx1 = s.x1[s.ordy[p]], by0 = s.y0[s.ordy[p]], by1 = s.y1[s.ordy[p]];
      for (int q = p + 1; q < s.start[r + 1]; ++q) {
        const int y = s.ordy[q];
        bx0 = fminf(bx0, s.x0[y]);
        bx1 = fmaxf(bx1, s.x1[y]);
        by0 = fminf(by0, s.y0[y]);
        by1 = fmaxf(by1, s.y1[y]);
      }
      float4* dst = (float4*)boxes + (size_t)(o + r) * 2;
      dst[0] = make_float4(bx0, by0, bx1, by0);
      dst[1] = make_float4(bx1, by1, bx0, by1);
    }
  }
  if (tid == 0) block_counts[page] = segments;
}

namespace {
int blocks_cap(int max_quads) { return (std::max(max_quads, 1) + 127) / 128 * 128; }  // two positions per lane, whole waves
size_t blocks_lds_bytes(int max_quads) { return (size_t)blocks_cap(max_quads) * BK_BYTES_PER_QUAD + BK_BYTES_FIXED; }
}  // namespace

int launch_blocks_cut(kocr_ctx* ctx, const float* d_quads, const int32_t* d_off, int N, int max_quads, double min_gap_x, double min_gap_y,
                      int32_t* d_block_of, int32_t* d_order, int32_t* d_block_counts, float* d_boxes) {
  if (N == 0) return KOCR_OK;
  if (max_quads > KOCR_LINES_MAX_WORDS) KOCR_FAIL(ctx, KOCR_EINVAL, "launch_blocks_cut: a page above KOCR_LINES_MAX_WORDS");
  static std::atomic<bool> attr_done[64];
  const int dev = ctx->device & 63;
  if (!attr_done[dev]) {
    KOCR_HIP(ctx, hipFuncSetAttribute((const void*)blocks_cut_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)blocks_lds_bytes(KOCR_LINES_MAX_WORDS)));
    attr_done[dev] = true;
  }
  const int cap = blocks_cap(max_quads);
  ProfScope ps(ctx, "blocks_cut", 0, 0);
  hipLaunchKernelGGL(blocks_cut_kernel, dim3(N), dim3(cap / 2), blocks_lds_bytes(max_quads), ctx->stream, d_quads, d_off, cap, min_gap_x,
                     min_gap_y, d_block_of, d_order, d_block_counts, d_boxes);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// ---- KOCR_LINES_DESKEW: the page's own frame (tests/deskew_statement.py) -------------------------------------------------

namespace {

struct BkCost {
  double c;  // the summed weighted chords of a candidate; +inf where there is none
  int k;     // the candidate
};
// the cheaper candidate, of two equal ones the smaller index: a total order, so the reduction is exact in any order
__device__ inline BkCost bk_cheaper(BkCost a, BkCost b) { return (b.c < a.c || (b.c == a.c && b.k < a.k)) ? b : a; }

constexpr int BK_NONE = 0x7fffffff;

}  // namespace

// One workgroup per page of at most `cap` quads, blockDim.x = cap / 2: lane t owns the candidates t and t + blockDim.x.
//   records   "Lines" per-word arithmetic: u = a / w and w of every quad into LDS as float64 (u = (1, 0), w = 0 for a quad
//             without direction)
//   costs     every lane walks j = 0 .. n - 1 in that order; the read of quad j is the same address in every lane (an LDS
//             broadcast), and c_k = c_k + w_j * sqrt(dx * dx + dy * dy) is the statement's sum, operation for operation
//   arg-min   over (c_k, k), by shuffles inside a wave and through LDS between them
//   output    axes[2 page], axes[2 page + 1] = the axis; (1, 0) for a page without any direction
__global__ __launch_bounds__(BK_MAX_THREADS) void blocks_axis_kernel(const float* __restrict__ quads, const int32_t* __restrict__ off, int cap,
                                                                      double* __restrict__ axes) {
  extern __shared__ double bk_axis_lds[];
  __shared__ double best_c[BK_WAVES];
  __shared__ int best_k[BK_WAVES];
  const int page = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int o = off[page];
  const int n = min(min(off[page + 1] - o, cap), 2 * T);
  if (n <= 0) {
    if (tid == 0) {
      axes[2 * (size_t)page] = 1.0;
      axes[2 * (size_t)page + 1] = 0.0;
    }
    return;
  }
  double *ux = bk_axis_lds, *uy = ux + cap, *wt = uy + cap;
  const float4* q4 = (const float4*)quads + (size_t)o * 2;

  // records
  for (int x = tid; x < n; x += T) {
    const float4 q01 = q4[2 * x], q23 = q4[2 * x + 1];
    const double p0x = q01.x, p0y = q01.y, p1x = q01.z, p1y = q01.w, p2x = q23.x, p2y = q23.y, p3x = q23.z, p3y = q23.w;
    const double lx = (p0x + p3x) * 0.5, ly = (p0y + p3y) * 0.5;
    const double rx = (p1x + p2x) * 0.5, ry = (p1y + p2y) * 0.5;
    const double ax = rx - lx, ay = ry - ly;
    const double w = __dsqrt_rn(ax * ax + ay * ay);
    ux[x] = w == 0 ? 1.0 : ax / w;
    uy[x] = w == 0 ? 0.0 : ay / w;
    wt[x] = w;
  }
  __syncthreads();

  // costs
  const int k0 = tid, k1 = tid + T;
  const bool has0 = k0 < n && wt[k0] > 0, has1 = k1 < n && wt[k1] > 0;
  const double u0x = has0 ? ux[k0] : 1.0, u0y = has0 ? uy[k0] : 0.0, u1x = has1 ? ux[k1] : 1.0, u1y = has1 ? uy[k1] : 0.0;
  double c0 = 0.0, c1 = 0.0;
  for (int j = 0; j < n; ++j) {
    const double wj = wt[j];
    if (!(wj > 0)) continue;  // the same j in every lane
    const double jx = ux[j], jy = uy[j];
    const double d0x = u0x - jx, d0y = u0y - jy, d1x = u1x - jx, d1y = u1y - jy;
    c0 = c0 + wj * __dsqrt_rn(d0x * d0x + d0y * d0y);
    c1 = c1 + wj * __dsqrt_rn(d1x * d1x + d1y * d1y);
  }

  // arg-min
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  BkCost best = bk_cheaper(BkCost{has0 ? c0 : inf, has0 ? k0 : BK_NONE}, BkCost{has1 ? c1 : inf, has1 ? k1 : BK_NONE});
  for (int d = 32; d > 0; d >>= 1) best = bk_cheaper(best, BkCost{__shfl_xor(best.c, d), __shfl_xor(best.k, d)});
  const int wave = tid >> 6, waves = (T + 63) >> 6;
  if ((tid & 63) == 0) {
    best_c[wave] = best.c;
    best_k[wave] = best.k;
  }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < waves; ++v) best = bk_cheaper(best, BkCost{best_c[v], best_k[v]});
    const bool any = best.k != BK_NONE;
    axes[2 * (size_t)page] = any ? ux[best.k] : 1.0;
    axes[2 * (size_t)page + 1] = any ? uy[best.k] : 0.0;
  }
}

// Every corner p of every quad into its page's frame: x' = p.x A.x + p.y A.y, y' = p.x V.x + p.y V.y with V = (-A.y, A.x),
// float64 of float32, each rounded to float32.  blockIdx.x is the page, one quad per lane.
__global__ __launch_bounds__(256) void blocks_frame_kernel(const float* __restrict__ quads, const int32_t* __restrict__ off,
                                                            const double* __restrict__ axes, float* __restrict__ frame) {
  const int page = blockIdx.x;
  const int o = off[page], n = off[page + 1] - o;
  const int x = blockIdx.y * blockDim.x + threadIdx.x;
  if (x >= n) return;
  const double ax = axes[2 * (size_t)page], ay = axes[2 * (size_t)page + 1];
  const double vx = -ay, vy = ax;
  const float4* src = (const float4*)quads + (size_t)(o + x) * 2;
  float4* dst = (float4*)frame + (size_t)(o + x) * 2;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float4 q = src[h];
    const double p0x = q.x, p0y = q.y, p1x = q.z, p1y = q.w;
    dst[h] = make_float4((float)(p0x * ax + p0y * ay), (float)(p0x * vx + p0y * vy), (float)(p1x * ax + p1y * ay), (float)(p1x * vx + p1y * vy));
  }
}

// The first counts[page] boxes of every page, which blocks_cut_kernel wrote at the page's quad offset as (X0, Y0), (X1, Y0),
// (X1, Y1), (X0, Y1) in the frame, back onto the page in place: tl = X0 A + Y0 V, tr = X1 A + Y0 V, br = X1 A + Y1 V,
// bl = X0 A + Y1 V, every coordinate a * b + c * d in that order in float64, rounded to float32.
__global__ __launch_bounds__(256) void blocks_unframe_kernel(float* __restrict__ boxes, const int32_t* __restrict__ off,
                                                              const int32_t* __restrict__ counts, const double* __restrict__ axes) {
  const int page = blockIdx.x;
  const int o = off[page], blocks = min(counts[page], off[page + 1] - o);  // a page has at most as many blocks as quads
  const double ax = axes[2 * (size_t)page], ay = axes[2 * (size_t)page + 1];
  const double vx = -ay, vy = ax;
  for (int k = threadIdx.x; k < blocks; k += blockDim.x) {
    float4* box = (float4*)boxes + (size_t)(o + k) * 2;
    const float4 b0 = box[0], b1 = box[1];
    const double X0 = b0.x, Y0 = b0.y, X1 = b0.z, Y1 = b1.y;
    box[0] = make_float4((float)(X0 * ax + Y0 * vx), (float)(X0 * ay + Y0 * vy), (float)(X1 * ax + Y0 * vx), (float)(X1 * ay + Y0 * vy));
    box[1] = make_float4((float)(X1 * ax + Y1 * vx), (float)(X1 * ay + Y1 * vy), (float)(X0 * ax + Y1 * vx), (float)(X0 * ay + Y1 * vy));
  }
}

int launch_blocks_axis(kocr_ctx* ctx, const float* d_quads, const int32_t* d_off, int N, int max_quads, double* d_axes) {
  if (N == 0) return KOCR_OK;
  if (max_quads > KOCR_LINES_MAX_WORDS) KOCR_FAIL(ctx, KOCR_EINVAL, "launch_blocks_axis: a page above KOCR_LINES_MAX_WORDS");
  const int cap = blocks_cap(max_quads);  // 24 bytes a quad: 48 KB at KOCR_LINES_MAX_WORDS, below the limit that needs no attribute
  static_assert((size_t)KOCR_LINES_MAX_WORDS * 3 * sizeof(double) + 256 <= 64 * 1024, "the axis kernel's page must fit the default LDS limit");
  ProfScope ps(ctx, "blocks_axis", 0, 0);
  hipLaunchKernelGGL(blocks_axis_kernel, dim3(N), dim3(cap / 2), (size_t)cap * 3 * sizeof(double), ctx->stream, d_quads, d_off, cap, d_axes);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

int launch_blocks_frame(kocr_ctx* ctx, const float* d_quads, const int32_t* d_off, const double* d_axes, int N, int max_quads, float* d_frame) {
  if (N == 0 || max_quads == 0) return KOCR_OK;
  ProfScope ps(ctx, "blocks_frame", 0, 0);
  hipLaunchKernelGGL(blocks_frame_kernel, dim3(N, (max_quads + 255) / 256), dim3(256), 0, ctx->stream, d_quads, d_off, d_axes, d_frame);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

int launch_blocks_unframe(kocr_ctx* ctx, float* d_boxes, const int32_t* d_off, const int32_t* d_counts, const double* d_axes, int N) {
  if (N == 0) return KOCR_OK;
  ProfScope ps(ctx, "blocks_unframe", 0, 0);
  hipLaunchKernelGGL(blocks_unframe_kernel, dim3(N), dim3(256), 0, ctx->stream, d_boxes, d_off, d_counts, d_axes);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}
