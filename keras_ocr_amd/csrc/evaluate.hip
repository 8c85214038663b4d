// evaluate.hip — evaluation.score on the device (kocr_iou_table / kocr_score; reference evaluation.py:13-53, :56-147).
// The rule is tests/evaluation_statement.py ("Evaluation"): every float64 operation below is one of
// the statement's, in its order; this file is compiled with -ffp-contract=off so that none is fused.
#include "common.h"
#include <algorithm>

namespace {

constexpr int EV_LANES = 64;  // one wave per block, one (truth, prediction) pair per lane
// A lane's LDS slice, in doubles: the two triangles of each quad (2 x 2 x 3 corners) and the two ping-pong polygons of the
// clipping.  A triangle clipped by three half-planes has at most 3 -> 4 -> 6 -> 9 corners whatever the signs of the inside
// tests are (a corner inside emits at most two, one outside at most one, and the two alternate at best).
constexpr int EV_POLY_MAX = 9;
constexpr int EV_TRI = 2 * 2 * 3 * 2, EV_POLY = EV_POLY_MAX * 2, EV_SLOTS = EV_TRI + 2 * EV_POLY;

struct P2 {
  double x, y;
};

__device__ inline double ev_cross(P2 o, P2 a, P2 b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); }
__device__ inline bool ev_same(P2 a, P2 b) { return a.x == b.x && a.y == b.y; }

// a lane's slice is a column of the block's [EV_SLOTS][EV_LANES] array: slot k of every lane side by side, no bank conflicts
#define EV_AT(base, k) (base)[(k) * EV_LANES]

__device__ inline P2 ev_load(const double* s, int corner) { return {EV_AT(s, 2 * corner), EV_AT(s, 2 * corner + 1)}; }
__device__ inline void ev_store(double* s, int corner, P2 p) {
  EV_AT(s, 2 * corner) = p.x;
  EV_AT(s, 2 * corner + 1) = p.y;
}

// statement: ccw_triangle -- (a, b, c) when its area2 > 0, else (c, b, a)
__device__ inline void ev_store_tri(double* s, P2 a, P2 b, P2 c) {
  double s1 = 0.0;
  s1 = s1 + a.x * b.y;
  s1 = s1 + b.x * c.y;
  s1 = s1 + c.x * a.y;
  double s2 = 0.0;
  s2 = s2 + a.y * b.x;
  s2 = s2 + b.y * c.x;
  s2 = s2 + c.y * a.x;
  const bool keep = s1 - s2 > 0;
  ev_store(s, 0, keep ? a : c);
  ev_store(s, 1, b);
  ev_store(s, 2, keep ? c : a);
}

// the three corners left when corner j of (p0, p1, p2, p3) is taken away, in their order
__device__ inline void ev_store_rest(double* s, int j, P2 p0, P2 p1, P2 p2, P2 p3) {
  ev_store_tri(s, j == 0 ? p1 : p0, j <= 1 ? p2 : p1, j == 3 ? p2 : p3);
}

__device__ inline bool ev_ear(P2 a, P2 b, P2 c, P2 q) {
  if (ev_cross(a, b, c) <= 0) return false;
  return !(ev_cross(a, b, q) >= 0 && ev_cross(b, c, q) >= 0 && ev_cross(c, a, q) >= 0);
}

// statement: triangulate_quad.  Writes 0, 1 or 2 counter-clockwise triangles of 6 doubles each to `tri`, returns how many.
__device__ int ev_triangulate(P2 q0, P2 q1, P2 q2, P2 q3, double a2, double* tri) {
  const bool fwd = a2 > 0;
  const P2 p0 = fwd ? q0 : q3, p1 = fwd ? q1 : q2, p2 = fwd ? q2 : q1, p3 = fwd ? q3 : q0;
  const bool k0 = !ev_same(p0, p3), k1 = !ev_same(p1, p0), k2 = !ev_same(p2, p1), k3 = !ev_same(p3, p2);
  const int kept = (int)k0 + (int)k1 + (int)k2 + (int)k3;
  if (kept < 3) return 0;
  if (kept == 3) {
    ev_store_rest(tri, !k0 ? 0 : !k1 ? 1 : !k2 ? 2 : 3, p0, p1, p2, p3);
    return 1;
  }
  if (ev_ear(p3, p0, p1, p2)) {
    ev_store_tri(tri, p3, p0, p1);
    ev_store_rest(tri + 6 * EV_LANES, 0, p0, p1, p2, p3);
  } else if (ev_ear(p0, p1, p2, p3)) {
    ev_store_tri(tri, p0, p1, p2);
    ev_store_rest(tri + 6 * EV_LANES, 1, p0, p1, p2, p3);
  } else if (ev_ear(p1, p2, p3, p0)) {
    ev_store_tri(tri, p1, p2, p3);
    ev_store_rest(tri + 6 * EV_LANES, 2, p0, p1, p2, p3);
  } else if (ev_ear(p2, p3, p0, p1)) {
    ev_store_tri(tri, p2, p3, p0);
    ev_store_rest(tri + 6 * EV_LANES, 3, p0, p1, p2, p3);
  } else {
    return 0;
  }
  return 2;
}

// statement: clip_triangle + abs(area2) / 2 of what is left (0 for fewer than three corners)
__device__ double ev_clip_area(const double* ta, const double* tb, double* buf0, double* buf1) {
  double* in = buf0;
  double* out = buf1;
  for (int c = 0; c < 3; ++c) ev_store(out, c, ev_load(ta, c));
  int n_out = 3;
  for (int e = 0; e < 3; ++e) {
    double* t = in;
    in = out;
    out = t;
    const int n_in = n_out;
    n_out = 0;
    if (n_in == 0) break;
    const P2 a = ev_load(tb, e), b = ev_load(tb, e == 2 ? 0 : e + 1);
    const double d1x = b.x - a.x, d1y = b.y - a.y;
    P2 s = ev_load(in, n_in - 1);
    bool s_in = d1x * (s.y - a.y) - d1y * (s.x - a.x) >= 0;
    for (int k = 0; k < n_in; ++k) {
      const P2 p = ev_load(in, k);
      const bool p_in = d1x * (p.y - a.y) - d1y * (p.x - a.x) >= 0;
      if (p_in != s_in) {
        const double d2x = p.x - s.x, d2y = p.y - s.y;
        const double den = d1x * d2y - d1y * d2x;
        const double tt = ((s.x - a.x) * d2y - (s.y - a.y) * d2x) / den;
        const P2 x = {a.x + tt * d1x, a.y + tt * d1y};
        if (n_out < EV_POLY_MAX) ev_store(out, n_out++, x);
      }
      if (p_in && n_out < EV_POLY_MAX) ev_store(out, n_out++, p);
      s = p;
      s_in = p_in;
    }
  }
  if (n_out < 3) return 0.0;
  double s1 = 0.0;
  for (int k = 0; k < n_out; ++k) s1 = s1 + EV_AT(out, 2 * k) * EV_AT(out, 2 * (k + 1 == n_out ? 0 : k + 1) + 1);
  double s2 = 0.0;
  for (int k = 0; k < n_out; ++k) s2 = s2 + EV_AT(out, 2 * k + 1) * EV_AT(out, 2 * (k + 1 == n_out ? 0 : k + 1));
  return fabs(s1 - s2) / 2;
}

__device__ inline double ev_quad_area2(P2 q0, P2 q1, P2 q2, P2 q3) {
  double s1 = 0.0;
  s1 = s1 + q0.x * q1.y;
  s1 = s1 + q1.x * q2.y;
  s1 = s1 + q2.x * q3.y;
  s1 = s1 + q3.x * q0.y;
  double s2 = 0.0;
  s2 = s2 + q0.y * q1.x;
  s2 = s2 + q1.y * q2.x;
  s2 = s2 + q2.y * q3.x;
  s2 = s2 + q3.y * q0.x;
  return s1 - s2;
}

__device__ inline P2 ev_corner(const int32_t* q, int c) { return {(double)q[2 * c], (double)q[2 * c + 1]}; }

// the image of flat pair k: the i with pair_off[i] <= k < pair_off[i + 1] (images without pairs have empty ranges)
__device__ inline int ev_image_of(const long long* pair_off, int N, long long k) {
  int lo = 0, hi = N;  // invariant: pair_off[lo] <= k < pair_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pair_off[mid] <= k) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace

// One lane per (truth, prediction) pair of one image; pair k of the flat range belongs to image i = ev_image_of(k), truth
// (k - pair_off[i]) / np_i, prediction (k - pair_off[i]) % np_i.  Nothing a lane computes depends on another lane, so an
// image's pairs carry the same bits whatever else is in the batch.  iou / pair_class may be null.  A pair that overlaps a
// truth that is not ignored is appended to `work` for eval_text_kernel (order irrelevant: each entry is its own pair).
__global__ __launch_bounds__(EV_LANES) void eval_iou_kernel(const int32_t* __restrict__ tq, const int32_t* __restrict__ toff,
                                                             const int32_t* __restrict__ pq, const int32_t* __restrict__ poff,
                                                             const long long* __restrict__ pair_off, int N, long long P,
                                                             double* __restrict__ iou, const uint8_t* __restrict__ ignore,
                                                             double iou_threshold, uint8_t* __restrict__ pair_class,
                                                             EvalWork* __restrict__ work, unsigned* __restrict__ work_count) {
  __shared__ double lds[EV_SLOTS * EV_LANES];
  const long long k = (long long)blockIdx.x * EV_LANES + threadIdx.x;
  if (k >= P) return;
  const int img = ev_image_of(pair_off, N, k);
  const long long local = k - pair_off[img];
  const int np_i = poff[img + 1] - poff[img];
  const int t = toff[img] + (int)(local / np_i), p = poff[img] + (int)(local % np_i);
  const int32_t *qa = tq + (size_t)t * 8, *qb = pq + (size_t)p * 8;
  const P2 a0 = ev_corner(qa, 0), a1 = ev_corner(qa, 1), a2 = ev_corner(qa, 2), a3 = ev_corner(qa, 3);
  const P2 b0 = ev_corner(qb, 0), b1 = ev_corner(qb, 1), b2 = ev_corner(qb, 2), b3 = ev_corner(qb, 3);
  const double a2a = ev_quad_area2(a0, a1, a2, a3), a2b = ev_quad_area2(b0, b1, b2, b3);
  const double area_a = fabs(a2a) / 2, area_b = fabs(a2b) / 2;
  double v = 0.0;
  if (area_a != 0 && area_b != 0) {
    double* mine = lds + threadIdx.x;
    double* tri_a = mine;
    double* tri_b = mine + 12 * EV_LANES;
    double* buf0 = mine + EV_TRI * EV_LANES;
    double* buf1 = buf0 + EV_POLY * EV_LANES;
    const int na = ev_triangulate(a0, a1, a2, a3, a2a, tri_a);
    const int nb = ev_triangulate(b0, b1, b2, b3, a2b, tri_b);
    double inter = 0.0;
    for (int i = 0; i < na; ++i)
      for (int j = 0; j < nb; ++j) {
        const double c = ev_clip_area(tri_a + i * 6 * EV_LANES, tri_b + j * 6 * EV_LANES, buf0, buf1);
        inter = inter + c;  // 0.0 where fewer than three corners are left: the same bits as not adding
      }
    v = inter / (area_a + area_b - inter);
  }
  if (iou) iou[k] = v;
  if (pair_class) {
    uint8_t c = 0;
    if (v >= iou_threshold) {
      if (ignore[t]) {
        c = 3;
      } else {
        c = 1;  // eval_text_kernel decides between 1 and 2
        const unsigned slot = atomicAdd(work_count, 1u);
        work[slot] = {k, t, p};
      }
    }
    pair_class[k] = c;
  }
}

// One wave per listed pair: Levenshtein distance of the two code-point rows by anti-diagonals, the cells of a diagonal
// across the lanes, three diagonals in LDS; then the statement's float64 similarity rule decides class 1 or 2.
__global__ __launch_bounds__(EV_LANES) void eval_text_kernel(const EvalWork* __restrict__ work, const unsigned* __restrict__ work_count,
                                                              const int32_t* __restrict__ ttext, const int32_t* __restrict__ ttoff,
                                                              const int32_t* __restrict__ ptext, const int32_t* __restrict__ ptoff,
                                                              double similarity_threshold, uint8_t* __restrict__ pair_class) {
  __shared__ int32_t a[KOCR_SCORE_MAX_TEXT], b[KOCR_SCORE_MAX_TEXT];
  __shared__ int diag[3][KOCR_SCORE_MAX_TEXT + 1];
  const unsigned count = *work_count;
  const int lane = threadIdx.x;
  for (unsigned w = blockIdx.x; w < count; w += gridDim.x) {
    const EvalWork item = work[w];
    const int n = min(max(ttoff[item.t + 1] - ttoff[item.t], 0), KOCR_SCORE_MAX_TEXT);
    const int m = min(max(ptoff[item.p + 1] - ptoff[item.p], 0), KOCR_SCORE_MAX_TEXT);
    __syncthreads();  // the previous pair's rows are no longer read
    for (int i = lane; i < n; i += EV_LANES) a[i] = ttext[ttoff[item.t] + i];
    for (int j = lane; j < m; j += EV_LANES) b[j] = ptext[ptoff[item.p] + j];
    __syncthreads();
    // diag[d % 3][j] = D[d - j][j], the distance of a[0 .. d - j) and b[0 .. j)
    for (int d = 0; d <= n + m; ++d) {
      int* cur = diag[d % 3];
      const int* prev = diag[(d + 2) % 3];
      const int* prev2 = diag[(d + 1) % 3];
      const int jlo = max(0, d - n), jhi = min(d, m);
      for (int j = jlo + lane; j <= jhi; j += EV_LANES) {
        const int i = d - j;
        int v;
        if (i == 0) v = j;
        else if (j == 0) v = i;
        else v = min(min(prev[j] + 1, prev[j - 1] + 1), prev2[j - 1] + (a[i - 1] != b[j - 1] ? 1 : 0));
        cur[j] = v;
      }
      __syncthreads();
    }
    if (lane == 0) {
      const int dist = diag[(n + m) % 3][m], longest = max(n, m);
      const double sim = longest == 0 ? 1.0 : 1.0 - (double)dist / (double)longest;
      pair_class[item.k] = sim >= similarity_threshold ? 1 : 2;
    }
  }
}

// One block per image: the missed flag of every truth, the unclaimed flag of every prediction, and the three counts
// (integers, so the order of the atomic additions does not matter).
constexpr int EV_REDUCE_THREADS = 256;
__global__ __launch_bounds__(EV_REDUCE_THREADS) void eval_reduce_kernel(const uint8_t* __restrict__ pair_class, const long long* __restrict__ pair_off,
                                                                         const int32_t* __restrict__ toff, const int32_t* __restrict__ poff,
                                                                         const uint8_t* __restrict__ ignore, uint8_t* __restrict__ truth_missed,
                                                                         uint8_t* __restrict__ pred_unclaimed, unsigned long long* __restrict__ counts) {
  __shared__ unsigned block_counts[3];
  const int img = blockIdx.x;
  if (threadIdx.x < 3) block_counts[threadIdx.x] = 0;
  __syncthreads();
  const int t0 = toff[img], nt = toff[img + 1] - t0, p0 = poff[img], np = poff[img + 1] - p0;
  const uint8_t* cls = pair_class + pair_off[img];
  unsigned matched = 0, unclaimed = 0, missed = 0;
  for (int t = threadIdx.x; t < nt; t += EV_REDUCE_THREADS) {
    bool any = false, good = false;
    for (int p = 0; p < np; ++p) {
      const uint8_t c = cls[(size_t)t * np + p];
      any |= c != 0;
      good |= c == 1;
    }
    const bool miss = !ignore[t0 + t] && !any;
    truth_missed[t0 + t] = miss ? 1 : 0;
    matched += good ? 1 : 0;
    missed += miss ? 1 : 0;
  }
  for (int p = threadIdx.x; p < np; p += EV_REDUCE_THREADS) {
    bool any = false;
    for (int t = 0; t < nt; ++t) any |= cls[(size_t)t * np + p] != 0;
    pred_unclaimed[p0 + p] = any ? 0 : 1;
    unclaimed += any ? 0 : 1;
  }
  if (matched) atomicAdd(&block_counts[0], matched);
  if (unclaimed) atomicAdd(&block_counts[1], unclaimed);
  if (missed) atomicAdd(&block_counts[2], missed);
  __syncthreads();
  if (threadIdx.x < 3 && block_counts[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)block_counts[threadIdx.x]);
}

int launch_eval_iou(kocr_ctx* ctx, const EvalBatch& b, double* d_iou, double iou_threshold, uint8_t* d_class, EvalWork* d_work,
                    unsigned* d_work_count) {
  if (b.P == 0) return KOCR_OK;
  ProfScope ps(ctx, "eval_iou", 0, (double)b.P * (64.0 + 9.0));
  const long long blocks = (b.P + EV_LANES - 1) / EV_LANES;
  hipLaunchKernelGGL(eval_iou_kernel, dim3((unsigned)blocks), dim3(EV_LANES), 0, ctx->stream, b.d_tq, b.d_toff, b.d_pq, b.d_poff,
                     b.d_pair_off, b.N, b.P, d_iou, b.d_ignore, iou_threshold, d_class, d_work, d_work_count);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

int launch_eval_text(kocr_ctx* ctx, const EvalBatch& b, const EvalWork* d_work, const unsigned* d_work_count, double similarity_threshold,
                     uint8_t* d_class) {
  if (b.P == 0) return KOCR_OK;
  ProfScope ps(ctx, "eval_text", 0, 0);
  // The list's length is known on the device only.  It holds about one pair per word (a word overlaps its partner and
  // seldom more), so that many one-wave blocks are launched, never more than pairs or than 1024; a longer list is walked
  // with the grid's stride.
  const unsigned blocks = (unsigned)std::min<long long>(std::min(b.P, b.words), 1024);
  hipLaunchKernelGGL(eval_text_kernel, dim3(blocks), dim3(EV_LANES), 0, ctx->stream, d_work, d_work_count, b.d_ttext, b.d_ttoff,
                     b.d_ptext, b.d_ptoff, similarity_threshold, d_class);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

int launch_eval_reduce(kocr_ctx* ctx, const EvalBatch& b, const uint8_t* d_class, uint8_t* d_missed, uint8_t* d_unclaimed, int64_t* d_counts) {
  if (b.N == 0) return KOCR_OK;
  ProfScope ps(ctx, "eval_reduce", 0, 2.0 * (double)b.P);
  hipLaunchKernelGGL(eval_reduce_kernel, dim3(b.N), dim3(EV_REDUCE_THREADS), 0, ctx->stream, d_class, b.d_pair_off, b.d_toff, b.d_poff,
                     b.d_ignore, d_missed, d_unclaimed, (unsigned long long*)d_counts);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}
