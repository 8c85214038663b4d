// warp_geom.h — the scalar half of the crop stage as host/device functions: box ordering, (w, h), the homography of an ordered
// quad and its inverse.  warp.hip and windows.hip compile the SAME functions (float64, fixed operation order,
// -ffp-contract=off), for the host and for the device.
#pragma once
#include "common.h"
#include <cmath>

#define HD __host__ __device__ inline

namespace {

struct P2 {
  double x, y;
};

HD double cross2(P2 o, P2 a, P2 b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); }

// shapely MultiPoint.minimum_rotated_rectangle (tools.py:543-547): min-area rectangle over the
// convex hull's edges.  Returns false for degenerate input (the reference's AttributeError path).
// The arrays the set-up indexes at run time reach it through pointers.  A kernel that must not use scratch hands every lane a
// slice of LDS (windows.hip: BoxWork, SolveWork); the overloads without storage keep them as locals, as warp.hip's kernels
// always did.  The arithmetic is the same either way.
struct HullWork {
  P2 u[4], lower[8], upper[8], hull[8];
};
struct BoxWork {
  P2 in[4], pts[4];
  int idx[4];
  HullWork hull;
};
struct SolveWork {
  double A[8][8], b[8], x[8];
};

HD bool min_rotated_rect(const P2* pts, P2* out, P2* u, P2* lower, P2* upper, P2* hull) {
  int n = 0;
  for (int i = 0; i < 4; ++i) {
    bool dup = false;
    for (int j = 0; j < n; ++j) dup |= (u[j].x == pts[i].x && u[j].y == pts[i].y);
    if (!dup) u[n++] = pts[i];
  }
  if (n < 3) return false;
  for (int i = 1; i < n; ++i)  // insertion sort by (x, y): at most 4 distinct points
    for (int j = i; j > 0 && (u[j].x < u[j - 1].x || (u[j].x == u[j - 1].x && u[j].y < u[j - 1].y)); --j) {
      const P2 t = u[j];
      u[j] = u[j - 1];
      u[j - 1] = t;
    }
  int nl = 0, nu = 0;
  for (int i = 0; i < n; ++i) {
    while (nl >= 2 && cross2(lower[nl - 2], lower[nl - 1], u[i]) <= 0) --nl;
    lower[nl++] = u[i];
  }
  for (int i = n - 1; i >= 0; --i) {
    while (nu >= 2 && cross2(upper[nu - 2], upper[nu - 1], u[i]) <= 0) --nu;
    upper[nu++] = u[i];
  }
  int nh = 0;
  for (int i = 0; i + 1 < nl; ++i) hull[nh++] = lower[i];
  for (int i = 0; i + 1 < nu; ++i) hull[nh++] = upper[i];
  if (nh < 3) return false;
  bool have = false;
  double barea = 0, bux = 0, buy = 0, bumin = 0, bumax = 0, bvmin = 0, bvmax = 0;
  for (int i = 0; i < nh; ++i) {
    const P2 p0 = hull[i], p1 = hull[(i + 1) % nh];
    const double dx = p1.x - p0.x, dy = p1.y - p0.y;
    const double ln = sqrt(dx * dx + dy * dy);
    const double ux = dx / ln, uy = dy / ln;
    double umin = 0, umax = 0, vmin = 0, vmax = 0;
    for (int j = 0; j < nh; ++j) {
      const double uu = hull[j].x * ux + hull[j].y * uy;
      const double vv = -hull[j].x * uy + hull[j].y * ux;
      if (j == 0) {
        umin = umax = uu;
        vmin = vmax = vv;
      } else {
        umin = uu < umin ? uu : umin;
        umax = uu > umax ? uu : umax;
        vmin = vv < vmin ? vv : vmin;
        vmax = vv > vmax ? vv : vmax;
      }
    }
    const double area = (umax - umin) * (vmax - vmin);
    if (!have || area < barea) {
      have = true;
      barea = area;
      bux = ux;
      buy = uy;
      bumin = umin;
      bumax = umax;
      bvmin = vmin;
      bvmax = vmax;
    }
  }
  const double us[4] = {bumin, bumax, bumax, bumin}, vs[4] = {bvmin, bvmin, bvmax, bvmax};
  for (int i = 0; i < 4; ++i) {
    out[i].x = us[i] * bux - vs[i] * buy;
    out[i].y = us[i] * buy + vs[i] * bux;
  }
  return true;
}

HD double dist2(const float* a, const float* b) {
  const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1];
  return sqrt(dx * dx + dy * dy);
}

// Gaussian elimination with partial pivoting, float64 (cv2.getPerspectiveTransform's solve).
HD bool solve8(double A[8][8], double b[8], double x[8]) {
  const int n = 8;
  for (int col = 0; col < n; ++col) {
    int piv = col;
    for (int r = col + 1; r < n; ++r)
      if (fabs(A[r][col]) > fabs(A[piv][col])) piv = r;
    if (A[piv][col] == 0.0) return false;
    if (piv != col) {
      for (int c = 0; c < n; ++c) {
        const double t = A[piv][c];
        A[piv][c] = A[col][c];
        A[col][c] = t;
      }
      const double tb = b[piv];
      b[piv] = b[col];
      b[col] = tb;
    }
    for (int r = col + 1; r < n; ++r) {
      const double f = A[r][col] / A[col][col];
      if (f != 0.0) {
        for (int c = col; c < n; ++c) A[r][c] = A[r][c] - f * A[col][c];
        b[r] = b[r] - f * b[col];
      }
    }
  }
  for (int r = n - 1; r >= 0; --r) {
    double s = b[r];
    for (int c = r + 1; c < n; ++c) s = s - A[r][c] * x[c];
    x[r] = s / A[r][r];
  }
  return true;
}

HD void invert3(const double m[9], double t[9]) {
  double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
             m[2] * (m[3] * m[7] - m[4] * m[6]);
  if (d == 0.0) {
    for (int i = 0; i < 9; ++i) t[i] = 0.0;
    return;
  }
  d = 1.0 / d;
  t[0] = (m[4] * m[8] - m[5] * m[7]) * d;
  t[1] = (m[2] * m[7] - m[1] * m[8]) * d;
  t[2] = (m[1] * m[5] - m[2] * m[4]) * d;
  t[3] = (m[5] * m[6] - m[3] * m[8]) * d;
  t[4] = (m[0] * m[8] - m[2] * m[6]) * d;
  t[5] = (m[2] * m[3] - m[0] * m[5]) * d;
  t[6] = (m[3] * m[7] - m[4] * m[6]) * d;
  t[7] = (m[1] * m[6] - m[0] * m[7]) * d;
  t[8] = (m[0] * m[4] - m[1] * m[3]) * d;
}

// cv2.getPerspectiveTransform(src, dst) (tools.py:96-106) and its inverse.  src / dst: 4x2 float32.  m_fwd may be null.
HD bool quad_homography(const float* src, const float* dst, double* m_fwd, double* m_inv, double (*A)[8], double* b, double* x) {
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) A[i][j] = 0.0;
  for (int i = 0; i < 4; ++i) {
    const double sx = src[2 * i], sy = src[2 * i + 1], dx = dst[2 * i], dy = dst[2 * i + 1];
    A[i][0] = A[i + 4][3] = sx;
    A[i][1] = A[i + 4][4] = sy;
    A[i][2] = A[i + 4][5] = 1.0;
    A[i][6] = -sx * dx;
    A[i][7] = -sy * dx;
    A[i + 4][6] = -sx * dy;
    A[i + 4][7] = -sy * dy;
    b[i] = dx;
    b[i + 4] = dy;
  }
  if (!solve8(A, b, x)) return false;
  const double M[9] = {x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], 1.0};
  if (m_fwd)
    for (int i = 0; i < 9; ++i) m_fwd[i] = M[i];
  invert3(M, m_inv);
  return true;
}

HD bool quad_homography(const float* src, const float* dst, double* m_fwd, double* m_inv, SolveWork& wk) {
  return quad_homography(src, dst, m_fwd, m_inv, wk.A, wk.b, wk.x);
}
HD bool quad_homography(const float* src, const float* dst, double* m_fwd, double* m_inv) {
  double A[8][8], b[8], x[8];
  return quad_homography(src, dst, m_fwd, m_inv, A, b, x);
}

// tools.get_rotated_box (tools.py:533-581): 4 points -> [tl, tr, br, bl] float32
// idx: {0, 1, 2, 3} on entry
HD void rotated_box(const float* box, float* ob, P2* in, P2* pts, int* idx, P2* u, P2* lower, P2* upper, P2* hull) {
  for (int i = 0; i < 4; ++i) in[i] = {(double)box[2 * i], (double)box[2 * i + 1]};
  if (!min_rotated_rect(in, pts, u, lower, upper, hull))
    for (int i = 0; i < 4; ++i) pts[i] = in[i];
  for (int i = 1; i < 4; ++i)  // stable insertion sort by x (np.argsort(kind="stable"))
    for (int j = i; j > 0 && pts[idx[j]].x < pts[idx[j - 1]].x; --j) {
      const int t = idx[j];
      idx[j] = idx[j - 1];
      idx[j - 1] = t;
    }
  const P2 l0 = pts[idx[0]], l1 = pts[idx[1]], r0 = pts[idx[2]], r1 = pts[idx[3]];
  P2 tl, bl, tr, br;
  if (l1.y < l0.y) {
    tl = l1;
    bl = l0;
  } else {
    tl = l0;
    bl = l1;
  }
  const double d0 = sqrt((tl.x - r0.x) * (tl.x - r0.x) + (tl.y - r0.y) * (tl.y - r0.y));
  const double d1 = sqrt((tl.x - r1.x) * (tl.x - r1.x) + (tl.y - r1.y) * (tl.y - r1.y));
  if (d0 > d1) {
    br = r0;
    tr = r1;
  } else {
    br = r1;
    tr = r0;
  }
  ob[0] = (float)tl.x;
  ob[1] = (float)tl.y;
  ob[2] = (float)tr.x;
  ob[3] = (float)tr.y;
  ob[4] = (float)br.x;
  ob[5] = (float)br.y;
  ob[6] = (float)bl.x;
  ob[7] = (float)bl.y;
}

HD void rotated_box(const float* box, float* ob, BoxWork& wk) {
  for (int i = 0; i < 4; ++i) wk.idx[i] = i;
  rotated_box(box, ob, wk.in, wk.pts, wk.idx, wk.hull.u, wk.hull.lower, wk.hull.upper, wk.hull.hull);
}
HD void rotated_box(const float* box, float* ob) {
  P2 in[4], pts[4], u[4], lower[8], upper[8], hull[8];
  int idx[4] = {0, 1, 2, 3};
  rotated_box(box, ob, in, pts, idx, u, lower, upper, hull);
}

// tools.warpBox's scalar half (tools.py:86-107), margin 0, on an ORDERED source quad q [tl, tr, br, bl] (4x2 float32).
// rc: 0 ok, 1 zero width/height (the reference raises ZeroDivisionError), 2 singular system.
HD int warp_prepare_quad(const float* q, int target_h, int target_w, WarpParam* out, double (*A)[8], double* b, double* x) {
  // ---- get_rotated_width_height (tools.py:41-57) ----
  const int w = (int)((dist2(q + 0, q + 2) + dist2(q + 4, q + 6)) / 2);
  const int h = (int)((dist2(q + 0, q + 6) + dist2(q + 2, q + 4)) / 2);
  if (w == 0 || h == 0) return 1;
  // ---- scale, destination quad, homography (tools.py:95-106) ----
  const double sw = (double)target_w / (double)w, sh = (double)target_h / (double)h;
  const double scale = sw < sh ? sw : sh;
  const float dst[8] = {0.f, 0.f, (float)(scale * w), 0.f, (float)(scale * w), (float)(scale * h),
                        0.f, (float)(scale * h)};
  if (!quad_homography(q, dst, nullptr, out->mi, A, b, x)) return 2;
  const int cw = (int)(scale * w), ch = (int)(scale * h);
  out->cw = cw < target_w ? cw : target_w;
  out->ch = ch < target_h ? ch : target_h;
  out->pad = 0;
  return 0;
}

HD int warp_prepare_quad(const float* q, int target_h, int target_w, WarpParam* out, SolveWork& wk) {
  return warp_prepare_quad(q, target_h, target_w, out, wk.A, wk.b, wk.x);
}
HD int warp_prepare_quad(const float* q, int target_h, int target_w, WarpParam* out) {
  double A[8][8], b[8], x[8];
  return warp_prepare_quad(q, target_h, target_w, out, A, b, x);
}

// ... on a box as getBoxes gives it: 4x2 float32, ordered by get_rotated_box first.
HD int warp_prepare_hd(const float* box, int target_h, int target_w, WarpParam* out, float* ordered_box) {
  float ob[8];
  rotated_box(box, ob);
  if (ordered_box)
    for (int i = 0; i < 8; ++i) ordered_box[i] = ob[i];
  return warp_prepare_quad(ob, target_h, target_w, out);
}

// Orientation (tests/orientation_statement.py; DESIGN.md section 4, "Orientation"): candidate c (0 or 1) of a box reads its
// ordered box ob through t = b + 2 c quarter turns, b = 1 for a tall box in mode KOCR_ORIENT_ANY (float(h) >= tall_ratio *
// float(w) in float64, (w, h) = get_rotated_width_height(ob)), else 0: the source quad is q[i] = ob[(i + t) % 4], the same
// four float32 corners renamed, and everything behind it is warp_prepare_quad.  t = 0 is warp_prepare_hd, operation for
// operation.  quad: q (8 floats); rc as warp_prepare_quad.
HD int warp_prepare_turned_hd(const float* box, int mode, double tall_ratio, int c, int target_h, int target_w, WarpParam* out,
                              int* turn, float* quad) {
  float ob[8];
  rotated_box(box, ob);
  const int w = (int)((dist2(ob + 0, ob + 2) + dist2(ob + 4, ob + 6)) / 2);
  const int h = (int)((dist2(ob + 0, ob + 6) + dist2(ob + 2, ob + 4)) / 2);
  const bool tall = mode == KOCR_ORIENT_ANY && (double)h >= tall_ratio * (double)w;
  const int t = (tall ? 1 : 0) + 2 * c;
  for (int i = 0; i < 4; ++i) {
    quad[2 * i] = ob[2 * ((i + t) % 4)];
    quad[2 * i + 1] = ob[2 * ((i + t) % 4) + 1];
  }
  *turn = t;
  return warp_prepare_quad(quad, target_h, target_w, out);
}

}  // namespace

#undef HD
