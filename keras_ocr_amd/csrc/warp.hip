// warp.hip — word-box crops for the recogniser.
//
// Replaces the per-box host loop of Recognizer.recognize_from_boxes (recognition.py:506-526):
// cv2.cvtColor(RGB2GRAY) of the whole image, tools.warpBox per box (tools.py:61-117:
// get_rotated_box :533-581, get_rotated_width_height :41-57, cv2.getPerspectiveTransform,
// cv2.warpPerspective, paste into a zero 31x200 canvas) and the float32 /255.
//
// Set-up (float64, fixed operation order, -ffp-contract=off; the SAME functions compile for host and device, and
// the pipeline runs them ON THE DEVICE, one thread per box, straight from the box buffer getBoxes filled -- no
// host round trip between boxes and crops): box ordering, (w,h), scale, 8x8 LU solve for the homography, 3x3
// adjugate inverse.  Warp: one thread per crop pixel maps (x,y) through M^-1 in float64, rounds to 1/32 px (half
// to even), gathers the 4 RGB taps from the uint8 image (coalescing is bounded by the box
// orientation; the whole crop stage moves ~25 KB per word), converts each tap to gray with
// OpenCV's 15-bit integer coefficients, blends with 15-bit bilinear weights, BORDER_CONSTANT
// 0, and writes float32 gray/255 — the gray image is never materialised.
#include "warp_geom.h"
#include <algorithm>

#define HD __host__ __device__


int warp_prepare(const float* box, int target_h, int target_w, WarpParam* out, float* ordered_box) {
  return warp_prepare_hd(box, target_h, target_w, out, ordered_box);
}

int warp_prepare_turned(const float* box, int mode, double tall_ratio, int c, int target_h, int target_w, WarpParam* out, int* turn,
                        float* quad) {
  return warp_prepare_turned_hd(box, mode, tall_ratio, c, target_h, target_w, out, turn, quad);
}

// One thread per box slot (image k, slot b < cap): boxes[k][b] -> prm[offset(k) + b], where offset(k) = number of
// boxes of the images before k.  status: atomicMax of the per-box return code (0 ok, 1 zero size, 2 singular).
__global__ void warp_prepare_kernel(const float* __restrict__ boxes, const int* __restrict__ counts, int N, int cap,
                                    int th, int tw, WarpParam* __restrict__ prm, int* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * cap) return;
  const int k = i / cap, b = i - k * cap;
  if (b >= counts[k]) return;
  long off = 0;
  for (int j = 0; j < k; ++j) off += counts[j];
  WarpParam p;
  const int rc = warp_prepare_hd(boxes + (size_t)i * 8, th, tw, &p, nullptr);
  if (rc != 0) {
    // keep the slot harmless: an empty crop
    for (int q = 0; q < 9; ++q) p.mi[q] = 0.0;
    p.cw = p.ch = 0;
    p.pad = 0;
    atomicMax(status, rc);
  }
  p.img = k;
  prm[off + b] = p;
}

int launch_warp_prepare(kocr_ctx* ctx, const float* d_boxes, const int* d_counts, int N, int cap, int th, int tw,
                        WarpParam* d_prm, int* d_status) {
  if (N <= 0 || cap <= 0) return KOCR_OK;
  ProfScope ps(ctx, "warp_prepare", 0, 0);
  const int n = N * cap;
  hipLaunchKernelGGL(warp_prepare_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, d_boxes, d_counts, N, cap, th, tw,
                     d_prm, d_status);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// The turned set-up: one thread per (box slot, candidate), boxes and counts read exactly as warp_prepare_kernel reads them.
// Crop 2 (offset(k) + b) + c is candidate c of box b of image k -- a word's two crops sit side by side --, with its turn
// and its source quad beside the WarpParam.
__global__ void warp_prepare_turned_kernel(const float* __restrict__ boxes, const int* __restrict__ counts, int N, int cap, int mode,
                                           double tall_ratio, int th, int tw, WarpParam* __restrict__ prm, int* __restrict__ turns,
                                           float* __restrict__ quads, int* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)N * cap * 2) return;
  const long slot = i >> 1;
  const int c = (int)(i & 1);
  const int k = (int)(slot / cap), b = (int)(slot - (long)k * cap);
  if (b >= counts[k]) return;
  long off = 0;
  for (int j = 0; j < k; ++j) off += counts[j];
  WarpParam p;
  int t;
  float q[8];
  const int rc = warp_prepare_turned_hd(boxes + (size_t)slot * 8, mode, tall_ratio, c, th, tw, &p, &t, q);
  if (rc != 0) {
    // keep the slot harmless: an empty crop
    for (int j = 0; j < 9; ++j) p.mi[j] = 0.0;
    p.cw = p.ch = 0;
    p.pad = 0;
    atomicMax(status, rc);
  }
  p.img = k;
  const size_t m = 2 * (size_t)(off + b) + c;
  prm[m] = p;
  turns[m] = t;
  for (int j = 0; j < 8; ++j) quads[m * 8 + j] = q[j];
}

int launch_warp_prepare_turned(kocr_ctx* ctx, const float* d_boxes, const int* d_counts, int N, int cap, int mode, double tall_ratio,
                               int th, int tw, WarpParam* d_prm, int* d_turns, float* d_quads, int* d_status) {
  if (N <= 0 || cap <= 0) return KOCR_OK;
  ProfScope ps(ctx, "warp_prepare_turned", 0, 0);
  const long n = (long)N * cap * 2;
  hipLaunchKernelGGL(warp_prepare_turned_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_boxes, d_counts, N, cap,
                     mode, tall_ratio, th, tw, d_prm, d_turns, d_quads, d_status);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// General quads (tools.warpBox with margin / skip_rotate / target size from the box, tools.py:61-117): the caller
// supplies the ordered source quad and the destination quad of every crop; the device solves the homographies.
__global__ void warp_quads_kernel(const float* __restrict__ src, const float* __restrict__ dst, const int* __restrict__ img,
                                  const int* __restrict__ cw, const int* __restrict__ ch, int M, WarpParam* __restrict__ prm,
                                  double* __restrict__ m_fwd, int* __restrict__ status) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  WarpParam p;
  double fwd[9];
  if (!quad_homography(src + (size_t)m * 8, dst + (size_t)m * 8, fwd, p.mi)) {
    for (int q = 0; q < 9; ++q) p.mi[q] = fwd[q] = 0.0;
    atomicMax(status, 2);
  }
  p.img = img[m];
  p.cw = cw[m];
  p.ch = ch[m];
  p.pad = 0;
  prm[m] = p;
  if (m_fwd)
    for (int q = 0; q < 9; ++q) m_fwd[(size_t)m * 9 + q] = fwd[q];
}

int launch_warp_quads(kocr_ctx* ctx, const float* d_src, const float* d_dst, const int* d_img, const int* d_cw,
                      const int* d_ch, int M, WarpParam* d_prm, double* d_mfwd, int* d_status) {
  if (M <= 0) return KOCR_OK;
  hipLaunchKernelGGL(warp_quads_kernel, dim3((M + 63) / 64), dim3(64), 0, ctx->stream, d_src, d_dst, d_img, d_cw, d_ch, M,
                     d_prm, d_mfwd, d_status);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

__global__ void warp_kernel(const uint8_t* __restrict__ img, int H, int W, const WarpParam* __restrict__ prm,
                            int th, int tw, float* __restrict__ crops) {
  const int m = blockIdx.y;
  const WarpParam p = prm[m];
  const uint8_t* im = img + (size_t)p.img * H * W * 3;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < th * tw; i += gridDim.x * blockDim.x) {
    const int y = i / tw, x = i - y * tw;
    float v = 0.f;
    if (x < p.cw && y < p.ch) {
      const double xd = (double)x, yd = (double)y;
      const double X0 = (p.mi[0] * xd + p.mi[1] * yd) + p.mi[2];
      const double Y0 = (p.mi[3] * xd + p.mi[4] * yd) + p.mi[5];
      const double W0 = (p.mi[6] * xd + p.mi[7] * yd) + p.mi[8];
      const double Wi = W0 != 0.0 ? 32.0 / W0 : 0.0;
      const double fX = fmax(-2147483648.0, fmin(2147483647.0, X0 * Wi));
      const double fY = fmax(-2147483648.0, fmin(2147483647.0, Y0 * Wi));
      const long X = (long)rint(fX), Y = (long)rint(fY);  // saturate_cast<int>: half to even
      const long sx = X >> 5, sy = Y >> 5;
      const int ax = (int)(X & 31), ay = (int)(Y & 31);
      auto tap = [&](long yy, long xx) -> int {
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) return 0;
        const uint8_t* q = im + ((size_t)yy * W + xx) * 3;
        // cv2.cvtColor(RGB2GRAY), uint8: 15-bit fixed point          (recognition.py:507-510)
        return (q[0] * 9798 + q[1] * 19235 + q[2] * 3735 + (1 << 14)) >> 15;
      };
      const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32;
      const int w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
      const int acc = w00 * tap(sy, sx) + w01 * tap(sy, sx + 1) + w10 * tap(sy + 1, sx) + w11 * tap(sy + 1, sx + 1);
      v = (float)((acc + (1 << 14)) >> 15) / 255.0f;  // recognition.py:524
    }
    crops[(size_t)m * th * tw + i] = v;
  }
}

int launch_warp(kocr_ctx* ctx, const uint8_t* d_img, int H, int W, const WarpParam* d_prm, int M, int th,
                int tw, float* d_crops) {
  if (M <= 0) return KOCR_OK;
  ProfScope ps(ctx, "warp_crops", 0, (double)M * th * tw * (4.0 + 12.0));
  const int bx = (th * tw + 255) / 256;
  for (int s = 0; s < M; s += 65535) {
    const int mb = std::min(65535, M - s);
    hipLaunchKernelGGL(warp_kernel, dim3(bx, mb), dim3(256), 0, ctx->stream, d_img, H, W, d_prm + s, th, tw,
                       d_crops + (size_t)s * th * tw);
  }
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}


// Float images (round 5): cvtColor(RGB2GRAY) + warpPerspective of a float32 image work in float (recognition.py:507-526 hands
// cv2 the image's own type): gray = (0.299 R + 0.587 G) + 0.114 B per tap in float32, the same 1/32-pixel source coordinates
// as the uint8 kernel (OpenCV's remap tables), FLOAT weights a / 32, four products summed in the order
// t00 w00 + t01 w01 + t10 w10 + t11 w11, constant-0 border; NO division by 255 (the caller's, recognition.py:524).
// C = 3 (RGB) or 1 (already gray).  -ffp-contract=off: equals oracle/tools.py::warp_box_float's arithmetic.
__global__ void warp_f32_kernel(const float* __restrict__ img, int H, int W, int C, const WarpParam* __restrict__ prm, int th, int tw,
                                float* __restrict__ crops) {
  const int m = blockIdx.y;
  const WarpParam p = prm[m];
  const float* im = img + (size_t)p.img * H * W * C;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < th * tw; i += gridDim.x * blockDim.x) {
    const int y = i / tw, x = i - y * tw;
    float v = 0.f;
    if (x < p.cw && y < p.ch) {
      const double xd = (double)x, yd = (double)y;
      const double X0 = (p.mi[0] * xd + p.mi[1] * yd) + p.mi[2];
      const double Y0 = (p.mi[3] * xd + p.mi[4] * yd) + p.mi[5];
      const double W0 = (p.mi[6] * xd + p.mi[7] * yd) + p.mi[8];
      const double Wi = W0 != 0.0 ? 32.0 / W0 : 0.0;
      const double fX = fmax(-2147483648.0, fmin(2147483647.0, X0 * Wi));
      const double fY = fmax(-2147483648.0, fmin(2147483647.0, Y0 * Wi));
      const long X = (long)rint(fX), Y = (long)rint(fY);
      const long sx = X >> 5, sy = Y >> 5;
      const float ax = (float)((double)(X & 31) / 32.0), ay = (float)((double)(Y & 31) / 32.0);
      auto tap = [&](long yy, long xx) -> float {
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) return 0.f;
        const float* q = im + ((size_t)yy * W + xx) * C;
        return C == 3 ? (q[0] * 0.299f + q[1] * 0.587f) + q[2] * 0.114f : q[0];
      };
      const float one = 1.f;
      v = ((tap(sy, sx) * ((one - ax) * (one - ay)) + tap(sy, sx + 1) * (ax * (one - ay))) + tap(sy + 1, sx) * ((one - ax) * ay)) +
          tap(sy + 1, sx + 1) * (ax * ay);
    }
    crops[(size_t)m * th * tw + i] = v;
  }
}

int launch_warp_f32(kocr_ctx* ctx, const float* d_img, int H, int W, int C, const WarpParam* d_prm, int M, int th, int tw, float* d_crops) {
  if (M <= 0) return KOCR_OK;
  ProfScope ps(ctx, "warp_crops_f32", 0, (double)M * th * tw * (4.0 + 16.0 * C));
  const int bx = (th * tw + 255) / 256;
  for (int s = 0; s < M; s += 65535) {
    const int mb = std::min(65535, M - s);
    hipLaunchKernelGGL(warp_f32_kernel, dim3(bx, mb), dim3(256), 0, ctx->stream, d_img, H, W, C, d_prm + s, th, tw,
                       d_crops + (size_t)s * th * tw);
  }
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}


// ---------------------------------------------------------------------------------------------------------------------
// Detector training targets: detection.compute_maps (detection.py:106-198) with tools.fix_line (tools.py:584-600) for a
// batch of pages.  The reference warps a Gaussian heat-map onto the WHOLE half-resolution map for every character and for
// every link between neighbours; a warp is non-zero only near its quad, so here each quad visits a pixel box.  Statement:
// tests/maps_statement.py, held bit for bit.
//   maps_char_kernel   one thread per character: rotated box, float32 centre ((p0 + p1) + p2) + p3 then / 4
//   maps_line_kernel   one wave per line: rank sort of the centres by x and by y (ties by index), orientation from the
//                      pairwise float32 sums, then per ordered character its quad slot and the slot of the link ending at
//                      it: homography from the heat-map rectangle, inverse (zero when singular), pixel box
//   maps_accum_kernel  one block per (slot, quarter of its box): the warp arithmetic of warp_kernel on the 1-channel
//                      heat-map, integer atomic adds into int32 text / link planes (exact in any order)
//   maps_finish_kernel clip to 255, then a 256-entry table of float32 v / 255 into the interleaved float32 maps
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int MAPS_LINE_THREADS = 64;
constexpr int MAPS_ACCUM_THREADS = 256;
constexpr int MAPS_ACCUM_SPLIT = 4;  // blocks per slot (grid.y); a quad's box is usually one block's worth of pixels

HD float clamp0(float v) { return v < 0.f ? 0.f : v; }  // max(v, 0) (detection.py:127-129)

// numpy's pairwise float32 sum (np.add.reduce) of d[k] = v[k + 1] - v[k], k < n, with v[k] = c[2 * perm[k] + comp]:
// below 8 terms a sequential sum from -0.0; up to 128, eight strided partial sums combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))
// and the remainder in order; above 128 a split at n / 2 rounded down to a multiple of 8 (an explicit stack: no recursion).
struct DiffSeq {
  const float* c;
  const int* perm;
  int comp;
  __device__ float v(int k) const { return c[2 * perm[k] + comp]; }
  __device__ float d(int k) const { return v(k + 1) - v(k); }
};

__device__ float pairwise_leaf(const DiffSeq& s, int st, int n) {
  if (n < 8) {
    float r = -0.0f;
    for (int i = 0; i < n; ++i) r = r + s.d(st + i);
    return r;
  }
  float r[8];
  for (int j = 0; j < 8; ++j) r[j] = s.d(st + j);
  int i = 8;
  for (; i < n - n % 8; i += 8)
    for (int j = 0; j < 8; ++j) r[j] = r[j] + s.d(st + i + j);
  float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res = res + s.d(st + i);
  return res;
}

__device__ float pairwise_diff_sum(const DiffSeq& s, int n) {
  struct Task {
    int st, n, combine;
  };
  Task tasks[96];
  float vals[48];
  int nt = 0, nv = 0;
  tasks[nt++] = {0, n, 0};
  while (nt > 0) {
    const Task t = tasks[--nt];
    if (t.combine) {
      const float b = vals[--nv];
      const float a = vals[--nv];
      vals[nv++] = a + b;
    } else if (t.n <= 128) {
      vals[nv++] = pairwise_leaf(s, t.st, t.n);
    } else {
      int n2 = t.n / 2;
      n2 -= n2 % 8;
      tasks[nt++] = {0, 0, 1};
      tasks[nt++] = {t.st + n2, t.n - n2, 0};
      tasks[nt++] = {t.st, n2, 0};
    }
  }
  return vals[0];
}

// One character after ordering (detection.py:125-165): the clamped half-scale quad and the two link endpoints, float32 in
// the reference's operation order.
HD void char_geometry(const float* ob, bool vertical, float* quad, float* lp) {
  const float x1 = clamp0(ob[0]), y1 = clamp0(ob[1]), x2 = clamp0(ob[2]), y2 = clamp0(ob[3]);
  const float x3 = clamp0(ob[4]), y3 = clamp0(ob[5]), x4 = clamp0(ob[6]), y4 = clamp0(ob[7]);
  const float yc = (((y4 + y1) + y3) + y2) / 4.f;
  const float xc = (((x1 + x2) + x3) + x4) / 4.f;
  if (!vertical) {
    lp[0] = ((xc + (x1 + x2) / 2.f) / 2.f) / 2.f;
    lp[1] = ((yc + (y1 + y2) / 2.f) / 2.f) / 2.f;
    lp[2] = ((xc + (x3 + x4) / 2.f) / 2.f) / 2.f;
    lp[3] = ((yc + (y3 + y4) / 2.f) / 2.f) / 2.f;
  } else {
    lp[0] = ((xc + (x1 + x4) / 2.f) / 2.f) / 2.f;
    lp[1] = ((yc + (y1 + y4) / 2.f) / 2.f) / 2.f;
    lp[2] = ((xc + (x2 + x3) / 2.f) / 2.f) / 2.f;
    lp[3] = ((yc + (y2 + y3) / 2.f) / 2.f) / 2.f;
  }
  const float q[8] = {x1, y1, x2, y2, x3, y3, x4, y4};
  for (int i = 0; i < 8; ++i) quad[i] = q[i] / 2.f;
}

// A denominator a x + b y + c of one strict sign at the four given points, with a relative margin.
HD bool one_sign(double a, double b, double c, const double* xs, const double* ys) {
  int pos = 0, neg = 0;
  for (int i = 0; i < 4; ++i) {
    const double d = (a * xs[i] + b * ys[i]) + c;
    const double tol = 1e-9 * ((fabs(a * xs[i]) + fabs(b * ys[i])) + fabs(c));
    pos += d > tol;
    neg += d < -tol;
  }
  return pos == 4 || neg == 4;
}

// The slot of one quad: inverse homography of the heat-map rectangle [0, hw] x [0, hh] onto `quad` (zero when the system
// or the matrix is singular: cv2 then samples the heat-map's (0, 0) everywhere) and a pixel box that holds every map pixel
// whose warp can be non-zero: the forward images of the source rectangle grown by 2 px, plus 1 map pixel, when the forward
// denominator has one strict sign at those corners and the inverse one at the map's corners; otherwise the whole map.
HD void quad_slot(const float* quad, int hh, int hw, int h, int w, MapSlot* s) {
  const float src[8] = {0.f, 0.f, (float)hw, 0.f, (float)hw, (float)hh, 0.f, (float)hh};
  double fwd[9];
  if (!quad_homography(src, quad, fwd, s->mi))
    for (int i = 0; i < 9; ++i) s->mi[i] = 0.0;
  s->x0 = 0;
  s->y0 = 0;
  s->x1 = w - 1;
  s->y1 = h - 1;
  const double* mi = s->mi;
  const double mx[4] = {0.0, (double)(w - 1), 0.0, (double)(w - 1)}, my[4] = {0.0, 0.0, (double)(h - 1), (double)(h - 1)};
  if (!one_sign(mi[6], mi[7], mi[8], mx, my)) return;
  const double sx[4] = {-2.0, hw + 2.0, hw + 2.0, -2.0}, sy[4] = {-2.0, -2.0, hh + 2.0, hh + 2.0};
  if (!one_sign(fwd[6], fwd[7], fwd[8], sx, sy)) return;
  double xmin = 0, xmax = 0, ymin = 0, ymax = 0;
  for (int i = 0; i < 4; ++i) {
    const double d = (fwd[6] * sx[i] + fwd[7] * sy[i]) + fwd[8];
    const double X = ((fwd[0] * sx[i] + fwd[1] * sy[i]) + fwd[2]) / d;
    const double Y = ((fwd[3] * sx[i] + fwd[4] * sy[i]) + fwd[5]) / d;
    if (!(fabs(X) < 1e9 && fabs(Y) < 1e9)) return;  // also NaN
    xmin = i ? fmin(xmin, X) : X;
    xmax = i ? fmax(xmax, X) : X;
    ymin = i ? fmin(ymin, Y) : Y;
    ymax = i ? fmax(ymax, Y) : Y;
  }
  s->x0 = (int)fmax(0.0, floor(xmin) - 1.0);
  s->y0 = (int)fmax(0.0, floor(ymin) - 1.0);
  s->x1 = (int)fmin((double)(w - 1), ceil(xmax) + 1.0);
  s->y1 = (int)fmin((double)(h - 1), ceil(ymax) + 1.0);
}

}  // namespace

__global__ void maps_char_kernel(const float* __restrict__ quads, int n, float* __restrict__ rbox, float* __restrict__ ctr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float ob[8];
  rotated_box(quads + (size_t)i * 8, ob);
  for (int q = 0; q < 8; ++q) rbox[(size_t)i * 8 + q] = ob[q];
  ctr[2 * i] = (((ob[0] + ob[2]) + ob[4]) + ob[6]) / 4.f;  // box.mean(axis=0) (tools.py:595)
  ctr[2 * i + 1] = (((ob[1] + ob[3]) + ob[5]) + ob[7]) / 4.f;
}

// Block = one wave = one line.  Offsets are clamped, and every permutation entry read back is range-checked: whatever the
// caller passes, the kernel reads and writes inside its buffers.
__global__ void maps_line_kernel(const float* __restrict__ rbox, const float* __restrict__ ctr, const uint8_t* __restrict__ space,
                                 int n_chars, const int* __restrict__ line_off, int n_lines, const int* __restrict__ img_off, int N,
                                 int hh, int hw, int h, int w, int* __restrict__ permx, int* __restrict__ permy,
                                 MapSlot* __restrict__ slots) {
  const int l = blockIdx.x;
  const int s = min(max(line_off[l], 0), n_chars);
  const int n = min(max(line_off[l + 1], s), n_chars) - s;
  int lo = 0, hi = N;  // image = the last k with img_off[k] <= l
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (img_off[mid] <= l) lo = mid; else hi = mid;
  }
  const int img = lo;
  const float* c = ctr + 2 * (size_t)s;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float xi = c[2 * i], yi = c[2 * i + 1];
    int rx = 0, ry = 0;
    for (int j = 0; j < n; ++j) {
      const float xj = c[2 * j], yj = c[2 * j + 1];
      rx += xj < xi || (xj == xi && j < i);
      ry += yj < yi || (yj == yi && j < i);
    }
    permx[s + min(rx, n - 1)] = i;
    permy[s + min(ry, n - 1)] = i;
  }
  __shared__ int vertical;
  __syncthreads();
  if (threadIdx.x == 0) {
    // a NaN centre leaves rank collisions: make every entry a valid index before anything reads them
    for (int k = 0; k < n; ++k) {
      if ((unsigned)permx[s + k] >= (unsigned)n) permx[s + k] = 0;
      if ((unsigned)permy[s + k] >= (unsigned)n) permy[s + k] = 0;
    }
    const float dy = n > 1 ? pairwise_diff_sum(DiffSeq{c, permy + s, 1}, n - 1) : -0.0f;
    const float dx = n > 1 ? pairwise_diff_sum(DiffSeq{c, permx + s, 0}, n - 1) : -0.0f;
    vertical = dy > dx;  // tools.py:598
  }
  __syncthreads();
  const int* perm = vertical ? permy + s : permx + s;
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    const int i = perm[k];
    MapSlot cs, ls;
    cs.img = ls.img = img;
    cs.plane = 0;
    ls.plane = 1;
    cs.x0 = ls.x0 = 0;
    cs.x1 = ls.x1 = -1;  // empty
    cs.y0 = ls.y0 = cs.y1 = ls.y1 = 0;
    if (!space[s + i]) {
      float quad[8], lp[4];
      char_geometry(rbox + (size_t)(s + i) * 8, vertical, quad, lp);
      quad_slot(quad, hh, hw, h, w, &cs);
      const int pi = k > 0 ? perm[k - 1] : 0;
      if (k > 0 && !space[s + pi]) {
        float pq[8], pp[4];
        char_geometry(rbox + (size_t)(s + pi) * 8, vertical, pq, pp);
        // detection.py:147-165: [prev0, cur0, cur1, prev1] along a row, [prev0, prev1, cur1, cur0] down a column
        const float lq_h[8] = {pp[0], pp[1], lp[0], lp[1], lp[2], lp[3], pp[2], pp[3]};
        const float lq_v[8] = {pp[0], pp[1], pp[2], pp[3], lp[2], lp[3], lp[0], lp[1]};
        quad_slot(vertical ? lq_v : lq_h, hh, hw, h, w, &ls);
      }
    }
    slots[2 * (size_t)(s + k)] = cs;
    slots[2 * (size_t)(s + k) + 1] = ls;
  }
}

// A slot no line wrote (offsets that skip characters) keeps its fill of -1 and is empty, as is any box outside the map.
__global__ void maps_accum_kernel(const uint8_t* __restrict__ heat, int hh, int hw, const MapSlot* __restrict__ slots, int N, int h,
                                  int w, int* __restrict__ planes) {
  const MapSlot p = slots[blockIdx.x];
  if (p.img < 0 || p.img >= N || p.plane < 0 || p.plane > 1 || p.x0 < 0 || p.y0 < 0 || p.x1 >= w || p.y1 >= h) return;
  const int bw = p.x1 - p.x0 + 1, bh = p.y1 - p.y0 + 1;
  if (bw <= 0 || bh <= 0) return;
  int* plane = planes + ((size_t)p.img * 2 + p.plane) * h * w;
  const int total = bw * bh;
  for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < total; i += gridDim.y * blockDim.x) {
    const int y = p.y0 + i / bw, x = p.x0 + i % bw;
    const double xd = (double)x, yd = (double)y;
    const double X0 = (p.mi[0] * xd + p.mi[1] * yd) + p.mi[2];
    const double Y0 = (p.mi[3] * xd + p.mi[4] * yd) + p.mi[5];
    const double W0 = (p.mi[6] * xd + p.mi[7] * yd) + p.mi[8];
    const double Wi = W0 != 0.0 ? 32.0 / W0 : 0.0;
    const double fX = fmax(-2147483648.0, fmin(2147483647.0, X0 * Wi));
    const double fY = fmax(-2147483648.0, fmin(2147483647.0, Y0 * Wi));
    const long X = (long)rint(fX), Y = (long)rint(fY);  // saturate_cast<int>: half to even
    const long sx = X >> 5, sy = Y >> 5;
    const int ax = (int)(X & 31), ay = (int)(Y & 31);
    auto tap = [&](long yy, long xx) -> int {
      if (yy < 0 || yy >= hh || xx < 0 || xx >= hw) return 0;
      return heat[(size_t)yy * hw + xx];
    };
    const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32;
    const int w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
    const int acc = w00 * tap(sy, sx) + w01 * tap(sy, sx + 1) + w10 * tap(sy + 1, sx) + w11 * tap(sy + 1, sx + 1);
    const int v = (acc + (1 << 14)) >> 15;
    if (v) atomicAdd(plane + (size_t)y * w + x, v);
  }
}

__global__ void maps_finish_kernel(const int* __restrict__ planes, const float* __restrict__ table, int N, int hw_px,
                                   float* __restrict__ maps) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)N * hw_px) return;
  const long n = i / hw_px, p = i - n * hw_px;
  const int t = planes[(2 * n) * hw_px + p], k = planes[(2 * n + 1) * hw_px + p];
  maps[2 * i] = table[min(max(t, 0), 255)];
  maps[2 * i + 1] = table[min(max(k, 0), 255)];
}

int launch_compute_maps(kocr_ctx* ctx, const uint8_t* d_heat, int hh, int hw, int N, int h, int w, int n_chars,
                        const float* d_quads, const uint8_t* d_space, int n_lines, const int* d_line_off, const int* d_img_off,
                        const MapsWork& wk, float* d_maps) {
  if (N <= 0) return KOCR_OK;
  ProfScope ps(ctx, "compute_maps", 0, (double)N * h * w * 16.0);
  KOCR_HIP(ctx, hipMemsetAsync(wk.planes, 0, (size_t)N * 2 * h * w * sizeof(int), ctx->stream));
  if (n_chars > 0 && n_lines > 0) {
    KOCR_HIP(ctx, hipMemsetAsync(wk.slots, 0xff, (size_t)n_chars * 2 * sizeof(MapSlot), ctx->stream));
    hipLaunchKernelGGL(maps_char_kernel, dim3((n_chars + 63) / 64), dim3(64), 0, ctx->stream, d_quads, n_chars, wk.rbox, wk.ctr);
    hipLaunchKernelGGL(maps_line_kernel, dim3(n_lines), dim3(MAPS_LINE_THREADS), 0, ctx->stream, wk.rbox, wk.ctr, d_space, n_chars,
                       d_line_off, n_lines, d_img_off, N, hh, hw, h, w, wk.permx, wk.permy, wk.slots);
    hipLaunchKernelGGL(maps_accum_kernel, dim3(2 * n_chars, MAPS_ACCUM_SPLIT), dim3(MAPS_ACCUM_THREADS), 0, ctx->stream, d_heat, hh,
                       hw, wk.slots, N, h, w, wk.planes);
  }
  const long px = (long)N * h * w;
  hipLaunchKernelGGL(maps_finish_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, ctx->stream, wk.planes, wk.table, N,
                     h * w, d_maps);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// Keras' compiled "mse" on the detector's maps (detection.py:696), the per-image half: S_n = sum over pixels of the mean over
// the two channels of (y - y_hat)^2, in float64.  One block per image; each thread sums a fixed stride of pixels, then a
// fixed tree: the result does not depend on timing, so the fused (kocr_craft_mse) and the given-prediction (kocr_heat_mse)
// paths agree bit for bit.  The sample weights and the 1 / (N h w) are the host's.
constexpr int MSE_THREADS = 256;

__global__ void heat_mse_kernel(const float* __restrict__ y_true, const float* __restrict__ y_pred, int hw_px, double* __restrict__ sums) {
  const size_t base = (size_t)blockIdx.x * hw_px * 2;
  double acc = 0.0;
  for (int p = threadIdx.x; p < hw_px; p += MSE_THREADS) {
    const double d0 = (double)y_true[base + 2 * p] - (double)y_pred[base + 2 * p];
    const double d1 = (double)y_true[base + 2 * p + 1] - (double)y_pred[base + 2 * p + 1];
    acc += (d0 * d0 + d1 * d1) / 2.0;
  }
  __shared__ double red[MSE_THREADS];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int k = MSE_THREADS / 2; k > 0; k /= 2) {
    if ((int)threadIdx.x < k) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = red[0];
}

int launch_heat_mse(kocr_ctx* ctx, const float* d_true, const float* d_pred, int N, int hw_px, double* d_sums) {
  if (N <= 0) return KOCR_OK;
  ProfScope ps(ctx, "heat_mse", 4.0 * N * hw_px, 16.0 * N * hw_px);
  hipLaunchKernelGGL(heat_mse_kernel, dim3(N), dim3(MSE_THREADS), 0, ctx->stream, d_true, d_pred, hw_px, d_sums);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}
