// crnn_kernels.hip — the non-GEMM kernels of the CRNN recogniser (recognition.py:187-333).
//
//   crnn_input_kernel   Permute((2,1,3)) + flip axis 2 (recognition.py:215-216)
//   stn_sample_kernel   _transform bilinear sampler (recognition.py:73-166)
//   lstm_kernel         keras LSTM recurrence on the matrix cores (recognition.py:292-319):
//                       one workgroup = 32 crops x one direction for all 50 steps; h lives in LDS,
//                       c in registers, h@U is 32x512x128 per step on v_mfma_f32_32x32x2_f32 with the
//                       four gates of a hidden unit in the same lane (so the cell update is
//                       register-only); x@W+b is precomputed by the conv/GEMM kernel.
//   ctc_kernel          fc_12 softmax + CTCDecoder (recognition.py:169-184, 322-328): one wave per
//                       crop, lanes = classes, per-step argmax as a wavefront reduction, repeat
//                       merge + blank removal by lane 0.
//   ctc_loss_kernel     keras.backend.ctc_batch_cost (recognition.py:340-347): CTC forward algorithm in
//                       log space, one wave per sample, states over the lanes.
//   ctc_scores_kernel   ctc_kernel's decode + character scores + the word log-probability (ctc_loss_kernel's forward
//                       algorithm on the crop's own decode) in one launch, one wave per crop.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// in: [M][Hc=31][Wc=200] -> out: [M][Wc][Hc] with out[m][w][j] = in[m][Hc-1-j][w]
__global__ void crnn_input_kernel(const float* __restrict__ in, float* __restrict__ out, int M, int Hc, int Wc) {
  const size_t total = (size_t)M * Hc * Wc;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j = i % Hc;
    const size_t t = i / Hc;
    const int w = t % Wc;
    const size_t m = t / Wc;
    out[i] = in[(m * Hc + (Hc - 1 - j)) * Wc + w];
  }
}

// in: [M][Hn][Wn][C] (natural crop orientation) -> out: [M][Wn][Hn][C] with out[m][w][j] = in[m][Hn-1-j][w]
// (the Permute((2,1,3)) + flip of recognition.py:215-216 applied after the conv stack instead of before)
// Wp = width pitch of `in` in pixels (>= Wn: a width-padded tensor, Tensor::Wv)
__global__ void crnn_to_keras_kernel(const float* __restrict__ in, float* __restrict__ out, int M, int Hn, int Wn,
                                     int C4, int Wp) {
  const size_t total = (size_t)M * Hn * Wn * C4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c4 = i % C4;
    size_t t = i / C4;
    const int j = t % Hn;
    t /= Hn;
    const int w = t % Wn;
    const size_t m = t / Wn;
    reinterpret_cast<float4*>(out)[i] =
        reinterpret_cast<const float4*>(in)[((m * Hn + (Hn - 1 - j)) * Wp + w) * C4 + c4];
  }
}

// ---- the recogniser's crop batch as a CELL GRID (Tensor::cellW; round 5) ------------------------------------------------------
// conv_1 (recognition.py:217: 1 -> 64 channels, 3x3 'same', bias, ReLU; natural orientation, see crnn.cpp) straight from
// the crop batch [M][31][200] into the level-1 cell grid out[R][32][cn * 208][64]: cell (n, j) holds crop n * cn + j in its
// rows 1 .. 31 and columns 0 .. 199; row 0, columns 200 .. 207 and the cells behind crop M - 1 are written as zeros.  K = 9:
// plain fp32 FMAs (9 per output; the layer is bound by its 256 bytes of output per pixel), the same fma chain order for
// every output.  Also maintains the per-cell max-|x| slots (exact maximum, so a crop's scale does not depend on its cell).
// grid = (cells, 32 cell rows); thread = (column slot t >> 4 of 16, channel quad t & 15), 13 column groups per row.
__global__ __launch_bounds__(256) void crnn_conv1_cells_kernel(const float* __restrict__ crops, const float* __restrict__ w,
                                                               const float* __restrict__ pre_a, const float* __restrict__ pre_b,
                                                               float* __restrict__ out, unsigned* __restrict__ amax, int M, int cn,
                                                               int Hc, int Wc, int cellH, int cellW, int cout_pad) {
  const int cell = blockIdx.x, crow = blockIdx.y;
  const int n = cell / cn, j = cell - n * cn;
  const int t = threadIdx.x, cq = t & 15, xs = t >> 4;
  float wk[9][4], pa[4], pb[4];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c) wk[k][c] = w[(size_t)k * cout_pad + cq * 4 + c];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    pa[c] = pre_a[cq * 4 + c];
    pb[c] = pre_b[cq * 4 + c];
  }
  const int y = crow - 1;  // crop row
  const bool live = cell < M && y >= 0 && y < Hc;
  const float* src = crops + (size_t)(cell < M ? cell : 0) * Hc * Wc;
  float4* dst = reinterpret_cast<float4*>(out + (((size_t)n * cellH + crow) * ((size_t)cn * cellW) + (size_t)j * cellW) * 64) + cq;
  float mx = 0.f;
  for (int x = xs; x < cellW; x += 16) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && x < Wc) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int yy = y + ky - 1, xx = x + kx - 1;
          const float v = ((unsigned)yy < (unsigned)Hc && (unsigned)xx < (unsigned)Wc) ? src[yy * Wc + xx] : 0.f;
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] = fmaf(v, wk[ky * 3 + kx][c], acc[c]);
        }
      o.x = fmaxf(fmaf(acc[0], pa[0], pb[0]), 0.f);
      o.y = fmaxf(fmaf(acc[1], pa[1], pb[1]), 0.f);
      o.z = fmaxf(fmaf(acc[2], pa[2], pb[2]), 0.f);
      o.w = fmaxf(fmaf(acc[3], pa[3], pb[3]), 0.f);
      mx = fmaxf(mx, fmaxf(fmaxf(o.x, o.y), fmaxf(o.z, o.w)));
    }
    dst[(size_t)x * 16] = o;
  }
  if (amax) {
    const unsigned bits = kocr_wave_max_bits(mx);
    if (bits != 0 && (t & 63) == 0) atomicMax(amax + cell, bits);
  }
}

// level-3 cell grid in[R][cellH][cn * cellW][C] (crop rows at cell rows 1 .. Hn, natural orientation) -> Keras layout
// out[M][Wn][Hn][C] with out[m][w][j] = crop_m[Hn - 1 - j][w] (the Permute((2,1,3)) + flip of recognition.py:215-216)
__global__ void crnn_cells_to_keras_kernel(const float* __restrict__ in, float* __restrict__ out, int M, int Hn, int Wn, int C4,
                                           int cn, int cellH, int cellW) {
  const size_t total = (size_t)M * Hn * Wn * C4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c4 = i % C4;
    size_t t = i / C4;
    const int j = t % Hn;
    t /= Hn;
    const int w = t % Wn;
    const size_t m = t / Wn;
    const size_t n = m / cn, jc = m - n * cn;
    reinterpret_cast<float4*>(out)[i] =
        reinterpret_cast<const float4*>(in)[((n * cellH + (size_t)(Hn - 1 - j) + 1) * ((size_t)cn * cellW) + jc * cellW + w) * C4 + c4];
  }
}

// x: [M][H][W][C], theta: [M][6] -> out [M][H][W][C]
__global__ void stn_sample_kernel(const float* __restrict__ x, const float* __restrict__ theta, float* __restrict__ out,
                                  int M, int H, int W, int C) {
  const int pix = blockIdx.x;  // m*H*W + oy*W + ox
  const int ox = pix % W;
  const int oy = (pix / W) % H;
  const int m = pix / (W * H);
  const float* th = theta + (size_t)m * 6;
  // tf.linspace(-1, 1, n): start + i*delta, last element exactly 1
  const float xt = (ox == W - 1) ? 1.f : -1.f + (float)ox * (2.f / (float)(W - 1));
  const float yt = (oy == H - 1) ? 1.f : -1.f + (float)oy * (2.f / (float)(H - 1));
  const float xs = (th[0] * xt + th[1] * yt) + th[2];
  const float ys = (th[3] * xt + th[4] * yt) + th[5];
  const float fx = 0.5f * (xs + 1.0f) * (float)W;   // scaled by W, not W-1 (recognition.py:109)
  const float fy = 0.5f * (ys + 1.0f) * (float)H;
  int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
  int x1 = x0 + 1, y1 = y0 + 1;
  x0 = min(max(x0, 0), W - 1);
  x1 = min(max(x1, 0), W - 1);
  y0 = min(max(y0, 0), H - 1);
  y1 = min(max(y1, 0), H - 1);
  // weights from the CLIPPED corners (recognition.py:144-152)
  const float wa = ((float)x1 - fx) * ((float)y1 - fy);
  const float wb = ((float)x1 - fx) * (fy - (float)y0);
  const float wc = (fx - (float)x0) * ((float)y1 - fy);
  const float wd = (fx - (float)x0) * (fy - (float)y0);
  const float* base = x + (size_t)m * H * W * C;
  const float* pa = base + ((size_t)y0 * W + x0) * C;
  const float* pb = base + ((size_t)y1 * W + x0) * C;
  const float* pc = base + ((size_t)y0 * W + x1) * C;
  const float* pd = base + ((size_t)y1 * W + x1) * C;
  float* o = out + (size_t)pix * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) o[c] = ((wa * pa[c] + wb * pb[c]) + wc * pc[c]) + wd * pd[c];
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// xp: [M][T][2*4*U] (dir-major, gate order i,f,c,o); Uf/Ub: [U][4U]; out: [M][T][2U] in PROCESSING order
template <int UNITS>
__global__ __launch_bounds__(256) void lstm_kernel(const float* __restrict__ xp, const float* __restrict__ Uf,
                                                   const float* __restrict__ Ub, float* __restrict__ out, int M,
                                                   int T) {
  static_assert(UNITS == 128, "4 waves x 32 hidden units");
  constexpr int LD = UNITS + 1;
  __shared__ float hs[32][LD];
  const int dir = blockIdx.y;
  const int m0 = blockIdx.x * 32;
  const float* Ur = dir ? Ub : Uf;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lk = lane >> 5;
  const int j = wave * 32 + lr;  // hidden unit of this lane
  for (int i = tid; i < 32 * LD; i += 256) (&hs[0][0])[i] = 0.f;
  float c[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] = 0.f;
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const int tin = dir ? (T - 1 - t) : t;
    f32x16 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        acc[g][r] = m < M ? xp[((size_t)m * T + tin) * (8 * UNITS) + dir * 4 * UNITS + g * UNITS + j] : 0.f;
      }
#pragma unroll 4
    for (int kp = 0; kp < UNITS / 2; ++kp) {
      const int k = 2 * kp + lk;
      const float a = hs[lr][k];
      const float* ur = Ur + (size_t)k * (4 * UNITS) + j;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ur[g * UNITS], acc[g], 0, 0, 0);
    }
    __syncthreads();  // every wave has finished reading h(t-1)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * lk;
      const float ig = sigmoidf_(acc[0][r]), fg = sigmoidf_(acc[1][r]);
      const float gg = tanhf(acc[2][r]), og = sigmoidf_(acc[3][r]);
      c[r] = fg * c[r] + ig * gg;
      const float h = og * tanhf(c[r]);
      hs[row][j] = h;
      const int m = m0 + row;
      if (m < M) out[((size_t)m * T + t) * (2 * UNITS) + dir * UNITS + j] = h;
    }
    __syncthreads();
  }
}

// Round 3: the recurrence is a chain of T = 50 dependent steps, so its time is (time of one step) x 50 whatever the
// batch: lstm16_kernel shortens the step.  One workgroup = 16 crops x one direction (twice as many workgroups, each with
// half the matrix work per step: 32 x 8 v_mfma_f32_16x16x4_f32 per wave), and the wave's slice of the recurrent kernel
// U (128 k x 32 hidden units x 4 gates = 256 values per lane) stays in REGISTERS for all 50 steps instead of being
// re-fetched from L2 every step (256 loads per wave and step before).  Same arithmetic: fp32 MFMA, gates i, f, c, o of a
// hidden unit in one lane, cell state in registers, h through LDS.
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int UNITS>
__global__ __launch_bounds__(256) void lstm16_kernel(const float* __restrict__ xp, const float* __restrict__ Uf,
                                                     const float* __restrict__ Ub, float* __restrict__ out, int M, int T) {
  static_assert(UNITS == 128, "4 waves x 32 hidden units");
  constexpr int LD = UNITS + 1;
  __shared__ float hs[16][LD];
  const int dir = blockIdx.y;
  const int m0 = blockIdx.x * 16;
  const float* Ur = dir ? Ub : Uf;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  // N-tile (g, uh): gate g, hidden units 32 wave + 16 uh + [0, 16); this lane's column is unit j[uh]
  const int j0 = wave * 32 + lr;
  float ureg[8][UNITS / 4];  // [g * 2 + uh][k step]: U[4 kp + lk][g UNITS + j0 + 16 uh]
#pragma unroll
  for (int gu = 0; gu < 8; ++gu)
#pragma unroll
    for (int kp = 0; kp < UNITS / 4; ++kp)
      ureg[gu][kp] = Ur[(size_t)(4 * kp + lk) * (4 * UNITS) + (gu >> 1) * UNITS + j0 + 16 * (gu & 1)];
  for (int i = tid; i < 16 * LD; i += 256) (&hs[0][0])[i] = 0.f;
  float c[2][4];
#pragma unroll
  for (int uh = 0; uh < 2; ++uh)
#pragma unroll
    for (int r = 0; r < 4; ++r) c[uh][r] = 0.f;
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const int tin = dir ? (T - 1 - t) : t;
    f32x4 acc[8];
    // 16x16 C/D map: column = lane & 15, row = 4 (lane >> 4) + r
#pragma unroll
    for (int gu = 0; gu < 8; ++gu)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + 4 * lk + r;
        acc[gu][r] = m < M ? xp[((size_t)m * T + tin) * (8 * UNITS) + dir * 4 * UNITS + (gu >> 1) * UNITS + j0 + 16 * (gu & 1)] : 0.f;
      }
#pragma unroll
    for (int kp = 0; kp < UNITS / 4; ++kp) {
      const float a = hs[lr][4 * kp + lk];  // A: row (crop) = lane & 15, k = lane >> 4
#pragma unroll
      for (int gu = 0; gu < 8; ++gu) acc[gu] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ureg[gu][kp], acc[gu], 0, 0, 0);
    }
    __syncthreads();  // every wave has finished reading h(t-1)
#pragma unroll
    for (int uh = 0; uh < 2; ++uh)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * lk + r;
        const float ig = sigmoidf_(acc[0 + uh][r]), fg = sigmoidf_(acc[2 + uh][r]);
        const float gg = tanhf(acc[4 + uh][r]), og = sigmoidf_(acc[6 + uh][r]);
        c[uh][r] = fg * c[uh][r] + ig * gg;
        const float h = og * tanhf(c[uh][r]);
        const int j = j0 + 16 * uh;
        hs[row][j] = h;
        const int m = m0 + row;
        if (m < M) out[((size_t)m * T + t) * (2 * UNITS) + dir * UNITS + j] = h;
      }
    __syncthreads();
  }
}

// ---- fc_12's softmax (recognition.py:324), shared by ctc_kernel and ctc_loss_kernel<true> so that the loss of the logits is
// computed on exactly the probabilities kocr_crnn_forward returns: p(c) = e^(row[c] - max) / sum, lane l owning the classes
// l, l + 64, ...; per-lane sums in ascending class order, then the xor butterfly.
// Per-lane argmax over its classes (ascending class index: first maximum wins), then the wave-level reduction of
// (value, index) pairs with lowest index on ties; every lane ends with the row's maximum and its first index.
//
// Character sets ("Character sets"; CharMask in common.h): the MASKED instantiations of the decode
// kernels read a row only through cm_at, which answers -inf for a class outside the crop's set -- the row fc_12 would have
// written had it known the set -- so every rule behind it is the unmasked rule on that row.  The crop's mask words
// (ceil(C / 32) of them, the blank's bit set) are loaded ONCE per crop into LDS (cm_load), never per frame from HBM.
// MASKED = false compiles to the code without the feature: cm_at is row[c] and nothing else is generated.
template <bool MASKED>
__device__ __forceinline__ bool cm_allowed(const uint32_t* w, int c) {
  if constexpr (MASKED) return (w[c >> 5] >> (c & 31)) & 1u;
  return true;
}
template <bool MASKED>
__device__ __forceinline__ float cm_at(const float* __restrict__ row, const uint32_t* w, int c) {
  if constexpr (MASKED) return cm_allowed<true>(w, c) ? row[c] : -INFINITY;
  return row[c];
}
// The mask words of crop m of the launch into w [ceil(C / 32)] (LDS), by one wave; set -1: every class.  The caller
// synchronises before the first cm_at.
__device__ __forceinline__ void cm_load(const uint32_t* __restrict__ bits, const int32_t* __restrict__ set_of, int uniform, int shift,
                                        int first, int m, int C, int lane, uint32_t* w) {
  const int nw = (C + 31) >> 5;
  int set = uniform;
  if (set_of) set = set_of[(first + m) >> shift];
  for (int i = lane; i < nw; i += 64) {
    uint32_t v = (i == nw - 1 && (C & 31)) ? (1u << (C & 31)) - 1u : ~0u;
    if (set >= 0) v = bits[(size_t)set * nw + i];
    w[i] = v;
  }
}

template <bool MASKED = false>
__device__ __forceinline__ void ctc_row_argmax(const float* __restrict__ row, int C, int lane, float& bv, int& bi,
                                               const uint32_t* w = nullptr) {
  bv = -INFINITY;
  bi = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float v = cm_at<MASKED>(row, w, c);
    if (v > bv) {
      bv = v;
      bi = c;
    }
  }
  for (int o = 32; o; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
}
// e^(v - mx) without the rounding error of the float32 difference.  On a saturated frame (a trained recogniser: the losers
// 30 below the winner) that error alone is up to 2^-20, 16 u relative to the probability -- more than the whole stated bound
// (C + 8) u of a 4-class softmax (tests/crnn_layer_check.py: check_ctc).  TwoSum (Knuth) gives it exactly:
// d + err == v - mx, and e^(d + err) = e^d (1 + err) to within err^2 <= 2^-40.
// (v = -inf: err is NaN but e^d is 0; a row's maximum has d = err = 0 and stays exactly 1.)
__device__ __forceinline__ float ctc_exp_diff(float v, float mx) {
  const float d = v - mx;
  const float t = d - v;
  const float err = (v - (d - t)) + (-mx - t);
  const float e = expf(d);
  return e == 0.f ? 0.f : fmaf(e, err, e);
}
template <bool MASKED = false>
__device__ __forceinline__ float ctc_row_expsum(const float* __restrict__ row, int C, int lane, float mx, const uint32_t* w = nullptr) {
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += ctc_exp_diff(cm_at<MASKED>(row, w, c), mx);
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
  return s;
}
__device__ __forceinline__ float ctc_softmax(float v, float mx, float s) { return ctc_exp_diff(v, mx) / s; }

// logits: [M][T][C]; labels: [M][T-discard] (-1 padded); probs (nullable): [M][T-discard][C].
// One wave per crop; lane l owns classes l, l+64, ... (any alphabet size).
// MASKED: cm's sets (dynamic LDS: ceil(C / 32) words per wave of the block).
template <bool MASKED>
__global__ void ctc_kernel(const float* __restrict__ logits, int M, int T, int C, int discard, int* __restrict__ labels,
                           float* __restrict__ probs, CharMask cm) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t* w = nullptr;
  if constexpr (MASKED) {
    extern __shared__ uint32_t cm_words[];
    uint32_t* mine = cm_words + (threadIdx.x >> 6) * ((C + 31) >> 5);
    if (m < M) cm_load(cm.bits, cm.set_of, cm.uniform, cm.shift, cm.first, m, C, lane, mine);
    __syncthreads();
    w = mine;
  }
  if (m >= M) return;
  const int To = T - discard;
  const int blank = C - 1;
  int prev = -1, k = 0;
  for (int t = 0; t < To; ++t) {
    const float* row = logits + ((size_t)m * T + t + discard) * C;
    float bv;
    int bi;
    ctc_row_argmax<MASKED>(row, C, lane, bv, bi, w);
    if (probs) {
      const float s = ctc_row_expsum<MASKED>(row, C, lane, bv, w);
      for (int c = lane; c < C; c += 64) probs[((size_t)m * To + t) * C + c] = ctc_softmax(cm_at<MASKED>(row, w, c), bv, s);
    }
    if (lane == 0) {
      if (bi != prev && bi != blank) labels[(size_t)m * To + k++] = bi;
      prev = bi;
    }
  }
  if (lane == 0)
    for (; k < To; ++k) labels[(size_t)m * To + k] = -1;
}

// ---- CTC loss: keras.backend.ctc_batch_cost (recognition.py:340-347), the forward algorithm of DESIGN.md section 4 ----------
// q_t(c) = (y[t][c] + eps) / sum_c' (y[t][c'] + eps), eps = 1e-7 (TF ctc_loss's softmax of log(y + eps)); extended label
// l' = (b, l_1, b, ..., l_L, b), S = 2L + 1 states, blank b = C - 1; loss = -log(alpha_{T_m-1}(S-1) + alpha_{T_m-1}(S-2)).
// One wave (= one workgroup) per sample; the states are spread over the 64 lanes in chunks of 64, log(alpha) of the previous
// and the current frame in LDS (2 x Sp floats, Sp = the padded state count of the longest label).  Per frame: one wave
// reduction of the normaliser over the C classes, then per state a gather of y[t][l'_s].  Float32 log space; a log-sum-exp
// whose terms are all -inf stays -inf, never NaN.  Masked states: s > 2t + 1 cannot be reached yet, s < S - 2(T_m - t) can no
// longer reach the end; both are -inf.
// LOGITS = false: y is [M][T][C] probabilities (kocr_ctc_batch_cost), t0 = 0.
// LOGITS = true: y is fc_12's output [M][T][C] (kocr_crnn_ctc_loss); frame t is row t0 + t (rnn_steps_to_discard) and its
// probabilities are ctc_kernel's, bit for bit (ctc_row_argmax / ctc_row_expsum / ctc_softmax).
// lab: [M][lstride] int32 (entries < len[m] are classes in [0, C-2]), len / in_len: [M]; loss: [M]
constexpr float CTC_EPS = 1e-7f;  // keras.backend.epsilon()

__device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
  const float mx = fmaxf(a, fmaxf(b, c));
  if (mx == -INFINITY) return -INFINITY;
  return mx + logf(expf(a - mx) + expf(b - mx) + expf(c - mx));
}

// The forward algorithm of one sample by one wave.  y0: the sample's first frame (row t of the loop is y0 + t * C); l: its L
// labels (global or LDS); la: [2][Sp] floats of LDS, Sp >= 2L + 1.  Returns the loss (every lane computes it from LDS).
// Shared by ctc_loss_kernel and ctc_scores_kernel, so that the word log-probability of a decode is, bit for bit, minus the
// loss kocr_crnn_ctc_loss gives for the same labels.
// MASKED (LOGITS only): the rows are read through the crop's mask words w (cm_at).
template <bool LOGITS, bool MASKED = false>
__device__ __forceinline__ float ctc_loss_wave(const float* __restrict__ y0, int C, const int* l, int L, int Tm, float* la, int Sp,
                                               int lane, const uint32_t* w = nullptr) {
  const int S = 2 * L + 1, blank = C - 1;
  for (int s = lane; s < 2 * Sp; s += 64) la[s] = -INFINITY;
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < Tm; ++t) {
    const float* row = y0 + (size_t)t * C;
    float mx = 0.f, es = 1.f;
    if (LOGITS) {
      int bi;
      ctc_row_argmax<MASKED>(row, C, lane, mx, bi, w);
      es = ctc_row_expsum<MASKED>(row, C, lane, mx, w);
    }
    float z = 0.f;
    for (int c = lane; c < C; c += 64) z += (LOGITS ? ctc_softmax(cm_at<MASKED>(row, w, c), mx, es) : row[c]) + CTC_EPS;
    for (int o = 32; o; o >>= 1) z += __shfl_xor(z, o);
    const float logz = logf(z);
    const int lo = max(0, S - 2 * (Tm - t)), hi = min(S - 1, 2 * t + 1);
    const float* prev = la + (cur ^ 1) * Sp;
    float* nxt = la + cur * Sp;
    for (int s0 = lo & ~63; s0 <= hi; s0 += 64) {
      const int s = s0 + lane;
      if (s >= S) break;
      float a = -INFINITY;
      if (s >= lo && s <= hi) {
        const int cls = (s & 1) ? l[s >> 1] : blank;
        const float v = cm_at<MASKED>(row, w, cls);
        const float lq = logf((LOGITS ? ctc_softmax(v, mx, es) : v) + CTC_EPS) - logz;
        if (t == 0) {
          a = lq;  // s <= 1 here (hi = 1)
        } else {
          const float a1 = s >= 1 ? prev[s - 1] : -INFINITY;
          const float a2 = ((s & 1) && s >= 3 && l[s >> 1] != l[(s >> 1) - 1]) ? prev[s - 2] : -INFINITY;
          a = ctc_lse3(prev[s], a1, a2) + lq;
        }
      }
      nxt[s] = a;
    }
    __syncthreads();
    cur ^= 1;
  }
  const float* fin = la + (cur ^ 1) * Sp;
  const float a = fin[S - 1], b = L > 0 ? fin[S - 2] : -INFINITY;
  const float mxv = fmaxf(a, b);
  return mxv == -INFINITY ? INFINITY : -(mxv + logf(expf(a - mxv) + expf(b - mxv)));
}

template <bool LOGITS>
__global__ __launch_bounds__(64) void ctc_loss_kernel(const float* __restrict__ y, int T, int C, int t0,
                                                      const int* __restrict__ lab, int lstride, const int* __restrict__ len,
                                                      const int* __restrict__ in_len, float* __restrict__ loss, int Sp) {
  extern __shared__ float la[];  // [2][Sp]
  const int m = blockIdx.x, lane = threadIdx.x;
  const float v = ctc_loss_wave<LOGITS>(y + ((size_t)m * T + t0) * C, C, lab + (size_t)m * lstride, len[m], in_len[m], la, Sp, lane);
  if (lane == 0) loss[m] = v;
}

// ---- scores ("Scores"): ctc_kernel's decode, the character scores and the word log-probability of
// every crop in one launch.  One wave (= one workgroup) per crop.  Pass 1 is ctc_kernel's loop: lane 0 emits the label row
// (bit for bit ctc_kernel's: the same arg-max and the same rule) and keeps, per emitted label, the maximum over the frames
// of its run of the arg-max's softmax probability -- ctc_softmax(max, max, sum), the very entry of `probs`.  Pass 2 is
// ctc_loss_wave<true> on the decoded label, all To frames: the label row (at most To ints) and its length stay in LDS beside
// the two alpha rows, so neither the labels, the length nor the states take a trip through the host; a crop's logits
// (T x C floats) come from cache the second time.  logw = -loss; chars: [M][To], 0 behind the decode.
// MASKED: behind them the crop's ceil(C / 32) mask words.
template <bool MASKED>
__global__ __launch_bounds__(64) void ctc_scores_kernel(const float* __restrict__ logits, int T, int C, int discard,
                                                        int* __restrict__ labels, float* __restrict__ probs,
                                                        float* __restrict__ logw, float* __restrict__ chars, int Sp, CharMask cm) {
  extern __shared__ float la[];  // [2][Sp] alpha rows, then int[To + 1]: the decoded label and its length
  int* dec = reinterpret_cast<int*>(la + 2 * Sp);
  const int m = blockIdx.x, lane = threadIdx.x;
  const int To = T - discard, blank = C - 1;
  const float* y0 = logits + ((size_t)m * T + discard) * C;
  const uint32_t* w = nullptr;
  if constexpr (MASKED) {
    uint32_t* mine = reinterpret_cast<uint32_t*>(dec + To + 1);
    cm_load(cm.bits, cm.set_of, cm.uniform, cm.shift, cm.first, m, C, lane, mine);
    __syncthreads();
    w = mine;
  }
  int prev = -1, k = 0;
  float run = 0.f;  // lane 0: the score of label k - 1 so far
  for (int t = 0; t < To; ++t) {
    const float* row = y0 + (size_t)t * C;
    float bv;
    int bi;
    ctc_row_argmax<MASKED>(row, C, lane, bv, bi, w);
    const float s = ctc_row_expsum<MASKED>(row, C, lane, bv, w);
    if (probs)
      for (int c = lane; c < C; c += 64) probs[((size_t)m * To + t) * C + c] = ctc_softmax(cm_at<MASKED>(row, w, c), bv, s);
    if (lane == 0) {
      const float p = ctc_softmax(bv, bv, s);
      if (bi != prev && bi != blank) {
        if (k) chars[(size_t)m * To + k - 1] = run;
        dec[k] = bi;
        labels[(size_t)m * To + k++] = bi;
        run = p;
      } else if (bi == prev && bi != blank) {
        run = fmaxf(run, p);
      }
      prev = bi;
    }
  }
  if (lane == 0) {
    if (k) chars[(size_t)m * To + k - 1] = run;
    dec[To] = k;
    for (; k < To; ++k) {
      labels[(size_t)m * To + k] = -1;
      chars[(size_t)m * To + k] = 0.f;
    }
  }
  __syncthreads();
  const float loss = ctc_loss_wave<true, MASKED>(y0, C, dec, dec[To], To, la, Sp, lane, w);
  if (lane == 0) logw[m] = -loss;
}

// ---- long words ("Long words"): ctc_scores_kernel on a RAGGED batch.  Word m's frames are rows
// roff[m] .. roff[m] + Tn[m] - 1 of seq [sum T'][C] (the stitched windows; nothing is discarded any more), its label and score
// rows are LW wide, LW >= every Tn (the launcher sizes the LDS from it: [2][Sp] alpha rows, then int[LW + 1]).  The two passes
// are ctc_scores_kernel's, expression for expression, through the same device functions: a word of one window comes out bit
// for bit as ctc_scores_kernel gives its crop, and since one wave owns a word and nothing is shared between words, a word's
// bits do not depend on the batch.  No character sets (the windowed calls refuse them): the unmasked instantiations.
__global__ __launch_bounds__(64) void ctc_scores_ragged_kernel(const float* __restrict__ seq, const long long* __restrict__ roff,
                                                               const int* __restrict__ Tn, int C, int LW, int* __restrict__ labels,
                                                               float* __restrict__ logw, float* __restrict__ chars, int Sp) {
  extern __shared__ float la[];
  int* dec = reinterpret_cast<int*>(la + 2 * Sp);
  const int m = blockIdx.x, lane = threadIdx.x;
  const int To = min(max(Tn[m], 0), LW), blank = C - 1;  // clamped: whatever the buffers hold, the rows are LW wide
  const float* y0 = seq + (size_t)roff[m] * C;
  int prev = -1, k = 0;
  float run = 0.f;
  for (int t = 0; t < To; ++t) {
    const float* row = y0 + (size_t)t * C;
    float bv;
    int bi;
    ctc_row_argmax<false>(row, C, lane, bv, bi);
    const float s = ctc_row_expsum<false>(row, C, lane, bv);
    if (lane == 0) {
      const float p = ctc_softmax(bv, bv, s);
      if (bi != prev && bi != blank) {
        if (k) chars[(size_t)m * LW + k - 1] = run;
        dec[k] = bi;
        labels[(size_t)m * LW + k++] = bi;
        run = p;
      } else if (bi == prev && bi != blank) {
        run = fmaxf(run, p);
      }
      prev = bi;
    }
  }
  if (lane == 0) {
    if (k) chars[(size_t)m * LW + k - 1] = run;
    dec[LW] = k;
    for (; k < LW; ++k) {
      labels[(size_t)m * LW + k] = -1;
      chars[(size_t)m * LW + k] = 0.f;
    }
  }
  __syncthreads();
  const float loss = ctc_loss_wave<true, false>(y0, C, dec, dec[LW], To, la, Sp, lane);
  if (lane == 0) logw[m] = -loss;
}

// ---- beam search ("Beam search"): CTC prefix beam search without a language model (Graves 2012,
// Hannun 2014; keras.backend.ctc_decode(greedy=False)), one wave (= one workgroup) per crop, lane i owning beam entry i.
// Frame probabilities are the loss's q_t (ctc_loss_wave<true>: fc_12's softmax + eps, renormalised), float32 log domain.
// An entry is a prefix with log p_blank / log p_nonblank (the summed probability of the alignments of the frames so far
// that collapse to the prefix and end / do not end in a blank).  Per frame every entry proposes
//   same      the prefix itself: pb' = tot + lq(blank), pnb' = pnb + lq(last label)           (tot = lse(pb, pnb))
//   ext(e)    the prefix + class cls[e]: pnb' = (cls[e] == last label ? pb : tot) + lq(cls[e]), pb' = -inf
// for the E = min(B, C - 1) non-blank classes of the largest logit (ties: the smaller class), which is q_t's order.  An
// ext that spells a prefix already in the beam is MERGED into that entry's `same` (log-add into pnb'): the entry finds its
// parent through the rolling 64-bit key of its prefix without the last label, confirmed by a full compare.  No two other
// candidates can spell the same prefix.  The best B candidates by total make the next beam, taken one per round.
// Tie rule: the higher total first, then the lexicographically smaller label row, -1 sorting after every label.
// After the last frame the K best entries are copied out by the same rounds, each is rescored by ctc_loss_wave<true> (the
// exact sum over all alignments: log_prob == -kocr_crnn_ctc_loss of that label, bit for bit) and the rows are written in
// the order of the rescored value (tie rule as above).  Every reduction has a fixed order and nothing is shared between
// crops, so a crop's result does not depend on M or on its place in the batch.
// LDS: two beams of B x (key, parent key, pb, pnb, len, last, prefix[Ls]), the loss's la [2][Sp], cls / lqc / par / pe [64 each]:
// 2 B (4 Ls + 32) + 8 Sp + 1024 bytes, 32.3 KB at B = 64, To = 50 (Ls = To | 1 keeps the rows off one bank).
struct BeamBuf {
  unsigned long long* key;   // rolling key of the prefix
  unsigned long long* pkey;  // ... of the prefix without its last label
  float* pb;
  float* pnb;
  int* len;
  int* last;
  int* pre;  // [B][Ls]
};
constexpr unsigned long long BEAM_KEY_MUL = 0x9E3779B97F4A7C15ull;
constexpr int BEAM_NONE = 0x7fffffff;  // "no label" in row comparisons: sorts after every label

__device__ __forceinline__ float ctc_lse2(float a, float b) {
  const float mx = fmaxf(a, b);
  if (mx == -INFINITY) return -INFINITY;
  return mx + logf(expf(a - mx) + expf(b - mx));
}

// Position p of the label row of a candidate: entry x's prefix, then class c (BEAM_NONE: none), then BEAM_NONE.
__device__ __forceinline__ int beam_row_at(const BeamBuf& b, int Ls, int x, int len, int c, int p) {
  return p < len ? b.pre[x * Ls + p] : (p == len ? c : BEAM_NONE);
}

// The wave's best candidate: every lane offers (v, its entry's length, the appended class or BEAM_NONE); returns the
// winning lane, or -1 when every v is -inf.  Equal v: the lexicographically smaller row, compared by the 64 lanes at once
// (rows are at most 64 long and differ, since equal prefixes were merged).
__device__ __forceinline__ int beam_pick(const BeamBuf& b, int Ls, float v, int len, int c, int lane) {
  float vmax = v;
  for (int o = 32; o; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
  if (vmax == -INFINITY) return -1;
  unsigned long long tied = __ballot(v == vmax);
  int w = __ffsll((long long)tied) - 1;
  tied &= tied - 1;
  while (tied) {
    const int u = __ffsll((long long)tied) - 1;
    tied &= tied - 1;
    const int a = beam_row_at(b, Ls, w, __shfl(len, w), __shfl(c, w), lane);
    const int d = beam_row_at(b, Ls, u, __shfl(len, u), __shfl(c, u), lane);
    const unsigned long long diff = __ballot(a != d);
    const int f = __ffsll((long long)diff) - 1;  // diff != 0: the rows differ
    if (__shfl(d, f) < __shfl(a, f)) w = u;
  }
  return w;
}

// MASKED (character sets): a prefix is extended only by classes of the crop's set A -- E = min(B, |A|), the selection rounds
// pass over the other classes, and the "all of them" shortcut holds only when |A| = C - 1; the mask words lie behind the
// prefixes in LDS.
template <bool MASKED>
__global__ __launch_bounds__(64) void ctc_beam_kernel(const float* __restrict__ logits, int T, int C, int discard, int B, int K,
                                                      int* __restrict__ labels, float* __restrict__ logp, int Sp, int Ls, CharMask cm) {
  extern __shared__ unsigned long long beam_lds[];
  const int m = blockIdx.x, lane = threadIdx.x;
  const int To = T - discard, blank = C - 1;
  int E = min(B, C - 1);
  // both beams side by side, array by array: buffer i starts i * B (i * B * Ls for the prefixes) into each
  unsigned long long* keys = beam_lds;            // [2][B]
  unsigned long long* pkeys = keys + 2 * B;       // [2][B]
  float* la = reinterpret_cast<float*>(pkeys + 2 * B);  // [2][Sp]
  float* pbs = la + 2 * Sp;                       // [2][B]
  float* pnbs = pbs + 2 * B;                      // [2][B]
  float* lqc = pnbs + 2 * B;                      // [64] log q of the frame's extension classes
  int* cls = reinterpret_cast<int*>(lqc + 64);    // [64] the frame's extension classes
  int* par = cls + 64;                            // [64] entry -> the entry whose ext it merges (-1: none)
  int* pe = par + 64;                             // [64] ... and which ext
  int* lens = pe + 64;                            // [2][B]
  int* lasts = lens + 2 * B;                      // [2][B]
  int* pres = lasts + 2 * B;                      // [2][B][Ls]
  auto beam = [&](int i) { return BeamBuf{keys + i * B, pkeys + i * B, pbs + i * B, pnbs + i * B, lens + i * B, lasts + i * B, pres + i * B * Ls}; };
  const float* y0 = logits + ((size_t)m * T + discard) * C;
  const uint32_t* w = nullptr;
  if constexpr (MASKED) {
    uint32_t* mine = reinterpret_cast<uint32_t*>(pres + 2 * B * Ls);  // [ceil(C / 32)]
    cm_load(cm.bits, cm.set_of, cm.uniform, cm.shift, cm.first, m, C, lane, mine);
    __syncthreads();
    int na = 0;  // |A|: the set bits without the blank's
    for (int i = lane; i < (C + 31) >> 5; i += 64) na += __popc(mine[i]);
    for (int o = 32; o; o >>= 1) na += __shfl_xor(na, o);
    E = min(B, na - 1);
    w = mine;
  }

  // the empty prefix: p_blank = 1
  if (lane == 0) {
    keys[0] = pkeys[0] = 0;
    pbs[0] = 0.f;
    pnbs[0] = -INFINITY;
    lens[0] = 0;
    lasts[0] = -1;
  }
  int nb = 1, cur = 0;
  __syncthreads();
  // frames 0 .. To - 1, then one more pass (t == To) that moves the K best entries, unchanged, into the other buffer
  for (int t = 0; t <= To; ++t) {
    const bool fin = t == To;
    const BeamBuf bc = beam(cur), bn = beam(cur ^ 1);
    const float* row = y0 + (size_t)t * C;
    float mx = 0.f, es = 1.f, logz = 0.f;
    if (!fin) {
      int bi;
      ctc_row_argmax<MASKED>(row, C, lane, mx, bi, w);
      es = ctc_row_expsum<MASKED>(row, C, lane, mx, w);
      float z = 0.f;
      for (int c = lane; c < C; c += 64) z += ctc_softmax(cm_at<MASKED>(row, w, c), mx, es) + CTC_EPS;
      for (int o = 32; o; o >>= 1) z += __shfl_xor(z, o);
      logz = logf(z);
      // the E extension classes: all of them, or E rounds of "the largest logit behind the last pick"
      if (E == C - 1) {
        if (lane < E) cls[lane] = lane;
      } else {
        float pv = INFINITY;
        int pc = -1;
        for (int e = 0; e < E; ++e) {
          float bv = -INFINITY;
          int bc_ = BEAM_NONE;
          for (int c = lane; c < blank; c += 64) {
            if (!cm_allowed<MASKED>(w, c)) continue;
            const float v = row[c];
            if ((v < pv || (v == pv && c > pc)) && (v > bv || (v == bv && c < bc_))) {
              bv = v;
              bc_ = c;
            }
          }
          for (int o = 32; o; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oc = __shfl_xor(bc_, o);
            if (ov > bv || (ov == bv && oc < bc_)) {
              bv = ov;
              bc_ = oc;
            }
          }
          pv = bv;
          pc = bc_;
          if (lane == e) cls[e] = bc_;
        }
      }
      if (lane < E) lqc[lane] = logf(ctc_softmax(cm_at<MASKED>(row, w, cls[lane]), mx, es) + CTC_EPS) - logz;
      __syncthreads();
    }
    // this lane's entry
    const bool valid = lane < nb;
    const float pb = valid ? bc.pb[lane] : -INFINITY, pnb = valid ? bc.pnb[lane] : -INFINITY;
    const int len = valid ? bc.len[lane] : 0, last = valid ? bc.last[lane] : -1;
    const unsigned long long key = valid ? bc.key[lane] : 0, pkey = valid ? bc.pkey[lane] : 0;
    const float tot = ctc_lse2(pb, pnb);
    float same_pb = pb, same_pnb = pnb;
    unsigned long long taken = E < 64 ? ~0ull << E : 0ull;  // exts that are no candidates of this lane
    if (fin) {
      taken = ~0ull;
    } else {
      // the entry whose prefix is this one's without the last label, and its ext that spells this prefix
      int pi = -1, pj = 0;
      float extv = -INFINITY;
      if (valid && len > 0) {
        for (int i = 0; i < nb && pi < 0; ++i) {
          if (bc.len[i] != len - 1 || bc.key[i] != pkey) continue;
          bool eq = true;
          for (int p = 0; p < len - 1 && eq; ++p) eq = bc.pre[i * Ls + p] == bc.pre[lane * Ls + p];
          if (eq) pi = i;
        }
        if (pi >= 0) {
          int e = 0;
          while (e < E && cls[e] != last) ++e;
          if (e < E) {
            pj = e;
            extv = (bc.last[pi] == last ? bc.pb[pi] : ctc_lse2(bc.pb[pi], bc.pnb[pi])) + lqc[e];
          } else {
            pi = -1;
          }
        }
      }
      par[lane] = pi;
      pe[lane] = pj;
      __syncthreads();
      for (int j = 0; j < nb; ++j)
        if (par[j] == lane) taken |= 1ull << pe[j];
      same_pb = tot + (logf(ctc_softmax(cm_at<MASKED>(row, w, blank), mx, es) + CTC_EPS) - logz);
      same_pnb = len > 0 ? pnb + (logf(ctc_softmax(cm_at<MASKED>(row, w, last), mx, es) + CTC_EPS) - logz) : -INFINITY;
      same_pnb = ctc_lse2(same_pnb, extv);
    }
    const float same_tot = valid ? ctc_lse2(same_pb, same_pnb) : -INFINITY;
    bool same_taken = false;
    const int rounds = fin ? K : B;
    int r = 0;
    bool rescan = true;
    float best_v = -INFINITY;
    int best_e = -1, best_c = BEAM_NONE;
    for (; r < rounds; ++r) {
      if (rescan) {  // this lane's best remaining candidate: the total, then ext before same, then the smaller class
        best_v = -INFINITY;
        best_e = -1;
        best_c = BEAM_NONE;
        for (int e = 0; e < E; ++e) {
          if ((taken >> e) & 1) continue;
          const int c = cls[e];
          const float v = (c == last ? pb : tot) + lqc[e];
          if (v > best_v || (v == best_v && c < best_c)) {
            best_v = v;
            best_e = e;
            best_c = c;
          }
        }
        if (!same_taken && same_tot > best_v) {
          best_v = same_tot;
          best_e = -1;
          best_c = BEAM_NONE;
        }
        rescan = false;
      }
      const int w = beam_pick(bc, Ls, best_v, len, best_c, lane);
      if (w < 0) break;
      // entry r of the next beam: the winner's row, then its values (written by the winner itself)
      const int wl = __shfl(len, w), wc = __shfl(best_c, w);
      if (lane < Ls) {
        const int v = beam_row_at(bc, Ls, w, wl, wc, lane);
        bn.pre[r * Ls + lane] = v == BEAM_NONE ? -1 : v;
      }
      if (lane == w) {
        if (best_e < 0) {
          bn.key[r] = key;
          bn.pkey[r] = pkey;
          bn.pb[r] = same_pb;
          bn.pnb[r] = same_pnb;
          bn.len[r] = len;
          bn.last[r] = last;
          same_taken = true;
        } else {
          bn.key[r] = key * BEAM_KEY_MUL + (unsigned long long)(best_c + 1);
          bn.pkey[r] = key;
          bn.pb[r] = -INFINITY;
          bn.pnb[r] = best_v;
          bn.len[r] = len + 1;
          bn.last[r] = best_c;
          taken |= 1ull << best_e;
        }
        rescan = true;
      }
    }
    nb = r;
    cur ^= 1;
    __syncthreads();
  }
  // rescoring: nb <= K rows
  const BeamBuf bo = beam(cur);
  float lp = -INFINITY;
  for (int k = 0; k < nb; ++k) {
    const float loss = ctc_loss_wave<true, MASKED>(y0, C, bo.pre + k * Ls, bo.len[k], To, la, Sp, lane, w);
    if (lane == k) lp = -loss;
  }
  // the rows in the order of the rescored value (tie rule), the rest -1 / -inf
  float* lps = lqc;  // [64]: the rescored values, for the ranks
  __syncthreads();
  lps[lane] = lp;
  __syncthreads();
  if (lane < K) {
    int rank = lane;
    if (lane < nb) {
      rank = 0;
      for (int j = 0; j < nb; ++j) {
        if (j == lane) continue;
        const float vj = lps[j];
        bool first = vj > lp;
        if (vj == lp) {
          int p = 0;
          while (p < To && bo.pre[j * Ls + p] == bo.pre[lane * Ls + p]) ++p;
          const int a = p < To ? bo.pre[j * Ls + p] : -1, d = p < To ? bo.pre[lane * Ls + p] : -1;
          first = (a < 0 ? BEAM_NONE : a) < (d < 0 ? BEAM_NONE : d);
        }
        rank += first ? 1 : 0;
      }
    }
    int* out = labels + ((size_t)m * K + rank) * To;
    for (int p = 0; p < To; ++p) out[p] = lane < nb ? bo.pre[lane * Ls + p] : -1;
    logp[(size_t)m * K + rank] = lp;
  }
}

int launch_crnn_input(kocr_ctx* ctx, const float* d_crops, float* d_x, int M, int Hc, int Wc) {
  const size_t total = (size_t)M * Hc * Wc;
  if (!total) return KOCR_OK;
  ProfScope ps(ctx, "crnn_input", 0, 8.0 * total);
  size_t b = (total + 255) / 256;
  if (b > 8192) b = 8192;
  hipLaunchKernelGGL(crnn_input_kernel, dim3((unsigned)b), dim3(256), 0, ctx->stream, d_crops, d_x, M, Hc, Wc);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

int launch_crnn_to_keras(kocr_ctx* ctx, const Tensor& in, const Tensor& out) {
  if (in.C % 4 || in.cs != in.C || out.cs != out.C || out.H != in.wv() || out.W != in.H || out.C != in.C)
    KOCR_FAIL(ctx, KOCR_EINVAL, "crnn_to_keras: bad shapes");
  const size_t total = out.pixels() * (in.C / 4);
  if (!total) return KOCR_OK;
  ProfScope ps(ctx, "crnn_to_keras", 0, 8.0 * in.pixels() * in.C);
  size_t b = (total + 255) / 256;
  if (b > 8192) b = 8192;
  hipLaunchKernelGGL(crnn_to_keras_kernel, dim3((unsigned)b), dim3(256), 0, ctx->stream, in.p, out.p, in.N, in.H, in.wv(),
                     in.C / 4, in.W);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// conv_1 of M crops [M][Hc][Wc] into the cell grid `out` (N rows of cells() cells, cell height out.H = Hc + 1)
int launch_crnn_conv1_cells(kocr_ctx* ctx, const ConvLayer& L, const float* d_crops, int M, int Hc, int Wc, const Tensor& out) {
  if (L.Cin != 1 || L.Cout != 64 || L.KH != 3 || L.KW != 3 || !out.cellW || out.C != 64 || out.cs != 64 || out.co || out.H != Hc + 1 ||
      out.cellWv != Wc || out.cellW < Wc || (size_t)out.N * out.cells() < (size_t)M || L.d_post_a || !L.relu)
    KOCR_FAIL(ctx, KOCR_EINVAL, "crnn_conv1_cells: bad layer / shapes");
  ProfScope ps(ctx, "crnn_conv1_cells", 2.0 * M * Hc * Wc * 9 * 64, 4.0 * ((double)M * Hc * Wc + (double)out.pixels() * 64));
  hipLaunchKernelGGL(crnn_conv1_cells_kernel, dim3((unsigned)(out.N * out.cells()), (unsigned)out.H), dim3(256), 0, ctx->stream, d_crops,
                     L.d_w, L.d_pre_a, L.d_pre_b, out.p, out.amax, M, out.cells(), Hc, Wc, out.H, out.cellW, L.Cout_pad);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// `in` = cell grid (crop rows at cell rows 1 .. in.H - 1), out = [M][cellWv][in.H - 1][C]
int launch_crnn_cells_to_keras(kocr_ctx* ctx, const Tensor& in, const Tensor& out) {
  if (!in.cellW || in.C % 4 || in.cs != in.C || in.co || out.cs != out.C || out.co || out.H != in.cellWv || out.W != in.H - 1 || out.C != in.C ||
      (size_t)in.N * in.cells() < (size_t)out.N)
    KOCR_FAIL(ctx, KOCR_EINVAL, "crnn_cells_to_keras: bad shapes");
  const size_t total = out.pixels() * (in.C / 4);
  if (!total) return KOCR_OK;
  ProfScope ps(ctx, "crnn_to_keras", 0, 8.0 * out.pixels() * in.C);
  size_t b = (total + 255) / 256;
  if (b > 8192) b = 8192;
  hipLaunchKernelGGL(crnn_cells_to_keras_kernel, dim3((unsigned)b), dim3(256), 0, ctx->stream, in.p, out.p, out.N, in.H - 1, in.cellWv,
                     in.C / 4, in.cells(), in.H, in.cellW);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

int launch_stn_sample(kocr_ctx* ctx, const Tensor& x, const float* d_theta, const Tensor& out) {
  if (x.cs != x.C || out.cs != out.C || x.co || out.co) KOCR_FAIL(ctx, KOCR_EINVAL, "stn: dense tensors only");
  const size_t pix = x.pixels();
  if (!pix) return KOCR_OK;
  ProfScope ps(ctx, "stn_sample", 0, 4.0 * pix * x.C * 5);
  hipLaunchKernelGGL(stn_sample_kernel, dim3((unsigned)pix), dim3(128), 0, ctx->stream, x.p, d_theta, out.p, x.N,
                     x.H, x.W, x.C);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// ---- stn_dense_1 (recognition.py:276: Dense(64, relu) over the flattened 50 x 7 x 32 localisation features) ---------------
// A 512 x 11200 x 64 GEMM: four 128-row tiles on the implicit-GEMM kernel left 252 CUs idle for 0.65 ms.  Split-K in two
// deterministic passes: partial[s][m][o] = sum over K slice s (fp32 FMA chain in k order), then out = act(sum_s partial).
constexpr int DSK_ROWS = 16, DSK_KCHUNK = 448;
__global__ __launch_bounds__(256) void dense_splitk_partial_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                  float* __restrict__ partial, int M, int K, int ldw) {
  __shared__ float xs[DSK_ROWS][DSK_KCHUNK + 1];
  const int m0 = blockIdx.x * DSK_ROWS, s = blockIdx.y, k0 = s * DSK_KCHUNK;
  const int kn = min(DSK_KCHUNK, K - k0);
  for (int i = threadIdx.x; i < DSK_ROWS * DSK_KCHUNK; i += 256) {
    const int r = i / DSK_KCHUNK, k = i - r * DSK_KCHUNK;
    xs[r][k] = (m0 + r < M && k < kn) ? x[(size_t)(m0 + r) * K + k0 + k] : 0.f;
  }
  __syncthreads();
  const int o = threadIdx.x & 63, rg = threadIdx.x >> 6;  // output column, group of four rows
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* wp = w + (size_t)k0 * ldw + o;
  for (int k = 0; k < kn; ++k) {
    const float wv = wp[(size_t)k * ldw];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = fmaf(xs[4 * rg + r][k], wv, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (m0 + 4 * rg + r < M) partial[((size_t)s * M + m0 + 4 * rg + r) * 64 + o] = acc[r];
}

__global__ void dense_splitk_reduce_kernel(const float* __restrict__ partial, float* __restrict__ out, const float* __restrict__ pre_a,
                                           const float* __restrict__ pre_b, int M, int S, int relu) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * 64) return;
  float v = 0.f;
  for (int s = 0; s < S; ++s) v += partial[(size_t)s * M * 64 + i];
  v = v * pre_a[i & 63] + pre_b[i & 63];
  out[i] = relu ? fmaxf(v, 0.f) : v;
}

// in: [M][K] contiguous, L: a 1x1 layer with Cout == 64 and Cin == K (weights [Kpad][Cout_pad], k-major), out: [M][64] contiguous;
// d_partial: ceil(K / 448) * M * 64 floats
size_t dense_splitk_workspace(int M, int K) { return (size_t)((K + DSK_KCHUNK - 1) / DSK_KCHUNK) * M * 64 * sizeof(float); }
int launch_dense_splitk(kocr_ctx* ctx, const ConvLayer& L, const float* d_in, float* d_out, float* d_partial, int M) {
  if (L.Cout != 64 || L.KH != 1 || L.KW != 1 || L.d_post_a) KOCR_FAIL(ctx, KOCR_EINVAL, "dense_splitk: unsupported layer " + L.name);
  const int K = L.Cin, S = (K + DSK_KCHUNK - 1) / DSK_KCHUNK;
  ProfScope ps(ctx, "dense_splitk", 2.0 * M * (double)K * 64, 4.0 * ((double)M * K + (double)K * 64));
  hipLaunchKernelGGL(dense_splitk_partial_kernel, dim3((M + DSK_ROWS - 1) / DSK_ROWS, S), dim3(256), 0, ctx->stream, d_in, L.d_w,
                     d_partial, M, K, L.Cout_pad);
  hipLaunchKernelGGL(dense_splitk_reduce_kernel, dim3((M * 64 + 255) / 256), dim3(256), 0, ctx->stream, d_partial, d_out, L.d_pre_a,
                     L.d_pre_b, M, S, L.relu);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

int launch_lstm(kocr_ctx* ctx, const float* d_xp, const float* d_Uf, const float* d_Ub, float* d_out, int M, int T) {
  if (M <= 0) return KOCR_OK;
  const bool old = !ctx->sw.lstm16;
  ProfScope ps(ctx, old ? "lstm_recurrence32" : "lstm_recurrence", 2.0 * 2 * M * (double)T * 128 * 512, 0);
  if (old)
    hipLaunchKernelGGL(lstm_kernel<128>, dim3((M + 31) / 32, 2), dim3(256), 0, ctx->stream, d_xp, d_Uf, d_Ub, d_out, M, T);
  else
    hipLaunchKernelGGL(lstm16_kernel<128>, dim3((M + 15) / 16, 2), dim3(256), 0, ctx->stream, d_xp, d_Uf, d_Ub, d_out, M, T);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// The decode launchers take the batch's character sets `cm` (CharMask, common.h): on -> the MASKED instantiation, with
// cm_bytes more LDS per wave for the crop's mask words; off -> the unmasked one.  The profiler row and the grid are the same.
static size_t cm_bytes(const CharMask& cm, int C) { return cm.on() ? (size_t)((C + 31) / 32) * sizeof(uint32_t) : 0; }

int launch_ctc(kocr_ctx* ctx, const float* d_logits, int M, int T, int C, int discard, int* d_labels, float* d_probs,
               const CharMask& cm) {
  if (M <= 0) return KOCR_OK;
  ProfScope ps(ctx, "ctc_greedy", 0, 4.0 * M * T * C);
  if (cm.on())
    hipLaunchKernelGGL(ctc_kernel<true>, dim3((M + 3) / 4), dim3(256), 4 * cm_bytes(cm, C), ctx->stream, d_logits, M, T, C, discard,
                       d_labels, d_probs, cm);
  else
    hipLaunchKernelGGL(ctc_kernel<false>, dim3((M + 3) / 4), dim3(256), 0, ctx->stream, d_logits, M, T, C, discard, d_labels,
                       d_probs, cm);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// y: device [M][T][C] (logits: fc_12's output, frames t0 .. t0 + T_m - 1; else probabilities, t0 = 0); d_lab: device
// ctc_scores_kernel: labels [M][T - discard], probs (nullable), logw [M], chars [M][T - discard]
int launch_ctc_scores(kocr_ctx* ctx, const float* d_logits, int M, int T, int C, int discard, int* d_labels, float* d_probs,
                      float* d_logw, float* d_chars, const CharMask& cm) {
  if (M <= 0) return KOCR_OK;
  const int To = T - discard;
  const int Sp = (2 * To + 1 + 63) & ~63;
  const size_t lds = (size_t)2 * Sp * sizeof(float) + (size_t)(To + 1) * sizeof(int);
  ProfScope ps(ctx, "ctc_scores", 0, 4.0 * M * T * C * 4);
  if (cm.on())
    hipLaunchKernelGGL(ctc_scores_kernel<true>, dim3(M), dim3(64), lds + cm_bytes(cm, C), ctx->stream, d_logits, T, C, discard, d_labels,
                       d_probs, d_logw, d_chars, Sp, cm);
  else
    hipLaunchKernelGGL(ctc_scores_kernel<false>, dim3(M), dim3(64), lds, ctx->stream, d_logits, T, C, discard, d_labels, d_probs, d_logw,
                       d_chars, Sp, cm);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// ctc_scores_ragged_kernel: one wave per word; labels / chars [M][LW], logw [M]
int launch_ctc_scores_ragged(kocr_ctx* ctx, const float* d_seq, const long long* d_roff, const int* d_T, int M, int C, int LW,
                             int* d_labels, float* d_logw, float* d_chars) {
  if (M <= 0) return KOCR_OK;
  if (LW < 1 || LW > KOCR_WINDOW_FRAMES_MAX || C < 1) KOCR_FAIL(ctx, KOCR_EINVAL, "ctc_scores_ragged: bad sizes");
  // LDS: two alpha rows of Sp floats, Sp = 2 LW + 1 rounded up to 64, then the label row and its length, LW + 1 ints; no
  // mask words (no character sets here).  At LW = KOCR_WINDOW_FRAMES_MAX = 2048: Sp = 4160, 2 * 4160 * 4 + 2049 * 4 =
  // 33 280 + 8 196 = 41 476 bytes, under the 64 KB a workgroup gets without raising the kernel's limit.
  const int Sp = (2 * LW + 1 + 63) & ~63;
  const size_t lds = (size_t)2 * Sp * sizeof(float) + (size_t)(LW + 1) * sizeof(int);
  ProfScope ps(ctx, "ctc_scores_ragged", 0, 4.0 * M * LW * C * 4);
  hipLaunchKernelGGL(ctc_scores_ragged_kernel, dim3(M), dim3(64), lds, ctx->stream, d_seq, d_roff, d_T, C, LW, d_labels, d_logw, d_chars,
                     Sp);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// ctc_beam_kernel: d_labels [M][top_paths][T - discard], d_logp [M][top_paths]
int launch_ctc_beam(kocr_ctx* ctx, const float* d_logits, int M, int T, int C, int discard, int beam_width, int top_paths,
                    int* d_labels, float* d_logp, const CharMask& cm) {
  if (M <= 0) return KOCR_OK;
  const int To = T - discard, B = beam_width;
  if (To < 1 || To > 63 || B < 1 || B > 64 || top_paths < 1 || top_paths > B || C < 1)
    KOCR_FAIL(ctx, KOCR_EINVAL, "ctc_beam: bad sizes");
  const int Sp = (2 * To + 1 + 63) & ~63, Ls = To | 1;
  const size_t lds = (size_t)2 * B * (4 * Ls + 32) + (size_t)8 * Sp + 1024;
  ProfScope ps(ctx, "ctc_beam", 0, 4.0 * M * T * C * (2 + top_paths));
  if (cm.on())
    hipLaunchKernelGGL(ctc_beam_kernel<true>, dim3(M), dim3(64), lds + cm_bytes(cm, C), ctx->stream, d_logits, T, C, discard, B, top_paths,
                       d_labels, d_logp, Sp, Ls, cm);
  else
    hipLaunchKernelGGL(ctc_beam_kernel<false>, dim3(M), dim3(64), lds, ctx->stream, d_logits, T, C, discard, B, top_paths, d_labels, d_logp,
                       Sp, Ls, cm);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// [M][lstride]; d_len / d_in_len: device [M], validated on the host (ctc_check); d_loss: device [M]
int launch_ctc_loss(kocr_ctx* ctx, bool logits, const float* d_y, int M, int T, int C, int t0, const int* d_lab, int lstride,
                    const int* d_len, const int* d_in_len, float* d_loss, int Lmax) {
  if (M <= 0) return KOCR_OK;
  const int Sp = (2 * Lmax + 1 + 63) & ~63;
  const size_t lds = 2 * (size_t)Sp * sizeof(float);
  if (lds > 64 * 1024) KOCR_FAIL(ctx, KOCR_ECAPACITY, "ctc_loss: labels longer than 8159 are not supported");
  ProfScope ps(ctx, logits ? "ctc_loss_logits" : "ctc_loss", 0, 4.0 * M * T * C * (logits ? 3 : 1));
  if (logits)
    hipLaunchKernelGGL(ctc_loss_kernel<true>, dim3(M), dim3(64), lds, ctx->stream, d_y, T, C, t0, d_lab, lstride, d_len, d_in_len,
                       d_loss, Sp);
  else
    hipLaunchKernelGGL(ctc_loss_kernel<false>, dim3(M), dim3(64), lds, ctx->stream, d_y, T, C, t0, d_lab, lstride, d_len, d_in_len,
                       d_loss, Sp);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// ---- lexicon ("Lexicon"): which of the caller's V words is this crop?  value[m][v] = the exact CTC
// log-probability of word v given crop m, -kocr_crnn_ctc_loss, for every pair; three launches per chunk of crops.
//   lexicon_logq_kernel    per (crop, frame) one wave: the To x C table lq_t(c) = logf(ctc_softmax(..) + CTC_EPS) - logz, the
//                          very expressions of ctc_loss_wave<true>, computed ONCE per crop instead of once per pair
//   lexicon_score_kernel   the forward algorithm of every (crop, word) pair, one LANE per word
//   lexicon_select_kernel  per crop the top_words best values, each rescored by ctc_loss_wave<true>
// The recursion stays in float32 LOG space, state by state the arithmetic of ctc_loss_wave (ctc_lse3 + lq, the same masks):
// a linear-domain recursion with a per-frame rescale loses the states that lie more than 2^-149 below the frame's largest,
// and on a peaked network (q of a wrong class at the 1e-7 floor) a word that disagrees with the crop in six or more
// letters carries its surviving paths through exactly such states until the end mask forces them forward.
// A lane keeps log(alpha) of its word's 2L + 1 states and the L labels in its own LDS row of R = (3 Lmax + 1) | 1 words (odd:
// the lanes of a wave touching the same state hit different banks) and updates alpha IN PLACE from the highest live state
// down: new[s] needs old[s], old[s-1], old[s-2] only, carried in three registers, so a state costs one LDS read, one LDS
// write and, at odd s, the gather lq_t(label).  TAB_LDS: the crop's table is copied into LDS (To x C floats: 7.1 KB for 37
// classes) and the gather is an LDS read; when table + rows exceed 64 KB (a 1000-class alphabet: 192 KB) the gather reads
// the table from global memory, i.e. L2 / the vector cache.  The launcher sorts nothing: `order` (host-made at load time)
// lists the words by ascending length, so the 64 words of a wave run the same trip count; results land in the CALLER's order.
// Nothing is shared between crops and every order of evaluation is fixed: a crop's values are the same bits in any batch.
constexpr int LEX_BLOCK = 128;  // words (= lanes) per workgroup of lexicon_score_kernel, all of one crop

// MASKED: the table of the masked rows (a masked class: logf(CTC_EPS) - logz, finite); the wave's one row takes the crop's
// mask words through LDS once.  lexicon_score_kernel reads only this table and needs no mask of its own.
template <bool MASKED>
__global__ __launch_bounds__(64) void lexicon_logq_kernel(const float* __restrict__ logits, int T, int C, int discard,
                                                          float* __restrict__ lq, CharMask cm) {
  const int To = T - discard, m = blockIdx.x / To, t = blockIdx.x % To, lane = threadIdx.x;
  const float* row = logits + ((size_t)m * T + discard + t) * C;
  const uint32_t* w = nullptr;
  if constexpr (MASKED) {
    extern __shared__ uint32_t cm_words[];
    cm_load(cm.bits, cm.set_of, cm.uniform, cm.shift, cm.first, m, C, lane, cm_words);
    __syncthreads();
    w = cm_words;
  }
  float mx;
  int bi;
  ctc_row_argmax<MASKED>(row, C, lane, mx, bi, w);
  const float es = ctc_row_expsum<MASKED>(row, C, lane, mx, w);
  float z = 0.f;
  for (int c = lane; c < C; c += 64) z += ctc_softmax(cm_at<MASKED>(row, w, c), mx, es) + CTC_EPS;
  for (int o = 32; o; o >>= 1) z += __shfl_xor(z, o);
  const float logz = logf(z);
  float* out = lq + ((size_t)m * To + t) * C;
  for (int c = lane; c < C; c += 64) out[c] = logf(ctc_softmax(cm_at<MASKED>(row, w, c), mx, es) + CTC_EPS) - logz;
}

// lq: [Mc][To][C]; words: [V][wstride] / lens: [V] in the caller's order; order: [V] sorted position -> caller index;
// values: [Mc][V] in the caller's order.  Grid (ceil(V / LEX_BLOCK), Mc).  LDS: TAB_LDS ? To * C : 0 floats, then LEX_BLOCK * R.
template <bool TAB_LDS>
__global__ __launch_bounds__(LEX_BLOCK) void lexicon_score_kernel(const float* __restrict__ lq, int To, int C,
                                                                  const int* __restrict__ words, int wstride,
                                                                  const int* __restrict__ lens, const int* __restrict__ order,
                                                                  int V, int Lmax, int R, float* __restrict__ values) {
  extern __shared__ float lex_lds[];
  const int m = blockIdx.y, j = blockIdx.x * LEX_BLOCK + threadIdx.x;
  const float* lqm = lq + (size_t)m * To * C;
  if (TAB_LDS)
    for (int i = threadIdx.x; i < To * C; i += LEX_BLOCK) lex_lds[i] = lqm[i];
  float* A = lex_lds + (TAB_LDS ? To * C : 0) + (size_t)threadIdx.x * R;  // [2 Lmax + 1] log alpha
  int* Lb = reinterpret_cast<int*>(A + 2 * Lmax + 1);                      // [Lmax] the word
  int w = 0, L = 0;
  if (j < V) {
    w = order[j];
    L = lens[w];
    for (int i = 0; i < L; ++i) Lb[i] = words[(size_t)w * wstride + i];
  }
  __syncthreads();
  if (j >= V) return;
  auto Q = [&](int i) { return TAB_LDS ? lex_lds[i] : lqm[i]; };
  const int S = 2 * L + 1, blank = C - 1;
  for (int s = 0; s < S; ++s) A[s] = -INFINITY;
  for (int t = 0; t < To; ++t) {
    // ctc_loss_wave's masks: s > 2t + 1 cannot be reached yet, s < S - 2 (To - t) can no longer reach the end
    const int lo = max(0, S - 2 * (To - t)), hi = min(S - 1, 2 * t + 1);
    const float lqb = Q(t * C + blank);
    if (t == 0) {
      for (int s = lo; s <= hi; ++s) A[s] = (s & 1) ? Q(Lb[0]) : lqb;  // hi <= 1
      continue;
    }
    float c0 = A[hi], c1 = hi >= 1 ? A[hi - 1] : -INFINITY;  // old[s], old[s - 1]
    for (int s = hi; s >= lo; --s) {
      const float c2 = s >= 2 ? A[s - 2] : -INFINITY;
      float a2 = -INFINITY, lqs = lqb;
      if (s & 1) {
        const int k = s >> 1, lab = Lb[k];
        lqs = Q(t * C + lab);
        if (k >= 1 && lab != Lb[k - 1]) a2 = c2;
      }
      A[s] = ctc_lse3(c0, c1, a2) + lqs;
      c0 = c1;
      c1 = c2;
    }
    if (lo >= 1) A[lo - 1] = -INFINITY;
    if (lo >= 2) A[lo - 2] = -INFINITY;
  }
  const float a = A[S - 1], b = A[S - 2];  // L >= 1
  const float mxv = fmaxf(a, b);
  values[(size_t)m * V + w] = mxv == -INFINITY ? -INFINITY : mxv + logf(expf(a - mxv) + expf(b - mxv));
}

// One wave (= one workgroup) per crop.  K rounds of "the largest value behind the last pick" over the crop's V values (the
// higher value first, then the smaller index; -inf is never picked), then ctc_loss_wave<true> on each pick -- log_prob is,
// bit for bit, -kocr_crnn_ctc_loss of the crop with that word -- and the rows in the order of the rescored value (same tie
// rule); behind them index -1, log_prob -inf.  LDS: the loss's la [2][Sp], then val [64], idx [64].
// MASKED: the rescoring reads the rows through the crop's mask words, kept behind idx.
template <bool MASKED>
__global__ __launch_bounds__(64) void lexicon_select_kernel(const float* __restrict__ logits, int T, int C, int discard,
                                                            const float* __restrict__ values, int V, const int* __restrict__ words,
                                                            int wstride, const int* __restrict__ lens, int K,
                                                            int* __restrict__ index, float* __restrict__ logp, int Sp, CharMask cm) {
  extern __shared__ float la[];
  float* val = la + 2 * Sp;
  int* idx = reinterpret_cast<int*>(val + 64);
  const int m = blockIdx.x, lane = threadIdx.x, To = T - discard;
  const float* y0 = logits + ((size_t)m * T + discard) * C;
  const uint32_t* w = nullptr;
  if constexpr (MASKED) {
    uint32_t* mine = reinterpret_cast<uint32_t*>(idx + 64);
    cm_load(cm.bits, cm.set_of, cm.uniform, cm.shift, cm.first, m, C, lane, mine);  // the __syncthreads() behind the selection rounds orders it before the first read
    w = mine;
  }
  const float* v = values + (size_t)m * V;
  float pv = INFINITY;
  int pi = -1, n = 0;
  for (; n < K; ++n) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < V; i += 64) {
      const float x = v[i];
      if ((x < pv || (x == pv && i > pi)) && x > bv) {  // ascending i: the first maximum of a lane wins
        bv = x;
        bi = i;
      }
    }
    for (int o = 32; o; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (bv == -INFINITY) break;  // uniform: fewer than K feasible words
    pv = bv;
    pi = bi;
    if (lane == 0) idx[n] = bi;
  }
  __syncthreads();
  float lp = -INFINITY;
  int mine = -1;
  for (int k = 0; k < n; ++k) {
    const int wd = idx[k];
    const float loss = ctc_loss_wave<true, MASKED>(y0, C, words + (size_t)wd * wstride, lens[wd], To, la, Sp, lane, w);
    if (lane == k) {
      lp = -loss;
      mine = wd;
    }
  }
  __syncthreads();
  val[lane] = lp;
  __syncthreads();
  if (lane < K) {
    int rank = lane;
    if (lane < n) {
      rank = 0;
      for (int j = 0; j < n; ++j) {
        if (j == lane) continue;
        const float vj = val[j];
        rank += (vj > lp || (vj == lp && idx[j] < mine)) ? 1 : 0;
      }
    }
    index[(size_t)m * K + rank] = mine;
    logp[(size_t)m * K + rank] = lp;
  }
}

// d_lq: [M][T - discard][C] scratch
int launch_lexicon_logq(kocr_ctx* ctx, const float* d_logits, int M, int T, int C, int discard, float* d_lq, const CharMask& cm) {
  if (M <= 0) return KOCR_OK;
  ProfScope ps(ctx, "lexicon_logq", 0, 4.0 * M * (T - discard) * C * 2);
  if (cm.on())
    hipLaunchKernelGGL(lexicon_logq_kernel<true>, dim3(M * (T - discard)), dim3(64), cm_bytes(cm, C), ctx->stream, d_logits, T, C, discard,
                       d_lq, cm);
  else
    hipLaunchKernelGGL(lexicon_logq_kernel<false>, dim3(M * (T - discard)), dim3(64), 0, ctx->stream, d_logits, T, C, discard, d_lq, cm);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// d_values: [M][V], the caller's word order
int launch_lexicon_score(kocr_ctx* ctx, const float* d_lq, int M, int To, int C, const int* d_words, int wstride, const int* d_lens,
                         const int* d_order, int V, int Lmax, float* d_values) {
  if (M <= 0 || V <= 0) return KOCR_OK;
  if (Lmax < 1 || Lmax > KOCR_LEXICON_MAX_WORD || To < 1 || C < 2) KOCR_FAIL(ctx, KOCR_EINVAL, "lexicon_score: bad sizes");
  const int R = (3 * Lmax + 1) | 1;
  const size_t rows = (size_t)LEX_BLOCK * R * sizeof(float), tab = (size_t)To * C * sizeof(float);
  const bool tab_lds = rows + tab <= 64 * 1024;
  const dim3 grid((V + LEX_BLOCK - 1) / LEX_BLOCK, M);
  // per pair To frames of about 2L + 1 states, each three expf, a logf and some twenty other operations
  ProfScope ps(ctx, "lexicon_score", 30.0 * M * V * To * (Lmax + 1), 4.0 * M * V);
  if (tab_lds)
    hipLaunchKernelGGL(lexicon_score_kernel<true>, grid, dim3(LEX_BLOCK), rows + tab, ctx->stream, d_lq, To, C, d_words, wstride,
                       d_lens, d_order, V, Lmax, R, d_values);
  else
    hipLaunchKernelGGL(lexicon_score_kernel<false>, grid, dim3(LEX_BLOCK), rows, ctx->stream, d_lq, To, C, d_words, wstride, d_lens,
                       d_order, V, Lmax, R, d_values);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// d_index / d_logp: [M][top_words]
int launch_lexicon_select(kocr_ctx* ctx, const float* d_logits, int M, int T, int C, int discard, const float* d_values, int V,
                          const int* d_words, int wstride, const int* d_lens, int top_words, int* d_index, float* d_logp,
                          const CharMask& cm) {
  if (M <= 0) return KOCR_OK;
  if (top_words < 1 || top_words > 64 || V < 1) KOCR_FAIL(ctx, KOCR_EINVAL, "lexicon_select: bad sizes");
  const int Sp = (2 * KOCR_LEXICON_MAX_WORD + 1 + 63) & ~63;
  const size_t lds = (size_t)2 * Sp * sizeof(float) + 64 * sizeof(float) + 64 * sizeof(int);
  ProfScope ps(ctx, "lexicon_select", 0, 4.0 * M * V * top_words);
  if (cm.on())
    hipLaunchKernelGGL(lexicon_select_kernel<true>, dim3(M), dim3(64), lds + cm_bytes(cm, C), ctx->stream, d_logits, T, C, discard,
                       d_values, V, d_words, wstride, d_lens, top_words, d_index, d_logp, Sp, cm);
  else
    hipLaunchKernelGGL(lexicon_select_kernel<false>, dim3(M), dim3(64), lds, ctx->stream, d_logits, T, C, discard, d_values, V, d_words,
                       wstride, d_lens, top_words, d_index, d_logp, Sp, cm);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// ---- patterns ("Patterns"): the best CTC alignment whose collapsed text a regular expression accepts.
// The pattern is a trimmed deterministic automaton (kocr_set_patterns); a NODE is (state, blank) or (state, label c) for a
// label that enters the state, in the order state ascending, blank first, labels ascending.  Viterbi over (frame x node) on
// the To x C table of lexicon_logq_kernel<false>: V_0 = 0 at node 0 = (0, blank), -inf elsewhere; per frame
//   (s, blank)  the best of itself, then the label nodes of s
//   (s, c)      the best of itself, then for every p with delta[p][c] == s (ascending): (p, blank), the nodes (p, c'), c' != c
// the FIRST of the largest, then + lq_t(blank or c): one float32 add per node per frame, in frame order.
//   pattern_viterbi_kernel  one workgroup per crop, the lanes over the nodes, the frame loop inside.  Phase A reduces the label
//                           nodes of every state to their best and second best (two distinct labels; first of the largest, so
//                           the smaller label); phase B then costs a label node its predecessor STATES, not their nodes: per
//                           p the blank node, then the best label node that is not c.  That is the statement's candidate
//                           order.  After the last frame the first of the largest among the accepting nodes, and lane 0 walks
//                           the 16-bit back-pointers into the label row.
//   pattern_rescore_kernel  ctc_loss_wave<true> on that row: log_prob == -kocr_crnn_ctc_loss of it, bit for bit.
// LDS: two value rows [NTmax], the per-state reductions, the crop's table when TAB_LDS, the back-pointers [To][NT] when
// BP_LDS (else they lie in the workspace, To x NTmax per crop).  Which of the two a launch takes changes no result.
// Device tables per pattern p: hdr[p] = {S, NT, first node, first state, first pred, ...}; nodes[i] = (label | state << 16,
// first pred) with label 0xffff for a blank node, one entry behind the last; states[s] = (its blank node, accept), one entry
// behind the last; pred: the predecessor states of the label nodes.
// Nothing is shared between crops and every order of evaluation is fixed: a crop's rows are the same bits in any batch.
constexpr int PAT_BLOCK = 256;
constexpr unsigned PAT_NONE = 0xffffffffu;

template <bool TAB_LDS, bool BP_LDS>
__global__ __launch_bounds__(PAT_BLOCK) void pattern_viterbi_kernel(const float* __restrict__ lq, int To, int C, PatternTables pt,
                                                                    const int32_t* __restrict__ pat_of, int uniform, int first,
                                                                    int NTmax, int Smax, unsigned short* __restrict__ bp_ws,
                                                                    int* __restrict__ labels, float* __restrict__ log_path) {
  extern __shared__ float pat_lds[];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int p = pat_of ? pat_of[first + m] : uniform;
  int* lab = labels + (size_t)m * To;
  const int* h = pt.hdr + (p < 0 ? 0 : p) * 8;
  const int S = h[0], NT = h[1];
  if (p < 0 || NT > NTmax || S > Smax) {  // no pattern for this crop (the launcher sizes NTmax / Smax for every pattern it is given)
    for (int i = tid; i < To; i += PAT_BLOCK) lab[i] = -1;
    if (tid == 0) log_path[m] = -INFINITY;
    return;
  }
  const int2* nodes = pt.nodes + h[2];
  const int2* states = pt.states + h[3];
  const int* pred = pt.pred + h[4];
  float* val = pat_lds;                                          // [2][NTmax]
  float* b1v = val + 2 * NTmax;                                  // [Smax] best label node of the state: value
  float* b2v = b1v + Smax;                                       // [Smax] second best
  unsigned* b1i = reinterpret_cast<unsigned*>(b2v + Smax);       // [Smax] label << 16 | node
  unsigned* b2i = b1i + Smax;                                    // [Smax]
  float* redv = reinterpret_cast<float*>(b2i + Smax);            // [PAT_BLOCK]
  int* redi = reinterpret_cast<int*>(redv + PAT_BLOCK);          // [PAT_BLOCK]
  float* tab = reinterpret_cast<float*>(redi + PAT_BLOCK);       // [To * C] when TAB_LDS
  unsigned short* bp = BP_LDS ? reinterpret_cast<unsigned short*>(tab + (TAB_LDS ? To * C : 0)) : bp_ws + (size_t)m * To * NTmax;
  const float* lqm = lq + (size_t)m * To * C;
  if (TAB_LDS)
    for (int i = tid; i < To * C; i += PAT_BLOCK) tab[i] = lqm[i];
  for (int i = tid; i < NT; i += PAT_BLOCK) val[i] = i == 0 ? 0.f : -INFINITY;
  __syncthreads();
  auto Q = [&](int i) { return TAB_LDS ? tab[i] : lqm[i]; };
  const int blank = C - 1;
  for (int t = 0; t < To; ++t) {
    const float* cur = val + (t & 1) * NTmax;
    float* nxt = val + ((t & 1) ^ 1) * NTmax;
    // phase A: per state the best and the second best of its label nodes
    for (int s = tid; s < S; s += PAT_BLOCK) {
      const int b = states[s].x, e = states[s + 1].x;
      float v1 = -INFINITY, v2 = -INFINITY;
      int i1 = -1, i2 = -1;
      for (int i = b + 1; i < e; ++i) {
        const float v = cur[i];
        if (v > v1) {
          v2 = v1;
          i2 = i1;
          v1 = v;
          i1 = i;
        } else if (v > v2) {
          v2 = v;
          i2 = i;
        }
      }
      b1v[s] = v1;
      b2v[s] = v2;
      b1i[s] = i1 < 0 ? PAT_NONE : ((unsigned)nodes[i1].x << 16) | (unsigned)i1;
      b2i[s] = i2 < 0 ? PAT_NONE : ((unsigned)nodes[i2].x << 16) | (unsigned)i2;
    }
    __syncthreads();
    // phase B: every node's best predecessor, the stay first
    for (int i = tid; i < NT; i += PAT_BLOCK) {
      const int2 nd = nodes[i];
      const unsigned label = (unsigned)nd.x & 0xffffu;
      float best = cur[i];
      int from = i;
      float q;
      if (label == 0xffffu) {
        const int s = nd.x >> 16;
        const float v = b1v[s];
        if (v > best) {
          best = v;
          from = (int)(b1i[s] & 0xffffu);
        }
        q = Q(t * C + blank);
      } else {
        const int ke = nodes[i + 1].y;
        for (int k = nd.y; k < ke; ++k) {
          const int ps = pred[k];
          const int pb = states[ps].x;
          float v = cur[pb];
          if (v > best) {
            best = v;
            from = pb;
          }
          unsigned u = b1i[ps];
          v = b1v[ps];
          if ((u >> 16) == label) {
            u = b2i[ps];
            v = b2v[ps];
          }
          if (v > best) {
            best = v;
            from = (int)(u & 0xffffu);
          }
        }
        q = Q(t * C + (int)label);
      }
      nxt[i] = best + q;
      bp[(size_t)t * NT + i] = (unsigned short)from;
    }
    __syncthreads();
  }
  // the first of the largest among the accepting nodes
  const float* fin = val + (To & 1) * NTmax;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = tid; i < NT; i += PAT_BLOCK) {
    const float v = fin[i];
    if (states[nodes[i].x >> 16].y && v > bv) {
      bv = v;
      bi = i;
    }
  }
  redv[tid] = bv;
  redi[tid] = bi;
  __syncthreads();
  if (tid != 0) return;
  for (int j = 1; j < PAT_BLOCK; ++j) {
    const float v = redv[j];
    const int i = redi[j];
    if (v > bv || (v == bv && i < bi)) {
      bv = v;
      bi = i;
    }
  }
  log_path[m] = bv;
  int n = 0;
  if (bv != -INFINITY) {
    int node = bi;
    for (int t = To - 1; t >= 0; --t) {  // the text backwards into redi (To <= PAT_BLOCK)
      const int from = bp[(size_t)t * NT + node];
      const int label = nodes[node].x & 0xffff;
      if (label != 0xffff && from != node) redi[n++] = label;
      node = from;
    }
  }
  for (int k = 0; k < To; ++k) lab[k] = k < n ? redi[n - 1 - k] : -1;
}

// One wave (= one workgroup) per crop: the label row of pattern_viterbi_kernel rescored by ctc_loss_wave<true>.
// LDS: the loss's la [2][Sp], then int[To]: the label.
__global__ __launch_bounds__(64) void pattern_rescore_kernel(const float* __restrict__ logits, int T, int C, int discard,
                                                             const int* __restrict__ labels, const float* __restrict__ log_path,
                                                             float* __restrict__ logp, int Sp) {
  extern __shared__ float la[];
  int* dec = reinterpret_cast<int*>(la + 2 * Sp);
  const int m = blockIdx.x, lane = threadIdx.x, To = T - discard;
  if (log_path[m] == -INFINITY) {  // uniform: nothing fits (or no pattern)
    if (lane == 0) logp[m] = -INFINITY;
    return;
  }
  int L = 0;
  for (int i = lane; i < To; i += 64) {
    const int v = labels[(size_t)m * To + i];
    dec[i] = v;
    L += v >= 0 ? 1 : 0;
  }
  for (int o = 32; o; o >>= 1) L += __shfl_xor(L, o);
  __syncthreads();
  const float loss = ctc_loss_wave<true>(logits + ((size_t)m * T + discard) * C, C, dec, L, To, la, Sp, lane);
  if (lane == 0) logp[m] = -loss;
}

// The LDS of one pattern_viterbi_kernel launch over patterns of at most NTmax nodes and Smax states: what always lies there,
// then the table and the back-pointers while the budget holds them.
constexpr size_t PAT_LDS_BUDGET = 64 * 1024;
static size_t pattern_lds(int To, int C, int NTmax, int Smax, bool* tab_lds, bool* bp_lds) {
  size_t b = ((size_t)2 * NTmax + 4 * (size_t)Smax + 2 * PAT_BLOCK) * sizeof(float);
  const size_t tab = (size_t)To * C * sizeof(float), bp = (size_t)To * NTmax * sizeof(unsigned short);
  *tab_lds = b + tab <= PAT_LDS_BUDGET;
  if (*tab_lds) b += tab;
  *bp_lds = b + bp <= PAT_LDS_BUDGET;
  if (*bp_lds) b += bp;
  return b;
}

size_t pattern_bp_bytes(int To, int C, int NTmax, int Smax) {
  bool tab_lds, bp_lds;
  pattern_lds(To, C, NTmax, Smax, &tab_lds, &bp_lds);
  return bp_lds ? 0 : (size_t)To * NTmax * sizeof(unsigned short);
}

// d_lq: [M][To][C] of launch_lexicon_logq; d_bp: [M][To][NTmax] 16-bit workspace (pattern_bp_bytes; unused when 0);
// d_labels [M][To], d_logpath / d_logp [M]
int launch_pattern(kocr_ctx* ctx, const float* d_logits, const float* d_lq, int M, int T, int C, int discard, const PatternTables& pt,
                   const int32_t* d_pat_of, int uniform, int first, int NTmax, int Smax, void* d_bp, int* d_labels, float* d_logpath,
                   float* d_logp) {
  if (M <= 0) return KOCR_OK;
  const int To = T - discard;
  if (To < 1 || To > PAT_BLOCK || C < 2 || NTmax < 1 || Smax < 1) KOCR_FAIL(ctx, KOCR_EINVAL, "pattern_viterbi: bad sizes");
  bool tab_lds, bp_lds;
  const size_t lds = pattern_lds(To, C, NTmax, Smax, &tab_lds, &bp_lds);
  if (lds > PAT_LDS_BUDGET) KOCR_FAIL(ctx, KOCR_EINVAL, "pattern_viterbi: the value rows exceed the LDS budget");
  if (!bp_lds && !d_bp) KOCR_FAIL(ctx, KOCR_EINVAL, "pattern_viterbi: no back-pointer workspace");
  {
    ProfScope ps(ctx, "pattern_viterbi", 8.0 * M * To * NTmax, 4.0 * M * To * C + (bp_lds ? 0.0 : 2.0 * M * To * NTmax));
    unsigned short* bp = (unsigned short*)d_bp;
#define KOCR_PAT_LAUNCH(TAB, BP)                                                                                                     \
  hipLaunchKernelGGL((pattern_viterbi_kernel<TAB, BP>), dim3(M), dim3(PAT_BLOCK), lds, ctx->stream, d_lq, To, C, pt, d_pat_of, uniform, \
                     first, NTmax, Smax, bp, d_labels, d_logpath)
    if (tab_lds && bp_lds) KOCR_PAT_LAUNCH(true, true);
    else if (tab_lds) KOCR_PAT_LAUNCH(true, false);
    else if (bp_lds) KOCR_PAT_LAUNCH(false, true);
    else KOCR_PAT_LAUNCH(false, false);
#undef KOCR_PAT_LAUNCH
    KOCR_HIP(ctx, hipGetLastError());
  }
  const int Sp = (2 * To + 1 + 63) & ~63;
  ProfScope ps(ctx, "pattern_rescore", 0, 4.0 * M * To * C);
  hipLaunchKernelGGL(pattern_rescore_kernel, dim3(M), dim3(64), (size_t)2 * Sp * sizeof(float) + To * sizeof(int), ctx->stream, d_logits, T,
                     C, discard, d_labels, d_logpath, d_logp, Sp);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}
