// orient.hip — the choice between the two readings of a word ("Orientation"; statement:
// tests/orientation_statement.py).  The crop stage has warped every box twice (warp.hip: warp_prepare_turned_kernel), the
// recogniser has read both crops with its scores; per word, candidate 1 wins iff
//   (n_1 > 0 and n_0 == 0) or ((n_1 > 0) == (n_0 > 0) and v_1 > v_0)
// with n_c the number of decoded labels (entries >= 0) and v_c the exact CTC log-probability of candidate c's own decode
// (ctc_scores_kernel's log_word): an empty decode loses to a non-empty one, otherwise the larger value wins, a tie or a NaN
// keeps candidate 0.  The winner's rows are copied into compact [M] buffers; nothing is computed.
#include "common.h"

namespace {
constexpr int SELECT_WAVES = 4;  // words per block
}

// One wave per word, lanes over the label width.  in: lab [M][2][LW], logw [M][2], chars [M][2][LW], turns [M][2], quads
// [M][2][8].  out: lab [M][LW], logw [M], chars [M][LW], turn [M], quad [M][8], pair [M][2] = (v_0, v_1).
__global__ void orient_select_kernel(const int* __restrict__ lab, const float* __restrict__ logw, const float* __restrict__ chars,
                                     const int* __restrict__ turns, const float* __restrict__ quads, int M, int LW,
                                     int* __restrict__ o_lab, float* __restrict__ o_logw, float* __restrict__ o_chars,
                                     int* __restrict__ o_turn, float* __restrict__ o_quad, float* __restrict__ o_pair) {
  const int lane = threadIdx.x & 63;
  const long m = (long)blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);
  if (m >= M) return;  // whole waves leave: no barrier below
  const int* l0 = lab + (size_t)m * 2 * LW;
  const int* l1 = l0 + LW;
  bool some0 = false, some1 = false;
  for (int l = lane; l < LW; l += 64) {
    some0 |= l0[l] >= 0;
    some1 |= l1[l] >= 0;
  }
  const bool any0 = __ballot(some0) != 0, any1 = __ballot(some1) != 0;  // wave-uniform
  const float v0 = logw[2 * m], v1 = logw[2 * m + 1];
  const int win = ((any1 && !any0) || (any1 == any0 && v1 > v0)) ? 1 : 0;
  const size_t src = (size_t)(2 * m + win);
  for (int l = lane; l < LW; l += 64) {
    o_lab[(size_t)m * LW + l] = lab[src * LW + l];
    o_chars[(size_t)m * LW + l] = chars[src * LW + l];
  }
  if (lane < 8) o_quad[(size_t)m * 8 + lane] = quads[src * 8 + lane];
  if (lane == 8) o_logw[m] = win ? v1 : v0;
  if (lane == 9) o_turn[m] = turns[src];
  if (lane == 10) o_pair[2 * m] = v0;
  if (lane == 11) o_pair[2 * m + 1] = v1;
}

int launch_orient_select(kocr_ctx* ctx, const int* d_lab, const float* d_logw, const float* d_chars, const int* d_turns,
                         const float* d_quads, long M, int LW, int* o_lab, float* o_logw, float* o_chars, int* o_turn, float* o_quad,
                         float* o_pair) {
  if (M <= 0) return KOCR_OK;
  ProfScope ps(ctx, "orient_select", 0, (double)M * (LW * 24.0 + 128.0));
  hipLaunchKernelGGL(orient_select_kernel, dim3((unsigned)((M + SELECT_WAVES - 1) / SELECT_WAVES)), dim3(64 * SELECT_WAVES), 0,
                     ctx->stream, d_lab, d_logw, d_chars, d_turns, d_quads, (int)M, LW, o_lab, o_logw, o_chars, o_turn, o_quad, o_pair);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}
