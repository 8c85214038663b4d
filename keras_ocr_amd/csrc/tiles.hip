// tiles.hip — the two copies of a tiled detector pass ("Tiled pages"; statement:
// tests/tiling_statement.py).  The resized page lies in a canvas that the tile plan (tile_plan, common.h) covers exactly;
// tile_gather copies the overlapping tiles out of it into the batch the detector runs on, heat_stitch copies every pixel of
// the page's heat-map from the one tile whose core contains it.  Nothing is computed: both are bit-exact by construction
// and independent of the launch geometry.
//
// Every origin is a multiple of the stride (a multiple of 32 input pixels) and every core bound a multiple of 16, so a tile
// row starts at a multiple of 96 bytes of the uint8 canvas and is a multiple of 96 bytes long, and a core row starts at a
// multiple of 64 bytes of a heat tile: one lane moves 16 bytes, unconditionally.  The pointers themselves must be 16-byte
// aligned (the launchers check).
#include "common.h"

namespace {
constexpr int COPY_BLOCK = 256;
// a memory-bound copy: as many blocks as there are 16-byte chunks, at most 8 per compute unit, the rest by grid stride
unsigned copy_grid(const kocr_ctx* ctx, size_t chunks) {
  const size_t blocks = (chunks + COPY_BLOCK - 1) / COPY_BLOCK;
  const size_t most = (size_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 8;
  return (unsigned)(blocks < most ? blocks : most);
}
}  // namespace

// canvas [N][Hc][Wc][3] uint8 -> tiles [N][ny * nx][T][T][3] uint8, tile (ky, kx) from the canvas rows ky S .., columns kx S ..
// One chunk = 16 bytes of a tile row; row_chunks = 3 T / 16.
__global__ void tile_gather_kernel(const uint4* __restrict__ canvas, uint4* __restrict__ tiles, TilePlan p, size_t chunks) {
  const unsigned row_chunks = 3u * (unsigned)p.T / 16u, canvas_row = 3u * (unsigned)p.Wc / 16u, step = 3u * (unsigned)p.S / 16u;
  for (size_t c = (size_t)blockIdx.x * COPY_BLOCK + threadIdx.x; c < chunks; c += (size_t)gridDim.x * COPY_BLOCK) {
    const size_t row = c / row_chunks;  // (image, tile, tile row)
    const unsigned q = (unsigned)(c - row * row_chunks);
    const size_t t = row / (unsigned)p.T;
    const unsigned r = (unsigned)(row - t * (unsigned)p.T);
    const size_t n = t / (unsigned)p.nT;
    const unsigned k = (unsigned)(t - n * (unsigned)p.nT), ky = k / (unsigned)p.nx, kx = k - ky * (unsigned)p.nx;
    const size_t y = (size_t)ky * p.S + r;  // < Hc: (ny - 1) S + T = Hc
    tiles[c] = canvas[(n * p.Hc + y) * canvas_row + (size_t)kx * step + q];
  }
}

// heat tiles [N][ny * nx][T/2][T/2][2] float32 -> page [N][Hc/2][Wc/2][2]: one chunk = two neighbouring page pixels (16 bytes),
// which no core bound separates (bounds are multiples of 8 heat pixels).  Along an axis the pixel v belongs to tile
// k = 0 for v < O/2, else min(n - 1, (v - O/2) / (S/2)): the cores [k S + O, (k + 1) S + O) of the plan, halved, the first
// starting at 0 and the last ending at the canvas.
__global__ void heat_stitch_kernel(const uint4* __restrict__ tiles, uint4* __restrict__ page, TilePlan p, size_t chunks) {
  const unsigned w2 = (unsigned)p.Wc / 2, h2 = (unsigned)p.Hc / 2, t2 = (unsigned)p.T / 2, s2 = (unsigned)p.S / 2, o2 = (unsigned)p.O / 2;
  const unsigned row_chunks = w2 / 2, tile_row = t2 / 2;
  for (size_t c = (size_t)blockIdx.x * COPY_BLOCK + threadIdx.x; c < chunks; c += (size_t)gridDim.x * COPY_BLOCK) {
    const size_t row = c / row_chunks;  // (image, page row)
    const unsigned x = 2u * (unsigned)(c - row * row_chunks);
    const size_t n = row / h2;
    const unsigned y = (unsigned)(row - n * h2);
    unsigned ky = y < o2 ? 0u : (y - o2) / s2, kx = x < o2 ? 0u : (x - o2) / s2;
    ky = ky < (unsigned)p.ny - 1 ? ky : (unsigned)p.ny - 1;
    kx = kx < (unsigned)p.nx - 1 ? kx : (unsigned)p.nx - 1;
    const unsigned ly = y - ky * s2, lx = x - kx * s2;  // < T/2: the core lies inside its tile
    page[c] = tiles[((n * p.nT + (size_t)ky * p.nx + kx) * t2 + ly) * tile_row + lx / 2];
  }
}

// d_canvas: N canvases of p.Hc x p.Wc x 3 bytes; d_tiles: N * p.nT tiles of p.T x p.T x 3 bytes
int launch_tile_gather(kocr_ctx* ctx, const uint8_t* d_canvas, int N, const TilePlan& p, uint8_t* d_tiles) {
  if (N <= 0) return KOCR_OK;
  if ((((uintptr_t)d_canvas | (uintptr_t)d_tiles) & 15) != 0) KOCR_FAIL(ctx, KOCR_EINVAL, "tile_gather: buffers must be 16-byte aligned");
  const size_t bytes = (size_t)N * p.nT * p.T * p.T * 3;
  ProfScope ps(ctx, "tile_gather", 0, 2.0 * (double)bytes);
  hipLaunchKernelGGL(tile_gather_kernel, dim3(copy_grid(ctx, bytes / 16)), dim3(COPY_BLOCK), 0, ctx->stream, (const uint4*)d_canvas,
                     (uint4*)d_tiles, p, bytes / 16);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}

// d_tile_heat: N * p.nT heat tiles of (p.T / 2)^2 x 2 floats; d_heat: N page maps of (p.Hc / 2) x (p.Wc / 2) x 2 floats
int launch_heat_stitch(kocr_ctx* ctx, const float* d_tile_heat, int N, const TilePlan& p, float* d_heat) {
  if (N <= 0) return KOCR_OK;
  if ((((uintptr_t)d_tile_heat | (uintptr_t)d_heat) & 15) != 0) KOCR_FAIL(ctx, KOCR_EINVAL, "heat_stitch: buffers must be 16-byte aligned");
  const size_t bytes = (size_t)N * (p.Hc / 2) * (p.Wc / 2) * 2 * sizeof(float);
  ProfScope ps(ctx, "heat_stitch", 0, 2.0 * (double)bytes);
  hipLaunchKernelGGL(heat_stitch_kernel, dim3(copy_grid(ctx, bytes / 16)), dim3(COPY_BLOCK), 0, ctx->stream, (const uint4*)d_tile_heat,
                     (uint4*)d_heat, p, bytes / 16);
  KOCR_HIP(ctx, hipGetLastError());
  return KOCR_OK;
}
