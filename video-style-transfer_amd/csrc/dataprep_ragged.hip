// On-device item preparation of the AdaAttN image datasets (AA/datasets.py:16-44, 173-185;
// AA/utilities.py:31-43): `toTensorCrop` = Resize(size_resize) -> RandomCrop(size_crop) -> toTensor255
// for a whole batch of images of DIFFERENT source sizes, in one launch, computing the crop window only.
//
// COCO / WikiArt images come in hundreds of sizes, so the batch is ragged: every item has its own
// source raster, its own resize target and its own crop origin; only the crop size is shared.  The
// caller packs one block (descriptors, coefficient tables, rasters; layout: include/vst_hip.h), copies
// it to the device once and launches once.  A raster holds only the source rows its crop reads.
//
// Exactness: Pillow's `resize(.., BILINEAR)` on 8-bit images is a horizontal pass (uint8 result) then
// a vertical pass, 22-bit fixed-point taps (dataprep.hip has the full description and the host routine
// vst_pil_bilinear_coeffs that builds the tables).  Output pixel (y, x) of the crop is the vertical
// filter of resized row y0 + y applied to horizontal-pass values of column x0 + x only, so restricting
// both passes to the window is exact: the caller slices the full tables to rows y0..y0+Hc and columns
// x0..x0+Wc, and the kernel sees a resize whose output is the Hc x Wc window.
//
// Tiled path: a workgroup owns a 64 x 8 output tile.  Its source window is streamed through LDS in
// chunks of whole rows (aligned dword loads; each row keeps its own byte lead), the horizontal pass
// turns every chunk into uint8 rows that stay in LDS for the whole tile (planar, one byte per
// column), and the vertical pass reads those.  Every source byte is fetched once per tile at any
// downscale up to the bounds below (about 20x horizontally, 15x vertically); tiles beyond them take
// the per-pixel path, block-uniformly.
#include "vst_common.h"
#include "vst_hip.h"

namespace {

constexpr int PT = 256;
constexpr int PIL_PRECISION_BITS = 32 - 8 - 2;  // Pillow Resample.c, 8 bits per channel
constexpr int HALF = 1 << (PIL_PRECISION_BITS - 1);
constexpr int C = 3;

constexpr int TX = 64, TY = 8;
constexpr int SRC_BYTES = 16384;   // one chunk of window rows
constexpr int SRC_ROW_MAX = 4096;  // a window row (dword padded): at least 4 rows per chunk
constexpr int H_ROWS = 128;        // horizontal-pass rows kept for one tile
constexpr int KX_MAX = 48;         // horizontal taps per column staged in LDS
static_assert(PT % TX == 0 && TX == 64, "one wave per row of the tile");

// Descriptor of one item: VST_RAGGED_DESC_INTS int32 at the start of the block (include/vst_hip.h).
enum { D_RASTER = 0, D_HS, D_WS, D_X0, D_Y0, D_HB, D_HK, D_HKS, D_VB, D_VK, D_VKS, D_HR, D_WR, D_ROW0, D_ROWS };

__device__ __forceinline__ int clip8(int v) {
  v >>= PIL_PRECISION_BITS;  // arithmetic shift, then Pillow's clip8 lookup (clamp to 0..255)
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ float tensor255(int acc) { return ((float)clip8(acc) / 255.0f) * 255.0f; }

__global__ __launch_bounds__(PT) void pil_resize_crop_ragged_kernel(const uint8_t* __restrict__ block,
                                                                    float* __restrict__ out, long item_stride, int Hc,
                                                                    int Wc, int tiles_x, int tiles_y) {
  __shared__ __attribute__((aligned(16))) uint8_t s_src[SRC_BYTES];
  __shared__ __attribute__((aligned(16))) uint8_t s_h[C * H_ROWS * TX];
  __shared__ int s_kx[KX_MAX * TX];
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles;
  const int t = blockIdx.x - n * tiles;
  const int ty0 = (t / tiles_x) * TY, tx0 = (t % tiles_x) * TX;
  const int txv = min(TX, Wc - tx0), tyv = min(TY, Hc - ty0);
  const int* tab = reinterpret_cast<const int*>(block);
  const int* d = tab + n * VST_RAGGED_DESC_INTS;  // block-uniform
  const uint8_t* img = block + (long)d[D_RASTER] * 16;
  const int Ws = d[D_WS];
  const int row0 = d[D_ROW0];  // the raster holds source rows row0 .. row0 + rows only
  const int* hb = tab + d[D_HB];
  const int* hk = tab + d[D_HK];
  const int hks = d[D_HKS];
  const int* vb = tab + d[D_VB];
  const int* vk = tab + d[D_VK];
  const int vks = d[D_VKS];
  float* o = out + n * item_stride;
  const long HW = (long)Hc * Wc;
  // window of the tile: the bounds are monotone in the output coordinate
  const int xs0 = hb[2 * tx0], xs1 = hb[2 * (tx0 + txv - 1)] + hb[2 * (tx0 + txv - 1) + 1];
  const int ys0 = vb[2 * ty0], ys1 = vb[2 * (ty0 + tyv - 1)] + vb[2 * (ty0 + tyv - 1) + 1];
  const int rw = (xs1 - xs0) * C, rh = ys1 - ys0;
  const int stride = ((rw + 6) >> 2) << 2;  // 3 lead bytes + the dword tail
  if (stride > SRC_ROW_MAX || rh > H_ROWS || hks > KX_MAX) {  // per-pixel path: correct, not fast
    for (int i = threadIdx.x; i < txv * tyv; i += PT) {
      const int y = i / txv, x = i - y * txv;
      const int yy = ty0 + y, xx = tx0 + x;
      const int xmin = hb[2 * xx], xcnt = hb[2 * xx + 1], ymin = vb[2 * yy], ycnt = vb[2 * yy + 1];
      int acc[C];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = HALF;
      for (int j = 0; j < ycnt; ++j) {
        const uint8_t* row = img + ((long)(ymin - row0 + j) * Ws + xmin) * C;
        int h[C];
#pragma unroll
        for (int c = 0; c < C; ++c) h[c] = HALF;
        for (int i2 = 0; i2 < xcnt; ++i2) {
          const int k = hk[(long)xx * hks + i2];
#pragma unroll
          for (int c = 0; c < C; ++c) h[c] += (int)row[i2 * C + c] * k;
        }
        const int k = vk[(long)yy * vks + j];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += clip8(h[c]) * k;
      }
#pragma unroll
      for (int c = 0; c < C; ++c) o[c * HW + (long)yy * Wc + xx] = tensor255(acc[c]);
    }
    return;
  }
  const int x = threadIdx.x % TX, rg = threadIdx.x / TX;
  // this column's taps -> LDS, tap-major (lane x reads s_kx[j * TX + x]: one bank per lane)
  int xmin = 0, nx = 0;
  if (x < txv) {
    xmin = (hb[2 * (tx0 + x)] - xs0) * C;
    nx = hb[2 * (tx0 + x) + 1];
    for (int j = rg; j < nx; j += PT / TX) s_kx[j * TX + x] = hk[(long)(tx0 + x) * hks + j];
  }
  const int words = stride >> 2;
  const int yr0 = ys0 - row0;  // the window's first row inside the raster
  const int cr = SRC_BYTES / stride;  // rows per chunk (>= 4)
  for (int r0 = 0; r0 < rh; r0 += cr) {
    const int rows = min(cr, rh - r0);
    // 1. chunk of window rows -> LDS, aligned dwords; a row starts at any byte, so it keeps its own lead.
    //    The last dword of the last raster row may reach up to 3 bytes past the raster: the block pads it.
    for (int i = threadIdx.x; i < rows * words; i += PT) {
      const int r = i / words, w = i - r * words;
      const long off = ((long)(yr0 + r0 + r) * Ws + xs0) * C;
      const int lead = (int)(off & 3);
      if (w < ((lead + rw + 3) >> 2))
        reinterpret_cast<uint32_t*>(s_src)[r * words + w] = reinterpret_cast<const uint32_t*>(img + (off - lead))[w];
    }
    __syncthreads();  // also orders the s_kx writes before the first horizontal pass
    // 2. horizontal pass over the chunk: Pillow's intermediate uint8 rows, planar in LDS
    if (x < txv) {
      for (int r = rg; r < rows; r += PT / TX) {
        const int lead = (int)((((long)(yr0 + r0 + r) * Ws + xs0) * C) & 3);
        const uint8_t* row = s_src + r * stride + lead + xmin;
        int h[C];
#pragma unroll
        for (int c = 0; c < C; ++c) h[c] = HALF;
        for (int j = 0; j < nx; ++j) {
          const int k = s_kx[j * TX + x];
#pragma unroll
          for (int c = 0; c < C; ++c) h[c] += (int)row[j * C + c] * k;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) s_h[(c * H_ROWS + r0 + r) * TX + x] = (uint8_t)clip8(h[c]);
      }
    }
    __syncthreads();
  }
  // 3. vertical pass over the kept rows, coalesced planar stores
  if (x < txv) {
    for (int y = rg; y < tyv; y += PT / TX) {
      const int yy = ty0 + y;
      const int ymin = vb[2 * yy] - ys0, ny = vb[2 * yy + 1];
      const int* k = vk + (long)yy * vks;
      int acc[C];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = HALF;
      for (int j = 0; j < ny; ++j) {
        const int kj = k[j];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += (int)s_h[(c * H_ROWS + ymin + j) * TX + x] * kj;
      }
#pragma unroll
      for (int c = 0; c < C; ++c) o[c * HW + (long)yy * Wc + tx0 + x] = tensor255(acc[c]);
    }
  }
}

// {min, count} pairs of one sliced axis: inside [first, end) of the source, at most ks taps, monotone
// (the kernel takes a tile's window from its first and last entry)
bool axis_ok(const int* b, int n, int first, int end, int ks) {
  int lo = first, hi = first;
  for (int i = 0; i < n; ++i) {
    const int mn = b[2 * i], cnt = b[2 * i + 1];
    if (mn < lo || cnt < 1 || cnt > ks || cnt > end - first || mn > end - cnt || mn + cnt < hi) return false;
    lo = mn;
    hi = mn + cnt;
  }
  return true;
}

// [first, first + count) int32 of the block, behind the descriptors
bool ints_ok(long first, long count, long desc_ints, long block_ints) {
  return first >= desc_ints && count >= 0 && first <= block_ints && count <= block_ints - first;
}

}  // namespace

extern "C" {

int vst_pil_ragged_check(const void* block_host, long block_bytes, int N, int Hc, int Wc) {
  VST_CHECK_ARG(block_host && N >= 0 && Hc > 0 && Wc > 0 && block_bytes >= 0);
  VST_CHECK_ARG(((uintptr_t)block_host & 3) == 0);
  const long desc_ints = (long)N * VST_RAGGED_DESC_INTS, block_ints = block_bytes / 4;
  VST_CHECK_ARG(desc_ints <= block_ints);
  const int* tab = (const int*)block_host;
  for (int n = 0; n < N; ++n) {
    const int* d = tab + (long)n * VST_RAGGED_DESC_INTS;
    const long Hs = d[D_HS], Ws = d[D_WS], hks = d[D_HKS], vks = d[D_VKS];
    VST_CHECK_ARG(Hs > 0 && Ws > 0 && hks > 0 && vks > 0);
    VST_CHECK_ARG(d[D_X0] >= 0 && d[D_Y0] >= 0 && d[D_X0] <= d[D_WR] - Wc && d[D_Y0] <= d[D_HR] - Hc);
    // the raster, with the dword tail the kernel may read, lies inside the block behind the descriptors
    const long row0 = d[D_ROW0], rows = d[D_ROWS];
    VST_CHECK_ARG(row0 >= 0 && rows > 0 && rows <= Hs - row0);
    const long r0 = (long)d[D_RASTER] * 16, rbytes = (rows * Ws * C + 3) & ~3L;
    VST_CHECK_ARG(d[D_RASTER] >= 0 && r0 >= desc_ints * 4 && r0 <= block_bytes && rbytes <= block_bytes - r0);
    VST_CHECK_ARG(ints_ok(d[D_HB], 2L * Wc, desc_ints, block_ints) && ints_ok(d[D_HK], Wc * hks, desc_ints, block_ints));
    VST_CHECK_ARG(ints_ok(d[D_VB], 2L * Hc, desc_ints, block_ints) && ints_ok(d[D_VK], Hc * vks, desc_ints, block_ints));
    VST_CHECK_ARG(axis_ok(tab + d[D_HB], Wc, 0, (int)Ws, (int)hks) &&
                  axis_ok(tab + d[D_VB], Hc, (int)row0, (int)(row0 + rows), (int)vks));
  }
  return VST_OK;
}

int vst_pil_resize_crop_ragged(const void* block_dev, const void* block_host, long block_bytes, int N, int Hc, int Wc,
                               float* out, long item_stride, void* stream) {
  VST_CHECK_ARG(block_dev && out && ((uintptr_t)block_dev & 15) == 0);
  const int rc = vst_pil_ragged_check(block_host, block_bytes, N, Hc, Wc);
  if (rc != VST_OK) return rc;
  VST_CHECK_ARG(item_stride >= (long)C * Hc * Wc);
  if (N == 0) return VST_OK;
  const int tiles_x = (Wc + TX - 1) / TX, tiles_y = (Hc + TY - 1) / TY;
  const long blocks = (long)N * tiles_x * tiles_y;
  VST_CHECK_ARG(blocks < (1L << 31));
  pil_resize_crop_ragged_kernel<<<(unsigned)blocks, PT, 0, (hipStream_t)stream>>>((const uint8_t*)block_dev, out,
                                                                                 item_stride, Hc, Wc, tiles_x, tiles_y);
  return vst_launch_status();
}

int vst_pil_ragged_tile_paths(const void* block_host, long block_bytes, int N, int Hc, int Wc, int* tiled, int* fallback) {
  VST_CHECK_ARG(tiled && fallback);
  const int rc = vst_pil_ragged_check(block_host, block_bytes, N, Hc, Wc);
  if (rc != VST_OK) return rc;
  const int* tab = (const int*)block_host;
  for (int n = 0; n < N; ++n) {
    const int* d = tab + (long)n * VST_RAGGED_DESC_INTS;
    const int* hb = tab + d[D_HB];
    const int* vb = tab + d[D_VB];
    tiled[n] = fallback[n] = 0;
    for (int ty0 = 0; ty0 < Hc; ty0 += TY)
      for (int tx0 = 0; tx0 < Wc; tx0 += TX) {
        const int x1 = (tx0 + TX < Wc ? tx0 + TX : Wc) - 1, y1 = (ty0 + TY < Hc ? ty0 + TY : Hc) - 1;
        const int rw = (hb[2 * x1] + hb[2 * x1 + 1] - hb[2 * tx0]) * C, rh = vb[2 * y1] + vb[2 * y1 + 1] - vb[2 * ty0];
        const int stride = ((rw + 6) >> 2) << 2;
        ++((stride > SRC_ROW_MAX || rh > H_ROWS || d[D_HKS] > KX_MAX) ? fallback : tiled)[n];
      }
  }
  return VST_OK;
}

}  // extern "C"
