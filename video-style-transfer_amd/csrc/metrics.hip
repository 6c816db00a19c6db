// Evaluation metrics on the device (the reference evaluates on whatever `device` it is given):
//   * vst_temporal_error: the masked warping error of a batch of frame pairs in one pass --
//     RT/utilities.py:231-236 (mask * MSELoss(none)(styled0, warp(styled1, flow)), then the mean) and
//     AA/exps_sintel.py:79-100 (clamp(0,255)/255 of both frames, mask * L1Loss(none)(cs2, warp(cs1, flow)),
//     then the sum / (C H W)).  The warped frame is never written: each pixel gathers its four taps
//     (warp_coords, vst_common.h: the arithmetic of vst_warp_fwd), forms the difference and goes
//     straight into a two-stage fp64 sum in a fixed order, which a one-block second stage adds to a
//     device accumulator (a scene accumulates without a host sync per pair);
//   * vst_ssim: SSIMMetric.forward (AA/eval.py:191-223) -- five depthwise Gaussian windows over
//     zero-padded planes, the SSIM map, mean over the plane then over the channels -- as one tile
//     kernel: tile + halo of both images staged in LDS once, separable horizontal then vertical pass
//     of the five moments, the map in registers, fp64 partial per tile; vst_ssim_c is the same with
//     C1 and C2 as arguments (a data range other than 1; the gradient is csrc/ssim_grad.hip);
//   * vst_hist_u8: np.bincount(channel, minlength=256) per image and channel (compute_histogram,
//     AA/eval.py:38-46, the input of kl_loss) with integer LDS atomics per block.
#include "vst_common.h"
#include "vst_hip.h"

namespace {

constexpr int MT = 256;     // threads per block of every kernel here
constexpr int TE_MAXB = 2048;  // blocks of the per-pixel (grid-stride) temporal-error kernel

// sum over the block's 256 threads in a fixed order (lanes by xor-shuffle, then waves 0..3);
// the result is valid in thread 0
__device__ __forceinline__ double block_sum_d(double v, int tid) {
  __shared__ double sh[MT / 64];
  v = wave_sum_d(v);
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (tid == 0)
    for (int w = 0; w < MT / 64; ++w) t += sh[w];
  return t;
}

// ---- temporal error --------------------------------------------------------------------------
// clamp(0, 255) / 255 with a true division (AA/exps_sintel.py:79-83); NaN stays NaN like torch.clamp
__device__ __forceinline__ float unit255(float v) {
  v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
  return v / 255.0f;
}

struct Taps {
  int off[4];   // nw, ne, sw, se offsets inside a plane (0 where the corner is outside the frame)
  float w[4];   // the corner's weight, zeroed outside the frame (ATen's zeros padding)
  bool ok[4];
};

__device__ __forceinline__ Taps te_taps(int x, int y, float u, float v, int H, int W) {
  const Bilin bl = warp_coords(x, y, u, v, H, W);
  Taps t;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // (unsigned adds: a target far outside saturates x0 / y0 at INT_MAX, and the +1 must wrap, not overflow)
    const int cx = (int)((unsigned)bl.x0 + (unsigned)(k & 1)), cy = (int)((unsigned)bl.y0 + (unsigned)(k >> 1));
    t.ok[k] = cx >= 0 && cx < W && cy >= 0 && cy < H;
    t.off[k] = t.ok[k] ? cy * W + cx : 0;
    t.w[k] = t.ok[k] ? bl.w[k] : 0.f;
  }
  return t;
}

// mask * |a - warp(b)|^power of one element; av = a's value, bc = b's plane
template <bool CLAMP>
__device__ __forceinline__ float te_term(float av, const float* __restrict__ bc, const Taps& t, int power, float m) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // ATen sums nw, ne, sw, se in this order
    float bv = bc[t.off[k]];
    bv = t.ok[k] ? bv : 0.f;
    if (CLAMP) bv = unit255(bv);
    s += bv * t.w[k];
  }
  if (CLAMP) av = unit255(av);
  const float d = av - s;
  return m * (power == 2 ? d * d : fabsf(d));
}

// one thread per pixel (grid-stride), all channels: any W, any alignment
template <bool CLAMP>
__global__ __launch_bounds__(MT) void te_pixel_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      const float* __restrict__ flo, const float* __restrict__ mask,
                                                      int B, int C, int H, int W, int power, int hwc,
                                                      double* __restrict__ partial) {
  const long HW = (long)H * W, total = (long)B * HW;
  double acc = 0.0;
  for (long idx = (long)blockIdx.x * MT + threadIdx.x; idx < total; idx += (long)gridDim.x * MT) {
    const int bi = (int)(idx / HW);
    const long p = idx - bi * HW;
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    float u, v;
    if (hwc) {
      u = flo[2 * idx];
      v = flo[2 * idx + 1];
    } else {
      const float* f = flo + (long)bi * 2 * HW;
      u = f[p];
      v = f[HW + p];
    }
    const float m = mask ? mask[idx] : 1.f;
    const Taps t = te_taps(x, y, u, v, H, W);
    const float* ab = a + (long)bi * C * HW + p;
    const float* bb = b + (long)bi * C * HW;
    for (int c = 0; c < C; ++c) acc += (double)te_term<CLAMP>(ab[c * HW], bb + c * HW, t, power, m);
  }
  acc = block_sum_d(acc, threadIdx.x);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// four pixels of one row per thread (W % 4 == 0, 16-byte aligned a / flo / mask): the image on
// blockIdx.z, the row on blockIdx.y * 4 + threadIdx.y, no index division; dwordx4 loads of a, the
// flow (two planes, or the eight interleaved values of a .flo payload) and the mask; b is gathered
template <bool CLAMP>
__global__ __launch_bounds__(MT) void te_quad_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     const float* __restrict__ flo, const float* __restrict__ mask,
                                                     int C, int H, int W, int power, int hwc,
                                                     double* __restrict__ partial) {
  const int j = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, bi = blockIdx.z;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  const long HW = (long)H * W;
  double acc = 0.0;
  if (j < (W >> 2) && y < H) {
    const long p = (long)y * W + 4 * j;
    float u[4], v[4];
    if (hwc) {
      const float4* f = reinterpret_cast<const float4*>(flo + 2 * ((long)bi * HW + p));
      const float4 f0 = f[0], f1 = f[1];
      u[0] = f0.x, v[0] = f0.y, u[1] = f0.z, v[1] = f0.w;
      u[2] = f1.x, v[2] = f1.y, u[3] = f1.z, v[3] = f1.w;
    } else {
      const float* f = flo + (long)bi * 2 * HW + p;
      const float4 f0 = *reinterpret_cast<const float4*>(f), f1 = *reinterpret_cast<const float4*>(f + HW);
      u[0] = f0.x, u[1] = f0.y, u[2] = f0.z, u[3] = f0.w;
      v[0] = f1.x, v[1] = f1.y, v[2] = f1.z, v[3] = f1.w;
    }
    float m[4] = {1.f, 1.f, 1.f, 1.f};
    if (mask) {
      const float4 m4 = *reinterpret_cast<const float4*>(mask + (long)bi * HW + p);
      m[0] = m4.x, m[1] = m4.y, m[2] = m4.z, m[3] = m4.w;
    }
    Taps t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = te_taps(4 * j + q, y, u[q], v[q], H, W);
    const float* ab = a + (long)bi * C * HW + p;
    const float* bb = b + (long)bi * C * HW;
    for (int c = 0; c < C; ++c) {
      const float4 a4 = *reinterpret_cast<const float4*>(ab + c * HW);
      const float av[4] = {a4.x, a4.y, a4.z, a4.w};
      const float* bc = bb + c * HW;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc += (double)te_term<CLAMP>(av[q], bc, t[q], power, m[q]);
    }
  }
  acc = block_sum_d(acc, tid);
  if (tid == 0) partial[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = acc;
}

// acc[0] += (sum of the partials, in index order per thread, then the block's fixed order) * scale;
// acc[1] += pairs
__global__ __launch_bounds__(MT) void te_finish_kernel(const double* __restrict__ partial, long nb, double scale,
                                                       double pairs, double* __restrict__ acc) {
  double s = 0.0;
  for (long i = threadIdx.x; i < nb; i += MT) s += partial[i];
  s = block_sum_d(s, threadIdx.x);
  if (threadIdx.x == 0) {
    acc[0] += s * scale;
    acc[1] += pairs;
  }
}

inline int te_pixel_blocks(long total) {
  const long b = (total + MT - 1) / MT;
  return (int)(b < 1 ? 1 : (b > TE_MAXB ? TE_MAXB : b));
}
inline dim3 te_quad_grid(int B, int H, int W) {
  return dim3((unsigned)ceil_div((long)(W >> 2), 64), (unsigned)ceil_div((long)H, 4), (unsigned)B);
}
inline bool te_quad_ok(int B, int H, int W, const void* a, const void* flo, const void* mask) {
  const uintptr_t m16 = (uintptr_t)a | (uintptr_t)flo | (uintptr_t)mask;
  return (W & 3) == 0 && (m16 & 15) == 0 && B <= 65535 && (H + 3) / 4 <= 65535;
}

// ---- SSIM ------------------------------------------------------------------------------------
constexpr int SSIM_MAXWIN = 11;
struct SsimTaps {
  float g[SSIM_MAXWIN];
};

// the map of one pixel from its five windowed moments, in the reference's own operation order
// (AA/eval.py:203-214), every product and sum rounded on its own (no contraction)
__device__ __forceinline__ float ssim_pixel(float mu1, float mu2, float e11, float e22, float e12, float C1, float C2) {
#pragma clang fp contract(off)
  const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
  const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu1_mu2;
  const float num = (2.f * mu1_mu2 + C1) * (2.f * s12 + C2);
  const float den = (mu1_sq + mu2_sq + C1) * (s1 + s2 + C2);
  return num / den;
}

// One block = one TW x TH output tile of one plane (TW * TH = 1024: four rows per thread in the
// vertical pass).  LDS: the tile + halo of both images (pitch TW + 2R; every pass reads rows with
// consecutive lanes on consecutive columns, and TW is a multiple of 32, so a 32-lane group of a
// ds_read_b32 never meets one bank twice), then the five horizontally filtered planes of TH + 2R rows.
template <int TW, int TH, int R>
__global__ __launch_bounds__(MT) void ssim_tile_kernel(const float* __restrict__ img1, const float* __restrict__ img2,
                                                       SsimTaps tp, int H, int W, float c1, float c2,
                                                       float* __restrict__ map, double* __restrict__ partial) {
  constexpr int WIN = 2 * R + 1, SW = TW + 2 * R, SH = TH + 2 * R, RPT = 4;
  static_assert(TW % 32 == 0 && TW * TH == MT * RPT, "tile shape");
  __shared__ float sx[SH * SW], sy[SH * SW];
  __shared__ float hb[5][SH * TW];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const long plane = (long)blockIdx.z * H * W;
  const float* px = img1 + plane;
  const float* py = img2 + plane;

  // 1. the tile and its halo, the zero border of conv2d(padding = win / 2) folded into the gather
  for (int i = tid; i < SH * SW; i += MT) {
    const int r = i / SW, c = i - r * SW;
    const int gy = y0 - R + r, gx = x0 - R + c;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const long o = (long)gy * W + gx;
    sx[i] = in ? px[o] : 0.f;
    sy[i] = in ? py[o] : 0.f;
  }
  __syncthreads();

  // 2. horizontal pass of mu1, mu2, E[x^2], E[y^2], E[xy] over all TH + 2R rows
  for (int i = tid; i < SH * TW; i += MT) {
    const int r = i / TW, c = i - r * TW;
    const float* rx = sx + r * SW + c;
    const float* ry = sy + r * SW + c;
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < WIN; ++k) {
      const float g = tp.g[k], xv = rx[k], yv = ry[k];
      m1 = fmaf(g, xv, m1);
      m2 = fmaf(g, yv, m2);
      e11 = fmaf(g, xv * xv, e11);
      e22 = fmaf(g, yv * yv, e22);
      e12 = fmaf(g, xv * yv, e12);
    }
    hb[0][i] = m1, hb[1][i] = m2, hb[2][i] = e11, hb[3][i] = e22, hb[4][i] = e12;
  }
  __syncthreads();

  // 3. vertical pass: a thread owns column c, rows r0 .. r0 + 3, and reads each of the WIN + 3 rows
  //    it needs once per moment
  const int c = tid % TW, r0 = (tid / TW) * RPT;
  float mom[5][RPT];
#pragma unroll
  for (int m = 0; m < 5; ++m) {
    float v[WIN + RPT - 1];
#pragma unroll
    for (int j = 0; j < WIN + RPT - 1; ++j) v[j] = hb[m][(r0 + j) * TW + c];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < WIN; ++k) s = fmaf(tp.g[k], v[q + k], s);
      mom[m][q] = s;
    }
  }

  // 4. the map in registers, 5. the tile's sum in fp64 (rows in order per thread, then the block)
  double acc = 0.0;
  const int gx = x0 + c;
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int gy = y0 + r0 + q;
    if (gx < W && gy < H) {
      const float s = ssim_pixel(mom[0][q], mom[1][q], mom[2][q], mom[3][q], mom[4][q], c1, c2);
      if (map) map[plane + (long)gy * W + gx] = s;
      acc += (double)s;
    }
  }
  acc = block_sum_d(acc, tid);
  if (tid == 0) partial[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = acc;
}

// out[b] = mean over channels of (mean over the plane): one block per image, the tile partials of
// each plane in index order per thread, then the block's fixed order
__global__ __launch_bounds__(MT) void ssim_finish_kernel(const double* __restrict__ partial, int ntiles, int C,
                                                         double inv_hw, float* __restrict__ out) {
  double img = 0.0;
  for (int c = 0; c < C; ++c) {
    const double* p = partial + ((long)blockIdx.x * C + c) * ntiles;
    double s = 0.0;
    for (int i = threadIdx.x; i < ntiles; i += MT) s += p[i];
    s = block_sum_d(s, threadIdx.x);
    img += s * inv_hw;  // (thread 0 holds the sum)
    __syncthreads();    // block_sum_d's LDS slots are reused by the next channel
  }
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(img / (double)C);
}

template <int TW, int TH>
int ssim_launch(const float* img1, const float* img2, const SsimTaps& tp, int win, int B, int C, int H, int W,
                float c1, float c2, float* out, float* map, double* ws, hipStream_t st) {
  const dim3 g((unsigned)ceil_div(W, TW), (unsigned)ceil_div(H, TH), (unsigned)(B * C));
  switch (win) {
    case 1: ssim_tile_kernel<TW, TH, 0><<<g, MT, 0, st>>>(img1, img2, tp, H, W, c1, c2, map, ws); break;
    case 3: ssim_tile_kernel<TW, TH, 1><<<g, MT, 0, st>>>(img1, img2, tp, H, W, c1, c2, map, ws); break;
    case 5: ssim_tile_kernel<TW, TH, 2><<<g, MT, 0, st>>>(img1, img2, tp, H, W, c1, c2, map, ws); break;
    case 7: ssim_tile_kernel<TW, TH, 3><<<g, MT, 0, st>>>(img1, img2, tp, H, W, c1, c2, map, ws); break;
    case 9: ssim_tile_kernel<TW, TH, 4><<<g, MT, 0, st>>>(img1, img2, tp, H, W, c1, c2, map, ws); break;
    default: ssim_tile_kernel<TW, TH, 5><<<g, MT, 0, st>>>(img1, img2, tp, H, W, c1, c2, map, ws); break;
  }
  ssim_finish_kernel<<<B, MT, 0, st>>>(ws, (int)(g.x * g.y), C, 1.0 / ((double)H * W), out);
  return vst_launch_status();
}

inline long ssim_tiles(int H, int W, int tw, int th) { return (long)ceil_div(W, tw) * ceil_div(H, th); }

// ---- histogram -------------------------------------------------------------------------------
constexpr int HIST_MAXB = 256;  // blocks per image

// grid (blocks per image, N): bytes of one image grid-stride over the row of blocks; the channel of
// byte i of an interleaved image is i % C
__global__ __launch_bounds__(MT) void hist_u8_kernel(const uint8_t* __restrict__ img, int* __restrict__ hist,
                                                     long per, int C, int words_ok) {
  __shared__ int sh[3 * 256];
  for (int i = threadIdx.x; i < C * 256; i += MT) sh[i] = 0;
  __syncthreads();
  const uint8_t* p = img + (long)blockIdx.y * per;
  if (words_ok) {  // per % 4 == 0 and a 4-byte aligned base: one dword = four bytes
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
    const long nw = per >> 2;
    for (long i = (long)blockIdx.x * MT + threadIdx.x; i < nw; i += (long)gridDim.x * MT) {
      const uint32_t v = w[i];
      int ch = C == 1 ? 0 : (int)((4 * i) % 3);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        atomicAdd(&sh[ch * 256 + ((v >> (8 * k)) & 255u)], 1);
        if (C != 1) ch = ch == 2 ? 0 : ch + 1;
      }
    }
  } else {
    for (long i = (long)blockIdx.x * MT + threadIdx.x; i < per; i += (long)gridDim.x * MT)
      atomicAdd(&sh[(C == 1 ? 0 : (int)(i % 3)) * 256 + p[i]], 1);
  }
  __syncthreads();
  int* out = hist + (long)blockIdx.y * C * 256;
  for (int i = threadIdx.x; i < C * 256; i += MT) {
    const int n = sh[i];
    if (n) atomicAdd(out + i, n);
  }
}

}  // namespace

extern "C" {

long vst_temporal_error_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const dim3 g = te_quad_grid(B, H, W);
  const long quad = (long)g.x * g.y * g.z, pix = te_pixel_blocks((long)B * H * W);
  return 8 * (quad > pix ? quad : pix);
}

int vst_temporal_error(const float* a, const float* b, const float* flo, const float* mask, int B, int C, int H, int W,
                       int power, int flo_hwc, int clamp_unit, double scale, void* workspace, double* acc,
                       void* stream) {
  VST_CHECK_ARG(a && b && flo && workspace && acc && B > 0 && C > 0 && H > 0 && W > 0);
  VST_CHECK_ARG((power == 1 || power == 2) && (flo_hwc == 0 || flo_hwc == 1) && (clamp_unit == 0 || clamp_unit == 1));
  VST_CHECK_ARG((long)H * W < (1L << 31) && scale == scale);
  VST_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)acc) & 7) == 0);
  hipStream_t st = (hipStream_t)stream;
  double* partial = static_cast<double*>(workspace);
  long nb;
  if (te_quad_ok(B, H, W, a, flo, mask)) {
    const dim3 g = te_quad_grid(B, H, W);
    nb = (long)g.x * g.y * g.z;
    if (clamp_unit)
      te_quad_kernel<true><<<g, dim3(64, 4), 0, st>>>(a, b, flo, mask, C, H, W, power, flo_hwc, partial);
    else
      te_quad_kernel<false><<<g, dim3(64, 4), 0, st>>>(a, b, flo, mask, C, H, W, power, flo_hwc, partial);
  } else {
    nb = te_pixel_blocks((long)B * H * W);
    if (clamp_unit)
      te_pixel_kernel<true><<<(unsigned)nb, MT, 0, st>>>(a, b, flo, mask, B, C, H, W, power, flo_hwc, partial);
    else
      te_pixel_kernel<false><<<(unsigned)nb, MT, 0, st>>>(a, b, flo, mask, B, C, H, W, power, flo_hwc, partial);
  }
  te_finish_kernel<<<1, MT, 0, st>>>(partial, nb, scale, (double)B, acc);
  return vst_launch_status();
}

long vst_ssim_workspace(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  const long t0 = ssim_tiles(H, W, 32, 32), t1 = ssim_tiles(H, W, 64, 16);
  return 8 * (long)B * C * (t0 > t1 ? t0 : t1);
}

int vst_ssim_c(const float* img1, const float* img2, const float* taps, int win, int B, int C, int H, int W, float c1,
               float c2, float* out, float* map, void* workspace, int tile, void* stream) {
  VST_CHECK_ARG(img1 && img2 && taps && out && workspace && B > 0 && C > 0 && H > 0 && W > 0);
  VST_CHECK_ARG(win >= 1 && win <= SSIM_MAXWIN && (win & 1) == 1 && tile >= 0 && tile <= 2);
  VST_CHECK_ARG((long)B * C <= 65535 && (H + 15) / 16 <= 65535 && (long)H * W < (1L << 31));
  VST_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && c1 == c1 && c2 == c2);
  SsimTaps tp;
  for (int k = 0; k < SSIM_MAXWIN; ++k) tp.g[k] = k < win ? taps[k] : 0.f;
  hipStream_t st = (hipStream_t)stream;
  double* ws = static_cast<double*>(workspace);
  // tile 0: the shape tools/eval_bench.py measured faster at 436 x 1024
  if (tile == 2) return ssim_launch<64, 16>(img1, img2, tp, win, B, C, H, W, c1, c2, out, map, ws, st);
  return ssim_launch<32, 32>(img1, img2, tp, win, B, C, H, W, c1, c2, out, map, ws, st);
}

int vst_ssim(const float* img1, const float* img2, const float* taps, int win, int B, int C, int H, int W, float* out,
             float* map, void* workspace, int tile, void* stream) {
  // the reference's Python doubles (AA/eval.py:176-177), to fp32
  return vst_ssim_c(img1, img2, taps, win, B, C, H, W, (float)(0.01 * 0.01), (float)(0.03 * 0.03), out, map, workspace,
                    tile, stream);
}

int vst_hist_u8(const void* images, void* hist, int N, int H, int W, int C, void* stream) {
  VST_CHECK_ARG(images && hist && N > 0 && N <= 65535 && H > 0 && W > 0 && (C == 1 || C == 3));
  VST_CHECK_ARG(((uintptr_t)hist & 3) == 0 && (long)H * W * C < (1L << 31));
  hipStream_t st = (hipStream_t)stream;
  const long per = (long)H * W * C;
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)N * C * 256 * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  const int words_ok = per % 4 == 0 && ((uintptr_t)images & 3) == 0;
  long nb = (per + MT * 64 - 1) / (MT * 64);  // about 64 bytes per thread
  nb = nb < 1 ? 1 : (nb > HIST_MAXB ? HIST_MAXB : nb);
  hist_u8_kernel<<<dim3((unsigned)nb, (unsigned)N), MT, 0, st>>>(static_cast<const uint8_t*>(images),
                                                                static_cast<int*>(hist), per, C, words_ok);
  return vst_launch_status();
}

}  // extern "C"
