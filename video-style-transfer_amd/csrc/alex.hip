// The two kernels torchvision's AlexNet `features` needs beyond the VGG set (the LPIPS trunk of
// AA/lpips/pretrained_networks.py:57-95): the 11x11 stride-4 pad-2 stem and MaxPool2d(3, 2).
//
// vst_conv_cin3_k11s4:
//   Y[n][co][oy][ox] = [relu](b[co] + sum_{ci,kh,kw} W[co][ci][kh][kw] * Xpad[n][ci][4 oy + kh][4 ox + kw]),
// Xpad = X with two zero rows / columns on every side.  Exact fp32 on the VALU, as the other image-space
// stems (stem.hip, vst_conv_cin3_k3): 363 MACs per output are far from a GEMM's K.
//
// A block of 512 lanes owns an 8 x 32 tile of outputs and up to 64 output channels (grid: tiles x
// ceil(Cout / 64) x N).  Per input channel it stages the (4 * 8 + 7) x (4 * 32 + 7) fp32 source patch of the
// tile in LDS, zero outside the image, every load bounds-checked (21 KB: one channel at a time, so three
// blocks -- 24 waves -- share a CU).  The block is four groups of 128 lanes (two waves), one per 16 output
// channels, which all read that one patch: the waves of a group stall on their weights four times per
// (ci, kh), and it is the other groups' waves that fill the VALU meanwhile (one group per block, seven
// blocks per CU: 0.30 of the fp32 vector rate at 16 x 3 x 436 x 1024; two groups: 0.50; four: 0.53 --
// DESIGN.md 4.18).  A lane owns two output pixels of one column, four rows apart, and its group's 16
// channels: 32 accumulators (four pixels per lane halve the weight traffic but double the patch, and were
// slower: fewer waves per CU).  Per (ci, kh) it reads the 12 floats at patch[4 r + kh][4 c ..] of each pixel
// with three 16-byte LDS reads -- the 4-pixel lane stride is a 16-byte stride, so the 32 lanes of a tile
// row read 32 consecutive 16-byte slots: every 16-lane group of a ds_read_b128 covers 16 distinct slots, no
// bank is hit twice (rows are 136 floats: 16-byte aligned) -- and runs 16 x 11 x 2 FMAs whose weights are
// wave-uniform: W[co][ci][kh][0..10] is 11 consecutive floats, fetched through the scalar cache into SGPRs,
// each used for both pixels (the compiler pairs two channels per v_pk_fma_f32).
//
// Accumulation order (fixed; independent of N and of the launch geometry, so an image in a batch is
// bitwise the image alone): an fma chain from 0 over ci = 0..2, then kh = 0..10, then kw = 0..10, then + b.
//
// vst_maxpool3x3s2_fwd: one lane per output, the nine window values in window order with ATen's
// comparison (`v > m || isnan(v)` from -inf), so the result is torch's bit for bit, NaN and signed zero
// included.  Neighbouring windows overlap by one row and one column; the re-reads are L1 / L2 hits.
#include "vst_common.h"
#include "vst_hip.h"

namespace {

constexpr int AX_K = 11, AX_S = 4, AX_PAD = 2;
constexpr int AX_PX = 2;                             // output pixels of a lane: one column, rows AX_RS apart
constexpr int AX_RS = 4;                             // tile rows per pixel slot (= rows of lanes)
constexpr int AX_TH = AX_PX * AX_RS, AX_TW = 32;     // output tile of a block
constexpr int AX_G = 16;                             // output channels of a lane
constexpr int AX_CG = 4;                             // channel groups of a block: AX_TW * AX_RS lanes each, one patch
constexpr int AX_GL = AX_TW * AX_RS;                 // 128 lanes of a channel group
constexpr int AX_NT = AX_CG * AX_GL;
constexpr int AX_PH = AX_S * AX_TH + AX_K - AX_S;    // 39 patch rows
constexpr int AX_PW = AX_S * AX_TW + AX_K - AX_S;    // 135 patch columns
constexpr int AX_LS = 136;                           // LDS row stride in floats (16-byte rows; column 135 is read, never used)
static_assert(AX_LS >= AX_PW && AX_LS % 4 == 0 && AX_LS >= AX_S * (AX_TW - 1) + 12, "a lane reads 12 floats from 4 c");

__global__ __launch_bounds__(AX_NT) void conv_cin3_k11s4_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ out,
                                                                int H, int W, int Ho, int Wo, int Cout, int tiles_x,
                                                                int relu) {
  __shared__ __attribute__((aligned(16))) float patch[AX_PH][AX_LS];
  const int tid = threadIdx.x % AX_GL;
  // wave-uniform (AX_GL is two waves), and said so: the weight addresses below must stay scalar
  const int cg = __builtin_amdgcn_readfirstlane(threadIdx.x / AX_GL);
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int g = blockIdx.y * AX_CG + cg, n = blockIdx.z;
  const bool active = g * AX_G < Cout;  // Cout / 16 need not be a multiple of AX_CG: idle groups only stage
  const int oy0 = ty * AX_TH, ox0 = tx * AX_TW;
  const int col = tid & (AX_TW - 1), row = tid / AX_TW;  // pixels (row + AX_RS p, col) of the tile, p < AX_PX
  const int iy0 = AX_S * oy0 - AX_PAD, ix0 = AX_S * ox0 - AX_PAD;
  // the last source row / column a window reaches: what lies beyond is never read
  const int Hr = min(H, AX_S * (Ho - 1) - AX_PAD + AX_K), Wr = min(W, AX_S * (Wo - 1) - AX_PAD + AX_K);
  const long plane = (long)H * W;
  const float* xn = x + (long)n * 3 * plane;

  float acc[AX_PX][AX_G];
#pragma unroll
  for (int p = 0; p < AX_PX; ++p)
#pragma unroll
    for (int o = 0; o < AX_G; ++o) acc[p][o] = 0.f;

#pragma unroll 1
  for (int ci = 0; ci < 3; ++ci) {
    if (ci) __syncthreads();  // the previous channel's reads are done
    const float* xc = xn + ci * plane;
    for (int i = threadIdx.x; i < AX_PH * AX_LS; i += AX_NT) {
      const int pr = i / AX_LS, pc = i - pr * AX_LS;
      const int iy = iy0 + pr, ix = ix0 + pc;
      const bool in = pc < AX_PW && iy >= 0 && iy < Hr && ix >= 0 && ix < Wr;
      patch[pr][pc] = in ? xc[(long)iy * W + ix] : 0.f;
    }
    __syncthreads();
    if (!active) continue;
#pragma unroll 1
    for (int kh = 0; kh < AX_K; ++kh) {
      float xv[AX_PX][12];
#pragma unroll
      for (int p = 0; p < AX_PX; ++p) {
        const float4* src = reinterpret_cast<const float4*>(&patch[AX_S * (row + p * AX_RS) + kh][AX_S * col]);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float4 v = src[q];
          xv[p][4 * q] = v.x, xv[p][4 * q + 1] = v.y, xv[p][4 * q + 2] = v.z, xv[p][4 * q + 3] = v.w;
        }
      }
      const float* wp = w + ((long)(g * AX_G) * 3 + ci) * (AX_K * AX_K) + kh * AX_K;  // wave-uniform
#pragma unroll
      for (int o = 0; o < AX_G; ++o) {
#pragma unroll
        for (int kw = 0; kw < AX_K; ++kw) {
          const float wv = wp[o * 3 * AX_K * AX_K + kw];
#pragma unroll
          for (int p = 0; p < AX_PX; ++p) acc[p][o] = __fmaf_rn(wv, xv[p][kw], acc[p][o]);
        }
        // 44 weights in flight at a time: hoisted together, the 176 of a (ci, kh) do not fit the SGPR file
        // and come back through v_readlane spills
        if ((o & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  const int ox = ox0 + col;
  if (ox >= Wo || !active) return;
  const long oplane = (long)Ho * Wo;
  float* on = out + ((long)n * Cout + g * AX_G) * oplane;
#pragma unroll
  for (int p = 0; p < AX_PX; ++p) {
    const int oy = oy0 + row + p * AX_RS;
    if (oy >= Ho) continue;
#pragma unroll
    for (int o = 0; o < AX_G; ++o) {
      float v = acc[p][o];
      if (bias) v = __fadd_rn(v, bias[g * AX_G + o]);
      if (relu) v = fmaxf(v, 0.f);
      on[o * oplane + (long)oy * Wo + ox] = v;
    }
  }
}

__global__ __launch_bounds__(256) void maxpool3x3s2_fwd_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                               long total, int H, int W, int Ho, int Wo) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long t = idx / Wo;
  const int ox = (int)(idx - t * Wo);
  const long nc = t / Ho;
  const int oy = (int)(t - nc * Ho);
  const float* p = x + (nc * H + 2 * oy) * W + 2 * ox;
  float m = -INFINITY;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const float v = p[(long)kh * W + kw];
      if (v > m || v != v) m = v;
    }
  out[idx] = m;
}

}  // namespace

extern "C" int vst_conv_cin3_k11s4(const float* x, const float* w, const float* b, float* out, int N, int H, int W,
                                   int Cout, int relu, void* stream) {
  VST_CHECK_ARG(x && w && out && N > 0 && N <= 65535 && H >= AX_K - 2 * AX_PAD && W >= AX_K - 2 * AX_PAD);
  VST_CHECK_ARG(Cout > 0 && Cout % AX_G == 0 && Cout <= 64 && (long)H * W < 0x7fffffffL);
  VST_CHECK_ARG((uintptr_t)x % 4 == 0 && (uintptr_t)w % 4 == 0 && (uintptr_t)out % 4 == 0);
  const int Ho = (H + 2 * AX_PAD - AX_K) / AX_S + 1, Wo = (W + 2 * AX_PAD - AX_K) / AX_S + 1;
  const int tiles_x = ceil_div(Wo, AX_TW), tiles_y = ceil_div(Ho, AX_TH);
  conv_cin3_k11s4_kernel<<<dim3(tiles_x * tiles_y, ceil_div(Cout / AX_G, AX_CG), N), AX_NT, 0, (hipStream_t)stream>>>(
      x, w, b, out, H, W, Ho, Wo, Cout, tiles_x, relu);
  return vst_launch_status();
}

extern "C" int vst_maxpool3x3s2_fwd(const float* x, float* out, long NC, int H, int W, void* stream) {
  VST_CHECK_ARG(x && out && NC > 0 && H >= 3 && W >= 3);
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
  VST_CHECK_ARG(NC <= 0x7fffffffL && (long)H * W < 0x7fffffffL && NC * ((long)Ho * Wo) < 256L * 0x7fffffffL);
  const long total = NC * Ho * Wo;
  maxpool3x3s2_fwd_kernel<<<ceil_div(total, 256), 256, 0, (hipStream_t)stream>>>(x, out, total, H, W, Ho, Wo);
  return vst_launch_status();
}
