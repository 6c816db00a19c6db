// The gradient of vst_ssim_c's per-image scores with respect to both images (vst.metrics.ssim_scores,
// SSIMLoss), and the loss form of the scores.
//
// Per plane, with G the zero-padded separable window and mu1 = G*x, mu2 = G*y, e11 = G*x^2, e22 = G*y^2,
// e12 = G*xy:
//   A1 = 2 mu1 mu2 + C1,  A2 = 2 (e12 - mu1 mu2) + C2,  B1 = mu1^2 + mu2^2 + C1,
//   B2 = (e11 - mu1^2) + (e22 - mu2^2) + C2,  S = A1 A2 / (B1 B2)
//   Dm  = dS/dmu1 = 2 mu2 (A2 - A1) / (B1 B2) - 2 mu1 S (1/B1 - 1/B2)      (Dm': mu1 <-> mu2)
//   D11 = dS/de11 = -S / B2  (= dS/de22: S sees e11 and e22 only through their sum in B2)
//   D12 = dS/de12 = 2 A1 / (B1 B2)
//   dL/dx = w (G*Dm + 2 x (G*D11) + y (G*D12)),   dL/dy = w (G*Dm' + 2 y (G*D11) + x (G*D12)),
// w = gout[b] / (C H W), the D maps taken as zero outside the image (the adjoint of the zero padding).
// One block recomputes the moments of its tile + R halo from the tile + 2R halo of both images (nothing
// is saved by the forward), forms the D maps there, runs the second separable pass and writes each
// gradient element once: no atomics, no workspace, no dependence on the rest of the batch.
#include "vst_common.h"
#include "vst_hip.h"

namespace {

constexpr int MT = 256;
constexpr int SSIM_MAXWIN = 11;
struct SsimTaps {
  float g[SSIM_MAXWIN];
};

// One block = one 32 x 32 tile of one plane.  LDS: sx, sy = the tile + 2R halo (kept to the end: the
// last step multiplies by x and y), and one buffer that holds in turn
//   hb: the five horizontally filtered moments, TH + 4R rows of TW + 2R columns,
//   dm: the 3 (4 with the y gradient) D maps on (TH + 2R) x (TW + 2R),
//   hd: their horizontal pass, TH + 2R rows of TW columns;
// dm and hd are formed in registers, and written after a barrier behind the last read of what they
// replace.  R = 5: 2 * 52 * 52 + 5 * 52 * 42 floats = 65312 bytes, two blocks per CU.
template <int R, bool Y2>
__global__ __launch_bounds__(MT) void ssim_bwd_tile_kernel(const float* __restrict__ img1,
                                                           const float* __restrict__ img2, SsimTaps tp, int C, int H,
                                                           int W, float c1, float c2, float inv_chw,
                                                           const float* __restrict__ gout, float* __restrict__ d1,
                                                           float* __restrict__ d2) {
  // every product and sum below rounds as written (the fmaf calls stay fused): d1's bits then do not
  // depend on what else the instantiation computes
#pragma clang fp contract(off)
  constexpr int TW = 32, TH = 32, WIN = 2 * R + 1;
  constexpr int SW = TW + 4 * R, SH = TH + 4 * R;  // staged images
  constexpr int MW = TW + 2 * R, MH = TH + 2 * R;  // moments and D maps
  constexpr int NMAP = Y2 ? 4 : 3;                 // Dm, D11, D12 (, Dm')
  constexpr int NG = MT / MW, VR = (MH + NG - 1) / NG;  // moment pass: NG row groups of VR rows per column
  constexpr int HI = (MH * TW + MT - 1) / MT;           // D horizontal pass: elements per thread
  constexpr int RPT = TW * TH / MT;                      // last pass: rows per thread
  static_assert(NG * VR >= MH && NMAP * MH * MW <= 5 * SH * MW && NMAP * MH * TW <= 5 * SH * MW, "layout");
  __shared__ float sx[SH * SW], sy[SH * SW];
  __shared__ float buf[5 * SH * MW];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const long plane = (long)blockIdx.z * H * W;
  const float* px = img1 + plane;
  const float* py = img2 + plane;

  // 1. the tile and its 2R halo, zero outside the image
  for (int i = tid; i < SH * SW; i += MT) {
    const int r = i / SW, c = i - r * SW;
    const int gy = y0 - 2 * R + r, gx = x0 - 2 * R + c;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const long o = (long)gy * W + gx;
    sx[i] = in ? px[o] : 0.f;
    sy[i] = in ? py[o] : 0.f;
  }
  __syncthreads();

  // 2. horizontal pass of the five moments: SH rows, MW columns
  for (int i = tid; i < SH * MW; i += MT) {
    const int r = i / MW, c = i - r * MW;
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
    buf[0 * SH * MW + i] = m1, buf[1 * SH * MW + i] = m2, buf[2 * SH * MW + i] = e11;
    buf[3 * SH * MW + i] = e22, buf[4 * SH * MW + i] = e12;
  }
  __syncthreads();

  // 3. vertical pass: a thread owns column mc, rows mr0 .. mr0 + VR - 1 of the moment region, then the
  //    D maps of those pixels in registers
  const int mc = tid % MW, mr0 = (tid / MW) * VR;
  const bool mact = tid < NG * MW;
  float dmap[NMAP][VR];
  {
    float mom[5][VR];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      float v[WIN + VR - 1];
#pragma unroll
      for (int j = 0; j < WIN + VR - 1; ++j) v[j] = (mact && mr0 + j < SH) ? buf[m * SH * MW + (mr0 + j) * MW + mc] : 0.f;
#pragma unroll
      for (int q = 0; q < VR; ++q) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) s = fmaf(tp.g[k], v[q + k], s);
        mom[m][q] = s;
      }
    }
    const int gx = x0 - R + mc;
#pragma unroll
    for (int q = 0; q < VR; ++q) {
      const int gy = y0 - R + mr0 + q;
      const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
      const float mu1 = mom[0][q], mu2 = mom[1][q];
      const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
      // (the three central moments with one rounding each: the product inside the fmaf is exact)
      const float A1 = 2.f * mu1_mu2 + c1, A2 = 2.f * fmaf(-mu1, mu2, mom[4][q]) + c2;
      const float B1 = mu1_sq + mu2_sq + c1, B2 = fmaf(-mu1, mu1, mom[2][q]) + fmaf(-mu2, mu2, mom[3][q]) + c2;
      const float inv = 1.f / (B1 * B2);
      const float S = A1 * A2 * inv;
      const float da = 2.f * (A2 - A1) * inv, db = 2.f * S * (B2 - B1) * inv;  // db = 2 S (1/B1 - 1/B2)
      dmap[0][q] = in ? mu2 * da - mu1 * db : 0.f;
      dmap[1][q] = in ? -S * B1 * inv : 0.f;
      dmap[2][q] = in ? 2.f * A1 * inv : 0.f;
      if (Y2) dmap[NMAP - 1][q] = in ? mu1 * da - mu2 * db : 0.f;
    }
  }
  __syncthreads();  // every read of hb is done: dm takes its place
  if (mact) {
#pragma unroll
    for (int q = 0; q < VR; ++q)
      if (mr0 + q < MH) {
#pragma unroll
        for (int k = 0; k < NMAP; ++k) buf[k * MH * MW + (mr0 + q) * MW + mc] = dmap[k][q];
      }
  }
  __syncthreads();

  // 4. the second separable pass, horizontal: MH rows, TW columns, in registers first
  float hreg[HI][NMAP];
#pragma unroll
  for (int it = 0; it < HI; ++it) {
    const int i = tid + it * MT;
    const int r = i / TW, c = i - r * TW;
#pragma unroll
    for (int k = 0; k < NMAP; ++k) {
      float s = 0.f;
      if (i < MH * TW) {
        const float* row = buf + k * MH * MW + r * MW + c;
#pragma unroll
        for (int t = 0; t < WIN; ++t) s = fmaf(tp.g[t], row[t], s);
      }
      hreg[it][k] = s;
    }
  }
  __syncthreads();  // every read of dm is done: hd takes its place
#pragma unroll
  for (int it = 0; it < HI; ++it) {
    const int i = tid + it * MT;
    if (i < MH * TW) {
#pragma unroll
      for (int k = 0; k < NMAP; ++k) buf[k * MH * TW + i] = hreg[it][k];
    }
  }
  __syncthreads();

  // 5. vertical, 6. combined with x and y; every element of the tile written once by its thread
  const int c = tid % TW, r0 = (tid / TW) * RPT;
  float conv[NMAP][RPT];
#pragma unroll
  for (int k = 0; k < NMAP; ++k) {
    float v[WIN + RPT - 1];
#pragma unroll
    for (int j = 0; j < WIN + RPT - 1; ++j) v[j] = buf[k * MH * TW + (r0 + j) * TW + c];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      float s = 0.f;
#pragma unroll
      for (int t = 0; t < WIN; ++t) s = fmaf(tp.g[t], v[q + t], s);
      conv[k][q] = s;
    }
  }
  const float w = gout[blockIdx.z / C] * inv_chw;
  const int gx = x0 + c;
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int gy = y0 + r0 + q;
    if (gx < W && gy < H) {
      const int si = (r0 + q + 2 * R) * SW + c + 2 * R;
      const float xv = sx[si], yv = sy[si];
      const long o = plane + (long)gy * W + gx;
      d1[o] = w * (conv[0][q] + 2.f * xv * conv[1][q] + yv * conv[2][q]);
      if (Y2) d2[o] = w * (conv[NMAP - 1][q] + 2.f * yv * conv[1][q] + xv * conv[2][q]);
    }
  }
}

template <int R>
void ssim_bwd_launch(dim3 g, hipStream_t st, const float* img1, const float* img2, const SsimTaps& tp, int C, int H,
                     int W, float c1, float c2, float inv_chw, const float* gout, float* d1, float* d2) {
  if (d2)
    ssim_bwd_tile_kernel<R, true><<<g, MT, 0, st>>>(img1, img2, tp, C, H, W, c1, c2, inv_chw, gout, d1, d2);
  else
    ssim_bwd_tile_kernel<R, false><<<g, MT, 0, st>>>(img1, img2, tp, C, H, W, c1, c2, inv_chw, gout, d1, d2);
}

// out[0] = weight * (1 - mean_b score[b]), summed in index order
__global__ void ssim_loss_kernel(const float* __restrict__ score, int B, float weight, float* __restrict__ out) {
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += score[b];
  out[0] = weight * (1.f - s / (float)B);
}

// gl[b] = -g[0] * weight / B
__global__ __launch_bounds__(256) void ssim_loss_bwd_kernel(const float* __restrict__ g, int B, float weight,
                                                            float* __restrict__ gl) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) gl[b] = -(g[0] * weight) / (float)B;
}

}  // namespace

extern "C" {

int vst_ssim_bwd(const float* img1, const float* img2, const float* taps, int win, int B, int C, int H, int W, float c1,
                 float c2, const float* gout, float* d1, float* d2, void* stream) {
  VST_CHECK_ARG(img1 && img2 && taps && gout && d1 && B > 0 && C > 0 && H > 0 && W > 0);
  VST_CHECK_ARG(win >= 1 && win <= SSIM_MAXWIN && (win & 1) == 1);
  VST_CHECK_ARG((long)B * C <= 65535 && (H + 15) / 16 <= 65535 && (long)H * W < (1L << 31));
  VST_CHECK_ARG(c1 == c1 && c2 == c2);
  SsimTaps tp;
  for (int k = 0; k < SSIM_MAXWIN; ++k) tp.g[k] = k < win ? taps[k] : 0.f;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)ceil_div(W, 32), (unsigned)ceil_div(H, 32), (unsigned)(B * C));
  const float inv_chw = (float)(1.0 / ((double)C * H * W));
  switch (win) {
    case 1: ssim_bwd_launch<0>(g, st, img1, img2, tp, C, H, W, c1, c2, inv_chw, gout, d1, d2); break;
    case 3: ssim_bwd_launch<1>(g, st, img1, img2, tp, C, H, W, c1, c2, inv_chw, gout, d1, d2); break;
    case 5: ssim_bwd_launch<2>(g, st, img1, img2, tp, C, H, W, c1, c2, inv_chw, gout, d1, d2); break;
    case 7: ssim_bwd_launch<3>(g, st, img1, img2, tp, C, H, W, c1, c2, inv_chw, gout, d1, d2); break;
    case 9: ssim_bwd_launch<4>(g, st, img1, img2, tp, C, H, W, c1, c2, inv_chw, gout, d1, d2); break;
    default: ssim_bwd_launch<5>(g, st, img1, img2, tp, C, H, W, c1, c2, inv_chw, gout, d1, d2); break;
  }
  return vst_launch_status();
}

int vst_ssim_loss(const float* score, int B, float weight, float* out, void* stream) {
  VST_CHECK_ARG(score && out && B > 0 && B <= 65535);
  ssim_loss_kernel<<<1, 1, 0, (hipStream_t)stream>>>(score, B, weight, out);
  return vst_launch_status();
}

int vst_ssim_loss_bwd(const float* g, int B, float weight, float* gl, void* stream) {
  VST_CHECK_ARG(g && gl && B > 0 && B <= 65535);
  ssim_loss_bwd_kernel<<<(B + 255) / 256, 256, 0, (hipStream_t)stream>>>(g, B, weight, gl);
  return vst_launch_status();
}

}  // extern "C"
