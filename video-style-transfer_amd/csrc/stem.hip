// The RTNSTV stem at inference (RT/network.py:71 conv1 = Conv(3, 16, 3, 1) behind RT/utilities.py:182-191
// cvframe_to_tensor): the 3x3 reflect-pad conv straight from the cv2 uint8 frame,
//   Y[co][y][x] = b[co] + sum_{ci,kh,kw} W[co][ci][kh][kw] * Xpad[ci][y + kh][x + kw],
// X = toTensor255 of the RGB byte (frame_elem.h to255: what vst_frames_to_tensor writes).  As a GEMM it
// is M = 16, K = 27 over a gathered fp32 copy of the frame that a pass of its own has just written;
// here the fp32 planes are never made.  Exact fp32 on the VALU: a lane owns 4 consecutive columns of
// one row and ALL output channels, loads the 3 rows x 6 pixels x 3 bytes of its window once (three
// dwords and the two neighbour pixels per row, in the way thin_fwd_kernel walks rows), turns them into
// floats through a 256-entry table in LDS (one IEEE division per table entry instead of one per byte)
// and runs Cout x 27 x 4 FMAs with the weights in scalar registers.
//
// Accumulation order (fixed; independent of N and of the launch geometry, so a frame in a batch is
// bitwise the frame alone): an fma chain from 0 over ci = 0..2, then kh = 0..2, then kw = 0..2, then + b.
#include "frame_elem.h"
#include "vst_common.h"
#include "vst_hip.h"

namespace {

constexpr int ST_NT = 256;

__global__ __launch_bounds__(ST_NT) void conv_stem_u8_kernel(const uint8_t* __restrict__ frames,
                                                             const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             int H, int W, int Cout, int swap) {
  __shared__ float lut[256];
  static_assert(ST_NT == 256, "one table entry per thread");
  lut[threadIdx.x] = to255(threadIdx.x);
  __syncthreads();
  const int quads = W >> 2;
  const int n = blockIdx.y;
  const int idx = blockIdx.x * ST_NT + threadIdx.x;
  if (idx >= quads * H) return;
  const int y = idx / quads, px0 = (idx - y * quads) * 4;
  const long plane = (long)H * W;
  const uint8_t* fr = frames + n * plane * 3;
  const int cl = px0 == 0 ? 1 : px0 - 1, cr = px0 + 4 >= W ? W - 2 : px0 + 4;  // reflect pad 1
  float X[3][3][6];  // [ci][kh][column px0 - 1 + j]
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    int r = y - 1 + kh;
    r = r < 0 ? 1 : (r >= H ? H - 2 : r);
    const uint8_t* row = fr + (long)r * W * 3;
    const uint32_t* body = reinterpret_cast<const uint32_t*>(row + 3 * px0);  // 12 bytes, dword aligned
    const uint32_t wd[3] = {body[0], body[1], body[2]};
    uint32_t p[6][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      p[0][c] = row[3 * cl + c];
      p[5][c] = row[3 * cr + c];
#pragma unroll
      for (int j = 0; j < 4; ++j) p[1 + j][c] = (wd[(3 * j + c) >> 2] >> (8 * ((3 * j + c) & 3))) & 255u;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const uint32_t c0 = swap ? p[j][2] : p[j][0], c2 = swap ? p[j][0] : p[j][2];  // cv2 BGR -> RGB
      X[0][kh][j] = lut[c0];
      X[1][kh][j] = lut[p[j][1]];
      X[2][kh][j] = lut[c2];
    }
  }
  float* op = out + ((long)n * Cout * H + y) * W + px0;
  for (int g = 0; g < Cout; g += 4) {
    float acc[4][4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const float* wp = w + (g + o) * 27;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[o][j] = 0.f;
#pragma unroll
      for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const float wv = wp[(ci * 3 + kh) * 3 + kw];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[o][j] = __fmaf_rn(wv, X[ci][kh][j + kw], acc[o][j]);
          }
      if (bias) {
        const float bv = bias[g + o];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[o][j] = __fadd_rn(acc[o][j], bv);
      }
      *reinterpret_cast<float4*>(op + (g + o) * plane) = make_float4(acc[o][0], acc[o][1], acc[o][2], acc[o][3]);
    }
  }
}

}  // namespace

extern "C" int vst_conv_stem_u8(const void* frames, const float* w, const float* bias, float* out, int N, int H, int W,
                                int Cout, int bgr, void* stream) {
  VST_CHECK_ARG(frames && w && out && N > 0 && N <= 65535 && H >= 2 && W >= 4 && W % 4 == 0 && Cout >= 4 &&
                Cout <= 16 && Cout % 4 == 0);
  // dword frame loads, 16-byte stores, 32-bit work index
  VST_CHECK_ARG((uintptr_t)frames % 4 == 0 && (uintptr_t)out % 16 == 0 && (long)H * W < 0x7fffffffL);
  const long items = (long)(W / 4) * H;
  conv_stem_u8_kernel<<<dim3(ceil_div(items, ST_NT), N), ST_NT, 0, (hipStream_t)stream>>>(
      (const uint8_t*)frames, w, bias, out, H, W, Cout, bgr);
  return vst_launch_status();
}
