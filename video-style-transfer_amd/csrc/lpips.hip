// LPIPS (VGG) on the device:
//   * vst_lpips_head: the distance head of one trunk level -- normalize_tensor of both features
//     (AA/lpips/__init__.py:13-15), their squared difference, the 1x1 NetLinLayer conv (or the plain channel
//     sum of lpips=False) and spatial_average (AA/lpips/lpips.py:139-152) -- as one kernel: a block owns PX
//     consecutive pixels and splits the C channels over G groups (thread = (group, pixel), a wave = 64 / PX
//     groups of PX consecutive pixels, so every load instruction reads whole 4 PX-byte runs of a plane).  A
//     thread loads its C / G channels of both features ONCE into registers; the groups' sums of squares
//     meet in a fixed order (the 64 / PX groups of a wave by xor-shuffle, then the waves in order through
//     LDS), the per-pixel reciprocals go back through LDS, the weighted squared differences are formed
//     from the registers and meet the same way; the block's pixels are summed in fp64 and a finishing
//     kernel adds the blocks in index order;
//   * vst_lpips_input: im2tensor / `2 x - 1` and ScalingLayer (AA/lpips/__init__.py:86-88,
//     AA/lpips/lpips.py:130-135,164-171) into one half of the trunk's 2N batch.
#include "vst_common.h"
#include "vst_hip.h"

namespace {

constexpr int LP_CPT = 32;         // most channels a thread keeps per feature (2 * LP_CPT registers)
constexpr long LP_SMALL_P = 4096;  // planes up to this size run 32-pixel blocks
constexpr float LP_EPS = 1e-10f;   // normalize_tensor's eps, added to the fp32 norm in fp32

// the weighted squared difference of the two normalised values; no contraction: a == b and ra == rb
// must give exactly 0, which a fused a * ra - round(b * rb) would not
__device__ __forceinline__ float lp_term(float a, float ra, float b, float rb, float w) {
#pragma clang fp contract(off)
  const float x = a * ra, y = b * rb;
  const float d = x - y;
  return w * (d * d);
}

// sum over the 64 / PX channel groups a wave holds (lanes px, px + PX, ...), in a fixed order; every
// lane receives it
template <int PX>
__device__ __forceinline__ float wave_groups_sum(float v) {
#pragma unroll
  for (int o = 32; o >= PX; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// grid (ceil(P / PX), N), PX * G threads; thread t: pixel t % PX of the block, channel group t / PX,
// channels g, g + G, g + 2G, ... (C / G <= CPT of them)
template <int PX, int G, int CPT>
__global__ __launch_bounds__(PX * G) void lpips_head_kernel(const float* __restrict__ f0, long bs0,
                                                           const float* __restrict__ f1, long bs1,
                                                           const float* __restrict__ w, int C, long P,
                                                           float* __restrict__ map, double* __restrict__ partial) {
  constexpr int NW = PX * G / 64;  // waves of the block
  __shared__ float s0[NW * PX], s1[NW * PX];
  __shared__ float r0[PX], r1[PX];
  const int tid = threadIdx.x, px = tid % PX, g = tid / PX;
  const int lane = tid & 63, slot = (tid >> 6) * PX + lane;  // the wave's row in s0 / s1, for lanes < PX
  const int n = blockIdx.y, cpt = C / G;
  const long p = (long)blockIdx.x * PX + px;
  const bool in = p < P;
  const float* a = f0 + (long)n * bs0 + (long)g * P + p;
  const float* b = f1 + (long)n * bs1 + (long)g * P + p;
  const long cstep = (long)G * P;

  // 1. the thread's channels of both features, once; sums of squares
  float av[CPT], bv[CPT];
  float sa = 0.f, sb = 0.f;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const bool ok = in && i < cpt;
    av[i] = ok ? a[i * cstep] : 0.f;
    bv[i] = ok ? b[i * cstep] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    sa = fmaf(av[i], av[i], sa);
    sb = fmaf(bv[i], bv[i], sb);
  }
  sa = wave_groups_sum<PX>(sa);
  sb = wave_groups_sum<PX>(sb);
  if (lane < PX) {
    s0[slot] = sa;
    s1[slot] = sb;
  }
  __syncthreads();

  // 2. per pixel: the waves in order, 1 / (norm + eps)
  if (tid < PX) {
    float ta = 0.f, tb = 0.f;
#pragma unroll 8
    for (int k = 0; k < NW; ++k) {
      ta += s0[k * PX + tid];
      tb += s1[k * PX + tid];
    }
    r0[tid] = 1.0f / (sqrtf(ta) + LP_EPS);
    r1[tid] = 1.0f / (sqrtf(tb) + LP_EPS);
  }
  __syncthreads();

  // 3. the weighted squared differences of the thread's channels, from registers
  const float ra = r0[px], rb = r1[px];
  float d = 0.f;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    if (i < cpt) {
      const float wc = w ? w[g + i * G] : 1.f;
      d += lp_term(av[i], ra, bv[i], rb, wc);
    }
  }
  d = wave_groups_sum<PX>(d);
  if (lane < PX) s0[slot] = d;  // (s0's sums of squares were last read before the barrier above)
  __syncthreads();

  // 4. per pixel: the waves in order; the map; the block's pixels in fp64 (lanes of wave 0)
  if (tid < 64) {
    double acc = 0.0;
    if (tid < PX) {
      float t = 0.f;
#pragma unroll 8
      for (int k = 0; k < NW; ++k) t += s0[k * PX + tid];
      if (in) {
        if (map) map[(long)n * P + p] = t;
        acc = (double)t;
      }
    }
    acc = wave_sum_d(acc);
    if (tid == 0) partial[(long)n * gridDim.x + blockIdx.x] = acc;
  }
}

// layer[n] = (sum of image n's block partials: index order per thread, lanes by xor-shuffle, waves in
// order) / P; total[n] = or += layer[n].  One 256-thread block per image.
__global__ __launch_bounds__(256) void lpips_finish_kernel(const double* __restrict__ partial, long nblk, double inv_p,
                                                           float* __restrict__ layer, float* __restrict__ total,
                                                           int accumulate) {
  __shared__ double sh[4];
  const int tid = threadIdx.x, n = blockIdx.x;
  const double* q = partial + (long)n * nblk;
  double s = 0.0;
  for (long i = tid; i < nblk; i += 256) s += q[i];
  s = wave_sum_d(s);
  if ((tid & 63) == 0) sh[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    const float v = (float)((((sh[0] + sh[1]) + sh[2]) + sh[3]) * inv_p);
    layer[n] = v;
    if (total) total[n] = accumulate ? total[n] + v : v;
  }
}

// the difference of the two normalised values, rounded as lp_term rounds it (no contraction)
__device__ __forceinline__ float lp_delta(float a, float ra, float b, float rb) {
#pragma clang fp contract(off)
  const float x = a * ra, y = b * rb;
  return x - y;
}

// The backward of lpips_head_kernel for the upstream gradient gl[n] of layer[n]: same grid, block and
// thread-to-(pixel, channel group) map, the same single load of both features into registers and the
// same fixed-order meeting of the groups (xor-shuffles in a wave, then the waves in order through LDS),
// first for the sums of squares, then for the dot products sum_k s_k a_k (and sum_k s_k b_k when d1 is
// wanted), s_c = w_c (2 gl[n] / P) delta_c.  With u = a / na (a unit vector, 0 where na == 0)
//   dA_c =  ra (s_c - (ra sum_k s_k a_k) u_c),   dB_c = -rb (s_c - (rb sum_k s_k b_k) v_c),
// the closed form of vst_hip.h with its factor ra^2 / na taken apart (ra^2 / na alone leaves fp32's
// range below na ~ 1e-20).  Nothing crosses blocks: no workspace, no atomics.
template <int PX, int G, int CPT>
__global__ __launch_bounds__(PX * G) void lpips_head_bwd_kernel(const float* __restrict__ f0, long bs0,
                                                               const float* __restrict__ f1, long bs1,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ gl, int C, long P,
                                                               float* __restrict__ d0, long bsd0,
                                                               float* __restrict__ d1, long bsd1) {
  constexpr int NW = PX * G / 64;  // waves of the block
  __shared__ float s0[NW * PX], s1[NW * PX];
  __shared__ float r0[PX], r1[PX], i0[PX], i1[PX];
  const int tid = threadIdx.x, px = tid % PX, g = tid / PX;
  const int lane = tid & 63, slot = (tid >> 6) * PX + lane;  // the wave's row in s0 / s1, for lanes < PX
  const int n = blockIdx.y, cpt = C / G;
  const long p = (long)blockIdx.x * PX + px;
  const bool in = p < P, want_b = d1 != nullptr;
  const long off = (long)g * P + p, cstep = (long)G * P;
  const float* a = f0 + (long)n * bs0 + off;
  const float* b = f1 + (long)n * bs1 + off;
  const float gs = (2.f * gl[n]) / (float)P;

  // 1. the thread's channels of both features, once; sums of squares (as the forward)
  float av[CPT], bv[CPT];
  float sa = 0.f, sb = 0.f;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const bool ok = in && i < cpt;
    av[i] = ok ? a[i * cstep] : 0.f;
    bv[i] = ok ? b[i * cstep] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    sa = fmaf(av[i], av[i], sa);
    sb = fmaf(bv[i], bv[i], sb);
  }
  sa = wave_groups_sum<PX>(sa);
  sb = wave_groups_sum<PX>(sb);
  if (lane < PX) {
    s0[slot] = sa;
    s1[slot] = sb;
  }
  __syncthreads();

  // 2. per pixel: the waves in order; 1 / (norm + eps) and 1 / norm (0 at a zero norm: the finite limit)
  if (tid < PX) {
    float ta = 0.f, tb = 0.f;
#pragma unroll 8
    for (int k = 0; k < NW; ++k) {
      ta += s0[k * PX + tid];
      tb += s1[k * PX + tid];
    }
    const float na = sqrtf(ta), nb = sqrtf(tb);
    r0[tid] = 1.0f / (na + LP_EPS);
    r1[tid] = 1.0f / (nb + LP_EPS);
    i0[tid] = na > 0.f ? 1.0f / na : 0.f;
    i1[tid] = nb > 0.f ? 1.0f / nb : 0.f;
  }
  __syncthreads();

  // 3. s_c of the thread's channels and the dot products; s_c is not kept (that would be CPT more live
  // registers): step 5 forms it again from the same operands in the same order
  const float ra = r0[px], rb = r1[px];
  float da = 0.f, db = 0.f;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    if (i < cpt) {
      const float wc = w ? w[g + i * G] : 1.f;
      const float s = (wc * gs) * lp_delta(av[i], ra, bv[i], rb);
      da = fmaf(s, av[i], da);
      if (want_b) db = fmaf(s, bv[i], db);
    }
  }
  da = wave_groups_sum<PX>(da);
  if (want_b) db = wave_groups_sum<PX>(db);
  if (lane < PX) {  // (s0 / s1's sums of squares were last read before the barrier above)
    s0[slot] = da;
    if (want_b) s1[slot] = db;
  }
  __syncthreads();

  // 4. per pixel: the waves in order (every thread sums its own pixel's column: broadcast LDS reads,
  // no third barrier), times ra / na
  float ta = 0.f, tb = 0.f;
#pragma unroll 8
  for (int k = 0; k < NW; ++k) {
    ta += s0[k * PX + px];
    if (want_b) tb += s1[k * PX + px];
  }
  const float ka = (ta * ra) * i0[px], kb = (tb * rb) * i1[px];

  // 5. the gradients from the registers, stored as the features were loaded
  if (!in) return;
  float* ga = d0 + (long)n * bsd0 + off;
  float* gb = want_b ? d1 + (long)n * bsd1 + off : nullptr;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    if (i < cpt) {
      const float wc = w ? w[g + i * G] : 1.f;
      const float s = (wc * gs) * lp_delta(av[i], ra, bv[i], rb);
      ga[i * cstep] = ra * (s - ka * av[i]);
      if (want_b) gb[i * cstep] = -(rb * (s - kb * bv[i]));
    }
  }
}

struct LpScale {
  float shift[3], scale[3];
};

// one thread per pixel (grid-stride over N * H * W), its three channels
__global__ __launch_bounds__(256) void lpips_input_kernel(const void* __restrict__ src, int src_u8,
                                                          float* __restrict__ out, long total, long HW, int swap_rb,
                                                          int normalize, int scaling, LpScale sc) {
#pragma clang fp contract(off)
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long n = idx / HW, p = idx - n * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float t;
      if (src_u8) {
        const uint8_t v = static_cast<const uint8_t*>(src)[3 * idx + (swap_rb ? 2 - c : c)];
        t = (float)((double)v / 127.5 - 1.0);
      } else {
        t = static_cast<const float*>(src)[(n * 3 + c) * HW + p];
        if (normalize == 2) t = t / 255.f;
        if (normalize) t = 2.f * t - 1.f;
      }
      if (scaling) t = (t - sc.shift[c]) / sc.scale[c];
      out[(n * 3 + c) * HW + p] = t;
    }
  }
}

// the backward of the fp32 form: dx = (dout / scale_c) * gain, gain = 1, 2 or 2 / 255 by `normalize`
__global__ __launch_bounds__(256) void lpips_input_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dx,
                                                              long total, long HW, int scaling, float gain, LpScale sc) {
#pragma clang fp contract(off)
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)((idx / HW) % 3);
    float g = dout[idx];
    if (scaling) g = g / (c == 0 ? sc.scale[0] : c == 1 ? sc.scale[1] : sc.scale[2]);
    dx[idx] = g * gain;
  }
}

// out[0] = weight * (total[0] + total[1] + ...) / N, in index order; one thread
__global__ void lpips_mean_kernel(const float* __restrict__ total, int N, float weight, float* __restrict__ out) {
  float s = 0.f;
  for (int n = 0; n < N; ++n) s += total[n];
  out[0] = weight * (s / (float)N);
}

// gl[n] = g[0] * weight / N
__global__ __launch_bounds__(256) void lpips_mean_bwd_kernel(const float* __restrict__ g, int N, float weight,
                                                             float* __restrict__ gl) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n < N) gl[n] = (g[0] * weight) / (float)N;
}

inline int lp_px(long P) { return P <= LP_SMALL_P ? 32 : 64; }
inline long lp_blocks(long P) { return (P + lp_px(P) - 1) / lp_px(P); }
inline bool lp_dims_ok(int N, int C, long P) {
  return N > 0 && N <= 65535 && C >= 16 && C <= 512 && C % 16 == 0 && P > 0 && P < (1L << 31);
}
inline unsigned lp_grid(long total) {
  const long b = (total + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

template <int PX, int G, int CPT>
void lp_launch(const float* f0, long bs0, const float* f1, long bs1, const float* w, int N, int C, long P, float* map,
               double* partial, hipStream_t st) {
  lpips_head_kernel<PX, G, CPT><<<dim3((unsigned)lp_blocks(P), (unsigned)N), PX * G, 0, st>>>(f0, bs0, f1, bs1, w, C, P,
                                                                                          map, partial);
}

struct LpBwdArgs {
  const float *f0, *f1, *w, *gl;
  float *d0, *d1;
  long bs0, bs1, bsd0, bsd1;
};

template <int PX, int G, int CPT>
void lp_launch_bwd(const LpBwdArgs& a, int N, int C, long P, hipStream_t st) {
  lpips_head_bwd_kernel<PX, G, CPT><<<dim3((unsigned)lp_blocks(P), (unsigned)N), PX * G, 0, st>>>(
      a.f0, a.bs0, a.f1, a.bs1, a.w, a.gl, C, P, a.d0, a.bsd0, a.d1, a.bsd1);
}

}  // namespace

extern "C" {

long vst_lpips_head_workspace(int N, int C, long P) {
  if (!lp_dims_ok(N, C, P)) return 0;
  return 8 * (long)N * lp_blocks(P);
}

int vst_lpips_head(const float* f0, long f0_bs, const float* f1, long f1_bs, const float* w, int N, int C, long P,
                   float* layer, float* total, int accumulate, float* map, void* workspace, void* stream) {
  VST_CHECK_ARG(f0 && f1 && layer && workspace && lp_dims_ok(N, C, P));
  VST_CHECK_ARG(f0_bs >= (long)C * P && f1_bs >= (long)C * P && (accumulate == 0 || accumulate == 1));
  VST_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && (!accumulate || total));
  hipStream_t st = (hipStream_t)stream;
  double* partial = static_cast<double*>(workspace);
  // the block shape depends on P and C alone, never on N: an image in a batch runs the same sums as alone
  if (lp_px(P) == 32) {
    if (C % 32 == 0)
      lp_launch<32, 32, 16>(f0, f0_bs, f1, f1_bs, w, N, C, P, map, partial, st);  // C / 32 <= 16 channels a thread
    else
      lp_launch<32, 16, LP_CPT>(f0, f0_bs, f1, f1_bs, w, N, C, P, map, partial, st);
  } else if (C <= 4 * LP_CPT) {
    lp_launch<64, 4, LP_CPT>(f0, f0_bs, f1, f1_bs, w, N, C, P, map, partial, st);
  } else if (C <= 8 * LP_CPT) {
    lp_launch<64, 8, LP_CPT>(f0, f0_bs, f1, f1_bs, w, N, C, P, map, partial, st);
  } else {
    lp_launch<64, 16, LP_CPT>(f0, f0_bs, f1, f1_bs, w, N, C, P, map, partial, st);
  }
  lpips_finish_kernel<<<N, 256, 0, st>>>(partial, lp_blocks(P), 1.0 / (double)P, layer, total, accumulate);
  return vst_launch_status();
}

int vst_lpips_input(const void* src, int src_u8, float* out, long batch_offset, int N, int H, int W, int swap_rb,
                    int normalize, int scaling, void* stream) {
  VST_CHECK_ARG(src && out && N > 0 && H > 0 && W > 0 && batch_offset >= 0 && (long)H * W < (1L << 31));
  VST_CHECK_ARG((src_u8 == 0 || src_u8 == 1) && (swap_rb == 0 || swap_rb == 1) && normalize >= 0 && normalize <= 2 &&
                (scaling == 0 || scaling == 1));
  // torch.Tensor([...]) of the reference's Python doubles: their nearest fp32 values
  const LpScale sc = {{-0.030f, -0.088f, -0.188f}, {0.458f, 0.448f, 0.450f}};
  const long HW = (long)H * W, total = (long)N * HW;
  lpips_input_kernel<<<lp_grid(total), 256, 0, (hipStream_t)stream>>>(src, src_u8, out + batch_offset * 3 * HW, total, HW,
                                                                      swap_rb, normalize, scaling, sc);
  return vst_launch_status();
}

int vst_lpips_head_bwd(const float* f0, long f0_bs, const float* f1, long f1_bs, const float* w, const float* gl, int N,
                       int C, long P, float* d0, long d0_bs, float* d1, long d1_bs, void* stream) {
  VST_CHECK_ARG(f0 && f1 && gl && d0 && lp_dims_ok(N, C, P));
  VST_CHECK_ARG(f0_bs >= (long)C * P && f1_bs >= (long)C * P && d0_bs >= (long)C * P && (!d1 || d1_bs >= (long)C * P));
  hipStream_t st = (hipStream_t)stream;
  const LpBwdArgs a = {f0, f1, w, gl, d0, d1, f0_bs, f1_bs, d0_bs, d1_bs};
  // the forward's block shapes (vst_lpips_head): the same sums in the same order
  if (lp_px(P) == 32) {
    if (C % 32 == 0)
      lp_launch_bwd<32, 32, 16>(a, N, C, P, st);
    else
      lp_launch_bwd<32, 16, LP_CPT>(a, N, C, P, st);
  } else if (C <= 4 * LP_CPT) {
    lp_launch_bwd<64, 4, LP_CPT>(a, N, C, P, st);
  } else if (C <= 8 * LP_CPT) {
    lp_launch_bwd<64, 8, LP_CPT>(a, N, C, P, st);
  } else {
    lp_launch_bwd<64, 16, LP_CPT>(a, N, C, P, st);
  }
  return vst_launch_status();
}

int vst_lpips_input_bwd(const float* dout, float* dx, int N, int H, int W, int normalize, int scaling, void* stream) {
  VST_CHECK_ARG(dout && dx && N > 0 && H > 0 && W > 0 && (long)H * W < (1L << 31));
  VST_CHECK_ARG(normalize >= 0 && normalize <= 2 && (scaling == 0 || scaling == 1));
  const LpScale sc = {{-0.030f, -0.088f, -0.188f}, {0.458f, 0.448f, 0.450f}};
  const float gain = normalize == 2 ? (float)(2.0 / 255.0) : normalize == 1 ? 2.f : 1.f;
  const long HW = (long)H * W, total = 3 * (long)N * HW;
  lpips_input_bwd_kernel<<<lp_grid(total), 256, 0, (hipStream_t)stream>>>(dout, dx, total, HW, scaling, gain, sc);
  return vst_launch_status();
}

int vst_lpips_mean(const float* total, int N, float weight, float* out, void* stream) {
  VST_CHECK_ARG(total && out && N > 0 && N <= 65535);
  lpips_mean_kernel<<<1, 1, 0, (hipStream_t)stream>>>(total, N, weight, out);
  return vst_launch_status();
}

int vst_lpips_mean_bwd(const float* g, int N, float weight, float* gl, void* stream) {
  VST_CHECK_ARG(g && gl && N > 0 && N <= 65535);
  lpips_mean_bwd_kernel<<<(N + 255) / 256, 256, 0, (hipStream_t)stream>>>(g, N, weight, gl);
  return vst_launch_status();
}

}  // extern "C"
