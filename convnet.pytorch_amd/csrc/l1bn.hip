// l1bn.hip -- L1 batch normalisation (training + inference) with fused residual-add and ReLU, NHWC, gfx950.
//
// Replaces the reference's L1BatchNorm2d (models/modules/lp_norm.py:238-291 there, normalized=True,
// noise=False), which resnet(bn_norm='L1') puts in the place of every nn.BatchNorm2d (models/resnet.py:393-399), and its
// autograd backward.  Per channel over the M = N*H*W values:
//   mu = mean(y)    V = mean|y - mu|    s = 1 / (V*sqrt(pi/2) + eps)    z = (y - mu)*s*gamma + beta
//   running_mean <- running_mean*momentum + mu*(1 - momentum)     running_var <- running_var*momentum + s*(1 - momentum)
//   (running_var holds the SCALE; inference is z = (y - running_mean)*running_var*gamma + beta)
// backward, with g the upstream gradient behind the ReLU mask, xhat = (y - mu)*s, sg = sign(y - mu), sign(0) = 0:
//   dbeta = sum g    dgamma = sum g*xhat    dy = gamma*s*[(g - mean g) - sqrt(pi/2)*(dgamma/M)*(sg - mean sg)]
//
// Same design as bn.hip (bn_common.h): a lane owns one 16-byte channel chunk and walks over pixels, fp32 accumulators, wave
// shuffles + one LDS step per workgroup, partial rows + a fixed-order finalize launch between workgroups (no atomics:
// deterministic).  V needs mu, so the forward reads y three times:
//   forward (train):  l1bn_sum -> l1bn_mean -> l1bn_absdev -> l1bn_finalize -> l1bn_apply
//   backward:         l1bn_bwd_reduce -> l1bn_bwd_finalize -> l1bn_bwd_apply
// The apply passes use the centred form (y - mu)*scale + beta: a constant channel (V = 0, scale = gamma/eps) then gives
// z = beta exactly, where y*scale + (beta - mu*scale) would round beta to an ulp of mu*scale.
#include "bn_common.h"

#define L1BN_K 1.2533141373155003   /* sqrt(pi / 2): E|x - mu| of a normal variable is sigma / this */
#define L1BN_STATS 7                /* stats = [mu | s | scale = gamma*s | beta | mean sg | mu_lo | s_lo], C floats each */
/* Up to this many values per channel the whole operator runs in float64, one thread per 16-byte chunk column
 * (l1bn_small_*).  The statistics of a handful of values are ill-conditioned: at M = 2 every |y - mu| is the same, xhat is
 * +-(1 - eps*s)/sqrt(pi/2) whatever the input, and the two terms of dy cancel to eps*s (~1e-5) of their size, so fp32 sums
 * and coefficients leave dy with a relative error of 1e-3..1e-2.  Tensors this small cost one short launch either way. */
#define L1BN_SMALL_M 32

__device__ __forceinline__ float l1bn_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// ------------------------------------------------------------------------------------------------
// Pass 1: per-channel sum of y, as two interleaved accumulator chains (rows u even | odd of the unrolled loop) that the
// partial row carries side by side: [sum even | sum odd].
template <typename T, bool NT>
__global__ __launch_bounds__(256) void l1bn_sum_kernel(const char* y, float* partial, int M, int C, int tpr_log2) {
  constexpr int CH = ElemTraits<T>::kChunk;
  constexpr int EB = ElemTraits<T>::kBytes;
  __shared__ float red[256 * 2 * CH];
  const int tid = threadIdx.x;
  const int tpr = 1 << tpr_log2, rpp = 256 >> tpr_log2;
  const int cpr = C / CH;
  const int tcol = tid & (tpr - 1), rsub = tid >> tpr_log2;
  const int col = blockIdx.y * tpr + tcol;
  float s0[CH], s1[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) { s0[e] = 0.f; s1[e] = 0.f; }
  if (col < cpr) {
    const int step = gridDim.x * rpp;
    const size_t cb = (size_t)col * CH * EB, rb = (size_t)C * EB;
    int row = blockIdx.x * rpp + rsub;
    for (; (long long)row + 3ll * step < M; row += 4 * step) {   // 4 independent 16-byte loads in flight per lane
      u32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = bn_ld<NT, 11>(y + (size_t)(row + u * step) * rb + cb);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float f[CH];
        Chunk<T>::unpack(v[u], f);
#pragma unroll
        for (int e = 0; e < CH; ++e) { if (u & 1) s1[e] += f[e]; else s0[e] += f[e]; }
      }
    }
    for (; row < M; row += step) {
      float f[CH];
      Chunk<T>::unpack(bn_ld<NT, 11>(y + (size_t)row * rb + cb), f);
#pragma unroll
      for (int e = 0; e < CH; ++e) s0[e] += f[e];
    }
  }
  bn_block_colsum<CH>(s0, s1, red, tpr_log2, tid);
  if (rsub == 0 && col < cpr) {
    float* dst = partial + (size_t)blockIdx.x * 2 * C + col * CH;
#pragma unroll
    for (int e = 0; e < CH; ++e) { dst[e] = s0[e]; dst[C + e] = s1[e]; }
  }
}

// mu[c] = (sum even + sum odd) / M
__global__ __launch_bounds__(256) void l1bn_mean_kernel(const float* partial, int nrb, int M, int C, float* mean) {
  __shared__ double red[512];
  const int c = blockIdx.x * BN_FC + (threadIdx.x % BN_FC);
  const int part = threadIdx.x / BN_FC;
  double s0, s1;
  bn_sum_partials(partial, nrb, C, c, part, red, s0, s1);
  if (c >= C || part != 0) return;
  mean[c] = (float)((s0 + s1) / (double)M);
}

// Pass 2: per-channel sum |y - mu| and sum sign(y - mu) (the differences in fp32, as the apply passes form them).
template <typename T, bool NT>
__global__ __launch_bounds__(256) void l1bn_absdev_kernel(const char* y, const float* mean, float* partial, int M, int C,
                                                         int tpr_log2) {
  constexpr int CH = ElemTraits<T>::kChunk;
  constexpr int EB = ElemTraits<T>::kBytes;
  __shared__ float red[256 * 2 * CH];
  const int tid = threadIdx.x;
  const int tpr = 1 << tpr_log2, rpp = 256 >> tpr_log2;
  const int cpr = C / CH;
  const int tcol = tid & (tpr - 1), rsub = tid >> tpr_log2;
  const int col = blockIdx.y * tpr + tcol;
  float a[CH], b[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) { a[e] = 0.f; b[e] = 0.f; }
  if (col < cpr) {
    float mu[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) mu[e] = mean[col * CH + e];
    const int step = gridDim.x * rpp;
    const size_t cb = (size_t)col * CH * EB, rb = (size_t)C * EB;
    int row = blockIdx.x * rpp + rsub;
    for (; (long long)row + 3ll * step < M; row += 4 * step) {   // 4 independent 16-byte loads in flight per lane
      u32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = bn_ld<NT, 12>(y + (size_t)(row + u * step) * rb + cb);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float f[CH];
        Chunk<T>::unpack(v[u], f);
#pragma unroll
        for (int e = 0; e < CH; ++e) { const float d = f[e] - mu[e]; a[e] += fabsf(d); b[e] += l1bn_sign(d); }
      }
    }
    for (; row < M; row += step) {
      float f[CH];
      Chunk<T>::unpack(bn_ld<NT, 12>(y + (size_t)row * rb + cb), f);
#pragma unroll
      for (int e = 0; e < CH; ++e) { const float d = f[e] - mu[e]; a[e] += fabsf(d); b[e] += l1bn_sign(d); }
    }
  }
  bn_block_colsum<CH>(a, b, red, tpr_log2, tid);
  if (rsub == 0 && col < cpr) {
    float* dst = partial + (size_t)blockIdx.x * 2 * C + col * CH;
#pragma unroll
    for (int e = 0; e < CH; ++e) { dst[e] = a[e]; dst[C + e] = b[e]; }
  }
}

// BN_FC channels per workgroup: V, s, the coefficients of the apply passes, mean sg, and both running buffers (updated on
// the device in the reference's fp32 arithmetic: old*momentum + new*(1 - momentum); running_var holds the scale s).
__global__ __launch_bounds__(256) void l1bn_finalize_kernel(const float* partial, int nrb, int M, int C, const float* gamma,
                                                           const float* beta, float* running_mean, float* running_var,
                                                           float momentum, float eps, float* stats) {
  __shared__ double red[512];
  const int c = blockIdx.x * BN_FC + (threadIdx.x % BN_FC);
  const int part = threadIdx.x / BN_FC;
  const bool owner = c < C && part == 0;   // operands requested before the partial reduction (latency)
  const float g_pre = (owner && gamma != nullptr) ? gamma[c] : 1.f;
  const float b_pre = (owner && beta != nullptr) ? beta[c] : 0.f;
  const float mu = owner ? stats[c] : 0.f;
  const float rm_pre = (owner && running_mean != nullptr) ? running_mean[c] : 0.f;
  const float rv_pre = (owner && running_mean != nullptr) ? running_var[c] : 0.f;
  double a, b;
  bn_sum_partials(partial, nrb, C, c, part, red, a, b);
  if (c >= C || part != 0) return;
  const double V = a / (double)M;
  const float s = (float)(1.0 / (V * L1BN_K + (double)eps));
  stats[C + c] = s;
  stats[2 * C + c] = g_pre * s;
  stats[3 * C + c] = b_pre;
  stats[4 * C + c] = (float)(b / (double)M);
  stats[5 * C + c] = 0.f;   // (the lo halves of mu and s: only the float64 path for small M carries them)
  stats[6 * C + c] = 0.f;
  if (running_mean != nullptr) {
    const float keep = (float)(1.0 - (double)momentum);
    running_mean[c] = rm_pre * momentum + mu * keep;
    running_var[c] = rv_pre * momentum + s * keep;
  }
}

// Inference coefficients from the running buffers: [running_mean | gamma*running_var | beta] (no eps, no square root).
__global__ __launch_bounds__(256) void l1bn_infer_coeffs_kernel(int C, const float* gamma, const float* beta,
                                                               const float* running_mean, const float* running_var,
                                                               float* coeffs) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  coeffs[c] = running_mean[c];
  coeffs[C + c] = (gamma != nullptr ? gamma[c] : 1.f) * running_var[c];
  coeffs[2 * C + c] = beta != nullptr ? beta[c] : 0.f;
}

// z = act((y - mu[c])*scale[c] + beta[c] (+ residual)).  `mask` (ReLU behind a residual add): one byte per 16-byte chunk
// records which outputs were positive, as in bn_apply_kernel.
template <typename T, bool NT>
__global__ __launch_bounds__(256) void l1bn_apply_kernel(const char* y, const char* res, char* z, unsigned char* mask,
                                                        const float* mean, const float* scale, const float* beta, int M,
                                                        int C, int relu, int tpr_log2) {
  constexpr int CH = ElemTraits<T>::kChunk;
  constexpr int EB = ElemTraits<T>::kBytes;
  const int tid = threadIdx.x;
  const int tpr = 1 << tpr_log2, rpp = 256 >> tpr_log2;
  const int cpr = C / CH;
  const int col = blockIdx.y * tpr + (tid & (tpr - 1)), rsub = tid >> tpr_log2;
  if (col >= cpr) return;
  float mu[CH], sc[CH], be[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) { mu[e] = mean[col * CH + e]; sc[e] = scale[col * CH + e]; be[e] = beta[col * CH + e]; }
  const int step = gridDim.x * rpp;
#pragma unroll 4
  for (int row = blockIdx.x * rpp + rsub; row < M; row += step) {
    const size_t off = ((size_t)row * C + (size_t)col * CH) * EB;
    float f[CH];
    Chunk<T>::unpack(bn_ld<NT, 13>(y + off), f);
#pragma unroll
    for (int e = 0; e < CH; ++e) f[e] = fmaf(f[e] - mu[e], sc[e], be[e]);
    if (res != nullptr) {
      float r[CH];
      Chunk<T>::unpack(bn_ld<NT, 14>(res + off), r);
#pragma unroll
      for (int e = 0; e < CH; ++e) f[e] += r[e];
    }
    if (relu) {
      unsigned int bits = 0;
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        bits |= (f[e] > 0.f ? 1u : 0u) << e;
        f[e] = f[e] > 0.f ? f[e] : 0.f;
      }
      if (mask != nullptr) mask[(size_t)row * cpr + col] = (unsigned char)bits;
    }
    cn_st16(z + off, Chunk<T>::pack(f));   // plain: the next convolution reads z straight away
  }
}

// Per-channel sum(g) and sum(g * xhat), g = dz * relu_mask; the mask is the byte mask the apply pass wrote (a residual was
// added) or, with zmask == nullptr and relu != 0, recomputed as (y - mu)*scale + beta > 0.
template <typename T, bool NT>
__global__ __launch_bounds__(256) void l1bn_bwd_reduce_kernel(const char* dz, const char* y, const unsigned char* zmask,
                                                             const float* stats, float* partial, int M, int C, int relu,
                                                             int tpr_log2) {
  constexpr int CH = ElemTraits<T>::kChunk;
  constexpr int EB = ElemTraits<T>::kBytes;
  __shared__ float red[256 * 2 * CH];
  const int tid = threadIdx.x;
  const int tpr = 1 << tpr_log2, rpp = 256 >> tpr_log2;
  const int cpr = C / CH;
  const int tcol = tid & (tpr - 1), rsub = tid >> tpr_log2;
  const int col = blockIdx.y * tpr + tcol;
  float s1[CH], s2[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
  if (col < cpr) {
    float mu[CH], is[CH], sc[CH], be[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      mu[e] = stats[col * CH + e];
      is[e] = stats[C + col * CH + e];
      sc[e] = stats[2 * C + col * CH + e];
      be[e] = stats[3 * C + col * CH + e];
    }
    const int step = gridDim.x * rpp;
    const size_t cb = (size_t)col * CH * EB, rb = (size_t)C * EB;
    auto accum = [&](const u32x4& gz, const u32x4& vy, unsigned int bits) {
      float g[CH], v[CH];
      Chunk<T>::unpack(gz, g);
      Chunk<T>::unpack(vy, v);
#pragma unroll
      for (int e = 0; e < CH; ++e) v[e] -= mu[e];
      if (relu) {
        if (zmask != nullptr) {
#pragma unroll
          for (int e = 0; e < CH; ++e) g[e] = ((bits >> e) & 1u) ? g[e] : 0.f;
        } else {
#pragma unroll
          for (int e = 0; e < CH; ++e) g[e] = fmaf(v[e], sc[e], be[e]) > 0.f ? g[e] : 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        s1[e] += g[e];
        s2[e] = fmaf(g[e], v[e] * is[e], s2[e]);
      }
    };
    int row = blockIdx.x * rpp + rsub;
    for (; (long long)row + 3ll * step < M; row += 4 * step) {   // 8-12 independent loads in flight per lane
      u32x4 gz[4], vy[4];
      unsigned int bits[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = row + u * step;
        gz[u] = bn_ld<NT, 15>(dz + (size_t)r * rb + cb);
        vy[u] = bn_ld<NT, 16>(y + (size_t)r * rb + cb);
        if (relu && zmask != nullptr) bits[u] = zmask[(size_t)r * cpr + col];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) accum(gz[u], vy[u], bits[u]);
    }
    for (; row < M; row += step) {
      unsigned int bits = 0u;
      if (relu && zmask != nullptr) bits = zmask[(size_t)row * cpr + col];
      accum(bn_ld<NT, 15>(dz + (size_t)row * rb + cb), bn_ld<NT, 16>(y + (size_t)row * rb + cb), bits);
    }
  }
  bn_block_colsum<CH>(s1, s2, red, tpr_log2, tid);
  if (rsub == 0 && col < cpr) {
    float* dst = partial + (size_t)blockIdx.x * 2 * C + col * CH;
#pragma unroll
    for (int e = 0; e < CH; ++e) { dst[e] = s1[e]; dst[C + e] = s2[e]; }
  }
}

// dgamma / dbeta (optionally accumulated) and the three per-channel coefficients of
//   dy = c1*g + c2*sg + c3     ( = gamma*s*[(g - mean g) - sqrt(pi/2)*(dgamma/M)*(sg - mean sg)] )
__global__ __launch_bounds__(256) void l1bn_bwd_finalize_kernel(const float* partial, int nrb, int M, int C,
                                                               const float* gamma, const float* stats, float* dgamma,
                                                               float* dbeta, float beta_acc, float gscale, float* coef) {
  __shared__ double red[512];
  const int c = blockIdx.x * BN_FC + (threadIdx.x % BN_FC);
  const int part = threadIdx.x / BN_FC;
  const bool owner = c < C && part == 0;   // operands requested before the partial reduction (latency)
  const float g = (owner && gamma != nullptr) ? gamma[c] : 1.f;
  const float s_pre = owner ? stats[C + c] : 0.f;
  const float msg_pre = owner ? stats[4 * C + c] : 0.f;
  const float dg_pre = (owner && dgamma != nullptr && beta_acc != 0.f) ? dgamma[c] : 0.f;
  const float db_pre = (owner && dbeta != nullptr && beta_acc != 0.f) ? dbeta[c] : 0.f;
  double s1, s2;
  bn_sum_partials(partial, nrb, C, c, part, red, s1, s2);
  if (c >= C || part != 0) return;
  if (dgamma != nullptr) dgamma[c] = (beta_acc != 0.f ? beta_acc * dg_pre : 0.f) + (float)s2 * gscale;
  if (dbeta != nullptr) dbeta[c] = (beta_acc != 0.f ? beta_acc * db_pre : 0.f) + (float)s1 * gscale;
  const double c1 = (double)g * (double)s_pre;
  const double c2 = -c1 * L1BN_K * s2 / (double)M;
  coef[c] = (float)c1;
  coef[C + c] = (float)c2;
  coef[2 * C + c] = (float)(-c1 * s1 / (double)M - c2 * (double)msg_pre);
}

template <typename T, bool NT>
__global__ __launch_bounds__(256) void l1bn_bwd_apply_kernel(const char* dz, const char* y, const unsigned char* zmask,
                                                            const float* stats, const float* coef, char* dy, char* dres,
                                                            int M, int C, int relu, int tpr_log2) {
  constexpr int CH = ElemTraits<T>::kChunk;
  constexpr int EB = ElemTraits<T>::kBytes;
  const int tid = threadIdx.x;
  const int tpr = 1 << tpr_log2, rpp = 256 >> tpr_log2;
  const int cpr = C / CH;
  const int col = blockIdx.y * tpr + (tid & (tpr - 1)), rsub = tid >> tpr_log2;
  if (col >= cpr) return;
  float c1[CH], c2[CH], c3[CH], mu[CH], sc[CH], be[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    c1[e] = coef[col * CH + e];
    c2[e] = coef[C + col * CH + e];
    c3[e] = coef[2 * C + col * CH + e];
    mu[e] = stats[col * CH + e];
    sc[e] = stats[2 * C + col * CH + e];
    be[e] = stats[3 * C + col * CH + e];
  }
  const int step = gridDim.x * rpp;
#pragma unroll 2
  for (int row = blockIdx.x * rpp + rsub; row < M; row += step) {
    const size_t off = ((size_t)row * C + (size_t)col * CH) * EB;
    float g[CH], v[CH];
    Chunk<T>::unpack(bn_ld<NT, 17>(dz + off), g);
    Chunk<T>::unpack(bn_ld<NT, 18>(y + off), v);
#pragma unroll
    for (int e = 0; e < CH; ++e) v[e] -= mu[e];
    if (relu) {
      if (zmask != nullptr) {
        const unsigned int bits = zmask[(size_t)row * cpr + col];
#pragma unroll
        for (int e = 0; e < CH; ++e) g[e] = ((bits >> e) & 1u) ? g[e] : 0.f;
      } else {
#pragma unroll
        for (int e = 0; e < CH; ++e) g[e] = fmaf(v[e], sc[e], be[e]) > 0.f ? g[e] : 0.f;
      }
    }
    if (dres != nullptr) bn_st<NT, 17>(dres + off, Chunk<T>::pack(g));
    float o[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) o[e] = fmaf(c1[e], g[e], fmaf(c2[e], l1bn_sign(v[e]), c3[e]));
    bn_st<NT, 17>(dy + off, Chunk<T>::pack(o));
  }
}

// ------------------------------------------------------------------------------------------------
// M <= L1BN_SMALL_M: float64 throughout.  mu and s are handed to the backward as (hi, lo) float pairs; the forward uses the
// pair's value itself, so both passes take the ReLU decision from the same numbers.
__device__ __forceinline__ double l1bn_pair(float hi, float lo) { return (double)hi + (double)lo; }
__device__ __forceinline__ float l1bn_lo(double v) { return (float)(v - (double)(float)v); }

template <typename T>
__global__ __launch_bounds__(256) void l1bn_small_fwd_kernel(const char* y, const char* res, char* z, unsigned char* mask,
                                                            const float* gamma, const float* beta, float* running_mean,
                                                            float* running_var, float momentum, float eps, float* stats,
                                                            int M, int C, int relu) {
  constexpr int CH = ElemTraits<T>::kChunk;
  constexpr int EB = ElemTraits<T>::kBytes;
  const int cpr = C / CH;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= cpr) return;
  const size_t cb = (size_t)col * CH * EB, rb = (size_t)C * EB;
  double mu[CH], a[CH], b[CH], sc[CH];
  float be[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) { mu[e] = 0.0; a[e] = 0.0; b[e] = 0.0; }
  for (int row = 0; row < M; ++row) {
    float f[CH];
    Chunk<T>::unpack(cn_ld16(y + (size_t)row * rb + cb), f);
#pragma unroll
    for (int e = 0; e < CH; ++e) mu[e] += (double)f[e];
  }
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    const double m = mu[e] / (double)M;
    mu[e] = l1bn_pair((float)m, l1bn_lo(m));
  }
  for (int row = 0; row < M; ++row) {
    float f[CH];
    Chunk<T>::unpack(cn_ld16(y + (size_t)row * rb + cb), f);
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      const double d = (double)f[e] - mu[e];
      a[e] += fabs(d);
      b[e] += d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    }
  }
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    const int c = col * CH + e;
    const double sd = 1.0 / (a[e] / (double)M * L1BN_K + (double)eps);
    const float s_hi = (float)sd, s_lo = l1bn_lo(sd);
    const float g = gamma != nullptr ? gamma[c] : 1.f;
    be[e] = beta != nullptr ? beta[c] : 0.f;
    sc[e] = (double)g * l1bn_pair(s_hi, s_lo);
    stats[c] = (float)mu[e];
    stats[C + c] = s_hi;
    stats[2 * C + c] = g * s_hi;
    stats[3 * C + c] = be[e];
    stats[4 * C + c] = (float)(b[e] / (double)M);
    stats[5 * C + c] = l1bn_lo(mu[e]);
    stats[6 * C + c] = s_lo;
    if (running_mean != nullptr) {
      const float keep = (float)(1.0 - (double)momentum);
      running_mean[c] = running_mean[c] * momentum + (float)mu[e] * keep;
      running_var[c] = running_var[c] * momentum + s_hi * keep;
    }
  }
  if (z == nullptr) return;
  for (int row = 0; row < M; ++row) {
    const size_t off = (size_t)row * rb + cb;
    float f[CH], r[CH];
    Chunk<T>::unpack(cn_ld16(y + off), f);
    if (res != nullptr) Chunk<T>::unpack(cn_ld16(res + off), r);
    unsigned int bits = 0;
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      double v = ((double)f[e] - mu[e]) * sc[e] + (double)be[e];
      if (res != nullptr) v += (double)r[e];
      if (relu) {
        bits |= (v > 0.0 ? 1u : 0u) << e;
        v = v > 0.0 ? v : 0.0;
      }
      f[e] = (float)v;
    }
    if (relu && mask != nullptr) mask[(size_t)row * cpr + col] = (unsigned char)bits;
    cn_st16(z + off, Chunk<T>::pack(f));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void l1bn_small_bwd_kernel(const char* dz, const char* y, const unsigned char* zmask,
                                                            const float* gamma, const float* stats, char* dy, char* dres,
                                                            float* dgamma, float* dbeta, float beta_acc, float gscale,
                                                            int M, int C, int relu) {
  constexpr int CH = ElemTraits<T>::kChunk;
  constexpr int EB = ElemTraits<T>::kBytes;
  const int cpr = C / CH;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= cpr) return;
  const size_t cb = (size_t)col * CH * EB, rb = (size_t)C * EB;
  double mu[CH], sd[CH], sc[CH], s1[CH], s2[CH], b[CH];
  float be[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    const int c = col * CH + e;
    mu[e] = l1bn_pair(stats[c], stats[5 * C + c]);
    sd[e] = l1bn_pair(stats[C + c], stats[6 * C + c]);
    sc[e] = (double)(gamma != nullptr ? gamma[c] : 1.f) * sd[e];
    be[e] = stats[3 * C + c];
    s1[e] = 0.0; s2[e] = 0.0; b[e] = 0.0;
  }
  // g = dz behind the ReLU mask (read, or recomputed from the forward's own expression)
  auto masked = [&](int row, const float* f, float* g) {
    Chunk<T>::unpack(cn_ld16(dz + (size_t)row * rb + cb), g);
    if (!relu) return;
    if (zmask != nullptr) {
      const unsigned int bits = zmask[(size_t)row * cpr + col];
#pragma unroll
      for (int e = 0; e < CH; ++e) g[e] = ((bits >> e) & 1u) ? g[e] : 0.f;
    } else {
#pragma unroll
      for (int e = 0; e < CH; ++e) g[e] = ((double)f[e] - mu[e]) * sc[e] + (double)be[e] > 0.0 ? g[e] : 0.f;
    }
  };
  for (int row = 0; row < M; ++row) {
    float f[CH], g[CH];
    Chunk<T>::unpack(cn_ld16(y + (size_t)row * rb + cb), f);
    masked(row, f, g);
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      const double d = (double)f[e] - mu[e];
      s1[e] += (double)g[e];
      s2[e] += (double)g[e] * (d * sd[e]);
      b[e] += d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    }
  }
  double t[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    const int c = col * CH + e;
    if (dgamma != nullptr) dgamma[c] = (beta_acc != 0.f ? beta_acc * dgamma[c] : 0.f) + (float)s2[e] * gscale;
    if (dbeta != nullptr) dbeta[c] = (beta_acc != 0.f ? beta_acc * dbeta[c] : 0.f) + (float)s1[e] * gscale;
    t[e] = L1BN_K * s2[e] / (double)M;
    s1[e] /= (double)M;
    b[e] /= (double)M;
  }
  for (int row = 0; row < M; ++row) {
    const size_t off = (size_t)row * rb + cb;
    float f[CH], g[CH], o[CH];
    Chunk<T>::unpack(cn_ld16(y + off), f);
    masked(row, f, g);
    if (dres != nullptr) cn_st16(dres + off, Chunk<T>::pack(g));
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      const double d = (double)f[e] - mu[e];
      const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
      o[e] = (float)(sc[e] * (((double)g[e] - s1[e]) - t[e] * (sg - b[e])));
    }
    cn_st16(dy + off, Chunk<T>::pack(o));
  }
}

extern "C" size_t cn_l1bn_workspace(int M, int C, int dtype) {
  if (!cn_dtype_ok(dtype)) return 0;
  const int CH = cn_dtype_chunk(dtype);
  if (C <= 0 || C % CH != 0 || M <= 0) return 0;
  BnMap m = bn_map(C / CH);
  const int nrb = bn_row_blocks(M, m, 2048);   // upper bound over the tunable reduce-grid sizes
  return (size_t)nrb * 2 * C * sizeof(float);
}

static int l1bn_check(const char* who, int M, int C, int dtype) {
  if (!cn_dtype_ok(dtype)) { cn_set_error("%s: bad dtype %d", who, dtype); return CN_EINVAL; }
  const int CH = cn_dtype_chunk(dtype);
  if (M <= 0 || M > (1 << 30) || C <= 0 || C % CH != 0) {   // (row indices stay in int through the unrolled loops)
    cn_set_error("%s: need 0 < M <= 2^30 and C (%d) a multiple of %d", who, C, CH);
    return CN_ESHAPE;
  }
  return CN_OK;
}

// Training forward.  stats_out = [mu | s | gamma*s | beta | mean sg | mu_lo | s_lo] (7*C floats).  z == NULL: statistics only.
extern "C" cn_status cn_l1bn_fwd_train(const void* y, const void* residual, void* z, unsigned char* relu_mask,
                                       const float* gamma, const float* beta, float* running_mean, float* running_var,
                                       float momentum, float eps, float* stats_out, int M, int C, int relu, int dtype,
                                       void* workspace, size_t ws_bytes, void* stream_) {
  int rc = l1bn_check("l1bn_fwd_train", M, C, dtype);
  if (rc) return rc;
  if (y == nullptr || stats_out == nullptr) { cn_set_error("l1bn_fwd_train: null operand"); return CN_EINVAL; }
  if ((running_mean == nullptr) != (running_var == nullptr)) {
    cn_set_error("l1bn_fwd_train: running_mean and running_var come together");
    return CN_EINVAL;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const int CH = cn_dtype_chunk(dtype);
  BnMap m = bn_map(C / CH);
  const int nrb = bn_row_blocks(M, m, cn_get_option("bn_reduce_blocks", BN_REDUCE_BLOCKS));
  if (workspace == nullptr || ws_bytes < (size_t)nrb * 2 * C * sizeof(float)) {
    cn_set_error("l1bn_fwd_train: workspace too small");
    return CN_EWORKSPACE;
  }
  float* partial = (float*)workspace;   // both reductions use it in turn (stream order)
  dim3 grid((unsigned)nrb, (unsigned)m.gy);
  dim3 fgrid((unsigned)((C + BN_FC - 1) / BN_FC));
  if (M <= L1BN_SMALL_M) {   // a handful of values per channel: float64, one launch
    CN_DISPATCH_T(dtype, CN_LAUNCH(l1bn_small_fwd_kernel<TT>, dim3((unsigned)((C / CH + 255) / 256)), dim3(256), stream,
                                   (const char*)y, (const char*)residual, (char*)z, relu_mask, gamma, beta, running_mean,
                                   running_var, momentum, eps, stats_out, M, C, relu));
    return cn_check_launch("l1bn_fwd_train");
  }
  CnMarkLast last;   // an armed completion mark goes on the call's last kernel only
  BN_DISPATCH_PLAIN(l1bn_sum_kernel, dtype, grid, stream, (const char*)y, partial, M, C, m.tpr_log2);
  CN_LAUNCH(l1bn_mean_kernel, fgrid, dim3(256), stream, (const float*)partial, nrb, M, C, stats_out);
  BN_DISPATCH_PLAIN(l1bn_absdev_kernel, dtype, grid, stream, (const char*)y, (const float*)stats_out, partial, M, C, m.tpr_log2);
  if (z == nullptr) last.release();
  CN_LAUNCH(l1bn_finalize_kernel, fgrid, dim3(256), stream, (const float*)partial, nrb, M, C, gamma, beta, running_mean,
            running_var, momentum, eps, stats_out);
  if (z == nullptr) return cn_check_launch("l1bn_fwd_train");
  const int nab = bn_row_blocks(M, m, cn_get_option("bn_apply_blocks", BN_APPLY_BLOCKS));
  dim3 agrid((unsigned)nab, (unsigned)m.gy);
  last.release();
  BN_DISPATCH(l1bn_apply_kernel, dtype, bn_nt_flag(M, C, dtype), agrid, stream, (const char*)y, (const char*)residual, (char*)z, relu_mask, (const float*)stats_out, (const float*)(stats_out + 2 * C), (const float*)(stats_out + 3 * C), M, C, relu, m.tpr_log2);
  return cn_check_launch("l1bn_fwd_train");
}

// Inference forward from the running buffers.  coeffs = scratch of 3*C floats.
extern "C" cn_status cn_l1bn_fwd_infer(const void* y, const void* residual, void* z, const float* gamma, const float* beta,
                                       const float* running_mean, const float* running_var, float* coeffs, int M, int C,
                                       int relu, int dtype, void* stream_) {
  int rc = l1bn_check("l1bn_fwd_infer", M, C, dtype);
  if (rc) return rc;
  if (y == nullptr || z == nullptr || running_mean == nullptr || running_var == nullptr || coeffs == nullptr) {
    cn_set_error("l1bn_fwd_infer: null operand");
    return CN_EINVAL;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const int CH = cn_dtype_chunk(dtype);
  BnMap m = bn_map(C / CH);
  CnMarkLast last;
  CN_LAUNCH(l1bn_infer_coeffs_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), stream, C, gamma, beta, running_mean,
            running_var, coeffs);
  const int nab = bn_row_blocks(M, m, cn_get_option("bn_apply_blocks", BN_APPLY_BLOCKS));
  dim3 agrid((unsigned)nab, (unsigned)m.gy);
  last.release();
  BN_DISPATCH(l1bn_apply_kernel, dtype, bn_nt_flag(M, C, dtype), agrid, stream, (const char*)y, (const char*)residual, (char*)z, (unsigned char*)nullptr, (const float*)coeffs, (const float*)(coeffs + C), (const float*)(coeffs + 2 * C), M, C, relu, m.tpr_log2);
  return cn_check_launch("l1bn_fwd_infer");
}

// Training backward.  stats = the 7*C floats written by cn_l1bn_fwd_train; coef_scratch = 3*C floats.  dgamma / dbeta are
// written (beta_acc = 0) or accumulated (beta_acc = 1); dres (optional) receives the masked upstream gradient.
extern "C" cn_status cn_l1bn_bwd(const void* dz, const void* y, const unsigned char* relu_mask, const float* gamma,
                                 const float* stats, void* dy, void* dres, float* dgamma, float* dbeta, float beta_acc,
                                 float gscale, float* coef_scratch, int M, int C, int relu, int dtype, void* workspace,
                                 size_t ws_bytes, void* stream_) {
  int rc = l1bn_check("l1bn_bwd", M, C, dtype);
  if (rc) return rc;
  if (dz == nullptr || y == nullptr || stats == nullptr || dy == nullptr || coef_scratch == nullptr) {
    cn_set_error("l1bn_bwd: null operand");
    return CN_EINVAL;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const int CH = cn_dtype_chunk(dtype);
  BnMap m = bn_map(C / CH);
  const int nrb = bn_row_blocks(M, m, cn_get_option("bn_reduce_blocks", BN_REDUCE_BLOCKS));
  if (workspace == nullptr || ws_bytes < (size_t)nrb * 2 * C * sizeof(float)) {
    cn_set_error("l1bn_bwd: workspace too small");
    return CN_EWORKSPACE;
  }
  float* partial = (float*)workspace;
  dim3 grid((unsigned)nrb, (unsigned)m.gy);
  if (M <= L1BN_SMALL_M) {
    CN_DISPATCH_T(dtype, CN_LAUNCH(l1bn_small_bwd_kernel<TT>, dim3((unsigned)((C / CH + 255) / 256)), dim3(256), stream,
                                   (const char*)dz, (const char*)y, relu_mask, gamma, stats, (char*)dy, (char*)dres, dgamma,
                                   dbeta, beta_acc, gscale, M, C, relu));
    return cn_check_launch("l1bn_bwd");
  }
  CnMarkLast last;   // an armed completion mark goes on the apply kernel only
  BN_DISPATCH_PLAIN(l1bn_bwd_reduce_kernel, dtype, grid, stream, (const char*)dz, (const char*)y, relu_mask, stats, partial, M, C, relu, m.tpr_log2);
  CN_LAUNCH(l1bn_bwd_finalize_kernel, dim3((unsigned)((C + BN_FC - 1) / BN_FC)), dim3(256), stream, (const float*)partial,
            nrb, M, C, gamma, stats, dgamma, dbeta, beta_acc, gscale, coef_scratch);
  const int nab = bn_row_blocks(M, m, cn_get_option("bn_apply_blocks", BN_APPLY_BLOCKS));
  dim3 agrid((unsigned)nab, (unsigned)m.gy);
  last.release();
  BN_DISPATCH(l1bn_bwd_apply_kernel, dtype, bn_nt_flag(M, C, dtype), agrid, stream, (const char*)dz, (const char*)y, relu_mask, stats, (const float*)coef_scratch, (char*)dy, (char*)dres, M, C, relu, m.tpr_log2);
  return cn_check_launch("l1bn_bwd");
}
