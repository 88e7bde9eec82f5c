// se.hip -- squeeze-and-excitation gate on an NHWC activation (training + inference), gfx950.
//
// Replaces the reference's SEBlock (models/modules/se.py:6-25 there), which resnet_se puts on the SHORTCUT of every
// residual block (models/resnet.py:112-113, 159-160), and its autograd backward.  For r[n][hw][c] (compute dtype T):
//   s[n][c]  = mean_hw r[n][hw][c]                                   (squeeze)
//   h[n][j]  = relu(W1[j][:] . s[n][:] + b1[j])      j < Cr          (excite: two tiny dense layers per sample,
//   m[n][c]  = sigmoid(W2[c][:] . h[n][:] + b2[c])                    fp32 master weights W1[Cr][C], W2[C][Cr])
//   rs       = round_T(r * m[n][c])                                  (scale)
// backward, with g = dL/drs:
//   dm[n][c] = sum_hw g*r        dz2 = dm*m*(1 - m)        dh = (W2^T dz2)*[h > 0]        ds = W1^T dh
//   dW2 = sum_n dz2 (x) h   db2 = sum_n dz2   dW1 = sum_n dh (x) s   db1 = sum_n dh       (dst = beta*dst + scale*sum)
//   dr  = round_T(g*m + ds/HW [+ addend])
// Everything of size N x C or N x Cr stays fp32.  The two activation-sized reductions (squeeze, dm) share one kernel: a
// lane owns one 16-byte channel chunk and walks over the pixels of one sample, a fixed tree through LDS joins the row
// lanes of a workgroup, partial rows + a fixed-order finalize launch join the pixel slices of a sample.  No atomics
// anywhere: every sum has one order, a run is bit-reproducible.
#include "cn_common.h"
#include "cn_api_internal.h"

#define SE_MAX_C 2048      /* s / dz2 of one sample sit in LDS in the excite kernels */
#define SE_MAX_CR 128
#define SE_MAX_SLICES 64
#define SE_TARGET_BLOCKS 1024

// ------------------------------------------------------------------------------------------------
// partial[slice][n][c] = scale * sum over the pixels of the slice of a (TWO: a*b).  Block = TC chunk columns x (256/TC) row
// lanes; grid = (column groups, slices, N).
template <typename T, bool TWO>
__global__ __launch_bounds__(256) void se_reduce_kernel(const char* a, const char* b, float* partial, int N, int HW, int C,
                                                        int tc_log2, int rows_per_slice, float scale) {
  constexpr int CH = ElemTraits<T>::kChunk;
  constexpr int EB = ElemTraits<T>::kBytes;
  __shared__ float red[256 * CH];
  const int tid = threadIdx.x;
  const int TC = 1 << tc_log2, RL = 256 >> tc_log2;
  const int cpr = C / CH;
  const int tcol = tid & (TC - 1), rl = tid >> tc_log2;
  const int col = blockIdx.x * TC + tcol;
  const int n = blockIdx.z;
  const int row0 = blockIdx.y * rows_per_slice;
  int row1 = row0 + rows_per_slice;
  if (row1 > HW) row1 = HW;
  float acc[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) acc[e] = 0.f;
  if (col < cpr) {
    const size_t cb = (size_t)col * CH * EB, rb = (size_t)C * EB;
    const size_t base = (size_t)n * HW * rb + cb;
    for (int row = row0 + rl; row < row1; row += RL) {
      float f[CH];
      Chunk<T>::unpack(cn_ld16(a + base + (size_t)row * rb), f);
      if (TWO) {
        float g[CH];
        Chunk<T>::unpack(cn_ld16(b + base + (size_t)row * rb), g);
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[e] = fmaf(f[e], g[e], acc[e]);
      } else {
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[e] += f[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < CH; ++e) red[tid * CH + e] = acc[e];
  for (int s = RL >> 1; s >= 1; s >>= 1) {      // fixed tree over the row lanes (tid = rl*TC + tcol)
    __syncthreads();
    if (rl < s) {
#pragma unroll
      for (int e = 0; e < CH; ++e) red[tid * CH + e] += red[(tid + s * TC) * CH + e];
    }
  }
  __syncthreads();
  if (rl == 0 && col < cpr) {
    float* dst = partial + ((size_t)blockIdx.y * N + n) * C + (size_t)col * CH;
#pragma unroll
    for (int e = 0; e < CH; ++e) dst[e] = red[tid * CH + e] * scale;
  }
}

// out[i] = scale * (partial[0][i] + partial[1][i] + ...), i < NC: the slices of a sample in their one order
__global__ __launch_bounds__(256) void se_finalize_kernel(const float* partial, float* out, int slices, int NC, float scale) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= NC) return;
  float acc = 0.f;
  for (int s = 0; s < slices; ++s) acc += partial[(size_t)s * NC + i];
  out[i] = acc * scale;
}

__device__ __forceinline__ float se_wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += cn_shfl_xor(v, d);
  return v;
}

// ------------------------------------------------------------------------------------------------
// One workgroup per sample.  h = relu(W1 s + b1): a wave per hidden unit, lanes along C.  m = sigmoid(W2 h + b2): a thread
// per channel walks its row of W2, h from LDS.  (Lanes along the hidden units with a shuffle reduction per row were measured
// 2.7x slower on the ResNet-50 shapes: one workgroup per CU, and the row loop becomes a chain of dependent shuffles.)
__global__ __launch_bounds__(256) void se_excite_fwd_kernel(const float* s, const float* w1, const float* b1, const float* w2,
                                                            const float* b2, float* h, float* m, int C, int Cr) {
  __shared__ float s_s[SE_MAX_C];
  __shared__ float s_h[SE_MAX_CR];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  for (int c = tid; c < C; c += 256) s_s[c] = s[(size_t)n * C + c];
  __syncthreads();
  for (int j = wave; j < Cr; j += 4) {     // (wave-uniform trip count: the shuffles below run with all 64 lanes)
    float acc = 0.f;
    for (int c = lane; c < C; c += 64) acc = fmaf(w1[(size_t)j * C + c], s_s[c], acc);
    acc = se_wave_sum(acc) + b1[j];
    acc = acc > 0.f ? acc : 0.f;
    if (lane == 0) { s_h[j] = acc; h[(size_t)n * Cr + j] = acc; }
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float acc = b2[c];
    for (int j = 0; j < Cr; ++j) acc = fmaf(w2[(size_t)c * Cr + j], s_h[j], acc);
    m[(size_t)n * C + c] = 1.f / (1.f + expf(-acc));
  }
}

// One workgroup per sample: dz2 = dm*m*(1 - m); dh = (W2^T dz2)*[h > 0]: 2^lpr_log2 lanes along the hidden units, the
// 256 >> lpr_log2 row groups split C and meet through a fixed tree in LDS; ds = W1^T dh: a thread per channel.
__global__ __launch_bounds__(256) void se_excite_bwd_kernel(const float* dm, const float* h, const float* m, const float* w1,
                                                            const float* w2, float* dz2, float* dh, float* ds, int C, int Cr,
                                                            int lpr_log2) {
  __shared__ float s_z[SE_MAX_C];
  __shared__ float s_p[512];               // [row group][hidden unit]: (256 >> lpr_log2) * Cr <= 512
  const int n = blockIdx.x, tid = threadIdx.x;
  for (int c = tid; c < C; c += 256) {
    const float mv = m[(size_t)n * C + c];
    const float z = dm[(size_t)n * C + c] * mv * (1.f - mv);
    s_z[c] = z;
    dz2[(size_t)n * C + c] = z;
  }
  __syncthreads();
  const int LPR = 1 << lpr_log2, R = 256 >> lpr_log2;
  const int jl = tid & (LPR - 1), rsub = tid >> lpr_log2;
  for (int j = jl; j < Cr; j += LPR) {     // (at most two trips: Cr <= 2 * LPR)
    float acc = 0.f;
    for (int c = rsub; c < C; c += R) acc = fmaf(w2[(size_t)c * Cr + j], s_z[c], acc);
    s_p[rsub * Cr + j] = acc;
  }
  for (int half = R >> 1; half >= 1; half >>= 1) {
    __syncthreads();
    for (int i = tid; i < half * Cr; i += 256) s_p[i] += s_p[i + half * Cr];
  }
  __syncthreads();
  for (int j = tid; j < Cr; j += 256) {
    const float v = h[(size_t)n * Cr + j] > 0.f ? s_p[j] : 0.f;
    s_p[j] = v;
    dh[(size_t)n * Cr + j] = v;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float acc = 0.f;
    for (int j = 0; j < Cr; ++j) acc = fmaf(w1[(size_t)j * C + c], s_p[j], acc);
    ds[(size_t)n * C + c] = acc;
  }
}

// Parameter gradients: a workgroup owns 4 channels c0..c0+3 and every hidden unit: 2^jp_log2 lanes along the hidden units,
// 256 >> jp_log2 groups split the samples and meet through a fixed tree in LDS.  Per thread:
//   dW2[c0+e][j] = sum_n dz2[n][c0+e]*h[n][j]      dW1[j][c0+e] = sum_n dh[n][j]*s[n][c0+e]
//   db2[c0+e]    = sum_n dz2[n][c0+e]  (lane j = 0)       db1[j] = sum_n dh[n][j]  (workgroup 0)
// dst = beta*dst + scale*sum.
#define SE_PG 13   /* floats a thread carries: 4 dW2 | 4 dW1 | 4 db2 | 1 db1 */
__global__ __launch_bounds__(256) void se_param_grad_kernel(const float* dz2, const float* dh, const float* s, const float* h,
                                                            float* dw1, float* db1, float* dw2, float* db2, float beta,
                                                            float scale, int N, int C, int Cr, int jp_log2) {
  __shared__ float red[256 * SE_PG];
  const int tid = threadIdx.x;
  const int JP = 1 << jp_log2, NG = 256 >> jp_log2;
  const int j = tid & (JP - 1), ng = tid >> jp_log2;
  const int c0 = blockIdx.x * 4;
  float acc[SE_PG];
#pragma unroll
  for (int e = 0; e < SE_PG; ++e) acc[e] = 0.f;
  if (j < Cr) {
    for (int n = ng; n < N; n += NG) {
      const float hv = h[(size_t)n * Cr + j], dhv = dh[(size_t)n * Cr + j];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float z = dz2[(size_t)n * C + c0 + e], sv = s[(size_t)n * C + c0 + e];
        acc[e] = fmaf(z, hv, acc[e]);
        acc[4 + e] = fmaf(dhv, sv, acc[4 + e]);
        acc[8 + e] += z;
      }
      acc[12] += dhv;
    }
  }
#pragma unroll
  for (int e = 0; e < SE_PG; ++e) red[tid * SE_PG + e] = acc[e];
  for (int half = NG >> 1; half >= 1; half >>= 1) {      // fixed tree over the sample groups (tid = ng*JP + j)
    __syncthreads();
    if (ng < half) {
#pragma unroll
      for (int e = 0; e < SE_PG; ++e) red[tid * SE_PG + e] += red[(tid + half * JP) * SE_PG + e];
    }
  }
  __syncthreads();
  if (ng != 0 || j >= Cr) return;
  const float* r = red + tid * SE_PG;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float* d2 = dw2 + (size_t)(c0 + e) * Cr + j;
    float* d1 = dw1 + (size_t)j * C + c0 + e;
    *d2 = (beta != 0.f ? beta * *d2 : 0.f) + scale * r[e];
    *d1 = (beta != 0.f ? beta * *d1 : 0.f) + scale * r[4 + e];
    if (j == 0) db2[c0 + e] = (beta != 0.f ? beta * db2[c0 + e] : 0.f) + scale * r[8 + e];
  }
  if (blockIdx.x == 0) db1[j] = (beta != 0.f ? beta * db1[j] : 0.f) + scale * r[12];
}

// ------------------------------------------------------------------------------------------------
// Streaming passes, one 16-byte chunk per lane per trip: out = x*m[n][c] (+ ds[n][c]*inv_hw) (+ addend)
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void se_scale_kernel(const char* x, const float* m, const float* ds, const char* addend,
                                                       char* out, long long total, int HW, int C, float inv_hw) {
  constexpr int CH = ElemTraits<T>::kChunk;
  constexpr int EB = ElemTraits<T>::kBytes;
  const int cpr = C / CH;
  const long long rowlen = (long long)HW * cpr;
  for (long long id = (long long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long long)gridDim.x * 256) {
    const int n = (int)(id / rowlen);
    const int col = (int)(id % cpr);
    const size_t gi = (size_t)n * C + (size_t)col * CH;
    float f[CH];
    Chunk<T>::unpack(cn_ld16_stream(x + (size_t)id * 16), f);
#pragma unroll
    for (int e = 0; e < CH; ++e) f[e] *= m[gi + e];
    if (BWD) {
#pragma unroll
      for (int e = 0; e < CH; ++e) f[e] = fmaf(ds[gi + e], inv_hw, f[e]);
      if (addend != nullptr) {
        float a[CH];
        Chunk<T>::unpack(cn_ld16_stream(addend + (size_t)id * 16), a);
#pragma unroll
        for (int e = 0; e < CH; ++e) f[e] += a[e];
      }
    }
    cn_st16_stream(out + (size_t)id * 16, Chunk<T>::pack(f));
  }
}

// ================================================================================================ host side
struct SeMap { int tc_log2, gx, slices, rows_per_slice; };

static SeMap se_map(int N, int HW, int C, int dtype) {
  const int cpr = C / cn_dtype_chunk(dtype);
  SeMap m;
  m.tc_log2 = 0;
  while ((1 << m.tc_log2) < cpr && m.tc_log2 < 6) ++m.tc_log2;
  const int TC = 1 << m.tc_log2, RL = 256 >> m.tc_log2;
  m.gx = (cpr + TC - 1) / TC;
  // enough workgroups to fill the machine, at least four trips of the row lanes per slice
  long long want = (SE_TARGET_BLOCKS + (long long)m.gx * N - 1) / ((long long)m.gx * N);
  long long cap = HW / (4 * RL);
  if (want > cap) want = cap;
  if (want > SE_MAX_SLICES) want = SE_MAX_SLICES;
  if (want < 1) want = 1;
  m.rows_per_slice = (int)((HW + want - 1) / want);
  m.slices = (HW + m.rows_per_slice - 1) / m.rows_per_slice;
  return m;
}

static int se_check(const char* who, int N, int HW, int C, int dtype) {
  if (!cn_dtype_ok(dtype)) { cn_set_error("%s: bad dtype %d", who, dtype); return CN_EINVAL; }
  const int CH = cn_dtype_chunk(dtype);
  if (N <= 0 || N > 65535 || HW <= 0 || HW > (1 << 24) || C <= 0 || C % CH != 0 || C > SE_MAX_C) {
    cn_set_error("%s: need 0 < N <= 65535, 0 < HW <= 2^24 and C (%d) a multiple of %d up to %d", who, C, CH, SE_MAX_C);
    return CN_ESHAPE;
  }
  return CN_OK;
}

// lanes that share a row of hidden units: the smallest power of two >= Cr, at most 2^cap
static int se_lanes_log2(int Cr, int cap) {
  int l = 0;
  while ((1 << l) < Cr && l < cap) ++l;
  return l;
}

static int se_check_dense(const char* who, int N, int C, int Cr) {
  if (N <= 0 || N > (1 << 20) || C <= 0 || C > SE_MAX_C || C % 4 != 0 || Cr <= 0 || Cr > SE_MAX_CR) {
    cn_set_error("%s: need 0 < N <= 2^20, C (%d) a multiple of 4 up to %d and 0 < hidden width (%d) <= %d", who, C, SE_MAX_C, Cr,
                 SE_MAX_CR);
    return CN_ESHAPE;
  }
  return CN_OK;
}

static unsigned se_stream_grid(long long total) {
  long long b = (total + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

// bytes of scratch: the partial rows of a reduction (cn_se_squeeze, cn_se_scale_bwd_reduce), dz2 + dh (cn_se_excite_bwd)
extern "C" size_t cn_se_workspace(int N, int HW, int C, int Cr, int dtype) {
  if (!cn_dtype_ok(dtype) || N <= 0 || HW <= 0 || C <= 0 || C % cn_dtype_chunk(dtype) != 0 || Cr < 0) return 0;
  const SeMap m = se_map(N, HW, C, dtype);
  size_t a = (size_t)m.slices * N * C, b = (size_t)N * ((size_t)C + Cr);
  return (a > b ? a : b) * sizeof(float);
}

template <bool TWO>
static int se_reduce(const char* who, const void* a, const void* b, float* out, int N, int HW, int C, int dtype, float scale,
                     void* workspace, size_t ws_bytes, hipStream_t stream) {
  const SeMap m = se_map(N, HW, C, dtype);
  float* partial = out;
  if (m.slices > 1) {
    if (workspace == nullptr || ws_bytes < (size_t)m.slices * N * C * sizeof(float)) {
      cn_set_error("%s: workspace too small", who);
      return CN_EWORKSPACE;
    }
    partial = (float*)workspace;
  }
  CnMarkLast last;
  if (m.slices == 1) last.release();
  dim3 grid((unsigned)m.gx, (unsigned)m.slices, (unsigned)N);
  CN_DISPATCH_T(dtype, CN_LAUNCH((se_reduce_kernel<TT, TWO>), grid, dim3(256), stream, (const char*)a, (const char*)b, partial,
                                 N, HW, C, m.tc_log2, m.rows_per_slice, m.slices == 1 ? scale : 1.f));
  if (m.slices > 1) {
    last.release();
    CN_LAUNCH(se_finalize_kernel, dim3((unsigned)((N * C + 255) / 256)), dim3(256), stream, (const float*)partial, out,
              m.slices, N * C, scale);
  }
  return cn_check_launch(who);
}

extern "C" cn_status cn_se_squeeze(const void* r, float* s, int N, int HW, int C, int dtype, void* workspace, size_t ws_bytes,
                                   void* stream) {
  int rc = se_check("se_squeeze", N, HW, C, dtype);
  if (rc) return rc;
  if (r == nullptr || s == nullptr) { cn_set_error("se_squeeze: null operand"); return CN_EINVAL; }
  return se_reduce<false>("se_squeeze", r, nullptr, s, N, HW, C, dtype, 1.f / (float)HW, workspace, ws_bytes,
                          (hipStream_t)stream);
}

extern "C" cn_status cn_se_excite_fwd(const float* s, const float* w1, const float* b1, const float* w2, const float* b2,
                                      float* h, float* m, int N, int C, int Cr, void* stream) {
  int rc = se_check_dense("se_excite_fwd", N, C, Cr);
  if (rc) return rc;
  if (s == nullptr || w1 == nullptr || b1 == nullptr || w2 == nullptr || b2 == nullptr || h == nullptr || m == nullptr) {
    cn_set_error("se_excite_fwd: null operand");
    return CN_EINVAL;
  }
  CN_LAUNCH(se_excite_fwd_kernel, dim3((unsigned)N), dim3(256), (hipStream_t)stream, s, w1, b1, w2, b2, h, m, C, Cr);
  return cn_check_launch("se_excite_fwd");
}

extern "C" cn_status cn_se_scale_fwd(const void* r, const float* m, void* rs, int N, int HW, int C, int dtype, void* stream) {
  int rc = se_check("se_scale_fwd", N, HW, C, dtype);
  if (rc) return rc;
  if (r == nullptr || m == nullptr || rs == nullptr) { cn_set_error("se_scale_fwd: null operand"); return CN_EINVAL; }
  const long long total = (long long)N * HW * (C / cn_dtype_chunk(dtype));
  CN_DISPATCH_T(dtype, CN_LAUNCH((se_scale_kernel<TT, false>), dim3(se_stream_grid(total)), dim3(256), (hipStream_t)stream,
                                 (const char*)r, m, (const float*)nullptr, (const char*)nullptr, (char*)rs, total, HW, C, 0.f));
  return cn_check_launch("se_scale_fwd");
}

extern "C" cn_status cn_se_scale_bwd_reduce(const void* g, const void* r, float* dm, int N, int HW, int C, int dtype,
                                            void* workspace, size_t ws_bytes, void* stream) {
  int rc = se_check("se_scale_bwd_reduce", N, HW, C, dtype);
  if (rc) return rc;
  if (g == nullptr || r == nullptr || dm == nullptr) { cn_set_error("se_scale_bwd_reduce: null operand"); return CN_EINVAL; }
  return se_reduce<true>("se_scale_bwd_reduce", g, r, dm, N, HW, C, dtype, 1.f, workspace, ws_bytes, (hipStream_t)stream);
}

extern "C" cn_status cn_se_excite_bwd(const float* dm, const float* s, const float* h, const float* m, const float* w1,
                                      const float* w2, float* ds, float* dw1, float* db1, float* dw2, float* db2, float beta,
                                      float scale, int N, int C, int Cr, void* workspace, size_t ws_bytes, void* stream_) {
  int rc = se_check_dense("se_excite_bwd", N, C, Cr);
  if (rc) return rc;
  if (dm == nullptr || s == nullptr || h == nullptr || m == nullptr || w1 == nullptr || w2 == nullptr || ds == nullptr ||
      dw1 == nullptr || db1 == nullptr || dw2 == nullptr || db2 == nullptr) {
    cn_set_error("se_excite_bwd: null operand");
    return CN_EINVAL;
  }
  if (workspace == nullptr || ws_bytes < (size_t)N * ((size_t)C + Cr) * sizeof(float)) {
    cn_set_error("se_excite_bwd: workspace too small");
    return CN_EWORKSPACE;
  }
  hipStream_t stream = (hipStream_t)stream_;
  float* dz2 = (float*)workspace;
  float* dh = dz2 + (size_t)N * C;
  CnMarkLast last;
  CN_LAUNCH(se_excite_bwd_kernel, dim3((unsigned)N), dim3(256), stream, dm, h, m, w1, w2, dz2, dh, ds, C, Cr,
            se_lanes_log2(Cr, 6));
  last.release();
  CN_LAUNCH(se_param_grad_kernel, dim3((unsigned)(C / 4)), dim3(256), stream, (const float*)dz2, (const float*)dh, s, h, dw1,
            db1, dw2, db2, beta, scale, N, C, Cr, se_lanes_log2(Cr, 7));
  return cn_check_launch("se_excite_bwd");
}

extern "C" cn_status cn_se_scale_bwd_apply(const void* g, const float* m, const float* ds, const void* addend, void* dr, int N,
                                           int HW, int C, int dtype, void* stream) {
  int rc = se_check("se_scale_bwd_apply", N, HW, C, dtype);
  if (rc) return rc;
  if (g == nullptr || m == nullptr || ds == nullptr || dr == nullptr) {
    cn_set_error("se_scale_bwd_apply: null operand");
    return CN_EINVAL;
  }
  const long long total = (long long)N * HW * (C / cn_dtype_chunk(dtype));
  CN_DISPATCH_T(dtype, CN_LAUNCH((se_scale_kernel<TT, true>), dim3(se_stream_grid(total)), dim3(256), (hipStream_t)stream,
                                 (const char*)g, m, ds, (const char*)addend, (char*)dr, total, HW, C, 1.f / (float)HW));
  return cn_check_launch("se_scale_bwd_apply");
}
