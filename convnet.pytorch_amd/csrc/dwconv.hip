// dwconv.hip -- depthwise 3x3 convolution (stride 1 or 2, padding 1): the first half of a MobileNet block
// (the reference's models/mobilenet.py: nn.Conv2d(C, C, 3, stride, padding=1, groups=C), bias included).  Forward, data
// gradient and weight + bias gradient, NHWC activations, fp32 / bf16 / f16 storage with fp32 accumulation.
//
// 9 multiply-adds per element: the layer is pure streaming and runs on the VALU (gconv.hip serves one channel per group
// as a 32-row block-diagonal MFMA product, 32x the useful matrix work).  A lane owns one 16-byte channel chunk (8 16-bit
// or 4 fp32 channels); the compute-dtype filter copy is TAP-MAJOR [3][3][C], so one 16-byte load gives a tap for the
// lane's channels.
//   * fwd / dgrad (dwconv_kernel): blockIdx.y walks image rows (n, output row), blockIdx.x * 256 + tid the (run, chunk)
//     pairs of one row; a lane produces a run of DW_RUN output pixels along W: per source row it loads the
//     (DW_RUN - 1) * stride + 3 columns the run touches once and slides the 3-tap window over them in registers, so an
//     input element is requested 3 times (once per filter row; the re-reads of the rows hit L1 / L2), not 9 times.
//     Stride-1 data gradient: the same pass with the flipped filter.  Stride-2 data gradient: the gather form, source
//     ((h + 1 - r) / 2, (w + 1 - s) / 2) where divisible, else zero - rows by a block-uniform test, columns resolved at
//     compile time (a run starts at an even w).  No atomics, no scatter.
//   * wgrad (dwconv_dw_kernel): per channel the 9 tap sums of dy * x[src] and the sum of dy.  A workgroup owns a slab
//     of DW_SLAB_ROWS (or more) output rows and 1 << cxs channel chunks; its pixel lanes walk the slab's runs, the
//     lanes' sums are added through LDS in lane order and go to the fp32 workspace [split][C][9] (+ [split][C] for the
//     bias); wgrad_reduce_kernel adds the slabs in a fixed order (deterministic).
#include "cn_common.h"
#include "cn_api_internal.h"

#define DW_RUN 4          /* output pixels per lane along W (even: a stride-2 data-gradient run starts at an even w) */
#define DW_SLAB_ROWS 16   /* least output rows per weight-gradient slab */

// MODE 0: forward (stride ST) or, with flip, the stride-1 data gradient; MODE 1: stride-2 data gradient (gather).
template <typename T, int ST, int MODE>
__global__ __launch_bounds__(256) void dwconv_kernel(const char* src, const char* w, const float* bias, char* out,
                                                    int rows, int Ho, int Wo, int Hs, int Ws, int C, int nruns, int flip,
                                                    FastDiv div_cpr, FastDiv div_ho) {
  constexpr int CH = ElemTraits<T>::kChunk;
  constexpr int EB = ElemTraits<T>::kBytes;
  constexpr int NCOL = MODE == 1 ? DW_RUN / 2 + 1 : (DW_RUN - 1) * ST + 3;
  const int cpr = C / CH;
  const int idr = blockIdx.x * 256 + threadIdx.x;
  if (idr >= nruns * cpr) return;
  const int run = (int)cn_fastdiv((unsigned)idr, div_cpr);
  const int col = idr - run * cpr;
  const int q0 = run * DW_RUN;
  const int xb = MODE == 1 ? q0 / 2 : q0 * ST - 1;      // first source column of the run
  u32x4 wq[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wq[t] = cn_ld16(w + ((size_t)(flip ? 8 - t : t) * C + (size_t)col * CH) * EB);
  float bv[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) bv[e] = bias != nullptr ? bias[col * CH + e] : 0.f;
  int sxc[NCOL];
  bool cok[NCOL];
#pragma unroll
  for (int j = 0; j < NCOL; ++j) {
    cok[j] = (unsigned)(xb + j) < (unsigned)Ws;
    sxc[j] = cok[j] ? xb + j : 0;
  }
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int n = (int)cn_fastdiv((unsigned)row, div_ho);
    const int p = row - n * Ho;
    float acc[DW_RUN][CH];
#pragma unroll
    for (int i = 0; i < DW_RUN; ++i)
#pragma unroll
      for (int e = 0; e < CH; ++e) acc[i][e] = bv[e];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      int sy;
      bool rok;
      if (MODE == 1) {
        const int ty = p + 1 - r;
        sy = ty >> 1;
        rok = ty >= 0 && (ty & 1) == 0 && sy < Hs;
      } else {
        sy = p * ST - 1 + r;
        rok = (unsigned)sy < (unsigned)Hs;
      }
      if (!rok) continue;     // the same for every lane of the workgroup
      const char* rp = src + ((size_t)(n * Hs + sy) * Ws * C + (size_t)col * CH) * EB;
      u32x4 raw[NCOL];
#pragma unroll
      for (int j = 0; j < NCOL; ++j) raw[j] = cn_ld16(rp + (size_t)sxc[j] * C * EB);
      float wf[3][CH];
#pragma unroll
      for (int s = 0; s < 3; ++s) Chunk<T>::unpack(wq[r * 3 + s], wf[s]);
#pragma unroll
      for (int j = 0; j < NCOL; ++j) {
        float xf[CH];
        Chunk<T>::unpack(raw[j], xf);
        if (!cok[j]) {
#pragma unroll
          for (int e = 0; e < CH; ++e) xf[e] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < DW_RUN; ++i) {
          // the tap of output i that reads source column j: forward j = i*ST + s; gather 2*j = i + 1 - s
          const int s = MODE == 1 ? i + 1 - 2 * j : j - i * ST;
          if (s < 0 || s > 2) continue;
#pragma unroll
          for (int e = 0; e < CH; ++e) acc[i][e] = fmaf(wf[s][e], xf[e], acc[i][e]);
        }
      }
    }
    char* op = out + (((size_t)row * Wo + q0) * C + (size_t)col * CH) * EB;
#pragma unroll
    for (int i = 0; i < DW_RUN; ++i)
      if (q0 + i < Wo) cn_st16(op + (size_t)i * C * EB, Chunk<T>::pack(acc[i]));
  }
}

// part[split][C][9] (+ [split][C] behind it): tap sums of dy * x[src] and the sum of dy over the slab's pixels.
template <typename T, int ST>
__global__ __launch_bounds__(256) void dwconv_dw_kernel(const char* x, const char* dy, float* part, int NP, int P, int Q,
                                                       int H, int W, int C, int nruns, int cxs, int rows_per,
                                                       FastDiv div_nruns, FastDiv div_p) {
  constexpr int CH = ElemTraits<T>::kChunk;
  constexpr int EB = ElemTraits<T>::kBytes;
  constexpr int NCOL = (DW_RUN - 1) * ST + 3;
  __shared__ float red[256 * CH];
  const int cpr = C / CH;
  const int CX = 1 << cxs, PL = 256 >> cxs;
  const int cx = threadIdx.x & (CX - 1), pl = threadIdx.x >> cxs;
  const int colr = blockIdx.x * CX + cx;
  const int col = colr < cpr ? colr : 0;      // lanes past the last chunk compute chunk 0 and are not written
  const int row0 = blockIdx.y * rows_per;
  const int row1 = row0 + rows_per < NP ? row0 + rows_per : NP;
  const int units = (row1 - row0) * nruns;
  float acc[9][CH], accb[CH];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < CH; ++e) acc[t][e] = 0.f;
#pragma unroll
  for (int e = 0; e < CH; ++e) accb[e] = 0.f;
  for (int u = pl; u < units; u += PL) {
    const int rl = (int)cn_fastdiv((unsigned)u, div_nruns);
    const int run = u - rl * nruns;
    const int row = row0 + rl;
    const int n = (int)cn_fastdiv((unsigned)row, div_p);
    const int p = row - n * P;
    const int q0 = run * DW_RUN;
    float g[DW_RUN][CH];
    const char* gp = dy + (((size_t)row * Q + q0) * C + (size_t)col * CH) * EB;
#pragma unroll
    for (int i = 0; i < DW_RUN; ++i) {
      const bool ok = q0 + i < Q;
      Chunk<T>::unpack(cn_ld16(gp + (size_t)(ok ? i : 0) * C * EB), g[i]);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        g[i][e] = ok ? g[i][e] : 0.f;
        accb[e] += g[i][e];
      }
    }
    const int xb = q0 * ST - 1;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int sy = p * ST - 1 + r;
      if ((unsigned)sy >= (unsigned)H) continue;
      const char* rp = x + ((size_t)(n * H + sy) * W * C + (size_t)col * CH) * EB;
      u32x4 raw[NCOL];
      bool cok[NCOL];
#pragma unroll
      for (int j = 0; j < NCOL; ++j) {
        cok[j] = (unsigned)(xb + j) < (unsigned)W;
        raw[j] = cn_ld16(rp + (size_t)(cok[j] ? xb + j : 0) * C * EB);
      }
#pragma unroll
      for (int j = 0; j < NCOL; ++j) {
        float xf[CH];
        Chunk<T>::unpack(raw[j], xf);
        if (!cok[j]) {
#pragma unroll
          for (int e = 0; e < CH; ++e) xf[e] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < DW_RUN; ++i) {
          const int s = j - i * ST;
          if (s < 0 || s > 2) continue;
#pragma unroll
          for (int e = 0; e < CH; ++e) acc[r * 3 + s][e] = fmaf(g[i][e], xf[e], acc[r * 3 + s][e]);
        }
      }
    }
  }
  // the pixel lanes' sums, added in lane order; tap 9 is the bias gradient
  float* pw = part + (size_t)blockIdx.y * C * 9;
  float* pb = part + (size_t)gridDim.y * C * 9 + (size_t)blockIdx.y * C;
#pragma unroll
  for (int t = 0; t < 10; ++t) {
#pragma unroll
    for (int e = 0; e < CH; ++e) red[threadIdx.x * CH + e] = t < 9 ? acc[t < 9 ? t : 0][e] : accb[e];
    __syncthreads();
    for (int o = threadIdx.x; o < CX * CH; o += 256) {
      const int ocx = o / CH, e = o - ocx * CH;
      const int c = (blockIdx.x * CX + ocx) * CH + e;
      float s = 0.f;
      for (int j = 0; j < PL; ++j) s += red[((j << cxs) + ocx) * CH + e];
      if (c < C) {
        if (t < 9) pw[(size_t)c * 9 + t] = s;
        else pb[c] = s;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ host side
extern "C" int cn_dwconv3x3_ok(int C, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int dtype) {
  if (!cn_dtype_ok(dtype) || C < 1) return 0;
  if (R != 3 || S != 3 || pad_h != 1 || pad_w != 1 || stride_h != stride_w || (stride_h != 1 && stride_h != 2)) return 0;
  return C % cn_dtype_chunk(dtype) == 0 ? 1 : 0;
}

static int dw_check(const char* who, int N, int H, int W, int C, int stride, int dtype) {
  if (!cn_dwconv3x3_ok(C, 3, 3, stride, stride, 1, 1, dtype) || N <= 0 || H <= 0 || W <= 0) {
    cn_set_error("%s: unsupported depthwise convolution (N=%d H=%d W=%d C=%d stride=%d dtype=%d): needs a 3x3 filter, "
                 "stride 1 or 2, padding 1, C a multiple of the dtype's chunk", who, N, H, W, C, stride, dtype);
    return CN_ESHAPE;
  }
  if ((long long)N * H * W * C >= (1ll << 40) || (long long)N * H >= (1ll << 30) || (long long)W * C >= (1ll << 30)) {
    cn_set_error("%s: tensor too large", who);
    return CN_ESHAPE;
  }
  return CN_OK;
}

// out[N][Ho][Wo][C] from src[N][Hs][Ws][C]; mode 0 forward / flipped stride-1 data gradient, mode 1 stride-2 gather
static int dw_run(const char* who, const void* src, const void* w, const float* bias, void* out, int N, int Ho, int Wo,
                  int Hs, int Ws, int C, int stride, int mode, int flip, int dtype, void* stream) {
  const int cpr = C / cn_dtype_chunk(dtype);
  const int nruns = (Wo + DW_RUN - 1) / DW_RUN;
  const int rows = N * Ho;
  const unsigned gx = (unsigned)(((long long)nruns * cpr + 255) / 256);
  int gy = cn_get_option("dwconv_wgs", 8192) / (int)gx;
  if (gy < 1) gy = 1;
  if (gy > rows) gy = rows;
  if (gy > 65535) gy = 65535;
  const dim3 grid(gx, (unsigned)gy);
  const FastDiv div_cpr = cn_make_fastdiv((unsigned)cpr), div_ho = cn_make_fastdiv((unsigned)Ho);
  const hipStream_t st = (hipStream_t)stream;
  const char* tn = dtype == CN_BF16 ? "bf16_t" : dtype == CN_F16 ? "f16_t" : "float";
  cn_set_last_kernel("dwconv_kernel<%s, %d, %d>%s", tn, mode ? 2 : stride, mode, mode || flip ? " [dgrad]" : "");
#define DW_GO(ST, MODE)                                                                                             \
  CN_DISPATCH_T(dtype, CN_LAUNCH((dwconv_kernel<TT, ST, MODE>), grid, dim3(256), st, (const char*)src, (const char*)w, \
                                 bias, (char*)out, rows, Ho, Wo, Hs, Ws, C, nruns, flip, div_cpr, div_ho))
  if (mode) DW_GO(2, 1);
  else if (stride == 2) DW_GO(2, 0);
  else DW_GO(1, 0);
#undef DW_GO
  return cn_check_launch(who);
}

extern "C" cn_status cn_dwconv3x3_fwd(const void* x, const void* w_rsc, const float* bias, void* y, int N, int H, int W,
                                      int C, int stride, int dtype, void* stream) {
  if (x == nullptr || w_rsc == nullptr || y == nullptr) { cn_set_error("dwconv3x3_fwd: null operand"); return CN_EINVAL; }
  const int rc = dw_check("dwconv3x3_fwd", N, H, W, C, stride, dtype);
  if (rc != CN_OK) return rc;
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  return dw_run("dwconv3x3_fwd", x, w_rsc, bias, y, N, P, Q, H, W, C, stride, 0, 0, dtype, stream);
}

extern "C" cn_status cn_dwconv3x3_dgrad(const void* dy, const void* w_rsc, void* dx, int N, int H, int W, int C, int stride,
                                        int dtype, void* stream) {
  if (dy == nullptr || w_rsc == nullptr || dx == nullptr) { cn_set_error("dwconv3x3_dgrad: null operand"); return CN_EINVAL; }
  const int rc = dw_check("dwconv3x3_dgrad", N, H, W, C, stride, dtype);
  if (rc != CN_OK) return rc;
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  if (stride == 1) return dw_run("dwconv3x3_dgrad", dy, w_rsc, nullptr, dx, N, H, W, P, Q, C, 1, 0, 1, dtype, stream);
  return dw_run("dwconv3x3_dgrad", dy, w_rsc, nullptr, dx, N, H, W, P, Q, C, 2, 1, 0, dtype, stream);
}

struct DwwPlan { int cxs, nbx, rows_per, nsplit, nruns; };
static DwwPlan dww_plan(int N, int H, int W, int C, int stride, int dtype) {
  DwwPlan d;
  const int cpr = C / cn_dtype_chunk(dtype);
  d.cxs = 0;
  while ((1 << d.cxs) < cpr && d.cxs < 6) ++d.cxs;       // chunks per workgroup: the power of two >= cpr, 64 at most
  d.nbx = (cpr + (1 << d.cxs) - 1) >> d.cxs;
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  const long long NP = (long long)N * P;
  int maxsplit = cn_get_option("dwconv_wgs", 8192) / 4 / d.nbx;
  if (maxsplit < 1) maxsplit = 1;
  long long rp = (NP + maxsplit - 1) / maxsplit;
  if (rp < DW_SLAB_ROWS) rp = DW_SLAB_ROWS;
  d.rows_per = (int)rp;
  d.nsplit = (int)((NP + rp - 1) / rp);
  d.nruns = (Q + DW_RUN - 1) / DW_RUN;
  return d;
}

extern "C" size_t cn_dwconv3x3_wgrad_workspace(int N, int H, int W, int C, int stride, int dtype) {
  if (!cn_dwconv3x3_ok(C, 3, 3, stride, stride, 1, 1, dtype) || N <= 0 || H <= 0 || W <= 0) return 0;
  const DwwPlan d = dww_plan(N, H, W, C, stride, dtype);
  return (size_t)d.nsplit * C * 10 * sizeof(float);
}

extern "C" cn_status cn_dwconv3x3_wgrad(const void* x, const void* dy, float* dw, float* dbias, int N, int H, int W, int C,
                                        int stride, int dtype, float beta, float scale, void* workspace, size_t ws_bytes,
                                        void* stream) {
  if (x == nullptr || dy == nullptr || dw == nullptr) { cn_set_error("dwconv3x3_wgrad: null operand"); return CN_EINVAL; }
  const int rc = dw_check("dwconv3x3_wgrad", N, H, W, C, stride, dtype);
  if (rc != CN_OK) return rc;
  const size_t need = cn_dwconv3x3_wgrad_workspace(N, H, W, C, stride, dtype);
  if (workspace == nullptr || ws_bytes < need) {
    cn_set_error("dwconv3x3_wgrad: workspace of %zu bytes < %zu", ws_bytes, need);
    return CN_EWORKSPACE;
  }
  const DwwPlan d = dww_plan(N, H, W, C, stride, dtype);
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  if ((long long)d.rows_per * d.nruns >= (1ll << 31)) { cn_set_error("dwconv3x3_wgrad: tensor too large"); return CN_ESHAPE; }
  const dim3 grid((unsigned)d.nbx, (unsigned)d.nsplit);
  const FastDiv div_nruns = cn_make_fastdiv((unsigned)d.nruns), div_p = cn_make_fastdiv((unsigned)P);
  const hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  CnMarkLast mark;
  cn_set_last_kernel("dwconv_dw_kernel<%s, %d>", dtype == CN_BF16 ? "bf16_t" : dtype == CN_F16 ? "f16_t" : "float", stride);
#define DWW_GO(ST)                                                                                                   \
  CN_DISPATCH_T(dtype, CN_LAUNCH((dwconv_dw_kernel<TT, ST>), grid, dim3(256), st, (const char*)x, (const char*)dy, part, \
                                 N * P, P, Q, H, W, C, d.nruns, d.cxs, d.rows_per, div_nruns, div_p))
  if (stride == 2) DWW_GO(2);
  else DWW_GO(1);
#undef DWW_GO
  int rc2 = cn_check_launch("dwconv3x3_wgrad");
  if (rc2 != CN_OK) return rc2;
  if (dbias != nullptr) {
    rc2 = wg_launch_reduce(st, part + (size_t)d.nsplit * C * 9, dbias, d.nsplit, C, 1, 1, 1, beta, scale);
    if (rc2 != CN_OK) return rc2;
  }
  mark.release();
  return wg_launch_reduce(st, part, dw, d.nsplit, C, 9, 1, 1, beta, scale);
}
