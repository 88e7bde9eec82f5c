// gconv.hip -- grouped 3x3 convolution (stride 1 or 2, padding 1): the conv3x3 of a ResNeXt block
// (/root/reference models/resnet.py:75-78 with groups > 1; models/resnext.py).  Forward, data gradient and weight
// gradient, NHWC activations, filters [K][3][3][C/g] (the arena's KRSC order with C/g input channels per filter).
//
// A grouped layer has too little reduction per output (9 * C/g) for the dense tile kernels and is bound by HBM, so the
// per-group GEMMs run on the matrix cores as BLOCK-DIAGONAL products: a channel block packs GB consecutive groups into
// one 32-row MFMA operand (GB * rows-per-group <= 32 rows, GB * reduction-per-group <= 64 reduction channels) whose
// off-diagonal entries are zero.  The MFMA work is 32 / (C/g) times the useful work at C/g = K/g (8x at ResNeXt's
// 32x4d first stage), which the matrix cores absorb: the layer stays HBM / L2 bound.
//   * fwd / dgrad (gconv_kernel): a workgroup stages its channel block's zero-expanded filter [32][9][<= 64] in LDS once
//     and its four waves walk tiles of 32 output pixels; per tap each lane loads its pixel fragment (8 reduction channels
//     of one source pixel, 16 bytes) straight from global memory (the 3x3 re-reads hit L1 / L2) and the A fragment out of
//     LDS.  The data gradient is the same kernel with the roles of C and K swapped: the source pixel of tap (r, s) for
//     input pixel (h, w) is ((h + 1 - r) / stride, (w + 1 - s) / stride) when divisible, else the fragment is zero.
//   * wgrad (gconv_dw_kernel): dW[k][tap][c] = sum over pixels of dy[m][k] * x[src(m, tap)][c]: rows = the channel
//     block's output channels, columns = (tap, reduction channel) in tiles of 32, reduction = 16 pixels per MFMA.  The
//     pixels are split over workgroups; per-workgroup partials go to the fp32 workspace [split][K][9][C/g] and
//     wgrad_reduce_kernel sums them in a fixed order (deterministic, no atomics).
// fp32 storage runs the same mapping on the 32x32x2 f32 MFMA.
#include "cn_common.h"
#include "cn_api_internal.h"
#include <type_traits>

#define GC_MAXRED 64    /* reduction channels per channel block */
#define GC_WAVES 4

// Channel-block geometry of one product: Rg rows (output channels of the product) and Dg reduction channels per group.
struct GcGeom {
  int G, Rg, Dg;   // groups, rows / reduction channels per group
  int GB;          // groups per block (1 when a group is split into two row blocks)
  int nsub;        // row blocks per group (2 when Rg > 32)
  int nblocks;
  int redp;        // reduction channels per block rounded up to the MFMA step
};

static GcGeom gc_geom(int G, int Rg, int Dg, int step) {
  GcGeom g;
  g.G = G; g.Rg = Rg; g.Dg = Dg;
  if (Rg <= 32) {
    int gb = 32 / Rg;
    if (gb > GC_MAXRED / Dg) gb = GC_MAXRED / Dg;
    if (gb > G) gb = G;
    g.GB = gb; g.nsub = 1;
    g.nblocks = (G + gb - 1) / gb;
  } else {
    g.GB = 1; g.nsub = 2;
    g.nblocks = 2 * G;
  }
  const int nred = g.GB * Dg;
  g.redp = (nred + step - 1) / step * step;
  return g;
}

// the block's rows [row0, row0 + nrows) and reduction channels [red0, red0 + nred)
struct GcBlock { int row0, nrows, red0, nred; };
__host__ __device__ __forceinline__ GcBlock gc_block(int b, int G, int Rg, int Dg, int GB, int nsub) {
  GcBlock k;
  if (nsub == 1) {
    const int g0 = b * GB;
    const int ng = G - g0 < GB ? G - g0 : GB;
    k.row0 = g0 * Rg; k.nrows = ng * Rg; k.red0 = g0 * Dg; k.nred = ng * Dg;
  } else {
    const int g = b >> 1, sub = b & 1;
    k.row0 = g * Rg + 32 * sub;
    k.nrows = Rg - 32 * sub < 32 ? Rg - 32 * sub : 32;
    k.red0 = g * Dg; k.nred = Dg;
  }
  return k;
}

struct GcParams {
  const char* src;    // [N][Hs][Ws][Csrc]: x (forward) or dy (data gradient)
  const char* w;      // [K][9][Cg] compute dtype
  char* out;          // [N][Ho][Wo][Cout]
  int N, Hs, Ws, Csrc, Ho, Wo, Cout, Cg;
  int G, Rg, Dg, GB, nsub, redp;
  int stride, dgrad;
  int M, ntiles;
  FastDiv div_wo, div_ho;
};

// zero-expanded filter of the block in LDS: [32 rows][9 taps][redp] (+16 bytes of row padding)
template <typename T>
__device__ __forceinline__ void gc_stage_filter(char* lds, int pitch, const char* w, const GcBlock& k, int Rg, int Dg,
                                                int Cg, int nsub, int redp, int dgrad) {
  const int total = 32 * 9 * redp;
  for (int id = threadIdx.x; id < total; id += 256) {
    const int i = id / (9 * redp), rem = id - i * (9 * redp);
    const int tap = rem / redp, cc = rem - tap * redp;
    float v = 0.f;
    if (i < k.nrows && cc < k.nred) {
      const int gi = nsub == 1 ? i / Rg : 0, gc = nsub == 1 ? cc / Dg : 0;
      if (gi == gc) {
        const int row = k.row0 + i, red = k.red0 + cc;
        const int g = row / Rg;
        // forward: w[row][tap][red - g*Dg]; data gradient: w[red][tap][row - g*Rg]
        const size_t idx = dgrad ? ((size_t)red * 9 + tap) * Cg + (row - g * Rg)
                                 : ((size_t)row * 9 + tap) * Cg + (red - g * Dg);
        v = cn_load_elem<T>((const T*)w + idx);
      }
    }
    cn_store_elem<T>((T*)(lds + i * pitch + (tap * redp + cc) * (int)sizeof(T)), v);
  }
}

// VEC (16-bit storage): every block's reduction range is whole 8-channel chunks -> one 16-byte load per fragment
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void gconv_kernel(GcParams p) {
  constexpr bool F32 = std::is_same<T, float>::value;
  constexpr int STEP = F32 ? 2 : 16;
  constexpr int ES = (int)sizeof(T);
  __shared__ __attribute__((aligned(16))) char lds[32 * (9 * GC_MAXRED * ES + 16)];
  const int pitch = 9 * p.redp * ES + 16;
  const GcBlock k = gc_block(blockIdx.x, p.G, p.Rg, p.Dg, p.GB, p.nsub);
  gc_stage_filter<T>(lds, pitch, p.w, k, p.Rg, p.Dg, p.Cg, p.nsub, p.redp, p.dgrad);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = cn_uniform(threadIdx.x >> 6);
  const int h = lane >> 5;
  const int nks = p.redp / STEP;
  const int sh = p.stride - 1;      // stride 1 or 2
  // the whole 32-row block is stored with 4-channel vector stores; they need a 4-aligned first row (Cout is a multiple of
  // 4), which a block that starts inside a group of 33..63 rows need not have (e.g. K/g = 34: row0 = g*34 + 32)
  const bool full = k.nrows == 32 && (k.row0 & 3) == 0;
  for (int tile = blockIdx.y * GC_WAVES + wave; tile < p.ntiles; tile += gridDim.y * GC_WAVES) {
    const int m = tile * 32 + (lane & 31);
    const bool mok = m < p.M;
    const int mc = mok ? m : p.M - 1;
    const int nq = (int)cn_fastdiv((unsigned)mc, p.div_wo);
    const int q = mc - nq * p.Wo;
    const int n = (int)cn_fastdiv((unsigned)nq, p.div_ho);
    const int pr = nq - n * p.Ho;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int tap = 0; tap < 9; ++tap) {
      const int tr = tap / 3, ts = tap - tr * 3;
      int sy, sx;
      bool ok = mok;
      if (p.dgrad) {
        const int ty = pr + 1 - tr, tx = q + 1 - ts;
        ok = ok && ty >= 0 && tx >= 0 && (ty & sh) == 0 && (tx & sh) == 0;
        sy = ty >> sh; sx = tx >> sh;
      } else {
        sy = pr * p.stride - 1 + tr; sx = q * p.stride - 1 + ts;
        ok = ok && sy >= 0 && sx >= 0;
      }
      ok = ok && sy < p.Hs && sx < p.Ws;
      const char* sp = p.src + ((((size_t)n * p.Hs + (size_t)(ok ? sy : 0)) * p.Ws + (size_t)(ok ? sx : 0)) * p.Csrc
                                + (size_t)k.red0) * ES;
      const char* ap = lds + (lane & 31) * pitch + tap * p.redp * ES;
      for (int ks = 0; ks < nks; ++ks) {
        if constexpr (F32) {
          const int cc = ks * 2 + h;
          const float b = ok && cc < k.nred ? *(const float*)(sp + cc * 4) : 0.f;
          const float a = *(const float*)(ap + cc * 4);
          acc = cn_mfma_32x32x2_f32(a, b, acc);
        } else {
          const int cc0 = ks * 16 + 8 * h;
          s16x8 b;
          if constexpr (VEC) {
            b = __builtin_bit_cast(s16x8, ok && cc0 < k.nred ? cn_ld16(sp + cc0 * 2) : cn_zero16());
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              b[e] = ok && cc0 + e < k.nred ? *(const short*)(sp + (cc0 + e) * 2) : (short)0;
          }
          const s16x8 a = __builtin_bit_cast(s16x8, cn_ld16(ap + cc0 * 2));
          if constexpr (std::is_same<T, f16_t>::value) acc = cn_mfma_32x32x16_f16(a, b, acc);
          else acc = cn_mfma_32x32x16_bf16(a, b, acc);
        }
      }
    }
    if (!mok) continue;
    char* op = p.out + ((size_t)m * p.Cout + (size_t)k.row0) * ES;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int i0 = 8 * qd + 4 * h;   // rows i0 .. i0 + 3 of this lane: acc[4 qd .. 4 qd + 3]
      if (full) {
        if constexpr (F32) {
          f32x4 v = {acc[4 * qd], acc[4 * qd + 1], acc[4 * qd + 2], acc[4 * qd + 3]};
          *(f32x4*)(op + i0 * 4) = v;
        } else {
          u32x2 v;
          v[0] = cn_pack2<T>(acc[4 * qd], acc[4 * qd + 1]);
          v[1] = cn_pack2<T>(acc[4 * qd + 2], acc[4 * qd + 3]);
          *(u32x2*)(op + i0 * 2) = v;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i0 + e < k.nrows) cn_store_elem<T>((T*)(op + (i0 + e) * ES), acc[4 * qd + e]);
      }
    }
  }
}

struct GcwParams {
  const char* x;      // [N][H][W][C]
  const char* dy;     // [N][P][Q][K]
  float* part;        // [nsplit][K][9][Cg]
  int N, H, W, C, P, Q, K, Cg;
  int G, Rg, Dg, GB, nsub;
  int stride, M, nchunks, nct, nctg;
  FastDiv div_q, div_p;
};

#define GCW_CT 3     /* column tiles (of 32) per wave */

template <typename T>
__global__ __launch_bounds__(256) void gconv_dw_kernel(GcwParams p) {
  constexpr bool F32 = std::is_same<T, float>::value;
  constexpr int ES = (int)sizeof(T);
  __shared__ __attribute__((aligned(16))) float red[GC_WAVES * GCW_CT * 1024];
  const int b = blockIdx.x / p.nctg, ctg = blockIdx.x - b * p.nctg;
  const GcBlock k = gc_block(b, p.G, p.Rg, p.Dg, p.GB, p.nsub);
  const int lane = threadIdx.x & 63;
  const int wave = cn_uniform(threadIdx.x >> 6);
  const int h = lane >> 5;
  const int i = lane & 31;
  const int ncol = 9 * k.nred;
  // this lane's B column in each of the wave's column tiles: (tap, reduction channel)
  int ctap[GCW_CT], ccol[GCW_CT];
  bool cok[GCW_CT];
#pragma unroll
  for (int t = 0; t < GCW_CT; ++t) {
    const int j = ((ctg * GCW_CT + t) * 32) + i;
    cok[t] = ctg * GCW_CT + t < p.nct && j < ncol;
    const int jj = cok[t] ? j : 0;
    ctap[t] = jj / k.nred;
    ccol[t] = jj - ctap[t] * k.nred;
  }
  f32x16 acc[GCW_CT];
#pragma unroll
  for (int t = 0; t < GCW_CT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const bool rok = i < k.nrows;
  const int nw = gridDim.y * GC_WAVES;
  for (int ch = blockIdx.y * GC_WAVES + wave; ch < p.nchunks; ch += nw) {
    // the pixels of this lane in the chunk's MFMA k dimension: 16-bit 8 * h + e (one MFMA), fp32 2 * e + h (eight)
    int pn[8], py[8], px[8];
    bool pok[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int m = ch * 16 + (F32 ? 2 * e + h : 8 * h + e);
      pok[e] = m < p.M;
      const int mc = pok[e] ? m : 0;
      const int nq = (int)cn_fastdiv((unsigned)mc, p.div_q);
      px[e] = mc - nq * p.Q;
      pn[e] = (int)cn_fastdiv((unsigned)nq, p.div_p);
      py[e] = nq - pn[e] * p.P;
    }
    float av[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const size_t mi = (((size_t)pn[e] * p.P + py[e]) * p.Q + px[e]);
      av[e] = pok[e] && rok ? cn_load_elem<T>((const T*)(p.dy + (mi * p.K + k.row0 + i) * ES)) : 0.f;
    }
#pragma unroll
    for (int t = 0; t < GCW_CT; ++t) {
      if (ctg * GCW_CT + t >= p.nct) break;
      const int tr = ctap[t] / 3, ts = ctap[t] - tr * 3;
      float bv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int iy = py[e] * p.stride - 1 + tr, ix = px[e] * p.stride - 1 + ts;
        const bool ok = pok[e] && cok[t] && iy >= 0 && ix >= 0 && iy < p.H && ix < p.W;
        bv[e] = ok ? cn_load_elem<T>((const T*)(p.x + ((((size_t)pn[e] * p.H + iy) * p.W + ix) * p.C + k.red0 + ccol[t]) * ES))
                   : 0.f;
      }
      if constexpr (F32) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[t] = cn_mfma_32x32x2_f32(av[e], bv[e], acc[t]);
      } else {
        s16x8 a, bb;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned pa = cn_pack2<T>(av[2 * e], av[2 * e + 1]), pb = cn_pack2<T>(bv[2 * e], bv[2 * e + 1]);
          a[2 * e] = (short)(pa & 0xffffu); a[2 * e + 1] = (short)(pa >> 16);
          bb[2 * e] = (short)(pb & 0xffffu); bb[2 * e + 1] = (short)(pb >> 16);
        }
        if constexpr (std::is_same<T, f16_t>::value) acc[t] = cn_mfma_32x32x16_f16(a, bb, acc[t]);
        else acc[t] = cn_mfma_32x32x16_bf16(a, bb, acc[t]);
      }
    }
  }
  // the four waves' sums, added in wave order; only the block-diagonal entries are written
#pragma unroll
  for (int t = 0; t < GCW_CT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ii = (r & 3) + 8 * (r >> 2) + 4 * h;
      red[((wave * GCW_CT + t) * 32 + ii) * 32 + i] = acc[t][r];
    }
  __syncthreads();
  float* dst = p.part + (size_t)blockIdx.y * p.K * 9 * p.Cg;
  for (int id = threadIdx.x; id < GCW_CT * 1024; id += 256) {
    const int t = id >> 10, ii = (id >> 5) & 31, jl = id & 31;
    const int j = (ctg * GCW_CT + t) * 32 + jl;
    if (ctg * GCW_CT + t >= p.nct || j >= ncol || ii >= k.nrows) continue;
    const int tap = j / k.nred, cc = j - tap * k.nred;
    const int gi = p.nsub == 1 ? ii / p.Rg : 0, gc = p.nsub == 1 ? cc / p.Dg : 0;
    if (gi != gc) continue;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < GC_WAVES; ++w) s += red[((w * GCW_CT + t) * 32 + ii) * 32 + jl];
    const int row = k.row0 + ii, g = row / p.Rg;
    dst[((size_t)row * 9 + tap) * p.Cg + (k.red0 + cc - g * p.Dg)] = s;
  }
}

// ------------------------------------------------------------------------------------------------ host side
static int gc_check(const char* who, int N, int H, int W, int C, int K, int groups, int stride, int dtype) {
  if (!cn_gconv2d_ok(C, K, groups, 3, 3, stride, stride, 1, 1, dtype) || N <= 0 || H <= 0 || W <= 0) {
    cn_set_error("%s: unsupported grouped convolution (N=%d H=%d W=%d C=%d K=%d groups=%d stride=%d dtype=%d): needs a "
                 "3x3 filter, stride 1 or 2, padding 1, groups dividing C and K, 1 <= C/g, K/g <= 64, C and K multiples "
                 "of the dtype's chunk",
                 who, N, H, W, C, K, groups, stride, dtype);
    return CN_ESHAPE;
  }
  return CN_OK;
}

extern "C" int cn_gconv2d_ok(int C, int K, int groups, int R, int S, int stride_h, int stride_w, int pad_h, int pad_w,
                             int dtype) {
  if (!cn_dtype_ok(dtype) || groups < 1 || C < 1 || K < 1) return 0;
  if (R != 3 || S != 3 || pad_h != 1 || pad_w != 1 || stride_h != stride_w || (stride_h != 1 && stride_h != 2)) return 0;
  if (C % groups != 0 || K % groups != 0) return 0;
  const int cg = C / groups, kg = K / groups, ch = cn_dtype_chunk(dtype);
  if (cg > GC_MAXRED || kg > GC_MAXRED) return 0;
  return C % ch == 0 && K % ch == 0 ? 1 : 0;
}

static int gc_wgs(int nblocks, int units) {
  int y = cn_get_option("gconv_wgs", 2048) / nblocks;
  if (y < 1) y = 1;
  return y < units ? y : units;
}

static int gc_run(const char* who, const void* src, const void* w, void* out, int N, int Hs, int Ws, int Csrc, int Ho,
                  int Wo, int Cout, int Cg, int groups, int stride, int dgrad, int dtype, void* stream) {
  const int step = dtype == CN_F32 ? 2 : 16;
  // forward: rows = K/g output channels, reduction = C/g; data gradient: rows = C/g, reduction = K/g
  const GcGeom g = gc_geom(groups, Cout / groups, Csrc / groups, step);
  GcParams p;
  memset(&p, 0, sizeof(p));
  p.src = (const char*)src; p.w = (const char*)w; p.out = (char*)out;
  p.N = N; p.Hs = Hs; p.Ws = Ws; p.Csrc = Csrc; p.Ho = Ho; p.Wo = Wo; p.Cout = Cout; p.Cg = Cg;
  p.G = g.G; p.Rg = g.Rg; p.Dg = g.Dg; p.GB = g.GB; p.nsub = g.nsub; p.redp = g.redp;
  p.stride = stride; p.dgrad = dgrad;
  const long long M = (long long)N * Ho * Wo;
  if (M >= (1ll << 31) || (long long)N * Hs * Ws * Csrc >= (1ll << 40)) { cn_set_error("%s: tensor too large", who); return CN_ESHAPE; }
  p.M = (int)M;
  p.ntiles = (int)((M + 31) / 32);
  p.div_wo = cn_make_fastdiv((unsigned)Wo);
  p.div_ho = cn_make_fastdiv((unsigned)Ho);
  // whole 8-channel chunks in every block (and in the last, partial one)
  const bool vec = (g.nsub == 2 ? g.Dg % 8 == 0 : (g.GB * g.Dg) % 8 == 0 && (g.G % g.GB == 0 || g.Dg % 8 == 0));
  const dim3 grid((unsigned)g.nblocks, (unsigned)gc_wgs(g.nblocks, (p.ntiles + GC_WAVES - 1) / GC_WAVES));
  const char* tn = dtype == CN_BF16 ? "bf16_t" : dtype == CN_F16 ? "f16_t" : "float";
  cn_set_last_kernel("gconv_kernel<%s, %s>%s", tn, vec ? "true" : "false", dgrad ? " [dgrad]" : "");
  if (dtype == CN_BF16) {
    if (vec) CN_LAUNCH((gconv_kernel<bf16_t, true>), grid, dim3(256), (hipStream_t)stream, p);
    else CN_LAUNCH((gconv_kernel<bf16_t, false>), grid, dim3(256), (hipStream_t)stream, p);
  } else if (dtype == CN_F16) {
    if (vec) CN_LAUNCH((gconv_kernel<f16_t, true>), grid, dim3(256), (hipStream_t)stream, p);
    else CN_LAUNCH((gconv_kernel<f16_t, false>), grid, dim3(256), (hipStream_t)stream, p);
  } else {
    CN_LAUNCH((gconv_kernel<float, false>), grid, dim3(256), (hipStream_t)stream, p);
  }
  return cn_check_launch(who);
}

// y[N][P][Q][K] = grouped conv3x3(x[N][H][W][C], w[K][3][3][C/g]), stride `stride`, padding 1.
extern "C" cn_status cn_gconv2d_fwd(const void* x, const void* w, void* y, int N, int H, int W, int C, int K, int groups,
                                    int stride, int dtype, void* stream) {
  if (x == nullptr || w == nullptr || y == nullptr) { cn_set_error("gconv2d_fwd: null operand"); return CN_EINVAL; }
  const int rc = gc_check("gconv2d_fwd", N, H, W, C, K, groups, stride, dtype);
  if (rc != CN_OK) return rc;
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  return gc_run("gconv2d_fwd", x, w, y, N, H, W, C, P, Q, K, C / groups, groups, stride, 0, dtype, stream);
}

// dx[N][H][W][C] from dy[N][P][Q][K] and the same filter w[K][3][3][C/g].
extern "C" cn_status cn_gconv2d_dgrad(const void* dy, const void* w, void* dx, int N, int H, int W, int C, int K, int groups,
                                      int stride, int dtype, void* stream) {
  if (dy == nullptr || w == nullptr || dx == nullptr) { cn_set_error("gconv2d_dgrad: null operand"); return CN_EINVAL; }
  const int rc = gc_check("gconv2d_dgrad", N, H, W, C, K, groups, stride, dtype);
  if (rc != CN_OK) return rc;
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  return gc_run("gconv2d_dgrad", dy, w, dx, N, P, Q, K, H, W, C, C / groups, groups, stride, 1, dtype, stream);
}

struct GcwPlan { GcGeom g; int nct, nctg, nchunks, nsplit; };
static GcwPlan gcw_plan(int N, int H, int W, int C, int K, int groups, int stride, int dtype) {
  GcwPlan w;
  w.g = gc_geom(groups, K / groups, C / groups, dtype == CN_F32 ? 2 : 16);
  const int nred = w.g.GB * w.g.Dg;
  w.nct = (9 * nred + 31) / 32;
  w.nctg = (w.nct + GCW_CT - 1) / GCW_CT;
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  const long long M = (long long)N * P * Q;
  w.nchunks = (int)((M + 15) / 16);
  w.nsplit = gc_wgs(w.g.nblocks * w.nctg, (w.nchunks + GC_WAVES - 1) / GC_WAVES);
  return w;
}

extern "C" size_t cn_gconv2d_wgrad_workspace(int N, int H, int W, int C, int K, int groups, int stride, int dtype) {
  if (!cn_gconv2d_ok(C, K, groups, 3, 3, stride, stride, 1, 1, dtype) || N <= 0 || H <= 0 || W <= 0) return 0;
  const GcwPlan w = gcw_plan(N, H, W, C, K, groups, stride, dtype);
  return (size_t)w.nsplit * K * 9 * (C / groups) * sizeof(float);
}

// dw[K][3][3][C/g] (fp32) = beta * dw + scale * wgrad(x, dy); `workspace` of cn_gconv2d_wgrad_workspace bytes.
extern "C" cn_status cn_gconv2d_wgrad(const void* x, const void* dy, float* dw, int N, int H, int W, int C, int K, int groups,
                                      int stride, int dtype, float beta, float scale, void* workspace, size_t ws_bytes,
                                      void* stream) {
  if (x == nullptr || dy == nullptr || dw == nullptr) { cn_set_error("gconv2d_wgrad: null operand"); return CN_EINVAL; }
  const int rc = gc_check("gconv2d_wgrad", N, H, W, C, K, groups, stride, dtype);
  if (rc != CN_OK) return rc;
  const size_t need = cn_gconv2d_wgrad_workspace(N, H, W, C, K, groups, stride, dtype);
  if (workspace == nullptr || ws_bytes < need) {
    cn_set_error("gconv2d_wgrad: workspace of %zu bytes < %zu", ws_bytes, need);
    return CN_EWORKSPACE;
  }
  const GcwPlan w = gcw_plan(N, H, W, C, K, groups, stride, dtype);
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  if ((long long)N * P * Q >= (1ll << 31)) { cn_set_error("gconv2d_wgrad: tensor too large"); return CN_ESHAPE; }
  GcwParams p;
  memset(&p, 0, sizeof(p));
  p.x = (const char*)x; p.dy = (const char*)dy; p.part = (float*)workspace;
  p.N = N; p.H = H; p.W = W; p.C = C; p.P = P; p.Q = Q; p.K = K; p.Cg = C / groups;
  p.G = w.g.G; p.Rg = w.g.Rg; p.Dg = w.g.Dg; p.GB = w.g.GB; p.nsub = w.g.nsub;
  p.stride = stride; p.M = N * P * Q; p.nchunks = w.nchunks; p.nct = w.nct; p.nctg = w.nctg;
  p.div_q = cn_make_fastdiv((unsigned)Q);
  p.div_p = cn_make_fastdiv((unsigned)P);
  const dim3 grid((unsigned)(w.g.nblocks * w.nctg), (unsigned)w.nsplit);
  const hipStream_t st = (hipStream_t)stream;
  CnMarkLast mark;
  cn_set_last_kernel("gconv_dw_kernel<%s>", dtype == CN_BF16 ? "bf16_t" : dtype == CN_F16 ? "f16_t" : "float");
  if (dtype == CN_BF16) CN_LAUNCH(gconv_dw_kernel<bf16_t>, grid, dim3(256), st, p);
  else if (dtype == CN_F16) CN_LAUNCH(gconv_dw_kernel<f16_t>, grid, dim3(256), st, p);
  else CN_LAUNCH(gconv_dw_kernel<float>, grid, dim3(256), st, p);
  int rc2 = cn_check_launch("gconv2d_wgrad");
  if (rc2 != CN_OK) return rc2;
  mark.release();
  return wg_launch_reduce(st, (const float*)workspace, dw, w.nsplit, K, 9, C / groups, C / groups, beta, scale);
}
