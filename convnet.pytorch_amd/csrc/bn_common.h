// bn_common.h -- helpers shared by the per-channel normalisation kernels (bn.hip, l1bn.hip): the lane / workgroup
// mapping of an NHWC tensor, cache-policy accessors, the workgroup column sum, the fixed-order reduction of partial
// rows, and the (dtype, cache policy) launch dispatch.
#pragma once
#include "cn_common.h"
#include "cn_api_internal.h"

static inline int bn_next_pow2_log2(int v) {
  int s = 0;
  while ((1 << s) < v) ++s;
  return s;
}

struct BnMap {
  int tpr_log2;  // threads per row (power of two, <= 256)
  int gy;        // column groups
  int rpp;       // rows per pass of one workgroup
};
static BnMap bn_map(int cpr) {
  BnMap m;
  int l = bn_next_pow2_log2(cpr);
  if (l > 8) l = 8;
  m.tpr_log2 = l;
  m.gy = (cpr + (1 << l) - 1) >> l;
  m.rpp = 256 >> l;
  return m;
}
// 1 = the apply passes use non-temporal accesses (default; tensors below "bn_nt_min_mb" MB and
// "bn_nt" = 0 use the cached policy: whole-step A/B knobs)
static int bn_nt_flag(long long M, int C, int dtype) {
  if (cn_get_option("bn_nt", 1) == 0) return 0;
  const long long bytes = M * C * cn_dtype_bytes(dtype);
  return bytes < (long long)cn_get_option("bn_nt_min_mb", 0) * (1ll << 20) ? 0 : 1;
}
// Cache policy of the streaming passes is a COMPILE-TIME parameter of the kernels (NT): a run-time select
// between a plain and a non-temporal access of the same address is folded by LLVM into one plain access
// (round 1 shipped exactly that; tools/check_nt.sh now greps the code object for the `nt` accesses).
template <bool NT, int SITE>
__device__ __forceinline__ u32x4 bn_ld(const void* p) {
  if constexpr (NT) return cn_ld16_stream<SITE>(p);
  else return cn_ld16(p);
}
template <bool NT, int SITE>
__device__ __forceinline__ void bn_st(void* p, const u32x4& v) {
  if constexpr (NT) cn_st16_stream<SITE>(p, v);
  else cn_st16(p, v);
}
static int bn_row_blocks(long long M, const BnMap& m, int target_blocks) {
  long long passes = (M + m.rpp - 1) / m.rpp;
  long long nb = target_blocks / m.gy;
  if (nb < 1) nb = 1;
  long long cap = (passes + 3) / 4;  // at least ~4 passes per workgroup
  if (cap < 1) cap = 1;
  if (nb > cap) nb = cap;
  return (int)nb;
}

// Column sums of a 256-thread workgroup laid out as row slices of `tpr` chunk columns (thread tid owns column
// tid & (tpr-1) of row slice tid >> tpr_log2): the row slices that live in one wave are folded with wavefront
// shuffles (an xor butterfly over the lane bits above log2(tpr)), LDS then carries one value set per wave instead of
// one per thread, and the owner (row slice 0) adds the <= 4 of them in a fixed order.  Deterministic.
template <int N>
__device__ __forceinline__ void bn_block_colsum(float (&a)[N], float (&b)[N], float* red /*[256][2N]*/, int tpr_log2,
                                                int tid) {
  const int tpr = 1 << tpr_log2;
  for (int m = 32; m >= tpr; m >>= 1) {   // wave-uniform trip count (0 when a row slice fills a wave or more)
#pragma unroll
    for (int e = 0; e < N; ++e) { a[e] += cn_shfl_xor(a[e], m); b[e] += cn_shfl_xor(b[e], m); }
  }
#pragma unroll
  for (int e = 0; e < N; ++e) { red[tid * 2 * N + e] = a[e]; red[tid * 2 * N + N + e] = b[e]; }
  __syncthreads();
  if ((tid >> tpr_log2) == 0) {
    const int stride = tpr > 64 ? tpr : 64;   // one representative per wave (or per row slice when slices span waves)
#pragma unroll
    for (int e = 0; e < N; ++e) { a[e] = 0.f; b[e] = 0.f; }
    for (int t = tid; t < 256; t += stride) {
      const float* o = red + t * 2 * N;
#pragma unroll
      for (int e = 0; e < N; ++e) { a[e] += o[e]; b[e] += o[N + e]; }
    }
  }
}

// Fixed-order, latency-tolerant reduction of the per-workgroup partials: BN_FC channels per workgroup,
// BN_FP threads per channel each summing every BN_FP-th partial row with 16 independent loads in
// flight, then a fixed-order LDS combine.  (A single thread walking all partials is a chain of
// dependent L2 round trips: measured 0.5 ms per launch at 2048 partials; with 8 threads per channel
// 512 rows still took 4 dependent rounds, with 32 it is one or two.)
#define BN_FC 8     /* channels per workgroup */
#define BN_FP 32    /* row slices (threads per channel) */
__device__ __forceinline__ void bn_sum_partials(const float* partial, int nrb, int C, int c, int part,
                                                double* red /*[2][BN_FP][BN_FC]*/, double& s_out, double& q_out) {
  double s = 0.0, q = 0.0;
  if (c < C) {
    int r = part;
    for (; r + 15 * BN_FP < nrb; r += 16 * BN_FP) {   // 32 independent loads in flight: 512 rows = one round trip
      float a[16], b[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        a[u] = partial[(size_t)(r + BN_FP * u) * 2 * C + c];
        b[u] = partial[(size_t)(r + BN_FP * u) * 2 * C + C + c];
      }
#pragma unroll
      for (int u = 0; u < 16; u += 4) {
        s += ((double)a[u] + (double)a[u + 1]) + ((double)a[u + 2] + (double)a[u + 3]);
        q += ((double)b[u] + (double)b[u + 1]) + ((double)b[u + 2] + (double)b[u + 3]);
      }
    }
    for (; r + 7 * BN_FP < nrb; r += 8 * BN_FP) {   // 16 independent loads in flight per thread
      float a[8], b[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        a[u] = partial[(size_t)(r + BN_FP * u) * 2 * C + c];
        b[u] = partial[(size_t)(r + BN_FP * u) * 2 * C + C + c];
      }
      s += (((double)a[0] + (double)a[1]) + ((double)a[2] + (double)a[3])) +
           (((double)a[4] + (double)a[5]) + ((double)a[6] + (double)a[7]));
      q += (((double)b[0] + (double)b[1]) + ((double)b[2] + (double)b[3])) +
           (((double)b[4] + (double)b[5]) + ((double)b[6] + (double)b[7]));
    }
    if (r < nrb) {   // < 8 rows left: requested together (one by one they are a chain of L2 round trips, ~1.4 us
      float a[7], b[7];   // each: 392 rows cost 5.4 us, 483 rows 9.6 us), added in row order; clamped index, not a
#pragma unroll            // branch around each load
      for (int u = 0; u < 7; ++u) {
        const int ru = r + BN_FP * u;
        const int rc = ru < nrb ? ru : nrb - 1;
        const float av = partial[(size_t)rc * 2 * C + c], bv = partial[(size_t)rc * 2 * C + C + c];
        a[u] = ru < nrb ? av : 0.f;
        b[u] = ru < nrb ? bv : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 7; ++u) { s += (double)a[u]; q += (double)b[u]; }
    }
  }
  const int lc = threadIdx.x % BN_FC;
  red[part * BN_FC + lc] = s;
  red[BN_FP * BN_FC + part * BN_FC + lc] = q;
  __syncthreads();
  s = 0.0;
  q = 0.0;
#pragma unroll
  for (int k = 0; k < BN_FP; ++k) { s += red[k * BN_FC + lc]; q += red[BN_FP * BN_FC + k * BN_FC + lc]; }
  s_out = s;
  q_out = q;
}

// ------------------------------------------------------------------------------------------------
// (dtype, cache policy) -> kernel instantiation
#define BN_DISPATCH(kern, dtype, nt, grid, stream, ...)                                            \
  do {                                                                                             \
    if ((dtype) == CN_BF16) {                                                                      \
      if (nt) CN_LAUNCH((kern<bf16_t, true>), grid, dim3(256), stream, __VA_ARGS__);                \
      else CN_LAUNCH((kern<bf16_t, false>), grid, dim3(256), stream, __VA_ARGS__);                  \
    } else if ((dtype) == CN_F16) {                                                                \
      if (nt) CN_LAUNCH((kern<f16_t, true>), grid, dim3(256), stream, __VA_ARGS__);                 \
      else CN_LAUNCH((kern<f16_t, false>), grid, dim3(256), stream, __VA_ARGS__);                   \
    } else {                                                                                       \
      if (nt) CN_LAUNCH((kern<float, true>), grid, dim3(256), stream, __VA_ARGS__);                 \
      else CN_LAUNCH((kern<float, false>), grid, dim3(256), stream, __VA_ARGS__);                   \
    }                                                                                              \
  } while (0)

// (the reduction passes: cached loads only - non-temporal loads there measured slower, profiles/README.md)
#define BN_DISPATCH_PLAIN(kern, dtype, grid, stream, ...)                                          \
  do {                                                                                             \
    if ((dtype) == CN_BF16) CN_LAUNCH((kern<bf16_t, false>), grid, dim3(256), stream, __VA_ARGS__); \
    else if ((dtype) == CN_F16) CN_LAUNCH((kern<f16_t, false>), grid, dim3(256), stream, __VA_ARGS__); \
    else CN_LAUNCH((kern<float, false>), grid, dim3(256), stream, __VA_ARGS__);                     \
  } while (0)

#define BN_TARGET_BLOCKS 512   /* partial rows per channel the finalize kernels take without a compression launch */
/* Row blocks of the standalone reduction passes (bn_stats / bn_bwd_reduce; knob "bn_reduce_blocks").  256: the kernels keep
 * 8-12 sixteen-byte loads in flight per lane, so 256 workgroups already saturate HBM, and fewer, longer workgroups leave the
 * chain's other kernels and the side stream more of the chip: 14.93k img/s vs 14.76k at 512, 14.59k at 128, 13.76k at 64
 * (round 4, profiles/README.md). */
#define BN_REDUCE_BLOCKS 256
#define BN_APPLY_BLOCKS 2048   /* pure streaming kernels */
/* Sweep direction of the streaming kernels, bit 0: forward apply, bit 1: backward reduce, bit 2: backward
 * apply.  A kernel that sweeps in the opposite direction to the one that last touched its input finds
 * the freshest part of that tensor still in the 256 MB Infinity Cache (tuning knob "bn_reverse"). */
#define BN_REVERSE_DEFAULT 0
