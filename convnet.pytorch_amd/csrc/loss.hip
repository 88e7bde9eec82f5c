// loss.hip -- softmax cross-entropy (forward + gradient in one pass), top-1/top-5 hit counting
// and on-device meter accumulation, gfx950.
//
// Replaces criterion(output, target) = CrossEntropyLoss(**{smooth_eps}) (/root/reference
// main.py:231-235, trainer.py:143; class lives in the un-vendored utils submodule and equals
// F.cross_entropy for smooth_eps = 0), its backward, and utils.meters.accuracy(output, target,
// topk=(1,5)) (trainer.py:224).  The reference pulls loss / prec@k to the host every step
// (trainer.py:153,225-229); here they are accumulated on the device and read when a report is due.
#include "cn_common.h"
#include "cn_api_internal.h"

__device__ __forceinline__ float ls_block_reduce(float v, float* red, bool is_max) {
  // 256 threads = 4 waves
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    float o = cn_shfl_xor(v, m);
    v = is_max ? fmaxf(v, o) : v + o;
  }
  const int tid = threadIdx.x;
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
  return r;
}

// One workgroup per sample.  row_out[b] = {loss_b, top1_hit, top5_hit}
template <typename TG>
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float* logits, const long long* target,
                                                        TG* dlogits, float* row_out, int B, int K,
                                                        float gscale, const float* gscale_dev,
                                                        float smooth_eps) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* row = logits + (size_t)b * K;
  const int tgt = (int)target[b];
  float mx = -INFINITY;
  for (int k = tid; k < K; k += 256) mx = fmaxf(mx, row[k]);
  mx = ls_block_reduce(mx, red, true);
  float se = 0.f, sl = 0.f;
  const float lt = row[tgt];
  float rank = 0.f;
  for (int k = tid; k < K; k += 256) {
    const float v = row[k];
    se += expf(v - mx);
    sl += v;
    // rank of the target among the logits; ties resolved towards the lower index (topk order)
    if (v > lt || (v == lt && k < tgt)) rank += 1.f;
  }
  se = ls_block_reduce(se, red, false);
  sl = ls_block_reduce(sl, red, false);
  rank = ls_block_reduce(rank, red, false);
  const float lse = mx + logf(se);
  if (dlogits != nullptr) {
    if (gscale_dev != nullptr) gscale *= gscale_dev[0];  // upstream d(loss) scalar, read on device
    const float on = 1.f - smooth_eps, off = smooth_eps / (float)K;
    for (int k = tid; k < K; k += 256) {
      const float p = expf(row[k] - lse);
      const float t = (k == tgt ? on : 0.f) + off;
      cn_store_elem<TG>(dlogits + (size_t)b * K + k, (p - t) * gscale);
    }
  }
  if (tid == 0) {
    const float nll = lse - lt;
    const float smooth = lse - sl / (float)K;  // mean_k(-log p_k)
    row_out[3 * b] = (1.f - smooth_eps) * nll + smooth_eps * smooth;
    row_out[3 * b + 1] = rank < 1.f ? 1.f : 0.f;
    row_out[3 * b + 2] = rank < 5.f ? 1.f : 0.f;
  }
}

// Fixed-order reduction over the batch.
//   step_out[0..2] = mean loss, prec@1 (%), prec@5 (%) of this batch (reference meter .val)
//   meters[0..3]  += loss*B, prec1*B, prec5*B, B                 (reference meter .sum / .count)
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* row_out, int B, float* step_out,
                                                         float* meters) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  float l = 0.f, c1 = 0.f, c5 = 0.f;
  for (int b = tid; b < B; b += 256) { l += row_out[3 * b]; c1 += row_out[3 * b + 1]; c5 += row_out[3 * b + 2]; }
  l = ls_block_reduce(l, red, false);
  c1 = ls_block_reduce(c1, red, false);
  c5 = ls_block_reduce(c5, red, false);
  if (tid == 0) {
    const float ml = l / (float)B, p1 = 100.f * c1 / (float)B, p5 = 100.f * c5 / (float)B;
    if (step_out != nullptr) { step_out[0] = ml; step_out[1] = p1; step_out[2] = p5; }
    if (meters != nullptr) { meters[0] += ml * (float)B; meters[1] += p1 * (float)B; meters[2] += p5 * (float)B; meters[3] += (float)B; }
  }
}

extern "C" cn_status cn_softmax_ce(const float* logits, const long long* target, void* dlogits, int grad_dtype,
                                   float* row_scratch, float* step_out, float* meters, int B, int K, float gscale,
                                   const float* gscale_dev, float smooth_eps, void* stream_) {
  if (B <= 0 || K <= 0) { cn_set_error("softmax_ce: empty"); return CN_ESHAPE; }
  hipStream_t stream = (hipStream_t)stream_;
  if (dlogits != nullptr && grad_dtype == CN_BF16)
    CN_LAUNCH(softmax_ce_kernel<bf16_t>, dim3((unsigned)B), dim3(256), stream, logits, target, (bf16_t*)dlogits,
              row_scratch, B, K, gscale, gscale_dev, smooth_eps);
  else if (dlogits != nullptr && grad_dtype == CN_F16)
    CN_LAUNCH(softmax_ce_kernel<f16_t>, dim3((unsigned)B), dim3(256), stream, logits, target, (f16_t*)dlogits,
              row_scratch, B, K, gscale, gscale_dev, smooth_eps);
  else
    CN_LAUNCH(softmax_ce_kernel<float>, dim3((unsigned)B), dim3(256), stream, logits, target, (float*)dlogits,
              row_scratch, B, K, gscale, gscale_dev, smooth_eps);
  CN_LAUNCH(loss_reduce_kernel, dim3(1), dim3(256), stream, (const float*)row_scratch, B, step_out, meters);
  return cn_check_launch("softmax_ce");
}

// ---- average over duplicates (trainer.py:32-41 _average_duplicates, batch_first) ---------------------------------------
// logits[B*D][K], the D rows of a sample consecutive -> mean[B][K]: the sum over d = 0..D-1 in that order in fp32, then a
// true division by (float)D (torch's mean: sum / count, not a multiply by the reciprocal).
__global__ __launch_bounds__(256) void avg_duplicates_fwd_kernel(const float* logits, float* mean, long long BK, int D, int K) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= BK) return;
  const long long b = i / K;
  const int k = (int)(i - b * K);
  const float* p = logits + (size_t)b * D * K + k;
  float s = p[0];
  for (int d = 1; d < D; ++d) s += p[(size_t)d * K];
  mean[i] = s / (float)D;
}

// dlogits[b*D + d][k] = dmean[b][k] / D for every d
template <typename TG>
__global__ __launch_bounds__(256) void avg_duplicates_bwd_kernel(const float* dmean, TG* dlogits, long long BK, int D, int K) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= BK) return;
  const long long b = i / K;
  const int k = (int)(i - b * K);
  const float g = dmean[i] / (float)D;
  TG* o = dlogits + (size_t)b * D * K + k;
  for (int d = 0; d < D; ++d) cn_store_elem<TG>(o + (size_t)d * K, g);
}

static bool avg_duplicates_shape_ok(int B, int D, int K, const char* what) {
  if (B <= 0 || D <= 0 || K <= 0 || ((long long)B * K + 255) / 256 > 0x7fffffffLL) { cn_set_error(what); return false; }
  return true;
}

extern "C" cn_status cn_avg_duplicates_fwd(const float* logits, float* mean, int B, int D, int K, void* stream_) {
  if (logits == nullptr || mean == nullptr) { cn_set_error("avg_duplicates_fwd: null operand"); return CN_EINVAL; }
  if (!avg_duplicates_shape_ok(B, D, K, "avg_duplicates_fwd: bad shape")) return CN_ESHAPE;
  const long long BK = (long long)B * K;
  CN_LAUNCH(avg_duplicates_fwd_kernel, dim3((unsigned)((BK + 255) / 256)), dim3(256), (hipStream_t)stream_, logits, mean, BK, D, K);
  return cn_check_launch("avg_duplicates_fwd");
}

extern "C" cn_status cn_avg_duplicates_bwd(const float* dmean, void* dlogits, int grad_dtype, int B, int D, int K, void* stream_) {
  if (dmean == nullptr || dlogits == nullptr) { cn_set_error("avg_duplicates_bwd: null operand"); return CN_EINVAL; }
  if (!avg_duplicates_shape_ok(B, D, K, "avg_duplicates_bwd: bad shape")) return CN_ESHAPE;
  const long long BK = (long long)B * K;
  const dim3 grid((unsigned)((BK + 255) / 256));
  hipStream_t stream = (hipStream_t)stream_;
  if (grad_dtype == CN_BF16) CN_LAUNCH(avg_duplicates_bwd_kernel<bf16_t>, grid, dim3(256), stream, dmean, (bf16_t*)dlogits, BK, D, K);
  else if (grad_dtype == CN_F16) CN_LAUNCH(avg_duplicates_bwd_kernel<f16_t>, grid, dim3(256), stream, dmean, (f16_t*)dlogits, BK, D, K);
  else if (grad_dtype == CN_F32) CN_LAUNCH(avg_duplicates_bwd_kernel<float>, grid, dim3(256), stream, dmean, (float*)dlogits, BK, D, K);
  else { cn_set_error("avg_duplicates_bwd: unknown gradient dtype"); return CN_EINVAL; }
  return cn_check_launch("avg_duplicates_bwd");
}
