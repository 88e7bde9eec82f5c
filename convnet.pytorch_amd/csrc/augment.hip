// augment.hip -- the CIFAR training / evaluation transform on a dataset that lives in device memory
// (preprocess.py:44-54 random_crop, :185-227 Cutout; data.DeviceCifarLoader): one pass cuts a batch of views out of the
// resident uint8 images and writes it in the form the step consumes.
//
//   RandomCrop(S, padding=pad)  the uint8 image is padded with 0 and an S x S window is taken at (top, left), both in
//                               [0, 2*pad]: a pixel of the padding is BYTE 0, i.e. lut[c][0] = -mean/std after Normalize
//   RandomHorizontalFlip        output column w reads window column S-1-w
//   ToTensor + Normalize        lut[c][byte] (ops.normalize_lut: the reference's own fp32 operations, so bit-identical)
//   Cutout                      the rectangle [y1, y2) x [x1, x2) of the OUTPUT is 0.0 (the reference multiplies the
//                               normalised tensor by a 0/1 mask); an empty rectangle is no cutout
//
// One lane per output pixel.  FORM 0 writes the reference loader's fp32 NCHW batch (three coalesced plane stores), FORM 1
// the NHWC compute-dtype tensor conv1 reads: the pixel's three channels and the zero pad channels are one 16-byte chunk,
// exactly what cn_nchw_to_nhwc makes of FORM 0.  No atomics, no host state: every input is a device buffer.
#include "cn_common.h"
#include "cn_api_internal.h"

#define AUG_NP CN_AUGMENT_PARAMS

template <typename T, int FORM>
__global__ __launch_bounds__(256) void augment_crop_flip_kernel(const unsigned char* data, const int* idx, const int* params,
                                                                const float* lut, char* out, int N, int V, int S, int pad) {
  __shared__ float s_lut[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) s_lut[i] = lut[i];
  __syncthreads();
  constexpr int CH = ElemTraits<T>::kChunk;
  constexpr int EB = ElemTraits<T>::kBytes;
  const int HW = S * S;
  const long long total = (long long)V * HW;
  for (long long id = (long long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long long)gridDim.x * 256) {
    const int v = (int)(id / HW);
    const int hw = (int)(id - (long long)v * HW);
    const int h = hw / S, w = hw - h * S;
    const int* p = params + (size_t)v * AUG_NP;
    const int top = p[0], left = p[1], flip = p[2];
    const int y1 = p[3], y2 = p[4], x1 = p[5], x2 = p[6];
    const int img = idx[v];
    float f[CH > 3 ? CH : 3];
#pragma unroll
    for (int c = 0; c < (CH > 3 ? CH : 3); ++c) f[c] = 0.f;
    const bool cut = h >= y1 && h < y2 && w >= x1 && w < x2;
    if (!cut) {
      const int sy = top + h - pad;
      const int sx = left + (flip ? S - 1 - w : w) - pad;
      // outside the image (the crop's zero padding) - or an index outside the dataset - is byte 0: no address is formed
      const bool in = (unsigned)sy < (unsigned)S && (unsigned)sx < (unsigned)S && (unsigned)img < (unsigned)N;
      const size_t off = in ? ((size_t)img * HW + (size_t)sy * S + sx) * 3 : 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) f[c] = s_lut[c * 256 + (in ? data[off + c] : 0)];
    }
    if (FORM == 0) {
      float* y = (float*)out + (size_t)v * 3 * HW + hw;
#pragma unroll
      for (int c = 0; c < 3; ++c) y[(size_t)c * HW] = f[c];
    } else {
      cn_st16(out + (size_t)id * CH * EB, Chunk<T>::pack(f));
    }
  }
}

extern "C" cn_status cn_augment_crop_flip(const unsigned char* data, long long data_bytes, const int* idx, const int* params,
                                          const float* lut, void* out, int N, int V, int S, int pad, int c_pad, int dtype,
                                          int form, void* stream) {
  if (data == nullptr || idx == nullptr || params == nullptr || lut == nullptr || out == nullptr) {
    cn_set_error("augment_crop_flip: null operand");
    return CN_EINVAL;
  }
  if (!cn_dtype_ok(dtype) || (form != 0 && form != 1)) { cn_set_error("augment_crop_flip: bad dtype %d / form %d", dtype, form); return CN_EINVAL; }
  if (form == 0 && dtype != CN_F32) { cn_set_error("augment_crop_flip: the NCHW form is fp32 (dtype %d)", dtype); return CN_EINVAL; }
  if (N <= 0 || V <= 0 || S <= 0 || S > 4096 || pad < 0 || pad > S) {
    cn_set_error("augment_crop_flip: bad shape (N=%d V=%d S=%d pad=%d)", N, V, S, pad);
    return CN_ESHAPE;
  }
  if ((long long)N * S * S * 3 != data_bytes) {
    cn_set_error("augment_crop_flip: %d images of %d x %d x 3 bytes do not fill a buffer of %lld bytes", N, S, S, data_bytes);
    return CN_ESHAPE;
  }
  if (form == 1 && c_pad != cn_dtype_chunk(dtype)) {
    cn_set_error("augment_crop_flip: the NHWC form writes one 16-byte chunk per pixel (c_pad=%d, need %d)", c_pad, cn_dtype_chunk(dtype));
    return CN_ESHAPE;
  }
  const long long total = (long long)V * S * S;
  long long nb = (total + 255) / 256;
  if (nb > 8192) nb = 8192;
  dim3 grid((unsigned)nb);
  hipStream_t s = (hipStream_t)stream;
#define AUG_GO(T, FORM) CN_LAUNCH((augment_crop_flip_kernel<T, FORM>), grid, dim3(256), s, data, idx, params, lut, (char*)out, N, V, S, pad)
  if (form == 0) AUG_GO(float, 0);
  else if (dtype == CN_BF16) AUG_GO(bf16_t, 1);
  else if (dtype == CN_F16) AUG_GO(f16_t, 1);
  else AUG_GO(float, 1);
#undef AUG_GO
  return cn_check_launch("augment_crop_flip");
}
