// Device-side batch assembly: the sample decode of the reference's generator
// (data/mj_dataGeneratorMMUWYHsingle_repetitions.py:300-318 `__load_dd`: int16 optical flow / compressFactor * 0.1 with the
// optional magnitude clipping of :303-306, uint8 gray / depth / 255 - 0.5, silhouettes / 255), its gaitset re-layout
// (:746-753: [60,60,T] -> [25,60,60,C], channel c of frame l = raw plane C*l + c) and the expansion into rows whose
// modality is either a copy of a base sample (flag 1) or the constant `noise` (flag 0) (:732-737, :776-806).  The raw
// int16 / uint8 samples are uploaded once; the fp32 clip tensors, 4-8x larger and `expand` times repeated, are produced
// in HBM.  Pure byte-moving work: one workgroup per (output row, image line), transposed through LDS so that both the raw
// read ([x][t], t fastest) and the fp32 write ([l][..][x][c]) are coalesced.
#include "common.h"

namespace {

constexpr int HW = 60, L = 25;

template <typename T, int C>
__global__ __launch_bounds__(256) void assemble_kernel(const T* __restrict__ raw, const int32_t* __restrict__ src_row,
                                                       float* __restrict__ x_out, float* __restrict__ flag_out, float divisor,
                                                       float offset, float post_mul, float clip_max, float clip_min,
                                                       float noise) {
  constexpr int TT = L * C;                 // raw planes per pixel
  __shared__ float sv[HW * TT];             // decoded line [x][t]
  const int row = blockIdx.y, y = blockIdx.x, tid = threadIdx.x;
  const int src = src_row[row];
  float* dst = x_out + (size_t)row * L * HW * HW * C;
  if (y == 0 && tid == 0) flag_out[row] = src >= 0 ? 1.f : 0.f;
  if (src < 0) {   // absent or disabled modality: the whole row is `noise`
    for (int e = tid; e < L * HW * C; e += 256) {
      const int l = e / (HW * C), rem = e - l * (HW * C);
      dst[((size_t)l * HW + y) * HW * C + rem] = noise;
    }
    return;
  }
  const T* line = raw + ((size_t)src * HW + y) * HW * TT;
  for (int e = tid; e < HW * TT; e += 256) {
    float v = (float)line[e];
    if (clip_max > 0.f && fabsf(v) > clip_max) v = 1e-8f;
    if (clip_min > 0.f && fabsf(v) < clip_min) v = 1e-8f;
    v = v / divisor;
    if (post_mul != 1.f) v = v * post_mul;
    sv[e] = v - offset;
  }
  __syncthreads();
  for (int e = tid; e < L * HW * C; e += 256) {
    const int l = e / (HW * C), rem = e - l * (HW * C);
    const int x = rem / C, c = rem - x * C;
    dst[((size_t)l * HW + y) * HW * C + rem] = sv[x * TT + l * C + c];
  }
}

// Row gather / scatter of the mask-skipping step (GaitCore(skip_masked=True)): a modality's encoder runs on the clips whose flag is 1
// only, so their rows are gathered into a dense batch on the way in and the branch outputs / gradients scattered back on the way out.
// t is [outer][rows][row_floats] fp32 (outer = 1 for the clip tensors, 62 for the [62,B,256] features); pure byte-moving, 16 bytes per
// lane, one workgroup per (outer, gathered row) striding over the row.
template <bool SCATTER>
__global__ __launch_bounds__(256) void move_rows_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                        const int64_t* __restrict__ idx, int nidx, int src_rows, int dst_rows, size_t row_f4) {
  const int o = blockIdx.y, i = blockIdx.x;
  const int64_t r = idx[i];
  const float4* s = src + ((size_t)o * src_rows + (SCATTER ? (size_t)i : (size_t)r)) * row_f4;
  float4* d = dst + ((size_t)o * dst_rows + (SCATTER ? (size_t)r : (size_t)i)) * row_f4;
  for (size_t e = threadIdx.x; e < row_f4; e += 256) d[e] = s[e];
}

}  // namespace

static int move_rows(const float* src, const int64_t* idx, float* dst, int outer, int src_rows, int dst_rows, int nidx, size_t row_floats,
                     bool scatter, void* stream, const char* what) {
  UGN_REQUIRE(src && idx && dst && outer > 0 && nidx > 0 && src_rows > 0 && dst_rows > 0, "%s: null pointer or empty shape", what);
  UGN_REQUIRE(row_floats % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "%s: rows must be whole, 16-byte aligned float4s", what);
  UGN_REQUIRE(outer <= 65535, "%s: outer extent %d too large", what, outer);
  const dim3 grid(nidx, outer), block(256);
  if (scatter)
    hipLaunchKernelGGL(move_rows_kernel<true>, grid, block, 0, (hipStream_t)stream, (const float4*)src, (float4*)dst, idx, nidx, src_rows,
                       dst_rows, row_floats / 4);
  else
    hipLaunchKernelGGL(move_rows_kernel<false>, grid, block, 0, (hipStream_t)stream, (const float4*)src, (float4*)dst, idx, nidx, src_rows,
                       dst_rows, row_floats / 4);
  UGN_CHECK_LAUNCH(what);
  return 0;
}

extern "C" int ugn_gather_rows(const float* src, const int64_t* idx, float* dst, int outer, int src_rows, int nidx, size_t row_floats,
                               void* stream) {
  return move_rows(src, idx, dst, outer, src_rows, nidx, nidx, row_floats, false, stream, "ugn_gather_rows");
}

extern "C" int ugn_scatter_rows(const float* src, const int64_t* idx, float* dst, int outer, int dst_rows, int nidx, size_t row_floats,
                                void* stream) {
  return move_rows(src, idx, dst, outer, nidx, dst_rows, nidx, row_floats, true, stream, "ugn_scatter_rows");
}

extern "C" int ugn_assemble_modality(const void* raw, int is_int16, const int32_t* src_row, int nrows, int channels,
                                     float divisor, float offset, float post_mul, float clip_max, float clip_min, float noise,
                                     float* x_out, float* flag_out, void* stream) {
  UGN_REQUIRE(src_row && x_out && flag_out && nrows > 0, "ugn_assemble_modality: null pointer or nrows <= 0");
  UGN_REQUIRE(channels == 1 || channels == 2, "ugn_assemble_modality: channels must be 1 or 2 (got %d)", channels);
  UGN_REQUIRE(divisor != 0.f, "ugn_assemble_modality: divisor is 0");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(HW, nrows), block(256);
#define UGN_ASM(T_, C_)                                                                                                 \
  hipLaunchKernelGGL((assemble_kernel<T_, C_>), grid, block, 0, st, (const T_*)raw, src_row, x_out, flag_out, divisor, \
                     offset, post_mul, clip_max, clip_min, noise)
  if (is_int16) {
    if (channels == 2) UGN_ASM(int16_t, 2); else UGN_ASM(int16_t, 1);
  } else {
    if (channels == 2) UGN_ASM(uint8_t, 2); else UGN_ASM(uint8_t, 1);
  }
#undef UGN_ASM
  UGN_CHECK_LAUNCH("assemble_modality");
  return 0;
}

// ---- the training generator's random affine / mirror augmentation (`augmentation_x > 0`) --------------------------------
// data/mj_augmentation.py `mj_transformsequence` + `mj_mirrorsequence` on the decoded frames of a base sample, as the reference's
// `__gen_batch*` apply them (:392-450, :592-624, :712-742).  Per transformed base sample, per raw plane t (a 60x60 frame):
//   1 the Keras affine (ImageDataGenerator.apply_transform -> scipy.ndimage.affine_transform, order 1, mode 'nearest'), separable:
//     out[r][c] = bilinear(f, R(r), C(c)) through the host's row / column tap tables (index i0, weight w: (1-w) f[i0] + w f[i0+1]);
//   2 non-OF generator only: Keras channel shift, v = clip(v + cs, min, max) over the warped frame;
//   3 non-OF generator only: Keras brightness through PIL (array_to_img: (v - min) / max * 255 truncated to uint8,
//     ImageEnhance.Brightness: level = min(255, trunc(float(b) * level)), img_to_array: the level as a float);
//   4 the sequence's range fix: if max_t |out| > 3 max_t |f|, out = out / 255 - 0.5;
//   5 if flipped, columns reversed (c -> 59 - c) and the even planes negated -- mj_mirrorsequence ignores its `isof`.
// Three launches: (1) one workgroup per (plane, base sample) decodes, warps and applies 2-3, keeping per-plane |f| / |out| maxima;
// (2) one per (plane, base sample) reduces those over the sequence and applies 4-5 in place; (3) the re-layout + expansion of
// assemble_kernel, reading a transformed base sample from the scratch and decoding an untransformed one from `raw` exactly as
// assemble_kernel does (the record's per-sample clip in place of the launch-wide one).
namespace {

constexpr int FR = HW * HW;     // floats per frame
constexpr int PER_THREAD = (FR + 255) / 256;

// one base sample's record, int32 words (ugaitnet_amd/augment.py `pack_records` writes it)
enum : int { AUG_ON = 0, AUG_PHOTO = 1, AUG_FLIP = 2, AUG_CLIP_MAX = 3, AUG_CLIP_MIN = 4, AUG_CS = 5, AUG_BRIGHT = 6,
             AUG_ROW_I = 8, AUG_ROW_W = AUG_ROW_I + HW, AUG_COL_I = AUG_ROW_W + HW, AUG_COL_W = AUG_COL_I + HW,
             AUG_REC = AUG_COL_W + HW };
static_assert(AUG_REC == UGN_AUG_RECORD_WORDS, "record layout out of sync with include/ugaitnet_hip.h");

__device__ __forceinline__ float rec_f(const int32_t* rec, int k) { return __int_as_float(rec[k]); }

// assemble_kernel's decode, word for word (an untransformed sample must come out bit-identical)
template <typename T>
__device__ __forceinline__ float decode(T raw, float divisor, float offset, float post_mul, float clip_max, float clip_min) {
  float v = (float)raw;
  if (clip_max > 0.f && fabsf(v) > clip_max) v = 1e-8f;
  if (clip_min > 0.f && fabsf(v) < clip_min) v = 1e-8f;
  v = v / divisor;
  if (post_mul != 1.f) v = v * post_mul;
  return v - offset;
}

// block-wide max over 256 threads (4 wave64s); `red` holds 4 floats per call site; every thread gets the result
__device__ __forceinline__ float block_max(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return r;
}

template <typename T, int TT>
__global__ __launch_bounds__(256) void aug_warp_kernel(const T* __restrict__ raw, const int32_t* __restrict__ aug,
                                                       float* __restrict__ frames, float* __restrict__ stats, float divisor,
                                                       float offset, float post_mul) {
  __shared__ float sf[FR];
  __shared__ float red[4];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int32_t* rec = aug + (size_t)b * AUG_REC;
  if (rec[AUG_ON] == 0) return;
  const float clip_max = rec_f(rec, AUG_CLIP_MAX), clip_min = rec_f(rec, AUG_CLIP_MIN);
  const T* plane = raw + (size_t)b * FR * TT + t;
  float in_max = 0.f;
  for (int e = tid; e < FR; e += 256) {
    const float v = decode<T>(plane[(size_t)e * TT], divisor, offset, post_mul, clip_max, clip_min);
    sf[e] = v;
    in_max = fmaxf(in_max, fabsf(v));
  }
  __syncthreads();
  // 1: the affine warp; the taps were clamped to [0, 59] on the host, clamped again here so that no table can read outside the frame
  float v[PER_THREAD];
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int k = 0; k < PER_THREAD; ++k) {
    const int e = tid + 256 * k;
    if (e < FR) {
      const int r = e / HW, c = e - r * HW;
      const int r0 = min(max(rec[AUG_ROW_I + r], 0), HW - 1), r1 = min(r0 + 1, HW - 1);
      const int c0 = min(max(rec[AUG_COL_I + c], 0), HW - 1), c1 = min(c0 + 1, HW - 1);
      const float wr = rec_f(rec, AUG_ROW_W + r), wc = rec_f(rec, AUG_COL_W + c);
      const float top = (1.f - wc) * sf[r0 * HW + c0] + wc * sf[r0 * HW + c1];
      const float bot = (1.f - wc) * sf[r1 * HW + c0] + wc * sf[r1 * HW + c1];
      v[k] = (1.f - wr) * top + wr * bot;
      lo = fminf(lo, v[k]);
      hi = fmaxf(hi, v[k]);
    }
  }
  if (rec[AUG_PHOTO]) {
    // 2: channel shift, clipped to the warped frame's own range
    const float cs = rec_f(rec, AUG_CS);
    const float m = -block_max(-lo, red), M = block_max(hi, red);
    lo = INFINITY;
    hi = -INFINITY;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k)
      if (tid + 256 * k < FR) {
        v[k] = fminf(fmaxf(v[k] + cs, m), M);
        lo = fminf(lo, v[k]);
        hi = fmaxf(hi, v[k]);
      }
    // 3: brightness: to uint8 levels (a true division by the range, as numpy's `x /= x_max`), scaled and truncated as PIL does
    const float m2 = -block_max(-lo, red), M2 = block_max(hi, red);
    const float range = M2 - m2;      // = max(v - m2): subtracting a constant is monotone under rounding
    const float bright = rec_f(rec, AUG_BRIGHT);
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k)
      if (tid + 256 * k < FR) {
        float s = v[k] - m2;
        if (range != 0.f) s = s / range;
        s = s * 255.f;
        const float level = (float)(int)s;
        v[k] = (float)min(255, (int)(bright * level));
      }
  }
  float out_max = 0.f;
  float* dst = frames + ((size_t)b * TT + t) * FR;
#pragma unroll
  for (int k = 0; k < PER_THREAD; ++k) {
    const int e = tid + 256 * k;
    if (e < FR) {
      dst[e] = v[k];
      out_max = fmaxf(out_max, fabsf(v[k]));
    }
  }
  in_max = block_max(in_max, red);
  out_max = block_max(out_max, red);
  if (tid == 0) {
    stats[((size_t)b * TT + t) * 2 + 0] = in_max;
    stats[((size_t)b * TT + t) * 2 + 1] = out_max;
  }
}

template <int TT>
__global__ __launch_bounds__(256) void aug_finish_kernel(const int32_t* __restrict__ aug, float* __restrict__ frames,
                                                         const float* __restrict__ stats) {
  __shared__ float sf[FR];
  __shared__ float red[4];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int32_t* rec = aug + (size_t)b * AUG_REC;
  if (rec[AUG_ON] == 0) return;
  float in_max = 0.f, out_max = 0.f;
  for (int i = tid; i < TT; i += 256) {
    in_max = fmaxf(in_max, stats[((size_t)b * TT + i) * 2 + 0]);
    out_max = fmaxf(out_max, stats[((size_t)b * TT + i) * 2 + 1]);
  }
  in_max = block_max(in_max, red);
  out_max = block_max(out_max, red);
  // 4: `np.abs(sample_out).max() > 3 * abs_max`, compared exactly (3x a float is exact in double)
  const bool fix = (double)out_max > 3.0 * (double)in_max;
  const bool flip = rec[AUG_FLIP] != 0, negate = flip && (t % 2 == 0);
  if (!fix && !flip) return;
  float* fr = frames + ((size_t)b * TT + t) * FR;
  for (int e = tid; e < FR; e += 256) sf[e] = fr[e];
  __syncthreads();
  for (int e = tid; e < FR; e += 256) {
    const int r = e / HW, c = e - r * HW;
    float v = sf[r * HW + (flip ? HW - 1 - c : c)];
    if (fix) v = v / 255.f - 0.5f;
    if (negate) v = -v;      // 5: every even plane, whatever the modality (the reference's mirror never reads `isof`)
    fr[e] = v;
  }
}

template <typename T, int C>
__global__ __launch_bounds__(256) void aug_assemble_kernel(const T* __restrict__ raw, const int32_t* __restrict__ src_row,
                                                           const int32_t* __restrict__ aug, const float* __restrict__ frames,
                                                           float* __restrict__ x_out, float* __restrict__ flag_out, float divisor,
                                                           float offset, float post_mul, float noise) {
  constexpr int TT = L * C;
  __shared__ float sv[HW * TT];             // line y of every plane, [x][t]
  const int row = blockIdx.y, y = blockIdx.x, tid = threadIdx.x;
  const int src = src_row[row];
  float* dst = x_out + (size_t)row * L * HW * HW * C;
  if (y == 0 && tid == 0) flag_out[row] = src >= 0 ? 1.f : 0.f;
  if (src < 0) {
    for (int e = tid; e < L * HW * C; e += 256) {
      const int l = e / (HW * C), rem = e - l * (HW * C);
      dst[((size_t)l * HW + y) * HW * C + rem] = noise;
    }
    return;
  }
  const int32_t* rec = aug + (size_t)src * AUG_REC;
  if (rec[AUG_ON]) {
    const float* fr = frames + (size_t)src * TT * FR + y * HW;
    for (int e = tid; e < HW * TT; e += 256) {      // (x fastest: 240-byte runs of one frame line)
      const int t = e / HW, x = e - t * HW;
      sv[x * TT + t] = fr[(size_t)t * FR + x];
    }
  } else {
    const float clip_max = rec_f(rec, AUG_CLIP_MAX), clip_min = rec_f(rec, AUG_CLIP_MIN);
    const T* line = raw + ((size_t)src * HW + y) * HW * TT;
    for (int e = tid; e < HW * TT; e += 256) sv[e] = decode<T>(line[e], divisor, offset, post_mul, clip_max, clip_min);
  }
  __syncthreads();
  for (int e = tid; e < L * HW * C; e += 256) {
    const int l = e / (HW * C), rem = e - l * (HW * C);
    const int x = rem / C, c = rem - x * C;
    dst[((size_t)l * HW + y) * HW * C + rem] = sv[x * TT + l * C + c];
  }
}

}  // namespace

extern "C" size_t ugn_assemble_modality_aug_ws(int nbase, int channels) {
  if (nbase <= 0 || (channels != 1 && channels != 2)) return 0;
  const size_t tt = (size_t)L * channels;
  return (size_t)nbase * tt * (FR + 2) * sizeof(float);
}

extern "C" int ugn_assemble_modality_aug(const void* raw, int is_int16, const int32_t* src_row, int nrows, int nbase, int channels,
                                         float divisor, float offset, float post_mul, float noise, const int32_t* aug, float* ws,
                                         size_t ws_bytes, float* x_out, float* flag_out, void* stream) {
  UGN_REQUIRE(raw && src_row && aug && ws && x_out && flag_out && nrows > 0 && nbase > 0,
              "ugn_assemble_modality_aug: null pointer, nrows <= 0 or nbase <= 0");
  UGN_REQUIRE(channels == 1 || channels == 2, "ugn_assemble_modality_aug: channels must be 1 or 2 (got %d)", channels);
  UGN_REQUIRE(divisor != 0.f, "ugn_assemble_modality_aug: divisor is 0");
  UGN_REQUIRE(nbase <= 65535 && nrows <= 65535, "ugn_assemble_modality_aug: %d base samples / %d rows: too many", nbase, nrows);
  const size_t need = ugn_assemble_modality_aug_ws(nbase, channels);
  UGN_REQUIRE(ws_bytes >= need, "ugn_assemble_modality_aug: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  float* frames = ws;
  float* stats = ws + (size_t)nbase * L * channels * FR;
  const dim3 block(256), pgrid(L * channels, nbase), grid(HW, nrows);
#define UGN_AUG(T_, C_)                                                                                                        \
  do {                                                                                                                         \
    hipLaunchKernelGGL((aug_warp_kernel<T_, L * C_>), pgrid, block, 0, st, (const T_*)raw, aug, frames, stats, divisor, offset, \
                       post_mul);                                                                                              \
    UGN_CHECK_LAUNCH("assemble_modality_aug: warp");                                                                           \
    hipLaunchKernelGGL((aug_finish_kernel<L * C_>), pgrid, block, 0, st, aug, frames, (const float*)stats);                    \
    UGN_CHECK_LAUNCH("assemble_modality_aug: finish");                                                                         \
    hipLaunchKernelGGL((aug_assemble_kernel<T_, C_>), grid, block, 0, st, (const T_*)raw, src_row, aug, (const float*)frames,  \
                       x_out, flag_out, divisor, offset, post_mul, noise);                                                     \
    UGN_CHECK_LAUNCH("assemble_modality_aug: assemble");                                                                       \
  } while (0)
  if (is_int16) {
    if (channels == 2) UGN_AUG(int16_t, 2); else UGN_AUG(int16_t, 1);
  } else {
    if (channels == 2) UGN_AUG(uint8_t, 2); else UGN_AUG(uint8_t, 1);
  }
#undef UGN_AUG
  return 0;
}
