// Input pipeline on the device: what the reference's DataLoader workers do on the CPU for
// every clip, as two HBM-bound kernels over a whole batch.
//
//   slv_clip_augment   datasets/video_transforms.py:462-510  uint8 THWC frames -> normalised, short-side-resized
//                      (bilinear, align_corners=False), cropped, optionally flipped float32 CTHW clip.  One read
//                      of the source bytes, one write of the clip; the reference materialises four intermediates.
//   slv_clip_augment_color  the same plus color_jitter (:273-363) and grayscale (:251-270, :498-500): the stage chain
//                      runs in registers behind the sampling; a contrast stage needs the mean gray value of each frame
//                      first, which a pass of its own recomputes from the uint8 source (no float clip is read back).
//   slv_clip_sample_augment[_color]  the same two, reading frame fidx[b][t] of a whole decoded video instead of frame t
//                      of a T-frame clip (datasets/decoder.py:21-38 temporal_sampling folded into the read): no gathered
//                      copy of the clip is written and read back, and several output clips may name one resident video.
//   slv_logfbank       datasets/audio_utils.py:46-72 -> python_speech_features.logfbank (0.6): pre-emphasis, framing
//                      (rectangular window), |rfft|^2/nfft, triangular mel filterbank, log -- in float64 like numpy,
//                      stored as float32 [B][1][nfilt][frames].
#include "common.hpp"

namespace slv {

// ---- video --------------------------------------------------------------------------------------------------------
struct ClipDesc {           // one per clip, int64 x 8 on the device
  long long src_off;        // byte offset of this clip's T*H*W*3 frames in the source buffer
  long long H, W;           // source size
  long long nh, nw;         // size after the short-side resize (== H, W: no resize)
  long long y_off, x_off;   // crop origin in the resized image
  long long flip;
};

// torch's bilinear coefficients (aten UpSample.h, align_corners=False), in float32 with the source index formed by
// one fused multiply-add -- bit-identical to the CPU build the reference runs on (oracle/input_ref.py:_axis)
__device__ __forceinline__ void axis_coef(int dst, int n_in, int n_out, int& i0, int& i1, float& w0, float& w1) {
  const float scale = (float)n_in / (float)n_out;
  float src = __fmaf_rn(scale, (float)dst + 0.5f, -0.5f);
  src = fmaxf(src, 0.f);
  i0 = min((int)src, n_in - 1);
  w1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
  w0 = 1.f - w1;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
}

__device__ __forceinline__ float norm_px(unsigned char v, float mean, float stdv) {
  return ((float)v / 255.0f - mean) / stdv;      // video_transforms.py:475-478, one rounding per step like torch
}

// one output pixel of frame f (all three channels: the source is channel-interleaved) at row ry / column rx of the
// resized image -- the spatial sampling every kernel below shares
__device__ __forceinline__ void sample_px(const unsigned char* __restrict__ f, int H, int W, int nh, int nw, int ry,
                                          int rx, const float (&mean)[3], const float (&stdv)[3], float (&px)[3]) {
  if (nh == H && nw == W) {                      // random_short_side_scale_jitter returned the images unchanged
    const unsigned char* q = f + ((size_t)ry * W + rx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = norm_px(q[c], mean[c], stdv[c]);
    return;
  }
  int y0, y1, x0, x1;
  float wy0, wy1, wx0, wx1;
  axis_coef(ry, H, nh, y0, y1, wy0, wy1);
  axis_coef(rx, W, nw, x0, x1, wx0, wx1);
  const unsigned char *q00 = f + ((size_t)y0 * W + x0) * 3, *q01 = f + ((size_t)y0 * W + x1) * 3,
                      *q10 = f + ((size_t)y1 * W + x0) * 3, *q11 = f + ((size_t)y1 * W + x1) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p00 = norm_px(q00[c], mean[c], stdv[c]), p01 = norm_px(q01[c], mean[c], stdv[c]);
    const float p10 = norm_px(q10[c], mean[c], stdv[c]), p11 = norm_px(q11[c], mean[c], stdv[c]);
    const float top = __fmaf_rn(p00, wx0, p01 * wx1), bot = __fmaf_rn(p10, wx0, p11 * wx1);
    px[c] = __fmaf_rn(top, wy0, bot * wy1);
  }
}

// Thread = one output pixel, all three channels.  kTable = false (slv_clip_augment): grid (ceil(S*S/256), T, B), clip b
// holds exactly T frames and output frame t reads frame t.  kTable = true (slv_clip_sample_augment): clip b names a whole
// video and output frame t reads frame fidx[b * T + t] of it (checked against the video's length on the host).
//
// Grid order with a table: (ceil(S*S/256), B, T), the clip index in front of the frame slot.  Output clips that share a
// video are neighbours in b (the two clips of a dual_data sample, the spatial crops of one test view), and the crops of
// one view read the SAME source frame in slot t.  With b next to the tile index their workgroups are dispatched back to
// back (49 tiles apart at crop 112) and are resident together, so the second and third crop find the frame's bytes in
// the L2 of the XCD they land on or in the Infinity Cache; in the (T, B) order of the clip kernel they would be a whole
// clip (T x tiles workgroups) apart.  Workgroups are dealt round-robin over the eight XCDs, so every XCD's L2 fetches a
// frame once either way; the order decides only how soon the re-reads follow.  The four bilinear taps stay single-byte
// loads: a pixel is three bytes, so a tap is never aligned for a wider access, neighbouring lanes read neighbouring
// pixels of the same two source rows (the wave's loads fall into the same few cache lines), and per thread they stand
// next to 24 IEEE divides and three float stores.
template <bool kTable>
__global__ __launch_bounds__(256) void clip_augment_kernel(const unsigned char* __restrict__ src,
                                                           const ClipDesc* __restrict__ desc,
                                                           const int* __restrict__ fidx, float* __restrict__ out,
                                                           int T, int S, float m0, float m1, float m2, float s0,
                                                           float s1, float s2) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= S * S) return;
  const int oy = p / S, ox = p - oy * S;
  const int t = kTable ? blockIdx.z : blockIdx.y, b = kTable ? blockIdx.y : blockIdx.z;
  const ClipDesc d = desc[b];
  const int H = (int)d.H, W = (int)d.W;
  const int ry = oy + (int)d.y_off, rx = (d.flip ? S - 1 - ox : ox) + (int)d.x_off;
  const int fr = kTable ? fidx[(size_t)b * T + t] : t;
  const unsigned char* f = src + d.src_off + (size_t)fr * H * W * 3;
  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
  float* o = out + (((size_t)b * 3) * T + t) * S * S + p;
  const size_t cstride = (size_t)T * S * S;
  float px[3];
  sample_px(f, H, W, (int)d.nh, (int)d.nw, ry, rx, mean, stdv, px);
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * cstride] = px[c];
}

// ---- colour jitter / grayscale (video_transforms.py:251-363, :491-500) ------------------------------------------------
// Every product and every sum below is rounded on its own, in the order torch evaluates them on the T x 3 x S x S float32
// clip (images * alpha + other * (1 - alpha), the two scalars rounded to float32 on the host): __fmul_rn / __fadd_rn are
// never contracted into a fused multiply-add.
enum { CJ_NONE = 0, CJ_BRIGHTNESS = 1, CJ_CONTRAST = 2, CJ_SATURATION = 3 };
struct ColorDesc {          // one per clip, 12 x 32 bit on the device (and, for the argument checks, on the host)
  int stage[3];             // CJ_* in application order
  int gray;                 // grayscale(frames) after the stages (:498-500)
  float alpha[3];           // (float)alpha of stage i
  float beta[3];            // (float)(1.0 - alpha) of stage i, formed in float64 on the host
  int pad[2];
};

// grayscale (:262-266): the indices as written there (the function assumes BGR), summed left to right
__device__ __forceinline__ float gray_px(const float (&px)[3]) {
  return __fadd_rn(__fadd_rn(__fmul_rn(0.299f, px[2]), __fmul_rn(0.587f, px[1])), __fmul_rn(0.114f, px[0]));
}

// blend (:248) with an image that is the same in its three channels
__device__ __forceinline__ void blend_px(float (&px)[3], float other, float alpha, float beta) {
  const float o = __fmul_rn(other, beta);
#pragma unroll
  for (int c = 0; c < 3; ++c) px[c] = __fadd_rn(__fmul_rn(px[c], alpha), o);
}

// stages [0, n) of one clip's chain on one pixel; frame_mean: the gray mean of this frame for the contrast stage
__device__ __forceinline__ void color_stages(float (&px)[3], const ColorDesc& cd, int n, float frame_mean) {
  for (int i = 0; i < n; ++i) {
    const int st = cd.stage[i];
    if (st == CJ_BRIGHTNESS) blend_px(px, 0.f, cd.alpha[i], cd.beta[i]);
    else if (st == CJ_CONTRAST) blend_px(px, frame_mean, cd.alpha[i], cd.beta[i]);
    else if (st == CJ_SATURATION) blend_px(px, gray_px(px), cd.alpha[i], cd.beta[i]);
  }
}

// pass 1 -- grid (T, B), GM_THREADS threads: the mean gray value of frame t as clip b stands in front of its contrast
// stage (:341-342; the mean over three equal channels is the mean over the pixels).  float64, fixed order: thread i sums
// pixels i, i + GM_THREADS, ... and the partial sums go through a fixed tree, so every launch gives the same bits.
// 1024 threads: a (clip, frame) is one workgroup, so a batch of 16 x 16 is one workgroup per CU, and the sampling is
// ALU-bound per pixel (24 IEEE divides) -- four waves per SIMD instead of one to overlap it with the byte loads.
// kTable: the frame comes through the frame table, as in clip_augment_kernel; the sum and its order are the same.
constexpr int GM_THREADS = 1024;
template <bool kTable>
__global__ __launch_bounds__(GM_THREADS) void clip_gray_mean_kernel(const unsigned char* __restrict__ src,
                                                             const ClipDesc* __restrict__ desc,
                                                             const ColorDesc* __restrict__ color,
                                                             const int* __restrict__ fidx,
                                                             float* __restrict__ frame_mean, int T, int S, float m0,
                                                             float m1, float m2, float s0, float s1, float s2) {
  __shared__ double part[GM_THREADS];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const ColorDesc cd = color[b];
  int k = -1;
  for (int i = 0; i < 3; ++i)
    if (cd.stage[i] == CJ_CONTRAST && k < 0) k = i;
  if (k < 0) return;                             // block-uniform: no barrier has been reached
  const ClipDesc d = desc[b];
  const int H = (int)d.H, W = (int)d.W, nh = (int)d.nh, nw = (int)d.nw;
  const int fr = kTable ? fidx[(size_t)b * T + t] : t;
  const unsigned char* f = src + d.src_off + (size_t)fr * H * W * 3;
  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
  double acc = 0.0;
  for (int p = tid; p < S * S; p += GM_THREADS) {
    const int oy = p / S, ox = p - oy * S;
    const int ry = oy + (int)d.y_off, rx = (d.flip ? S - 1 - ox : ox) + (int)d.x_off;
    float px[3];
    sample_px(f, H, W, nh, nw, ry, rx, mean, stdv, px);
    color_stages(px, cd, k, 0.f);
    acc += (double)gray_px(px);
  }
  part[tid] = acc;
  __syncthreads();
  for (int w = GM_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) part[tid] += part[tid + w];
    __syncthreads();
  }
  if (tid == 0) frame_mean[(size_t)b * T + t] = (float)(part[0] / (double)((long long)S * S));
}

// pass 2 -- the grid of clip_augment_kernel (with a table: its (tiles, B, T) order): sampling, the whole chain and the
// grayscale flag in registers, one write of the clip
template <bool kTable>
__global__ __launch_bounds__(256) void clip_augment_color_kernel(const unsigned char* __restrict__ src,
                                                                 const ClipDesc* __restrict__ desc,
                                                                 const ColorDesc* __restrict__ color,
                                                                 const int* __restrict__ fidx,
                                                                 const float* __restrict__ frame_mean,
                                                                 float* __restrict__ out, int T, int S, float m0,
                                                                 float m1, float m2, float s0, float s1, float s2) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= S * S) return;
  const int oy = p / S, ox = p - oy * S;
  const int t = kTable ? blockIdx.z : blockIdx.y, b = kTable ? blockIdx.y : blockIdx.z;
  const ClipDesc d = desc[b];
  const ColorDesc cd = color[b];
  const int H = (int)d.H, W = (int)d.W;
  const int ry = oy + (int)d.y_off, rx = (d.flip ? S - 1 - ox : ox) + (int)d.x_off;
  const int fr = kTable ? fidx[(size_t)b * T + t] : t;
  const unsigned char* f = src + d.src_off + (size_t)fr * H * W * 3;
  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
  float px[3];
  sample_px(f, H, W, (int)d.nh, (int)d.nw, ry, rx, mean, stdv, px);
  const bool contrast = cd.stage[0] == CJ_CONTRAST || cd.stage[1] == CJ_CONTRAST || cd.stage[2] == CJ_CONTRAST;
  color_stages(px, cd, 3, contrast ? frame_mean[(size_t)b * T + t] : 0.f);
  if (cd.gray) px[0] = px[1] = px[2] = gray_px(px);
  float* o = out + (((size_t)b * 3) * T + t) * S * S + p;
  const size_t cstride = (size_t)T * S * S;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * cstride] = px[c];
}

// ---- audio --------------------------------------------------------------------------------------------------------
constexpr int FB_MAX_FRAME = 2048, FB_MAX_NFFT = 2048;

// grid (nframes, B), 256 threads.  LDS: the pre-emphasised frame, the twiddle table, the power spectrum.
__global__ __launch_bounds__(256) void logfbank_kernel(const short* __restrict__ wav, const long long* __restrict__ start,
                                                       const double* __restrict__ volume, long long wav_stride,
                                                       int slen, int frame_len, int frame_step, int nfft, int nfilt,
                                                       const double* __restrict__ twiddle,   // cos[nfft], sin[nfft]
                                                       const int* __restrict__ bins,         // nfilt + 2
                                                       double preemph, int z_normalize, float* __restrict__ out,
                                                       int nframes) {
  extern __shared__ double lds[];
  double* x = lds;                         // frame_len
  double* tc = x + frame_len;              // nfft
  double* ts = tc + nfft;                  // nfft
  double* ps = ts + nfft;                  // nfft/2 + 1
  const int fr = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const short* w = wav + (size_t)b * wav_stride + start[b];
  const double vol = volume ? volume[b] : 1.0;
  const bool scaled = volume != nullptr;
  for (int i = tid; i < frame_len; i += 256) {
    const int n = fr * frame_step + i;     // sample index inside the (zero-padded) signal
    double v = 0.0;
    if (n < slen) {                        // sigproc.preemphasis: s[0], s[n] - coeff*s[n-1]
      const double cur = scaled ? (double)w[n] * vol : (double)w[n];
      if (n == 0) v = cur;
      else {
        const double prev = scaled ? (double)w[n - 1] * vol : (double)w[n - 1];
        v = cur - preemph * prev;
      }
    }
    x[i] = v;
  }
  for (int i = tid; i < nfft; i += 256) {
    tc[i] = twiddle[i];
    ts[i] = twiddle[nfft + i];
  }
  __syncthreads();
  const int nbin = nfft / 2 + 1, mask = nfft - 1;
  for (int k = tid; k < nbin; k += 256) {
    double re = 0.0, im = 0.0;
    int idx = 0;
    for (int n = 0; n < frame_len; ++n) {
      re = fma(x[n], tc[idx], re);
      im = fma(x[n], ts[idx], im);
      idx = (idx + k) & mask;
    }
    ps[k] = (re * re + im * im) * (1.0 / nfft);
  }
  __syncthreads();
  for (int j = tid; j < nfilt; j += 256) {
    const int b0 = bins[j], b1 = bins[j + 1], b2 = bins[j + 2];
    double acc = 0.0;
    for (int i = b0; i < b1; ++i) acc += ps[i] * ((double)(i - b0) / (double)(b1 - b0));
    for (int i = b1; i < b2; ++i) acc += ps[i] * ((double)(b2 - i) / (double)(b2 - b1));
    if (acc == 0.0) acc = 2.220446049250313e-16;   // numpy.finfo(float).eps
    float v = (float)log(acc);
    if (z_normalize) v = (v - 1.93f) / 17.89f;     // audio_utils.py:71-72
    out[((size_t)b * nfilt + j) * nframes + fr] = v;
  }
}

}  // namespace slv

extern "C" {

// the launches behind the four video entry points; fidx == nullptr: the clip kernels (frame t of a T-frame clip)
// (fn: the entry point's name, for the error text)
static int launch_clip_augment(const char* fn, const void* frames_u8, const int64_t* desc, const int32_t* fidx, float* out,
                               int B, int T, int S, const float* mean3, const float* std3, void* stream) {
  using namespace slv;
  const unsigned tiles = cdiv((long)S * S, 256);
  if (fidx) {
    hipLaunchKernelGGL(clip_augment_kernel<true>, dim3(tiles, B, T), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)frames_u8, (const ClipDesc*)desc, (const int*)fidx, (float*)out, T, S,
                       mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
  } else {
    hipLaunchKernelGGL(clip_augment_kernel<false>, dim3(tiles, T, B), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)frames_u8, (const ClipDesc*)desc, (const int*)nullptr, (float*)out, T, S,
                       mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
  }
  return launch_check(fn);
}

// the argument checks of the colour words (host copy); *any_contrast: whether pass 1 is needed
// SLV_CHECK_ARG for the helpers below: the message names the entry point (fn), which has noted pending errors already
#define SLV_CHECK_ARG_FN(cond, msg) \
  do {                             \
    if (!(cond)) return ::slv::fail(-2, "%s: bad argument: " msg, fn); \
  } while (0)
static int check_color_host(const char* fn, const void* color_host, int B, bool* any_contrast) {
  using namespace slv;
  const ColorDesc* ch = (const ColorDesc*)color_host;
  *any_contrast = false;
  for (int b = 0; b < B; ++b) {
    int n_contrast = 0;
    for (int i = 0; i < 3; ++i) {
      SLV_CHECK_ARG_FN(ch[b].stage[i] >= CJ_NONE && ch[b].stage[i] <= CJ_SATURATION, "unknown stage code");
      n_contrast += ch[b].stage[i] == CJ_CONTRAST;
    }
    SLV_CHECK_ARG_FN(n_contrast <= 1, "more than one contrast stage in a clip");
    *any_contrast = *any_contrast || n_contrast;
  }
  return 0;
}

static int launch_clip_augment_color(const char* fn, const void* frames_u8, const int64_t* desc, const void* color, const int32_t* fidx,
                                     bool any_contrast, float* frame_mean_ws, float* out, int B, int T, int S,
                                     const float* mean3, const float* std3, void* stream) {
  using namespace slv;
  const unsigned tiles = cdiv((long)S * S, 256);
  if (any_contrast) {
    if (fidx)
      hipLaunchKernelGGL(clip_gray_mean_kernel<true>, dim3(T, B), dim3(GM_THREADS), 0, (hipStream_t)stream,
                         (const unsigned char*)frames_u8, (const ClipDesc*)desc, (const ColorDesc*)color,
                         (const int*)fidx, frame_mean_ws, T, S, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    else
      hipLaunchKernelGGL(clip_gray_mean_kernel<false>, dim3(T, B), dim3(GM_THREADS), 0, (hipStream_t)stream,
                         (const unsigned char*)frames_u8, (const ClipDesc*)desc, (const ColorDesc*)color,
                         (const int*)nullptr, frame_mean_ws, T, S, mean3[0], mean3[1], mean3[2], std3[0], std3[1],
                         std3[2]);
    if (int rc = launch_check(fn)) return rc;
  }
  if (fidx)
    hipLaunchKernelGGL(clip_augment_color_kernel<true>, dim3(tiles, B, T), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)frames_u8, (const ClipDesc*)desc, (const ColorDesc*)color, (const int*)fidx,
                       frame_mean_ws, (float*)out, T, S, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
  else
    hipLaunchKernelGGL(clip_augment_color_kernel<false>, dim3(tiles, T, B), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)frames_u8, (const ClipDesc*)desc, (const ColorDesc*)color,
                       (const int*)nullptr, frame_mean_ws, (float*)out, T, S, mean3[0], mean3[1], mean3[2], std3[0],
                       std3[1], std3[2]);
  return launch_check(fn);
}

// every entry of the host copy of the frame table against the length of the video its clip names
static int check_frame_table(const char* fn, const int32_t* fidx_host, const int64_t* n_frames_host, int B, int T) {
  for (int b = 0; b < B; ++b) {
    SLV_CHECK_ARG_FN(n_frames_host[b] > 0, "a video without frames");
    for (int t = 0; t < T; ++t) {
      const int32_t i = fidx_host[(size_t)b * T + t];
      SLV_CHECK_ARG_FN(i >= 0 && (int64_t)i < n_frames_host[b], "frame index outside the video");
    }
  }
  return 0;
}
#undef SLV_CHECK_ARG_FN

int slv_clip_augment(const void* frames_u8, const int64_t* desc, float* out, int B, int T, int S,
                     const float* mean3, const float* std3, void* stream) {
  SLV_CHECK_ARG(frames_u8 && desc && out && mean3 && std3, "null pointer");
  SLV_CHECK_ARG(B > 0 && T > 0 && S > 0 && B <= 65535 && T <= 65535, "bad sizes");
  return launch_clip_augment(__func__, frames_u8, desc, nullptr, out, B, T, S, mean3, std3, stream);
}

int slv_clip_augment_color(const void* frames_u8, const int64_t* desc, const void* color, const void* color_host,
                           float* frame_mean_ws, float* out, int B, int T, int S, const float* mean3,
                           const float* std3, void* stream) {
  SLV_CHECK_ARG(frames_u8 && desc && color && color_host && out && mean3 && std3, "null pointer");
  SLV_CHECK_ARG(B > 0 && T > 0 && S > 0 && B <= 65535 && T <= 65535, "bad sizes");
  bool any_contrast = false;
  if (int rc = check_color_host(__func__, color_host, B, &any_contrast)) return rc;
  SLV_CHECK_ARG(!any_contrast || frame_mean_ws, "a contrast stage needs the B x T frame-mean workspace");
  return launch_clip_augment_color(__func__, frames_u8, desc, color, nullptr, any_contrast, frame_mean_ws, out, B, T, S, mean3,
                                   std3, stream);
}

int slv_clip_sample_augment(const void* frames_u8, const int64_t* desc, const int32_t* fidx, const int32_t* fidx_host,
                            const int64_t* n_frames_host, float* out, int B, int T, int S, const float* mean3,
                            const float* std3, void* stream) {
  SLV_CHECK_ARG(frames_u8 && desc && fidx && fidx_host && n_frames_host && out && mean3 && std3, "null pointer");
  SLV_CHECK_ARG(B > 0 && T > 0 && S > 0 && B <= 65535 && T <= 65535, "bad sizes");
  if (int rc = check_frame_table(__func__, fidx_host, n_frames_host, B, T)) return rc;
  return launch_clip_augment(__func__, frames_u8, desc, fidx, out, B, T, S, mean3, std3, stream);
}

int slv_clip_sample_augment_color(const void* frames_u8, const int64_t* desc, const int32_t* fidx,
                                  const int32_t* fidx_host, const int64_t* n_frames_host, const void* color,
                                  const void* color_host, float* frame_mean_ws, float* out, int B, int T, int S,
                                  const float* mean3, const float* std3, void* stream) {
  SLV_CHECK_ARG(frames_u8 && desc && fidx && fidx_host && n_frames_host && color && color_host && out && mean3 && std3,
                "null pointer");
  SLV_CHECK_ARG(B > 0 && T > 0 && S > 0 && B <= 65535 && T <= 65535, "bad sizes");
  if (int rc = check_frame_table(__func__, fidx_host, n_frames_host, B, T)) return rc;
  bool any_contrast = false;
  if (int rc = check_color_host(__func__, color_host, B, &any_contrast)) return rc;
  SLV_CHECK_ARG(!any_contrast || frame_mean_ws, "a contrast stage needs the B x T frame-mean workspace");
  return launch_clip_augment_color(__func__, frames_u8, desc, color, fidx, any_contrast, frame_mean_ws, out, B, T, S, mean3, std3,
                                   stream);
}

int32_t slv_logfbank_frames(int slen, int frame_len, int frame_step) {
  if (slen <= 0 || frame_len <= 0 || frame_step <= 0) return -1;
  if (slen <= frame_len) return 1;
  return 1 + (int)((slen - frame_len + frame_step - 1) / frame_step);
}

int slv_logfbank(const void* wav_i16, const int64_t* start_i64, const double* volume_f64, int64_t wav_stride, int B,
                 int slen, int frame_len, int frame_step, int nfft, int nfilt, const double* twiddle_f64,
                 const int32_t* bins_i32, double preemph, int z_normalize, float* out_f32, void* stream) {
  using namespace slv;
  SLV_CHECK_ARG(wav_i16 && start_i64 && twiddle_f64 && bins_i32 && out_f32, "null pointer");
  SLV_CHECK_ARG(B > 0 && B <= 65535 && slen > 0 && nfilt > 0, "bad sizes");
  SLV_CHECK_ARG(nfft > 0 && (nfft & (nfft - 1)) == 0 && nfft <= FB_MAX_NFFT, "nfft must be a power of two <= 2048");
  SLV_CHECK_ARG(frame_len > 0 && frame_len <= nfft && frame_len <= FB_MAX_FRAME && frame_step > 0,
                "frame length must not exceed nfft");
  const int nframes = slv_logfbank_frames(slen, frame_len, frame_step);
  const size_t lds = sizeof(double) * ((size_t)frame_len + 2 * (size_t)nfft + nfft / 2 + 1);
  hipLaunchKernelGGL(logfbank_kernel, dim3(nframes, B), dim3(256), lds, (hipStream_t)stream, (const short*)wav_i16,
                     (const long long*)start_i64, (const double*)volume_f64, wav_stride, slen, frame_len, frame_step,
                     nfft, nfilt, (const double*)twiddle_f64, (const int*)bins_i32, preemph, z_normalize,
                     (float*)out_f32, nframes);
  SLV_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
