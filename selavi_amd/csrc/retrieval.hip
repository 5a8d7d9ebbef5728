// Video-retrieval evaluation (reference video_retrieval.py, src/retrieval_utils.py):
//   slv_pool222_f32 / slv_pool222_cl16 <- MaxPool3d / AvgPool3d((2,2,2), stride 2) + Flatten behind layer4 (:86-98)
//   slv_row_sqnorm / slv_segment_mean  <- the per-clip L2 normalisation and the per-video np.mean of average_features
//   slv_knn_select                      <- NearestNeighbors(50).kneighbors of retrieval (:410-440), after the dot
//                                          products of slv_gemm_nt: d^2 completion + k smallest per query row
#include "common.hpp"
#include "../../include/selavi_hip.h"

namespace slv {
namespace {

__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float(((unsigned)h) << 16); }

// torch's max_pool3d order: window walked t, h, w; a value replaces the running max if greater or NaN.  Avg: the same
// walk summed, divided by the window size (no padding: the divisor is always 8).
template <int AVG>
__device__ __forceinline__ float pool_step(float acc, float v) {
  if constexpr (AVG) return acc + v;
  else return (v > acc || __builtin_isnan(v)) ? v : acc;
}

// one thread per output element, in output order [N][C][To][Ho][Wo]
template <int AVG>
__global__ __launch_bounds__(256) void pool222_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int T, int H,
                                                          int W, int To, int Ho, int Wo, long long total) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const int wo = (int)(o % Wo);
  long long r = o / Wo;
  const int ho = (int)(r % Ho);
  r /= Ho;
  const int to = (int)(r % To);
  r /= To;                                               // r = n * C + c
  const float* p = x + ((r * T + 2 * to) * H + 2 * ho) * (long long)W + 2 * wo;
  float acc = AVG ? 0.f : -__builtin_inff();
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int w = 0; w < 2; ++w) acc = pool_step<AVG>(acc, p[((long long)t * H + h) * W + w]);
  y[o] = AVG ? acc / 8.f : acc;
}

// bf16 channels-last [N][T][H][W][Cp] in; one thread per output element with the channel fastest (coalesced reads),
// written to the flattened NCTHW position
template <int AVG>
__global__ __launch_bounds__(256) void pool222_cl16_kernel(const unsigned short* __restrict__ x, float* __restrict__ y, int T,
                                                           int H, int W, int C, int Cp, int To, int Ho, int Wo,
                                                           long long total) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const int c = (int)(o % C);
  long long r = o / C;
  const int wo = (int)(r % Wo);
  r /= Wo;
  const int ho = (int)(r % Ho);
  r /= Ho;
  const int to = (int)(r % To);
  const long long n = r / To;
  float acc = AVG ? 0.f : -__builtin_inff();
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        const long long pix = ((n * T + 2 * to + t) * H + 2 * ho + h) * (long long)W + 2 * wo + w;
        acc = pool_step<AVG>(acc, bf16_to_f32(x[pix * Cp + c]));
      }
  const long long P = (long long)To * Ho * Wo;
  y[(n * C + c) * P + ((long long)to * Ho + ho) * Wo + wo] = AVG ? acc / 8.f : acc;
}

// sum of squares of one row per workgroup (fp32; lanes strided, then a fixed-order wave and workgroup reduction)
__global__ __launch_bounds__(256) void row_sqnorm_kernel(const float* __restrict__ x, int D, float* __restrict__ out) {
  __shared__ float part[4];
  const float* p = x + (long long)blockIdx.x * D;
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) s += p[d] * p[d];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// out[s][d] = (sum over the segment's rows, in clip order, of x[r][d] (/ sqrt(sq[r]))) / count -- what np.mean(axis=0)
// of a float32 stack computes: one running fp32 sum per column, rows added in order
__global__ __launch_bounds__(256) void segment_mean_kernel(const float* __restrict__ x, int D, const int32_t* __restrict__ perm,
                                                           const int32_t* __restrict__ offsets, int dblocks,
                                                           const float* __restrict__ sq /* nullable */, float* __restrict__ out) {
  const long long seg = blockIdx.x / dblocks;
  const int d = (int)(blockIdx.x % dblocks) * 256 + threadIdx.x;
  if (d >= D) return;
  const int b = offsets[seg], e = offsets[seg + 1];
  float s = 0.f;
  for (int j = b; j < e; ++j) {
    const long long r = perm[j];
    float v = x[r * D + d];
    if (sq != nullptr) v = v / sqrtf(sq[r]);
    s += v;
  }
  out[seg * D + d] = s / (float)(e - b);
}

// ------------------------------------------------------------------ k smallest squared distances per query row
// The row's elements are ordered by the 64-bit key (bits of d^2 << 32 | bank index): d^2 >= 0, so its bits order like the
// value, and the index makes every key distinct (ties go to the lower index).  An MSB-first radix select (8-bit digits,
// per-wave LDS histograms) narrows the prefix of the k-th smallest key until the bin it falls in is taken whole; one more
// pass gathers the k keys at or below that prefix and a rank sort writes them ascending.  Every pass recomputes d^2 from
// the dot product with the same expression, so all passes see the same values.
constexpr int KNN_THREADS = 256;
constexpr int KNN_MAXK = 64;

__device__ __forceinline__ unsigned long long knn_key(const float* __restrict__ drow, const float* __restrict__ tn, float qn,
                                                      int j) {
  float d2 = (qn + tn[j]) - 2.f * drow[j];
  d2 = d2 > 0.f ? d2 : 0.f;                              // (also maps -0 and NaN to +0)
  return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)j;
}

__global__ __launch_bounds__(KNN_THREADS) void knn_select_kernel(const float* __restrict__ dots, long long ldd, int N,
                                                                 const float* __restrict__ q_sq, const float* __restrict__ t_sq,
                                                                 int k, float* __restrict__ d2_out, int32_t* __restrict__ idx_out) {
  __shared__ unsigned hist[4][256];
  __shared__ unsigned sel[3];                            // chosen bin, elements below it, elements in it
  __shared__ unsigned long long cand[KNN_MAXK];
  __shared__ unsigned n_cand;
  const long long row = blockIdx.x;
  const float* drow = dots + row * ldd;
  const float qn = q_sq[row];
  const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;

  unsigned long long prefix = 0;
  int depth = 0;                                         // bits of the prefix fixed so far
  unsigned need = (unsigned)k;                           // rank of the k-th key among those matching the prefix
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int i = tid; i < 4 * 256; i += KNN_THREADS) (&hist[0][0])[i] = 0u;
    __syncthreads();
    const unsigned long long want = depth ? prefix >> (64 - depth) : 0ull;
    for (int j = tid; j < N; j += KNN_THREADS) {
      const unsigned long long key = knn_key(drow, t_sq, qn, j);
      if (depth == 0 || (key >> (64 - depth)) == want) atomicAdd(&hist[wv][(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (wv == 0) {                                       // lane l owns bins 4l..4l+3
      unsigned c[4], tot = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int bin = 4 * ln + b;
        c[b] = hist[0][bin] + hist[1][bin] + hist[2][bin] + hist[3][bin];
        tot += c[b];
      }
      unsigned inc = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o, 64);
        if (ln >= o) inc += t;
      }
      unsigned before = inc - tot;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (before < need && need <= before + c[b]) {    // exactly one (lane, bin) holds the rank
          sel[0] = 4 * ln + b;
          sel[1] = before;
          sel[2] = c[b];
        }
        before += c[b];
      }
    }
    __syncthreads();
    const unsigned bin = sel[0], below = sel[1], inbin = sel[2];
    prefix |= (unsigned long long)bin << shift;
    depth += 8;
    need -= below;
    if (need == inbin) break;                            // the whole bin is selected (always true at depth 64)
  }

  if (tid == 0) n_cand = 0u;
  __syncthreads();
  const unsigned long long lim = prefix >> (64 - depth);
  for (int j = tid; j < N; j += KNN_THREADS) {
    const unsigned long long key = knn_key(drow, t_sq, qn, j);
    if ((key >> (64 - depth)) <= lim) {
      const unsigned slot = atomicAdd(&n_cand, 1u);
      if (slot < (unsigned)KNN_MAXK) cand[slot] = key;
    }
  }
  __syncthreads();
  if (tid < k) {                                         // the k keys are distinct: their ranks are a permutation
    const unsigned long long key = cand[tid];
    int rank = 0;
    for (int s = 0; s < k; ++s) rank += cand[s] < key ? 1 : 0;
    d2_out[row * k + rank] = __uint_as_float((unsigned)(key >> 32));
    idx_out[row * k + rank] = (int32_t)(unsigned)(key & 0xffffffffull);
  }
}

}  // namespace
}  // namespace slv

extern "C" {

int slv_pool222_f32(const float* x, float* out, int64_t N, int C, int T, int H, int W, int avg, slv_stream_t stream) {
  using namespace slv;
  SLV_CHECK_ARG(x && out && N > 0 && C > 0 && T >= 2 && H >= 2 && W >= 2, "null pointer or a pooled extent of 0");
  const int To = T / 2, Ho = H / 2, Wo = W / 2;
  const long long total = (long long)N * C * To * Ho * Wo;
  SLV_CHECK_ARG((total + 255) / 256 < 0x7FFFFFFFLL, "tensor too large");
  const dim3 grid((unsigned)((total + 255) / 256));
  if (avg)
    hipLaunchKernelGGL(pool222_f32_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, out, T, H, W, To, Ho, Wo, total);
  else
    hipLaunchKernelGGL(pool222_f32_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, x, out, T, H, W, To, Ho, Wo, total);
  SLV_LAUNCH_CHECK();
  return 0;
}

int slv_pool222_cl16(const void* x_bf16, float* out, int64_t N, int T, int H, int W, int C, int Cp, int avg,
                     slv_stream_t stream) {
  using namespace slv;
  SLV_CHECK_ARG(x_bf16 && out && N > 0 && C > 0 && Cp >= C && T >= 2 && H >= 2 && W >= 2,
                "null pointer, C > Cp or a pooled extent of 0");
  const int To = T / 2, Ho = H / 2, Wo = W / 2;
  const long long total = (long long)N * C * To * Ho * Wo;
  SLV_CHECK_ARG((total + 255) / 256 < 0x7FFFFFFFLL, "tensor too large");
  const dim3 grid((unsigned)((total + 255) / 256));
  const unsigned short* x = (const unsigned short*)x_bf16;
  if (avg)
    hipLaunchKernelGGL(pool222_cl16_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, out, T, H, W, C, Cp, To, Ho, Wo, total);
  else
    hipLaunchKernelGGL(pool222_cl16_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, x, out, T, H, W, C, Cp, To, Ho, Wo, total);
  SLV_LAUNCH_CHECK();
  return 0;
}

int slv_row_sqnorm(const float* x, int64_t rows, int D, float* out, slv_stream_t stream) {
  using namespace slv;
  SLV_CHECK_ARG(x && out && rows > 0 && rows < 0x7FFFFFFFLL && D > 0, "null pointer or bad shape");
  hipLaunchKernelGGL(row_sqnorm_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, D, out);
  SLV_LAUNCH_CHECK();
  return 0;
}

int slv_segment_mean(const float* x, int64_t rows, int D, const int32_t* perm, const int32_t* offsets, int64_t n_seg,
                     int normalize, float* ws, float* out, float* out_sqnorm, slv_stream_t stream) {
  using namespace slv;
  SLV_CHECK_ARG(x && perm && offsets && out && rows > 0 && rows < 0x7FFFFFFFLL && D > 0 && n_seg > 0 && n_seg <= rows,
                "null pointer or bad shape");
  SLV_CHECK_ARG(!normalize || ws, "normalize needs the rows-float workspace");
  const int dblocks = (D + 255) / 256;
  SLV_CHECK_ARG(n_seg * dblocks < 0x7FFFFFFFLL, "too many segments");
  if (normalize) {
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, D, ws);
    SLV_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(segment_mean_kernel, dim3((unsigned)(n_seg * dblocks)), dim3(256), 0, (hipStream_t)stream, x, D, perm,
                     offsets, dblocks, normalize ? ws : nullptr, out);
  SLV_LAUNCH_CHECK();
  if (out_sqnorm) {
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((unsigned)n_seg), dim3(256), 0, (hipStream_t)stream, out, D, out_sqnorm);
    SLV_LAUNCH_CHECK();
  }
  return 0;
}

int slv_knn_select(const float* dots, int64_t ldd, int64_t rows, int N, const float* q_sqnorm, const float* t_sqnorm, int k,
                   float* d2_out, int32_t* idx_out, slv_stream_t stream) {
  using namespace slv;
  SLV_CHECK_ARG(dots && q_sqnorm && t_sqnorm && d2_out && idx_out, "null pointer");
  SLV_CHECK_ARG(rows > 0 && rows < 0x7FFFFFFFLL && N > 0 && ldd >= N, "bad shape");
  SLV_CHECK_ARG(k >= 1 && k <= KNN_MAXK && k <= N, "k must be in [1, min(64, N)]");
  hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)rows), dim3(KNN_THREADS), 0, (hipStream_t)stream, dots, (long long)ldd,
                     N, q_sqnorm, t_sqnorm, k, d2_out, idx_out);
  SLV_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
