// Fine-tuning for action recognition (finetune_video.py of the reference): the classifier head of Finetune_Model
// (:83-92) fused with its loss and accuracy epilogue, its backward, the top-k rank count of utils.accuracy /
// aggregrate_video_accuracy (utils.py:336-374) and multi-tensor optimizer steps with per-tensor hyperparameters (the
// reference's one-param-group-per-tensor optimizer, :150-173 and :259-271).
//
// Head, per row b of the [B, 512] trunk features x:
//   u = x / max(||x||, 1e-12)                 (use_l2_norm; else u = x)
//   v = (u - mean) * invstd * gamma + beta    (use_bn; train: batch statistics, running update; eval: running statistics)
//   y = v * keep * 1/(1-p)                    (use_dropout, train; keep from Philox on (seed, offset), element b*512+c)
//   z = W y + bias                            (Linear(512, K))
// then per-row softmax cross-entropy, dlogits = (softmax - onehot) / B and the target's rank.
//
// Two paths, same device phases:
//   B <= 64: ONE workgroup of 1024 threads runs every phase, with the [B][512] fp32 rows resident in LDS (128 KiB of the
//            CU's 160 KiB) and __syncthreads between phases: forward + epilogue is one launch, backward one launch.
//   B > 64:  the phases as separate launches over the whole chip (forward: statistics (train + BN only), rows, totals;
//            backward: elementwise, column reductions, rows), with the rows in global workspaces.
//
// Rank rule (deterministic, unlike torch.topk's order on ties): target t of a row z is in the top k iff
//   #{j : z_j > z_t} + #{j < t : z_j == z_t} < k
// i.e. ties are broken towards the lower class index.  A target outside [0, K) counts as wrong (its loss is NaN).
#include "common.hpp"
#include "philox.hpp"
#include "../../include/selavi_hip.h"

namespace slv {

constexpr int FD = 512;           // feature width of the r2plus1d_18 trunk (get_video_dim)
constexpr int FJ = FD / 64;       // values of a row per lane
constexpr int SMALL_B = 64;       // rows of the one-workgroup path
constexpr int SMALL_T = 1024;

struct FtFwd {
  const float* x;
  const float* W;
  const float* bias;
  const float* gamma;
  const float* beta;
  float* rmean;
  float* rvar;
  const float* mask;              // injected keep mask [B][FD] (nullable: Philox)
  unsigned long long seed, offset;
  unsigned thresh;
  float msc;                      // 1/(1-p); dropout is on iff drop != 0
  const int64_t* target;          // nullable: no loss / accuracy epilogue
  float* logits;                  // [B][K]
  float* u;                       // [B][FD] saved: rows after the L2 normalisation
  float* norms;                   // [B] saved: max(||x||, eps) (1 without L2)
  float* mi;                      // [2][FD] saved: BN mean, invstd
  float* dlogits;                 // [B][K] nullable
  float* loss_rows;               // [B]
  float* corr_rows;               // [B][2]
  float* loss;                    // [1]
  float* correct;                 // [2]: correct@1, correct@5 counts
  float gscale, momentum, eps;
  int B, K, l2, bn, train, drop;
};

struct FtBwd {
  const float* dz_ext;            // incoming dlogits (nullable)
  const float* dl_saved;          // forward's dlogits (nullable), scaled by *gout
  const float* gout;
  const float* u;
  const float* norms;
  const float* mi;
  const float* W;
  const float* gamma;
  const float* beta;
  const float* mask;
  unsigned long long seed, offset;
  unsigned thresh;
  float msc;
  float* dW;                      // [K][FD]
  float* db;                      // [K]
  float* dgamma;                  // [FD] (BN only)
  float* dbeta;                   // [FD] (BN only)
  float* dfeat;                   // [B][FD]
  float* ybuf;                    // [B][FD] workspace of the B > 64 path
  float* dvbuf;                   // [B][FD] workspace of the B > 64 path
  int B, K, l2, bn, train, drop;
};

__device__ __forceinline__ float keep_of(const float* mask, unsigned long long seed, unsigned long long off,
                                         unsigned thresh, size_t e) {
  if (mask) return mask[e];
  const size_t blk = e >> 2;
  unsigned r[4];
  philox4x32_10((unsigned)blk, (unsigned)(blk >> 32), (unsigned)off, (unsigned)(off >> 32), (unsigned)seed,
                (unsigned)(seed >> 32), r);
  const unsigned w = (e & 3) == 0 ? r[0] : (e & 3) == 1 ? r[1] : (e & 3) == 2 ? r[2] : r[3];
  return w >= thresh ? 1.f : 0.f;
}

// rank of target t in row z (the rule at the top), one wave; every lane gets it
__device__ __forceinline__ int target_rank(const float* __restrict__ z, int K, int t, int lane) {
  const float zt = z[t];
  int cnt = 0;
  for (int k = lane; k < K; k += 64) {
    const float v = z[k];
    cnt += (v > zt || (v == zt && k < t)) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  return cnt;
}

// ---- forward phases
// u and norms of row b (lane holds columns lane + 64 j)
__device__ __forceinline__ void row_u(const FtFwd& a, int b, int lane, float (&v)[FJ]) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < FJ; ++j) {
    v[j] = a.x[(size_t)b * FD + lane + 64 * j];
    s += v[j] * v[j];
  }
  if (a.l2) {
    s = wave_sum(s);
    const float n = fmaxf(sqrtf(s), 1e-12f);
#pragma unroll
    for (int j = 0; j < FJ; ++j) v[j] = v[j] / n;
    if (lane == 0) a.norms[b] = n;
  } else if (lane == 0) {
    a.norms[b] = 1.f;
  }
}

// rows -> u (saved, and into arr when it is not the saved buffer), one wave per row
__device__ void phase_u(const FtFwd& a, float* arr, int wave, int nwaves, int lane) {
  for (int b = wave; b < a.B; b += nwaves) {
    float v[FJ];
    row_u(a, b, lane, v);
#pragma unroll
    for (int j = 0; j < FJ; ++j) {
      a.u[(size_t)b * FD + lane + 64 * j] = v[j];
      if (arr != a.u) arr[(size_t)b * FD + lane + 64 * j] = v[j];
    }
  }
}

// BatchNorm1d statistics of column c (train: batch, biased variance to normalise, unbiased into running_var; eval: running)
__device__ void phase_stats(const FtFwd& a, const float* arr, int tid, int nthreads) {
  for (int c = tid; c < FD; c += nthreads) {
    float mean, invstd;
    if (a.train) {
      double s = 0.0, q = 0.0;
      for (int b = 0; b < a.B; ++b) {
        const double v = (double)arr[(size_t)b * FD + c];
        s += v;
        q += v * v;
      }
      const double m = s / a.B;
      double var = q / a.B - m * m;
      if (var < 0.0) var = 0.0;
      mean = (float)m;
      invstd = (float)(1.0 / sqrt(var + (double)a.eps));
      const float unb = (float)(var * a.B / (a.B - 1));
      a.rmean[c] = (1.f - a.momentum) * a.rmean[c] + a.momentum * mean;
      a.rvar[c] = (1.f - a.momentum) * a.rvar[c] + a.momentum * unb;
    } else {
      mean = a.rmean[c];
      invstd = 1.f / sqrtf(a.rvar[c] + a.eps);
    }
    a.mi[c] = mean;
    a.mi[FD + c] = invstd;
  }
}

// R rows per wave: y, logits, and (with targets) the loss / dlogits / rank epilogue.  src: u rows (nullable: from x)
template <int R>
__device__ void phase_rows(const FtFwd& a, const float* src, int grp, int ngrp, int lane) {
  const int B = a.B, K = a.K;
  for (int b0 = grp * R; b0 < B; b0 += ngrp * R) {
    float y[R][FJ];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int b = b0 + r;
      if (b >= B) {
#pragma unroll
        for (int j = 0; j < FJ; ++j) y[r][j] = 0.f;
        continue;
      }
      if (src) {
#pragma unroll
        for (int j = 0; j < FJ; ++j) y[r][j] = src[(size_t)b * FD + lane + 64 * j];
      } else {
        row_u(a, b, lane, y[r]);
#pragma unroll
        for (int j = 0; j < FJ; ++j) a.u[(size_t)b * FD + lane + 64 * j] = y[r][j];
      }
#pragma unroll
      for (int j = 0; j < FJ; ++j) {
        const int c = lane + 64 * j;
        float v = y[r][j];
        if (a.bn) {                                   // (eval: from the running buffers, as phase_stats forms them)
          const float m = a.train ? a.mi[c] : a.rmean[c];
          const float is = a.train ? a.mi[FD + c] : 1.f / sqrtf(a.rvar[c] + a.eps);
          v = (v - m) * is * a.gamma[c] + a.beta[c];
        }
        if (a.drop) v = v * (keep_of(a.mask, a.seed, a.offset, a.thresh, (size_t)b * FD + c) * a.msc);
        y[r][j] = v;
      }
    }
    // z = W y + bias: lane l keeps the logits of classes k = l (mod 64)
    for (int kb = 0; kb < K; kb += 64) {
      const int kn = min(64, K - kb);
      float zm[R];
#pragma unroll
      for (int r = 0; r < R; ++r) zm[r] = 0.f;
      for (int kk = 0; kk < kn; ++kk) {
        const float* __restrict__ w = a.W + (size_t)(kb + kk) * FD;
        float wv[FJ];
#pragma unroll
        for (int j = 0; j < FJ; ++j) wv[j] = w[lane + 64 * j];
        const float bk = a.bias[kb + kk];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          float s = 0.f;
#pragma unroll
          for (int j = 0; j < FJ; ++j) s += y[r][j] * wv[j];
          s = wave_sum(s) + bk;
          if (lane == kk) zm[r] = s;
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (b0 + r < B && lane < kn) a.logits[(size_t)(b0 + r) * K + kb + lane] = zm[r];
    }
    if (!a.target) continue;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int b = b0 + r;
      if (b >= B) continue;
      const float* __restrict__ z = a.logits + (size_t)b * K;     // (each lane reads back only what it wrote)
      float mx = -INFINITY;
      for (int k = lane; k < K; k += 64) mx = fmaxf(mx, z[k]);
      mx = wave_max(mx);
      float se = 0.f;
      for (int k = lane; k < K; k += 64) se += expf(z[k] - mx);
      se = wave_sum(se);
      const int64_t t64 = a.target[b];
      const bool tv = t64 >= 0 && t64 < K;
      const int t = tv ? (int)t64 : 0;
      float zt = (lane == (t & 63)) ? z[t] : 0.f;
      zt = __shfl(zt, t & 63, 64);
      int cnt = 0;
      for (int k = lane; k < K; k += 64) {
        const float v = z[k];
        cnt += (v > zt || (v == zt && k < t)) ? 1 : 0;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
      if (lane == 0) {
        a.loss_rows[b] = tv ? mx + logf(se) - zt : __builtin_nanf("");
        a.corr_rows[2 * b] = (tv && cnt < 1) ? 1.f : 0.f;
        a.corr_rows[2 * b + 1] = (tv && cnt < 5) ? 1.f : 0.f;
      }
      if (a.dlogits) {
        const float inv = 1.f / se;
        for (int k = lane; k < K; k += 64)
          a.dlogits[(size_t)b * K + k] = (expf(z[k] - mx) * inv - ((tv && k == t) ? 1.f : 0.f)) * a.gscale;
      }
    }
  }
}

// batch-mean loss and correct counts, fixed order (every thread of ONE block calls it)
__device__ void phase_total(const FtFwd& a, float* sh /* [3][nthreads] */, int tid, int nthreads) {
  float s = 0.f, c1 = 0.f, c5 = 0.f;
  for (int b = tid; b < a.B; b += nthreads) {
    s += a.loss_rows[b];
    c1 += a.corr_rows[2 * b];
    c5 += a.corr_rows[2 * b + 1];
  }
  sh[tid] = s;
  sh[nthreads + tid] = c1;
  sh[2 * nthreads + tid] = c5;
  __syncthreads();
  for (int o = nthreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      sh[tid] += sh[tid + o];
      sh[nthreads + tid] += sh[nthreads + tid + o];
      sh[2 * nthreads + tid] += sh[2 * nthreads + tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.loss[0] = sh[0] / (float)a.B;
    a.correct[0] = sh[nthreads];
    a.correct[1] = sh[2 * nthreads];
  }
}

__global__ __launch_bounds__(SMALL_T) void ft_head_fwd_small_kernel(const FtFwd a) {
  __shared__ float rows[SMALL_B * FD];                 // 128 KiB: u of every row
  __shared__ float red[3 * SMALL_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  phase_u(a, rows, wave, SMALL_T / 64, lane);
  __syncthreads();
  if (a.bn) phase_stats(a, rows, tid, SMALL_T);
  __syncthreads();
  phase_rows<2>(a, rows, wave, SMALL_T / 64, lane);
  if (a.target) {
    __syncthreads();
    phase_total(a, red, tid, SMALL_T);
  }
}

// B > 64, train + BN: u of every row, then the column statistics (one block: the statistics couple all rows)
__global__ __launch_bounds__(1024) void ft_head_stats_kernel(const FtFwd a) {
  const int tid = threadIdx.x;
  phase_u(a, a.u, tid >> 6, 16, tid & 63);
  __syncthreads();
  phase_stats(a, a.u, tid, 1024);
}

// B > 64: 4 waves x 4 rows per block; eval BN statistics come from the running buffers (block 0 writes them out)
__global__ __launch_bounds__(256) void ft_head_rows_kernel(const FtFwd a) {
  const int tid = threadIdx.x;
  if (a.bn && !a.train && blockIdx.x == 0) phase_stats(a, nullptr, tid, 256);
  if (a.bn && !a.train) __syncthreads();
  phase_rows<4>(a, nullptr, blockIdx.x * 4 + (tid >> 6), gridDim.x * 4, tid & 63);
}

__global__ __launch_bounds__(256) void ft_head_total_kernel(const FtFwd a) {
  __shared__ float red[3 * 256];
  phase_total(a, red, threadIdx.x, 256);
}

// ---- backward phases
__device__ __forceinline__ float dz_of(const FtBwd& a, float g, int b, int k) {
  const size_t i = (size_t)b * a.K + k;
  float d = a.dz_ext ? a.dz_ext[i] : 0.f;
  if (a.dl_saved) d += g * a.dl_saved[i];
  return d;
}

__device__ __forceinline__ float dropscale(const FtBwd& a, size_t e) {
  return a.drop ? keep_of(a.mask, a.seed, a.offset, a.thresh, e) * a.msc : 1.f;
}

// y (the Linear's input) of element e = b*FD + c, recomputed from the saved rows and the regenerated mask
__device__ __forceinline__ float y_of(const FtBwd& a, size_t e) {
  const int c = (int)(e % FD);
  float v = a.u[e];
  if (a.bn) v = (v - a.mi[c]) * a.mi[FD + c] * a.gamma[c] + a.beta[c];
  return v * dropscale(a, e);
}

// dv[b][c] = (sum_k dz[b][k] W[k][c]) * keep * msc: the gradient at the BatchNorm's output
__device__ __forceinline__ float dv_of(const FtBwd& a, float g, size_t e) {
  const int b = (int)(e / FD), c = (int)(e % FD);
  float s = 0.f;
  for (int k = 0; k < a.K; ++k) s += dz_of(a, g, b, k) * a.W[(size_t)k * FD + c];
  return s * dropscale(a, e);
}

// dW[k][c] = sum_b dz[b][k] y[b][c]; db[k] = sum_b dz[b][k] (item c == 0)
__device__ __forceinline__ void dw_item(const FtBwd& a, float g, const float* ya, int k, int c) {
  float s = 0.f, sb = 0.f;
  for (int b = 0; b < a.B; ++b) {
    const float d = dz_of(a, g, b, k);
    s += d * ya[(size_t)b * FD + c];
    sb += d;
  }
  a.dW[(size_t)k * FD + c] = s;
  if (c == 0) a.db[k] = sb;
}

// dbeta[c] = sum_b dv ; dgamma[c] = sum_b dv * xhat
__device__ __forceinline__ void cols_item(const FtBwd& a, const float* dva, int c) {
  const float m = a.mi[c], is = a.mi[FD + c];
  float s1 = 0.f, s2 = 0.f;
  for (int b = 0; b < a.B; ++b) {
    const float dv = dva[(size_t)b * FD + c];
    s1 += dv;
    s2 += dv * ((a.u[(size_t)b * FD + c] - m) * is);
  }
  a.dbeta[c] = s1;
  a.dgamma[c] = s2;
}

// BatchNorm backward then L2-normalisation backward of row b (one wave) -> dfeat
__device__ void brow(const FtBwd& a, const float* dva, int b, int lane) {
  float du[FJ], uu[FJ];
  float dot = 0.f;
#pragma unroll
  for (int j = 0; j < FJ; ++j) {
    const int c = lane + 64 * j;
    const size_t e = (size_t)b * FD + c;
    const float dv = dva[e];
    uu[j] = a.u[e];
    float d = dv;
    if (a.bn) {
      const float is = a.mi[FD + c], gs = a.gamma[c] * is;
      if (a.train) {
        const float xh = (uu[j] - a.mi[c]) * is;
        d = gs * (dv - a.dbeta[c] / (float)a.B - xh * (a.dgamma[c] / (float)a.B));
      } else {
        d = gs * dv;
      }
    }
    du[j] = d;
    dot += uu[j] * d;
  }
  if (a.l2) {
    dot = wave_sum(dot);
    const float n = a.norms[b];
    const bool clamped = n <= 1e-12f;                  // max(||x||, eps) took eps: u = x / eps, a linear map
#pragma unroll
    for (int j = 0; j < FJ; ++j) du[j] = clamped ? du[j] / n : (du[j] - uu[j] * dot) / n;
  }
#pragma unroll
  for (int j = 0; j < FJ; ++j) a.dfeat[(size_t)b * FD + lane + 64 * j] = du[j];
}

__device__ __forceinline__ float gout_of(const FtBwd& a) { return a.dl_saved ? a.gout[0] : 0.f; }

__global__ __launch_bounds__(SMALL_T) void ft_head_bwd_small_kernel(const FtBwd a) {
  __shared__ float rows[SMALL_B * FD];                 // y, then dv
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float g = gout_of(a);
  const size_t n = (size_t)a.B * FD;
  for (size_t e = tid; e < n; e += SMALL_T) rows[e] = y_of(a, e);
  __syncthreads();
  for (int i = tid; i < a.K * FD; i += SMALL_T) dw_item(a, g, rows, i / FD, i % FD);
  __syncthreads();
  for (size_t e = tid; e < n; e += SMALL_T) rows[e] = dv_of(a, g, e);
  __syncthreads();
  if (a.bn) {
    for (int c = tid; c < FD; c += SMALL_T) cols_item(a, rows, c);
    __syncthreads();
  }
  for (int b = wave; b < a.B; b += SMALL_T / 64) brow(a, rows, b, lane);
}

__global__ __launch_bounds__(256) void ft_head_bwd_elem_kernel(const FtBwd a) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)a.B * FD) return;
  a.ybuf[e] = y_of(a, e);
  a.dvbuf[e] = dv_of(a, gout_of(a), e);
}

__global__ __launch_bounds__(256) void ft_head_bwd_cols_kernel(const FtBwd a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.K * FD) dw_item(a, gout_of(a), a.ybuf, i / FD, i % FD);
  else if (a.bn && i < (a.K + 1) * FD) cols_item(a, a.dvbuf, i - a.K * FD);
}

__global__ __launch_bounds__(256) void ft_head_bwd_rows_kernel(const FtBwd a) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b < a.B) brow(a, a.dvbuf, b, threadIdx.x & 63);
}

// ---- top-k rank counts: one workgroup, one wave per row, per-wave counts summed in wave order (deterministic)
__global__ __launch_bounds__(1024) void topk_correct_kernel(const float* __restrict__ scores, int64_t N, int K,
                                                            const int64_t* __restrict__ target, float* __restrict__ correct) {
  __shared__ float part[16][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float c1 = 0.f, c5 = 0.f;
  for (int64_t r = wave; r < N; r += 16) {
    const int64_t t = target[r];
    if (t < 0 || t >= K) continue;
    const int rank = target_rank(scores + (size_t)r * K, K, (int)t, lane);
    c1 += rank < 1 ? 1.f : 0.f;
    c5 += rank < 5 ? 1.f : 0.f;
  }
  if (lane == 0) {
    part[wave][0] = c1;
    part[wave][1] = c5;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s1 = 0.f, s5 = 0.f;
    for (int w = 0; w < 16; ++w) {
      s1 += part[w][0];
      s5 += part[w][1];
    }
    correct[0] = s1;
    correct[1] = s5;
  }
}

// ---- multi-tensor optimizer steps, per-tensor hyperparameters (<= 48 tensors per launch, 4096 elements per block)
constexpr int OPT_CHUNK = 48;
struct SgdGroupedTable {
  float* p[OPT_CHUNK];
  const float* g[OPT_CHUNK];
  float* m[OPT_CHUNK];
  long long n[OPT_CHUNK];
  int blk0[OPT_CHUNK + 1];
  float lr[OPT_CHUNK], wd[OPT_CHUNK], mu[OPT_CHUNK];
  int first[OPT_CHUNK];
  int count;
};

__device__ __forceinline__ int table_slot(const int* blk0, int count) {
  int ti = 0;
  while (ti + 1 < count && (int)blockIdx.x >= blk0[ti + 1]) ++ti;
  return ti;
}

// torch.optim.SGD (no nesterov, no dampening), the arithmetic of elementwise.hip's sgd_kernel
__global__ __launch_bounds__(256) void sgd_grouped_kernel(const SgdGroupedTable t) {
  const int ti = table_slot(t.blk0, t.count);
  const long long base = (long long)(blockIdx.x - t.blk0[ti]) * 4096;
  float* __restrict__ p = t.p[ti];
  const float* __restrict__ g = t.g[ti];
  float* __restrict__ m = t.m[ti];
  const long long n = t.n[ti];
  const float lr = t.lr[ti], wd = t.wd[ti], mu = t.mu[ti];
  const int first = t.first[ti];
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const long long i = base + j * 256 + threadIdx.x;
    if (i < n) {
      const float pv = p[i];
      const float d = g[i] + wd * pv;
      const float b = first ? d : mu * m[i] + d;
      m[i] = b;
      p[i] = pv - lr * b;
    }
  }
}

struct AdamTable {
  float* p[OPT_CHUNK];
  const float* g[OPT_CHUNK];
  float* m[OPT_CHUNK];
  float* v[OPT_CHUNK];
  long long n[OPT_CHUNK];
  int blk0[OPT_CHUNK + 1];
  float step_size[OPT_CHUNK];     // lr / (1 - beta1^step)
  float bc2_sqrt[OPT_CHUNK];      // sqrt(1 - beta2^step)
  float wd[OPT_CHUNK];
  int count;
};

// torch.optim.Adam (L2 weight decay added to the gradient, no amsgrad), the order of its single-tensor path
__global__ __launch_bounds__(256) void adam_kernel(const AdamTable t, float beta1, float beta2, float eps) {
  const int ti = table_slot(t.blk0, t.count);
  const long long base = (long long)(blockIdx.x - t.blk0[ti]) * 4096;
  float* __restrict__ p = t.p[ti];
  const float* __restrict__ g = t.g[ti];
  float* __restrict__ m = t.m[ti];
  float* __restrict__ v = t.v[ti];
  const long long n = t.n[ti];
  const float ss = t.step_size[ti], bc2s = t.bc2_sqrt[ti], wd = t.wd[ti];
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const long long i = base + j * 256 + threadIdx.x;
    if (i < n) {
      const float pv = p[i];
      float gv = g[i];
      if (wd != 0.f) gv = gv + wd * pv;
      const float mv = m[i] + omb1 * (gv - m[i]);
      const float vv = v[i] * beta2 + omb2 * gv * gv;
      m[i] = mv;
      v[i] = vv;
      const float denom = sqrtf(vv) / bc2s + eps;
      p[i] = pv + (-ss) * (mv / denom);
    }
  }
}

}  // namespace slv

using namespace slv;

namespace {
unsigned dropout_thresh(float p) {             // keep iff word >= p * 2^32 (slv_dropout_masks)
  const double t = (double)(p * 4294967296.0f);
  return t >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)t;
}
}  // namespace

extern "C" {

int slv_ft_head_fwd(const float* x, const float* W, const float* bias, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, const float* mask, uint64_t seed, uint64_t offset,
                    float p, const int64_t* target, float* logits, float* u, float* norms, float* mean_invstd,
                    float* dlogits, float* ws, float* loss, float* correct, int B, int K, int l2, int bn, int train,
                    int drop, float momentum, float eps, slv_stream_t stream) {
  SLV_CHECK_ARG(x && W && bias && logits && u && norms && mean_invstd && B > 0 && K > 0 && K <= (1 << 20),
                "bad argument");
  SLV_CHECK_ARG(!bn || (gamma && beta && running_mean && running_var), "BatchNorm needs gamma, beta, running stats");
  SLV_CHECK_ARG(!(bn && train) || B > 1, "train-mode BatchNorm needs more than one row");
  SLV_CHECK_ARG(!drop || (p >= 0.f && p < 1.f), "dropout probability outside [0, 1)");
  SLV_CHECK_ARG(!target || (ws && loss && correct), "the loss epilogue needs ws, loss and correct");
  FtFwd a;
  a.x = x; a.W = W; a.bias = bias; a.gamma = gamma; a.beta = beta; a.rmean = running_mean; a.rvar = running_var;
  a.mask = mask; a.seed = seed; a.offset = offset; a.thresh = dropout_thresh(p); a.msc = drop ? 1.f / (1.f - p) : 1.f;
  a.target = target; a.logits = logits; a.u = u; a.norms = norms; a.mi = mean_invstd; a.dlogits = dlogits;
  a.loss_rows = ws; a.corr_rows = ws ? ws + B : nullptr; a.loss = loss; a.correct = correct;
  a.gscale = 1.f / (float)B; a.momentum = momentum; a.eps = eps;
  a.B = B; a.K = K; a.l2 = l2; a.bn = bn; a.train = train; a.drop = drop ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (B <= SMALL_B) {
    hipLaunchKernelGGL(ft_head_fwd_small_kernel, dim3(1), dim3(SMALL_T), 0, st, a);
    SLV_LAUNCH_CHECK();
    return 0;
  }
  if (bn && train) hipLaunchKernelGGL(ft_head_stats_kernel, dim3(1), dim3(1024), 0, st, a);
  hipLaunchKernelGGL(ft_head_rows_kernel, dim3((B + 15) / 16), dim3(256), 0, st, a);
  if (target) hipLaunchKernelGGL(ft_head_total_kernel, dim3(1), dim3(256), 0, st, a);
  SLV_LAUNCH_CHECK();
  return 0;
}

int slv_ft_head_bwd(const float* dlogits_in, const float* dlogits_saved, const float* gout, const float* u,
                    const float* norms, const float* mean_invstd, const float* W, const float* gamma, const float* beta,
                    const float* mask, uint64_t seed, uint64_t offset, float p, float* dW, float* db, float* dgamma,
                    float* dbeta, float* dfeat, float* ws, int B, int K, int l2, int bn, int train, int drop,
                    slv_stream_t stream) {
  SLV_CHECK_ARG((dlogits_in || (dlogits_saved && gout)) && u && norms && mean_invstd && W && dW && db && dfeat &&
                B > 0 && K > 0 && K <= (1 << 20), "bad argument");
  SLV_CHECK_ARG(!bn || (gamma && beta && dgamma && dbeta), "BatchNorm needs gamma, beta, dgamma, dbeta");
  SLV_CHECK_ARG(!drop || (p >= 0.f && p < 1.f), "dropout probability outside [0, 1)");
  SLV_CHECK_ARG(B <= SMALL_B || ws, "B > 64 needs a 2 x B x 512 workspace");
  SLV_CHECK_ARG((long long)(K + 1) * FD < 0x7FFFFFFFLL, "too many classes");
  FtBwd a;
  a.dz_ext = dlogits_in; a.dl_saved = dlogits_saved; a.gout = gout; a.u = u; a.norms = norms; a.mi = mean_invstd;
  a.W = W; a.gamma = gamma; a.beta = beta; a.mask = mask; a.seed = seed; a.offset = offset;
  a.thresh = dropout_thresh(p); a.msc = drop ? 1.f / (1.f - p) : 1.f;
  a.dW = dW; a.db = db; a.dgamma = dgamma; a.dbeta = dbeta; a.dfeat = dfeat;
  a.ybuf = ws; a.dvbuf = ws ? ws + (size_t)B * FD : nullptr;
  a.B = B; a.K = K; a.l2 = l2; a.bn = bn; a.train = train; a.drop = drop ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (B <= SMALL_B) {
    hipLaunchKernelGGL(ft_head_bwd_small_kernel, dim3(1), dim3(SMALL_T), 0, st, a);
    SLV_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(ft_head_bwd_elem_kernel, dim3((unsigned)(((size_t)B * FD + 255) / 256)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(ft_head_bwd_cols_kernel, dim3((unsigned)(((size_t)(K + 1) * FD + 255) / 256)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(ft_head_bwd_rows_kernel, dim3((B + 3) / 4), dim3(256), 0, st, a);
  SLV_LAUNCH_CHECK();
  return 0;
}

int slv_topk_correct(const float* scores, int64_t N, int K, const int64_t* target, float* correct, slv_stream_t stream) {
  SLV_CHECK_ARG(scores && target && correct && N > 0 && K > 0, "bad argument");
  hipLaunchKernelGGL(topk_correct_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, scores, N, K, target, correct);
  SLV_LAUNCH_CHECK();
  return 0;
}

int slv_sgd_step_grouped(const void* const* params, const void* const* grads, const void* const* bufs,
                         const int64_t* sizes, const float* lrs, const float* weight_decays, const float* momenta,
                         const int32_t* first_step, int n_tensors, slv_stream_t stream) {
  SLV_CHECK_ARG(params && grads && bufs && sizes && lrs && weight_decays && momenta && first_step && n_tensors >= 0,
                "null pointer (host arrays expected)");
  int i = 0;
  while (i < n_tensors) {
    SgdGroupedTable t;
    t.count = 0;
    long long blocks = 0;
    while (i < n_tensors && t.count < OPT_CHUNK) {
      if (sizes[i] > 0) {
        const int k = t.count++;
        t.p[k] = (float*)params[i];
        t.g[k] = (const float*)grads[i];
        t.m[k] = (float*)bufs[i];
        t.n[k] = sizes[i];
        t.blk0[k] = (int)blocks;
        t.lr[k] = lrs[i];
        t.wd[k] = weight_decays[i];
        t.mu[k] = momenta[i];
        t.first[k] = first_step[i];
        blocks += (sizes[i] + 4095) / 4096;
      }
      ++i;
    }
    if (t.count == 0) break;
    SLV_CHECK_ARG(blocks < 0x7FFFFFFFLL, "tensors too large");
    t.blk0[t.count] = (int)blocks;
    hipLaunchKernelGGL(sgd_grouped_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t);
    SLV_LAUNCH_CHECK();
  }
  return 0;
}

int slv_adam_step(const void* const* params, const void* const* grads, const void* const* exp_avgs,
                  const void* const* exp_avg_sqs, const int64_t* sizes, const float* step_sizes,
                  const float* bias_correction2_sqrt, const float* weight_decays, int n_tensors, float beta1,
                  float beta2, float eps, slv_stream_t stream) {
  SLV_CHECK_ARG(params && grads && exp_avgs && exp_avg_sqs && sizes && step_sizes && bias_correction2_sqrt &&
                weight_decays && n_tensors >= 0, "null pointer (host arrays expected)");
  int i = 0;
  while (i < n_tensors) {
    AdamTable t;
    t.count = 0;
    long long blocks = 0;
    while (i < n_tensors && t.count < OPT_CHUNK) {
      if (sizes[i] > 0) {
        const int k = t.count++;
        t.p[k] = (float*)params[i];
        t.g[k] = (const float*)grads[i];
        t.m[k] = (float*)exp_avgs[i];
        t.v[k] = (float*)exp_avg_sqs[i];
        t.n[k] = sizes[i];
        t.blk0[k] = (int)blocks;
        t.step_size[k] = step_sizes[i];
        t.bc2_sqrt[k] = bias_correction2_sqrt[i];
        t.wd[k] = weight_decays[i];
        blocks += (sizes[i] + 4095) / 4096;
      }
      ++i;
    }
    if (t.count == 0) break;
    SLV_CHECK_ARG(blocks < 0x7FFFFFFFLL, "tensors too large");
    t.blk0[t.count] = (int)blocks;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t, beta1, beta2, eps);
    SLV_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
