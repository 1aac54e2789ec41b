// Dataset-level statistics of the pull-back metric G = J^T J: running sums of G and of the cosine similarities of the Jacobian
// columns over every sample a caller streams through (the quantities of the reference's visualizer.py:191-198,
// :305-317: batch-mean g_kk and the mean absolute cosine similarity).
//
// Per sample, all in float64 on the float32 input:  n_k = sqrt(G_kk) + 1e-8,  cos_ij = G_ij / (n_i n_j) formed as
// G_ij * (1 / n_i) * (1 / n_j).  A sample counts iff every diagonal entry is finite and > 0; otherwise it only bumps `skipped`.
//
// cmf_metric_stats_accumulate ADDS to state = [S_G (d^2) | S_cos (d^2) | count | skipped] (doubles) in two launches, with no
// floating-point atomics and a summation order that is a function of (B, d, chunk) alone:
//   1. partial_kernel, grid (chunks, tiles).  A workgroup owns a block of whole rows (<= TILE consecutive matrix elements, K per
//      thread, lanes along the contiguous index) for `chunk` consecutive samples.  Per sample it reads the d diagonal entries
//      (stride d + 1), stages the inverse norms in LDS (double-buffered: one barrier per sample, which is also the block-wide AND
//      of "this diagonal entry is valid"), then streams its rows once and adds G_ij and cos_ij to 2 K float64 registers -- no
//      d x d tile anywhere.  The sums of the chunk go to the caller's workspace; the workgroup of tile 0 also writes the chunk's
//      (count, skipped).  With sample_macs, every workgroup leaves sum_{i != j} |cos_ij| over its rows per sample (NaN for a
//      skipped sample) behind the chunk partials: wave shuffles, then the four wave totals through LDS after the sample loop.
//   2. fold_kernel.  state[e] += partial(chunk 0)[e], then chunk 1, ... in chunk order; sample_macs[b] = the row-block sums of
//      sample b in block order / (d (d - 1)), rounded to float32 (NaN propagates; 0 for d = 1).
// HBM- and latency-bound: 4 B d^2 bytes read once, 16 d^2 bytes of partials per chunk written and read once.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int K = 4;                  // matrix elements per thread
constexpr int TILE = NT * K;
constexpr int MAXD = 512;
constexpr int MAXCHUNK = 64;

inline int rows_per_tile(int d) { return TILE / d < d ? TILE / d : d; }       // d <= MAXD < TILE: at least two rows

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(NT) void partial_kernel(const float* __restrict__ jtj, int d, int B, int chunk, int rows,
                                                     double* __restrict__ part, long long part_stride,
                                                     double* __restrict__ macs_part, int n_tiles) {
  __shared__ double rn[2][MAXD];                  // 1 / n_k of the current sample, double-buffered
  __shared__ double red[MAXCHUNK][NT / 64];
  const int tid = threadIdx.x, c = blockIdx.x, tile = blockIdx.y;
  const int row0 = tile * rows;
  const int nrows = d - row0 < rows ? d - row0 : rows;
  const int n_el = nrows * d;                     // <= TILE
  const long long dd = (long long)d * d;
  const int b0 = c * chunk, b1 = b0 + chunk < B ? b0 + chunk : B;

  int ri[K], ci[K];
  double sg[K], sc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = tid + k * NT;
    ri[k] = row0 + e / d;
    ci[k] = e % d;
    sg[k] = 0.0;
    sc[k] = 0.0;
  }
  int count = 0;
  for (int b = b0; b < b1; ++b) {
    const float* __restrict__ G = jtj + b * dd;
    const float* __restrict__ Gt = G + (long long)row0 * d;
    float g[K];
#pragma unroll
    for (int k = 0; k < K; ++k) g[k] = tid + k * NT < n_el ? Gt[tid + k * NT] : 0.f;
    double* r = rn[(b - b0) & 1];
    int ok = 1;
    for (int k = tid; k < d; k += NT) {
      const double gkk = (double)G[(long long)k * (d + 1)];
      ok &= gkk > 0.0 && gkk < __builtin_inf();
      r[k] = 1.0 / (sqrt(gkk) + 1e-8);
    }
    const int valid = __syncthreads_and(ok);      // uniform; also publishes r
    double mac = 0.0;
    if (valid) {
      ++count;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (tid + k * NT < n_el) {
          const double v = (double)g[k];
          const double cs = v * r[ri[k]] * r[ci[k]];
          sg[k] += v;
          sc[k] += cs;
          mac += ri[k] != ci[k] ? fabs(cs) : 0.0;
        }
      }
    } else {
      mac = __builtin_nan("");
    }
    if (macs_part) {
      mac = wave_sum_f64(mac);
      if ((tid & 63) == 0) red[b - b0][tid >> 6] = mac;
    }
  }
  double* p = part + c * part_stride;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = tid + k * NT;
    if (e < n_el) {
      p[(long long)row0 * d + e] = sg[k];
      p[dd + (long long)row0 * d + e] = sc[k];
    }
  }
  if (tile == 0 && tid == 0) {
    p[2 * dd] = (double)count;
    p[2 * dd + 1] = (double)(b1 - b0 - count);
  }
  if (macs_part) {
    __syncthreads();
    if (tid < b1 - b0)
      macs_part[(long long)(b0 + tid) * n_tiles + tile] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
  }
}

__global__ __launch_bounds__(NT) void fold_kernel(double* __restrict__ state, long long n_state, const double* __restrict__ part,
                                                  int n_chunks, int state_blocks, const double* __restrict__ macs_part,
                                                  int n_tiles, int d, int B, float* __restrict__ sample_macs) {
  if ((int)blockIdx.x < state_blocks) {
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e >= n_state) return;
    double v = state[e];
    for (int c = 0; c < n_chunks; ++c) v += part[c * n_state + e];
    state[e] = v;
  } else {
    const long long b = (long long)(blockIdx.x - state_blocks) * NT + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int t = 0; t < n_tiles; ++t) s += macs_part[b * n_tiles + t];
    sample_macs[b] = (float)(d > 1 ? s / ((double)d * (double)(d - 1)) : s);
  }
}

}  // namespace

extern "C" long long cmf_metric_stats_ws(int d, int B, int chunk, int with_sample_macs) {
  if (d < 1 || d > MAXD || B <= 0 || chunk < 1 || chunk > MAXCHUNK) return CMF_EINVAL;
  const long long n_state = 2LL * d * d + 2, n_chunks = cmf_ceil_div(B, chunk);
  const long long n_tiles = cmf_ceil_div(d, rows_per_tile(d));
  return n_chunks * n_state + (with_sample_macs ? (long long)B * n_tiles : 0);
}

extern "C" int cmf_metric_stats_accumulate(const float* jtj, int d, int B, int chunk, double* state, double* ws,
                                           long long ws_doubles, float* sample_macs, void* stream) {
  if (!jtj || !state || !ws || (uintptr_t)state % 8 || (uintptr_t)ws % 8) return CMF_EINVAL;
  const long long need = cmf_metric_stats_ws(d, B, chunk, sample_macs != nullptr);
  if (need < 0) return (int)need;
  if (ws_doubles < need) return CMF_EINVAL;
  const int rows = rows_per_tile(d), n_tiles = cmf_ceil_div(d, rows), n_chunks = cmf_ceil_div(B, chunk);
  const long long n_state = 2LL * d * d + 2;
  double* macs_part = sample_macs ? ws + n_chunks * n_state : nullptr;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(partial_kernel, dim3(n_chunks, n_tiles), dim3(NT), 0, s, jtj, d, B, chunk, rows, ws, n_state, macs_part,
                     n_tiles);
  CMF_LAUNCH_CHECK();
  const int state_blocks = cmf_ceil_div(n_state, NT), macs_blocks = sample_macs ? cmf_ceil_div(B, NT) : 0;
  hipLaunchKernelGGL(fold_kernel, dim3(state_blocks + macs_blocks), dim3(NT), 0, s, state, n_state, (const double*)ws, n_chunks,
                     state_blocks, (const double*)macs_part, n_tiles, d, B, sample_macs);
  CMF_LAUNCH_CHECK();
  return 0;
}
