// Per-sample condition number of the Gram matrix the head factorised, and the list of samples above a threshold.
//
// cmf_gram_condition reads the (possibly jittered) J^T J that cmf_gram_cholesky / cmf_cholesky_retry leave in jtj and computes
// kappa_1(G) = ||G||_1 ||G^-1||_1 EXACTLY (up to float64 rounding), not by a norm estimator: at the widths of the head the
// inverse costs ~d^3 multiply-adds per sample (0.26 M at d = 64), negligible against the tangent sweep that produced G, and an
// exact value needs no iteration count or accuracy argument.  The arithmetic is float64 throughout: in float32 the computed
// G^-1 of a kappa ~ 1e6 matrix is off by ~kappa * 2^-24 ~ 6 % of its norm, in float64 by ~1e-10.
//
// One 256-thread workgroup per sample, three phases on a d x d float64 matrix A (LDS for d <= 128, the caller's workspace in
// global memory for 128 < d <= 512; only the workgroup that owns a sample touches its slice, __syncthreads orders the phases):
//   1. Cholesky without square roots on the lower triangle (the elimination of gram_chol.hip's block_cholesky, in float64):
//      A_ij -= A_ik A_jk / p_k for k < j <= i, one barrier per step; the pivots p_k land on the diagonal, column k keeps the
//      unscaled multipliers, so L_ik = A_ik / sqrt(p_k).  A pivot that is not positive and finite marks the sample failed.
//   2. W = L^-1 in place, columns right to left (LAPACK dtrti2, lower): W(j+1:, j) = -W(j+1:, j+1:) L(j+1:, j) / L_jj with the
//      finished columns to the right; two barriers per column.
//   3. G^-1 = W^T W, column sums of |G^-1| (each entry a dot product of two columns of W over rows >= max(i, j)), reduced in a
//      fixed order; ||G^-1||_1 is their maximum (G^-1 is symmetric).
// ||G||_1 comes from the float32 input while it is loaded.  cond = +inf when info[b] != 0, a pivot fails or the product is not
// finite.  jtj is only read.
//
// flag_kernel then lists the samples with cond > threshold in ascending order: one workgroup, chunks of 256 samples, wave
// ballots and a scan over the four waves -- a prefix sum, so the order never depends on which workgroup finished first.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MAXD = 512;
constexpr int LDS_MAXD = 128;

// Phases 1 - 3 on A (row stride d, float64) for one sample.  Returns ||G^-1||_1, or a negative value for a failed pivot.
// dk, xv: >= d doubles of LDS, part: NT doubles of LDS.
__device__ __forceinline__ double inverse_norm(double* A, int d, double* dk, double* xv, double* part) {
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  // 1. pivots and multipliers
  for (int k = 0; k < d; ++k) {
    const double piv = A[k * d + k];             // uniform
    if (!(piv > 0.0) || !(piv < 1.0e300)) return -1.0;
    const double rp = 1.0 / piv;
    for (int i = k + 1 + ti; i < d; i += 16) {
      const double aik = A[i * d + k] * rp;
      for (int j = k + 1 + tj; j <= i; j += 16) A[i * d + j] -= aik * A[j * d + k];
    }
    if (tid == 0) dk[k] = sqrt(piv);             // L_kk; nobody reads dk before the last step's barrier
    __syncthreads();
  }
  // 2. W = L^-1, column j from the finished columns j+1 .. d-1
  for (int j = d - 1; j >= 0; --j) {
    const double ljj = dk[j];
    for (int i = j + 1 + tid; i < d; i += NT) xv[i] = A[i * d + j] / ljj;       // L(i, j)
    __syncthreads();
    const double a = -1.0 / ljj;
    for (int i = j + 1 + tid; i < d; i += NT) {
      const double* wi = A + (long long)i * d;
      double s0 = 0.0, s1 = 0.0;
      int k = j + 1;
      for (; k + 2 <= i + 1; k += 2) {
        s0 += wi[k] * xv[k];
        s1 += wi[k + 1] * xv[k + 1];
      }
      if (k <= i) s0 += wi[k] * xv[k];
      A[(long long)i * d + j] = a * (s0 + s1);
    }
    if (tid == 0) A[(long long)j * d + j] = -a;
    __syncthreads();
  }
  // 3. column sums of |W^T W|: thread (slice s, column c) sums rows r = s, s + ns, ...
  const int ns = d <= NT ? NT / d : 1;
  double colmax = 0.0;
  for (int c0 = 0; c0 < d; c0 += NT) {
    double acc = 0.0;
    const int c = c0 + (d <= NT ? tid % d : tid), s = d <= NT ? tid / d : 0;
    const bool live = c < d && s < ns;
    if (live) {
      for (int r = s; r < d; r += ns) {
        double e0 = 0.0, e1 = 0.0;
        int k = r > c ? r : c;
        for (; k + 2 <= d; k += 2) {
          e0 += A[(long long)k * d + r] * A[(long long)k * d + c];
          e1 += A[(long long)(k + 1) * d + r] * A[(long long)(k + 1) * d + c];
        }
        if (k < d) e0 += A[(long long)k * d + r] * A[(long long)k * d + c];
        acc += fabs(e0 + e1);
      }
    }
    __syncthreads();                              // thread 0 has finished reading the previous pass's part
    part[tid] = live ? acc : 0.0;
    __syncthreads();
    if (tid == 0) {
      const int ncol = d - c0 < NT ? d - c0 : NT;
      for (int cc = 0; cc < ncol; ++cc) {
        double t = 0.0;
        for (int ss = 0; ss < ns; ++ss) t += part[ss * d + cc];   // ns > 1 only when d <= NT (a single pass, c0 == 0)
        colmax = t > colmax || t != t ? t : colmax;
      }
    }
  }
  return colmax;                                  // meaningful in thread 0
}

// Load G (float32, [d][d]) into the float64 matrix A and return ||G||_1 in thread 0.
__device__ __forceinline__ double load_and_norm(const float* __restrict__ G, double* A, int d, double* part) {
  const int tid = threadIdx.x;
  const long long dd = (long long)d * d;
  for (long long e = tid; e < dd; e += NT) A[e] = (double)G[e];
  __syncthreads();
  double colmax = 0.0;
  for (int c0 = 0; c0 < d; c0 += NT) {
    const int c = c0 + tid;
    double acc = 0.0;
    if (c < d)
      for (int r = 0; r < d; ++r) acc += fabs(A[(long long)r * d + c]);
    part[tid] = acc;
    __syncthreads();
    if (tid == 0) {
      const int ncol = d - c0 < NT ? d - c0 : NT;
      for (int cc = 0; cc < ncol; ++cc) colmax = part[cc] > colmax || part[cc] != part[cc] ? part[cc] : colmax;
    }
    __syncthreads();
  }
  return colmax;
}

template <bool WIDE>
__global__ __launch_bounds__(NT) void gram_cond_kernel(const float* __restrict__ jtj, const int* __restrict__ info, int d,
                                                        float* __restrict__ cond, double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int b = blockIdx.x;
  if (info[b] != 0) {                             // uniform: the factorisation of this sample failed
    if (threadIdx.x == 0) cond[b] = __builtin_inff();
    return;
  }
  double* dk = lds;                               // [MAXD]
  double* xv = lds + MAXD;                        // [MAXD]
  double* part = lds + 2 * MAXD;                  // [NT]
  double* A = WIDE ? ws + (long long)b * d * d : lds + 2 * MAXD + NT;
  const double ng = load_and_norm(jtj + (long long)b * d * d, A, d, part);
  const double ni = inverse_norm(A, d, dk, xv, part);
  if (threadIdx.x == 0) {
    const double c = ni < 0.0 ? __builtin_inf() : ng * ni;
    cond[b] = c <= 3.4e38 ? (float)c : __builtin_inff();       // NaN and overflow: +inf
  }
}

__global__ __launch_bounds__(NT) void flag_kernel(const float* __restrict__ cond, int B, float threshold, int* __restrict__ idx,
                                                  int* __restrict__ count) {
  __shared__ int wtot[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int base = 0;
  for (int b0 = 0; b0 < B; b0 += NT) {
    const int b = b0 + tid;
    const bool f = b < B && cond[b] > threshold;
    const unsigned long long m = __ballot(f);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[w] = __popcll(m);
    __syncthreads();
    int off = base, tot = 0;
    for (int i = 0; i < NT / 64; ++i) {
      off += i < w ? wtot[i] : 0;
      tot += wtot[i];
    }
    if (f) idx[off + below] = b;
    base += tot;
    __syncthreads();                              // wtot is rewritten by the next chunk
  }
  for (int b = base + tid; b < B; b += NT) idx[b] = -1;
  if (tid == 0) count[0] = base;
}

}  // namespace

extern "C" int cmf_gram_condition(const float* jtj, const int* info, int d, int B, float threshold, float* cond, int* flagged_idx,
                                  int* flagged_count, float* ws, void* stream) {
  if (!jtj || !info || !cond || !flagged_idx || !flagged_count || d < 1 || d > MAXD || B <= 0) return CMF_EINVAL;
  if (threshold != threshold) return CMF_EINVAL;
  if (d > LDS_MAXD && (!ws || (uintptr_t)ws % 8)) return CMF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const size_t small = (size_t)(2 * MAXD + NT) * sizeof(double);
  if (d > LDS_MAXD) {
    hipLaunchKernelGGL(gram_cond_kernel<true>, dim3(B), dim3(NT), small, s, jtj, info, d, cond, (double*)ws);
  } else {
    const size_t lds = small + (size_t)d * d * sizeof(double);
    if (lds > 48 * 1024) {
      hipError_t e = cmf_set_dynamic_lds((const void*)gram_cond_kernel<false>, (int)lds);
      if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(gram_cond_kernel<false>, dim3(B), dim3(NT), lds, s, jtj, info, d, cond, (double*)nullptr);
  }
  CMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(flag_kernel, dim3(1), dim3(NT), 0, s, cond, B, threshold, flagged_idx, flagged_count);
  CMF_LAUNCH_CHECK();
  return 0;
}
