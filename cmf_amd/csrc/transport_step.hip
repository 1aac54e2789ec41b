// Parallel transport of latent tangent vectors along discretised curves on the manifold: the per-curve float64 chain
// between the Gram / cross-Gram launches of one decode sweep and the host.
//
// cmf_transport_chain takes, per curve of P points z_0 .. z_{P-1}, the metrics G_i = J_i^T J_i as one cmf_gram_cholesky attempt leaves
// them (float32, the lower triangles are read), the cross blocks C_i = J_i^T J_{i+1} of cmf_cross_gram (float32, whole blocks) and m
// vectors w_0 (float64 latent components at point 0), and walks the N = P - 1 segments in order:
//   b = C_i^-1 (G_i w_i)          the inverse of the projection T_{i+1} -> T_i      (Gaussian elimination, partial pivoting)
//   a = G_{i+1}^-1 (C_i^T w_i)    the projection T_i -> T_{i+1}                      (Cholesky without square roots)
//   w_{i+1} = 1/2 (a + b)         in principal-angle coordinates diag((cos + sec) / 2): the rotation between the planes to O(theta^4)
// and norm2_i = w_i^T G_i w_i at every point.  One 256-thread workgroup per curve; nothing is shared between workgroups, there are no
// atomics.  All arithmetic is float64 without contraction.
//
// Per point i:
//   1. G_i's lower triangle -> the float64 window A in LDS (row stride (d + m) | 1, odd: column reads spread over the banks);
//      u = G_i w_i, j ascending, into columns d .. d + m - 1 of A (w_i is re-read from `out`); norm2_i = sum_r w_i[r] u[r], r ascending.
//   2. (i < N) C_i -> columns 0 .. d - 1 of A: the augmented matrix [C_i | G_i w_i].  Per column k: every wave finds the pivot row --
//      the largest |A_rk|, r >= k, the lowest r among equals -- by itself; rows k and p swap their columns > k; multipliers by
//      division, A_ij -= (A_ik / piv) A_kj; two barriers per column.  Column k is never swapped: the pivots live in pv[].  Then the
//      back substitution, last column first, one barrier per column; b goes straight to `bwd`.
//   3. G_{i+1}'s lower triangle -> A with row stride d | 1, the m right-hand sides C_i^T w_i (r ascending, straight from the float32
//      block) as rows d .. d + m - 1; the elimination of shoot_step.hip / gn_step.hip (dense_f64.h, eliminate) with m extra rows,
//      which end forward-substituted.  Then the back substitution on those rows; a goes straight to `fwd`.
//   4. out_{i+1} = 0.5 (a + b).
// The order of every sum is a function of (d, m) alone.
//
// info: 0 ok; 1 a pivot of some G_{i+1} that is not positive and finite or a pivot of some C_i that is zero or not finite (fwd / bwd
// of that segment and of the later ones, out / norm2 from point i + 1 on = NaN; everything before keeps its bits); 2 a non-finite
// value in w0 or in a part of jtj / cross that is read (every output NaN; found by a pass over the curve's inputs before anything
// is written, so it takes precedence).
#pragma clang fp contract(off)
#include "dense_f64.h"                             // after the pragma: the helpers are compiled without contraction

namespace {

constexpr int NT = 256;
static_assert(NT == F64_NT, "dense_f64.h is written for this workgroup size");
constexpr int MAXD = 128;
constexpr int MAXM = 16;

inline __host__ __device__ int stride_lu(int d, int m) { return (d + m) | 1; }
inline __host__ __device__ int stride_chol(int d) { return d | 1; }
inline __host__ __device__ int window(int d, int m) {
  const int a = d * stride_lu(d, m), b = (d + m) * stride_chol(d);
  return a > b ? a : b;
}

__device__ __forceinline__ void fill(double* p, long long n, double v) {
  for (long long e = threadIdx.x; e < n; e += NT) p[e] = v;
}

__global__ __launch_bounds__(NT) void transport_chain_kernel(const float* __restrict__ jtj, const float* __restrict__ cross,
                                                             const double* __restrict__ w0, int d, int m, int P, double* out,
                                                             double* fwd, double* bwd, double* __restrict__ norm2,
                                                             int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, c0 = blockIdx.x;
  double* pv = lds;                               // [MAXD] the pivots of the LU
  double* A = lds + MAXD;                         // the window
  const int N = P - 1, dd = d * d, md = m * d;
  const int LB = stride_lu(d, m), LF = stride_chol(d);
  const double nan = __builtin_nan("");
  const float* __restrict__ Gc = jtj + (long long)c0 * P * dd;      // point i of the curve: Gc + i dd
  const float* __restrict__ Cc = cross + (long long)c0 * P * dd;    // segment i: Cc + i dd, i < N
  double* o = out + (long long)c0 * P * md;       // [P][m][d]
  double* fa = fwd + (long long)c0 * N * md;      // [N][m][d]
  double* fb = bwd + (long long)c0 * N * md;
  double* n2 = norm2 + (long long)c0 * P * m;     // [P][m]

  // 0. everything that will be read must be finite
  int bad = 0;
  for (long long e = tid; e < (long long)P * dd; e += NT) {
    const int r = (int)(e % dd), i = r / d, j = r - i * d;
    if (j <= i) bad |= not_finite(Gc[e]);
  }
  for (long long e = tid; e < (long long)N * dd; e += NT) bad |= not_finite(Cc[e]);
  for (int e = tid; e < md; e += NT) {
    const double v = w0[(long long)c0 * md + e];
    bad |= not_finite(v);
    o[e] = v;
  }
  if (__syncthreads_or(bad)) {                    // uniform; the barrier also publishes out[0]
    fill(o, (long long)P * md, nan);
    fill(fa, (long long)N * md, nan);
    fill(fb, (long long)N * md, nan);
    fill(n2, (long long)P * m, nan);
    if (tid == 0) info[c0] = 2;
    return;
  }

  const int ti = tid >> 4, tj = tid & 15;
  int fail_at = -1;
  for (int i = 0; i < P; ++i) {
    const double* w = o + (long long)i * md;      // [m][d], written by this workgroup before the last barrier
    // 1. u = G_i w_i into columns d .. d + m - 1; norm2_i
    load_lower<false>(Gc + (long long)i * dd, d, A, LB);
    __syncthreads();
    for (int e = tid; e < md; e += NT) {
      const int r = e / m, c = e - r * m;
      const double* wc = w + c * d;
      double s = 0.0;
      for (int j = 0; j < d; ++j) s += (j <= r ? A[r * LB + j] : A[j * LB + r]) * wc[j];
      A[r * LB + d + c] = s;
    }
    __syncthreads();
    if (tid < m) {
      const double* wc = w + tid * d;
      double s = 0.0;
      for (int r = 0; r < d; ++r) s += wc[r] * A[r * LB + d + tid];
      n2[(long long)i * m + tid] = s;
    }
    if (i == N) break;

    // 2. b = C_i^-1 u: Gaussian elimination with partial pivoting on [C_i | u]
    const float* __restrict__ C = Cc + (long long)i * dd;
    for (int e = tid; e < dd; e += NT) {
      const int r = e / d, j = e - r * d;
      A[r * LB + j] = (double)C[e];
    }
    __syncthreads();
    const int W = d + m;
    int fail = 0;
    for (int k = 0; k < d; ++k) {
      // every wave by itself: the largest |A_rk|, r >= k, the lowest r among equals
      const int lane = tid & 63;
      double best = -1.0;
      int p = 0x7fffffff;
      for (int r = k + lane; r < d; r += 64) {    // ascending r: '>' keeps the lowest row among equals
        const double v = fabs(A[r * LB + k]);
        if (v > best) {
          best = v;
          p = r;
        }
      }
      for (int s = 32; s > 0; s >>= 1) {
        const double ob = __shfl_xor(best, s, 64);
        const int op = __shfl_xor(p, s, 64);
        if (ob > best || (ob == best && op < p)) {
          best = ob;
          p = op;
        }
      }
      if (!(best > 0.0) || !(best <= __DBL_MAX__)) {      // uniform: zero, or not finite (a NaN entry never wins and hides nothing:
        fail = 1;                                         // the inputs are finite, a NaN here comes from an overflow)
        break;
      }
      const double piv = A[p * LB + k];
      const double akk = A[k * LB + k];           // row p's entry of column k after the swap; column k itself stays as it is
      if (p != k)
        for (int j = k + 1 + tid; j < W; j += NT) {
          const double a = A[k * LB + j], b = A[p * LB + j];
          A[k * LB + j] = b;
          A[p * LB + j] = a;
        }
      if (tid == 0) pv[k] = piv;
      __syncthreads();
      for (int r = k + 1 + ti; r < d; r += 16) {
        const double l = (r == p ? akk : A[r * LB + k]) / piv;
        for (int j = k + 1 + tj; j < W; j += 16) A[r * LB + j] -= l * A[k * LB + j];
      }
      __syncthreads();
    }
    if (fail) {                                   // uniform
      fail_at = i;
      break;
    }
    {
      double* b = fb + (long long)i * md;
      for (int r = d - 1; r >= 0; --r) {
        if (tj < m) {
          const double x = A[r * LB + d + tj] / pv[r];
          for (int t = ti; t < r; t += 16) A[t * LB + d + tj] -= A[t * LB + r] * x;
          if (ti == 0) b[tj * d + r] = x;
        }
        __syncthreads();
      }
    }

    // 3. a = G_{i+1}^-1 (C_i^T w_i): pivots and multipliers on the lower triangle; rows d .. d + m - 1 are the right-hand sides
    load_lower<false>(Gc + (long long)(i + 1) * dd, d, A, LF);
    for (int e = tid; e < md; e += NT) {
      const int c = e / d, j = e - c * d;
      const double* wc = w + c * d;
      double s = 0.0;
      for (int r = 0; r < d; ++r) s += (double)C[r * d + j] * wc[r];
      A[(d + c) * LF + j] = s;
    }
    __syncthreads();
    if (eliminate(A, LF, d, d, d, m)) {           // uniform
      fail_at = i;
      break;
    }
    {
      double* a = fa + (long long)i * md;
      for (int r = d - 1; r >= 0; --r) {
        if (ti < m) {
          double* wr = A + (d + ti) * LF;
          const double x = wr[r] / A[r * LF + r];
          for (int t = tj; t < r; t += 16) wr[t] -= A[r * LF + t] * x;
          if (tj == 0) a[ti * d + r] = x;
        }
        __syncthreads();
      }
    }

    // 4. w_{i+1}
    {
      const double* a = fa + (long long)i * md;
      const double* b = fb + (long long)i * md;
      double* wn = o + (long long)(i + 1) * md;
      for (int e = tid; e < md; e += NT) wn[e] = 0.5 * (a[e] + b[e]);
    }
    __syncthreads();                              // publishes w_{i+1}; the window is free
  }

  if (fail_at >= 0) {
    __syncthreads();
    const long long from = (long long)fail_at * md;
    fill(fa + from, (long long)N * md - from, nan);
    fill(fb + from, (long long)N * md - from, nan);
    fill(o + from + md, (long long)P * md - from - md, nan);
    fill(n2 + (long long)(fail_at + 1) * m, (long long)(N - fail_at) * m, nan);
  }
  if (tid == 0) info[c0] = fail_at >= 0 ? 1 : 0;
}

}  // namespace

extern "C" int cmf_transport_chain(const float* jtj, const float* cross, const double* w0, int d, int m, int points, int curves,
                                   double* out, double* fwd, double* bwd, double* norm2, int* info, void* stream) {
  if (!jtj || !cross || !w0 || !out || !fwd || !bwd || !norm2 || !info || curves <= 0) return CMF_EINVAL;
  if (d < 1 || d > MAXD || m < 1 || m > MAXM || points < 2) return CMF_EINVAL;
  if ((uintptr_t)jtj % 4 || (uintptr_t)cross % 4 || (uintptr_t)w0 % 8 || (uintptr_t)out % 8 || (uintptr_t)fwd % 8 ||
      (uintptr_t)bwd % 8 || (uintptr_t)norm2 % 8 || (uintptr_t)info % 4)
    return CMF_EINVAL;
  const size_t lds = sizeof(double) * ((size_t)MAXD + (size_t)window(d, m));
  if (int e = raise_lds(transport_chain_kernel, lds)) return e;
  hipLaunchKernelGGL(transport_chain_kernel, dim3(curves), dim3(NT), lds, (hipStream_t)stream, jtj, cross, w0, d, m, points, out,
                     fwd, bwd, norm2, info);
  CMF_LAUNCH_CHECK();
  return 0;
}
