// The per-sample float64 step of geodesic shooting: between the Gram matrix of a d-column decode sweep and the narrow
// sweep over the velocity.
//
// cmf_metric_solve takes G = J^T J as one cmf_gram_cholesky attempt leaves it (float32, the lower triangle is read) and a float64
// right-hand side per sample, and computes in float64
//   solve:  out = G^-1 rhs   (the velocity v of the momentum p: z' = G^-1 p),
//   apply:  out = G rhs      (the momentum p of the initial velocity v), the symmetric product from the lower triangle,
//   stats = { rhs^T out, max_k |out_k| }   (solve: rhs^T out = p^T v, the squared speed).
// One 256-thread workgroup per sample; nothing is shared between workgroups, there are no atomics.
//
//   1. The lower triangle of G is loaded into the float64 matrix A in LDS, with rhs as row d below it.  The row stride is d | 1:
//      odd, so that the column reads of the elimination (16 rows of one column per wave) spread over the banks.
//   2. solve: Cholesky without square roots on the lower triangle with rhs as the extra row d, which ends forward-substituted,
//      then the back substitution on row d (dense_f64.h: eliminate, back_substitute -- the elimination of gn_step.hip).
//      apply: thread i sums A_[max(i,j)][min(i,j)] rhs_j over j = 0 .. d - 1 in that order.
//   3. rhs^T out and max |out_k|: one value per thread, folded by a fixed binary tree in LDS.
// The order of every sum is a function of d alone.
//
// info: 0 ok; 1 (solve) a pivot that is not positive and finite (out64, out32, stats = NaN); 2 a non-finite value in the lower
// triangle of jtj or in rhs (every output NaN).
#include "dense_f64.h"                             // no fp-contract pragma in this file: the helpers fuse multiply-adds

namespace {

constexpr int NT = 256;
static_assert(NT == F64_NT, "dense_f64.h is written for this workgroup size");
constexpr int MAXD = 128;
constexpr int SMALL = NT + MAXD;                  // doubles: the tree's partials [NT], out [MAXD]; then A [(d + 1) * row_stride(d)]

template <bool APPLY>
__global__ __launch_bounds__(NT) void metric_solve_kernel(const float* __restrict__ jtj, const double* __restrict__ rhs, int d,
                                                           double* __restrict__ out64, float* __restrict__ out32,
                                                           double* __restrict__ stats, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, b = blockIdx.x;
  double* part = lds;
  double* xs = lds + NT;                          // [MAXD]
  double* A = lds + SMALL;                        // [(d + 1) * LD]
  const int LD = row_stride(d), dd = d * d;
  const double nan = __builtin_nan("");
  const long long ob = (long long)b * d;

  // 1. the lower triangle of G, rhs below it
  int bad = load_lower<true>(jtj + (long long)b * dd, d, A, LD);
  double rk = 0.0;                                // thread k < d keeps rhs_k
  if (tid < d) {
    rk = rhs[ob + tid];
    bad |= not_finite(rk);
    A[d * LD + tid] = rk;
  }
  if (__syncthreads_or(bad)) {                    // uniform; the barrier also publishes A
    if (tid < d) {
      out64[ob + tid] = nan;
      out32[ob + tid] = (float)nan;
    }
    if (tid < 2) stats[2LL * b + tid] = nan;
    if (tid == 0) info[b] = 2;
    return;
  }

  double ok = 0.0;                                // thread k < d: out_k
  if (APPLY) {
    // 2. out_i = sum_j G_ij rhs_j, j ascending
    if (tid < d) {
      const double* r = A + d * LD;
      for (int j = 0; j < d; ++j) ok += (j <= tid ? A[tid * LD + j] : A[j * LD + tid]) * r[j];
    }
  } else {
    // 2. pivots and multipliers; row d is rhs
    if (eliminate(A, LD, d, d, d, 1)) {           // uniform
      if (tid < d) {
        out64[ob + tid] = nan;
        out32[ob + tid] = (float)nan;
      }
      if (tid < 2) stats[2LL * b + tid] = nan;
      if (tid == 0) info[b] = 1;
      return;
    }
    // the back substitution on row d
    back_substitute(A, LD, d, A + d * LD, xs);
    if (tid < d) ok = xs[tid];
  }

  // 3. the outputs and the two statistics
  if (tid < d) {
    out64[ob + tid] = ok;
    out32[ob + tid] = (float)ok;
  }
  const double dot = block_fold<false>(tid < d ? rk * ok : 0.0, part);
  const double big = block_fold<true>(tid < d ? fabs(ok) : 0.0, part);
  if (tid == 0) {
    stats[2LL * b] = dot;
    stats[2LL * b + 1] = big;
    info[b] = 0;
  }
}

template <bool APPLY>
int launch(const float* jtj, const double* rhs, int d, int B, double* out64, float* out32, double* stats, int* info,
           hipStream_t s) {
  const size_t lds = sizeof(double) * ((size_t)SMALL + (size_t)(d + 1) * row_stride(d));
  if (int e = raise_lds(metric_solve_kernel<APPLY>, lds)) return e;
  hipLaunchKernelGGL(metric_solve_kernel<APPLY>, dim3(B), dim3(NT), lds, s, jtj, rhs, d, out64, out32, stats, info);
  CMF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cmf_metric_solve(const float* jtj, const double* rhs, int d, int B, int apply, double* out64, float* out32,
                                double* stats, int* info, void* stream) {
  if (!jtj || !rhs || !out64 || !out32 || !stats || !info || B <= 0) return CMF_EINVAL;
  if (d < 1 || d > MAXD || (apply != 0 && apply != 1)) return CMF_EINVAL;
  if ((uintptr_t)jtj % 4 || (uintptr_t)rhs % 8 || (uintptr_t)out64 % 8 || (uintptr_t)out32 % 4 || (uintptr_t)stats % 8 ||
      (uintptr_t)info % 4)
    return CMF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  return apply ? launch<true>(jtj, rhs, d, B, out64, out32, stats, info, s)
               : launch<false>(jtj, rhs, d, B, out64, out32, stats, info, s);
}
