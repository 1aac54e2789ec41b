// One damped Gauss-Newton step of the projection onto the manifold, per sample.
//
// cmf_gauss_newton_step takes what one decode sweep leaves on the device -- x_hat, the Jacobian stack t (all d columns of J) and
// the Gram matrix G = J^T J of one cmf_gram_cholesky attempt -- and the head-space input x, and computes in float64
//   r = x - x_hat,   g = J^T r,   A = G + lambda diag(G)  (Marquardt scaling),   delta = A^-1 g,
//   stats = { ||r||^2, g^T delta, delta^T G delta, max_k |g_k| }.
// One 256-thread workgroup per sample; nothing is shared between workgroups, there are no atomics.
//
//   1. ||r||^2: thread i sums rows i, i + 256, ... and the 256 partials are folded by a fixed binary tree in LDS.  The
//      residual-only launch (t == NULL) is this phase alone, so both modes give the same bits.
//   2. g = J^T r streams J once.  LP = 4, 8, 16 or 32 lanes (the power of two >= min(nc, 128) / 4) run along the column index
//      with one 16-byte load each, the 256 / LP row groups stride over the rows; every thread keeps four float64 accumulators,
//      which are folded through LDS in row-group order.  The summation order is a function of (n_rows, nc) alone.  Columns >= d
//      are padding: lanes that hold none of the first d columns load nothing, and the padding columns a live lane loads are
//      neither tested for NaN nor folded.
//   3. The lower triangle of G is loaded into the float64 matrix A in LDS; from there on the kernel is damped_solve of
//      dense_f64.h, which weighted_step.hip ends in too: g goes into row d below the triangle and the diagonal is scaled
//      by 1 + lambda.  The row stride is d | 1: odd, so that the column reads of the elimination (16 rows of one column per
//      wave) spread over the banks instead of landing on one.
//   4. Cholesky without square roots on the lower triangle with g as the extra row d (dense_f64.h, eliminate): the pivots p_k
//      land on the diagonal, row d ends forward-substituted.
//   5. Back substitution on row d (dense_f64.h, back_substitute).
//   6. delta^T G delta from the float32 lower triangle in global memory (A no longer holds G): sum of G_ii delta_i^2 and
//      2 G_ij delta_i delta_j over i > j, element e of the matrix to thread e mod 256, tree-folded; g^T delta and max |g_k| alike.
//
// info: 0 ok; 1 a pivot that is not positive and finite (delta, stats[1], stats[2] = NaN; grad, stats[0], stats[3] valid);
// 2 a non-finite value in x, x_hat, the first d columns of t or the lower triangle of jtj (every output NaN).
#include "dense_f64.h"                             // no fp-contract pragma in this file: the helpers fuse multiply-adds

namespace {

constexpr int NT = 256;
static_assert(NT == F64_NT, "dense_f64.h is written for this workgroup size");
constexpr int MAXD = 128;
constexpr int PART = 4 * NT;                      // doubles: the J^T r partials [row group][4 LP]; the trees use the first NT
constexpr int SMALL = PART + MAXD;                // + delta [MAXD]; then A [(d + 1) * row_stride(d)]

template <bool FULL>
__global__ __launch_bounds__(NT) void gn_step_kernel(const float* __restrict__ t, long long t_b, long long t_r, int n_rows, int d,
                                                      int LP, const float* __restrict__ jtj, const float* __restrict__ x,
                                                      const float* __restrict__ xhat, const double* __restrict__ damping,
                                                      double* __restrict__ grad, double* __restrict__ delta,
                                                      double* __restrict__ stats, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, b = blockIdx.x;
  double* part = lds;
  const float* __restrict__ xb = x + (long long)b * n_rows;
  const float* __restrict__ hb = xhat + (long long)b * n_rows;
  const double nan = __builtin_nan("");

  // 1. ||r||^2
  int bad = 0;
  double acc = 0.0;
  for (int i = tid; i < n_rows; i += NT) {
    const float a = xb[i], h = hb[i];
    bad |= not_finite(a) | not_finite(h);
    const double rr = (double)a - (double)h;
    acc += rr * rr;
  }
  const double r2 = block_fold<false>(acc, part);
  if (!FULL) {
    bad = __syncthreads_or(bad);
    if (tid == 0) {
      stats[4LL * b] = bad ? nan : r2;
      info[b] = bad ? 2 : 0;
    }
    return;
  }

  // 2. g = J^T r: the partials of (row group rg, columns c0 .. c0 + 3)
  double* dl = lds + PART;                        // [MAXD]
  double* A = lds + SMALL;                        // [(d + 1) * LD]
  const int LD = row_stride(d);
  jt_stream(t + (long long)b * t_b, t_r, n_rows, d, LP, part, [=](int r) { return (double)xb[r] - (double)hb[r]; }, bad);

  // 3. the lower triangle of G
  const int dd = d * d;
  const float* __restrict__ G = jtj + (long long)b * dd;
  bad |= load_lower<true>(G, d, A, LD);
  if (__syncthreads_or(bad)) {                    // uniform; the barrier also publishes part and A
    for (int k = tid; k < d; k += NT) {
      grad[(long long)b * d + k] = nan;
      delta[(long long)b * d + k] = nan;
    }
    if (tid < 4) stats[4LL * b + tid] = nan;
    if (tid == 0) info[b] = 2;
    return;
  }
  double gk = 0.0;                                // thread k < d keeps g_k
  if (tid < d) {
    const int RG = NT / LP;
    for (int q = 0; q < RG; ++q) gk += part[q * (4 * LP) + tid];
    grad[(long long)b * d + tid] = gk;
  }

  // 3b - 6. the damped solve and the two forms (dense_f64.h, damped_solve)
  damped_solve(G, d, A, LD, gk, damping[b], r2, part, dl, delta + (long long)b * d, stats + 4LL * b, info + b);
}

}  // namespace

extern "C" int cmf_gauss_newton_step(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B,
                                     const float* jtj, const float* x, const float* xhat, const double* damping, double* grad,
                                     double* delta, double* stats, int* info, void* stream) {
  if (!x || !xhat || !stats || !info || n_rows <= 0 || B <= 0) return CMF_EINVAL;
  if ((uintptr_t)x % 4 || (uintptr_t)xhat % 4 || (uintptr_t)stats % 8 || (uintptr_t)info % 4) return CMF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (!t) {                                       // residual-only: the Jacobian arguments are not looked at
    hipLaunchKernelGGL(gn_step_kernel<false>, dim3(B), dim3(NT), NT * sizeof(double), s, nullptr, 0LL, 0LL, n_rows, 0, 0, nullptr,
                       x, xhat, nullptr, nullptr, nullptr, stats, info);
    CMF_LAUNCH_CHECK();
    return 0;
  }
  if (!jtj || !damping || !grad || !delta) return CMF_EINVAL;
  if (d < 1 || d > MAXD || nc % 16 || d > nc) return CMF_EINVAL;
  if (bad_panel(t, t_b, t_r, nc)) return CMF_EINVAL;
  if ((uintptr_t)jtj % 4 || (uintptr_t)damping % 8 || (uintptr_t)grad % 8 || (uintptr_t)delta % 8) return CMF_EINVAL;
  const size_t lds = sizeof(double) * ((size_t)SMALL + (size_t)(d + 1) * row_stride(d));
  if (int e = raise_lds(gn_step_kernel<true>, lds)) return e;
  hipLaunchKernelGGL(gn_step_kernel<true>, dim3(B), dim3(NT), lds, s, t, t_b, t_r, n_rows, d, jt_lanes(nc), jtj, x, xhat, damping, grad,
                     delta, stats, info);
  CMF_LAUNCH_CHECK();
  return 0;
}
