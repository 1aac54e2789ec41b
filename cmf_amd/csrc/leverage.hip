// The covariance of a Gauss-Newton fit carried back over the rows of the Jacobian, per sample.
//
// cmf_tangent_leverage takes the Jacobian stack t of one decode sweep (all d columns of J, n_rows rows) and ANY symmetric
// positive definite d x d normal matrix in the form a step kernel consumes it -- J^T J, J^T diag(w) J, or K^T K of a measured
// stack K = a diag(s) J; the kernel does not assume it is the Gram matrix of the t it is given -- and computes in float64
//   cov = gram^-1,   lev_i = j_i^T gram^-1 j_i  for every row j_i of J,   stats = { sum_i lev_i, max_i lev_i }.
// One 256-thread workgroup per sample; nothing is shared between workgroups, there are no atomics.
//
//   1. The lower triangle of gram goes into the float64 matrix A in LDS (dense_f64.h, load_lower; row stride d | 1).
//   2. Cholesky without square roots (dense_f64.h, eliminate): gram = L D L^T, the pivots p_k = D_kk on the diagonal, column k
//      holding the unscaled multipliers L_rk p_k.
//   3. unit_lower_inverse: column k is divided by p_k (A holds the unit-lower L below the diagonal), q_k = 1 / p_k is kept, and
//      W = L^-1 is formed in place, columns right to left (LAPACK dtrti2, lower, unit diagonal -- gram_cond.hip's phase 2 without
//      the square roots): W_ij = -(L_ij + sum_{j < k < i} W_ik L_kj).  The diagonal of A keeps the pivots; W_ii = 1 is implied.
//   4. cov_ij = sum_{k >= i} W_ki W_kj q_k for j <= i, element e of the matrix to thread e mod 256; (j, i) is written from the
//      same register, so cov is symmetric bit for bit.  The cov-only launch (t == NULL) ends here: both modes give the same bits.
//   5. The row pass streams J once, 32 rows at a time through a float32 slab in LDS (16-byte loads of the quarter-rows that hold
//      the first d columns).  16 lanes share two rows (slab rows ri and ri + 16): lane tj takes k = tj, tj + 16, ... and forms
//      y_k = j_k + sum_{m < k} W_km j_m  against the W row broadcast from LDS, then q_k y_k^2 into its partial; the 16 partials of
//      a row are folded by a fixed xor tree.  Every term is a square times a positive q_k, so no lev is negative or -0.0.
//      The summation order is a function of (n_rows, d) alone.  Columns >= d are padding: a live quarter-row brings them into the
//      slab, where nothing reads them, and they are not tested for NaN.
//   6. stats: lane 0 of a row's 16 keeps the sum and the maximum of its rows; both are folded by block_fold.
//
// LDS at d = 128: A 129 KiB, the slab 16.5 KiB, 4 KiB of vectors: 149.5 of 160 KiB, one workgroup per CU; at d = 64, 46 KiB, three.
//
// info: 0 ok; 1 a pivot that is not positive and finite (cov, lev, stats NaN); 2 a non-finite value in the lower triangle of gram
// or (full mode) in the first d columns of t (every output NaN; 2 wins over 1).
#include "dense_f64.h"                             // no fp-contract pragma in this file: the helpers fuse multiply-adds

namespace {

constexpr int NT = 256;
static_assert(NT == F64_NT, "dense_f64.h is written for this workgroup size");
constexpr int MAXD = 128;
constexpr int SLAB = 32;                          // rows of J per pass: two per 16-lane group
constexpr int SMALL = NT + 2 * MAXD;              // doubles: part [NT], xv [MAXD], q [MAXD]; then A, then the slab

// Row stride (floats) of the slab: whole quarter-rows, plus one so that the four rows a wavefront reads at once sit in
// different banks (a stride of 64 or 128 floats would put them in one).
inline __host__ __device__ int slab_stride(int d) { return ((d + 3) & ~3) + 4; }
// Doubles of A, rounded up to keep the slab behind it 16-byte aligned.
inline __host__ __device__ int a_doubles(int d) { return (d * row_stride(d) + 1) & ~1; }

// From "eliminate has run on A" to "A holds W = L^-1 below the diagonal, the pivots on it, q_k = 1 / p_k" (published).
// xv: d doubles of LDS.
static __device__ __forceinline__ void unit_lower_inverse(double* A, int LD, int d, double* xv, double* q) {
  const int tid = threadIdx.x;
  for (int e = tid; e < d * d; e += NT) {
    const int i = e / d, j = e - i * d;
    if (j < i) A[i * LD + j] /= A[j * LD + j];    // the diagonal is only read here
  }
  if (tid < d) q[tid] = 1.0 / A[tid * LD + tid];
  __syncthreads();
  for (int j = d - 2; j >= 0; --j) {
    const int i = j + 1 + tid;                    // d <= MAXD < NT: one row per thread
    if (i < d) xv[i] = A[i * LD + j];             // L(i, j), which the threads of the rows below still need
    __syncthreads();
    if (i < d) {
      const double* wi = A + i * LD;
      double s0 = xv[i], s1 = 0.0;                // W_ii = 1
      int k = j + 1;
      for (; k + 2 <= i; k += 2) {
        s0 += wi[k] * xv[k];
        s1 += wi[k + 1] * xv[k + 1];
      }
      if (k < i) s0 += wi[k] * xv[k];
      A[i * LD + j] = -(s0 + s1);
    }
    __syncthreads();
  }
}

template <bool ROWS>
__global__ __launch_bounds__(NT) void leverage_kernel(const float* __restrict__ t, long long t_b, long long t_r, int n_rows, int d,
                                                       const float* __restrict__ gram, double* __restrict__ cov,
                                                       double* __restrict__ lev, double* __restrict__ stats,
                                                       int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, b = blockIdx.x;
  double* part = lds;                             // [NT]
  double* xv = lds + NT;                          // [MAXD]
  double* q = lds + NT + MAXD;                    // [MAXD]
  double* A = lds + SMALL;                        // [d * LD]
  const int LD = row_stride(d), dd = d * d;
  const float* __restrict__ G = gram + (long long)b * dd;
  double* __restrict__ cb = cov + (long long)b * dd;
  const double nan = __builtin_nan("");

  // 1 - 4. the factor, its inverse, cov
  int bad = __syncthreads_or(load_lower<true>(G, d, A, LD));      // uniform; the barrier also publishes A
  int fail = 0;
  if (!bad) fail = eliminate(A, LD, d, d, d, 0);
  const bool ok = !bad && !fail;                  // uniform
  if (ok) {
    unit_lower_inverse(A, LD, d, xv, q);
    for (int e = tid; e < dd; e += NT) {
      const int i = e / d, j = e - i * d;
      if (j <= i) {
        double s = (j < i ? A[i * LD + j] : 1.0) * q[i];
        for (int k = i + 1; k < d; ++k) s += A[k * LD + i] * q[k] * A[k * LD + j];
        cb[i * d + j] = s;
        if (j < i) cb[j * d + i] = s;
      }
    }
  }

  // 5. the row pass; with a refused pivot it only looks for non-finite entries of J
  double lsum = 0.0, lmax = 0.0;
  if (ROWS && !bad) {
    float* slab = (float*)(A + a_doubles(d));     // [SLAB][SL]
    const int SL = slab_stride(d), nq = (d + 3) >> 2;
    const int ri = tid >> 4, tj = tid & 15;
    const float* __restrict__ tp = t + (long long)b * t_b;
    double* __restrict__ lb = lev + (long long)b * n_rows;
    const float* s0 = slab + ri * SL;
    const float* s1 = slab + (ri + 16) * SL;
    for (int r0 = 0; r0 < n_rows; r0 += SLAB) {
      __syncthreads();                            // the previous slab has been read
      for (int e = tid; e < SLAB * nq; e += NT) {
        const int rr = e / nq, c0 = 4 * (e - rr * nq), r = r0 + rr;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r < n_rows) {                         // c0 + 3 < nc: nc is a multiple of 16 and >= d
          v = *(const f32x4*)(tp + (long long)r * t_r + c0);
          bad |= not_finite(v.x) | ((c0 + 1 < d) & not_finite(v.y)) | ((c0 + 2 < d) & not_finite(v.z)) |
                 ((c0 + 3 < d) & not_finite(v.w));
        }
        *(f32x4*)(slab + rr * SL + c0) = v;
      }
      __syncthreads();
      if (fail) continue;                         // uniform
      double a0 = 0.0, a1 = 0.0;
      for (int k = tj; k < d; k += 16) {
        const double* wk = A + k * LD;
        double y0 = (double)s0[k], y1 = (double)s1[k];
        int m = 0;
        for (; m + 4 <= k; m += 4) {
          const f32x4 u0 = *(const f32x4*)(s0 + m), u1 = *(const f32x4*)(s1 + m);
          const double w0 = wk[m], w1 = wk[m + 1], w2 = wk[m + 2], w3 = wk[m + 3];
          y0 += w0 * (double)u0.x;
          y1 += w0 * (double)u1.x;
          y0 += w1 * (double)u0.y;
          y1 += w1 * (double)u1.y;
          y0 += w2 * (double)u0.z;
          y1 += w2 * (double)u1.z;
          y0 += w3 * (double)u0.w;
          y1 += w3 * (double)u1.w;
        }
        for (; m < k; ++m) {
          const double w = wk[m];
          y0 += w * (double)s0[m];
          y1 += w * (double)s1[m];
        }
        const double qk = q[k];
        a0 += y0 * y0 * qk;
        a1 += y1 * y1 * qk;
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {           // the 16 lanes of a row: a fixed tree, the total in each
        a0 += __shfl_xor(a0, o, 64);
        a1 += __shfl_xor(a1, o, 64);
      }
      if (tj == 0) {
        const int ra = r0 + ri, rb = ra + 16;
        if (ra < n_rows) {
          lb[ra] = a0;
          lsum += a0;
          lmax = a0 > lmax ? a0 : lmax;
        }
        if (rb < n_rows) {
          lb[rb] = a1;
          lsum += a1;
          lmax = a1 > lmax ? a1 : lmax;
        }
      }
    }
  }

  // 6. stats, or NaN everywhere
  if (ROWS) {
    lsum = block_fold<false>(lsum, part);
    lmax = block_fold<true>(lmax, part);
  }
  bad = __syncthreads_or(bad);                    // the barrier also orders the NaN fill after the stores above
  if (bad || fail) {
    for (int e = tid; e < dd; e += NT) cb[e] = nan;
    if (ROWS) {
      for (int i = tid; i < n_rows; i += NT) lev[(long long)b * n_rows + i] = nan;
      if (tid < 2) stats[2LL * b + tid] = nan;
    }
    if (tid == 0) info[b] = bad ? 2 : 1;
    return;
  }
  if (tid == 0) {
    if (ROWS) {
      stats[2LL * b] = lsum;
      stats[2LL * b + 1] = lmax;
    }
    info[b] = 0;
  }
}

}  // namespace

extern "C" int cmf_tangent_leverage(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B,
                                    const float* gram, double* cov, double* lev, double* stats, int* info, void* stream) {
  if (!gram || !cov || !info || B <= 0) return CMF_EINVAL;
  if (d < 1 || d > MAXD) return CMF_EINVAL;
  if ((uintptr_t)gram % 4 || (uintptr_t)cov % 8 || (uintptr_t)info % 4) return CMF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const size_t small = sizeof(double) * ((size_t)SMALL + (size_t)a_doubles(d));
  if (!t) {                                       // cov only: the Jacobian arguments, lev and stats are not looked at
    if (int e = raise_lds(leverage_kernel<false>, small)) return e;
    hipLaunchKernelGGL(leverage_kernel<false>, dim3(B), dim3(NT), small, s, nullptr, 0LL, 0LL, 0, d, gram, cov, nullptr, nullptr,
                       info);
    CMF_LAUNCH_CHECK();
    return 0;
  }
  if (!lev || !stats || n_rows <= 0) return CMF_EINVAL;
  if (nc % 16 || d > nc) return CMF_EINVAL;
  if (bad_panel(t, t_b, t_r, nc)) return CMF_EINVAL;
  if ((uintptr_t)lev % 8 || (uintptr_t)stats % 8) return CMF_EINVAL;
  const size_t lds = small + sizeof(float) * (size_t)SLAB * slab_stride(d);
  if (int e = raise_lds(leverage_kernel<true>, lds)) return e;
  hipLaunchKernelGGL(leverage_kernel<true>, dim3(B), dim3(NT), lds, s, t, t_b, t_r, n_rows, d, gram, cov, lev, stats, info);
  CMF_LAUNCH_CHECK();
  return 0;
}
