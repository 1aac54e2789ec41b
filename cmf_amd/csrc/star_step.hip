// One damped Gauss-Newton step on a whole star of discretised curves that share one free end point, per star.
//
// A star has K arms of P points; the stack is star-major, then arm-major: point i of arm k of star s is sample (s K + k) P + i.
// Point 0 is the arm's fixed end, point N = P - 1 the arm's own copy of the centre (the K copies hold the same latent; every arm
// reads only its own copy's xhat, J and G), M = P - 2 interior points.  Per arm, with r_i = xhat_{i+1} - xhat_i and the unweighted
// objective 1/2 sum ||r_i||^2, the model of curve_step.hip with one more block:
//   g_i = J_i^T (xhat_{i-1} + xhat_{i+1} - 2 xhat_i), i = 1 .. M;   g^c = J_N^T (xhat_M - xhat_N) at the centre copy;
//   H_ii = 2 G_i, H_{i,i+1} = -C_i = -J_i^T J_{i+1} for i = 1 .. M (the last pair couples to the centre), centre contribution G_N.
// The star is Phi = sum_k w_k phi_k, A = H + lambda diag(H) with one lambda per star, delta = A^-1 g: K block tridiagonal bands
// that end in one shared d x d centre block -- a block arrow without fill-in.  Scaling an arm's rows by w_k does not change its
// elimination, so the weights enter at the centre only.  Three launches, 256 threads per workgroup, float64, no atomics, nothing
// shared between the workgroups of a launch:
//   forward, one workgroup per (star, arm): phases 1 - 3 of curve_step_kernel over the blocks 1 .. M, none of which is the last:
//     after block M the window's lower left holds -C_M^T, its lower right G_N with (1 + lambda) on the diagonal (factor 1, not 2)
//     and the extra row g^c.  Eliminating block M leaves the arm's Schur contribution T_k = (1 + lambda diag) G_N - C_M^T S_M^-1 C_M
//     there and the forward-substituted right-hand side r_k in the extra row; both go to the arm's workspace slice with g^c, the
//     arm's code and the finished columns of every block.  The window lives in LDS for d <= 64, in the slice above that.
//   centre, one workgroup per star: A_c = sum_k w_k T_k, rhs = sum_k w_k r_k and grad_centre = sum_k w_k g^c_k, each summed in arm
//     order; the elimination and back substitution of dense_f64.h on the d x d triangle in LDS give delta_centre.  The star's
//     code is settled here: 2 if an arm read a non-finite value or a weight is not positive and finite, else 1 if a pivot of an
//     arm or of the centre failed.
//   backward, one workgroup per (star, arm): phase 4 of curve_step_kernel with delta_centre as the block after block M; writes
//     delta of the interior points, the arm's forms g_k^T delta_k and delta^T H_k delta (with its centre terms), scales the arm's
//     gradient by w_k, and turns the star's code into NaN outputs.
// No fused multiply-adds (fp contract off), as curve_step.hip: phase 1 is that kernel's, operation for operation, so seg2 and the
// arm's sum have the bits of cmf_curve_step's energy-only mode on the arm as a curve.
//
// info: 0 ok; 1 a pivot of some arm or of the centre not positive and finite (delta, delta_centre and the two forms NaN; the
// gradients, seg2 and the sums of ||r||^2 valid); 2 a non-finite value in what is read (every output of the star NaN).
#pragma clang fp contract(off)
#include "dense_f64.h"                             // after the pragma: the helpers are compiled without contraction

namespace {

constexpr int NT = 256;
static_assert(NT == F64_NT, "dense_f64.h is written for this workgroup size");
constexpr int MAXD = 128;
constexpr int MAXK = 64;
constexpr int LDS_MAXD = 64;                      // widest d whose window sits in LDS
constexpr int PART = 4 * NT;                      // doubles: the J^T s partials [row group][4 LP]; the trees use the first NT
constexpr int SMALL = PART + 3 * MAXD;            // + delta of this block, delta of the next block, w; then the window / triangle

inline __host__ __device__ int window_stride(int d) { return 2 * d + 1; }
inline __host__ __device__ long long save_doubles(int d) { return (long long)(2 * d + 1) * d; }
inline __host__ __device__ long long window_doubles(int d) { return d > LDS_MAXD ? (long long)(2 * d + 1) * window_stride(d) : 0; }
// the head of an arm's slice: T_k [d][d] (lower triangle), r_k [d], g^c_k [d], the arm's code
inline __host__ __device__ long long head_doubles(int d) { return (long long)d * d + 2 * d + 1; }

// MODE 1: the window in LDS (d <= 64); 2: the window in the workspace slice
template <int MODE>
__global__ __launch_bounds__(NT) void star_forward_kernel(const float* __restrict__ t, long long t_b, long long t_r, int n_rows, int d,
                                                           int LP, int P, int K, const float* __restrict__ jtj,
                                                           const float* __restrict__ cross, const float* __restrict__ xhat,
                                                           const double* __restrict__ damping, double* grad,
                                                           double* __restrict__ arm_stats, double* __restrict__ seg2, double* ws,
                                                           long long ws_slice) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, N = P - 1, M = P - 2;
  const long long a = blockIdx.x, q0 = a * P;     // the arm and its first sample
  double* part = lds;
  const float* __restrict__ xc = xhat + q0 * n_rows;

  // 1. ||r_i||^2 and their sum
  int bad = 0;
  double esum = 0.0;
  for (int i = 0; i < N; ++i) {
    const float* __restrict__ u0 = xc + (long long)i * n_rows;
    const float* __restrict__ u1 = u0 + n_rows;
    double acc = 0.0;
    for (int r = tid; r < n_rows; r += NT) {
      const float u = u0[r], v = u1[r];
      bad |= not_finite(u) | not_finite(v);
      const double rr = (double)v - (double)u;
      acc += rr * rr;
    }
    const double s = block_fold<false>(acc, part);
    esum += s;
    if (tid == 0) seg2[a * N + i] = s;             // the backward kernel rewrites it when the star is bad
  }

  const long long dd = (long long)d * d, Md = (long long)M * d;
  double* gc = grad + a * Md;
  double* head = ws + a * ws_slice;
  double* Tk = head;
  double* rk = Tk + dd;
  double* gcen = rk + d;
  double* code = gcen + d;

  // 2. g_i = J_i^T s_i for the interior points and the centre copy; thread k < d keeps g_ik in turn and the running max |g_ik|
  double gmax = 0.0;
  for (int i = 1; i <= N; ++i) {
    const float* __restrict__ x0 = xc + (long long)i * n_rows;
    const float* __restrict__ xm = x0 - n_rows;
    const bool centre = i == N;                     // uniform: the centre copy has no point after it
    const float* __restrict__ xp = centre ? x0 : x0 + n_rows;
    jt_stream(t + (q0 + i) * t_b, t_r, n_rows, d, LP, part,
              [=](int r) {
                const double um = (double)xm[r], u0 = (double)x0[r], up = (double)xp[r];
                return centre ? um - u0 : (um + up) - 2.0 * u0;
              },
              bad);
    __syncthreads();
    if (tid < d) {
      double gk = 0.0;
      for (int q = 0; q < NT / LP; ++q) gk += part[q * (4 * LP) + tid];
      if (i < N) {
        gc[(long long)(i - 1) * d + tid] = gk;     // read back by this same thread only
        const double ag = fabs(gk);
        gmax = ag > gmax ? ag : gmax;
      } else {
        gcen[tid] = gk;
      }
    }
    __syncthreads();
  }
  // the parts of jtj and cross that are read
  for (int i = 1; i <= N; ++i) {
    const float* __restrict__ G = jtj + (q0 + i) * dd;
    for (int e = tid; e < dd; e += NT) {
      const int r = e / d, c = e - r * d;
      if (c <= r) bad |= not_finite(G[e]);
    }
  }
  const float* __restrict__ Cc = cross + (q0 + 1) * dd;            // the pairs (i, i + 1), i = 1 .. M
  for (long long e = tid; e < (long long)M * dd; e += NT) bad |= not_finite(Cc[e]);
  if (__syncthreads_or(bad)) {                    // uniform
    if (tid == 0) code[0] = 2.0;
    return;
  }
  gmax = block_fold<true>(gmax, part);
  if (tid == 0) {
    arm_stats[4 * a] = esum;
    arm_stats[4 * a + 3] = gmax;
  }

  // 3. block elimination: M blocks, each with the block after it in the window
  double* A = lds + SMALL;
  const long long SAVE = save_doubles(d);
  double* saves = head + head_doubles(d);
  double* W = MODE == 1 ? A : saves + (long long)M * SAVE;
  const int LD = window_stride(d), R = 2 * d;
  const double lam = damping[a / K];

  // diagonal block of point i at window offset o (0 or d), its g in the extra row; the centre copy counts once
  auto load_block = [&](int i, int o) {
    const float* __restrict__ G = jtj + (q0 + i) * dd;
    const double factor = i == N ? 1.0 : 2.0;
    for (int e = tid; e < dd; e += NT) {
      const int r = e / d, c = e - r * d;
      if (c <= r) {
        const double v = factor * (double)G[e];
        W[(o + r) * LD + o + c] = r == c ? v + lam * v : v;
      }
    }
    if (tid < d) W[R * LD + o + tid] = i == N ? gcen[tid] : gc[(long long)(i - 1) * d + tid];
  };
  load_block(1, 0);
  int fail = 0;
  for (int i = 1; i <= M; ++i) {
    const float* __restrict__ Ci = Cc + (long long)(i - 1) * dd;     // lower left: -C_i^T
    for (int e = tid; e < dd; e += NT) {
      const int c = e / d, r = e - c * d;
      W[(d + r) * LD + c] = -(double)Ci[e];
    }
    load_block(i + 1, d);
    __syncthreads();
    fail = eliminate(W, LD, d, R, R, 1);
    if (fail) break;                                // uniform
    // the finished columns: rows 0 .. 2 d - 1 and the extra row, columns 0 .. d - 1
    double* Ls = saves + (long long)(i - 1) * SAVE;
    for (int e = tid; e < (R + 1) * d; e += NT) {
      const int r = e / d, k = e - r * d;
      if (r >= d || k <= r) Ls[e] = W[r * LD + k];
    }
    __syncthreads();
    if (i < M) {                                    // S_{i+1} and its g to the upper left
      for (int e = tid; e < dd; e += NT) {
        const int r = e / d, c = e - r * d;
        if (c <= r) W[r * LD + c] = W[(d + r) * LD + d + c];
      }
      if (tid < d) W[R * LD + tid] = W[R * LD + d + tid];
      __syncthreads();
    }
  }
  if (!fail) {                                      // uniform: T_k and r_k from the lower right
    for (int e = tid; e < dd; e += NT) {
      const int r = e / d, c = e - r * d;
      if (c <= r) Tk[e] = W[(d + r) * LD + d + c];
    }
    if (tid < d) rk[tid] = W[R * LD + d + tid];
  }
  if (tid == 0) code[0] = fail ? 1.0 : 0.0;
}

__global__ __launch_bounds__(NT) void star_centre_kernel(int d, int K, const double* __restrict__ weights,
                                                          const double* __restrict__ ws, long long ws_slice,
                                                          double* __restrict__ grad_centre, double* __restrict__ delta_centre,
                                                          int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, LT = d | 1;
  const long long s = blockIdx.x, dd = (long long)d * d;
  double* dl = lds;                                // [MAXD]
  double* A = lds + MAXD;                          // [(d + 1) * LT]: the triangle, the right-hand side as row d
  const double* __restrict__ w = weights + s * K;
  const double* __restrict__ arms = ws + s * K * ws_slice;
  const double nan = __builtin_nan("");
  double* gcs = grad_centre + s * d;
  double* dcs = delta_centre + s * d;

  int two = 0, one = 0;
  if (tid < K) {                                    // K <= 64
    const double c = arms[tid * ws_slice + dd + 2 * d], wk = w[tid];
    two = c == 2.0 || !(wk > 0.0) || not_finite(wk);
    one = c == 1.0;
  }
  two = __syncthreads_or(two);
  one = __syncthreads_or(one);
  if (two) {                                        // uniform
    if (tid < d) {
      gcs[tid] = nan;
      dcs[tid] = nan;
    }
    if (tid == 0) info[s] = 2;
    return;
  }
  if (tid < d) {
    double g = 0.0;
    for (int k = 0; k < K; ++k) g += w[k] * arms[k * ws_slice + dd + d + tid];
    gcs[tid] = g;
  }
  int fail = one;
  if (!fail) {
    for (int e = tid; e < dd; e += NT) {
      const int r = e / d, c = e - r * d;
      if (c <= r) {
        double v = 0.0;
        for (int k = 0; k < K; ++k) v += w[k] * arms[k * ws_slice + e];
        A[r * LT + c] = v;
      }
    }
    if (tid < d) {
      double v = 0.0;
      for (int k = 0; k < K; ++k) v += w[k] * arms[k * ws_slice + dd + tid];
      A[d * LT + tid] = v;
    }
    __syncthreads();
    fail = eliminate(A, LT, d, d, d, 1);
  }
  if (fail) {                                       // uniform
    if (tid < d) dcs[tid] = nan;
    if (tid == 0) info[s] = 1;
    return;
  }
  back_substitute(A, LT, d, A + d * LT, dl);
  if (tid < d) dcs[tid] = dl[tid];
  if (tid == 0) info[s] = 0;
}

__global__ __launch_bounds__(NT) void star_backward_kernel(int d, int P, int K, const float* __restrict__ jtj,
                                                            const float* __restrict__ cross, const double* __restrict__ weights,
                                                            const double* __restrict__ delta_centre, const int* __restrict__ info,
                                                            double* grad, double* __restrict__ delta, double* __restrict__ arm_stats,
                                                            double* __restrict__ seg2, const double* __restrict__ ws,
                                                            long long ws_slice) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, N = P - 1, M = P - 2;
  const long long a = blockIdx.x, q0 = a * P, star = a / K;
  const long long dd = (long long)d * d, Md = (long long)M * d;
  double* part = lds;
  double* dcur = lds + PART;                      // [MAXD]
  double* dnext = dcur + MAXD;                    // [MAXD]
  double* wv = dnext + MAXD;                      // [MAXD]
  double* A = lds + SMALL;                        // the triangle of one block
  double* gc = grad + a * Md;
  double* dc = delta + a * Md;
  const double nan = __builtin_nan("");
  const int code = info[star];                    // uniform
  const double wk = weights[a];

  if (code == 2) {
    for (long long k = tid; k < Md; k += NT) {
      gc[k] = nan;
      dc[k] = nan;
    }
    for (int i = tid; i < N; i += NT) seg2[a * N + i] = nan;
    if (tid < 4) arm_stats[4 * a + tid] = nan;
    return;
  }
  if (code == 1) {
    for (long long k = tid; k < Md; k += NT) {
      gc[k] = wk * gc[k];
      dc[k] = nan;
    }
    if (tid == 1 || tid == 2) arm_stats[4 * a + tid] = nan;
    return;
  }

  const double* head = ws + a * ws_slice;
  const double* gcen = head + dd + d;
  const double* saves = head + head_doubles(d);
  const long long SAVE = save_doubles(d);
  const float* __restrict__ Cc = cross + (q0 + 1) * dd;
  const int LT = d | 1, R = 2 * d;

  // 4. back substitution, block M first, with delta_centre as the block after it; the two forms start with the centre's terms
  if (tid < d) dnext[tid] = delta_centre[star * d + tid];
  __syncthreads();
  double gd = 0.0, qf = 0.0;
  if (tid < d) gd = gcen[tid] * dnext[tid];
  {
    const float* __restrict__ G = jtj + (q0 + N) * dd;
    for (int e = tid; e < dd; e += NT) {
      const int r = e / d, c = e - r * d;
      if (c <= r) {
        const double term = (double)G[e] * dnext[r] * dnext[c];
        qf += c < r ? 2.0 * term : term;
      }
    }
  }
  for (int i = M; i >= 1; --i) {
    const double* Ls = saves + (long long)(i - 1) * SAVE;
    for (int e = tid; e < dd; e += NT) {
      const int r = e / d, c = e - r * d;
      if (c <= r) A[r * LT + c] = Ls[e];
    }
    if (tid < d) {
      double acc = 0.0;
      for (int r = 0; r < d; ++r) acc += Ls[(long long)(d + r) * d + tid] * dnext[r];
      wv[tid] = Ls[(long long)R * d + tid] - acc;
    }
    __syncthreads();
    back_substitute(A, LT, d, wv, dcur);
    if (tid < d) {
      const double dk = dcur[tid];
      dc[(long long)(i - 1) * d + tid] = dk;
      gd += gc[(long long)(i - 1) * d + tid] * dk;
    }
    const float* __restrict__ G = jtj + (q0 + i) * dd;
    for (int e = tid; e < dd; e += NT) {
      const int r = e / d, c = e - r * d;
      if (c <= r) {
        const double term = (double)G[e] * dcur[r] * dcur[c];
        qf += c < r ? 4.0 * term : 2.0 * term;
      }
    }
    const float* __restrict__ Ci = Cc + (long long)(i - 1) * dd;
    for (int e = tid; e < dd; e += NT) {
      const int r = e / d, c = e - r * d;
      qf -= 2.0 * ((double)Ci[e] * dcur[r] * dnext[c]);
    }
    __syncthreads();
    if (tid < d) dnext[tid] = dcur[tid];
    __syncthreads();
  }
  gd = block_fold<false>(gd, part);
  qf = block_fold<false>(qf, part);               // its barriers order the reads of gc above before the scaling below
  if (tid == 0) {
    arm_stats[4 * a + 1] = gd;
    arm_stats[4 * a + 2] = qf;
  }
  for (long long k = tid; k < Md; k += NT) gc[k] = wk * gc[k];
}

long long slice_doubles(int d, int points) { return head_doubles(d) + (long long)(points - 2) * save_doubles(d) + window_doubles(d); }

bool shape_ok(int d, int points, int arms, int stars) {
  if (d < 1 || d > MAXD || points < 3 || arms < 1 || arms > MAXK || stars < 1) return false;
  if ((long long)points * arms * stars > 0x7fffffffLL) return false;
  return slice_doubles(d, points) <= 0x7fffffffffffLL / ((long long)arms * stars);
}

}  // namespace

extern "C" long long cmf_star_step_ws(int d, int points, int arms, int stars) {
  if (!shape_ok(d, points, arms, stars)) return CMF_EINVAL;
  return slice_doubles(d, points) * arms * stars;
}

extern "C" int cmf_star_step(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int points, int arms, int stars,
                             long long first, const float* jtj, const float* cross, const float* xhat, const double* weights,
                             const double* damping, double* grad, double* grad_centre, double* delta, double* delta_centre,
                             double* arm_stats, double* seg2, int* info, double* ws, long long ws_doubles, void* stream) {
  if (!t || !jtj || !cross || !xhat || !weights || !damping || !grad || !grad_centre || !delta || !delta_centre || !arm_stats ||
      !seg2 || !info || !ws)
    return CMF_EINVAL;
  if (n_rows <= 0 || first < 0 || !shape_ok(d, points, arms, stars) || nc % 16 || d > nc) return CMF_EINVAL;
  if (bad_panel(t, t_b, t_r, nc)) return CMF_EINVAL;
  if ((uintptr_t)jtj % 4 || (uintptr_t)cross % 4 || (uintptr_t)xhat % 4 || (uintptr_t)info % 4) return CMF_EINVAL;
  if ((uintptr_t)weights % 8 || (uintptr_t)damping % 8 || (uintptr_t)grad % 8 || (uintptr_t)grad_centre % 8 || (uintptr_t)delta % 8 ||
      (uintptr_t)delta_centre % 8 || (uintptr_t)arm_stats % 8 || (uintptr_t)seg2 % 8 || (uintptr_t)ws % 8)
    return CMF_EINVAL;
  const long long slice = slice_doubles(d, points);
  const int n_arms = arms * stars;
  if (ws_doubles < slice * n_arms) return CMF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int LP = jt_lanes(nc);
  const float* t0 = t + first * t_b;
  const bool in_lds = d <= LDS_MAXD;
  const size_t lds_f = sizeof(double) * ((size_t)SMALL + (in_lds ? (size_t)(2 * d + 1) * window_stride(d) : 0));
  const size_t lds_c = sizeof(double) * ((size_t)MAXD + (size_t)(d + 1) * (d | 1));
  const size_t lds_b = sizeof(double) * ((size_t)SMALL + (size_t)d * (d | 1));
  auto fwd = in_lds ? star_forward_kernel<1> : star_forward_kernel<2>;
  int e = raise_lds(fwd, lds_f);
  if (!e) e = raise_lds(star_centre_kernel, lds_c);
  if (!e) e = raise_lds(star_backward_kernel, lds_b);
  if (e) return e;
  hipLaunchKernelGGL(fwd, dim3(n_arms), dim3(NT), lds_f, s, t0, t_b, t_r, n_rows, d, LP, points, arms, jtj, cross, xhat, damping, grad,
                     arm_stats, seg2, ws, slice);
  CMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(star_centre_kernel, dim3(stars), dim3(NT), lds_c, s, d, arms, weights, ws, slice, grad_centre, delta_centre, info);
  CMF_LAUNCH_CHECK();
  hipLaunchKernelGGL(star_backward_kernel, dim3(n_arms), dim3(NT), lds_b, s, d, points, arms, jtj, cross, weights, delta_centre,
                     info, grad, delta, arm_stats, seg2, ws, slice);
  CMF_LAUNCH_CHECK();
  return 0;
}
