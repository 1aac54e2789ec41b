// The float64 linear algebra that the per-sample / per-curve manifold kernels share: gn_step.hip, weighted_step.hip,
// shoot_step.hip, transport_step.hip, second_form.hip, curve_step.hip and star_step.hip.  Every piece is
// for one workgroup of F64_NT = 256 threads, all of which call it (the barriers inside are unconditional), and is inlined into
// its caller.  tangent_pca.hip and gram_spectrum.hip take row_stride alone.
//
// Contraction: this header carries no fp-contract pragma; the helpers take the state in force where the header is INCLUDED.
// curve_step.hip, transport_step.hip, star_step.hip and second_form.hip include it after their `#pragma clang fp contract(off)` (one
// rounded operation per multiply and add); gn_step.hip, weighted_step.hip and shoot_step.hip have no pragma and fuse multiply-adds.
// Moving an #include across a pragma, or adding a pragma here, changes output bits.
#pragma once
#include "common.h"

constexpr int F64_NT = 256;

// Row stride (doubles) of an n-column matrix in LDS: odd, so that the column reads of the elimination (16 rows of one column per
// wave) spread over the banks instead of landing on one.
inline __host__ __device__ int row_stride(int n) { return n | 1; }

static __device__ __forceinline__ bool not_finite(float v) { return !(fabsf(v) <= __FLT_MAX__); }
static __device__ __forceinline__ bool not_finite(double v) { return !(fabs(v) <= __DBL_MAX__); }

// Fold one value per thread by a fixed binary tree (sum, or maximum with MAX); the result in every thread.  part: F64_NT doubles
// that nobody else touches between the two barriers that bracket the call.
template <bool MAX>
static __device__ __forceinline__ double block_fold(double v, double* part) {
  const int tid = threadIdx.x;
  part[tid] = v;
  __syncthreads();
  for (int s = F64_NT / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const double a = part[tid], c = part[tid + s];
      part[tid] = MAX ? (c > a ? c : a) : a + c;
    }
    __syncthreads();
  }
  const double out = part[0];
  __syncthreads();                                // part may be rewritten by the caller
  return out;
}

// The float64 copy of the lower triangle of the float32 d x d matrix G, into A at row stride LD.  Returns (CHECK) this thread's
// "a non-finite entry" flag, else 0.  No barrier: the caller publishes A.
template <bool CHECK>
static __device__ __forceinline__ int load_lower(const float* __restrict__ G, int d, double* A, int LD) {
  int bad = 0;
  for (int e = threadIdx.x; e < d * d; e += F64_NT) {
    const int i = e / d, j = e - i * d;
    if (j <= i) {
      const float v = G[e];
      if (CHECK) bad |= not_finite(v);
      A[i * LD + j] = (double)v;
    }
  }
  return bad;
}

// One J^T s stream over the n_rows rows of a Jacobian panel (tp: its first row, row stride t_r floats, 16-byte aligned):
// LP = 4 .. 32 lanes run along the columns with one 16-byte load each, the F64_NT / LP row groups stride over the rows, four
// float64 accumulators per thread; s(r) is the caller's float64 scalar of row r.  The partials of (row group rg, columns
// 4 lane .. 4 lane + 3) land in part[rg * 4 LP + 4 lane ..] (4 F64_NT doubles; the caller's barrier publishes them and its fold
// sums them in row-group order).  Columns >= d are padding: lanes that hold none of the first d load nothing, and the padding
// columns of a live lane are neither tested nor folded.  ORs this thread's "a non-finite entry of J" flag into bad (the caller's
// own flag, not a returned one: the compiler keeps the four loads of the unrolled loop in flight only this way).
inline int jt_lanes(int nc) {                     // LP: the power of two >= min(nc, 128) / 4, at least 4
  int LP = 4;
  while (4 * LP < nc && LP < 32) LP <<= 1;
  return LP;
}

template <class S>
static __device__ __forceinline__ void jt_stream(const float* __restrict__ tp, long long t_r, int n_rows, int d, int LP, double* part,
                                                 S s, int& bad) {
  const int tid = threadIdx.x, lane = tid & (LP - 1), rg = tid / LP, RG = F64_NT / LP, c0 = 4 * lane;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (c0 < d) {                                   // c0 + 3 < nc: nc is a multiple of 16 and >= d
    const bool m1 = c0 + 1 < d, m2 = c0 + 2 < d, m3 = c0 + 3 < d;
    const float* __restrict__ tc = tp + c0;
#pragma unroll 4
    for (int r = rg; r < n_rows; r += RG) {
      const f32x4 v = *(const f32x4*)(tc + (long long)r * t_r);
      const double sr = s(r);
      bad |= not_finite(v.x) | (m1 & not_finite(v.y)) | (m2 & not_finite(v.z)) | (m3 & not_finite(v.w));
      a0 += (double)v.x * sr;
      a1 += (double)v.y * sr;
      a2 += (double)v.z * sr;
      a3 += (double)v.w * sr;
    }
  }
  double* p = part + rg * (4 * LP) + c0;          // < 4 F64_NT: rg < RG, c0 + 3 < 4 LP
  p[0] = a0;
  p[1] = a1;
  p[2] = a2;
  p[3] = a3;
}

// Cholesky without square roots on a lower triangle in A (row stride LD; LDS, or global memory that only this workgroup touches),
// with right-hand sides as extra rows: columns 0 .. nk - 1 of the triangle of extent n >= nk are eliminated,
//   A_rj -= (A_rk / p_k) A_jk   for k < j <= min(r, n - 1),
// over the rows k < r < n and the nx extra rows, which sit at the physical rows x0 .. x0 + nx - 1 and take part like any other
// row -- which IS their forward substitution: they end as w_k = y_k L_kk, L y = rhs.  The pivots p_k land on the diagonal, column k
// keeps the unscaled multipliers L_rk L_kk; for nk < n the lower right is left holding the Schur complement.  16 x 16 threads over
// (rows, columns), one barrier per column; the caller publishes A before the call.  The multiplier is a division: x / x = 1, so a
// duplicate column cancels its pivot exactly.  Returns 1 (uniform) at the first pivot that is not positive and below 1e300.
static __device__ __forceinline__ int eliminate(double* A, int LD, int nk, int n, int x0, int nx) {
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  int fail = 0;
  for (int k = 0; k < nk; ++k) {
    const double piv = A[k * LD + k];             // uniform
    if (!(piv > 0.0) || !(piv < 1.0e300)) {
      fail = 1;
      break;
    }
    for (int r = k + 1 + ti; r < n + nx; r += 16) {
      const int ro = (r < n ? r : x0 + (r - n)) * LD;
      const double ark = A[ro + k] / piv;
      const int jmax = r < n ? r : n - 1;
      for (int j = k + 1 + tj; j <= jmax; j += 16) A[ro + j] -= ark * A[j * LD + k];
    }
    __syncthreads();
  }
  return fail;
}

// Back substitution of one eliminated right-hand side w (d doubles, overwritten) on the d x d triangle in A, last column first:
// out_i = (w_i - sum_{k > i} A_ki out_k) / p_i, one barrier per column; out is published on return.
static __device__ __forceinline__ void back_substitute(const double* A, int LD, int d, double* w, double* out) {
  const int tid = threadIdx.x;
  for (int i = d - 1; i >= 0; --i) {
    const double di = w[i] / A[i * LD + i];
    if (tid < i) w[tid] -= A[i * LD + tid] * di;
    if (tid == i) out[i] = di;
    __syncthreads();
  }
}

// The damped solve of one sample, from "the float64 lower triangle of G is in A (row stride LD, published), thread k < d holds
// g_k in gk" to the end of the kernel: A = G + lam diag(G) with g as row d, eliminate, back_substitute into dl (d doubles of LDS),
// delta, and stats = { cost, g^T delta, delta^T G delta, max |g_k| } with the second form from the float32 lower triangle G in
// global memory (A no longer holds it), element e to thread e mod F64_NT, tree-folded through part (F64_NT doubles).  A refused
// pivot gives info 1: delta and the two forms NaN, cost and max |g_k| valid.  delta, stats and info point at this sample's outputs.
static __device__ __forceinline__ void damped_solve(const float* G, int d, double* A, int LD, double gk, double lam, double cost,
                                                    double* part, double* dl, double* __restrict__ delta,
                                                    double* __restrict__ stats, int* __restrict__ info) {
  const int tid = threadIdx.x;
  const double nan = __builtin_nan("");
  if (tid < d) {
    A[d * LD + tid] = gk;
    const double gkk = A[tid * LD + tid];
    A[tid * LD + tid] = gkk + lam * gkk;
  }
  __syncthreads();
  const int fail = eliminate(A, LD, d, d, d, 1);
  const double gmax = block_fold<true>(tid < d ? fabs(gk) : 0.0, part);
  if (fail) {                                     // uniform
    if (tid < d) delta[tid] = nan;
    if (tid == 0) {
      stats[0] = cost;
      stats[1] = nan;
      stats[2] = nan;
      stats[3] = gmax;
      info[0] = 1;
    }
    return;
  }
  back_substitute(A, LD, d, A + d * LD, dl);
  double gd = 0.0, q = 0.0;
  if (tid < d) {
    const double dk = dl[tid];
    delta[tid] = dk;
    gd = gk * dk;
  }
  for (int e = tid; e < d * d; e += F64_NT) {
    const int i = e / d, j = e - i * d;
    if (j <= i) {
      const double term = (double)G[e] * dl[i] * dl[j];
      q += j < i ? 2.0 * term : term;
    }
  }
  gd = block_fold<false>(gd, part);
  q = block_fold<false>(q, part);
  if (tid == 0) {
    stats[0] = cost;
    stats[1] = gd;
    stats[2] = q;
    stats[3] = gmax;
    info[0] = 0;
  }
}
