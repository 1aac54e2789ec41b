// One damped Gauss-Newton step on a whole discretised curve of the manifold, per curve.
//
// A curve has P points z_0 .. z_{P-1} with fixed ends, N = P - 1 segments and M = P - 2 interior points; samples are curve-major:
// point i of curve c is sample c P + i of the Jacobian stack and of xhat.  With r_i = xhat_{i+1} - xhat_i the Gauss-Newton model
// of 1/2 sum ||r_i||^2 has
//   g_i = J_i^T (xhat_{i-1} + xhat_{i+1} - 2 xhat_i),   H_ii = 2 G_i = 2 J_i^T J_i,   H_{i,i+1} = -C_i = -J_i^T J_{i+1},
// a block tridiagonal H; A = H + lambda diag(H) (Marquardt scaling, as gn_step.hip), delta = A^-1 g.
//
// cmf_cross_gram forms the blocks C_i that cmf_gram_cholesky does not: one 256-thread workgroup per pair of neighbouring interior
// points, 32-row slabs of both Jacobians staged in LDS, v_mfma_f32_16x16x4_f32 with fp32 accumulation.  Every output tile runs
// over all rows in the same order, so the order of a sum depends on (n_rows, nc) alone, not on the tile or on the pair.
//
// cmf_curve_step: one 256-thread workgroup per curve, everything in float64, nothing shared between workgroups, no atomics.
//   1. ||r_i||^2 per segment: thread t sums rows t, t + 256, ..., folded by a fixed binary tree; their sum in segment order.
//      The energy-only launch (t == NULL) is this phase alone, so both modes give the same bits.
//   2. g_i = J_i^T s_i streams J_i once per interior point, as phase 2 of gn_step.hip (dense_f64.h, jt_stream), with the second
//      difference s = (xhat_{i-1} + xhat_{i+1}) - 2 xhat_i formed in float64 on the fly.  Then the lower triangles of jtj and the
//      cross blocks are scanned for non-finite values (info 2 takes precedence over a failed pivot).
//   3. Block elimination on a window of 2 d + 1 rows: [S_i, . ; -C_i^T, 2 G_{i+1} (1 + lambda on the diagonal)] with the g entries of
//      the two blocks as the extra row.  The d columns of block i are eliminated by the pivot-only elimination of gn_step.hip
//      (dense_f64.h, eliminate: d columns of a triangle of extent 2 d, the extra row parked at row 2 d); that leaves the Schur
//      complement S_{i+1} and the forward-substituted g_{i+1} in the lower right, which move to the upper left for the next block.
//      The finished columns (unscaled multipliers, pivots, w_k = y_k L_kk) go to the curve's workspace slice.
//      The window (row stride 2 d + 1: odd) lives in LDS for d <= 64 and in the workspace slice for 64 < d <= 128, where only the
//      owning workgroup touches it and the barriers order the steps.
//   4. Back substitution, last block first: the d x d triangle of a block comes back into LDS, the coupling to the block after it
//      is folded into w by one thread per column, then the back substitution of dense_f64.h.
//      delta^T H delta is summed on the way from the float32 inputs (the window no longer holds H), g^T delta and max |g| alike.
// No fused multiply-adds (fp contract off): every operation is one correctly rounded float64 operation, those of a plain float64
// emulation of the same sequence.
//
// info: 0 ok; 1 a pivot that is not positive and finite (delta, stats[1], stats[2] = NaN; the rest valid); 2 a non-finite value
// in xhat, the first d columns of an interior point's t, the lower triangle of an interior jtj or a cross block (every output NaN).
#pragma clang fp contract(off)
#include "dense_f64.h"                             // after the pragma: the helpers are compiled without contraction

namespace {

constexpr int NT = 256;
static_assert(NT == F64_NT, "dense_f64.h is written for this workgroup size");
constexpr int MAXD = 128;
constexpr int LDS_MAXD = 64;                      // widest d whose window sits in LDS
constexpr int PART = 4 * NT;                      // doubles: the J^T s partials [row group][4 LP]; the trees use the first NT
constexpr int SMALL = PART + 3 * MAXD;            // + delta of this block, delta of the next block, w; then the window / triangle
constexpr int KC = 32;                            // J rows per LDS slab of the cross-Gram kernel

inline __host__ __device__ int window_stride(int d) { return 2 * d + 1; }
inline __host__ __device__ long long save_doubles(int d) { return (long long)(2 * d + 1) * d; }
inline __host__ __device__ long long window_doubles(int d) { return d > LDS_MAXD ? (long long)(2 * d + 1) * window_stride(d) : 0; }

// C = Ja^T Jb for one pair of neighbouring points: NTL x NTL tiles of 16 x 16, wave w owns the row tiles w, w + 4.
template <int NTL>
__global__ __launch_bounds__(256) void cross_gram_kernel(const float* __restrict__ t, long long t_b, long long t_r, int n_rows, int d,
                                                          int points, float* __restrict__ cross) {
  constexpr int NC = NTL * 16;
  constexpr int LDJ = (NC % 32 == 0) ? NC + 16 : NC;
  constexpr int NI = (NTL + 3) / 4;
  constexpr int ITEMS = KC * NC / 4;               // float4 per slab and matrix
  constexpr int NIT = (ITEMS + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Ja = smem;                                // [KC][LDJ]
  float* Jb = smem + KC * LDJ;                     // [KC][LDJ]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, cl = lane & 15;
  const int pairs = points - 3;
  const long long blk = blockIdx.x;
  const long long c = blk / pairs, q = blk - c * pairs;
  const float* ta = t + (c * points + 1 + q) * t_b;
  const float* tb = ta + t_b;

  f32x4 acc[NI][NTL];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NTL; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 pa[NIT], pb[NIT];
  auto prefetch = [&](int k0) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      int i = tid + 256 * it;
      i = i < ITEMS ? i : ITEMS - 1;
      const int row = i / (NC / 4), c4 = i % (NC / 4);
      const bool ok = (k0 + row) < n_rows;
      const long long off = (ok ? (long long)(k0 + row) * t_r : 0) + c4 * 4;
      const f32x4 va = *reinterpret_cast<const f32x4*>(ta + off);
      const f32x4 vb = *reinterpret_cast<const f32x4*>(tb + off);
      pa[it] = ok ? va : f32x4{0.f, 0.f, 0.f, 0.f};
      pb[it] = ok ? vb : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + 256 * it;
      if (i < ITEMS) {
        const int o = (i / (NC / 4)) * LDJ + (i % (NC / 4)) * 4;
        *reinterpret_cast<f32x4*>(Ja + o) = pa[it];
        *reinterpret_cast<f32x4*>(Jb + o) = pb[it];
      }
    }
  };

  prefetch(0);
  for (int k0 = 0; k0 < n_rows; k0 += KC) {
    commit();
    __syncthreads();
    if (k0 + KC < n_rows) prefetch(k0 + KC);
#pragma unroll
    for (int kg = 0; kg < KC / 4; ++kg) {
      const int o = (kg * 4 + kq) * LDJ + cl;
      float bv[NTL];
#pragma unroll
      for (int j = 0; j < NTL; ++j) bv[j] = Jb[o + j * 16];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int it = wave + 4 * i;
        if (it < NTL) {                            // wave-uniform
          const float av = Ja[o + it * 16];
#pragma unroll
          for (int j = 0; j < NTL; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j], acc[i][j], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // tile (it, jt), register r: C[it 16 + kq 4 + r][jt 16 + cl]
  float* out = cross + blk * d * d;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int it = wave + 4 * i;
    if (it < NTL) {
#pragma unroll
      for (int j = 0; j < NTL; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = it * 16 + kq * 4 + r, col = j * 16 + cl;
          if (row < d && col < d) out[row * d + col] = acc[i][j][r];
        }
    }
  }
}

template <int NTL>
int launch_cross(const float* t, long long t_b, long long t_r, int n_rows, int d, int points, long long blocks, float* cross,
                 hipStream_t s) {
  constexpr int NC = NTL * 16;
  constexpr int LDJ = (NC % 32 == 0) ? NC + 16 : NC;
  const size_t lds = (size_t)2 * KC * LDJ * sizeof(float);        // <= 36 KiB
  hipLaunchKernelGGL(cross_gram_kernel<NTL>, dim3((unsigned)blocks), dim3(256), lds, s, t, t_b, t_r, n_rows, d, points, cross);
  CMF_LAUNCH_CHECK();
  return 0;
}

// MODE 0: energy only; 1: the window in LDS (d <= 64); 2: the window in the workspace slice
template <int MODE>
__global__ __launch_bounds__(NT) void curve_step_kernel(const float* __restrict__ t, long long t_b, long long t_r, int n_rows, int d,
                                                         int LP, int P, const float* __restrict__ jtj,
                                                         const float* __restrict__ cross, const float* __restrict__ xhat,
                                                         const double* __restrict__ damping, double* grad, double* delta,
                                                         double* __restrict__ stats, double* __restrict__ seg2,
                                                         int* __restrict__ info, double* ws, long long ws_slice) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, N = P - 1, M = P - 2;
  const long long c = blockIdx.x;
  double* part = lds;
  const float* __restrict__ xc = xhat + c * P * n_rows;
  const double nan = __builtin_nan("");

  // 1. ||r_i||^2 and their sum
  int bad = 0;
  double esum = 0.0;
  for (int i = 0; i < N; ++i) {
    const float* __restrict__ a = xc + (long long)i * n_rows;
    const float* __restrict__ b = a + n_rows;
    double acc = 0.0;
    for (int r = tid; r < n_rows; r += NT) {
      const float u = a[r], v = b[r];
      bad |= not_finite(u) | not_finite(v);
      const double rr = (double)v - (double)u;
      acc += rr * rr;
    }
    const double s = block_fold<false>(acc, part);
    esum += s;
    if (tid == 0) seg2[c * N + i] = s;             // thread 0 rewrites it below when the curve is bad
  }
  if (MODE == 0) {
    bad = __syncthreads_or(bad);
    if (tid == 0) {
      if (bad)
        for (int i = 0; i < N; ++i) seg2[c * N + i] = nan;
      stats[4 * c] = bad ? nan : esum;
      info[c] = bad ? 2 : 0;
    }
    return;
  }

  const long long dd = (long long)d * d, Md = (long long)M * d;
  double* gc = grad + c * Md;
  double* dc = delta + c * Md;

  // 2. g_i = J_i^T s_i for the interior points; thread k < d keeps g_ik in turn and the running max |g_ik|
  double gmax = 0.0;
  for (int i = 1; i <= M; ++i) {
    const float* __restrict__ x0 = xc + (long long)i * n_rows;
    const float* __restrict__ xm = x0 - n_rows;
    const float* __restrict__ xp = x0 + n_rows;
    jt_stream(t + (c * P + i) * t_b, t_r, n_rows, d, LP, part,
              [=](int r) { return ((double)xm[r] + (double)xp[r]) - 2.0 * (double)x0[r]; }, bad);
    __syncthreads();
    if (tid < d) {
      double gk = 0.0;
      for (int q = 0; q < NT / LP; ++q) gk += part[q * (4 * LP) + tid];
      gc[(long long)(i - 1) * d + tid] = gk;       // read back by this same thread only
      const double ag = fabs(gk);
      gmax = ag > gmax ? ag : gmax;
    }
    __syncthreads();
  }
  // the parts of jtj and cross that are read
  for (int i = 1; i <= M; ++i) {
    const float* __restrict__ G = jtj + (c * P + i) * dd;
    for (int e = tid; e < dd; e += NT) {
      const int a = e / d, b = e - a * d;
      if (b <= a) bad |= not_finite(G[e]);
    }
  }
  const float* __restrict__ Cc = cross + c * (P - 3) * dd;          // not dereferenced when P == 3
  for (long long e = tid; e < (long long)(M - 1) * dd; e += NT) bad |= not_finite(Cc[e]);
  if (__syncthreads_or(bad)) {                    // uniform
    for (long long k = tid; k < Md; k += NT) {
      gc[k] = nan;
      dc[k] = nan;
    }
    if (tid == 0) {
      for (int i = 0; i < N; ++i) seg2[c * N + i] = nan;
      for (int k = 0; k < 4; ++k) stats[4 * c + k] = nan;
      info[c] = 2;
    }
    return;
  }
  gmax = block_fold<true>(gmax, part);

  // 3. block elimination
  double* dcur = lds + PART;                      // [MAXD]
  double* dnext = dcur + MAXD;                    // [MAXD]
  double* wv = dnext + MAXD;                      // [MAXD]
  double* A = lds + SMALL;                        // the window (MODE 1), later the triangle of one block
  double* wsc = ws + c * ws_slice;
  const long long SAVE = save_doubles(d);
  double* W = MODE == 1 ? A : wsc + (long long)M * SAVE;
  const int LD = window_stride(d), R = 2 * d;
  const double lam = damping[c];

  // diagonal block of interior point i at window offset o (0 or d), its g in the extra row
  auto load_block = [&](int i, int o) {
    const float* __restrict__ G = jtj + (c * P + i) * dd;
    for (int e = tid; e < dd; e += NT) {
      const int a = e / d, b = e - a * d;
      if (b <= a) {
        const double v = 2.0 * (double)G[e];
        W[(o + a) * LD + o + b] = a == b ? v + lam * v : v;
      }
    }
    if (tid < d) W[R * LD + o + tid] = gc[(long long)(i - 1) * d + tid];
  };
  load_block(1, 0);
  int fail = 0;
  for (int i = 1; i <= M; ++i) {
    const bool last = i == M;
    const int nw = last ? d : 2 * d;
    if (!last) {
      const float* __restrict__ Ci = Cc + (long long)(i - 1) * dd;   // lower left: -C_i^T
      for (int e = tid; e < dd; e += NT) {
        const int b = e / d, a = e - b * d;
        W[(d + a) * LD + b] = -(double)Ci[e];
      }
      load_block(i + 1, d);
    }
    __syncthreads();
    fail = eliminate(W, LD, d, nw, R, 1);
    if (fail) break;                                // uniform
    // the finished columns: rows 0 .. nw - 1 and the extra row (as row 2 d), columns 0 .. d - 1
    double* Ls = wsc + (long long)(i - 1) * SAVE;
    for (int e = tid; e < (nw + 1) * d; e += NT) {
      const int r = e / d, k = e - r * d;
      if (r == nw) Ls[(long long)R * d + k] = W[R * LD + k];
      else if (r >= d || k <= r) Ls[e] = W[r * LD + k];
    }
    __syncthreads();
    if (!last) {                                    // S_{i+1} and its g to the upper left
      for (int e = tid; e < dd; e += NT) {
        const int a = e / d, b = e - a * d;
        if (b <= a) W[a * LD + b] = W[(d + a) * LD + d + b];
      }
      if (tid < d) W[R * LD + tid] = W[R * LD + d + tid];
      __syncthreads();
    }
  }
  if (fail) {                                       // uniform
    for (long long k = tid; k < Md; k += NT) dc[k] = nan;
    if (tid == 0) {
      stats[4 * c] = esum;
      stats[4 * c + 1] = nan;
      stats[4 * c + 2] = nan;
      stats[4 * c + 3] = gmax;
      info[c] = 1;
    }
    return;
  }

  // 4. back substitution, last block first, and the two forms
  const int LT = d | 1;
  double gd = 0.0, qf = 0.0;
  for (int i = M; i >= 1; --i) {
    const bool last = i == M;
    const double* Ls = wsc + (long long)(i - 1) * SAVE;
    for (int e = tid; e < dd; e += NT) {
      const int a = e / d, b = e - a * d;
      if (b <= a) A[a * LT + b] = Ls[e];
    }
    if (tid < d) {
      double acc = 0.0;
      if (!last)
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
    const float* __restrict__ G = jtj + (c * P + i) * dd;
    for (int e = tid; e < dd; e += NT) {
      const int a = e / d, b = e - a * d;
      if (b <= a) {
        const double term = (double)G[e] * dcur[a] * dcur[b];
        qf += b < a ? 4.0 * term : 2.0 * term;
      }
    }
    if (!last) {
      const float* __restrict__ Ci = Cc + (long long)(i - 1) * dd;
      for (int e = tid; e < dd; e += NT) {
        const int a = e / d, b = e - a * d;
        qf -= 2.0 * ((double)Ci[e] * dcur[a] * dnext[b]);
      }
    }
    __syncthreads();
    if (tid < d) dnext[tid] = dcur[tid];
    __syncthreads();
  }
  gd = block_fold<false>(gd, part);
  qf = block_fold<false>(qf, part);
  if (tid == 0) {
    stats[4 * c] = esum;
    stats[4 * c + 1] = gd;
    stats[4 * c + 2] = qf;
    stats[4 * c + 3] = gmax;
    info[c] = 0;
  }
}

template <int MODE>
int launch_step(size_t lds, const float* t, long long t_b, long long t_r, int n_rows, int d, int LP, int P, int curves,
                const float* jtj, const float* cross, const float* xhat, const double* damping, double* grad, double* delta,
                double* stats, double* seg2, int* info, double* ws, long long ws_slice, hipStream_t s) {
  auto k = curve_step_kernel<MODE>;
  if (int e = raise_lds(k, lds)) return e;
  hipLaunchKernelGGL(k, dim3(curves), dim3(NT), lds, s, t, t_b, t_r, n_rows, d, LP, P, jtj, cross, xhat, damping, grad, delta, stats,
                     seg2, info, ws, ws_slice);
  CMF_LAUNCH_CHECK();
  return 0;
}

long long slice_doubles(int d, int points) { return (long long)(points - 2) * save_doubles(d) + window_doubles(d); }

bool shape_ok(int d, int points, int curves) {
  if (d < 1 || d > MAXD || points < 3 || curves < 1) return false;
  if ((long long)points * curves > 0x7fffffffLL) return false;
  return slice_doubles(d, points) <= 0x7fffffffffffLL / curves;
}

}  // namespace

extern "C" int cmf_cross_gram(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int points, int curves,
                              float* cross, void* stream) {
  if (!t || n_rows <= 0 || !shape_ok(d, points, curves)) return CMF_EINVAL;
  if (nc % 16 || d > nc || nc > MAXD) return CMF_EINVAL;
  if (bad_panel(t, t_b, t_r, nc)) return CMF_EINVAL;
  if (points == 3) return 0;                      // no pair of neighbouring interior points
  if (!cross || (uintptr_t)cross % 4) return CMF_EINVAL;
  const long long blocks = (long long)curves * (points - 3);
  if (blocks > 0x7fffffffLL) return CMF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
#define CMF_CROSS_CASE(N) \
  case N: return launch_cross<N>(t, t_b, t_r, n_rows, d, points, blocks, cross, s);
  switch (nc / 16) {
    CMF_CROSS_CASE(1) CMF_CROSS_CASE(2) CMF_CROSS_CASE(3) CMF_CROSS_CASE(4)
    CMF_CROSS_CASE(5) CMF_CROSS_CASE(6) CMF_CROSS_CASE(7) CMF_CROSS_CASE(8)
  }
#undef CMF_CROSS_CASE
  return CMF_EINVAL;
}

extern "C" long long cmf_curve_step_ws(int d, int points, int curves) {
  if (!shape_ok(d, points, curves)) return CMF_EINVAL;
  return slice_doubles(d, points) * curves;
}

extern "C" int cmf_curve_step(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int points, int curves,
                              const float* jtj, const float* cross, const float* xhat, const double* damping, double* grad,
                              double* delta, double* stats, double* seg2, int* info, double* ws, long long ws_doubles,
                              void* stream) {
  if (!xhat || !stats || !seg2 || !info || n_rows <= 0 || points < 3 || curves < 1) return CMF_EINVAL;
  if ((long long)points * curves > 0x7fffffffLL) return CMF_EINVAL;
  if ((uintptr_t)xhat % 4 || (uintptr_t)stats % 8 || (uintptr_t)seg2 % 8 || (uintptr_t)info % 4) return CMF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (!t)                                         // energy only: the other arguments are not looked at
    return launch_step<0>(NT * sizeof(double), nullptr, 0, 0, n_rows, 0, 0, points, curves, nullptr, nullptr, xhat, nullptr, nullptr,
                          nullptr, stats, seg2, info, nullptr, 0, s);
  if (!jtj || !damping || !grad || !delta || !ws || (!cross && points > 3)) return CMF_EINVAL;
  if (!shape_ok(d, points, curves) || nc % 16 || d > nc) return CMF_EINVAL;
  if (bad_panel(t, t_b, t_r, nc)) return CMF_EINVAL;
  if ((uintptr_t)jtj % 4 || (uintptr_t)cross % 4 || (uintptr_t)damping % 8 || (uintptr_t)grad % 8 || (uintptr_t)delta % 8 ||
      (uintptr_t)ws % 8)
    return CMF_EINVAL;
  const long long slice = slice_doubles(d, points);
  if (ws_doubles < slice * curves) return CMF_EINVAL;
  const int LP = jt_lanes(nc);
  const bool in_lds = d <= LDS_MAXD;
  const size_t big = in_lds ? (size_t)(2 * d + 1) * window_stride(d) : (size_t)d * (d | 1);
  const size_t lds = sizeof(double) * ((size_t)SMALL + big);
  return in_lds ? launch_step<1>(lds, t, t_b, t_r, n_rows, d, LP, points, curves, jtj, cross, xhat, damping, grad, delta, stats, seg2,
                                 info, ws, slice, s)
                : launch_step<2>(lds, t, t_b, t_r, n_rows, d, LP, points, curves, jtj, cross, xhat, damping, grad, delta, stats, seg2,
                                 info, ws, slice, s);
}
