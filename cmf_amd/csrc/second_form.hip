// The second fundamental form of the manifold in a latent frame, per sample: the float64 reduction between two decode
// sweeps and the curvature tensors the host forms from it.
//
// cmf_second_form takes, per sample, the Jacobian stack t of the centre sweep (all d columns of J), the metric G = J^T J of one
// cmf_gram_cholesky attempt (float32, the lower triangle is read), a frame of m unit latent directions u_0 .. u_{m-1}, the step h and
// the shifted sweep s: for every direction a and sign the m columns J(z +- h u_a) u_c.  With q = m (m + 1) / 2 pairs p = (a, b),
// a <= b, a-major, it computes in float64
//   delta_ab[r] = s(+a)[r][b] - s(-a)[r][b]              (exact: a difference of two float32)
//   E_p[r]      = delta_ab[r] + delta_ba[r]              H_p = E_p / (4 h): the symmetrised mixed second derivative of the decoder
//   A  = J^T H   (d x q)      S2 = H^T H   (q x q)       N = S2 - A^T G^-1 A: the Gram matrix of the normal components II_p
//   Gamma_p = G^-1 A_p        g_ab = u_a^T G u_b
//   stats = { sum_{a<b} ||D_ab - D_ba||^2, sum_{a<b} ||H_ab||^2, trace S2, trace N },  D_ab = delta_ab / (2 h).
// One 256-thread workgroup per sample; nothing is shared between workgroups, there are no atomics.  All arithmetic is float64
// without contraction: one rounded operation per multiply and per add, which tests/_second_form_emulation.py repeats in numpy.
//
// Where the division by the step happens: every sum over the rows is taken over the RAW differences (E_p, delta_ab - delta_ba), and
// each folded sum is divided once, by w = 4 h (A), by w w (S2, the H sum) or by w w / 4 (the D sum).  w is exact; w w is one rounding,
// none when h is a power of two.
//
//   1. A streams J once.  LP = 4 .. 32 lanes (the power of two >= min(nc, 128) / 4) run along the columns with one 16-byte load each,
//      the 256 / LP row groups stride over the rows; every live thread also loads the 2 m first quarter-rows of the shifted sweep
//      (columns 0 .. 3 of its 16), forms the q values E_p[r] and keeps 4 q accumulators.  The partials are folded through LDS in
//      row-group order.  Padding columns (>= d of t, >= m of s) are neither tested nor folded.
//   2. S2 and the two asymmetry sums: thread t re-forms the E values of the rows t, t + 256, ... exactly as phase 1 does and keeps
//      all q (q + 1) / 2 + 2 sums; each is folded by the xor tree of its wave (32, 16, .. 1: every lane ends with the same bits) and the
//      four wave sums are added in wave order.
//   3. G's lower triangle -> the float64 window in LDS (row stride d | 1); u_c = G u_c (j ascending) and g_ab = sum_r u_a[r] (G u_b)[r]
//      (r ascending), the lower triangle computed and mirrored; A^T / w as the q extra rows d .. d + q - 1.
//   4. eliminate(window, d | 1, d, d, d, q) (dense_f64.h): the extra rows end as w_p[k] = y_k L_kk, L y = A_p.
//   5. N_pp' = S2_pp' - sum_k (w_p[k] / p_k) w_p'[k], k ascending, p >= p', mirrored.
//   6. Back substitution on the q rows, last column first (transport_step.hip's forward half): Gamma_p.
// The order of every sum is a function of (d, m, n_rows, nc) alone.
//
// info: 0 ok; 1 a pivot of G that is not positive and finite (second_gram, christoffel, stats[3] = NaN; frame_metric, stats[0 .. 2]
// valid); 2 a non-finite value in the first d columns of t, the first m columns of s, the lower triangle of jtj or in frame, or a
// step that is not finite and > 0 (every float output NaN; found before anything is written, so it takes precedence).
#pragma clang fp contract(off)
#include "dense_f64.h"                             // after the pragma: the helpers are compiled without contraction

namespace {

constexpr int NT = 256;
static_assert(NT == F64_NT, "dense_f64.h is written for this workgroup size");
constexpr int MAXD = 128;
constexpr int MAXM = 4;
constexpr int SM_PART = 0;                        // [4][64] the wave sums of phase 2
constexpr int SM_S2 = SM_PART + NT;               // [64] the folded sums of phase 2: S2's lower triangle, then the D and the H sum
constexpr int SM_ND = SM_S2 + 64;                 // [16] N's diagonal
constexpr int SM_GU = SM_ND + 16;                 // [MAXM * MAXD] G u_c
constexpr int SMALL = SM_GU + MAXM * MAXD;        // then the window, which phase 1's partials [row group][4 LP][q] use first

inline __host__ __device__ int window(int d, int q) {
  const int a = (d + q) * row_stride(d), b = 4 * NT * q;
  return a > b ? a : b;
}

__device__ __forceinline__ void fill(double* p, int n, double v) {
  for (int e = threadIdx.x; e < n; e += NT) p[e] = v;
}

template <int M>
__global__ __launch_bounds__(NT) void second_form_kernel(const float* __restrict__ t, long long t_b, long long t_r, int n_rows, int d,
                                                          int LP, const float* __restrict__ jtj, const float* __restrict__ s,
                                                          long long s_b, long long s_r, const double* __restrict__ frame,
                                                          const double* __restrict__ step, double* __restrict__ second_gram,
                                                          double* __restrict__ christoffel, double* __restrict__ frame_metric,
                                                          double* __restrict__ stats, int* __restrict__ info) {
  constexpr int Q = M * (M + 1) / 2;
  constexpr int NS2 = Q * (Q + 1) / 2;            // + 2 <= 57 lanes of phase 2
  constexpr int NA = (Q * MAXD + NT - 1) / NT;    // entries of A one thread folds, at most
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, b = blockIdx.x;
  double* W = lds + SMALL;
  const int LD = row_stride(d);
  const double nan = __builtin_nan("");
  const float* __restrict__ tp = t + (long long)b * t_b;
  const float* __restrict__ sp = s + (long long)b * (2 * M) * s_b;
  const double* __restrict__ fr = frame + (long long)b * M * d;
  double* ng = second_gram + (long long)b * Q * Q;
  double* ch = christoffel + (long long)b * Q * d;
  double* fm = frame_metric + (long long)b * M * M;
  double* st = stats + 4LL * b;

  // 0. the step and the frame
  const double h = step[b];
  int bad = !(h > 0.0) || not_finite(h);
  for (int e = tid; e < M * d; e += NT) bad |= not_finite(fr[e]);
  const double w = 4.0 * h, w2 = w * w;

  // 1. the partials of J^T E: (row group rg, columns c0 .. c0 + 3) x q
  {
    const int lane = tid & (LP - 1), rg = tid / LP, RG = NT / LP, c0 = 4 * lane;
    double acc[4][Q];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int p = 0; p < Q; ++p) acc[i][p] = 0.0;
    if (c0 < d) {                                 // c0 + 3 < nc: nc is a multiple of 16 and >= d
      const bool m1 = c0 + 1 < d, m2 = c0 + 2 < d, m3 = c0 + 3 < d;
      const float* __restrict__ tc = tp + c0;
#pragma unroll 2
      for (int r = rg; r < n_rows; r += RG) {
        const f32x4 v = *(const f32x4*)(tc + (long long)r * t_r);
        const float* __restrict__ sr = sp + (long long)r * s_r;
        double dl[M][M];
#pragma unroll
        for (int a = 0; a < M; ++a) {
          const f32x4 pl = *(const f32x4*)(sr + (long long)(2 * a) * s_b);
          const f32x4 mi = *(const f32x4*)(sr + (long long)(2 * a + 1) * s_b);
#pragma unroll
          for (int c = 0; c < M; ++c) {
            bad |= not_finite(pl[c]) | not_finite(mi[c]);
            dl[a][c] = (double)pl[c] - (double)mi[c];
          }
        }
        bad |= not_finite(v.x) | (m1 & not_finite(v.y)) | (m2 & not_finite(v.z)) | (m3 & not_finite(v.w));
        const double j0 = (double)v.x, j1 = (double)v.y, j2 = (double)v.z, j3 = (double)v.w;
        int p = 0;
#pragma unroll
        for (int a = 0; a < M; ++a)
#pragma unroll
          for (int c = a; c < M; ++c, ++p) {
            const double E = dl[a][c] + dl[c][a];
            acc[0][p] += j0 * E;
            acc[1][p] += j1 * E;
            acc[2][p] += j2 * E;
            acc[3][p] += j3 * E;
          }
      }
    }
    double* pp = W + (rg * (4 * LP) + c0) * Q;    // < 4 NT Q: rg < RG, c0 + 3 < 4 LP
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int p = 0; p < Q; ++p) pp[i * Q + p] = acc[i][p];
  }

  // 2. S2's lower triangle and the two asymmetry sums, raw: thread t takes the rows t, t + 256, ...
  {
    double a2[NS2 + 2];
#pragma unroll
    for (int e = 0; e < NS2 + 2; ++e) a2[e] = 0.0;
    for (int r = tid; r < n_rows; r += NT) {
      const float* __restrict__ sr = sp + (long long)r * s_r;
      double dl[M][M];
#pragma unroll
      for (int a = 0; a < M; ++a) {
        const f32x4 pl = *(const f32x4*)(sr + (long long)(2 * a) * s_b);
        const f32x4 mi = *(const f32x4*)(sr + (long long)(2 * a + 1) * s_b);
#pragma unroll
        for (int c = 0; c < M; ++c) dl[a][c] = (double)pl[c] - (double)mi[c];
      }
      double E[Q];
      int p = 0;
#pragma unroll
      for (int a = 0; a < M; ++a)
#pragma unroll
        for (int c = a; c < M; ++c, ++p) E[p] = dl[a][c] + dl[c][a];
      int e = 0;
#pragma unroll
      for (int pp = 0; pp < Q; ++pp)
#pragma unroll
        for (int pq = 0; pq <= pp; ++pq, ++e) a2[e] += E[pp] * E[pq];
#pragma unroll
      for (int a = 0; a < M; ++a)
#pragma unroll
        for (int c = a + 1; c < M; ++c) {
          const double x = dl[a][c] - dl[c][a], y = dl[a][c] + dl[c][a];
          a2[NS2] += x * x;
          a2[NS2 + 1] += y * y;
        }
    }
    const int wv = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int e = 0; e < NS2 + 2; ++e) {
      double v = a2[e];
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, 64);
      if (lane == 0) lds[SM_PART + wv * 64 + e] = v;
    }
  }
  __syncthreads();                                // the partials of both phases

  // fold A into registers (the window is about to take G), the phase 2 sums into LDS
  double areg[NA];
  {
    const int RG = NT / LP;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int e = tid + i * NT;
      double sum = 0.0;
      if (e < d * Q)
        for (int g = 0; g < RG; ++g) sum += W[g * (4 * LP) * Q + e];
      areg[i] = sum / w;
    }
    if (tid < NS2 + 2) {
      const double* pt = lds + SM_PART;
      const double sum = ((pt[tid] + pt[64 + tid]) + pt[128 + tid]) + pt[192 + tid];
      lds[SM_S2 + tid] = sum / (tid == NS2 ? 0.25 * w2 : w2);
    }
  }
  __syncthreads();                                // the window is free

  // 3. the lower triangle of G
  const int dd = d * d;
  const float* __restrict__ G = jtj + (long long)b * dd;
  bad |= load_lower<true>(G, d, W, LD);
  if (__syncthreads_or(bad)) {                    // uniform; the barrier also publishes the window.  Nothing has been written yet.
    fill(ng, Q * Q, nan);
    fill(ch, Q * d, nan);
    fill(fm, M * M, nan);
    if (tid < 4) st[tid] = nan;
    if (tid == 0) info[b] = 2;
    return;
  }
  double* gu = lds + SM_GU;                       // [M][d]
  for (int e = tid; e < M * d; e += NT) {
    const int r = e / M, c = e - r * M;
    const double* uc = fr + c * d;
    double sum = 0.0;
    for (int j = 0; j < d; ++j) sum += (j <= r ? W[r * LD + j] : W[j * LD + r]) * uc[j];
    gu[c * d + r] = sum;
  }
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int e = tid + i * NT;
    if (e < d * Q) {
      const int j = e / Q, p = e - j * Q;
      W[(d + p) * LD + j] = areg[i];
    }
  }
  __syncthreads();
  if (tid < M * M) {
    const int a = tid / M, c = tid - a * M;
    if (c <= a) {
      const double* ua = fr + a * d;
      double sum = 0.0;
      for (int r = 0; r < d; ++r) sum += ua[r] * gu[c * d + r];
      fm[a * M + c] = sum;
      fm[c * M + a] = sum;
    }
  }
  double tr2 = 0.0;
  if (tid == 0) {
    int e = 0;
    for (int p = 0; p < Q; ++p) {                 // the diagonal entries sit at p (p + 1) / 2 + p
      e += p;
      tr2 += lds[SM_S2 + e + p];
    }
  }

  // 4. pivots and multipliers; rows d .. d + q - 1 are A^T
  if (eliminate(W, LD, d, d, d, Q)) {             // uniform
    fill(ng, Q * Q, nan);
    fill(ch, Q * d, nan);
    if (tid == 0) {
      st[0] = lds[SM_S2 + NS2];
      st[1] = lds[SM_S2 + NS2 + 1];
      st[2] = tr2;
      st[3] = nan;
      info[b] = 1;
    }
    return;
  }

  // 5. the Schur complement
  if (tid < NS2) {
    int p = 0;
    while ((p + 1) * (p + 2) / 2 <= tid) ++p;
    const int pq = tid - p * (p + 1) / 2;
    const double* wp = W + (d + p) * LD;
    const double* wq = W + (d + pq) * LD;
    double sum = 0.0;
    for (int k = 0; k < d; ++k) sum += (wp[k] / W[k * LD + k]) * wq[k];
    const double n = lds[SM_S2 + tid] - sum;
    ng[p * Q + pq] = n;
    ng[pq * Q + p] = n;
    if (p == pq) lds[SM_ND + p] = n;
  }
  __syncthreads();                                // the rows are free for the back substitution
  if (tid == 0) {
    double trn = 0.0;
    for (int p = 0; p < Q; ++p) trn += lds[SM_ND + p];
    st[0] = lds[SM_S2 + NS2];
    st[1] = lds[SM_S2 + NS2 + 1];
    st[2] = tr2;
    st[3] = trn;
    info[b] = 0;
  }

  // 6. Gamma_p: back substitution on the q rows
  const int ti = tid >> 4, tj = tid & 15;
  for (int r = d - 1; r >= 0; --r) {
    if (ti < Q) {
      double* wr = W + (d + ti) * LD;
      const double x = wr[r] / W[r * LD + r];
      for (int c = tj; c < r; c += 16) wr[c] -= W[r * LD + c] * x;
      if (tj == 0) ch[ti * d + r] = x;
    }
    __syncthreads();
  }
}

template <int M>
int launch(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B, const float* jtj, const float* s,
           long long s_b, long long s_r, const double* frame, const double* step, double* second_gram, double* christoffel,
           double* frame_metric, double* stats, int* info, hipStream_t stream) {
  const int LP = jt_lanes(nc);
  const size_t lds = sizeof(double) * ((size_t)SMALL + (size_t)window(d, M * (M + 1) / 2));
  if (int e = raise_lds(second_form_kernel<M>, lds)) return e;
  hipLaunchKernelGGL(second_form_kernel<M>, dim3(B), dim3(NT), lds, stream, t, t_b, t_r, n_rows, d, LP, jtj, s, s_b, s_r, frame, step,
                     second_gram, christoffel, frame_metric, stats, info);
  CMF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cmf_second_form(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int m, int B,
                               const float* jtj, const float* s, long long s_b, long long s_r, const double* frame,
                               const double* step, double* second_gram, double* christoffel, double* frame_metric, double* stats,
                               int* info, void* stream) {
  if (!t || !jtj || !s || !frame || !step || !second_gram || !christoffel || !frame_metric || !stats || !info) return CMF_EINVAL;
  if (n_rows <= 0 || B <= 0 || d < 1 || d > MAXD || m < 1 || m > MAXM || m > d || nc % 16 || d > nc) return CMF_EINVAL;
  if (bad_panel(t, t_b, t_r, nc)) return CMF_EINVAL;
  if (s_b < 16 || s_r < 16 || (s_b | s_r) % 4 || (uintptr_t)s % 16) return CMF_EINVAL;
  if ((uintptr_t)jtj % 4 || (uintptr_t)frame % 8 || (uintptr_t)step % 8 || (uintptr_t)second_gram % 8 || (uintptr_t)christoffel % 8 ||
      (uintptr_t)frame_metric % 8 || (uintptr_t)stats % 8 || (uintptr_t)info % 4)
    return CMF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  switch (m) {
    case 1: return launch<1>(t, t_b, t_r, n_rows, nc, d, B, jtj, s, s_b, s_r, frame, step, second_gram, christoffel, frame_metric, stats, info, st);
    case 2: return launch<2>(t, t_b, t_r, n_rows, nc, d, B, jtj, s, s_b, s_r, frame, step, second_gram, christoffel, frame_metric, stats, info, st);
    case 3: return launch<3>(t, t_b, t_r, n_rows, nc, d, B, jtj, s, s_b, s_r, frame, step, second_gram, christoffel, frame_metric, stats, info, st);
    default: return launch<4>(t, t_b, t_r, n_rows, nc, d, B, jtj, s, s_b, s_r, frame, step, second_gram, christoffel, frame_metric, stats, info, st);
  }
}
