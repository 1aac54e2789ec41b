// Principal geodesic analysis of one group of K tangent vectors at a point of the manifold: PCA in the tangent plane
// in the pull-back metric G = J^T J, in its dual (K x K) form, which needs no factorisation of G and is complete because the rank
// is at most K.
//
// cmf_tangent_pca reads the lower triangle of jtj [B][d][d] (float32, as cmf_gram_cholesky leaves it after ONE attempt), the tangent
// vectors V [B][K][d] and the weights w [B][K] (float64).  One 256-thread workgroup per group, everything in float64:
//   phase 1  G lives in LDS as float64 with an odd row stride (d | 1, as in gram_spectrum.hip: 129 KiB at d = 128);
//            y_k = G v_k, one thread per (k, i), j ascending, goes to the group's slice of `covectors`;
//   phase 2  the tile is reused for M (K x (K | 1)) and P beside it: with W = sum_k w_k (arm order), q_kl = sum_i y_k[i] v_l[i]
//            (i ascending, l <= k), M_kl = M_lk = ((sqrt(w_k) sqrt(w_l)) q_kl) / W, norm2_k = q_kk, total = (sum_k w_k q_kk) / W
//            (arm order); then M = P Lambda P^T by the cyclic Jacobi method of gram_spectrum.hip -- the same round-robin ordering,
//            rotation rule, closed-form diagonal and stop, so tests/_jacobi_emulation.jacobi describes it;
//   phase 3  the eigenvalues are ranked by counting, DESCENDING (the reverse of the spectrum kernel's ascending ranks: equal values
//            in descending diagonal order); rank = #{ lambda_j > (d 2^-24) lambda_1 }: below that a float32 metric leaves an
//            eigenvalue undetermined.  For j < rank, with c the column of P that ranks j-th and s_j = sqrt(W lambda_j):
//              u_j[i] = (sum_k (sqrt(w_k) p_kc) v_k[i]) / s_j   (k ascending),     score_kj = (s_j p_kc) / sqrt(w_k),
//            then the sign rule on u_j (largest-magnitude component positive, lowest index on ties) flips both.  For j >= rank
//            directions and scores are 0; the variances are reported as computed.
// The group's slices of `covectors` and `directions` are also working storage: written and read back by their owning workgroup only,
// ordered by __syncthreads (the precedent is the spectrum kernel's `vectors`).
//
// No fused multiply-adds (fp contract off): every operation is one correctly rounded float64 operation in a fixed order, so the
// numbers are those of a plain float64 emulation of the same sequence (tests/_tangent_pca_emulation.py).  A group's result depends
// on its own inputs and on (d, K, r) alone: no atomics, nothing shared between workgroups.
#include "dense_f64.h"                             // row_stride alone: none of its float64 helpers is used here

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int MAXD = 128;
constexpr int MAXK = 64;
constexpr int MAXPAIR = MAXK / 2;
// LDS before the tile, in doubles: c, s, new a_pp, new a_qq per pair; eigenvalues (before the sweeps: q_kk), column signs, sqrt(w), w
// per arm; W; then p, q per pair and the diagonal entry of every rank (ints)
constexpr int SCAL = 2;
constexpr int SMALL = 4 * MAXPAIR + 4 * MAXK + SCAL + (2 * MAXPAIR + MAXK) / 2;


__global__ __launch_bounds__(NT) void tangent_pca_kernel(const float* __restrict__ jtj, const double* __restrict__ vin,
                                                         const double* __restrict__ win, int d, int K, int r,
                                                         double* __restrict__ var, double* dir, double* __restrict__ sc, double* cov,
                                                         double* __restrict__ norm2, double* __restrict__ total,
                                                         int* __restrict__ rank, int* __restrict__ sweeps, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, b = blockIdx.x, LD = row_stride(d), LK = row_stride(K), dd = d * d, Kd = K * d, KK = K * K;
  double* rc = lds;                               // [MAXPAIR] each
  double* rs = rc + MAXPAIR;
  double* rpp = rs + MAXPAIR;
  double* rqq = rpp + MAXPAIR;
  double* lam = rqq + MAXPAIR;                    // [MAXK] each
  double* sgn = lam + MAXK;
  double* sw = sgn + MAXK;
  double* wl = sw + MAXK;
  double* scal = wl + MAXK;                       // [SCAL]
  int* ip = (int*)(scal + SCAL);                  // [MAXPAIR]: p of a pair that rotates in this step, else -1
  int* iq = ip + MAXPAIR;                         // [MAXPAIR]
  int* col = iq + MAXPAIR;                        // [MAXK]: the diagonal entry of descending rank j
  double* A = lds + SMALL;                        // phase 1: G, d x LD
  double* M = A;                                  // phases 2, 3: M and P, K x LK each
  double* P = M + K * LK;

  const float* __restrict__ G = jtj + (long long)b * dd;
  const double* __restrict__ V = vin + (long long)b * Kd;
  double* covb = cov + (long long)b * Kd;
  double* dirb = dir + (long long)b * r * d;
  double* scb = sc + (long long)b * K * r;

  int bad = 0;
  for (int e = tid; e < dd; e += NT) {
    const int i = e / d, j = e - i * d;
    if (j <= i) {
      const float g = G[e];
      bad |= !(fabsf(g) <= __FLT_MAX__);          // NaN or inf
      A[i * LD + j] = (double)g;
      A[j * LD + i] = (double)g;
    }
  }
  for (int e = tid; e < Kd; e += NT) bad |= !(fabs(V[e]) <= __DBL_MAX__);
  if (tid < K) {
    const double x = win[(long long)b * K + tid];
    bad |= !(x > 0.0 && x <= __DBL_MAX__);
    wl[tid] = x;
    sw[tid] = sqrt(x);
  }
  if (__syncthreads_or(bad)) {                    // uniform
    const double nan = __builtin_nan("");
    for (int e = tid; e < r; e += NT) var[(long long)b * r + e] = nan;
    for (int e = tid; e < r * d; e += NT) dirb[e] = nan;
    for (int e = tid; e < K * r; e += NT) scb[e] = nan;
    for (int e = tid; e < Kd; e += NT) covb[e] = nan;
    for (int e = tid; e < K; e += NT) norm2[(long long)b * K + e] = nan;
    if (tid == 0) {
      total[b] = nan;
      rank[b] = 0;
      sweeps[b] = 0;
      info[b] = 2;
    }
    return;
  }

  // phase 1: y_k = G v_k
  if (tid == NT - 1) {
    double W = wl[0];
    for (int k = 1; k < K; ++k) W = W + wl[k];
    scal[0] = W;
  }
  for (int e = tid; e < Kd; e += NT) {
    const int k = e / d, i = e - k * d;
    const double* __restrict__ v = V + k * d;
    const double* a = A + i * LD;
    double y = 0.0;
    for (int j = 0; j < d; ++j) y = y + a[j] * v[j];
    covb[e] = y;
  }
  __syncthreads();                                // G is done with: the tile becomes M and P

  // phase 2: the dual matrix
  const double W = scal[0];
  for (int e = tid; e < KK; e += NT) {
    const int k = e / K, l = e - k * K;
    P[k * LK + l] = k == l ? 1.0 : 0.0;
    if (l <= k) {
      const double* y = covb + k * d;
      const double* __restrict__ v = V + l * d;
      double q = 0.0;
      for (int i = 0; i < d; ++i) q = q + y[i] * v[i];
      const double m = ((sw[k] * sw[l]) * q) / W;
      M[k * LK + l] = m;
      M[l * LK + k] = m;
      if (l == k) {
        norm2[(long long)b * K + k] = q;
        lam[k] = q;
      }
    }
  }
  __syncthreads();
  if (tid == NT - 1) {                            // lam is not written again before the sweeps have ended
    double t = wl[0] * lam[0];
    for (int k = 1; k < K; ++k) t = t + wl[k] * lam[k];
    total[b] = t / W;
  }

  // the sweeps of gram_spectrum.hip on M, width K
  const int n = K + (K & 1), n1 = n - 1, npair = n >> 1;
  int KP = 1, DP = 1;
  while (KP < npair) KP <<= 1;                    // <= 32
  while (DP < K) DP <<= 1;                        // <= 64
  const int kb = tid & (KP - 1), rb = tid / KP, rstep = NT / KP;       // phase (b): pair kb, rows rb, rb + rstep, ...
  const int jc = tid & (DP - 1), kc = tid / DP, kstep = NT / DP;       // phase (c): column jc, pairs kc, kc + kstep, ...

  int nsweep = 0, any = 1;
  while (any && nsweep < CMF_SPECTRUM_MAX_SWEEPS) {
    int rot = 0;
    for (int s = 0; s < n1; ++s) {
      if (tid < npair) {                          // (a); the barrier that ended the previous step (or the set-up) published M
        const int u = tid == 0 ? n1 : (s + tid) % n1, v = tid == 0 ? s : (s + n1 - tid) % n1;
        const int p = u < v ? u : v, q = u < v ? v : u;
        int pk = -1;
        if (q < K) {
          const double apq = M[q * LK + p], app = M[p * LK + p], aqq = M[q * LK + q];
          if (fabs(apq) > 0x1p-53 * sqrt(fabs(app * aqq))) {
            const double th = (aqq - app) / (2.0 * apq);
            const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(1.0 + th * th));
            const double c = 1.0 / sqrt(1.0 + t * t), h = t * apq;
            rc[tid] = c;
            rs[tid] = t * c;
            rpp[tid] = app - h;
            rqq[tid] = aqq + h;
            pk = p;
            rot = 1;
          }
        }
        ip[tid] = pk;
        iq[tid] = q;
      }
      __syncthreads();
      if (kb < npair) {                           // (b)
        const int p = ip[kb];
        if (p >= 0) {
          const int q = iq[kb];
          const double c = rc[kb], sn = rs[kb];
          for (int i = rb; i < K; i += rstep) {
            const double x = M[i * LK + p], y = M[i * LK + q];
            M[i * LK + p] = c * x - sn * y;
            M[i * LK + q] = sn * x + c * y;
          }
          for (int i = rb; i < K; i += rstep) {
            const double x = P[i * LK + p], y = P[i * LK + q];
            P[i * LK + p] = c * x - sn * y;
            P[i * LK + q] = sn * x + c * y;
          }
        }
      }
      __syncthreads();
      if (jc < K) {                               // (c)
        for (int k = kc; k < npair; k += kstep) {
          const int p = ip[k];
          if (p < 0) continue;
          const int q = iq[k];
          const double c = rc[k], sn = rs[k];
          const double x = M[p * LK + jc], y = M[q * LK + jc];
          double xn = c * x - sn * y, yn = sn * x + c * y;
          if (jc == p) {
            xn = rpp[k];
            yn = 0.0;
          } else if (jc == q) {
            xn = 0.0;
            yn = rqq[k];
          }
          M[p * LK + jc] = xn;
          M[q * LK + jc] = yn;
        }
      }
      __syncthreads();
    }
    any = __syncthreads_or(rot);
    ++nsweep;
  }

  // phase 3: descending order by counting, the numerical rank, the modes
  if (tid < K) {
    lam[tid] = M[tid * LK + tid];
    col[tid] = tid;                               // stays inside [0, K) even where an overflow left no order to count
  }
  __syncthreads();
  if (tid < K) {
    const double li = lam[tid];
    int up = 0;
    for (int j = 0; j < K; ++j) up += lam[j] < li || (lam[j] == li && j < tid);
    col[K - 1 - up] = tid;                        // a permutation of 0 .. K - 1 for finite values; always inside [0, K)
  }
  __syncthreads();
  const double thr = ((double)d * 0x1p-24) * lam[col[0]];
  int rk = 0;
  for (int k = 0; k < K; ++k) rk += lam[k] > thr;
  if (tid < r) var[(long long)b * r + tid] = lam[col[tid]];
  if (tid == 0) {
    rank[b] = rk;
    sweeps[b] = nsweep;
    info[b] = any ? 1 : 0;
  }
  for (int e = tid; e < r * d; e += NT) {
    const int j = e / d, i = e - j * d;
    double u = 0.0;
    if (j < rk) {
      const int c = col[j];
      const double den = sqrt(W * lam[c]);
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc = acc + (sw[k] * P[k * LK + c]) * V[k * d + i];
      u = acc / den;
    }
    dirb[e] = u;
  }
  __syncthreads();
  if (tid < r) {
    double best = -1.0, bv = 1.0;
    for (int i = 0; i < d; ++i) {
      const double v = dirb[tid * d + i];
      if (fabs(v) > best) {
        best = fabs(v);
        bv = v;
      }
    }
    sgn[tid] = bv < 0.0 ? -1.0 : 1.0;
  }
  __syncthreads();
  for (int e = tid; e < r * d; e += NT) {         // every thread meets the entries it wrote itself
    const int j = e / d;
    dirb[e] = sgn[j] * dirb[e];
  }
  for (int e = tid; e < K * r; e += NT) {
    const int k = e / r, j = e - k * r;
    double s = 0.0;
    if (j < rk) {
      const int c = col[j];
      s = sgn[j] * ((sqrt(W * lam[c]) * P[k * LK + c]) / sw[k]);
    }
    scb[e] = s;
  }
}

}  // namespace

extern "C" int cmf_tangent_pca(const float* jtj, const double* vectors, const double* weights, int d, int arms, int components, int B,
                               double* variances, double* directions, double* scores, double* covectors, double* norm2,
                               double* total, int* rank, int* sweeps, int* info, void* stream) {
  if (!jtj || !vectors || !weights || !variances || !directions || !scores || !covectors || !norm2 || !total || !rank || !sweeps ||
      !info)
    return CMF_EINVAL;
  if (d < 1 || d > MAXD || arms < 1 || arms > MAXK || components < 1 || components > arms || B < 1) return CMF_EINVAL;
  if ((uintptr_t)vectors % 8 || (uintptr_t)weights % 8 || (uintptr_t)variances % 8 || (uintptr_t)directions % 8 ||
      (uintptr_t)scores % 8 || (uintptr_t)covectors % 8 || (uintptr_t)norm2 % 8 || (uintptr_t)total % 8)
    return CMF_EINVAL;
  if ((uintptr_t)jtj % 4 || (uintptr_t)rank % 4 || (uintptr_t)sweeps % 4 || (uintptr_t)info % 4) return CMF_EINVAL;
  const size_t g = (size_t)d * row_stride(d), m = 2 * (size_t)arms * row_stride(arms);
  const size_t lds = sizeof(double) * ((size_t)SMALL + (g > m ? g : m));
  if (int e = raise_lds(tangent_pca_kernel, lds)) return e;
  hipLaunchKernelGGL(tangent_pca_kernel, dim3(B), dim3(NT), lds, (hipStream_t)stream, jtj, vectors, weights, d, arms, components,
                     variances, directions, scores, covectors, norm2, total, rank, sweeps, info);
  CMF_LAUNCH_CHECK();
  return 0;
}
