// Per-sample spectrum of the Gram matrix G = J^T J: all eigenvalues and, on request, the eigenvectors.
//
// cmf_gram_spectrum reads the lower triangle of jtj [B][d][d] (float32, as cmf_gram_cholesky leaves it after ONE attempt) and
// diagonalises it in float64 by the cyclic two-sided Jacobi method.  One 256-thread workgroup per sample; the matrix A lives
// in LDS as float64 with an odd row stride (d | 1: the column update of several rows by one wave then spreads over the banks),
// at d = 128 that is 129 KiB of the CU's 160 KiB.
//
// Ordering.  Round-robin ("tournament") on n = d rounded up to even players: step s = 0 .. n - 2 pairs player n - 1 with s and,
// for k = 1 .. n/2 - 1, (s + k) mod (n - 1) with (s - k) mod (n - 1); a pair that contains player d (odd d: the one that sits
// out) is skipped.  A sweep is n - 1 steps of floor(d / 2) disjoint pairs p < q, fixed by d alone.
//
// One step, three phases separated by barriers:
//   (a) one thread per pair: rotate iff |a_qp| > 2^-53 sqrt(|a_pp a_qq|) (relative: on a positive-definite matrix the small
//       eigenvalues converge to relative accuracy).  theta = (a_qq - a_pp) / (2 a_qp), t = sign(theta) / (|theta| +
//       sqrt(1 + theta^2)) (theta = 0: t = 1; infinite theta: t = 0), c = 1 / sqrt(1 + t^2), s = t c.  c, s and the new diagonal
//       a_pp - t a_qp, a_qq + t a_qp (the closed form, from the values BEFORE the rotation) go to LDS.
//   (b) A <- A R, one rotation per (row, pair): col_p' = c col_p - s col_q, col_q' = s col_p + c col_q; the same on V.
//   (c) A <- R^T A, one rotation per (pair, column); a_pq = a_qp = 0 exactly and the diagonal from (a).
// The sweeps end after the first one in which no pair rotated (__syncthreads_or), or after CMF_SPECTRUM_MAX_SWEEPS.
// No fused multiply-adds (fp contract off): every operation is one correctly rounded float64 operation, so the numbers are those
// of a plain float64 emulation of the same sequence, and identical with and without eigenvectors.
//
// V starts as the identity and takes phase (b) only: in LDS beside A for d <= 64, in the sample's own slice of `vectors` for
// 64 < d (touched by its owning workgroup only; __syncthreads orders the steps).  At the end the eigenvalues are ranked by
// counting (ascending, equal values in diagonal order), each column's sign is fixed (largest-magnitude component positive,
// lowest row on ties) and the columns are written in rank order -- for 64 < d through the LDS tile A has vacated.
//
// A sample's result depends on its d x d input alone: no atomics, nothing shared between workgroups.
#include "dense_f64.h"                             // row_stride alone: none of its float64 helpers is used here

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int MAXD = 128;
constexpr int VEC_LDS_MAXD = 64;                  // widest V that sits in LDS beside A
constexpr int MAXPAIR = MAXD / 2;
// LDS before A, in doubles: c, s, new a_pp, new a_qq per pair; eigenvalues and column signs; then p, q per pair and the ranks (ints)
constexpr int SMALL = 4 * MAXPAIR + 2 * MAXD + (2 * MAXPAIR + MAXD) / 2;


// VM: 0 = no eigenvectors, 1 = V in LDS, 2 = V in the output slice
template <int VM>
__global__ __launch_bounds__(NT) void gram_spectrum_kernel(const float* __restrict__ jtj, int d, double* __restrict__ eig,
                                                           double* vec, int* __restrict__ sweeps, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, b = blockIdx.x, LD = row_stride(d), dd = d * d;
  double* rc = lds;                               // [MAXPAIR] each
  double* rs = rc + MAXPAIR;
  double* rpp = rs + MAXPAIR;
  double* rqq = rpp + MAXPAIR;
  double* lam = rqq + MAXPAIR;                    // [MAXD]
  double* sgn = lam + MAXD;                       // [MAXD]
  int* ip = (int*)(sgn + MAXD);                   // [MAXPAIR]: p of a pair that rotates in this step, else -1
  int* iq = ip + MAXPAIR;                         // [MAXPAIR]
  int* rnk = iq + MAXPAIR;                        // [MAXD]
  double* A = lds + SMALL;
  double* out = VM ? vec + (long long)b * dd : nullptr;
  double* V = VM == 1 ? A + d * LD : out;
  const int LV = VM == 1 ? LD : d;

  const float* __restrict__ G = jtj + (long long)b * dd;
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
  if (__syncthreads_or(bad)) {                    // uniform
    const double nan = __builtin_nan("");
    for (int k = tid; k < d; k += NT) eig[(long long)b * d + k] = nan;
    if (VM)
      for (int e = tid; e < dd; e += NT) out[e] = nan;
    if (tid == 0) {
      sweeps[b] = 0;
      info[b] = 2;
    }
    return;
  }
  if (VM) {
    for (int e = tid; e < dd; e += NT) {
      const int i = e / d, j = e - i * d;
      V[i * LV + j] = i == j ? 1.0 : 0.0;
    }
  }

  const int n = d + (d & 1), n1 = n - 1, npair = n >> 1;
  int KP = 1, DP = 1;
  while (KP < npair) KP <<= 1;                    // <= 64
  while (DP < d) DP <<= 1;                        // <= 128
  const int kb = tid & (KP - 1), rb = tid / KP, rstep = NT / KP;       // phase (b): pair kb, rows rb, rb + rstep, ...
  const int jc = tid & (DP - 1), kc = tid / DP, kstep = NT / DP;       // phase (c): column jc, pairs kc, kc + kstep, ...

  int nsweep = 0, any = 1;
  while (any && nsweep < CMF_SPECTRUM_MAX_SWEEPS) {
    int rot = 0;
    for (int s = 0; s < n1; ++s) {
      if (tid < npair) {                          // (a); the barrier that ended the previous step (or the load) published A
        const int u = tid == 0 ? n1 : (s + tid) % n1, v = tid == 0 ? s : (s + n1 - tid) % n1;
        const int p = u < v ? u : v, q = u < v ? v : u;
        int pk = -1;
        if (q < d) {
          const double apq = A[q * LD + p], app = A[p * LD + p], aqq = A[q * LD + q];
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
          for (int r = rb; r < d; r += rstep) {
            const double x = A[r * LD + p], y = A[r * LD + q];
            A[r * LD + p] = c * x - sn * y;
            A[r * LD + q] = sn * x + c * y;
          }
          if (VM) {
            for (int r = rb; r < d; r += rstep) {
              const double x = V[r * LV + p], y = V[r * LV + q];
              V[r * LV + p] = c * x - sn * y;
              V[r * LV + q] = sn * x + c * y;
            }
          }
        }
      }
      __syncthreads();
      if (jc < d) {                               // (c)
        for (int k = kc; k < npair; k += kstep) {
          const int p = ip[k];
          if (p < 0) continue;
          const int q = iq[k];
          const double c = rc[k], sn = rs[k];
          const double x = A[p * LD + jc], y = A[q * LD + jc];
          double xn = c * x - sn * y, yn = sn * x + c * y;
          if (jc == p) {
            xn = rpp[k];
            yn = 0.0;
          } else if (jc == q) {
            xn = 0.0;
            yn = rqq[k];
          }
          A[p * LD + jc] = xn;
          A[q * LD + jc] = yn;
        }
      }
      __syncthreads();
    }
    any = __syncthreads_or(rot);
    ++nsweep;
  }

  // eigenvalue order by counting, column signs
  if (tid < d) lam[tid] = A[tid * LD + tid];
  __syncthreads();
  if (tid < d) {
    const double li = lam[tid];
    int r = 0;
    for (int j = 0; j < d; ++j) r += lam[j] < li || (lam[j] == li && j < tid);
    rnk[tid] = r;                                 // a permutation of 0 .. d - 1 for finite values; always inside [0, d)
    eig[(long long)b * d + r] = li;
    if (VM) {
      double best = -1.0, bv = 1.0;
      for (int i = 0; i < d; ++i) {
        const double v = V[i * LV + tid];
        if (fabs(v) > best) {
          best = fabs(v);
          bv = v;
        }
      }
      sgn[tid] = bv < 0.0 ? -1.0 : 1.0;
    }
  }
  if (tid == 0) {
    sweeps[b] = nsweep;
    info[b] = any ? 1 : 0;
  }
  if (VM) {
    __syncthreads();
    if (VM == 2) {                                // the ordered copy is in place: stage V in the tile A has vacated
      for (int e = tid; e < dd; e += NT) {
        const int i = e / d, j = e - i * d;
        A[i * LD + j] = V[e];
      }
      __syncthreads();
    }
    const double* S = VM == 2 ? A : V;
    for (int e = tid; e < dd; e += NT) {
      const int i = e / d, j = e - i * d;
      out[i * d + rnk[j]] = sgn[j] * S[i * LD + j];
    }
  }
}

template <int VM>
int launch(const float* jtj, int d, int B, double* eig, double* vec, int* sweeps, int* info, hipStream_t s) {
  const size_t lds = sizeof(double) * ((size_t)SMALL + (size_t)d * row_stride(d) * (VM == 1 ? 2 : 1));
  if (int e = raise_lds(gram_spectrum_kernel<VM>, lds)) return e;
  hipLaunchKernelGGL(gram_spectrum_kernel<VM>, dim3(B), dim3(NT), lds, s, jtj, d, eig, vec, sweeps, info);
  CMF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cmf_gram_spectrum(const float* jtj, int d, int B, double* eigenvalues, double* vectors, int* sweeps, int* info,
                                 void* stream) {
  if (!jtj || !eigenvalues || !sweeps || !info || d < 1 || d > MAXD || B <= 0) return CMF_EINVAL;
  if ((uintptr_t)eigenvalues % 8 || (uintptr_t)vectors % 8) return CMF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (!vectors) return launch<0>(jtj, d, B, eigenvalues, nullptr, sweeps, info, s);
  if (d <= VEC_LDS_MAXD) return launch<1>(jtj, d, B, eigenvalues, vectors, sweeps, info, s);
  return launch<2>(jtj, d, B, eigenvalues, vectors, sweeps, info, s);
}
