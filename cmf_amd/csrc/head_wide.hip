// Jacobian head for wide latents, 128 < nc <= 512 (d up to 512), for gfx950 (MI355X).
//
// The head kernels of gram_chol.hip / gram_backward.hip / hutch_cg.hip keep the whole d x d Gram matrix in LDS, which caps
// them at d = 128 (a 512 x 512 fp32 matrix is 1 MiB; LDS is 160 KiB).  This file carries the same operations for wider panels
// with the matrix in global memory and LDS used for panels only.  The arithmetic is small next to the tangent sweep that feeds it
// (C5-shaped CIFAR at d = 512: Gram 2 * 3072 * 512^2 = 1.6 GFLOP, Cholesky d^3 / 3 = 45 MFLOP, the sweep ~3 TFLOP per sample),
// so the kernels are written for exactness and clarity first:
//
//   tile_gemm_kernel   batched C = A B^T over 64 x 64 output tiles, fp32 MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products,
//                      fp32 accumulation), operands staged in LDS in 32-deep slabs with a register prefetch of the next slab.
//                      The grid is (tile, sample): at the small per-GPU batches a d = 512 model forces, one workgroup per sample
//                      would leave most of the chip idle.  Operand offsets are 64-bit (a B x 3072 x 512 panel passes 2 GiB).
//                      Used for the Gram matrix J^T J (lower tiles only, written to both triangles: exactly symmetric), the
//                      backward products dJ = J M, and the Hutchinson cotangent M = A eps^T.
//   ldl_kernel         one workgroup per sample: the pivot-only symmetric elimination of block_cholesky (gram_chol.hip), blocked
//                      right-looking in 32-column panels.  A panel is factorised in LDS, the trailing lower triangle is updated in
//                      global memory with the panel's terms subtracted in column order, so every element sees exactly the
//                      operations of the unblocked sweep (an exactly singular matrix still gives an exact zero pivot).  Only the
//                      lower triangle is touched; for cmf_gram_cholesky the original diagonal is kept in LDS and jtj is restored
//                      from its upper triangle at the end, so the factorisation needs no workspace and leaves jtj intact for its
//                      consumers (g_ij, the backward pass, Hutchinson, head.last_gram).
//   inverse_kernel     G^-1 from the factor (backward pass): forward / backward substitution, one lane per column of G^-1.
//   hutch_wide_kernel  CG on the explicit Gram matrix read from global memory (see the header comment of the kernel).
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// batched fp32 MFMA GEMM:  C(b, m, n) = sum_k A(b, m, k) Bt(b, n, k)
// ------------------------------------------------------------------------------------------------
constexpr int TT = 64;         // output tile edge
constexpr int TK = 32;         // reduction slab depth
constexpr int LDT = TT + 16;   // LDS row stride of a staged slab [k][r]: lanes kq * 80 + cl hit 64 distinct banks

// Element (r, k) of a strided operand: base + b * sb + r * sr + k * sk, zero outside rows x cols.  sym adds the transposed element
// (r <-> k; for the square cotangent matrices of cmf_gram_backward_matrix).
struct Strided {
  const float* p;
  long long sb, sr, sk;
  int rows, cols, sym;
  __device__ float operator()(int b, int r, int k) const {
    if (r >= rows || k >= cols) return 0.f;
    const float* q = p + (long long)b * sb;
    float v = q[(long long)r * sr + (long long)k * sk];
    if (sym) v += q[(long long)k * sr + (long long)r * sk];
    return v;
  }
  __device__ bool r_contiguous() const { return sr == 1; }
};

// Left factor of the Hutchinson cotangent (hutch_cg.hip, hutch_cotangent_kernel): A(i, s) = g_val/S u_is + (g_off [i != s] +
// g_diag [i == s]) sign(w_is), all [B][d][S]
struct HutchLeft {
  const float *u, *w, *gv, *go, *gd;
  int d, S;
  __device__ float operator()(int b, int i, int s) const {
    if (i >= d || s >= S) return 0.f;
    const long long o = ((long long)b * d + i) * S + s;
    float a = gv ? gv[b] / (float)S * u[o] : 0.f;
    const float g = i == s ? (gd ? gd[b] : 0.f) : (go ? go[b] : 0.f);
    if (g != 0.f) {
      const float wv = w[o];
      a += g * (wv > 0.f ? 1.f : (wv < 0.f ? -1.f : 0.f));
    }
    return a;
  }
  __device__ bool r_contiguous() const { return false; }
};

struct Out {
  float* p;
  long long sb, sm, sn;
  int rows, cols;   // stored extent; columns of C beyond Bt's rows are written as exact zeros
};

// SYM: C is symmetric (A == Bt): only tiles with tm >= tn run, element (m, n), m >= n, is stored to (m, n) and (n, m).
template <bool SYM, typename LA, typename LB>
__global__ __launch_bounds__(256) void tile_gemm_kernel(LA la, LB lb, int K, int ntm, Out out) {
  __shared__ __attribute__((aligned(16))) float As[TK * LDT];
  __shared__ __attribute__((aligned(16))) float Bs[TK * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, cl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int b = blockIdx.y;
  int tm, tn;
  if (SYM) {                                        // lower-triangle tile index -> (tm >= tn)
    int t = blockIdx.x;
    tm = 0;
    while (t > tm) t -= ++tm;
    tn = t;
  } else {
    tm = blockIdx.x % ntm;
    tn = blockIdx.x / ntm;
  }
  const int m0 = tm * TT, n0 = tn * TT;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int NL = TK * TT / 256;                 // elements per thread and operand per slab
  float ra[NL], rb[NL];
  const bool a_rc = la.r_contiguous(), b_rc = lb.r_contiguous();
  // slab element e -> (k, r): r fastest when the operand's rows are contiguous in memory, k fastest otherwise (coalesced loads)
  auto kr = [](bool rc, int e, int& k, int& r) {
    if (rc) { k = e >> 6; r = e & 63; } else { r = e >> 5; k = e & 31; }
  };
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      int k, r;
      kr(a_rc, tid + 256 * q, k, r);
      ra[q] = la(b, m0 + r, k0 + k);
      kr(b_rc, tid + 256 * q, k, r);
      rb[q] = lb(b, n0 + r, k0 + k);
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += TK) {
    __syncthreads();                                // the previous slab's MFMAs are done with As / Bs
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      int k, r;
      kr(a_rc, tid + 256 * q, k, r);
      As[k * LDT + r] = ra[q];
      kr(b_rc, tid + 256 * q, k, r);
      Bs[k * LDT + r] = rb[q];
    }
    __syncthreads();
    if (k0 + TK < K) fetch(k0 + TK);                // in flight under this slab's MFMAs
#pragma unroll
    for (int kg = 0; kg < TK / 4; ++kg) {
      const float* arow = As + (kg * 4 + kq) * LDT + wm * 32 + cl;
      const float* brow = Bs + (kg * 4 + kq) * LDT + wn * 32 + cl;
      const float a0 = arow[0], a1 = arow[16], b0 = brow[0], b1 = brow[16];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }

  // accumulator (i, j), register r = C(m0 + 32 wm + 16 i + 4 kq + r, n0 + 32 wn + 16 j + cl)
  float* cb = out.p + (long long)b * out.sb;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 32 + i * 16 + kq * 4 + r, n = n0 + wn * 32 + j * 16 + cl;
        if (m >= out.rows || n >= out.cols) continue;
        if (SYM) {
          if (m < n) continue;
          cb[(long long)n * out.sm + (long long)m * out.sn] = acc[i][j][r];
        }
        cb[(long long)m * out.sm + (long long)n * out.sn] = acc[i][j][r];
      }
}

template <bool SYM, typename LA, typename LB>
int launch_gemm(const LA& la, const LB& lb, int M, int N, int K, int B, const Out& out, hipStream_t s) {
  const int ntm = cmf_ceil_div(M, TT), ntn = cmf_ceil_div(N, TT);
  const int tiles = SYM ? ntm * (ntm + 1) / 2 : ntm * ntn;
  hipLaunchKernelGGL((tile_gemm_kernel<SYM, LA, LB>), dim3(tiles, B), dim3(256), 0, s, la, lb, K, ntm, out);
  CMF_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// blocked pivot-only LDL^T on global memory, one workgroup per sample
// ------------------------------------------------------------------------------------------------
constexpr int PW = 32;         // panel width
constexpr int LDP = PW + 1;

enum { LDL_GRAM = 0, LDL_RETRY = 1, LDL_FACTOR = 2 };

size_t ldl_lds_bytes(int d) { return ((size_t)2 * d * LDP + d) * sizeof(float); }

// LDL_GRAM   jtj as cmf_gram_cholesky left it: l1 terms, factorisation, jtj restored, attempt 0 reported.
// LDL_RETRY  unless fail[attempt - 1] is clear: jtj diagonal += eps (in place), l1_diag, factorisation, jtj restored, reported.
// LDL_FACTOR mat = a copy of src (the workspace of the backward pass): factorised, left as  lower: c_ik = l_ik p_k, diagonal: p_k,
//            upper: the mirror of the lower triangle (row i holds c_ki, k > i: the back substitution reads rows).
template <int MODE>
__global__ __launch_bounds__(256) void ldl_kernel(float* __restrict__ mat, const float* __restrict__ src, int d, int attempt,
                                                  float eps, float* __restrict__ logdet, float* __restrict__ l1_off,
                                                  float* __restrict__ l1_diag, int* __restrict__ info, int* __restrict__ fail) {
  if (MODE == LDL_RETRY && fail[attempt - 1] == 0) return;      // the previous attempt succeeded for the whole batch
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* P = smem;                 // [d][LDP] panel: rows k0.., columns k0..k0+31
  float* L = P + d * LDP;          // [d][LDP] row factors P_ik / p_k of the panel
  float* dsave = L + d * LDP;      // [d] the diagonal jtj must get back
  __shared__ float red[16];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15, b = blockIdx.x;
  const long long dd = (long long)d * d;
  float* A = mat + b * dd;

  if (MODE == LDL_GRAM) {
    float so = 0.f, sd = 0.f;
    for (int idx = tid; idx < d * d; idx += 256) {
      const int i = idx / d, j = idx - i * d;
      const float v = A[idx];
      if (i == j) { sd += fabsf(v); dsave[i] = v; } else so += fabsf(v);
    }
    so = block_sum(so, red);
    sd = block_sum(sd, red);
    if (tid == 0) { l1_off[b] = so; l1_diag[b] = sd; }
  } else if (MODE == LDL_RETRY) {
    float sd = 0.f;
    for (int i = tid; i < d; i += 256) {
      const float v = A[(long long)i * d + i] + eps;              // jitter EVERY sample (non_square.py:286)
      A[(long long)i * d + i] = v;
      dsave[i] = v;
      sd += fabsf(v);
    }
    sd = block_sum(sd, red);
    if (tid == 0) l1_diag[b] = sd;
  } else {
    const float* S = src + b * dd;
    for (int idx = tid; idx < d * d; idx += 256) A[idx] = S[idx];
  }
  __syncthreads();

  float ld = 0.f;
  int inf = 0;
  for (int k0 = 0; k0 < d; k0 += PW) {
    const int w = min(PW, d - k0), nr = d - k0;
    for (int e = tid; e < nr * PW; e += 256) {
      const int r = e / PW, c = e - r * PW;
      P[r * LDP + c] = (c < w && c <= r) ? A[(long long)(k0 + r) * d + k0 + c] : 0.f;
    }
    __syncthreads();
    // the panel: G_ij -= (G_ik / p_k) G_jk for k <= j <= i inside its columns, one barrier per column
    for (int kk = 0; kk < w; ++kk) {
      const float piv = P[kk * LDP + kk];                        // uniform
      if (!(piv > 0.f) || !(piv < 3.0e38f)) {
        inf = k0 + kk + 1;
        break;
      }
      ld += logf(piv);
      for (int r = kk + 1 + tid; r < nr; r += 256) {
        const float l = P[r * LDP + kk] / piv;                   // IEEE division, as block_cholesky
        L[r * LDP + kk] = l;
        const int cmax = min(w - 1, r);
        for (int c = kk + 1; c <= cmax; ++c) P[r * LDP + c] -= l * P[c * LDP + kk];
      }
      __syncthreads();
    }
    if (inf) break;                                              // uniform
    if (MODE == LDL_FACTOR)
      for (int e = tid; e < nr * PW; e += 256) {
        const int r = e / PW, c = e - r * PW;
        if (c < w && c <= r) A[(long long)(k0 + r) * d + k0 + c] = P[r * LDP + c];
      }
    // trailing lower triangle: the panel's w terms in column order (the unblocked sweep's order)
    const int t0 = k0 + w, nt = d - t0;
    for (int i = ti; i < nt; i += 16) {
      const float* li = L + (w + i) * LDP;
      float* arow = A + (long long)(t0 + i) * d + t0;
      for (int j = tj; j <= i; j += 16) {
        const float* pj = P + (w + j) * LDP;
        float a = arow[j];
        for (int kk = 0; kk < w; ++kk) a -= li[kk] * pj[kk];
        arow[j] = a;
      }
    }
    __syncthreads();
  }
  __syncthreads();

  if (MODE == LDL_FACTOR) {
    for (int idx = tid; idx < d * d; idx += 256) {
      const int i = idx / d, j = idx - i * d;
      if (i > j) A[(long long)j * d + i] = A[idx];
    }
    return;
  }
  for (int idx = tid; idx < d * d; idx += 256) {                 // jtj back: lower from upper, the diagonal from LDS
    const int i = idx / d, j = idx - i * d;
    if (i > j) A[idx] = A[(long long)j * d + i];
    else if (i == j) A[idx] = dsave[i];
  }
  if (tid == 0) {
    info[b] = inf;
    logdet[b] = inf ? __builtin_nanf("") : ld;
    if (inf) atomicOr(fail + attempt, 1);
  }
}

// ------------------------------------------------------------------------------------------------
// M = 2 (g_logdet G^-1 + g_l1off sign(G)[i != j] + g_l1diag sign(G)[i == j]) from the factor of ldl_kernel<LDL_FACTOR>
// ------------------------------------------------------------------------------------------------
// One 64-lane workgroup per 64 columns of G^-1 (grid (ceil(d / 64), B)); lane j solves G x = e_j with its column in LDS
// ([d][64]: 128 KiB at d = 512).  Factor reads are uniform across the lanes.  Forward: z_i = [i == j] - sum_{k<i} c_ik y_k,
// y_i = z_i / p_i (so that sum_k l_ik z_k = sum_k c_ik y_k); backward: x_i = y_i - (sum_{k>i} c_ki x_k) / p_i.  Rows below the
// workgroup's first column are zero in y and are skipped.
__global__ __launch_bounds__(64) void inverse_kernel(const float* __restrict__ F, const float* __restrict__ jtj, int d,
                                                     const float* __restrict__ g_logdet, const float* __restrict__ g_l1off,
                                                     const float* __restrict__ g_l1diag, float* __restrict__ M) {
  extern __shared__ __attribute__((aligned(16))) float Y[];     // [d][64]
  const int lane = threadIdx.x, b = blockIdx.y, j0 = blockIdx.x * 64, j = j0 + lane;
  const long long dd = (long long)d * d;
  const float* Fb = F + b * dd;
  for (int i = 0; i < j0; ++i) Y[i * 64 + lane] = 0.f;
  for (int i = j0; i < d; ++i) {
    const float* fi = Fb + (long long)i * d;
    float z0 = i == j ? 1.f : 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
    int k = j0;
    for (; k + 4 <= i; k += 4) {
      z0 -= fi[k] * Y[k * 64 + lane];
      z1 -= fi[k + 1] * Y[(k + 1) * 64 + lane];
      z2 -= fi[k + 2] * Y[(k + 2) * 64 + lane];
      z3 -= fi[k + 3] * Y[(k + 3) * 64 + lane];
    }
    for (; k < i; ++k) z0 -= fi[k] * Y[k * 64 + lane];
    Y[i * 64 + lane] = ((z0 + z1) + (z2 + z3)) / fi[i];
  }
  for (int i = d - 1; i >= 0; --i) {
    const float* ui = Fb + (long long)i * d;                    // upper triangle: ui[k] = c_ki for k > i
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = i + 1;
    for (; k + 4 <= d; k += 4) {
      s0 += ui[k] * Y[k * 64 + lane];
      s1 += ui[k + 1] * Y[(k + 1) * 64 + lane];
      s2 += ui[k + 2] * Y[(k + 2) * 64 + lane];
      s3 += ui[k + 3] * Y[(k + 3) * 64 + lane];
    }
    for (; k < d; ++k) s0 += ui[k] * Y[k * 64 + lane];
    Y[i * 64 + lane] -= ((s0 + s1) + (s2 + s3)) / ui[i];
  }
  if (j >= d) return;
  const float ga = g_logdet ? g_logdet[b] : 0.f, go = g_l1off ? g_l1off[b] : 0.f, gd = g_l1diag ? g_l1diag[b] : 0.f;
  const float* G = jtj + b * dd;
  float* Mb = M + b * dd;
  for (int i = 0; i < d; ++i) {
    const float g = G[(long long)i * d + j];
    const float sg = g > 0.f ? 1.f : g < 0.f ? -1.f : 0.f;
    Mb[(long long)i * d + j] = 2.f * (ga * Y[i * 64 + lane] + (i == j ? gd : go) * sg);
  }
}

// ------------------------------------------------------------------------------------------------
// Hutchinson + CG on the explicit Gram matrix, d <= 512
// ------------------------------------------------------------------------------------------------
// Why the explicit matrix still wins for d > 128 (hutch_cg.hip argues d <= 128): the exact-path Jacobian sweep over all d columns
// is already paid for by cmf_gram_cholesky, and a matrix-free CG step costs one JVP and one VJP sweep of S columns (rounded up
// to 16 column slots) through the whole network -- ~(16 + 16) / (2 + d) of the full sweep per step, so the default image setting
// (S = 1, ~11 steps) would spend 11 * 2 * 16 / 514 ~ 70 % of the sweep again at d = 512, and S = d with max_iter = d many sweeps.
// Against the explicit G a step is one d x d matrix-vector product per probe chunk: 1 MiB of G read from L2 per step.
//
// One 256-thread workgroup per (sample, chunk of NP <= 16 probes); grid (B, ceil(S / 16)).  Thread t owns rows t and t + 256 of
// every probe of the chunk in registers (x, r); the search directions live in LDS ([d][NP]) and G is read column-wise, G[j][k]
// for the thread's rows k (coalesced; G is symmetric, as cmf_gram_cholesky writes it).  NP is the smallest of 1, 4, 16 that
// holds the chunk, so S = 1 pays for one probe.  Stopping rule, normalisation and min_iter as hutch_cg_kernel: per work item
// (one sample's chunk), mean relative residual 2-norm < tol after at least min_iter iterations.
template <int NP>
__device__ __forceinline__ void block_sum_np(float (&v)[NP], float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < NP; ++s) v[s] = wave_sum(v[s]);
  if (lane == 0)
#pragma unroll
    for (int s = 0; s < NP; ++s) red[wave * NP + s] = v[s];
  __syncthreads();
#pragma unroll
  for (int s = 0; s < NP; ++s) v[s] = (red[s] + red[NP + s]) + (red[2 * NP + s] + red[3 * NP + s]);
  __syncthreads();
}

template <int NP>
__global__ __launch_bounds__(256) void hutch_wide_kernel(const float* __restrict__ jtj, const float* __restrict__ eps, int d, int S,
                                                         int max_iter, int min_iter, float tol, float* __restrict__ u_out,
                                                         float* __restrict__ w_out, float* __restrict__ val,
                                                         int* __restrict__ iters) {
  extern __shared__ __attribute__((aligned(16))) float Ps[];    // [d][NP] search directions (first: the raw probes)
  __shared__ float red[4 * NP];
  const int tid = threadIdx.x, b = blockIdx.x, s_lo = blockIdx.y * 16, Sc = min(16, S - s_lo);
  const bool chunked = gridDim.y > 1;
  const long long dd = (long long)d * d;
  const float* G = jtj + b * dd;
  const int k0 = tid, k1 = tid + 256;
  const bool h0 = k0 < d, h1 = k1 < d;
  auto io = [&](int k, int s) { return ((long long)b * d + k) * S + s_lo + s; };

  for (int idx = tid; idx < d * NP; idx += 256) {
    const int k = idx / NP, s = idx - k * NP;
    Ps[idx] = s < Sc ? eps[io(k, s)] : 0.f;
  }
  __syncthreads();
  // q = G p for the thread's rows, p = Ps
  float q[2][NP];
  auto matvec = [&]() {
#pragma unroll
    for (int s = 0; s < NP; ++s) q[0][s] = q[1][s] = 0.f;
    for (int j = 0; j < d; ++j) {
      const float g0 = h0 ? G[(long long)j * d + k0] : 0.f, g1 = h1 ? G[(long long)j * d + k1] : 0.f;
#pragma unroll
      for (int s = 0; s < NP; ++s) {
        const float p = Ps[j * NP + s];
        q[0][s] += g0 * p;
        q[1][s] += g1 * p;
      }
    }
  };

  // w = G eps (un-normalised); CG set-up on the unit-normalised right-hand sides
  matvec();
  float nb[NP], rr[NP], x[2][NP], r[2][NP];
#pragma unroll
  for (int s = 0; s < NP; ++s) {
    const float e0 = h0 ? Ps[k0 * NP + s] : 0.f, e1 = h1 ? Ps[k1 * NP + s] : 0.f;
    nb[s] = e0 * e0 + e1 * e1;
    if (s < Sc) {
      if (h0) w_out[io(k0, s)] = q[0][s];
      if (h1) w_out[io(k1, s)] = q[1][s];
    }
  }
  block_sum_np<NP>(nb, red);
#pragma unroll
  for (int s = 0; s < NP; ++s) {
    nb[s] = sqrtf(nb[s]);
    const float inv = nb[s] > 0.f ? 1.f / nb[s] : 0.f;
    r[0][s] = h0 ? Ps[k0 * NP + s] * inv : 0.f;
    r[1][s] = h1 ? Ps[k1 * NP + s] * inv : 0.f;
    x[0][s] = x[1][s] = 0.f;
    rr[s] = nb[s] > 0.f ? 1.f : 0.f;
  }
  __syncthreads();                                               // every read of the raw probes is done
#pragma unroll
  for (int s = 0; s < NP; ++s) {
    if (h0) Ps[k0 * NP + s] = r[0][s];
    if (h1) Ps[k1 * NP + s] = r[1][s];
  }
  __syncthreads();

  int it;
  for (it = 1; it <= max_iter; ++it) {
    matvec();
    float pq[NP], p0[NP], p1[NP];
#pragma unroll
    for (int s = 0; s < NP; ++s) {
      p0[s] = h0 ? Ps[k0 * NP + s] : 0.f;
      p1[s] = h1 ? Ps[k1 * NP + s] : 0.f;
      pq[s] = p0[s] * q[0][s] + p1[s] * q[1][s];
    }
    block_sum_np<NP>(pq, red);                                   // its barriers also end every read of Ps
    float rn[NP];
#pragma unroll
    for (int s = 0; s < NP; ++s) {
      const float alpha = (pq[s] > 0.f && rr[s] > 0.f) ? rr[s] / pq[s] : 0.f;
      x[0][s] += alpha * p0[s];
      x[1][s] += alpha * p1[s];
      r[0][s] -= alpha * q[0][s];
      r[1][s] -= alpha * q[1][s];
      rn[s] = r[0][s] * r[0][s] + r[1][s] * r[1][s];
    }
    block_sum_np<NP>(rn, red);
    float m = 0.f;
#pragma unroll
    for (int s = 0; s < NP; ++s) {
      const float beta = rr[s] > 0.f ? rn[s] / rr[s] : 0.f;
      if (h0) Ps[k0 * NP + s] = r[0][s] + beta * p0[s];
      if (h1) Ps[k1 * NP + s] = r[1][s] + beta * p1[s];
      rr[s] = rn[s];
      if (s < Sc) m += sqrtf(rn[s]);
    }
    __syncthreads();
    if (it >= min_iter && m / (float)Sc < tol) break;           // uniform: every thread holds the same block sums
  }
  if (it > max_iter) it = max_iter;

  float acc = 0.f;
#pragma unroll
  for (int s = 0; s < NP; ++s) {
    if (s >= Sc) continue;
    if (h0) {
      const float uv = x[0][s] * nb[s];
      u_out[io(k0, s)] = uv;
      acc += uv * w_out[io(k0, s)];
    }
    if (h1) {
      const float uv = x[1][s] * nb[s];
      u_out[io(k1, s)] = uv;
      acc += uv * w_out[io(k1, s)];
    }
  }
  __shared__ float red1[16];
  acc = block_sum(acc, red1);
  if (tid == 0) {
    if (!chunked) {
      val[b] = acc / (float)S;
      iters[b] = it;
    } else {
      atomicMax(iters + b, it);
    }
  }
}

__global__ void zero_int_kernel(int* p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}

// val[b] = mean_s sum_k u w over the finished (B, d, S) arrays of a chunked launch (a fixed summation order)
__global__ __launch_bounds__(256) void value_kernel(const float* __restrict__ u, const float* __restrict__ w, int n, int S,
                                                    float* __restrict__ val) {
  __shared__ float red[16];
  const long long o = (long long)blockIdx.x * n;
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += u[o + i] * w[o + i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) val[blockIdx.x] = acc / (float)S;
}

template <int MODE>
int launch_ldl(float* mat, const float* src, int d, int B, int attempt, float eps, float* logdet, float* l1_off, float* l1_diag,
               int* info, int* fail, hipStream_t s) {
  const size_t lds = ldl_lds_bytes(d);
  auto k = ldl_kernel<MODE>;
  if (hipError_t e = cmf_set_dynamic_lds((const void*)k, (int)lds); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k, dim3(B), dim3(256), lds, s, mat, src, d, attempt, eps, logdet, l1_off, l1_diag, info, fail);
  CMF_LAUNCH_CHECK();
  return 0;
}

template <int NP>
int launch_hutch(const float* jtj, const float* eps, int d, int S, int B, int max_iter, int min_iter, float tol, float* u, float* w,
                 float* val, int* iters, hipStream_t s) {
  const size_t lds = (size_t)d * NP * sizeof(float);
  auto k = hutch_wide_kernel<NP>;
  if (hipError_t e = cmf_set_dynamic_lds((const void*)k, (int)lds); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k, dim3(B, cmf_ceil_div(S, 16)), dim3(256), lds, s, jtj, eps, d, S, max_iter, min_iter, tol, u, w, val, iters);
  CMF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// dispatch targets of the C entry points (arguments validated by the callers)
// ------------------------------------------------------------------------------------------------
int cmf_wide_gram_cholesky(const float* t, long long t_b, long long t_r, int n_rows, int d, int B, float* jtj, float* logdet,
                           float* l1_off, float* l1_diag, int* info, int* fail, hipStream_t s) {
  const Strided j{t, t_b, 1, t_r, d, n_rows, 0};                // J^T(i, r) = T(b, r, i)
  if (int e = launch_gemm<true>(j, j, d, d, n_rows, B, Out{jtj, (long long)d * d, d, 1, d, d}, s)) return e;
  return launch_ldl<LDL_GRAM>(jtj, nullptr, d, B, 0, 0.f, logdet, l1_off, l1_diag, info, fail, s);
}

int cmf_wide_cholesky_retry(float* jtj, int d, int B, int attempt, float eps, float* logdet, float* l1_diag, int* info, int* fail,
                            hipStream_t s) {
  return launch_ldl<LDL_RETRY>(jtj, nullptr, d, B, attempt, eps, logdet, nullptr, l1_diag, info, fail, s);
}

// dt(b, r, 0:nc) = t(b, r, 0:d) m'(b) with m' = m (sym = 0) or m + m^T (sym = 1), m [B][d][d]; columns d..nc-1 are zeros
static int wide_product(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B, const float* m, int sym,
                        float* dt, long long dt_b, long long dt_r, hipStream_t s) {
  const Strided a{t, t_b, t_r, 1, n_rows, d, 0};                // A(r, k) = T(b, r, k)
  const Strided bt{m, (long long)d * d, 1, d, d, d, sym};       // Bt(n, k) = m(k, n) (+ m(n, k))
  return launch_gemm<false>(a, bt, n_rows, nc, d, B, Out{dt, dt_b, dt_r, 1, n_rows, nc}, s);
}

int cmf_wide_gram_backward_matrix(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B, const float* m,
                                  float* dt, long long dt_b, long long dt_r, hipStream_t s) {
  return wide_product(t, t_b, t_r, n_rows, nc, d, B, m, 1, dt, dt_b, dt_r, s);
}

int cmf_wide_gram_backward(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B, const float* jtj,
                           const float* g_logdet, const float* g_l1off, const float* g_l1diag, float* dt, long long dt_b,
                           long long dt_r, float* ws, hipStream_t s) {
  float* F = ws;                                                 // factor of jtj
  float* M = ws + (long long)B * d * d;                          // 2 dG
  if (int e = launch_ldl<LDL_FACTOR>(F, jtj, d, B, 0, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, s)) return e;
  const size_t lds = (size_t)d * 64 * sizeof(float);
  if (hipError_t e = cmf_set_dynamic_lds((const void*)inverse_kernel, (int)lds); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(inverse_kernel, dim3(cmf_ceil_div(d, 64), B), dim3(64), lds, s, F, jtj, d, g_logdet, g_l1off, g_l1diag, M);
  CMF_LAUNCH_CHECK();
  return wide_product(t, t_b, t_r, n_rows, nc, d, B, M, 0, dt, dt_b, dt_r, s);
}

int cmf_wide_hutch_cg(const float* jtj, const float* eps, int d, int S, int B, int max_iter, int min_iter, float tol, float* u,
                      float* w, float* val, int* iters, hipStream_t s) {
  const int chunks = cmf_ceil_div(S, 16);
  if (chunks > 1) {
    hipLaunchKernelGGL(zero_int_kernel, dim3(cmf_ceil_div(B, 256)), dim3(256), 0, s, iters, B);
    CMF_LAUNCH_CHECK();
  }
  int e;
  if (S == 1) e = launch_hutch<1>(jtj, eps, d, S, B, max_iter, min_iter, tol, u, w, val, iters, s);
  else if (S <= 4) e = launch_hutch<4>(jtj, eps, d, S, B, max_iter, min_iter, tol, u, w, val, iters, s);
  else e = launch_hutch<16>(jtj, eps, d, S, B, max_iter, min_iter, tol, u, w, val, iters, s);
  if (e) return e;
  if (chunks > 1) {
    hipLaunchKernelGGL(value_kernel, dim3(B), dim3(256), 0, s, u, w, d * S, S, val);
    CMF_LAUNCH_CHECK();
  }
  return 0;
}

int cmf_wide_hutch_cotangent(const float* u, const float* eps, const float* w, int d, int S, int B, const float* g_val,
                             const float* g_off, const float* g_diag, float* M, hipStream_t s) {
  const HutchLeft a{u, w, g_val, g_off, g_diag, d, S};
  const Strided e{eps, (long long)d * S, S, 1, d, S, 0};        // Bt(j, s) = eps(b, j, s)
  return launch_gemm<false>(a, e, d, d, S, B, Out{M, (long long)d * d, d, 1, d, d}, s);
}
