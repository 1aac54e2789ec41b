// Hutchinson log-det surrogate with conjugate gradients on the explicit Gram matrix, for gfx950.
//
// Reference: NonSquareHeadDensity._approx_log_det_jac_and_reconstruction
// (cmf/models/components/densities/non_square.py:203-258):
//     u = linear_cg(v -> J^T J v, eps).detach();  w = J^T J eps;  value[b] = mean_s sum_k u[b,k,s] * w[b,k,s]
// with the matrix-vector product evaluated matrix-free (one jvp decode + one autograd vjp per product,
// :190-201) and gpytorch.utils.linear_cg @ fc2053b as the solver (un-vendored: PARITY UNPINNED for the CG
// iterates; J^T J eps itself is pinned by tests/golden).
//
// On MI355X the tangent kernels move Jacobian columns in granules of 16, so S = 1..4 probe columns cost as
// much as 16, and (n_cg + 1) matrix-free products of 2 sweeps each exceed ONE sweep over all d columns for
// every configuration on the path (d <= 128).  The native form therefore reuses the exact-path Jacobian:
// G = J^T J comes from cmf_gram_cholesky and this kernel runs CG against the explicit d x d matrix held in
// LDS, one workgroup per sample, one wavefront per probe column (all reductions are wavefront shuffles).
//
// Stopping rule.  gpytorch's linear_cg is public (cornellius-gp/gpytorch, gpytorch/utils/linear_cg.py): x0 = 0, every
// right-hand side normalised to unit 2-norm (solution rescaled at the end), plain CG updates, and after iteration k
// (0-based) it stops when  k >= min(10, max_iter - 1)  and  mean(||r_k||_2) < tolerance, the mean taken over EVERY
// (sample, probe) of the call.  Implemented here: the same normalisation, updates and minimum iteration count
// (min_iter = min(10, max_iter - 1) + 1 in 1-based counting), with the mean residual taken per WORK ITEM = one sample's
// probes (a chunk of at most 16 of them when S > 16) instead of over the whole batch -- a batch-wide mean would need a
// grid-wide barrier per iteration.  The reference's default tolerance is 1 and relative residuals start at 1, but the
// 2-norm residual of CG is not monotone: in the float64 model of this rule (tests/_hutch_cg_reference.py) the mean rises
// to 1.2 - 1.3 in the first iterations before it falls.  At condition number 1e2 (d = 64 .. 512) it is 0.17 - 0.19 at
// iteration 11 and the rule stops at the minimum count; at condition number 1e3 it is still 0.94 - 1.03 at iterations
// 11 - 14 and the stop comes at 12 - 14, where it is decided by rounding.  For d <= 11 the minimum count is
// max_iter = d iterations, i.e. the exact solve.  gpytorch's source is not vendored with the reference, so the iterates
// stay PARITY-UNPINNED against it; this rule itself is pinned per element by tests/test_gpu_hutch_cg.py.
//
// d > 128 or S > 128 dispatches to hutch_wide_kernel (head_wide.hip), whose header argues the explicit form for d up to 512.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void hutch_cg_kernel(const float* __restrict__ jtj, const float* __restrict__ eps,
                                                        int d, int S, int max_iter, int min_iter, float tol,
                                                        float* __restrict__ u_out, float* __restrict__ w_out,
                                                        float* __restrict__ val, int* __restrict__ iters) {
  // blockIdx.y = probe chunk: this workgroup owns probes [s_lo, s_lo + Sc) of the sample's S (one chunk when S <= 16)
  const int s_lo = blockIdx.y * 16, Sc = min(16, S - s_lo), chunked = gridDim.y > 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ldg = d + 1;
  float* G = smem;                       // [d][d+1]
  const int Sl = min(S, 16);             // probes per workgroup the LDS arrays are sized for
  float* X = G + d * ldg;                // [Sl][d]  solution (normalised rhs)
  float* R = X + Sl * d;                 // residual
  float* P = R + Sl * d;                 // search direction
  float* Q = P + Sl * d;                 // G p
  float* rn = Q + Sl * d;                // [Sl] current relative residual norms
  __shared__ int stop_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const float* gb = jtj + (long long)b * d * d;
  const float* eb = eps + (long long)b * d * S;
  for (int i = tid; i < d * d; i += 256) G[(i / d) * ldg + i % d] = gb[i];
  if (tid == 0) stop_flag = 0;
  __syncthreads();

  // w = G eps (un-normalised), and CG set-up; probes are dealt to wavefronts round-robin
  float bnorm[4];                        // S <= 16 -> at most 4 probes per wave
  float rr[4];
  int np = 0;
  for (int s = wave; s < Sc; s += 4, ++np) {
    const int sg = s_lo + s;             // probe index in the (B, d, S) arrays
    float nb = 0.f;
    for (int k = lane; k < d; k += 64) {
      const float e = eb[k * S + sg];
      nb += e * e;
    }
    nb = sqrtf(wave_sum(nb));
    bnorm[np] = nb;
    const float inv = nb > 0.f ? 1.f / nb : 0.f;
    for (int k = lane; k < d; k += 64) {
      float acc = 0.f;
      for (int j = 0; j < d; ++j) acc += G[k * ldg + j] * eb[j * S + sg];
      w_out[((long long)b * d + k) * S + sg] = acc;
      const float r0 = eb[k * S + sg] * inv;
      X[s * d + k] = 0.f;
      R[s * d + k] = r0;
      P[s * d + k] = r0;
    }
    rr[np] = nb > 0.f ? 1.f : 0.f;       // ||r0||^2 of the normalised system
    if (lane == 0) rn[s] = rr[np];
  }
  __syncthreads();

  int it = 0;
  for (it = 1; it <= max_iter; ++it) {
    int q = 0;
    for (int s = wave; s < Sc; s += 4, ++q) {
      float pq = 0.f;
      for (int k = lane; k < d; k += 64) {
        float acc = 0.f;
        for (int j = 0; j < d; ++j) acc += G[k * ldg + j] * P[s * d + j];
        Q[s * d + k] = acc;
        pq += acc * P[s * d + k];
      }
      pq = wave_sum(pq);
      const float alpha = (pq > 0.f && rr[q] > 0.f) ? rr[q] / pq : 0.f;
      float rr_new = 0.f;
      for (int k = lane; k < d; k += 64) {
        X[s * d + k] += alpha * P[s * d + k];
        const float r = R[s * d + k] - alpha * Q[s * d + k];
        R[s * d + k] = r;
        rr_new += r * r;
      }
      rr_new = wave_sum(rr_new);
      const float beta = rr[q] > 0.f ? rr_new / rr[q] : 0.f;
      for (int k = lane; k < d; k += 64) P[s * d + k] = R[s * d + k] + beta * P[s * d + k];
      rr[q] = rr_new;
      if (lane == 0) rn[s] = sqrtf(rr_new);
    }
    __syncthreads();
    if (tid == 0) {
      float m = 0.f;
      for (int s = 0; s < Sc; ++s) m += rn[s];
      stop_flag = (it >= min_iter && m / (float)Sc < tol) ? 1 : 0;
    }
    __syncthreads();
    if (stop_flag) break;
  }
  if (it > max_iter) it = max_iter;

  // u = x * ||b||; value = mean_s sum_k u * w
  float acc = 0.f;
  int q = 0;
  for (int s = wave; s < Sc; s += 4, ++q)
    for (int k = lane; k < d; k += 64) {
      const float u = X[s * d + k] * bnorm[q];
      const long long o = ((long long)b * d + k) * S + s_lo + s;
      u_out[o] = u;
      acc += u * w_out[o];
    }
  __shared__ float red[16];
  acc = block_sum(acc, red);
  if (tid == 0) {
    if (!chunked) {
      val[b] = acc / (float)S;
      iters[b] = it;
    } else {
      atomicMax(iters + b, it);          // integer: order-independent; the value is summed by hutch_value_kernel
    }
  }
}

__global__ void zero_int_kernel(int* p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}

// val[b] = mean_s sum_k u w over the finished (B, d, S) arrays (chunked launches: a fixed summation order instead of
// float atomics across the chunks' workgroups)
__global__ __launch_bounds__(256) void hutch_value_kernel(const float* __restrict__ u, const float* __restrict__ w, int n, int S,
                                                           float* __restrict__ val) {
  __shared__ float red[16];
  const long long o = (long long)blockIdx.x * n;
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += u[o + i] * w[o + i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) val[blockIdx.x] = acc / (float)S;
}

// Metric term on the Hutchinson product (non_square.py:87-100 applied to the third return value of :253-258, W = G eps of
// shape (B, d, S)): g_kk = diagonal(W) -> l1_diag = sum_k |W_kk|;  g_ij = W.masked_select(~eye(d)).view(B, d(d-1)) -> l1_off =
// sum_{i != j} |W_ij|.  The reference's view() of the off-diagonal entries only works for S == d (the launcher's precondition for
// l1_off); its diagonal branch (:87-92) takes torch.diagonal of the (B, d, S) product, valid for any S: min(d, S) entries.
__global__ __launch_bounds__(256) void hutch_metric_kernel(const float* __restrict__ w, int d, int S, float* __restrict__ l1_off,
                                                            float* __restrict__ l1_diag) {
  __shared__ float red[16];
  const long long o = (long long)blockIdx.x * d * S;
  float off = 0.f, dg = 0.f;
  for (int i = threadIdx.x; i < d * S; i += 256) {
    const float a = fabsf(w[o + i]);
    if (i / S == i % S) dg += a; else off += a;               // diagonal(W, dim1=-2, dim2=-1): min(d, S) entries
  }
  off = block_sum(off, red);
  dg = block_sum(dg, red);
  if (threadIdx.x == 0) {
    if (l1_off) l1_off[blockIdx.x] = off;
    if (l1_diag) l1_diag[blockIdx.x] = dg;
  }
}

// Cotangent of the Gram matrix for the train-mode objective on the Hutchinson product (u detached, non_square.py:236-247):
//   value_b = mean_s u_s^T (G eps_s)        -> d value / dG = (1/S) sum_s u_s eps_s^T
//   l1_off  = sum_{i != s} |(G eps)_{is}|    -> d / dG_ij    = sum_{s != i} sign(W_is) eps_js
//   l1_diag = sum_i |(G eps)_{ii}|           -> d / dG_ij    = sign(W_ii) eps_ji
//   M(b) = g_val[b] d value/dG + g_off[b] d l1_off/dG + g_diag[b] d l1_diag/dG      (any of the three may be NULL)
// One workgroup per sample; eps and the signs staged in LDS (d, S <= 128: 2 x 64 KB at most).
__global__ __launch_bounds__(256) void hutch_cotangent_kernel(const float* __restrict__ u, const float* __restrict__ eps,
                                                               const float* __restrict__ w, int d, int S,
                                                               const float* __restrict__ g_val, const float* __restrict__ g_off,
                                                               const float* __restrict__ g_diag, float* __restrict__ M) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* E = smem;                       // [d][S+1] eps
  float* A = E + d * (S + 1);            // [d][S+1] left factor: (gv/S) u + (g_off [i != s] + g_diag [i == s]) sign(w)
  const int b = blockIdx.x, tid = threadIdx.x, lds = S + 1;
  const long long o = (long long)b * d * S;
  const float gv = g_val ? g_val[b] / (float)S : 0.f, go = g_off ? g_off[b] : 0.f, gd = g_diag ? g_diag[b] : 0.f;
  for (int i = tid; i < d * S; i += 256) {
    const int r = i / S, c = i % S;
    E[r * lds + c] = eps[o + i];
    float a = gv * u[o + i];
    if (go != 0.f || gd != 0.f) {
      const float wv = w[o + i];
      const float sg = wv > 0.f ? 1.f : (wv < 0.f ? -1.f : 0.f);
      a += (r == c ? gd : go) * sg;
    }
    A[r * lds + c] = a;
  }
  __syncthreads();
  for (int idx = tid; idx < d * d; idx += 256) {
    const int i = idx / d, j = idx % d;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += A[i * lds + s] * E[j * lds + s];
    M[(long long)b * d * d + idx] = acc;
  }
}

// LOW-RANK form of the same cotangent (S << d).  With V = [u_1..u_S | eps_1..eps_S | e_0..e_{K-1}] (d x n, n = 2S + K) and
// P = J V (one n-column tangent sweep), the train-mode objective is a sum of inner products of COLUMNS of P:
//   value_b   = 1/S sum_s <P_s, P_{S+s}>                    (u detached: V is a constant)
//   l1_diag_b = sum_{k < K} |<P_{2S+k}, P_{S+k}>|,  K = min(d, S)      (W_kk = e_k^T J^T J eps_k)
// so d objective / d (P^T P) is the n x n matrix  C[s][S+s] = g_val/S,  C[2S+k][S+k] = g_diag sign(W_kk)  and the cotangent of P is
// P (C + C^T): cmf_gram_backward_matrix on the n-column stack.  One thread per matrix entry.
__global__ void hutch_lowrank_cotangent_kernel(const float* __restrict__ w, int d, int S, int n, const float* __restrict__ g_val,
                                               const float* __restrict__ g_diag, float* __restrict__ C, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % n), i = (int)((idx / n) % n);
  const long long b = idx / ((long long)n * n);
  float v = 0.f;
  if (i < S && j == S + i) v = g_val ? g_val[b] / (float)S : 0.f;
  if (g_diag && i >= 2 * S && j == S + (i - 2 * S)) {
    const int k = i - 2 * S;
    const float wkk = w[(b * d + k) * S + k];
    v = g_diag[b] * (wkk > 0.f ? 1.f : (wkk < 0.f ? -1.f : 0.f));
  }
  C[idx] = v;
}

}  // namespace

extern "C" int cmf_hutch_lowrank_cotangent(const float* w, int d, int S, int B, const float* g_val, const float* g_diag, int n,
                                           float* cmat, void* stream) {
  if (!cmat || d <= 0 || d > 512 || S <= 0 || S > 512 || B <= 0) return CMF_EINVAL;
  const int K = g_diag ? (d < S ? d : S) : 0;
  if (n != 2 * S + K || (g_diag && !w)) return CMF_EINVAL;
  const long long total = (long long)B * n * n;
  hipLaunchKernelGGL(hutch_lowrank_cotangent_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, d, S,
                     n, g_val, g_diag, cmat, total);
  CMF_LAUNCH_CHECK();
  return 0;
}

extern "C" int cmf_hutch_cg(const float* jtj, const float* eps, int d, int S, int B, int max_iter, int min_iter, float tol,
                            float* u, float* w, float* val, int* iters, void* stream) {
  if (!jtj || !eps || !u || !w || !val || !iters || d <= 0 || d > 512 || S <= 0 || S > 512 || B <= 0 || max_iter <= 0)
    return CMF_EINVAL;
  if (d > 128 || S > 128)
    return cmf_wide_hutch_cg(jtj, eps, d, S, B, max_iter, min_iter, tol, u, w, val, iters, (hipStream_t)stream);
  const int Sl = S < 16 ? S : 16, chunks = (S + 15) / 16;
  const size_t lds = (size_t)(d * (d + 1) + 4 * Sl * d + Sl) * sizeof(float);      // <= 66 + 32 KB
  hipStream_t s = (hipStream_t)stream;
  if (lds > 48 * 1024) {
    hipError_t e = cmf_set_dynamic_lds((const void*)hutch_cg_kernel, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  if (chunks > 1) {
    hipLaunchKernelGGL(zero_int_kernel, dim3(cmf_ceil_div(B, 256)), dim3(256), 0, s, iters, B);
    CMF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(hutch_cg_kernel, dim3(B, chunks), dim3(256), lds, s, jtj, eps, d, S, max_iter, min_iter, tol,
                     u, w, val, iters);
  CMF_LAUNCH_CHECK();
  if (chunks > 1) {
    hipLaunchKernelGGL(hutch_value_kernel, dim3(B), dim3(256), 0, s, u, w, d * S, S, val);
    CMF_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int cmf_hutch_metric(const float* w, int d, int S, int B, float* l1_off, float* l1_diag, void* stream) {
  if (!w || d <= 0 || d > 512 || S <= 0 || S > 512 || B <= 0 || (!l1_off && !l1_diag)) return CMF_EINVAL;
  if (l1_off && S != d) return CMF_EINVAL;                       // non_square.py:98: the off-diagonal view needs a square block
  hipLaunchKernelGGL(hutch_metric_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, w, d, S, l1_off, l1_diag);
  CMF_LAUNCH_CHECK();
  return 0;
}

extern "C" int cmf_hutch_cotangent(const float* u, const float* eps, const float* w, int d, int S, int B, const float* g_val,
                                   const float* g_off, const float* g_diag, float* M, void* stream) {
  if (!u || !eps || !M || d <= 0 || d > 512 || S <= 0 || S > 512 || B <= 0) return CMF_EINVAL;
  if ((g_off || g_diag) && !w) return CMF_EINVAL;
  if (g_off && S != d) return CMF_EINVAL;
  if (d > 128 || S > 128) return cmf_wide_hutch_cotangent(u, eps, w, d, S, B, g_val, g_off, g_diag, M, (hipStream_t)stream);
  const size_t lds = (size_t)2 * d * (S + 1) * sizeof(float);
  if (lds > 48 * 1024) {
    hipError_t e = cmf_set_dynamic_lds((const void*)hutch_cotangent_kernel, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(hutch_cotangent_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, u, eps, w, d, S, g_val, g_off,
                     g_diag, M);
  CMF_LAUNCH_CHECK();
  return 0;
}
