// One damped, WEIGHTED Gauss-Newton step per sample: the projection with missing or unevenly trusted elements.
//
// cmf_weighted_gauss_newton_step takes what one decode sweep leaves on the device -- x_hat and the Jacobian stack t (all d columns
// of J) --, the head-space input x and the non-negative weights w, and computes in ONE pass over the live rows of J
//   G_w = J^T diag(w) J   (float32, v_mfma_f32_16x16x4_f32 on LDS slabs: the A operand is float32(w_r J_ri), the B operand J_rj),
//   g_w = J^T (w o r),  r = x - x_hat   (float64, from the same slab),    cost = sum_i w_i r_i^2   (float64),
// then, in float64 on the float32 matrix it has just written,
//   A = G_w + lambda diag(G_w),   delta = A^-1 g_w,   stats = { cost, g^T delta, delta^T G_w delta, max_k |g_k| }.
// One 256-thread workgroup per sample; nothing is shared between workgroups, there are no atomics.
//
//   1. Scan.  The rows go by in chunks of CH = 1024: thread i looks at rows base + i, base + i + 256, ... .  A row with w == 0 is
//      dead: x, x_hat and row i of J are never loaded.  A live row adds fma(w r, r, .) to the thread's cost partial (the
//      residual-only launch is this phase alone, so both modes give the same bits) and is appended -- in row order, by wavefront
//      ballots and a prefix over the four waves -- to the live list in LDS with w and w r (float64).
//   2. Stream.  The live list is consumed in slabs of KC = 32 rows; what is left of a chunk (< KC rows) is carried into the next
//      chunk, so only the last slab of a sample is short.  A slab is loaded with one 16-byte load per thread and item (register
//      prefetch of the next slab under the work of the current one) and committed to LDS, missing rows as zeros.  Wave w
//      accumulates the row tiles w, 7 - w of the LOWER tile triangle, 36 of 64 tiles at d > 112 (only the 16-column tiles that
//      hold the first d columns are loaded, whatever nc is); the A operand is scaled
//      by w_r as it is read.  Thread (column c, row group rg) folds J_rc (w r)_r over the slab's rows in float64 and tests the
//      first d columns for non-finite values.  The summation order is a function of (n_rows, d) and of the positions of the
//      live rows alone.
//   3. The tiles are parked in LDS (over the slab: the float64 matrix below aliases all of it) and written out as gram, element
//      (i, j) with j > i from its mirror (j, i): symmetric bit for bit.
//   4. The lower triangle of gram is read back from global memory into the float64 matrix A in LDS (the step solves the equations
//      of the matrix it returns); the rest is damped_solve of dense_f64.h, which gn_step.hip ends in too: g is row d, the diagonal
//      is scaled by 1 + lambda, eliminate, back_substitute, and the two forms from the float32 lower triangle.
//
// info: 0 ok; 1 a pivot that is not positive and finite (delta, stats[1], stats[2] = NaN; gram, grad, stats[0], stats[3] valid):
// fewer live rows than d at lambda = 0, an all-zero weight row; 2 a weight that is negative or not finite, or a non-finite value
// in a live row of x, x_hat or the first d columns of t (every output NaN).
#include "dense_f64.h"                             // no fp-contract pragma in this file, as in gn_step.hip

namespace {

constexpr int NTH = 256;
static_assert(NTH == F64_NT, "dense_f64.h is written for this workgroup size");
constexpr int MAXD = 128;
constexpr int KC = 32;                            // live rows per LDS slab
constexpr int CH = 4 * NTH;                       // rows per scan chunk
constexpr int CAP = CH + KC;                      // live-list capacity: a chunk plus the carry (< KC)
constexpr int SMALL = NTH + MAXD;                 // doubles: the fold / g partials [NTH], delta [MAXD]; then the aliased region

inline __host__ __device__ constexpr int slab_stride(int NC) { return NC % 32 == 0 ? NC + 16 : NC; }
// byte offsets inside the aliased region while J streams: w r [CAP] doubles, row index [CAP] ints, w [CAP] floats, the slab
constexpr int OFF_LIST = CAP * 8, OFF_W = OFF_LIST + CAP * 4, OFF_SLAB = OFF_W + CAP * 4;
static_assert(OFF_SLAB % 16 == 0, "the slab takes 16-byte stores");

// One chunk of the scan: rows base + q NTH + tid, q = 0 .. 3.  Adds this thread's live rows to `acc`, ORs the non-finite / negative
// flags into `bad`; with LIST, appends the live rows in row order behind the `n` entries the list holds and returns the new count.
template <bool LIST>
__device__ __forceinline__ int scan_chunk(long long base, int n_rows, const float* __restrict__ wb, const float* __restrict__ xb,
                                          const float* __restrict__ hb, double& acc, int& bad, int n, int* wtot, int* list, float* wl,
                                          double* wrl) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float wq[4];
  double wr[4];
  int pre[4];
  bool live[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long long i = base + q * NTH + tid;
    float w = 0.f;
    if (i < n_rows) w = wb[i];
    bad |= !(w >= 0.f) | not_finite(w);
    live[q] = w > 0.f;
    wq[q] = w;
    wr[q] = 0.0;
    if (live[q]) {
      const float a = xb[i], h = hb[i];
      bad |= not_finite(a) | not_finite(h);
      const double r = (double)a - (double)h;
      wr[q] = (double)w * r;
      acc = __builtin_fma(wr[q], r, acc);
    }
    if (LIST) {
      const unsigned long long m = __ballot(live[q]);
      pre[q] = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) wtot[q * 4 + wave] = __popcll(m);
    }
  }
  if (!LIST) return 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int c = wtot[q * 4 + v];
      before += v < wave ? c : 0;
      total += c;
    }
    if (live[q]) {
      const int p = n + before + pre[q];          // < CAP: n < KC on entry, at most CH live rows in a chunk
      list[p] = (int)(base + q * NTH + tid);
      wl[p] = wq[q];
      wrl[p] = wr[q];
    }
    n += total;
  }
  __syncthreads();                                // publishes the list; wtot may be rewritten
  return n;
}

__global__ __launch_bounds__(NTH) void weighted_cost_kernel(int n_rows, const float* __restrict__ w, const float* __restrict__ x,
                                                            const float* __restrict__ xhat, double* __restrict__ stats,
                                                            int* __restrict__ info) {
  __shared__ double part[NTH];
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* __restrict__ wb = w + (long long)b * n_rows;
  const float* __restrict__ xb = x + (long long)b * n_rows;
  const float* __restrict__ hb = xhat + (long long)b * n_rows;
  int bad = 0;
  double acc = 0.0;
  for (long long base = 0; base < n_rows; base += CH)
    scan_chunk<false>(base, n_rows, wb, xb, hb, acc, bad, 0, nullptr, nullptr, nullptr, nullptr);
  const double c = block_fold<false>(acc, part);
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    stats[4LL * b] = bad ? __builtin_nan("") : c;
    info[b] = bad ? 2 : 0;
  }
}

template <int NT>
__global__ __launch_bounds__(NTH) void weighted_step_kernel(const float* __restrict__ t, long long t_b, long long t_r, int n_rows,
                                                            int d, const float* __restrict__ w, const float* __restrict__ x,
                                                            const float* __restrict__ xhat, const double* __restrict__ damping,
                                                            float* __restrict__ gram, double* __restrict__ grad,
                                                            double* __restrict__ delta, double* __restrict__ stats,
                                                            int* __restrict__ info) {
  constexpr int NC = NT * 16, LDJ = slab_stride(NC), LDG = NC + 1;
  constexpr int NI = (NT + 3) / 4;                 // row tiles per wave
  constexpr int ITEMS = KC * NC / 4;               // 16-byte items per slab
  constexpr int NIT = (ITEMS + NTH - 1) / NTH;
  constexpr int RG = NTH / NC;                     // row groups of the float64 gradient pass; threads >= RG NC sit it out
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int wtot[16];
  double* part = lds;                              // [NTH]
  double* dl = lds + NTH;                          // [MAXD]
  char* region = reinterpret_cast<char*>(lds + SMALL);
  double* wrl = reinterpret_cast<double*>(region);
  int* list = reinterpret_cast<int*>(region + OFF_LIST);
  float* wl = reinterpret_cast<float*>(region + OFF_W);
  float* Js = reinterpret_cast<float*>(region + OFF_SLAB);            // [KC][LDJ]
  float* Gp = reinterpret_cast<float*>(region);                       // [NC][LDG], once J has streamed
  double* A = lds + SMALL;                                            // [(d + 1) * LD], once gram is out

  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, cl = lane & 15;
  const float* __restrict__ tb = t + (long long)b * t_b;
  const float* __restrict__ wb = w + (long long)b * n_rows;
  const float* __restrict__ xb = x + (long long)b * n_rows;
  const float* __restrict__ hb = xhat + (long long)b * n_rows;
  const double nan = __builtin_nan("");

  f32x4 acc[NI][NT];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int gc = tid % NC, grg = tid / NC;         // this thread's column and row group of the gradient pass
  const bool gon = grg < RG && gc < d;
  double ga = 0.0, cost = 0.0;
  int bad = 0, n = 0;

  f32x4 pr[NIT];
  auto prefetch = [&](int s0, int cnt) {            // the slab of list entries s0 .. s0 + KC - 1, of which the first cnt exist
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + NTH * it;
      const int row = i / (NC / 4), c4 = i % (NC / 4);
      pr[it] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < ITEMS && row < cnt) pr[it] = *reinterpret_cast<const f32x4*>(tb + (long long)list[s0 + row] * t_r + c4 * 4);
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + NTH * it;
      if (i < ITEMS) *reinterpret_cast<f32x4*>(Js + (i / (NC / 4)) * LDJ + (i % (NC / 4)) * 4) = pr[it];
    }
  };

  for (long long base = 0; base < n_rows; base += CH) {
    n = scan_chunk<true>(base, n_rows, wb, xb, hb, cost, bad, n, wtot, list, wl, wrl);
    const bool last = base + CH >= n_rows;
    // full slabs; the last chunk also takes the short one
    auto rows_at = [&](int s0) { const int left = n - s0; return left >= KC ? KC : (last && left > 0 ? left : 0); };
    int s0 = 0, nl = rows_at(0);
    if (nl) prefetch(0, nl);
    while (nl) {
      commit();
      __syncthreads();
      const int nxt = rows_at(s0 + KC);
      if (nxt) prefetch(s0 + KC, nxt);
      // G_w: the lower tile triangle, 4 rows per MFMA
#pragma unroll
      for (int kg = 0; kg < KC / 4; ++kg) {
        if (kg * 4 < nl) {                          // uniform: the short slab's empty row groups
          const int rr = kg * 4 + kq;
          const float* row = Js + rr * LDJ + cl;
          const float wk = rr < nl ? wl[s0 + rr] : 0.f;
          float bv[NT];
#pragma unroll
          for (int j = 0; j < NT; ++j) bv[j] = row[j * 16];
#pragma unroll
          for (int i = 0; i < NI; ++i) {
            const int it = (i & 1) ? 4 * i + 3 - wave : 4 * i + wave;
            if (it < NT) {                          // wave-uniform
              const float av = row[it * 16] * wk;
#pragma unroll
              for (int j = 0; j < NT; ++j)
                if (j <= it) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j], acc[i][j], 0, 0, 0);
            }
          }
        }
      }
      // g_w in float64 from the same slab
      if (gon) {
        for (int r = grg; r < nl; r += RG) {
          const float v = Js[r * LDJ + gc];
          bad |= not_finite(v);
          ga = __builtin_fma((double)v, wrl[s0 + r], ga);
        }
      }
      __syncthreads();
      s0 += KC;
      nl = nxt;
    }
    // carry what is left (< KC entries) to the front of the list
    const int rem = n - s0;
    int ci = 0;
    float cw = 0.f;
    double cr = 0.0;
    if (tid < rem) {
      ci = list[s0 + tid];
      cw = wl[s0 + tid];
      cr = wrl[s0 + tid];
    }
    __syncthreads();
    if (tid < rem) {
      list[tid] = ci;
      wl[tid] = cw;
      wrl[tid] = cr;
    }
    n = rem > 0 ? rem : 0;                          // published by the next chunk's barrier; 0 after the last chunk
  }

  const int dd = d * d;
  float* G = gram + (long long)b * dd;              // written, then read back below: no __restrict__
  if (__syncthreads_or(bad)) {                      // uniform
    for (int e = tid; e < dd; e += NTH) G[e] = __builtin_nanf("");
    for (int k = tid; k < d; k += NTH) {
      grad[(long long)b * d + k] = nan;
      delta[(long long)b * d + k] = nan;
    }
    if (tid < 4) stats[4LL * b + tid] = nan;
    if (tid == 0) info[b] = 2;
    return;
  }

  // 3. park the tiles (the slab and the list are dead: every thread is past the last barrier of the loop), gram out
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int it = (i & 1) ? 4 * i + 3 - wave : 4 * i + wave;
    if (it < NT) {
#pragma unroll
      for (int j = 0; j < NT; ++j)
        if (j <= it) {
#pragma unroll
          for (int r = 0; r < 4; ++r) Gp[(it * 16 + kq * 4 + r) * LDG + j * 16 + cl] = acc[i][j][r];
        }
    }
  }
  if (grg < RG) part[grg * NC + gc] = ga;           // < NTH
  __syncthreads();
  for (int e = tid; e < dd; e += NTH) {
    const int i = e / d, j = e - i * d;
    G[e] = j <= i ? Gp[i * LDG + j] : Gp[j * LDG + i];
  }
  double gk = 0.0;                                  // thread k < d keeps g_k
  if (tid < d) {
    for (int q = 0; q < RG; ++q) gk += part[q * NC + tid];
    grad[(long long)b * d + tid] = gk;
  }
  __syncthreads();                                  // gram is visible to the workgroup; Gp and part are free
  const double c2 = block_fold<false>(cost, part);

  // 4. the float64 matrix from the float32 values just written, then the damped solve and the two forms (dense_f64.h)
  const int LD = row_stride(d);
  load_lower<false>(G, d, A, LD);
  __syncthreads();
  damped_solve(G, d, A, LD, gk, damping[b], c2, part, dl, delta + (long long)b * d, stats + 4LL * b, info + b);
}

template <int NT>
int launch_weighted(const float* t, long long t_b, long long t_r, int n_rows, int d, int B, const float* w, const float* x,
                    const float* xhat, const double* damping, float* gram, double* grad, double* delta, double* stats, int* info,
                    hipStream_t s) {
  constexpr int NC = NT * 16;
  size_t region = (size_t)OFF_SLAB + sizeof(float) * KC * slab_stride(NC);
  const size_t park = sizeof(float) * NC * (NC + 1), mat = sizeof(double) * (size_t)(d + 1) * row_stride(d);
  region = region > park ? region : park;
  region = region > mat ? region : mat;
  const size_t lds = sizeof(double) * SMALL + region;
  auto k = weighted_step_kernel<NT>;
  if (int e = raise_lds(k, lds)) return e;
  hipLaunchKernelGGL(k, dim3(B), dim3(NTH), lds, s, t, t_b, t_r, n_rows, d, w, x, xhat, damping, gram, grad, delta, stats, info);
  CMF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cmf_weighted_gauss_newton_step(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B,
                                              const float* w, const float* x, const float* xhat, const double* damping, float* gram,
                                              double* grad, double* delta, double* stats, int* info, void* stream) {
  if (!w || !x || !xhat || !stats || !info || n_rows <= 0 || B <= 0) return CMF_EINVAL;
  if ((uintptr_t)w % 4 || (uintptr_t)x % 4 || (uintptr_t)xhat % 4 || (uintptr_t)stats % 8 || (uintptr_t)info % 4) return CMF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (!t) {                                       // cost-only: the Jacobian arguments are not looked at
    hipLaunchKernelGGL(weighted_cost_kernel, dim3(B), dim3(NTH), 0, s, n_rows, w, x, xhat, stats, info);
    CMF_LAUNCH_CHECK();
    return 0;
  }
  if (!damping || !gram || !grad || !delta) return CMF_EINVAL;
  if (d < 1 || d > MAXD || nc % 16 || d > nc) return CMF_EINVAL;
  if (bad_panel(t, t_b, t_r, nc)) return CMF_EINVAL;
  if ((uintptr_t)gram % 4 || (uintptr_t)damping % 8 || (uintptr_t)grad % 8 || (uintptr_t)delta % 8) return CMF_EINVAL;
#define CMF_WEIGHTED_CASE(N) \
  case N: return launch_weighted<N>(t, t_b, t_r, n_rows, d, B, w, x, xhat, damping, gram, grad, delta, stats, info, s);
  switch ((d + 15) / 16) {                        // the 16-column tiles that hold the first d columns; the rest of nc is never loaded
    CMF_WEIGHTED_CASE(1) CMF_WEIGHTED_CASE(2) CMF_WEIGHTED_CASE(3) CMF_WEIGHTED_CASE(4)
    CMF_WEIGHTED_CASE(5) CMF_WEIGHTED_CASE(6) CMF_WEIGHTED_CASE(7) CMF_WEIGHTED_CASE(8)
  }
#undef CMF_WEIGHTED_CASE
  return CMF_EINVAL;
}
