// Robust scale, IRLS weights and robust cost of a residual, per sample: the piece of ManifoldProjector.robust that
// turns r = x - x_hat into what the weighted step kernel (weighted_step.hip) consumes.
//
// cmf_robust_weights works in float64 on r_i = (double)x_i - (double)xhat_i (exact) over the USED elements, those with prior_i > 0
// (prior NULL: all of them, prior 1); an element with prior_i == 0 is never read in x or xhat -- the weighted step kernel's contract.
//   s    = scale_in[b], or 1.4826 med with med the LOWER median of |r_i| over the m used elements (0-based rank (m - 1) / 2), exact;
//   u_i  = r_i / s;   Huber:  omega = |u| <= c ? 1 : c / |u|,      rho = |u| <= c ? u^2 / 2 : c |u| - c^2 / 2;
//                     Tukey:  t = max(0, 1 - (u / c)^2),  omega = t^2,  rho = (c^2 / 6) (1 - t^3);
//   w_i  = float(prior_i omega_i), exactly 0.0f where prior_i == 0;   stats = { s, 2 s^2 sum prior_i rho_i, m, sum omega_i }.
// One 256-thread workgroup per sample; thread i looks at elements i, i + 256, ...; nothing is shared between workgroups.
//
//   1. Validate and count.  One pass over prior and the used x, x_hat: the "negative / non-finite" flags, and the histogram of the
//      TOP byte of the keys -- its total is m.  The key of an element is the 64-bit pattern of |r| (fabs clears the sign, so -0.0 is
//      +0.0): a float64 >= 0 orders like its pattern.
//   2. Select (scale_in == NULL).  Radix select of the key of rank (m - 1) / 2, most significant byte first: eight 8-bit passes
//      (the first is pass 1's histogram), each a 256-bin LDS histogram of the keys that match the bytes chosen so far -- integer
//      LDS atomics only, whose result does not depend on their order -- then a prefix sum over the 256 bins (one per thread:
//      wavefront shuffles, the four wave totals through LDS) picks the bin that holds the rank.  x and x_hat are read again from
//      L2 in every pass and nothing per element is kept in LDS, so n is not capped.
//   3. Weights.  One more pass: u, omega, rho; w out; the two sums as one partial per thread in element order, folded by the fixed
//      binary tree of dense_f64.h.  No floating-point atomics: a sample's outputs are a function of its own inputs and of n alone,
//      independent of B and of its position in the batch, and they repeat bit for bit.
//
// info: 0 ok; 2 a prior that is negative or not finite, or a non-finite x / x_hat at a used element (w and stats NaN); 3 s not
// finite or not > 0 -- no used element, a zero median, a bad scale_in -- (w and stats NaN, except stats[0] = s).  With m == 0 and
// scale_in == NULL the median of nothing is NaN.  NaN weights make the weighted step kernel report info 2.
#pragma clang fp contract(off)                    // one rounded operation per multiply and add: the formulas above, as written
#include "dense_f64.h"

namespace {

constexpr int NTH = 256;
static_assert(NTH == F64_NT, "dense_f64.h is written for this workgroup size");
constexpr double MAD_TO_SIGMA = 1.4826;           // 1 / Phi^-1(3/4), to the digits every textbook gives

__device__ __forceinline__ unsigned long long abs_key(float a, float h) {
  return (unsigned long long)__double_as_longlong(fabs((double)a - (double)h));
}

// The bin of hist[256] (one bin per thread) that holds rank k, and k's rank inside it; `total` = the sum of all bins.  With
// total == 0 no bin holds anything: bin and k come back as sel was left (the caller looks at total first).
__device__ __forceinline__ void pick_bin(const unsigned* hist, unsigned* wtot, unsigned* sel, unsigned& k, unsigned& bin,
                                         unsigned& total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned cnt = hist[tid];
  unsigned inc = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  unsigned before = 0;
  total = 0;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const unsigned c = wtot[v];
    before += v < wave ? c : 0u;
    total += c;
  }
  inc += before;
  if (k >= inc - cnt && k < inc) {                // one thread, when k < total
    sel[0] = (unsigned)tid;
    sel[1] = k - (inc - cnt);
  }
  __syncthreads();
  bin = sel[0];
  k = sel[1];
  __syncthreads();                                // hist, wtot and sel may be rewritten
}

__global__ __launch_bounds__(NTH) void robust_weights_kernel(int n, const float* __restrict__ x, const float* __restrict__ xhat,
                                                             const float* __restrict__ prior, int loss, double c,
                                                             const double* __restrict__ scale_in, float* __restrict__ w,
                                                             double* __restrict__ stats, int* __restrict__ info) {
  __shared__ double part[NTH];
  __shared__ unsigned hist[256];
  __shared__ unsigned wtot[4];
  __shared__ unsigned sel[2];
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* __restrict__ xb = x + (long long)b * n;
  const float* __restrict__ hb = xhat + (long long)b * n;
  const float* __restrict__ pb = prior ? prior + (long long)b * n : nullptr;
  float* __restrict__ wb = w ? w + (long long)b * n : nullptr;
  const double nan = __builtin_nan("");

  auto fail = [&](int code, double s) {             // uniform: NaN rows, stats NaN but for the scale slot
    if (wb)
      for (long long i = tid; i < n; i += NTH) wb[i] = __builtin_nanf("");
    if (tid < 4) stats[4LL * b + tid] = tid == 0 ? s : nan;
    if (tid == 0) info[b] = code;
  };

  // 1. validate, and the histogram of the top byte
  hist[tid] = 0u;
  if (tid < 2) sel[tid] = 0u;
  __syncthreads();
  int bad = 0;
  for (long long i = tid; i < n; i += NTH) {
    const float p = pb ? pb[i] : 1.f;
    bad |= !(p >= 0.f) | not_finite(p);
    if (p > 0.f) {
      const float a = xb[i], h = hb[i];
      bad |= not_finite(a) | not_finite(h);
      atomicAdd(&hist[abs_key(a, h) >> 56], 1u);
    }
  }
  if (__syncthreads_or(bad)) {                      // uniform; the barrier also completes hist
    fail(2, nan);
    return;
  }
  unsigned k = 0u, bin, m;
  pick_bin(hist, wtot, sel, k, bin, m);             // rank 0: only m is kept
  double s;
  if (scale_in) {
    s = scale_in[b];
  } else if (m == 0u) {
    s = nan;
  } else {
    // 2. the key of rank (m - 1) / 2, byte by byte
    k = (m - 1u) / 2u;
    unsigned total;
    pick_bin(hist, wtot, sel, k, bin, total);
    unsigned long long prefix = bin;
    for (int shift = 48; shift >= 0; shift -= 8) {
      hist[tid] = 0u;
      __syncthreads();
      for (long long i = tid; i < n; i += NTH) {
        const float p = pb ? pb[i] : 1.f;
        if (p > 0.f) {
          const unsigned long long key = abs_key(xb[i], hb[i]);
          if ((key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255ull], 1u);
        }
      }
      __syncthreads();
      pick_bin(hist, wtot, sel, k, bin, total);
      prefix = (prefix << 8) | bin;
    }
    s = MAD_TO_SIGMA * __longlong_as_double((long long)prefix);
  }
  if (!(s > 0.0) || not_finite(s)) {                // uniform
    fail(3, s);
    return;
  }

  // 3. weights, cost and the sum of omega
  const double c2_6 = c * c / 6.0, c2_2 = c * c / 2.0;
  double cost = 0.0, eff = 0.0;
  for (long long i = tid; i < n; i += NTH) {
    const float p = pb ? pb[i] : 1.f;
    float wv = 0.f;
    if (p > 0.f) {
      const double r = (double)xb[i] - (double)hb[i];
      const double u = r / s, au = fabs(u);
      double om, rho;
      if (loss == 0) {
        const bool in = au <= c;
        om = in ? 1.0 : c / au;
        rho = in ? u * u / 2.0 : c * au - c2_2;
      } else {
        const double q = u / c;
        double t = 1.0 - q * q;
        t = t > 0.0 ? t : 0.0;
        om = t * t;
        rho = c2_6 * (1.0 - t * t * t);
      }
      cost += (double)p * rho;
      eff += om;
      wv = (float)((double)p * om);
    }
    if (wb) wb[i] = wv;
  }
  cost = block_fold<false>(cost, part);
  eff = block_fold<false>(eff, part);
  if (tid == 0) {
    stats[4LL * b] = s;
    stats[4LL * b + 1] = 2.0 * s * s * cost;
    stats[4LL * b + 2] = (double)m;
    stats[4LL * b + 3] = eff;
    info[b] = 0;
  }
}

}  // namespace

extern "C" int cmf_robust_weights(const float* x, const float* xhat, const float* prior, int n, int B, int loss, double tuning,
                                  const double* scale_in, float* w, double* stats, int* info, void* stream) {
  if (!x || !xhat || !stats || !info || n < 1 || B < 1) return CMF_EINVAL;
  if ((loss != 0 && loss != 1) || !(tuning > 0.0)) return CMF_EINVAL;
  if ((uintptr_t)x % 4 || (uintptr_t)xhat % 4 || (uintptr_t)prior % 4 || (uintptr_t)w % 4 || (uintptr_t)info % 4) return CMF_EINVAL;
  if ((uintptr_t)stats % 8 || (uintptr_t)scale_in % 8) return CMF_EINVAL;
  hipLaunchKernelGGL(robust_weights_kernel, dim3(B), dim3(NTH), 0, (hipStream_t)stream, n, x, xhat, prior, loss, tuning, scale_in, w,
                     stats, info);
  CMF_LAUNCH_CHECK();
  return 0;
}
