// A linear measurement operator carried through one decode sweep, per sample.
//
// cmf_operator_apply takes what a decode sweep leaves on the device -- x_hat and the Jacobian stack t -- and a dense operator
// a [M][D] shared by the batch, and writes
//   K_b = a J_b   (M rows, the same nc columns: a Jacobian stack again, for cmf_gram_cholesky and cmf_gauss_newton_step)
//   yhat_b = a x_hat_b.
// Two kernels behind the one entry point:
//
//   operator_image_kernel   yhat.  One 256-thread workgroup per (sample, 64 rows of a); a wave owns rows w, w + 4, ... of the
//                           group, four of them at a time; its 64 lanes stride over the D elements with a float64 accumulator
//                           per row (the product of two floats is exact in float64), and the 64 partials of a row are folded
//                           by a fixed xor butterfly.  The image-only mode (t == NULL) is this launch alone, so both modes give
//                           the same bits.
//   operator_apply_kernel   K.  One 256-thread workgroup per (sample, 64-column slab of t, group of NRT <= 16 row tiles of a);
//                           wave w owns the slab's 16-column tile w and keeps NRT accumulators of v_mfma_f32_16x16x4_f32 (exact
//                           fp32 products, fp32 accumulation: the instruction of head_wide.hip's tile_gemm_kernel, with the same
//                           operand placement).  The reduction runs over the D rows of J in slabs of KD = 32 rows (64 with NRT
//                           <= 4): the slab of J (KD x 64, one 16-byte load per thread and 16 rows, along the column index in
//                           both layouts) and of a (16 NRT x KD, 4-byte loads -- a row of a is not 16-byte aligned in general)
//                           are staged in LDS, the next slab's loads are in flight in registers under this slab's MFMAs.  Rows
//                           >= M of a, elements >= D and columns >= nc are never read: their LDS slots are zeros.  NRT is a
//                           template parameter, 1 .. 16, so that the MFMA loop carries no test: the row tiles of a are dealt
//                           evenly to the fewest groups of <= 16 (M = 196: one group of 13; M = 784: 4 groups of 13).
//
// Column c of K is a function of column c of t alone (a lane's accumulator column is fed by that column's B operands only), so
// whatever the padding columns d .. nc - 1 hold -- NaN included -- stays in them.  The accumulation along D is one chain of fused
// multiply-adds in the order of D, four terms per MFMA, whatever the slab depth: a function of D alone.  All M fits one row group
// up to M = 256 (then J is read once per launch); beyond that every further group reads J again.  No atomics; nothing is shared
// between workgroups.
//
// cmf_operator_apply_wrapped is the same pair of kernels behind the fused pre-head wrapper v = [logit](wa x + wc) of the image
// configurations: a acts on the DATA-space value u(v) = (p - wc) / wa, p = sigmoid(v) or v.  The image kernel
// evaluates u in float64 from the fp32 x_hat in front of its product; a small launch writes the derivative s = du/dv (float64,
// rounded once) to scale [B][D], and the apply kernel multiplies each staged row of J by its scale value on the way into LDS -- one
// fp32 multiply per element, the MFMA chain and every zero fill as above.  With (wa, wc, logit) = (1, 0, 0) u is x_hat and s is
// 1.0f exactly, so both outputs are cmf_operator_apply's bits.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int CS = 64;            // columns of t per workgroup
constexpr int LDJ = CS + 16;      // LDS row stride of the J slab [k][c]: lanes kq * 80 + cl hit 64 distinct banks
constexpr int MAX_RT = 16;        // row tiles of a per workgroup
constexpr int IMG_ROWS = 64;      // rows of a per workgroup of the image kernel
constexpr int IMG_ILP = 4;        // rows a wave of the image kernel sums side by side
// reduction slab depth (rows of J): few row tiles leave the MFMAs of a slab short, so the slab is deeper and more of J is in flight
constexpr int slab_depth(int nrt) { return nrt <= 4 ? 64 : 32; }

// The fused pre-head wrapper v = [logit](wa x + wc), seen from the head's side in float64.  The sigmoid goes through e = exp(-|v|)
// <= 1: p = 1 / (1 + e) or e / (1 + e), and p (1 - p) = e / (1 + e)^2 -- no 1 - p next to p = 1, so both keep a relative error of
// a few 2^-53 over the whole range of v.
struct Wrapper {
  double wa, wc;
  int logit;
};

// the data-space value u = (p - wc) / wa
__device__ __forceinline__ double wrapper_data(double v, const Wrapper w) {
  if (w.logit) {
    const double e = exp(-fabs(v));
    v = (v >= 0.0 ? 1.0 : e) / (1.0 + e);
  }
  return (v - w.wc) / w.wa;
}

// its derivative s = du / dv = [p (1 - p)] / wa
__device__ __forceinline__ double wrapper_slope(double v, const Wrapper w) {
  if (!w.logit) return 1.0 / w.wa;
  const double e = exp(-fabs(v)), q = 1.0 + e;
  return e / (q * q) / w.wa;
}

__global__ __launch_bounds__(NT) void operator_scale_kernel(const float* __restrict__ xhat, long long n, const Wrapper w,
                                                            float* __restrict__ scale) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i < n) scale[i] = (float)wrapper_slope((double)xhat[i], w);
}

template <bool WRAPPED>
__global__ __launch_bounds__(NT) void operator_image_kernel(const float* __restrict__ a, int M, int D,
                                                            const float* __restrict__ xhat, float* __restrict__ yhat, int groups,
                                                            const Wrapper w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long b = blockIdx.x / groups;
  const int m0 = (int)(blockIdx.x % groups) * IMG_ROWS;
  const float* __restrict__ xb = xhat + b * D;
  const int m1 = min(M, m0 + IMG_ROWS);
  // four rows at a time, so that their loads overlap; every row's sum is its own chain, in the same order whatever its company
  for (int m = m0 + wave; m < m1; m += 4 * IMG_ILP) {
    double acc[IMG_ILP];
#pragma unroll
    for (int j = 0; j < IMG_ILP; ++j) acc[j] = 0.0;
    for (int i = lane; i < D; i += 64) {
      double xv = (double)xb[i];
      if constexpr (WRAPPED) xv = wrapper_data(xv, w);
#pragma unroll
      for (int j = 0; j < IMG_ILP; ++j)
        if (m + 4 * j < m1) acc[j] += (double)a[(long long)(m + 4 * j) * D + i] * xv;
    }
#pragma unroll
    for (int j = 0; j < IMG_ILP; ++j) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
      if (lane == 0 && m + 4 * j < m1) yhat[b * M + m + 4 * j] = (float)acc[j];
    }
  }
}

// SCALED: row i of sample b's J is multiplied by scale[b D + i] on its way into LDS.  The scaled kernel of 13 row tiles -- C3's
// row group (M = 196, 784) -- is asked to stay at two workgroups per CU like the plain one: left alone it takes 270 registers for
// the plain kernel's 252, one wave per SIMD; asked, it fits 213 without a spill.
template <int NRT, bool SCALED>
__global__ __launch_bounds__(NT, (SCALED && NRT == 13) ? 2 : 1) void operator_apply_kernel(
    const float* __restrict__ a, int M, int D, const float* __restrict__ t, long long t_b, long long t_r, int nc,
    const float* __restrict__ scale, float* __restrict__ k, long long k_b, long long k_r, int slabs, int groups) {
  constexpr int KD = slab_depth(NRT);
  constexpr int LDA = KD + 4;                       // LDS row stride of the a slab [m][k]: lanes cl * LDA + kq hit 64 distinct banks
  __shared__ __attribute__((aligned(16))) float As[NRT * 16 * LDA];
  __shared__ __attribute__((aligned(16))) float Js[KD * LDJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, cl = lane & 15;
  int w = blockIdx.x;
  const int slab = w % slabs;
  w /= slabs;
  const int m0 = (w % groups) * (NRT * 16);
  const long long b = w / groups;
  const int c0 = slab * CS;
  const float* __restrict__ tb = t + b * t_b;
  const float* __restrict__ sb = SCALED ? scale + b * D : nullptr;

  f32x4 acc[NRT];
#pragma unroll
  for (int r = 0; r < NRT; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int NA = NRT * 16 * KD / NT;            // elements of a per thread and slab: element e = (row e / KD, k e % KD)
  constexpr int NJ = KD / 16;                       // 16-byte loads of J per thread and slab
  float ra[NA];
  f32x4 rj[NJ];                                     // rows jr, jr + 16, ... of the slab, columns jc .. jc + 3
  float rs[SCALED ? NJ : 1];                        // and their scale values
  const int jr = tid >> 4, jc = c0 + 4 * (tid & 15);
  auto fetch = [&](int i0) {
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      const int e = tid + NT * q, m = m0 + e / KD, i = i0 + e % KD;
      ra[q] = (m < M && i < D) ? a[(long long)m * D + i] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      const int i = i0 + jr + 16 * q;
      rj[q] = (i < D && jc < nc) ? *(const f32x4*)(tb + (long long)i * t_r + jc) : f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (SCALED) rs[q] = i < D ? sb[i] : 0.f;
    }
  };
  const bool live = c0 + 16 * wave < nc;            // the wave's column tile exists (uniform per wave)
  fetch(0);
  for (int i0 = 0; i0 < D; i0 += KD) {
    __syncthreads();                                // the previous slab's MFMAs are done with As / Js
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      const int e = tid + NT * q;
      As[(e / KD) * LDA + e % KD] = ra[q];
    }
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      if constexpr (SCALED) rj[q] *= rs[q];         // here, not in fetch: the loads stay in flight under the previous slab's MFMAs
      *(f32x4*)(Js + (jr + 16 * q) * LDJ + 4 * (tid & 15)) = rj[q];
    }
    __syncthreads();
    if (i0 + KD < D) fetch(i0 + KD);                // in flight under this slab's MFMAs
    if (live) {
#pragma unroll
      for (int kg = 0; kg < KD / 4; ++kg) {
        const float bv = Js[(kg * 4 + kq) * LDJ + 16 * wave + cl];
#pragma unroll
        for (int r = 0; r < NRT; ++r) {             // rows past M are zeros in As: no test per MFMA
          const float av = As[(16 * r + cl) * LDA + kg * 4 + kq];
          acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[r], 0, 0, 0);
        }
      }
    }
  }
  if (!live) return;
  // accumulator r, register q = K(m0 + 16 r + 4 kq + q, c0 + 16 wave + cl)
  float* __restrict__ kb = k + b * k_b + c0 + 16 * wave + cl;
#pragma unroll
  for (int r = 0; r < NRT; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + 16 * r + 4 * kq + q;
      if (m < M) kb[(long long)m * k_r] = acc[r][q];
    }
}

template <int NRT, bool SCALED>
int launch_apply(const float* a, int M, int D, const float* t, long long t_b, long long t_r, int nc, int B, const float* scale,
                 float* k, long long k_b, long long k_r, hipStream_t s) {
  const int slabs = cmf_ceil_div(nc, CS), groups = cmf_ceil_div(M, NRT * 16);
  const long long grid = (long long)B * slabs * groups;     // < 2^31: checked by the entry point
  hipLaunchKernelGGL((operator_apply_kernel<NRT, SCALED>), dim3((unsigned)grid), dim3(NT), 0, s, a, M, D, t, t_b, t_r, nc, scale, k,
                     k_b, k_r, slabs, groups);
  CMF_LAUNCH_CHECK();
  return 0;
}

// the instantiation with nrt row tiles per workgroup, 1 <= nrt <= MAX_RT
template <bool SCALED, int NRT = 1>
int dispatch_apply(int nrt, const float* a, int M, int D, const float* t, long long t_b, long long t_r, int nc, int B,
                   const float* scale, float* k, long long k_b, long long k_r, hipStream_t s) {
  if constexpr (NRT < MAX_RT) {
    if (nrt > NRT) return dispatch_apply<SCALED, NRT + 1>(nrt, a, M, D, t, t_b, t_r, nc, B, scale, k, k_b, k_r, s);
  }
  return launch_apply<NRT, SCALED>(a, M, D, t, t_b, t_r, nc, B, scale, k, k_b, k_r, s);
}

// What both entry points refuse, and the launches behind them.  ``w`` == nullptr: the plain operator (scale is not looked at).
int operator_apply(const float* a, int M, int D, const float* t, long long t_b, long long t_r, int nc, int B, const float* xhat,
                   const Wrapper* w, float* scale, float* k, long long k_b, long long k_r, float* yhat, hipStream_t s) {
  if (!a || !xhat || !yhat || M < 1 || D < 1 || B < 1) return CMF_EINVAL;
  if ((uintptr_t)a % 4 || (uintptr_t)xhat % 4 || (uintptr_t)yhat % 4) return CMF_EINVAL;
  if (t) {
    if (!k || nc < 16 || nc % 16 || nc > 512) return CMF_EINVAL;
    if (bad_panel(t, t_b, t_r, nc) || bad_panel(k, k_b, k_r, nc)) return CMF_EINVAL;
    if (w && (!scale || (uintptr_t)scale % 4)) return CMF_EINVAL;
  }
  const int groups = cmf_ceil_div(M, IMG_ROWS);
  // the larger of the two grids: one workgroup per (sample, slab, 16 rows) at the least
  if ((long long)B * cmf_ceil_div(M, 16) * (t ? cmf_ceil_div(nc, CS) : 1) > 0x7fffffffLL) return CMF_ERANGE;
  const long long n = (long long)B * D;
  if (w && t && (n + NT - 1) / NT > 0x7fffffffLL) return CMF_ERANGE;
  const dim3 image_grid((unsigned)((long long)B * groups));
  if (w)
    hipLaunchKernelGGL(operator_image_kernel<true>, image_grid, dim3(NT), 0, s, a, M, D, xhat, yhat, groups, *w);
  else
    hipLaunchKernelGGL(operator_image_kernel<false>, image_grid, dim3(NT), 0, s, a, M, D, xhat, yhat, groups, Wrapper{1.0, 0.0, 0});
  CMF_LAUNCH_CHECK();
  if (!t) return 0;                                  // image only: the Jacobian arguments are not looked at
  if (w) {
    hipLaunchKernelGGL(operator_scale_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, xhat, n, *w, scale);
    CMF_LAUNCH_CHECK();
  }
  // the row tiles of a, dealt evenly to the fewest row groups that hold them (M = 784: 49 tiles as 4 groups of 13, not 16)
  const int tiles = cmf_ceil_div(M, 16), row_groups = cmf_ceil_div(tiles, MAX_RT), nrt = cmf_ceil_div(tiles, row_groups);
  if (w) return dispatch_apply<true>(nrt, a, M, D, t, t_b, t_r, nc, B, scale, k, k_b, k_r, s);
  return dispatch_apply<false>(nrt, a, M, D, t, t_b, t_r, nc, B, nullptr, k, k_b, k_r, s);
}

}  // namespace

extern "C" int cmf_operator_apply(const float* a, int M, int D, const float* t, long long t_b, long long t_r, int nc, int B,
                                  const float* xhat, float* k, long long k_b, long long k_r, float* yhat, void* stream) {
  return operator_apply(a, M, D, t, t_b, t_r, nc, B, xhat, nullptr, nullptr, k, k_b, k_r, yhat, (hipStream_t)stream);
}

extern "C" int cmf_operator_apply_wrapped(const float* a, int M, int D, const float* t, long long t_b, long long t_r, int nc, int B,
                                          const float* xhat, float wa, float wc, int logit, float* scale, float* k, long long k_b,
                                          long long k_r, float* yhat, void* stream) {
  // wa == 0 or not finite, wc not finite (a finite float less itself is 0; an infinity or a NaN gives NaN), logit no flag
  if (wa == 0.f || wa - wa != 0.f || wc - wc != 0.f || (logit != 0 && logit != 1)) return CMF_EINVAL;
  const Wrapper w{(double)wa, (double)wc, logit};
  return operator_apply(a, M, D, t, t_b, t_r, nc, B, xhat, &w, scale, k, k_b, k_r, yhat, (hipStream_t)stream);
}
