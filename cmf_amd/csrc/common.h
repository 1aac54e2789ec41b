// Shared helpers for the gfx950 kernels of libcmf_amd.so.
#pragma once
#include <hip/hip_runtime.h>
#include "cmf_amd.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CMF_LAUNCH_CHECK()                         \
  do {                                             \
    hipError_t e_ = hipGetLastError();             \
    if (e_ != hipSuccess) return (int)e_;          \
  } while (0)

// runtime.hip: per-(device, kernel) memo of the dynamic-LDS attribute and the per-device CU count (keyed by the calling
// thread's current device; see the file header for why a process-wide flag is wrong)
hipError_t cmf_set_dynamic_lds(const void* fn, int bytes);
int cmf_device_cus();

static inline int cmf_ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// A launch gets 48 KiB of dynamic LDS without asking: above that, kernel k's attribute is raised first.  0, or the HIP error.
template <class Kern>
static inline int raise_lds(Kern k, size_t lds) {
  if (lds <= 48 * 1024) return 0;
  return (int)cmf_set_dynamic_lds((const void*)k, (int)lds);
}

// What every kernel that streams a Jacobian stack asks of it: panels of nc floats per row, sample stride t_b and row stride t_r
// (floats) that hold a row and keep every row 16-byte aligned.  True when the stack must be refused (CMF_EINVAL).
static inline bool bad_panel(const float* t, long long t_b, long long t_r, int nc) {
  return t_b < nc || t_r < nc || (t_b | t_r) % 4 || (uintptr_t)t % 16;
}

// sum over the 64 lanes of a wavefront (every lane gets the total)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block-wide sum for blocks of up to 1024 threads; `red` is >= 16 floats of LDS; result in every thread
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < nw; ++i) t += red[i];
  return t;
}

// conv_head.hip: the folded head (last hidden conv + 1x1 output conv) behind cmf_conv_tangent_bf16x3; validates its own arguments
int cmf_conv_head(const cmf_conv_tangent_args& a, hipStream_t s);
// conv_block_head.hip: the folded block (last block's conv1 + conv2 + 1x1 conv), cmf_conv_head's dispatch target when a.block_w1 is set
int cmf_conv_block_head(const cmf_conv_tangent_args& a, hipStream_t s);

// head_wide.hip: the Jacobian head for 128 < nc <= 512 (d <= 512); dispatch targets of the C entry points, arguments validated there
int cmf_wide_gram_cholesky(const float* t, long long t_b, long long t_r, int n_rows, int d, int B, float* jtj, float* logdet,
                           float* l1_off, float* l1_diag, int* info, int* fail, hipStream_t s);
int cmf_wide_cholesky_retry(float* jtj, int d, int B, int attempt, float eps, float* logdet, float* l1_diag, int* info, int* fail,
                            hipStream_t s);
int cmf_wide_gram_backward(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B, const float* jtj,
                           const float* g_logdet, const float* g_l1off, const float* g_l1diag, float* dt, long long dt_b,
                           long long dt_r, float* ws, hipStream_t s);
int cmf_wide_gram_backward_matrix(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B, const float* m,
                                  float* dt, long long dt_b, long long dt_r, hipStream_t s);
int cmf_wide_hutch_cg(const float* jtj, const float* eps, int d, int S, int B, int max_iter, int min_iter, float tol, float* u,
                      float* w, float* val, int* iters, hipStream_t s);
int cmf_wide_hutch_cotangent(const float* u, const float* eps, const float* w, int d, int S, int B, const float* g_val,
                             const float* g_off, const float* g_diag, float* M, hipStream_t s);
