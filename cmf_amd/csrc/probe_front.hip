// Entry of a checkerboard ResNet coupler's tangent network (evaluation): the tangent u0 of block 0's first conv from PROBE
// RESPONSES instead of one 64 -> 64 conv over every Jacobian column.  conv0 (cin <= 2 -> 64) and block 0's conv1 (64 -> 64) with the
// relu' between them are one linear map from the network's input rows v to u0 whose support per output pixel p is the 5 x 5 window,
// and only the pass-through (mask != 0) pixels of it carry an input row:
//
//   u0(b,co,p,:) = sum_{q in win5(p), cls(c,q) >= 0}  K(b,co,p,q,c) v(b,c,q,:)
//   K(b,co,p,q,c) = sum_{ci,tap1,tap0: p+tap1+tap0 = q}  W1[co,ci,tap1] [a0(b,ci,p+tap1) > 0] mask(c,q) W0[ci,c,tap0]
//
// K depends on the sample (through relu') but not on the column.  The input rows are coloured with classes such that a 5 x 5 window
// holds every class at most once (engine.probe_plan: 13 classes per input channel); pushing ONE probe column per class -- the sum of
// the unit impulses at that class's pixels -- through conv0 and conv1 with the existing kernels gives R(b,p,cls,co) = K(b,co,p,q,c)
// for the one (c, q) of class cls in win5(p).  This kernel applies K to the real columns:
//
//   u0[b,p,sl,co,0:16] = sum over (dy,dx) in raster order of win5, q = p + (dy,dx) inside the image, c ascending, cls(c,q) >= 0 of
//                          R[b,p,cls/16,co,cls%16] T[b,c,q,16 sl : 16 sl + 16]                       (fp32 fmaf in exactly that order)
//
// <= 13 cin FMAs per output element instead of 2 x 576 x 64 split-precision products: the pass is a memory stream that writes u0
// (live rows only) and reads R (live rows only), one 8-byte mask word per pixel and a few cache-resident input rows.
//
// Work item = (sample, pixel), 256 threads:
//   A  wave 0 lists the window's terms (lane = window position x channel, compacted in order by ballot): class and row offset
//   B  the pixel's R block(s), [64][16] each, -> LDS as [class][channel]; a row whose store-filter bit is clear is not fetched
//   C  per pass of 64 columns: the terms' input rows -> LDS; wave w owns 16-column slice w of the pass, lane l the channels
//      l/4 + 16 i (i < 4) and columns 4 (l%4) .. +3: per term one 16-byte LDS read of 4 coefficients and one of 4 row values feed
//      16 FMAs.  Store i of a wave is one contiguous KiB of the [64][16] block (16-byte pieces, live rows only).
// A column's sum is a function of (sample, pixel, channel) and that column's input values alone: it does not depend on the column's
// slot, nc, the batch, the grid or the workgroup shape.  No atomics, no cross-workgroup communication.
#include <stdint.h>

#include "common.h"

namespace {

constexpr int HID = 64, NT = 256, SLICE = HID * 16;         // floats of one [64][16] block
constexpr int MAXT = 50;                                     // 25 window pixels x cin <= 2
constexpr int MAXCLS = 32;                                   // classes: two 16-column slices of R
constexpr int PASS = 64;                                     // columns per pass (one 16-column slice per wave)

__global__ __launch_bounds__(NT) void probe_apply_kernel(cmf_probe_apply_args a, int nitems) {
  __shared__ __attribute__((aligned(16))) float Rs[MAXCLS * HID];      // [class][l/4][i]: channel l/4 + 16 i
  __shared__ __attribute__((aligned(16))) float Ts[MAXT * PASS];       // [term][column of this pass]
  __shared__ int tcls[MAXT], toff[MAXT];
  __shared__ int nterm;

  // blocks 8 apart run on one XCD: give each XCD a contiguous range of items, so the input rows neighbouring pixels of a sample
  // share meet in that XCD's L2 (placement changes speed only)
  const int per = (nitems + 7) >> 3;
  const int item = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (item >= nitems) return;
  const int H = a.H, W = a.W, HW = H * W;
  const int b = item / HW, p = item - b * HW;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ncls = a.ns * 16;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  unsigned long long live = ~0ull;                             // store filter: bit co of the pixel's word
  if (a.ymask)
    live = *reinterpret_cast<const unsigned long long*>(reinterpret_cast<const unsigned char*>(a.ymask) + (long long)b * a.ymask_np +
                                                        (long long)p * (HID / 8));

  // ---- A
  if (wv == 0) {
    int cls = -1, off = 0;
    if (lane < 25 * a.cin) {
      const int w = lane / a.cin, c = lane - w * a.cin;
      const int r = p / W + w / 5 - 2, col = p % W + w % 5 - 2;
      if (r >= 0 && r < H && col >= 0 && col < W) {
        const int q = r * W + col, k = a.cls[c * HW + q];
        if (k >= 0 && k < ncls) {
          cls = k;
          off = (int)(c * a.t_c + q * a.t_px);                 // below 2^31: checked by the launcher
        }
      }
    }
    const unsigned long long bal = __ballot(cls >= 0);
    if (cls >= 0) {
      const int pos = __popcll(bal & ((1ull << lane) - 1ull));
      tcls[pos] = cls;
      toff[pos] = off;
    }
    if (lane == 0) nterm = __popcll(bal);
  }

  // ---- B  (thread t holds channel t/4, classes 4 (t%4) .. +3 of a block: the block is read as one contiguous 4 KiB)
  {
    const int co = tid >> 2, k4 = (tid & 3) * 4;
    const float* rb = a.r + (long long)b * a.r_np + (long long)p * a.r_px + tid * 4;
    for (int s = 0; s < a.ns; ++s) {
      f32x4 v = zero;
      if ((live >> co) & 1) v = *reinterpret_cast<const f32x4*>(rb + s * SLICE);
#pragma unroll
      for (int m = 0; m < 4; ++m) Rs[(s * 16 + k4 + m) * HID + (co & 15) * 4 + (co >> 4)] = v[m];
    }
  }
  __syncthreads();

  // ---- C
  const int n = nterm, nsl = a.nc >> 4, cg = lane >> 2, quad = lane & 3;
  const float* tb = a.t + (long long)b * a.t_np;
  for (int s0 = 0; s0 < nsl; s0 += PASS / 16) {
    const int w4 = (nsl - s0 < PASS / 16 ? nsl - s0 : PASS / 16) * 4;    // 16-byte pieces per row in this pass
    if (s0) __syncthreads();                                             // the previous pass's rows have been read
    for (int i = tid; i < n * w4; i += NT) {
      const int j = i / w4, x = i - j * w4;
      *reinterpret_cast<f32x4*>(&Ts[j * PASS + 4 * x]) = *reinterpret_cast<const f32x4*>(tb + toff[j] + s0 * 16 + 4 * x);
    }
    __syncthreads();
    const int sl = s0 + wv;
    if (sl >= nsl) continue;
    f32x4 acc[4] = {zero, zero, zero, zero};
    for (int j = 0; j < n; ++j) {
      const f32x4 c4 = *reinterpret_cast<const f32x4*>(&Rs[tcls[j] * HID + cg * 4]);
      const f32x4 t4 = *reinterpret_cast<const f32x4*>(&Ts[j * PASS + wv * 16 + quad * 4]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[i][k] = fmaf(c4[i], t4[k], acc[i][k]);
    }
    float* yb = a.y + (long long)b * a.y_np + (long long)p * a.y_px + sl * SLICE + quad * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = cg + 16 * i;
      if ((live >> co) & 1) *reinterpret_cast<f32x4*>(yb + co * 16) = acc[i];
    }
  }
}

bool fits_i32(long long v) { return v >= 0 && v <= 0x7fffffffLL; }

}  // namespace

extern "C" int cmf_probe_apply(const cmf_probe_apply_args* ap, void* stream) {
  if (!ap) return CMF_EINVAL;
  const cmf_probe_apply_args& a = *ap;
  if (!a.r || !a.t || !a.cls || !a.y) return CMF_EINVAL;
  if (a.np <= 0 || a.H <= 0 || a.W <= 0 || a.nc <= 0 || a.nc % 16) return CMF_EINVAL;
  if (a.cin < 1 || 25 * a.cin > MAXT || a.ns < 1 || a.ns * 16 > MAXCLS) return CMF_EINVAL;
  if ((a.r_np | a.r_px | a.t_np | a.t_c | a.t_px | a.y_np | a.y_px) % 4) return CMF_EINVAL;                      // 16-byte accesses
  if ((uintptr_t)a.r % 16 || (uintptr_t)a.t % 16 || (uintptr_t)a.y % 16) return CMF_EINVAL;
  if (a.r_np < 0 || a.t_np < 0 || a.y_np < 0 || a.t_c < 0) return CMF_EINVAL;
  if (a.r_px < (long long)a.ns * SLICE || a.y_px < (long long)HID * a.nc || a.t_px < a.nc) return CMF_EINVAL;
  const long long HW = (long long)a.H * a.W;
  if (a.ymask && ((uintptr_t)a.ymask % 8 || a.ymask_np % 8 || a.ymask_np < HW * (HID / 8))) return CMF_EINVAL;   // one 8-byte word per pixel
  if (HW > (1 << 24) || !fits_i32(a.cin * a.t_c + HW * a.t_px + a.nc)) return CMF_ERANGE;
  const long long nitems = HW * a.np;
  if (nitems > 0x7ffffff0LL) return CMF_ERANGE;
  const int grid = 8 * (int)((nitems + 7) / 8);
  hipLaunchKernelGGL(probe_apply_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, a, (int)nitems);
  CMF_LAUNCH_CHECK();
  return 0;
}
