// Folded head of a ResNet coupler's tangent network (evaluation): the LAST hidden 3x3 conv (64 -> 64, with its residual) and the
// 1x1 output conv behind it (64 -> cout <= 8) as ONE pass that never forms the 64 hidden channels.  Both maps are linear in the
// tangent and the relu' between them depends on (sample, channel, pixel) but not on the Jacobian column, so per output pixel p
//
//   yt(b,o,p,:) = sum_c G(o,c) h(b,c,p,:) + sum_{ci,tap} E(o,ci,tap) [c1(b,ci,p+tap) > 0] u(b,ci,p+tap,:)
//   G(o,c)      = Wf[o][c] [a(b,c,p) > 0]                    (64 x cout,  from the float activation a)
//   E(o,ci,tap) = sum_c G(o,c) W2[c][ci][tap]                (576 x cout, a 64-term dot each, built once per pixel in LDS)
//
// 2 cout 640 fp32 FMAs per pixel and column instead of 2 64 576 x 3 MFMA products: the pass is a memory stream over u (live rows
// only), h (the rows with a > 0 at the output pixels) and the small yt.
//
// Work item = (sample, P consecutive OUTPUT pixels), P cout' = 16 (cout' = cout rounded up to 2 / 4 / 8), 192 threads:
//   A  relu' masks of the 9 taps of each pixel (0 outside the image), relu' of a by ballot, G -> LDS
//   B  E -> LDS: thread t of 192 owns the three (ci, tap) pairs t, t + 192, t + 384 of W2's own inner order, streams W2[c][.] (L2
//      resident, coalesced) over c = 0..63 in order and feeds 3 x P cout' accumulators -- W2 is read once per item, not once per
//      pixel, and every G value read from LDS feeds three FMAs (one pair per thread made the CU's LDS pipe the limit at cout' = 4)
//   C  stream: a wave takes one (pixel, 16-column slice) at a time.  Lane l reads the float4 at channel l/4 (+ 16 per chunk), columns
//      4 (l%4) .. +3 of a [64][16] slice-major block -- 1 KiB per wave instruction -- predicated on the row's relu' bit, so a dead row
//      (which may hold anything, NaN included) is neither fetched nor multiplied.  E / G come from LDS (one 16-byte read per load).
//      Each lane sums its 4 h terms, then 36 (tap, chunk) terms in tap order; the 16 channel lanes are added by an xor tree.
// The order of every sum is fixed by (pixel, channel, tap) alone: it does not depend on the column's slot, nc, the batch, the grid,
// the pixel's place in its item or the compact / full form.  No atomics, no cross-column operation.
#include <stdint.h>

#include "common.h"

namespace {

constexpr int HID = 64, KJ = HID * 9, NT = 192, ACC = 16;
constexpr int SLICE = HID * 16;                               // floats of one [64][16] block

// full-image pixel of output pixel po (live != 0: compact index row * (W/2) + col/2 of the pixels with (row + col) % 2 == live - 1)
__device__ __forceinline__ int out_pixel(int po, int W, int live) {
  if (!live) return po;
  const int wh = W >> 1, row = po / wh, k = po - row * wh;
  return row * W + 2 * k + ((row + live - 1) & 1);
}

template <int CP>
__global__ __launch_bounds__(NT, CP == 8 ? 2 : 3) void conv_head_kernel(cmf_conv_tangent_args a, int n_out, int tiles_per_sample, int ntiles) {
  constexpr int P = ACC / CP;
  __shared__ __attribute__((aligned(16))) float Es[P * KJ * CP];       // [p][ci][tap][o]
  __shared__ __attribute__((aligned(16))) float Gs[HID * ACC];         // [c][p][o]
  __shared__ unsigned long long um[P * 9];                             // relu'(c1) of the 64 channels at (p, tap); 0 outside the image
  __shared__ unsigned long long alv[P];                                // relu'(a) of the 64 channels at p
  __shared__ int pixs[P];

  // blocks 8 apart run on one XCD: give each XCD a contiguous range of items, so the image rows a sample's neighbouring items
  // share meet in that XCD's L2 (placement changes speed only)
  const int per = (ntiles + 7) >> 3;
  const int item = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (item >= ntiles) return;
  const int b = item / tiles_per_sample, p0 = (item - b * tiles_per_sample) * P;
  const int cnt = n_out - p0 < P ? n_out - p0 : P;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int H = a.H, W = a.W, cout = a.head_cout;

  // ---- A
  if (tid < P * 9) {
    const int p = tid / 9, tap = tid - p * 9;
    unsigned long long m = 0;
    if (p < cnt) {
      const int pix = out_pixel(p0 + p, W, a.live);
      const int r = pix / W + tap / 3 - 1, c = pix % W + tap % 3 - 1;
      if (r >= 0 && r < H && c >= 0 && c < W)
        m = *reinterpret_cast<const unsigned long long*>(reinterpret_cast<const unsigned char*>(a.f) + (long long)b * a.f_np +
                                                         (long long)(r * W + c) * (HID / 8));
    }
    um[tid] = m;
  }
  for (int p = wv; p < P; p += NT / 64) {
    const int pix = p < cnt ? out_pixel(p0 + p, W, a.live) : 0;
    bool on = false;
    if (p < cnt) on = a.head_a[(long long)b * a.head_a_np + (long long)lane * a.head_a_c + (long long)pix * a.head_a_px] > 0.f;
    const unsigned long long bal = __ballot(on);
    if (lane == 0) {
      alv[p] = bal;
      pixs[p] = pix;
    }
#pragma unroll
    for (int o = 0; o < CP; ++o) Gs[(lane * P + p) * CP + o] = (on && o < cout) ? a.head_w[o * HID + lane] : 0.f;
  }
  __syncthreads();

  // ---- B  (every thread owns the three (ci, tap) pairs tid, tid + 192, tid + 384: a G value read from LDS feeds three FMAs)
  {
    static_assert(3 * NT == KJ, "three (ci, tap) pairs per thread");
    float acc[3][ACC];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int i = 0; i < ACC; ++i) acc[r][i] = 0.f;
#pragma unroll 2
    for (int c = 0; c < HID; ++c) {
      float w[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) w[r] = a.w[c * KJ + tid + r * NT];
#pragma unroll
      for (int i = 0; i < ACC / 4; ++i) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(&Gs[c * ACC + 4 * i]);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[r][4 * i + k] = fmaf(g[k], w[r], acc[r][4 * i + k]);
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int o = 0; o < CP; ++o) Es[(p * KJ + tid + r * NT) * CP + o] = acc[r][p * CP + o];
  }
  __syncthreads();

  // ---- C
  const int nsl = a.nc >> 4, cl = lane >> 2;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int unit = wv; unit < nsl * P; unit += NT / 64) {
    const int sl = unit / P, p = unit - sl * P;
    if (p >= cnt) continue;
    const int pix = pixs[p];
    const float* hb = a.r + (long long)b * a.r_np + (long long)pix * a.r_px + sl * SLICE + lane * 4;
    const float* ub = a.x + (long long)b * a.x_np + sl * SLICE + lane * 4;
    f32x4 acc[CP];
#pragma unroll
    for (int o = 0; o < CP; ++o) acc[o] = zero;

    // the four channel chunks of one [64][16] block, each lane's row fetched only where its relu' bit is set.  The load sits under
    // the bit's branch (exec mask): a global load is never speculated above its guard (it may fault), so a dead row costs no
    // request; the disassembly shows each global_load_dwordx4 behind its own s_cbranch_execz
    auto load4 = [&](f32x4* v, const float* src, unsigned long long m) {
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        v[ch] = zero;
        if ((m >> (ch * 16 + cl)) & 1) v[ch] = *reinterpret_cast<const f32x4*>(src + ch * 256);
      }
    };
    auto load_row = [&](f32x4* v, int ty) {
#pragma unroll
      for (int tx = 0; tx < 3; ++tx)                                     // pixel pix + (ty-1) W + (tx-1): inside the image wherever the mask is not 0
        load4(v + 4 * tx, ub + (long long)(pix + (ty - 1) * W + (tx - 1)) * a.x_px, um[p * 9 + ty * 3 + tx]);
    };
    auto fma4 = [&](const f32x4* v, const float* coef, int stride) {     // coef + ch * stride: the cout' weights of channel ch * 16 + cl
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        const float* e4 = static_cast<const float*>(__builtin_assume_aligned(coef + ch * stride, CP < 4 ? 8 : 16));
#pragma unroll
        for (int o = 0; o < CP; ++o) {
          const float e = e4[o];
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[o][k] = fmaf(e, v[ch][k], acc[o][k]);
        }
      }
    };
    auto fma_row = [&](const f32x4* v, int ty) {
#pragma unroll
      for (int tx = 0; tx < 3; ++tx) fma4(v + 4 * tx, &Es[(p * KJ + cl * 9 + ty * 3 + tx) * CP], 16 * 9 * CP);
    };
    // per lane: the 4 h terms, then the 36 (tap, chunk) terms in tap order; one tap row = 12 loads in flight (16 with h)
    {
      f32x4 vh[4], v[12];
      load4(vh, hb, alv[p]);
      load_row(v, 0);
      fma4(vh, &Gs[(cl * P + p) * CP], 16 * P * CP);
      fma_row(v, 0);
    }
#pragma unroll 1
    for (int ty = 1; ty < 3; ++ty) {
      f32x4 v[12];
      load_row(v, ty);
      fma_row(v, ty);
    }

    // sum over the 16 channel lanes l ^ {32, 16, 8, 4} of a column group, as an xor tree in that order.  Both lanes of a pair would
    // form the same sum (a + b = b + a), so each keeps half of the values and sends the other half: N/2 + N/4 + .. exchanges
    // instead of 4 N, the same bits.  The survivors of lane l: values (l/4) N/16 .. of the N = 4 cout' (o, column) sums.
    constexpr int N = 4 * CP;
    float val[N];
#pragma unroll
    for (int o = 0; o < CP; ++o)
#pragma unroll
      for (int k = 0; k < 4; ++k) val[4 * o + k] = acc[o][k];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int off = 32 >> s, n = N >> s;
      if (n >= 2) {
        const bool hi = lane & off;
#pragma unroll
        for (int i = 0; i < n / 2; ++i) {
          const float mine = hi ? val[n / 2 + i] : val[i], send = hi ? val[i] : val[n / 2 + i];
          val[i] = mine + __shfl_xor(send, off, 64);
        }
      } else {
        val[0] += __shfl_xor(val[0], off, 64);
      }
    }
    float* yb = a.head_y + (long long)b * a.head_y_np + (long long)(p0 + p) * a.head_y_px + sl * 16 + (lane & 3) * 4;
    constexpr int KEEP = N >= 16 ? N / 16 : 1;
#pragma unroll
    for (int i = 0; i < KEEP; ++i) {
      const int idx = ((cl * N) >> 4) + i, o = idx >> 2;
      if (o < cout && (N >= 16 || !(lane & 4))) yb[(long long)o * a.head_y_co + (idx & 3)] = val[i];
    }
  }
}

template <int CP>
int launch(const cmf_conv_tangent_args& a, hipStream_t s) {
  constexpr int P = ACC / CP;
  const int n_out = a.live ? a.H * a.W / 2 : a.H * a.W;
  const long long tiles = (n_out + P - 1) / P, ntiles = tiles * a.np;
  if (ntiles > 0x7ffffff0LL) return CMF_ERANGE;
  const int grid = 8 * (int)((ntiles + 7) / 8);
  hipLaunchKernelGGL(conv_head_kernel<CP>, dim3(grid), dim3(NT), 0, s, a, n_out, (int)tiles, (int)ntiles);
  CMF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// dispatch target of cmf_conv_tangent_bf16x3 (a.head_w != NULL); validates everything it relies on
int cmf_conv_head(const cmf_conv_tangent_args& a, hipStream_t s) {
  if (a.block_w1) return cmf_conv_block_head(a, s);             // folded block: conv1 of the last block taken in as well (conv_block_head.hip)
  if (!a.x || !a.w || !a.f || !a.r || !a.head_w || !a.head_a || !a.head_y) return CMF_EINVAL;
  if (a.fmode != CMF_F_RELU_BITS || a.taps != 9 || a.cin != HID || a.cout != HID) return CMF_EINVAL;
  if (a.head_cout < 1 || a.head_cout > 8 || a.np <= 0 || a.H <= 0 || a.W <= 0 || a.nc <= 0 || a.nc % 16) return CMF_EINVAL;
  if (a.bias || a.fo || a.ymask || a.mask_out || a.live < 0 || a.live > 2 || (a.live && a.W % 2)) return CMF_EINVAL;
  if (!((a.W % 14 == 0 && a.H % 2 == 0) || (a.W % 8 == 0 && a.H % 4 == 0))) return CMF_EINVAL;
  const long long HW = (long long)a.H * a.W;
  if (HW > (1 << 24)) return CMF_ERANGE;
  if (a.x_ci != 16 || a.x_sl != SLICE || a.r_co != 16 || a.r_sl != SLICE) return CMF_EINVAL;                 // slice-major blocks
  if ((a.x_np | a.x_px | a.r_np | a.r_px | a.head_y_np | a.head_y_co | a.head_y_px) % 4) return CMF_EINVAL;   // 16-byte accesses
  if (a.x_px < (long long)HID * a.nc || a.r_px < (long long)HID * a.nc || a.head_y_px < a.nc) return CMF_EINVAL;
  if ((uintptr_t)a.x % 16 || (uintptr_t)a.r % 16 || (uintptr_t)a.head_y % 16 || (uintptr_t)a.w % 4 || (uintptr_t)a.head_w % 4) return CMF_EINVAL;
  if ((uintptr_t)a.f % 8 || a.f_np % 8 || a.f_np < HW * (HID / 8)) return CMF_EINVAL;                         // one 8-byte word per pixel
  const int cp = a.head_cout <= 2 ? 2 : a.head_cout <= 4 ? 4 : 8;
  return cp == 2 ? launch<2>(a, s) : cp == 4 ? launch<4>(a, s) : launch<8>(a, s);
}
