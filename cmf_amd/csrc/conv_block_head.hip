// Folded LAST BLOCK of a ResNet coupler's tangent network (evaluation): the folded head of conv_head.hip taken one conv further.  The
// last residual block's conv1 (64 -> 64), its conv2 (64 -> 64, with the residual) and the 1x1 output conv (64 -> cout <= 8) as ONE pass
// over the block's input h that forms neither conv1's output u nor the block's output.  All three maps are linear in the tangent and
// the relu' masks between them depend on (sample, channel, pixel) but not on the Jacobian column, so per output pixel p
//
//   G(o,c)     = Wf[o][c] [a(c,p) > 0]
//   E(o,t2,ci) = sum_c G(o,c) W2[c][ci][t2]                                  (fp32, c ascending: conv_head.hip's E)
//   e(o,t2,ci) = E(o,t2,ci) [c1(ci, p+t2) > 0]                               (0 where p+t2 is outside the image)
//   K(o,d,c)   = sum_{t1 asc, t2 = d - t1} sum_ci e(o,t2,ci) W1[ci][c][t1]   (d: the 25 offsets of the 5 x 5 window of p)
//   yt(o,p,:)  = sum_{r in win5(p) inside the image, raster order} sum_c coef(o,r-p,c) h(c,r,:)
//   coef(o,d,c) = K(o,d,c) [ma(c,r) > 0]  (+ G(o,c) at d = 0);  row (c,r) is fetched where ma is set (at d = 0: or G != 0)
//
// K is a GEMM per pixel -- (t2, o) rows, K = 64 ci, N = (c, t1) -- and runs as split bf16 products hi*hi + hi*lo + lo*hi on
// v_mfma_f32_16x16x32_bf16 (pack_hi / pack_lo as in conv_tangent_bf16x3.hip): the 16 MFMA rows are the (pixel, o) pairs of a work item,
// an MFMA column is a channel c, and a (t2, t1) pair accumulates straight into the accumulator of its offset d = t2 + t1, so the 81
// tap pairs fold into the 25 offsets inside the MFMA accumulators.  The apply is fp32 FMAs like conv_head.hip's stream.
//
// Work item = (sample, tile of P output pixels), P cout' = 16, 512 threads, one workgroup per CU (the coefficients of an item fill
// 100 KiB of LDS).  The tile is P/2 image rows x 2 output columns (4 x 4 image pixels of a checkerboard at cout' = 2), so neighbouring
// windows share their rows of h: an item fetches each row of its halo once per 16-column slice.
//   A  relu' masks: c1 at the 9 taps of each pixel, ma over the tile's halo (0 outside the image), a by ballot; G -> LDS
//   B  E in fp32 (W2 streamed once per item), masked by c1, split into bf16 hi / lo, written as MFMA A fragments
//   C  K: wave w owns channel tile w % 4 and one half of the offsets; W1's B fragments come pre-split from cmf_pack_block_weight
//      and stream through; the wave's A fragments are read from LDS once and stay in registers
//   D  apply: a wave takes one 16-column slice of half the tile's pixels; lane l handles channels l/4 + 16 ch, columns 4 (l % 4) .. + 3,
//      walks the halo in raster order -- every load predicated on the row's bit, a dead row is neither fetched nor multiplied -- and
//      the 16 channel lanes are added by the xor tree of conv_head.hip.
// The order of every sum is fixed by (pixel, channel, tap / offset) alone: not by the column's slot, nc, the batch, the grid, the
// pixel's place in its tile or the compact / full form.  No atomics, no cross-workgroup communication.
#include <stdint.h>

#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int HID = 64, KJ = HID * 9, NT = 512, ROWS = 16, ND = 25, HALO = 8, XB = 4;
constexpr int SLICE = HID * 16;                               // floats of one [64][16] block
static_assert(2 * KJ > 2 * NT && 2 * KJ <= 3 * NT && (2 * KJ - 2 * NT) % 64 == 0, "phase B: two units per thread, a third for whole waves");
constexpr int W1_FRAGS = 9 * 4 * 2 * 2 * 64;                  // 16-byte fragments of the W1 pack: [t1][c tile][k half][hi / lo][lane]

__device__ __forceinline__ unsigned pack_hi(float a, float b, float& ra, float& rb) {
  // RNE to bf16, return the packed pair and the exact fp32 remainders
  bf16x2 h = __builtin_convertvector(f32x2{a, b}, bf16x2);
  const unsigned bits = __builtin_bit_cast(unsigned, h);
  ra = a - __builtin_bit_cast(float, bits << 16);
  rb = b - __builtin_bit_cast(float, bits & 0xffff0000u);
  return bits;
}
__device__ __forceinline__ unsigned pack_lo(float a, float b) {
  bf16x2 h = __builtin_convertvector(f32x2{a, b}, bf16x2);
  return __builtin_bit_cast(unsigned, h);
}

// W1 = conv1's weight [ci][c][3][3] -> B fragments of v_mfma_f32_16x16x32_bf16: fragment ((t1 4 + ct) 2 + ks) 2 + hl, lane l, element j =
// hi (hl = 0) or lo (hl = 1) half of W1[32 ks + 8 (l / 16) + j][16 ct + l % 16][t1]
__global__ void pack_block_weight_kernel(const float* __restrict__ w, u32x4* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= W1_FRAGS) return;
  const int l = idx & 63, hl = (idx >> 6) & 1, ks = (idx >> 7) & 1, ct = (idx >> 8) & 3, t1 = idx >> 10;
  const int c = 16 * ct + (l & 15), ci0 = 32 * ks + 8 * (l >> 4);
  unsigned r[4];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const float v0 = w[((ci0 + 2 * jj) * HID + c) * 9 + t1], v1 = w[((ci0 + 2 * jj + 1) * HID + c) * 9 + t1];
    float ra, rb;
    const unsigned h = pack_hi(v0, v1, ra, rb);
    r[jj] = hl ? pack_lo(ra, rb) : h;
  }
  out[idx] = u32x4{r[0], r[1], r[2], r[3]};
}

// geometry of a tile: slot p = 2 i + j is image row ty TR + i, output column 2 tx + j (compact column under live)
struct Tile {
  int row0, s0, xb, Ws, H, W, live;
  __device__ __forceinline__ bool slot(int p, int& row, int& col, int& po) const {
    const int s = s0 + (p & 1);
    row = row0 + (p >> 1);
    col = live ? 2 * s + ((row + live - 1) & 1) : s;
    po = row * Ws + s;
    return row < H && s < Ws;
  }
};

// the four B fragments (k half, hi / lo) of tap t1, channel tile ct
__device__ __forceinline__ void load_w1(u32x4 (&b)[2][2], const u32x4* __restrict__ wp, int ct, int lane, int t1) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int hl = 0; hl < 2; ++hl) b[ks][hl] = wp[(((t1 * 4 + ct) * 2 + ks) * 2 + hl) * 64 + lane];
}

// phase C of one wave: the offsets [D0, D0 + NDH) of channel tile ct.  Fully unrolled: d = t2 + t1 is a compile-time constant.  The
// wave reads its 36 A fragments from LDS ONCE and keeps them in registers (no re-read per t1); W1's B fragments stream through, one tap ahead.
template <int HALF, int CP>
__device__ __forceinline__ void build_half(const u32x4* __restrict__ wp, const u32x4* As, float* Ks, const float* Gs,
                                           const unsigned long long* ha, const int* ctr, int ct, int lane) {
  constexpr int D0 = HALF ? 12 : 0, NDH = HALF ? 13 : 12;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[NDH];
  u32x4 af[9][2][2], bw[2][2][2];                                 // A: [t2][k half][hi / lo];  B: [t1 parity][k half][hi / lo]
#pragma unroll
  for (int i = 0; i < NDH; ++i) acc[i] = zero;
  load_w1(bw[0], wp, ct, lane, 0);
#pragma unroll
  for (int t2 = 0; t2 < 9; ++t2)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int hl = 0; hl < 2; ++hl) af[t2][ks][hl] = As[((t2 * 2 + ks) * 2 + hl) * 64 + lane];
#pragma unroll
  for (int t1 = 0; t1 < 9; ++t1) {
    if (t1 < 8) load_w1(bw[(t1 + 1) & 1], wp, ct, lane, t1 + 1);
#pragma unroll
    for (int t2 = 0; t2 < 9; ++t2) {
      const int d = (t1 / 3 + t2 / 3) * 5 + t1 % 3 + t2 % 3;
      if (d >= D0 && d < D0 + NDH) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8 ah = __builtin_bit_cast(bf16x8, af[t2][ks][0]), al = __builtin_bit_cast(bf16x8, af[t2][ks][1]);
          const bf16x8 bh = __builtin_bit_cast(bf16x8, bw[t1 & 1][ks][0]), bl = __builtin_bit_cast(bf16x8, bw[t1 & 1][ks][1]);
          acc[d - D0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc[d - D0], 0, 0, 0);
          acc[d - D0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc[d - D0], 0, 0, 0);
          acc[d - D0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc[d - D0], 0, 0, 0);
        }
      }
    }
  }
  // accumulator element i of lane l: row 4 (l / 16) + i = (pixel, o), column c = 16 ct + l % 16
  const int c = 16 * ct + (lane & 15);
#pragma unroll
  for (int dl = 0; dl < NDH; ++dl) {
    const int d = D0 + dl;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * (lane >> 4) + i, p = row / CP, o = row % CP;
      // K only where ma is set at p + d: the apply also fetches rows with ma clear (the centre rows of the tile's OTHER output
      // pixels, for their residual path), and those must meet an exact zero here.  The centre adds the residual path's G.
      const int at = ctr[p];
      const bool on = at >= 0 && ((ha[at + (d / 5 - 2) * HALO + d % 5 - 2] >> c) & 1);
      float v = on ? acc[dl][i] : 0.f;
      if (d == 12) v = Gs[c * ROWS + row] + v;
      Ks[((p * ND + d) * HID + c) * CP + o] = v;
    }
  }
}

// phase B of one thread: units u = tid + NT r, r < R
template <int R, int CP>
__device__ __forceinline__ void phase_b(const float* __restrict__ w2, const float* Gs, const unsigned long long* um, u32x4* As, int tid) {
  int q[R], rh[R];
  float acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int u = tid + r * NT;
    rh[r] = u >= KJ, q[r] = u - rh[r] * KJ;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[r][i] = 0.f;
  }
#pragma unroll 8
  for (int c = 0; c < HID; ++c) {
    float w[R];
#pragma unroll
    for (int r = 0; r < R; ++r) w[r] = w2[c * KJ + q[r]];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(&Gs[c * ROWS + rh[r] * 8]), g1 = *reinterpret_cast<const f32x4*>(&Gs[c * ROWS + rh[r] * 8 + 4]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        acc[r][k] = fmaf(g0[k], w[r], acc[r][k]);
        acc[r][4 + k] = fmaf(g1[k], w[r], acc[r][4 + k]);
      }
    }
  }
  // A fragment of v_mfma_f32_16x16x32_bf16: lane 16 (k / 8) + row holds k = 8 (lane / 16) + j of its row, k = ci % 32
  unsigned short* A16 = reinterpret_cast<unsigned short*>(As);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int ci = q[r] / 9, tap = q[r] - ci * 9, ks = ci >> 5, kq = (ci >> 3) & 3, j = ci & 7;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = rh[r] * 8 + i, p = row / CP;
      const float e = ((um[p * 9 + tap] >> ci) & 1) ? acc[r][i] : 0.f;
      float ra, rb;
      const unsigned h = pack_hi(e, 0.f, ra, rb);
      const unsigned l = pack_lo(ra, 0.f);
      const int at = ((tap * 2 + ks) * 2 * 64 + kq * 16 + row) * 8 + j;
      A16[at] = (unsigned short)(h & 0xffffu);
      A16[at + 64 * 8] = (unsigned short)(l & 0xffffu);
    }
  }
}

template <int CP>
__global__ __launch_bounds__(NT, 2) void conv_block_head_kernel(cmf_conv_tangent_args a, int tiles_x, int tiles_per_sample, int ntiles) {
  constexpr int P = ROWS / CP, TR = P / 2 > 0 ? P / 2 : 1, PU = P / 2;
  static_assert(P >= 2, "two output columns per tile");
  __shared__ __attribute__((aligned(16))) float Ks[ROWS * ND * HID];      // [p][d][c][o]
  __shared__ __attribute__((aligned(16))) u32x4 As[9 * 2 * 2 * 64];       // A fragments of e: [t2][k half][hi / lo][lane]
  __shared__ __attribute__((aligned(16))) float Gs[HID * ROWS];           // [c][p][o]
  __shared__ unsigned long long um[P * 9];                                // relu'(c1) at (p, t2); 0 outside the image
  __shared__ unsigned long long ha[HALO * HALO];                          // relu'(a_in) over the tile's halo; 0 outside the image
  __shared__ unsigned long long hl[HALO * HALO];                          // the rows the apply fetches: ha, | relu'(a) at the output pixels
  __shared__ unsigned long long alv[P];
  __shared__ int ctr[P];                                                  // halo index of output pixel p (-1: no such pixel)

  const int per = (ntiles + 7) >> 3;
  const int item = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (item >= ntiles) return;
  const int b = item / tiles_per_sample, tl = item - b * tiles_per_sample, ty = tl / tiles_x, tx = tl - ty * tiles_x;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, W = a.W, cout = a.head_cout;
  Tile T;
  T.H = H, T.W = W, T.live = a.live, T.Ws = a.live ? W >> 1 : W, T.row0 = ty * TR, T.s0 = 2 * tx, T.xb = a.live ? 4 * tx : 2 * tx;
  const int y0 = T.row0 - 2, x0 = T.xb - 2;                               // the halo's corner

  // ---- A
  if (tid < P * 9) {
    const int p = tid / 9, tap = tid - p * 9;
    int row, col, po;
    unsigned long long m = 0;
    if (T.slot(p, row, col, po)) {
      const int r = row + tap / 3 - 1, c = col + tap % 3 - 1;
      if (r >= 0 && r < H && c >= 0 && c < W)
        m = *reinterpret_cast<const unsigned long long*>(reinterpret_cast<const unsigned char*>(a.block_m1) + (long long)b * a.block_m1_np +
                                                         (long long)(r * W + c) * (HID / 8));
    }
    um[tid] = m;
  } else if (tid >= 256 && tid < 256 + HALO * HALO) {
    const int q = tid - 256, r = y0 + (q >> 3), c = x0 + (q & 7);
    unsigned long long m = 0;
    if (r >= 0 && r < H && c >= 0 && c < W)
      m = *reinterpret_cast<const unsigned long long*>(reinterpret_cast<const unsigned char*>(a.f) + (long long)b * a.f_np +
                                                       (long long)(r * W + c) * (HID / 8));
    ha[q] = m;
    hl[q] = m;
  }
  for (int p = wv; p < P; p += NT / 64) {
    int row, col, po;
    const bool ok = T.slot(p, row, col, po);
    bool on = false;
    if (ok) on = a.head_a[(long long)b * a.head_a_np + (long long)lane * a.head_a_c + (long long)(row * W + col) * a.head_a_px] > 0.f;
    const unsigned long long bal = __ballot(on);
    if (lane == 0) {
      alv[p] = bal;
      ctr[p] = ok ? (row - y0) * HALO + (col - x0) : -1;
    }
#pragma unroll
    for (int o = 0; o < CP; ++o) Gs[(lane * P + p) * CP + o] = (on && o < cout) ? a.head_w[o * HID + lane] : 0.f;
  }
  __syncthreads();
  if (tid < P) {
    int row, col, po;
    if (T.slot(tid, row, col, po)) hl[ctr[tid]] |= alv[tid];
  }

  // ---- B  (unit u = (row half, (ci, tap) pair of W2's own inner order): 8 accumulators, W2[c][.] streamed over c in order; a thread
  //          runs its 2 or 3 units side by side so that as many loads of W2 are in flight)
  if (wv < (2 * KJ - 2 * NT) / 64)
    phase_b<3, CP>(a.w, Gs, um, As, tid);
  else
    phase_b<2, CP>(a.w, Gs, um, As, tid);
  __syncthreads();

  // ---- C
  {
    const u32x4* wp = reinterpret_cast<const u32x4*>(a.block_w1);
    if (wv < 4)
      build_half<0, CP>(wp, As, Ks, Gs, ha, ctr, wv & 3, lane);
    else
      build_half<1, CP>(wp, As, Ks, Gs, ha, ctr, wv & 3, lane);
  }
  __syncthreads();

  // ---- D
  const int nsl = a.nc >> 4, cl = lane >> 2;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int unit = wv; unit < nsl * 2; unit += NT / 64) {
    const int sl = unit >> 1, ph = unit & 1;
    // the half's pixels and the box of their windows, clipped to the image (all wave-uniform)
    int prow[PU], pcol[PU], ppo[PU];
    bool pok[PU];
    int ylo = H, yhi = -1, xlo = W, xhi = -1;
#pragma unroll
    for (int k = 0; k < PU; ++k) {
      pok[k] = T.slot(ph * PU + k, prow[k], pcol[k], ppo[k]);
      if (pok[k]) {
        ylo = min(ylo, prow[k] - 2), yhi = max(yhi, prow[k] + 2);
        xlo = min(xlo, pcol[k] - 2), xhi = max(xhi, pcol[k] + 2);
      }
    }
    if (yhi < 0) continue;
    ylo = max(ylo, 0), yhi = min(yhi, H - 1), xlo = max(xlo, 0), xhi = min(xhi, W - 1);
    const float* hb = a.x + (long long)b * a.x_np + sl * SLICE + lane * 4;
    f32x4 acc[PU][CP];
#pragma unroll
    for (int k = 0; k < PU; ++k)
#pragma unroll
      for (int o = 0; o < CP; ++o) acc[k][o] = zero;

    for (int y = ylo; y <= yhi; ++y) {
#pragma unroll 1
      for (int xs = xlo; xs <= xhi; xs += XB) {
        // XB halo pixels at a time: 4 XB loads in flight, each under its row's bit (exec mask): a dead row costs no request
        f32x4 v[XB][4];
#pragma unroll
        for (int xi = 0; xi < XB; ++xi) {
#pragma unroll
          for (int ch = 0; ch < 4; ++ch) v[xi][ch] = zero;
          const int x = xs + xi;
          if (x <= xhi) {
            const unsigned long long m = hl[(y - y0) * HALO + (x - x0)];
            const float* src = hb + (long long)(y * W + x) * a.x_px;
#pragma unroll
            for (int ch = 0; ch < 4; ++ch)
              if ((m >> (ch * 16 + cl)) & 1) v[xi][ch] = *reinterpret_cast<const f32x4*>(src + ch * 256);
          }
        }
#pragma unroll
        for (int xi = 0; xi < XB; ++xi) {
          const int x = xs + xi;
#pragma unroll
          for (int k = 0; k < PU; ++k) {
            const int dy = y - prow[k] + 2, dx = x - pcol[k] + 2;
            if (x <= xhi && pok[k] && dy >= 0 && dy < 5 && dx >= 0 && dx < 5) {
              const float* coef = &Ks[(((ph * PU + k) * ND + dy * 5 + dx) * HID + cl) * CP];
#pragma unroll
              for (int ch = 0; ch < 4; ++ch) {
                const float* e4 = static_cast<const float*>(__builtin_assume_aligned(coef + ch * 16 * CP, CP < 4 ? 8 : 16));
#pragma unroll
                for (int o = 0; o < CP; ++o) {
                  const float e = e4[o];
#pragma unroll
                  for (int q = 0; q < 4; ++q) acc[k][o][q] = fmaf(e, v[xi][ch][q], acc[k][o][q]);
                }
              }
            }
          }
        }
      }
    }

    // sum over the 16 channel lanes l ^ {32, 16, 8, 4} of a column group: conv_head.hip's xor tree (each lane of a pair keeps half of
    // the values and sends the other half; the same bits as the plain tree)
    constexpr int N = 4 * CP;
#pragma unroll
    for (int k = 0; k < PU; ++k) {
      float val[N];
#pragma unroll
      for (int o = 0; o < CP; ++o)
#pragma unroll
        for (int q = 0; q < 4; ++q) val[4 * o + q] = acc[k][o][q];
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
      if (pok[k]) {
        float* yb = a.head_y + (long long)b * a.head_y_np + (long long)ppo[k] * a.head_y_px + sl * 16 + (lane & 3) * 4;
        constexpr int KEEP = N >= 16 ? N / 16 : 1;
#pragma unroll
        for (int i = 0; i < KEEP; ++i) {
          const int idx = ((cl * N) >> 4) + i, o = idx >> 2;
          if (o < cout && (N >= 16 || !(lane & 4))) yb[(long long)o * a.head_y_co + (idx & 3)] = val[i];
        }
      }
    }
  }
}

template <int CP>
int launch(const cmf_conv_tangent_args& a, hipStream_t s) {
  constexpr int P = ROWS / CP, TR = P / 2;
  const int Ws = a.live ? a.W / 2 : a.W;
  const long long tiles_x = (Ws + 1) / 2, tiles = tiles_x * ((a.H + TR - 1) / TR), ntiles = tiles * a.np;
  if (ntiles > 0x7ffffff0LL) return CMF_ERANGE;
  const int grid = 8 * (int)((ntiles + 7) / 8);
  hipLaunchKernelGGL(conv_block_head_kernel<CP>, dim3(grid), dim3(NT), 0, s, a, (int)tiles_x, (int)tiles, (int)ntiles);
  CMF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cmf_pack_block_weight(const float* w, void* out, long long* out_bytes, void* stream) {
  if (!out) {
    if (!out_bytes) return CMF_EINVAL;
    *out_bytes = (long long)W1_FRAGS * 16;
    return 0;
  }
  if (!w || (uintptr_t)out % 16 || (uintptr_t)w % 4) return CMF_EINVAL;
  hipLaunchKernelGGL(pack_block_weight_kernel, dim3((W1_FRAGS + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, (u32x4*)out);
  CMF_LAUNCH_CHECK();
  return 0;
}

// dispatch target of cmf_conv_head (a.block_w1 != NULL); validates everything it relies on
int cmf_conv_block_head(const cmf_conv_tangent_args& a, hipStream_t s) {
  if (!a.x || !a.w || !a.f || !a.block_w1 || !a.block_m1 || !a.head_w || !a.head_a || !a.head_y) return CMF_EINVAL;
  if (a.r && a.r != a.x) return CMF_EINVAL;                                                                   // the residual IS x here
  if (a.fmode != CMF_F_RELU_BITS || a.taps != 9 || a.cin != HID || a.cout != HID) return CMF_EINVAL;
  if (a.head_cout < 1 || a.head_cout > 8 || a.np <= 0 || a.H <= 0 || a.W <= 0 || a.nc <= 0 || a.nc % 16) return CMF_EINVAL;
  if (a.bias || a.fo || a.ymask || a.mask_out || a.seed || a.live < 0 || a.live > 2 || (a.live && a.W % 2)) return CMF_EINVAL;
  if (!((a.W % 14 == 0 && a.H % 2 == 0) || (a.W % 8 == 0 && a.H % 4 == 0))) return CMF_EINVAL;
  const long long HW = (long long)a.H * a.W;
  if (HW > (1 << 24)) return CMF_ERANGE;
  if (a.x_ci != 16 || a.x_sl != SLICE) return CMF_EINVAL;                                                     // slice-major blocks
  if ((a.x_np | a.x_px | a.head_y_np | a.head_y_co | a.head_y_px) % 4) return CMF_EINVAL;                     // 16-byte accesses
  if (a.x_px < (long long)HID * a.nc || a.head_y_px < a.nc) return CMF_EINVAL;
  if ((uintptr_t)a.x % 16 || (uintptr_t)a.head_y % 16 || (uintptr_t)a.w % 4 || (uintptr_t)a.head_w % 4 || (uintptr_t)a.block_w1 % 16)
    return CMF_EINVAL;
  if ((uintptr_t)a.f % 8 || a.f_np % 8 || a.f_np < HW * (HID / 8)) return CMF_EINVAL;                         // one 8-byte word per pixel
  if ((uintptr_t)a.block_m1 % 8 || a.block_m1_np % 8 || a.block_m1_np < HW * (HID / 8)) return CMF_EINVAL;
  const int cp = a.head_cout <= 2 ? 2 : a.head_cout <= 4 ? 4 : 8;
  return cp == 2 ? launch<2>(a, s) : cp == 4 ? launch<4>(a, s) : launch<8>(a, s);
}
