/* cmf_amd.h -- C ABI of libcmf_amd.so: the MI355X (gfx950) kernels of the non-square-flow
 * log-density path of k-flouris/cmf.
 *
 * The reference is pure Python/PyTorch and has no FFI; each entry point below replaces a group of
 * ATen dispatches issued by the reference functions cited next to it (paths relative to the
 * reference repository root).  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 (or int32 where stated); the caller owns all
 *     buffers (no hidden allocations), sizes/strides are in ELEMENTS, not bytes;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); launches are asynchronous;
 *   - return value: 0 on success, a positive hipError_t from the launch, or a negative
 *     CMF_E* code for invalid arguments.  Nothing throws across this boundary;
 *   - every call is re-entrant and uses the calling thread's CURRENT device (one Python thread per GPU in one process is
 *     fine).  The only mutable global is a lock-free per-(device, kernel) memo of launch attributes already set
 *     (csrc/runtime.hip: dynamic-LDS limit, CU count); entries are idempotent and never removed.
 *
 * Data layouts
 *   primal tensor   P(b, r)        = p[b*p_b + r*p_r]                  (B, N) row-major, = torch layout
 *   tangent tensor  T(b, r, col)   = t[b*t_b + r*t_r + col]            col = Jacobian column, NC = ceil16(d)
 *       image nets : t_b = N*NC, t_r = NC          ("J panel" per sample: (B, C, H, W, NC))
 *       MLP nets   : t_b = NC,   t_r = B*NC        (feature-major: (F, B, NC))
 */
#ifndef CMF_AMD_H
#define CMF_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define CMF_EINVAL (-1)   /* bad shape / stride / mode                                   */
#define CMF_ERANGE (-2)   /* size exceeds what the kernel's index arithmetic supports    */

/* factor modes: how the per-(channel,pixel) multiplier applied to a conv/linear INPUT is derived
 * from the primal tensor `f` (jvp_layers.py:38-47 activation rules, applied on load) */
#define CMF_F_NONE 0      /* no multiplier                                               */
#define CMF_F_RELU 1      /* (f > 0)           relu'  : jvp_layers.py:40                 */
#define CMF_F_TANH 2      /* 1 - f*f           tanh'  with f = tanh output: :42-44       */
#define CMF_F_RAW  3      /* f itself          checkerboard mask: acl.py:54              */
#define CMF_F_SELF_RELU 4 /* relu of the input itself, elementwise (primal data carried in the column slots) */
#define CMF_F_RELU_BITS 5 /* relu' from a BIT MASK (cmf_conv_tangent_bf16x3 only): f points to bytes, one per (sample, pixel,
                             8-channel octet): bit j of f[np*f_np + px*(cin/8) + ci/8] = [activation(ci = 8*(ci/8)+j) > 0];
                             f_np in BYTES.  Written by cmf_conv_tangent's mask_out (below): 1/32 of the bytes of the
                             activation tensor, one byte load per loader thread and chunk instead of eight dwords.
                             A row (np, ci, px, :) of x whose bit is clear is NOT FETCHED and contributes an exact 0: a
                             non-finite value there does not propagate (with the float factor CMF_F_RELU it does: NaN * 0) */

/* primal epilogues */
#define CMF_O_NONE  0
#define CMF_O_TANH  1     /* y = tanh(v)                         (MLP hidden layer)                  */
#define CMF_O_STANH 2     /* y = w*tanh(v)+b2, g = w*(1-tanh^2)  (ScaledTanh2dModule networks.py:96-113) */

const char* cmf_version(void);

/* ---------------------------------------------------------------------------------------------
 * Weight packing.  w: [cout][cin][kh][kw] (nn.Conv2d / nn.Linear with kh=kw=1).
 * out: [ncog][taps][cin_pad][64] with cin_pad = ceil8(cin), ncog = ceil(cout/64); zero padded.
 * transpose != 0 packs the adjoint operator (cout<->cin swapped, taps flipped) used by the
 * reverse-mode sweep of the Hutchinson path (non_square.py:190-201).
 * Returns the number of floats written through *out_floats when out == NULL (size query).       */
int cmf_pack_weight(const float* w, float* out, int cout, int cin, int taps, int transpose,
                    long long* out_floats, void* stream);

/* Every stale pack of a model in ONE launch (a training step re-packs ~780 weights: round 3).  `table` is a DEVICE array of n
 * descriptors; entry k writes `total` elements of layout `kind` (0: cmf_pack_weight's floats, 1: cmf_pack_weight_bf16x3_t's bf16
 * halves, 2: cmf_pack_weight_f16x3's fp16 halves followed by its 16-byte trailer) of the weight `w` to `out`, exactly as the single-weight entry points do.  For kind 1 with transpose != 0, cout / cin are
 * the ADJOINT operator's (already swapped), as cmf_pack_weight_bf16x3_t expects them. */
typedef struct {
  const float* w; void* out; long long total;
  int cout, cin, taps, transpose, kind, reserved;
} cmf_pack_desc;
int cmf_pack_weights_batched(const cmf_pack_desc* table, int n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Tangent convolution / linear layer on fp32 MFMA (v_mfma_f32_16x16x4_f32).
 * Replaces, for all d Jacobian columns at once, the tangent half of get_conv2d_jvp / get_linear_jvp
 * (jvp_layers.py:49-64) fused with the activation rule of the preceding layer (:38-47) and the
 * residual add of ResidualBlock.jvp (networks.py:62-79):
 *     y(np, co, px, :) = sum_{ci,tap} W[co][ci][tap] * F(np, ci, px+tap) * x(np, ci, px+tap, :)  [+ r(np, co, px, :)]
 * taps == 9: 3x3, stride 1, zero padding 1 over an H x W image; taps == 1: 1x1 over H*W flat pixels
 * (an MLP layer is the 1x1 case with pixels = batch samples).                                    */
typedef struct {
  const float* x; long long x_np, x_ci, x_px;   /* input tangent tensor, NC contiguous columns       */
  const float* f; long long f_np, f_ci, f_px;   /* primal tensor the factor is derived from (or NULL) */
  int fmode;                                    /* CMF_F_*                                            */
  const float* w;                               /* packed by cmf_pack_weight                          */
  float* y;       long long y_np, y_co, y_px;
  const float* r; long long r_np, r_co, r_px;   /* residual (same shape as y) or NULL                 */
  int np, cin, cout, H, W, nc, taps;
  const float* bias;                            /* per-output-channel constant added to every column, or NULL  */
  int f_group;                                  /* >1: the factor tensor is sample-grouped: element (np, ci, px)
                                                   lives at f[(np / f_group)*f_np + ci*f_ci + px*f_px + np % f_group]
                                                   (primal activations kept in the "16 samples as columns" layout) */
  long long x_sl, y_sl, r_sl;                   /* element stride between 16-column slices: column col of x lives at
                                                   (col / 16)*x_sl + col % 16 (likewise y, r).  0 means 16 = plain
                                                   contiguous columns.  The slice-major hidden layout
                                                   [pixel][slice][channel][16] (x_px = C*nc, x_sl = C*16, x_ci = 16)
                                                   makes a wave's 16 channels x 16 columns one contiguous KiB        */
  const float* fo; long long fo_np, fo_co, fo_px; int fomode;
                                                /* OUTPUT-side factor (cmf_conv_tangent only; the split kernel rejects
                                                   it): y = Fo(np, co, px) * conv(F * x) + bias + r, Fo derived from fo
                                                   by fomode like F from f (NONE / RELU / TANH / RAW; SELF_RELU: fo is laid
                                                   out like y, columns included, and Fo = [fo > 0] per column -- primal
                                                   backward with 16 samples in the column slots).  This is what the
                                                   reverse (cotangent) sweep needs: the adjoint of "mask, then conv" is
                                                   "transposed conv, then mask" (weights from cmf_pack_weight(transpose=1)) */
  void* mask_out; long long mask_np;            /* cmf_conv_tangent only, cout % 16 == 0: also write the sign bits of the
                                                   stored values, [y > 0], in the CMF_F_RELU_BITS layout of the NEXT conv:
                                                   byte (sample*mask_np + px*(cout/8) + co/8), sample = np*nc + column
                                                   (primal pass: 16 samples in the column slots); NULL = off            */
  const float* amax_in; float* amax_out;        /* cmf_conv_tangent_f16x3 only (else ignored).  amax_in: one device float >= the largest
                                                   |x| the launch reads (NULL or 0: unknown -> no input scaling); the kernel multiplies x
                                                   by the power of two that puts that maximum in [2^13, 2^14) before the fp16 split, so no
                                                   input overflows fp16 and small ones keep their low half.  amax_out: one device float,
                                                   atomically raised to max(y) over the stored values (the caller zeroes it: the next
                                                   conv's amax_in, whose relu-on-load ignores negative values); NULL = off              */
  int live;                                     /* cmf_conv_tangent_bf16x3 only, fmode RELU / RELU_BITS, whole 64-channel groups, no bias / fo:
                                                   CHECKERBOARD output.  0 = every pixel.  1 / 2: only the pixels with (row + col) % 2 ==
                                                   live - 1 are computed -- the (1 - mask) pixels of Checkerboard2dAffineCouplingBijection
                                                   (acl.py:48-66, :68-78), all a coupler network's LAST hidden conv is ever read at, since the
                                                   1x1 conv behind it is pointwise -- and y is COMPACT: pixel (row, col) is stored at pixel
                                                   index row*(W/2) + col/2 (y_px = stride between compact pixels).  x, f and the residual r
                                                   keep the full H x W image; r is read at the live pixels.                              */
  const void* ymask; long long ymask_np;        /* cmf_conv_tangent_bf16x3 only (the other entry points reject it), fmode RELU / RELU_BITS, whole
                                                   64-channel groups, no live / fo / r / bias: STORE FILTER.  A relu' bit mask over the OUTPUT
                                                   channels in the CMF_F_RELU_BITS layout (byte np*ymask_np + px*(cout/8) + co/8, ymask_np in
                                                   bytes, both multiples of 4): rows (np, co, px, :) whose bit is clear are NOT WRITTEN -- y keeps
                                                   whatever it held there.  For an output whose only reader is a CMF_F_RELU_BITS launch with
                                                   this very mask, which does not fetch those rows.  NULL = store everything.             */
  const float* head_w; int head_cout;           /* cmf_conv_tangent_bf16x3 only: FOLDED HEAD (csrc/conv_head.hip).  head_w != NULL turns the launch
                                                   into a coupler network's last hidden conv AND the 1x1 output conv behind it (networks.py:50-60,
                                                   jvp_layers.py:38-64), without ever forming the hidden conv's 64 output channels:
                                                     yt(np, o, p, :) = sum_c G(o,c,p) r(np, c, p, :) + sum_{tap,ci} E(o,p,tap,ci) F(np, ci, p+tap) x(np, ci, p+tap, :)
                                                     G(o,c,p) = head_w[o][c] [head_a(np, c, p) > 0],   E(o,p,tap,ci) = sum_c G(o,c,p) w[c][ci][tap]
                                                   in plain fp32 FMAs, per-pixel E built in LDS.  Then: w is the RAW conv weight [64][64][3][3] (not a
                                                   pack), head_w the raw 1x1 weight [head_cout][64], head_cout <= 8, cin == cout == 64, taps == 9,
                                                   fmode CMF_F_RELU_BITS (rows of x whose bit is clear are not fetched), x and the residual r both
                                                   slice-major (x_ci = r_co = 16, x_sl = r_sl = 1024; r = the block's input h, required), live as
                                                   above, H x W as the split kernel accepts, no bias / fo / ymask / mask_out; y and its strides
                                                   are ignored.  Anything else: CMF_EINVAL.                                                  */
  const float* head_a; long long head_a_np, head_a_c, head_a_px;
                                                /* the float activation the 1x1 conv takes relu' from, (np, 64, H*W), always the FULL image */
  float* head_y; long long head_y_np, head_y_co, head_y_px;
                                                /* yt: nc contiguous columns per (np, o, pixel); live != 0: compact pixels, row*(W/2) + col/2 */
  const float* seed; long long seed_np, seed_col; const void* seed_w;
                                                /* cmf_conv_tangent_bf16x3 only: SEEDED RESIDUAL.  seed != NULL: the launch is block 0's conv2 of a
                                                   coupler network whose first conv has ONE input channel, and its residual h0 = conv0(mask . v)
                                                   (networks.py:40-47, :62-79) is not read but formed: y = conv(F . x) + conv0(seed), the second
                                                   term as one extra K-step per pixel on the fp32 MFMA (v_mfma_f32_16x16x4_f32).  seed is the panel cmf_seed_panel
                                                   writes (element np*seed_np + col*seed_col + r*(W+2) + c of the zero-bordered image), seed_w the
                                                   4 KiB pack of conv0's weight from cmf_pack_seed_weight.  Requires fmode CMF_F_RELU_BITS,
                                                   cout == 64, W % 14 == 0, H % 2 == 0, r == NULL, no live / ymask / fo / bias; else CMF_EINVAL. */
  const void* block_w1; const void* block_m1; long long block_m1_np;
                                                /* cmf_conv_tangent_bf16x3 only, with head_w: FOLDED BLOCK (csrc/conv_block_head.hip).  block_w1 != NULL
                                                   takes the folded head one conv further: the launch is the last residual block's conv1 AND its
                                                   conv2 (with the residual) AND the 1x1 output conv, and forms neither conv1's output nor the block's:
                                                     yt(np, o, p, :) = sum_c G(o,c,p) x(np, c, p, :) + sum_{d in 5x5, c} K(o,p,d,c) F(np, c, p+d) x(np, c, p+d, :)
                                                     K(o,p,d,c) = sum_{t2 + t1 = d} sum_ci E(o,p,t2,ci) [block_m1(np, ci, p+t2)] W1[ci][c][t1]
                                                   with G and E as in the folded head.  WHICH IS WHICH: x is now the block's INPUT h (slice-major, also
                                                   the residual: r must be NULL or x) and f / f_np the bit mask of ITS relu' (the activation in front
                                                   of conv1); block_m1 / block_m1_np (bytes) is the bit mask between conv1 and conv2 (what f is for the
                                                   folded head), same CMF_F_RELU_BITS layout; w stays conv2's RAW weight; block_w1 is conv1's weight as
                                                   packed by cmf_pack_block_weight.  K is built from split bf16 products (hi*hi + hi*lo + lo*hi, fp32
                                                   accumulation), everything else in fp32 FMAs.  A row of x is fetched only where F is set (at d = 0:
                                                   F or head_a > 0).  Other requirements as for the folded head; else CMF_EINVAL.              */
} cmf_conv_tangent_args;
/* (A launch with taps == 9, cin <= 2, cout % 64 == 0, no residual / bias / output factor / mask_out and fmode NONE or RAW -- the
 * first conv of a coupler network, networks.py:40-47 -- is an HBM write stream and runs on a VALU kernel instead of the MFMA one:
 * same contract, fp32 FMAs.)                                                                                                     */
int cmf_conv_tangent(const cmf_conv_tangent_args* a, void* stream);

/* Split-precision variant of cmf_conv_tangent for taps == 9, cin % 32 == 0, (W % 14 == 0 and H % 2 == 0) or (W % 8 == 0 and H % 4 == 0), and
 * cout % 64 == 0 or cout == 32 (anything else: CMF_EINVAL, use cmf_conv_tangent): operands are split
 * v = hi + lo (bf16 each) and multiplied as hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 with fp32
 * accumulation (fp32-grade result, ~2^-16 relative per product).  `w` must come from
 * cmf_pack_weight_bf16x3 (out == NULL: size query in bytes through *out_bytes).  Output-side factor: only with
 * fmode CMF_F_NONE, no residual, cout % 64 == 0 and fomode CMF_F_RELU_BITS -- fo is then a relu' bit mask over the OUTPUT
 * channels (byte np*fo_np + px*(cout/8) + co/8, fo_np in bytes; written by cmf_relu_bits or mask_out): the transposed convs of
 * the reverse sweep.  A residual is accepted together with that bit mask only IN PLACE (r == y with y's strides, no bias):  y <- y + Fo . conv(x)  -- the skip connection of the reverse sweep; entries the mask switches off are not written at all
 * (they keep their bits).  mask_out is not supported. */
int cmf_pack_weight_bf16x3(const float* w, void* out, int cout, int cin, long long* out_bytes, void* stream);
/* the same pack of the ADJOINT operator straight from the layer's weight: transpose != 0 reads w as [cin][cout][3][3] and packs
 * [cout][cin][tap] = w[ci][co][8 - tap] (channels swapped, taps flipped: cmf_pack_weight's transpose for the split kernel) */
int cmf_pack_weight_bf16x3_t(const float* w, void* out, int cout, int cin, int transpose, long long* out_bytes, void* stream);
int cmf_conv_tangent_bf16x3(const cmf_conv_tangent_args* a, void* stream);
/* The seeded residual's operands (cmf_conv_tangent_args.seed).  cmf_pack_seed_weight: w = conv0's weight [64][1][3][3] -> out, 4096
 * bytes, 16-byte aligned: [co tile 4][lane 64][4] fp32, lane = 16 kq + co % 16, element j = tap 3 kq + j (kq, j < 3, else 0).
 * cmf_seed_panel: out(np, col, r, c) = mask(r-1, c-1) * v(np, (r-1) W + (c-1), col) over the (H+2) x (W+2) image with an exact-zero
 * border (and an exact 0 wherever mask == 0, whatever v holds there; mask NULL = all ones); v has nc contiguous columns per pixel
 * (pixel stride v_px, sample stride v_np), out_col >= (H+2)(W+2) + 1 floats per column plane (the padding is zeroed), out_np >=
 * nc out_col, nc % 16 == 0.                                                                                                      */
int cmf_pack_seed_weight(const float* w, void* out, void* stream);
/* The folded block's W1 operand (cmf_conv_tangent_args.block_w1): w = conv1's weight [64][64][3][3] -> out (16-byte aligned), split into
 * bf16 hi / lo halves and laid out as the B fragments of v_mfma_f32_16x16x32_bf16.  out == NULL: size query in bytes through *out_bytes. */
int cmf_pack_block_weight(const float* w, void* out, long long* out_bytes, void* stream);
int cmf_seed_panel(const float* v, long long v_np, long long v_px, const float* mask, float* out, long long out_np, long long out_col,
                   int np, int H, int W, int nc, void* stream);

/* Probe front of a checkerboard ResNet coupler's tangent network (evaluation; csrc/probe_front.hip).  The network's first conv
 * (cin <= 2 -> 64, networks.py:40-47, input mask . v: acl.py:48-52) and block 0's conv1 (64 -> 64, networks.py:62-79) are one linear
 * map from the input rows v to conv1's output u0 with a 5 x 5 support per output pixel, in which only the pass-through pixels carry
 * a row.  With the rows coloured so that a 5 x 5 window holds every class at most once, the response R of the two convs to one probe
 * column per class (the sum of the unit impulses at that class's rows) holds the map's coefficients, and
 *     y(np, p, sl, co, 0:16) = sum over (dy, dx) in raster order of the window, q = p + (dy, dx) inside the image, c ascending,
 *                                cls[c*H*W + q] >= 0 of   r(np, p, cls/16, co, cls%16) * t(np, c, q, 16 sl : 16 sl + 16)
 * in fp32 fmaf, in exactly that order (a column's bits do not depend on its slot, nc or np).
 *   r   probe responses, [64][16] blocks: element at np*r_np + p*r_px + (cls/16)*1024 + co*16 + cls%16; ns blocks per pixel (1 or 2)
 *   t   input rows: nc contiguous columns at np*t_np + c*t_c + q*t_px
 *   cls class table, cin*H*W signed bytes on the device; entries outside [0, 16 ns) mean "no input row here"
 *   y   slice-major like the hidden tangents: element at np*y_np + p*y_px + (col/16)*1024 + co*16 + col%16
 *   ymask (or NULL) STORE FILTER as in cmf_conv_tangent_args (byte np*ymask_np + p*8 + co/8, both multiples of 8): a row (np, co, p)
 *       whose bit is clear is neither computed nor written, and its r row is not fetched (it may hold anything).
 * cin 1 or 2, 64 output channels, nc % 16 == 0, 16-byte aligned pointers, strides % 4 == 0; else CMF_EINVAL / CMF_ERANGE.           */
typedef struct {
  const float* r; long long r_np, r_px;
  const float* t; long long t_np, t_c, t_px;
  const signed char* cls;
  float* y;       long long y_np, y_px;
  const void* ymask; long long ymask_np;
  int np, cin, H, W, nc, ns;
} cmf_probe_apply_args;
int cmf_probe_apply(const cmf_probe_apply_args* a, void* stream);

/* fp16 split-precision variant for the PRIMAL hidden convs of a ResNet coupler (networks.py:50-60 with 16 samples in the column
 * slots): fmode CMF_F_SELF_RELU, taps == 9, cin % 32 == 0, cout % 64 == 0, tiles as cmf_conv_tangent_bf16x3, no output factor.
 * Operands are split v = hi + lo with hi = fp16(v), lo = fp16(v - hi) (11 + 11 significant bits) and multiplied as
 * hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_f16 with fp32 accumulation: ~2^-22 relative per product against bf16x3's 2^-16, so
 * the relu masks taken from these activations flip as rarely as with exact fp32 products (profiles/r04_primal_precision_study.txt)
 * at the bf16 MFMA rate.  fp16's narrow exponent is handled by exact power-of-two scales: the weights are packed times 2^k with
 * max |w| 2^k in [2^11, 2^12) (cmf_pack_weight_f16x3: same layout as cmf_pack_weight_bf16x3_t plus a 16-byte trailer
 * {2^k, 2^-k, 0, 0}; the max is taken on the device, no host synchronisation), the inputs times the power of two derived from
 * amax_in; the epilogue undoes both (exact), the residual enters scaled.  mask_out IS supported (the sign bits of the stored
 * values, as cmf_conv_tangent writes them).  `w` must come from cmf_pack_weight_f16x3.
 * BACKWARD form (the data-gradient convs of the same blocks under loss.backward(), trainer.py:213): fmode CMF_F_NONE, `w` the pack of
 * the adjoint operator (transpose = 1), fo != NULL with fomode CMF_F_SELF_RELU -- a float tensor laid out like y (strides fo_np /
 * fo_co / fo_px, columns included) -- and  y = [fo > 0] * conv(x) + r  per column; no bias, no mask_out; *amax_out = max |y|.          */
int cmf_pack_weight_f16x3(const float* w, void* out, int cout, int cin, int transpose, long long* out_bytes, void* stream);
int cmf_conv_tangent_f16x3(const cmf_conv_tangent_args* a, void* stream);
/* the same with the work-item size chosen by the caller: item_channels = 64 (a workgroup's item is a pixel tile x 16 samples x 64
 * output channels), 32 (half of a 64-channel group per item: twice the items, for launches that would leave most CUs without one)
 * or 0 = cmf_conv_tangent_f16x3's own choice (32 when the 64-channel items number at most half the CUs).  Results are
 * bit-identical between the two sizes.  Launches on 4 x 8 pixel tiles (16- / 32-wide images) always run 32-channel items: the
 * 64-channel form does not fit the 256 VGPRs of a wave there (it spilled to scratch).                                          */
int cmf_conv_tangent_f16x3_item(const cmf_conv_tangent_args* a, int item_channels, void* stream);
/* out[0] = max(out[0], max_i |x[i]|) over n floats (out is NOT cleared: the caller zeroes it or chains several tensors).   */
int cmf_absmax(const float* x, long long n, float* out, void* stream);

/* Weight gradient of the tangent convolution (training; the reference gets it from autograd through
 * get_conv2d_jvp / get_linear_jvp, jvp_layers.py:49-64, under loss.backward(), trainer.py:213):
 *     dw[co][ci][tap] += sum_{np, px, col} gy(np, co, px, col) * F(np, ci, px+tap) * x(np, ci, px+tap, col)
 * `a` describes the FORWARD launch: x, f, fmode (NONE / RELU / TANH / RAW, or SELF_RELU: x's own relu, elementwise), f_group, np, cin, cout, H, W, nc, taps and the
 * strides are read from it; gy is the cotangent of y and is addressed like y (y_np, y_co, y_px, y_sl); a->w, y, r, bias,
 * fo and mask_out are ignored.  dw: [cout][cin][taps] fp32 (the nn.Conv2d / nn.Linear weight layout), accumulated into.
 * ws: caller-owned workspace of cmf_conv_tangent_wgrad_ws(a) bytes (partial sums, reduced in a fixed order).         */
long long cmf_conv_tangent_wgrad_ws(const cmf_conv_tangent_args* a);
int cmf_conv_tangent_wgrad(const cmf_conv_tangent_args* a, const float* gy, float* dw, float* ws, long long ws_bytes,
                           void* stream);
/* Split-precision variant (hi*hi + hi*lo + lo*hi on bf16 MFMA, fp32 accumulation, like cmf_conv_tangent_bf16x3) for taps == 9,
 * cin % 64 == 0, cout % 64 == 0, nc % 32 == 0, fmode CMF_F_NONE, CMF_F_RELU (float factor tensor, f_group <= 1), CMF_F_RELU_BITS (f = the
 * relu' bit mask of cmf_conv_tangent_bf16x3's input factor: byte np*f_np + px*(cin/8) + ci/8, f_np in bytes) or CMF_F_SELF_RELU;
 * anything else: CMF_EINVAL, use cmf_conv_tangent_wgrad.  Same arguments and workspace.                                      */
int cmf_conv_tangent_wgrad_bf16x3(const cmf_conv_tangent_args* a, const float* gy, float* dw, float* ws, long long ws_bytes,
                                  void* stream);
/* nprob <= CMF_WGRAD_MAX_BATCH problems of ONE shape in one launch: x[p], gy[p], dw[p] are HOST arrays of device pointers (a->x is
 * ignored; everything else -- strides, np, nc, H, W, fmode NONE or SELF_RELU -- is read from `a` and shared).  The 256 persistent
 * workgroups are split evenly over the problems.  Made for the primal weight gradients of a coupler's hidden convs at a training
 * shard's few sample groups (trainer.py:213 differentiates 16 such convs per coupler): 28 - 56 image rows per problem leave most of the
 * chip idle when launched one by one.  Same workspace as the single-problem call. */
#define CMF_WGRAD_MAX_BATCH 16
int cmf_conv_tangent_wgrad_bf16x3_batched(const cmf_conv_tangent_args* a, int nprob, const float* const* x, const float* const* gy,
                                          float* const* dw, float* ws, long long ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Primal convolution / linear layer on fp32 MFMA: nn.Conv2d / nn.Linear forward of the coupler
 * networks (networks.py:50-60, :103-106, :206-224) with the preceding activation fused on load and
 * bias / residual / tanh epilogues:
 *     v(b, co, px) = sum W[co][ci][tap] * in(b, ci, px+tap) + bias[co] [+ r(b, co, px)]
 *     in = x | relu(x) | x*f        (imode CMF_F_NONE | CMF_F_RELU | CMF_F_RAW with mask f(ci,px))
 * omode CMF_O_NONE: y = v;  CMF_O_TANH: y = tanh(v);  CMF_O_STANH: y = sw[co]*tanh(v)+sb[co] and
 * g = sw[co]*(1-tanh(v)^2) (the tangent multiplier of ScaledTanh2dModule.jvp, networks.py:108-113).
 * Element (b, c, px) of a tensor t lives at t[b*t_b + c*t_c + px*t_px].                           */
typedef struct {
  const float* x; long long x_b, x_c, x_px;
  const float* f; long long f_c, f_px;          /* CMF_F_RAW mask (shared over the batch) or NULL     */
  int imode;
  const float* w; const float* bias;            /* packed weights; bias[cout] or NULL                 */
  const float* sw; const float* sb;             /* CMF_O_STANH per-channel scale / offset             */
  float* y;       long long y_b, y_c, y_px;
  float* g;                                     /* CMF_O_STANH derivative factor (strides of y)|NULL  */
  const float* r; long long r_b, r_c, r_px;
  int omode;
  int B, cin, cout, H, W, taps;
} cmf_conv_primal_args;
int cmf_conv_primal(const cmf_conv_primal_args* a, void* stream);

/* (B, N) row-major  <->  (B/G, N, G) sample-grouped layout, G = 16: the primal hidden activations of the ResNet
 * couplers run through the tangent kernels with 16 samples in the 16 column slots (B % 16 == 0).             */
int cmf_primal_regroup(const float* in, float* out, int B, long long N, int to_grouped, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Affine coupling transforms (acl.py:43-66, :101-146), in place on the primal / tangent tensors.
 * The three mask types (checkerboard acl.py:68-78, split-channel :185-189, alternating :207-214)
 * are all expressed by index maps over the n_mod modified elements of a sample:
 *   zi[e]: element of z that is modified; ti[e] / si[e]: elements of the coupler output holding its
 *   shift / log-scale (couplers.py:52-59 chunking).  Pass-through elements are untouched.
 * encode (x_to_z): z = (x + t) * exp(s);  if lj != NULL: lj[b] += sum_e s       (log-jac, acl.py:22-23)
 * decode (z_to_x): x = z * exp(-s) - t                                                             */
int cmf_acl_primal(float* z, long long z_b, const float* y, long long y_b, const int* zi, const int* si,
                   const int* ti, int n_mod, int B, int decode, float* lj, void* stream);
/* tangent: T(b, zi[e], :) = exp(-s) * (T(b, zi[e], :) - z_old * sdot) - tdot   (acl.py:61-64, :137-144)
 *   sdot = gs * yt(b, si[e], :), tdot = gt * yt(b, ti[e], :), gs/gt = g(b, si[e]) / g(b, ti[e]) or 1 when
 *   g == NULL; z_old = z(b, zi[e]) BEFORE cmf_acl_primal decode is applied; s from y.
 * yt == NULL: the network's tangent is identically zero (its pass-through input is structurally zero, e.g. the channels
 *   SplitDensity.pad_inputs appended, split.py:50-52): T(b, zi[e], :) *= exp(-s).
 * y_b == 0 (here and in cmf_acl_primal): one network output shared by every sample (same situation: the input is zero).  */
/* cotangent (adjoint of cmf_acl_tangent, for J^T w / the reverse sweep): with c = C(b, zi[e], :) on entry,
 *   yc(b, ti[e], :) = -gt * c,   yc(b, si[e], :) = -(exp(-s) * z_old * gs) * c,   C(b, zi[e], :) = exp(-s) * c.
 * yc rows that no element maps to must be zero (the caller clears yc).
 * yc == NULL: only C is updated (the cotangent of the network's input lands on rows that are dropped).   */
int cmf_acl_cotangent(float* c, long long c_b, long long c_r, float* yc, long long yc_b, long long yc_r, int nc,
                      const float* z, long long z_b, const float* y, long long y_b, const float* g, const int* zi,
                      const int* si, const int* ti, int n_mod, int B, void* stream);
/* Primal backward of the coupling update (training), in place on the primal cotangent dx (z-shaped; pass-through elements keep
 * their value), accumulating the cotangent of the network output into dy (y-shaped):
 *   decode != 0 (x_mod = z_mod e^{-s} - t, `z` = the tensor BEFORE the update, acl.py:57-66):
 *       dx[zi] *= e^{-s};  dy[si] -= dx z_mod e^{-s};  dy[ti] -= dx
 *   decode == 0 (z_mod = (x_mod + t) e^{s}, `z` = the layer INPUT x, acl.py:43-46):
 *       dx[zi] *= e^{s};   dy[ti] += dz e^{s};  dy[si] += dz (x_mod + t) e^{s} + dlj[b]   (dlj: cotangent of the log-jacobian, or NULL) */
int cmf_acl_primal_backward(float* dx, long long dx_b, const float* z, long long z_b, const float* y, long long y_b, float* dy,
                            const int* zi, const int* si, const int* ti, int n_mod, int B, int decode, const float* dlj,
                            void* stream);
/* Cross terms of the coupling update for training (autograd through acl.py:48-66, :113-146 in the reference): the tangent
 * update  out(b, zi[e], :) = es (v - zo gs sd) - gt td  of cmf_acl_tangent also depends on primal values.  Given the
 * cotangent c of `out` (rows zi[e], BEFORE cmf_acl_cotangent rewrites them), the saved input rows v (compact: row e at
 * v + b*v_b + e*v_r) and the network's raw tangent yt, accumulates (+=) the column reductions
 *   dy[b][si[e]] += d/ds,   dz[b][zi[e]] += d/d zo,   dg[b][si[e]] += d/d gs,   dg[b][ti[e]] += d/d gt
 * (dg and g both NULL for networks without the ScaledTanh output stage).
 * yt == NULL (network tangent identically zero): only dy[b][si[e]] -= sum_col c es v is accumulated; dz, dg unused.  */
int cmf_acl_cross_terms(const float* c, long long c_b, long long c_r, const float* v, long long v_b, long long v_r,
                        const float* yt, long long yt_b, long long yt_r, int nc, const float* z, long long z_b,
                        const float* y, long long y_b, const float* g, const int* zi, const int* si, const int* ti,
                        int n_mod, int B, float* dz, float* dy, float* dg, void* stream);
int cmf_acl_tangent(float* t, long long t_b, long long t_r, const float* yt, long long yt_b, long long yt_r,
                    int nc, const float* z, long long z_b, const float* y, long long y_b, const float* g,
                    const int* zi, const int* si, const int* ti, int n_mod, int B, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Index-map moves: squeeze / unsqueeze (reshaping.py:89-114), split padding (split.py:50-52), tail
 * gather / scatter (non_square.py:381-384, :397-404), layout changes.
 * out(b, r) = idx[r] >= 0 ? in(b, idx[r]) : 0,   r < n_out.                                        */
int cmf_gather_primal(const float* in, long long in_b, float* out, long long out_b, const int* idx,
                      int n_out, int B, void* stream);
int cmf_gather_tangent(const float* in, long long in_b, long long in_r, float* out, long long out_b,
                       long long out_r, const int* idx, int n_out, int nc, int B, void* stream);
/* Column expansion of a contiguous tangent tensor of `rows` rows: out(row, c) = colmap[c] >= 0 ? in(row, colmap[c]) : 0 for c <
 * nc_out (nc_out % 4 == 0).  The first coupling layer of the decode sweep sees one-hot seed tangents (non_square.py:303-304): a
 * Jacobian column whose seed element is not among the elements that layer's network reads has an identically zero network tangent
 * there, so the network runs on the other columns only (nc_in of them, packed) and its output is expanded back with this.    */
int cmf_expand_columns(const float* in, int nc_in, float* out, int nc_out, const int* colmap, long long rows, void* stream);
/* Seed tangents at the tail (non_square.py:303-304, :406-410): col_of[r] = Jacobian column whose unit
 * vector lands on element r (or -1).  eps == NULL: T(b, r, c) = (col_of[r] == c)  (identity seed, exact
 * path); else T(b, r, c) = eps[b][col_of[r]][c] for c < S (Hutchinson probes, non_square.py:204-215).  */
int cmf_seed_tangent(float* t, long long t_b, long long t_r, const int* col_of, int n_rows, int nc,
                     const float* eps, int d, int S, int B, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused J^T J Gram (MFMA) + Cholesky + log-det + metric L1 terms: replaces
 * non_square.py:307-308 (stack + bmm), :280-294 (cholesky, 2*sum log diag) and :87-100 (g_kk / g_ij).
 *   jtj   [B][d][d]  out, the (possibly jittered) Gram matrix;  logdet, l1_off, l1_diag: [B]
 *   info  [B] int32: 0 ok, k+1 = non-positive / non-finite pivot at column k
 *   fail  int32[8]: fail[a] != 0 iff attempt a failed for ANY sample (whole-batch retry, :284-288)
 * cmf_gram_cholesky is attempt 0.  cmf_cholesky_retry(attempt = a >= 1) returns immediately on the
 * device unless fail[a-1] != 0; otherwise it adds eps * 10^(a-1) to the diagonal of EVERY sample's
 * jtj (in place) and refactorises.  The host may enqueue all retries without synchronising.
 * Widths: nc % 16 == 0, d <= nc <= 512 (cmf_cholesky_retry: d <= 512).  nc <= 128 keeps the whole matrix in LDS; 128 < nc runs
 * head_wide.hip (Gram on a (tile, sample) grid, blocked factorisation in global memory that restores jtj afterwards, so jtj is
 * exactly symmetric and intact on return).  Wider: CMF_EINVAL.
 * Layout contract: row r of sample b is the nc floats at t + b * t_b + r * t_r (t_r >= nc, t_b and t_r multiples of 4, t 16-byte
 * aligned); nothing outside those nc floats of a row is read.  The padding columns d .. nc - 1 must hold ZEROS: the nc <= 64
 * kernel sums |G_ij| over whole 4 x 4 register blocks and relies on the padding rows / columns of G being exact zeros.       */
int cmf_gram_cholesky(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B,
                      float* jtj, float* logdet, float* l1_off, float* l1_diag, int* info, int* fail,
                      void* stream);
int cmf_cholesky_retry(float* jtj, int d, int B, int attempt, float eps0, float* logdet, float* l1_diag,
                       int* info, int* fail, void* stream);
/* Which kernel cmf_gram_cholesky runs for (n_rows, nc, t_r): a host-only query, no launch, no device access, and the function the
 * dispatcher itself switches on.  CMF_GRAM_STAGED1 .. 8: the LDS-staged kernel with NT = nc / 16 column tiles (64-bit addressing);
 * CMF_GRAM_RING64 (nc 32 / 48 / 64) and CMF_GRAM_DIRECT128 (nc 128): the kernels that stream the panel through a buffer
 * descriptor with 32-bit byte offsets, chosen only when every offset they form -- the descriptor range n_rows * t_r * 4, the
 * group offset the prefetch ring runs past the panel's end, the lane offset -- stays below CMF_GRAM_RING_LIMIT; CMF_GRAM_WIDE:
 * head_wide.hip (nc > 128); CMF_GRAM_INVALID: n_rows <= 0, nc not a multiple of 16 in 16 .. 512, t_r < nc or t_r % 4 != 0.   */
#define CMF_GRAM_INVALID   0
#define CMF_GRAM_STAGED1   1
#define CMF_GRAM_STAGED8   8
#define CMF_GRAM_RING64    64
#define CMF_GRAM_DIRECT128 128
#define CMF_GRAM_WIDE      512
#define CMF_GRAM_RING_LIMIT 0x7fffff00LL
int cmf_gram_cholesky_family(int n_rows, int nc, long long t_r);
/* Conditioning of the factorised Gram matrices (the precision guard of the no-grad log-density path):
 *   cond[b] = kappa_1(G_b) = ||G_b||_1 ||G_b^-1||_1 of the matrix cmf_gram_cholesky / cmf_cholesky_retry left in jtj (the
 *   jittered Gram whose log-det is reported), computed exactly in float64 (Cholesky, triangular inverse, |G^-1| column sums);
 *   +inf when info[b] != 0, when the float64 factorisation meets a non-positive pivot, or when the value is not finite.
 *   jtj is read (whole for ||G||_1, its lower triangle for the factorisation) and never written.
 *   flagged_idx [B] int32: the samples with cond > threshold in ascending order (a prefix-sum compaction: independent of the order
 *   in which workgroups finish), -1 after the last one;  flagged_count [1] int32: their number.  threshold may be +inf (nothing
 *   flagged); NaN: CMF_EINVAL.
 * Widths 1 <= d <= 512 (else CMF_EINVAL).  d <= 128 works in LDS and ignores ws (may be NULL); 128 < d needs a caller-owned
 * workspace ws of 2 * B * d * d floats, 8-byte aligned (a float64 d x d matrix per sample).  No allocation, no synchronisation. */
int cmf_gram_condition(const float* jtj, const int* info, int d, int B, float threshold, float* cond, int* flagged_idx,
                       int* flagged_count, float* ws, void* stream);
/* Dataset-level statistics of the pull-back metric (the reference's visualizer.py:191-198, :305-317): the launch
 * ADDS the samples of jtj [B][d][d] to  state = [S_G (d*d) | S_cos (d*d) | count | skipped]  (2 d^2 + 2 doubles, 8-byte aligned):
 *   n_k = sqrt(G_kk) + 1e-8,  cos_ij = G_ij / (n_i n_j), float64 arithmetic on the float32 input;
 *   a sample is valid iff every G_kk is finite and > 0: valid samples add G to S_G, cos to S_cos and 1 to count, the others
 *   add 1 to skipped and nothing else;
 *   sample_macs [B] float32 (or NULL): mean over i != j of |cos_ij| (0 for d = 1), NaN for a skipped sample.
 * No floating-point atomics: workgroups sum `chunk` (1 .. 64) consecutive samples into ws, a second launch folds the chunks
 * onto state in chunk order -- the summation order depends on (B, d, chunk) only and repeated call sequences are bit-identical.
 * ws: caller-owned, 8-byte aligned, ws_doubles >= cmf_metric_stats_ws(d, B, chunk, sample_macs != NULL) doubles (that function
 * returns CMF_EINVAL for sizes out of range).  1 <= d <= 512.  jtj is only read.  No allocation, no synchronisation.        */
long long cmf_metric_stats_ws(int d, int B, int chunk, int with_sample_macs);
int cmf_metric_stats_accumulate(const float* jtj, int d, int B, int chunk, double* state, double* ws, long long ws_doubles,
                                float* sample_macs, void* stream);
/* Per-sample spectrum of the Gram matrix: the symmetric eigen-decomposition G_b = V_b diag(lambda_b) V_b^T of
 * jtj [B][d][d] (float32, as cmf_gram_cholesky leaves it after one attempt; only the lower triangle i >= j is read, jtj is never
 * written), in float64 by the cyclic two-sided Jacobi method with the round-robin ordering, one workgroup per sample.  A pair
 * (p, q) is rotated iff |a_pq| > 2^-53 sqrt(|a_pp a_qq|); the sweeps end after the first one without a rotation or after
 * CMF_SPECTRUM_MAX_SWEEPS.
 *   eigenvalues [B][d] float64: ascending; equal values keep the order of their position on the converged diagonal.  Zero and
 *     negative eigenvalues are reported as they are.
 *   vectors [B][d][d] float64 or NULL: column k belongs to eigenvalue k; its component of largest magnitude is positive (lowest
 *     row index on ties).  For 64 < d the slice of a sample is also its workgroup's working storage during the launch.
 *   sweeps [B] int32: sweeps executed, the final rotation-free one included (1 for a diagonal input).
 *   info [B] int32: 0 converged; 1 sweep cap reached (eigenvalues / vectors hold the current diagonal / V); 2 a non-finite entry
 *     in the lower triangle (eigenvalues and vectors filled with NaN, sweeps = 0).
 * A sample's outputs are a function of its d x d input alone (no atomics; independent of B, of its position in the batch and of
 * the order in which workgroups finish), and the eigenvalues are the same bits with and without vectors.
 * 1 <= d <= 128 (the float64 matrix lives in LDS), B >= 1, eigenvalues and vectors 8-byte aligned, else CMF_EINVAL.  No
 * allocation, no synchronisation.                                                                                            */
#define CMF_SPECTRUM_MAX_SWEEPS 64
int cmf_gram_spectrum(const float* jtj, int d, int B, double* eigenvalues, double* vectors, int* sweeps, int* info, void* stream);
/* One damped Gauss-Newton step of the projection onto the manifold, per sample, in float64 on float32 inputs:
 *   r = x - xhat,  g = J^T r,  A = G + damping[b] diag(G),  delta = A^-1 g  (Cholesky of A in LDS, pivots only).
 *   t, t_b, t_r, n_rows, nc: the Jacobian stack as cmf_gram_cholesky takes it (both layouts through the two strides); columns
 *     d .. nc - 1 are padding whose contents influence no output.
 *   jtj [B][d][d] float32: the Gram matrix as one cmf_gram_cholesky attempt leaves it; only the lower triangle i >= j is read,
 *     nothing is written.  x, xhat [B][n_rows] float32, contiguous.  damping [B] float64, >= 0.
 *   grad [B][d], delta [B][d] float64;  stats [B][4] float64 = { ||r||^2, g^T delta, delta^T G delta, max_k |g_k| };
 *   info [B] int32: 0 ok; 1 a pivot of A was not positive and finite (delta, stats[1], stats[2] are NaN; grad, stats[0], stats[3]
 *     are valid); 2 a non-finite value in x, xhat, the first d columns of t or the lower triangle of jtj (every output is NaN).
 * Residual-only mode, t == NULL: only stats[b][0] = ||r||^2 and info[b] (0 or 2) are written -- the same bits as the full mode
 * gives; t_b, t_r, nc, d are ignored and jtj, damping, grad, delta may be NULL.
 * A sample's outputs are a function of its own inputs and of (n_rows, nc, d) alone: no atomics, independent of B, of its position
 * in the batch and of the order in which workgroups finish, and they repeat bit for bit.
 * With t: 1 <= d <= 128 (the float64 matrix lives in LDS), nc % 16 == 0, d <= nc, t_b and t_r >= nc and % 4 == 0, t 16-byte
 * aligned; always: n_rows, B >= 1, float64 pointers 8-byte aligned.  Anything else: CMF_EINVAL.  No allocation, no
 * synchronisation.                                                                                                            */
int cmf_gauss_newton_step(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B,
                          const float* jtj, const float* x, const float* xhat, const double* damping,
                          double* grad, double* delta, double* stats, int* info, void* stream);
/* One damped, weighted Gauss-Newton step per sample: the projection with missing or unevenly trusted elements,
 *   min_z sum_i w_i (x_i - g(z)_i)^2.  In one pass over the rows of J with w_i > 0:
 *   G_w = J^T diag(w) J (float32 MFMA accumulation; the operand w_i J_ik is rounded to float32),  r = x - xhat,
 *   g_w = J^T (w o r) and cost = sum_i w_i r_i^2 in float64;  then  A = G_w + damping[b] diag(G_w),  delta = A^-1 g_w  in float64
 *   on the float32 matrix written to gram (Cholesky of A in LDS, pivots only: the elimination of cmf_gauss_newton_step).
 *   t, t_b, t_r, n_rows, nc, x, xhat, damping: as for cmf_gauss_newton_step.  w [B][n_rows] float32, contiguous, >= 0.
 *   A row with w == 0 is never read -- x, xhat and row i of t may hold anything there, NaN included, and reach no output.
 *   gram [B][d][d] float32 = G_w, symmetric bit for bit (the lower tile triangle is computed, the rest mirrored);
 *   grad [B][d], delta [B][d] float64;  stats [B][4] float64 = { cost, g^T delta, delta^T G_w delta, max_k |g_k| };
 *   info [B] int32: 0 ok; 1 a pivot of A was not positive and finite (delta, stats[1], stats[2] are NaN; gram, grad, stats[0],
 *     stats[3] are valid): fewer rows with w > 0 than d at damping 0, or no such row at all; 2 a weight that is negative or not
 *     finite, or a non-finite value in a row with w > 0 of x, xhat or the first d columns of t (every output is NaN).
 * Cost-only mode, t == NULL: only stats[b][0] and info[b] (0 or 2) are written -- the same bits as the full mode gives; t_b, t_r,
 *   nc, d are ignored and damping, gram, grad, delta may be NULL.
 * A sample's outputs are a function of its own inputs and of (n_rows, d) alone, the summation order of (n_rows, d) and of the
 * positions of the rows with w > 0: no atomics, independent of B, of the sample's position in the batch and of the order in which
 * workgroups finish, and they repeat bit for bit.
 * With t: 1 <= d <= 128, nc % 16 == 0, d <= nc, t_b and t_r >= nc and % 4 == 0, t 16-byte aligned; always: n_rows, B >= 1,
 * float64 pointers 8-byte aligned.  Anything else: CMF_EINVAL.  No allocation, no synchronisation.                             */
int cmf_weighted_gauss_newton_step(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B,
                                   const float* w, const float* x, const float* xhat, const double* damping, float* gram,
                                   double* grad, double* delta, double* stats, int* info, void* stream);
/* Robust scale, IRLS weights and robust cost of a residual, per sample: what turns the weighted projection into
 * one that finds its own outliers.  In float64 on r_i = (double)x_i - (double)xhat_i over the USED elements, prior_i > 0:
 *   s = scale_in[b], or (scale_in == NULL) 1.4826 med with med the LOWER median of |r_i| over the m used elements -- the order
 *     statistic of 0-based rank (m - 1) / 2, exact for any n_rows (a radix select on the bit patterns; -0.0 counts as +0.0);
 *   u_i = r_i / s;  loss 0, Huber:  omega = |u| <= c ? 1 : c / |u|,  rho = |u| <= c ? u^2 / 2 : c |u| - c^2 / 2;
 *                   loss 1, Tukey:  t = max(0, 1 - (u / c)^2),  omega = t^2,  rho = (c^2 / 6) (1 - t^3);   c = tuning;
 *   w[b][i] = float(prior_i omega_i), exactly 0.0f where prior_i == 0;
 *   stats[b] = { s, 2 s^2 sum_i prior_i rho_i, m, sum_i omega_i } -- the cost is sum_i prior_i r_i^2 where nothing is down-weighted.
 *   x, xhat [B][n_rows] float32, contiguous.  prior [B][n_rows] float32 >= 0, or NULL for all 1: the known weights of
 *     cmf_weighted_gauss_newton_step.  An element with prior == 0 is never read in x or xhat -- they may hold anything there, NaN
 *     included, and reach no output.  w [B][n_rows] float32, or NULL: cost-only mode, the same stats and info bits.
 *   info [B] int32: 0 ok; 2 a prior that is negative or not finite, or a non-finite x or xhat at a used element (w and stats are
 *     NaN); 3 s is not finite or not > 0 -- no used element (the median of nothing is NaN), a zero median, a bad scale_in -- (w
 *     and stats are NaN, except stats[0] = s).  NaN weights make cmf_weighted_gauss_newton_step report info 2.
 * A sample's outputs are a function of its own inputs and of n_rows alone: the sums run in a fixed order, there are no
 * floating-point atomics, and they are independent of B, of the sample's position in the batch and repeat bit for bit.
 * n_rows, B >= 1; x, xhat, stats, info not NULL; loss 0 or 1; tuning > 0; float64 pointers 8-byte aligned.  Anything else:
 * CMF_EINVAL, and nothing is launched.  No allocation, no synchronisation.                                                       */
int cmf_robust_weights(const float* x, const float* xhat, const float* prior, int n_rows, int B, int loss, double tuning,
                       const double* scale_in, float* w, double* stats, int* info, void* stream);
/* A linear measurement operator carried through one decode sweep: for the recovery min_z ||y - a g(z)||^2.
 *   k(b, m, c) = sum_i a[m][i] t(b, i, c)  for every column c < nc  (the Jacobian stack K_b = a J_b of M rows),
 *   yhat[b][m] = fl32(sum_i a[m][i] xhat[b][i]).
 *   a [M][D] float32, row-major, contiguous, shared by the batch; any M, D >= 1 (a row need not be 16-byte aligned).
 *   t, t_b, t_r, nc: the Jacobian stack of D rows as cmf_gauss_newton_step takes it (both layouts through the two strides);
 *     k, k_b, k_r: a stack of M rows and the same nc, written whole.  Column c of k depends on column c of t alone: what the
 *     padding columns of t hold -- NaN included -- stays in the padding columns of k.  Products and sums are fp32
 *     (v_mfma_f32_16x16x4_f32); the order of accumulation along i is a function of D alone.
 *   xhat [B][D], yhat [B][M] float32, contiguous.  The sum of yhat runs in float64 in a fixed order and is rounded once.
 * Image-only mode, t == NULL: only yhat is written -- the same bits as the full mode gives; t_b, t_r, nc, k, k_b, k_r are ignored.
 * There is no info output: non-finite values propagate by IEEE rules (cmf_gauss_newton_step reports them as info 2).
 * A sample's outputs are a function of its own inputs, of a and of (M, D, nc) alone: no atomics, independent of B, of its position
 * in the batch and of the order in which workgroups finish, and they repeat bit for bit.
 * M, D, B >= 1, a, xhat, yhat not NULL; with t: k not NULL, nc % 16 == 0, 16 <= nc <= 512, the strides of t and of k >= nc and
 * % 4 == 0, t and k 16-byte aligned.  Anything else: CMF_EINVAL.  No allocation, no synchronisation.                          */
int cmf_operator_apply(const float* a, int M, int D, const float* t, long long t_b, long long t_r, int nc, int B,
                       const float* xhat, float* k, long long k_b, long long k_r, float* yhat, void* stream);
/* The same operator in DATA space, behind the fused pre-head wrapper v = [logit](wa x + wc) that cmf_prehead applies in front of the
 * head: for the recovery min_z ||y - a u(g(z))||^2 with a blur or a down-sampling a, linear in pixel values.  For a
 * head-space value v:  p = logit ? 1 / (1 + exp(-v)) : v,  u = (p - wc) / wa,  s = du/dv = (logit ? p (1 - p) : 1) / wa.
 *   yhat[b][m]  = fl32(sum_i a[m][i] u(xhat[b][i])): u in float64 from the fp32 xhat, the sum in float64 in cmf_operator_apply's
 *     order, rounded once.
 *   scale[b][i] = fl32(s(xhat[b][i])), s in float64; [B][D] float32, contiguous, caller-owned, written whole.
 *   k(b, m, c)  = sum_i a[m][i] fl32(scale[b][i] t(b, i, c)): the measured Jacobian a diag(s_b) J_b.  One fp32 multiply per element
 *     of t on its way to the MFMAs of cmf_operator_apply, which are otherwise unchanged -- the order of accumulation, the columns
 *     kept apart, what the padding columns hold (NaN times a finite s is NaN).
 * With (wa, wc, logit) = (1, 0, 0): u is xhat and s is 1.0f exactly, and k and yhat are cmf_operator_apply's, bit for bit.
 * Image-only mode, t == NULL: only yhat is written -- the same bits as the full mode gives; scale, k and the stack arguments are
 * ignored.  A sample's outputs are a function of its own inputs, of a, of the triple and of (M, D, nc) alone; no atomics.
 * Refused with CMF_EINVAL before any launch: what cmf_operator_apply refuses; wa zero or not finite; wc not finite; logit not 0 or
 * 1; with t, scale NULL or not 4-byte aligned.  No allocation, no synchronisation.                                               */
int cmf_operator_apply_wrapped(const float* a, int M, int D, const float* t, long long t_b, long long t_r, int nc, int B,
                               const float* xhat, float wa, float wc, int logit, float* scale, float* k, long long k_b,
                               long long k_r, float* yhat, void* stream);
/* The covariance of a Gauss-Newton fit carried back over the rows of the Jacobian, per sample in float64:
 *   cov = gram^-1,   lev[i] = j_i^T gram^-1 j_i  for every row j_i (the first d columns of row i of t),
 *   stats = { sum_i lev[i], max_i lev[i] }.
 *   t, t_b, t_r, n_rows, nc, d: the Jacobian stack as cmf_gauss_newton_step takes it (both layouts through the two strides);
 *     columns d .. nc - 1 are padding whose contents, NaN included, reach no output.
 *   gram [B][d][d] float32: any symmetric positive definite normal matrix in the form a step kernel consumes it -- the jtj of one
 *     cmf_gram_cholesky attempt, the gram of cmf_weighted_gauss_newton_step, or the Gram matrix of a measured stack k.  Only the
 *     lower triangle i >= j is read, nothing is written; it need not be the Gram matrix of this t.
 *   cov [B][d][d] float64, symmetric bit for bit;  lev [B][n_rows] float64, every value >= +0.0 (a sum of squares over positive
 *     pivots);  stats [B][2] float64.
 *   The elimination is that of cmf_gauss_newton_step, undamped (Cholesky in LDS, pivots only); the unit-lower factor is inverted
 *     in place and lev[i] = sum_k y_k^2 / p_k with y = L^-1 j_i.
 *   info [B] int32: 0 ok; 1 a pivot was not positive and finite (cov, lev, stats are NaN); 2 a non-finite value in the lower
 *     triangle of gram or in the first d columns of t (every output is NaN; 2 wins over 1).
 * Covariance-only mode, t == NULL: only cov and info are written -- the same bits as the full mode gives for finite t; t_b, t_r,
 *   n_rows, nc, lev and stats are ignored.
 * A sample's outputs are a function of its own inputs and of (n_rows, nc, d) alone: no atomics, independent of B, of its position
 * in the batch and of the order in which workgroups finish, and they repeat bit for bit.
 * Always: 1 <= d <= 128 (the float64 factor lives in LDS), B >= 1, gram, cov, info not NULL, cov 8-byte aligned; with t: lev,
 * stats not NULL and 8-byte aligned, n_rows >= 1, nc % 16 == 0, d <= nc, t_b and t_r >= nc and % 4 == 0, t 16-byte aligned.
 * Anything else: CMF_EINVAL before any launch.  No allocation, no synchronisation.                                           */
int cmf_tangent_leverage(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B, const float* gram,
                         double* cov, double* lev, double* stats, int* info, void* stream);
/* One damped Gauss-Newton step on whole discretised curves with fixed end points.  A curve has `points` = P >= 3
 * points, N = P - 1 segments and M = P - 2 interior points; samples are curve-major: point i of curve c is sample c P + i of the
 * Jacobian stack t, of jtj and of xhat.  With r_i = xhat_{i+1} - xhat_i:
 *   g_i = J_i^T (xhat_{i-1} + xhat_{i+1} - 2 xhat_i),  H block tridiagonal with H_ii = 2 J_i^T J_i, H_{i,i+1} = -C_i,
 *   C_i = J_i^T J_{i+1},  A = H + damping[c] diag(H),  delta = A^-1 g  over the interior points i = 1 .. M.
 *
 * cmf_cross_gram: cross [curves][P - 3][d][d] float32, cross[c][i - 1][a][b] = sum_r J_{c,i}[r][a] J_{c,i+1}[r][b] for i = 1 ..
 * P - 3, the whole (unsymmetric) block, by fp32 MFMA with fp32 accumulation.  With P == 3 nothing is written and cross may be
 * NULL.  t, t_b, t_r, n_rows, nc as cmf_gram_cholesky takes them, nc <= 128; columns d .. nc - 1 are padding whose contents
 * influence no output.  The order of every sum is a function of (n_rows, nc, d) alone -- not of the column's position, of the
 * pair, of `curves` or of completion order: two bit-identical columns of J give bit-identical rows of cross.  A non-finite input
 * reaches its own pair's block only.
 *
 * cmf_curve_step, per curve in float64:
 *   jtj [curves P][d][d] float32 as ONE cmf_gram_cholesky attempt leaves it: the lower triangles of the interior points are read,
 *     nothing is written; cross as above; xhat [curves P][n_rows] float32; damping [curves] float64, >= 0.
 *   seg2 [curves][N] = ||r_i||^2;  grad, delta [curves][M][d];
 *   stats [curves][4] = { sum_i ||r_i||^2, g^T delta, delta^T H delta, max |g| };
 *   info [curves] int32: 0 ok; 1 a pivot of A was not positive and finite (delta, stats[1], stats[2] are NaN, the rest is valid);
 *     2 a non-finite value in xhat, in the first d columns of an interior point's t or in the parts of jtj / cross that are read
 *     (every output of the curve is NaN).
 *   ws: caller-owned, 8-byte aligned, ws_doubles >= cmf_curve_step_ws(d, points, curves) doubles (CMF_EINVAL for arguments out of
 *     range): the eliminated columns of every block and, for 64 < d, the elimination window, one slice per curve.
 * Energy-only mode, t == NULL: only seg2, stats[c][0] and info[c] (0 or 2) are written -- the same bits as the full mode gives;
 * the Jacobian arguments, jtj, cross, damping, grad, delta and ws are not looked at.
 * A curve's outputs are a function of its own inputs and of (n_rows, nc, d, P) alone: no atomics, independent of `curves`, of the
 * curve's position and of completion order, and they repeat bit for bit.
 * 1 <= d <= 128, nc % 16 == 0, d <= nc, t_b and t_r >= nc and % 4 == 0, t 16-byte aligned, float64 pointers 8-byte aligned,
 * n_rows, curves >= 1.  Anything else: CMF_EINVAL.  No allocation, no synchronisation.                                        */
int cmf_cross_gram(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int points, int curves, float* cross,
                   void* stream);
long long cmf_curve_step_ws(int d, int points, int curves);
int cmf_curve_step(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int points, int curves,
                   const float* jtj, const float* cross, const float* xhat, const double* damping, double* grad, double* delta,
                   double* stats, double* seg2, int* info, double* ws, long long ws_doubles, void* stream);
/* The per-sample float64 step of geodesic shooting, on the metric G = J^T J of one sample:
 *   apply == 0 (solve):  out = G^-1 rhs  (Cholesky of G in LDS, pivots only: the elimination of cmf_gauss_newton_step, undamped);
 *   apply == 1:          out = G rhs, the symmetric product from the lower triangle.
 *   jtj [B][d][d] float32: the Gram matrix as one cmf_gram_cholesky attempt leaves it; only the lower triangle i >= j is read,
 *     nothing is written.  rhs [B][d] float64.
 *   out64 [B][d] float64;  out32 [B][d] float32, out64 rounded to nearest;
 *   stats [B][2] float64 = { rhs^T out, max_k |out_k| };
 *   info [B] int32: 0 ok; 1 (solve only) a pivot of G was not positive and finite (out64, out32 and stats are NaN); 2 a non-finite
 *     value in the lower triangle of jtj or in rhs (every output is NaN).
 * A sample's outputs are a function of its own inputs and of d alone: no atomics, independent of B, of its position in the batch
 * and of the order in which workgroups finish, and they repeat bit for bit.
 * 1 <= d <= 128 (the float64 matrix lives in LDS), B >= 1, apply 0 or 1, float64 pointers 8-byte aligned, the others 4-byte.
 * Anything else: CMF_EINVAL.  No allocation, no synchronisation.                                                               */
int cmf_metric_solve(const float* jtj, const double* rhs, int d, int B, int apply, double* out64, float* out32, double* stats,
                     int* info, void* stream);
/* Parallel transport of m latent tangent vectors along discretised curves.  A curve has `points` = P >= 2 points and
 * N = P - 1 segments; samples are curve-major: point i of curve c is sample c P + i.  With G_i = J_i^T J_i and C_i = J_i^T J_{i+1},
 * per curve and per vector in float64 (no contraction), segment by segment:
 *   fwd_i = G_{i+1}^-1 (C_i^T w_i)   (Cholesky of G_{i+1} in LDS, pivots only: the elimination of cmf_metric_solve);
 *   bwd_i = C_i^-1 (G_i w_i)         (Gaussian elimination with partial pivoting: the pivot of a column is its largest |entry|, the
 *                                     lowest row among equals; multipliers by division);
 *   w_{i+1} = 0.5 (fwd_i + bwd_i);   norm2_i = w_i^T G_i w_i = sum_r w_r (sum_j G_rj w_j), j and r ascending.
 *   jtj [curves P][d][d] float32 as ONE cmf_gram_cholesky attempt leaves it: the lower triangles are read, nothing is written.
 *   cross [curves P - 1][d][d] float32: block s = J_s^T J_{s+1} over the sample stack, the whole (unsymmetric) block; the blocks
 *     s = c P - 1 straddle two curves and are never read.  w0 [curves][m][d] float64.
 *   out [curves][P][m][d] float64, out[c][0] = w0[c];  fwd, bwd [curves][N][m][d];  norm2 [curves][P][m].
 *   info [curves] int32: 0 ok; 1 a pivot of some G_{i+1} was not positive and finite or a pivot of some C_i was zero or not finite
 *     (fwd and bwd of segment i and of the later segments, out and norm2 from point i + 1 on are NaN; everything before keeps the
 *     bits it would have had); 2 a non-finite value in w0 or in a part of jtj / cross that is read (every output of the curve is
 *     NaN; takes precedence over 1).
 * A curve's outputs are a function of its own inputs and of (d, m, P) alone: no atomics, independent of `curves`, of the curve's
 * position and of completion order, and they repeat bit for bit.
 * 1 <= d <= 128, 1 <= m <= 16 (the float64 window lives in LDS), P >= 2, curves >= 1, no pointer NULL, float64 pointers 8-byte
 * aligned, the others 4-byte.  Anything else: CMF_EINVAL.  No allocation, no synchronisation.                                  */
int cmf_transport_chain(const float* jtj, const float* cross, const double* w0, int d, int m, int points, int curves, double* out,
                        double* fwd, double* bwd, double* norm2, int* info, void* stream);
/* One damped Gauss-Newton step on whole stars: `arms` = K discretised curves of `points` = P >= 3 points that share one free end
 * point, the centre.  The stack is star-major, then arm-major: point i of arm k of star s is sample q = (s K + k) P + i
 * of jtj and xhat and sample first + q of the Jacobian stack t (first >= 0: a sweep padded in front needs no copy).  Point 0 is the
 * arm's fixed end, point N = P - 1 the arm's own copy of the centre, M = P - 2 interior points.  Per arm, unweighted:
 *   g_i = J_i^T (xhat_{i-1} + xhat_{i+1} - 2 xhat_i), i = 1 .. M;  g^c_k = J_N^T (xhat_M - xhat_N);
 *   H_ii = 2 J_i^T J_i, H_{i,i+1} = -C_i = -J_i^T J_{i+1} for i = 1 .. M, centre contribution J_N^T J_N.
 * The star is sum_k weights[s][k] (that of arm k), A = H + damping[s] diag(H), delta = A^-1 g, in float64.
 *   jtj [stars K P][d][d] float32 as ONE cmf_gram_cholesky attempt leaves it: the lower triangles of the points 1 .. N are read;
 *   cross [stars K P - 1][d][d] float32: block q = J_q^T J_{q+1} of neighbouring samples of the stack, as cmf_cross_gram gives them
 *     for a stack padded by one sample at each end (the blocks that straddle two arms and those of the points 0 are not read);
 *   xhat [stars K P][n_rows] float32; weights [stars][K] float64, finite and > 0; damping [stars] float64, >= 0.
 *   grad [stars][K][M][d] = weights_k g_{k,i};  grad_centre [stars][d] = sum_k weights_k g^c_k, summed in arm order;
 *   delta [stars][K][M][d];  delta_centre [stars][d];  seg2 [stars][K][N] = ||r_i||^2, the bits of cmf_curve_step's on the arm;
 *   arm_stats [stars][K][4] = { sum_i ||r_i||^2, g_k^T delta_k, delta^T H_k delta, max_i |g_{k,i}| } of the unweighted arm, the
 *     two forms with the arm's centre terms g^c_k^T delta_centre and delta_centre^T J_N^T J_N delta_centre; the maximum is over the
 *     interior points;
 *   info [stars] int32: 0 ok; 1 a pivot of some arm or of the centre was not positive and finite (delta, delta_centre and the two
 *     forms of every arm are NaN, the rest is valid); 2 a non-finite value in what is read, or a weight that is not finite and > 0
 *     (every output of the star is NaN; takes precedence over 1).  Other stars are unaffected.
 *   ws: caller-owned, 8-byte aligned, ws_doubles >= cmf_star_step_ws(d, points, arms, stars) doubles (CMF_EINVAL for arguments out
 *     of range): per arm its Schur contribution to the centre block, the eliminated columns of every block and, for 64 < d, the
 *     elimination window.
 * Three launches: per arm forward, per star the centre, per arm backward.  A star's outputs are a function of its own inputs and
 * of (n_rows, nc, d, P, K) alone: no atomics, independent of `stars`, of the star's position and of completion order, and they
 * repeat bit for bit.
 * 1 <= d <= 128, 1 <= arms <= 64, nc % 16 == 0, d <= nc, t_b and t_r >= nc and % 4 == 0, t 16-byte aligned, float64 pointers 8-byte
 * aligned, the others 4-byte, no pointer NULL, n_rows, stars >= 1.  Anything else: CMF_EINVAL.  No allocation, no synchronisation. */
long long cmf_star_step_ws(int d, int points, int arms, int stars);
int cmf_star_step(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int points, int arms, int stars,
                  long long first, const float* jtj, const float* cross, const float* xhat, const double* weights,
                  const double* damping, double* grad, double* grad_centre, double* delta, double* delta_centre, double* arm_stats,
                  double* seg2, int* info, double* ws, long long ws_doubles, void* stream);
/* Principal geodesic analysis of groups of `arms` = K tangent vectors at one point each: PCA in the tangent plane in the
 * pull-back metric G = J^T J, in its dual (K x K) form, per group in float64 (no contraction), one workgroup per group.
 *   jtj [B][d][d] float32: the Gram matrix as ONE cmf_gram_cholesky attempt leaves it; only the lower triangle i >= j is read,
 *     nothing is written.  vectors [B][K][d] float64: the latent components v_k.  weights [B][K] float64, finite and > 0.
 * With W = sum_k w_k (arm order), y_k = G v_k (j ascending) and q_kl = sum_i y_k[i] v_l[i] (i ascending):
 *   M_kl = M_lk = ((sqrt(w_k) sqrt(w_l)) q_kl) / W for l <= k;  M = P Lambda P^T by the cyclic Jacobi method of cmf_gram_spectrum
 *   (the same ordering, rotation rule and stop, CMF_SPECTRUM_MAX_SWEEPS);  lambda descending (equal values in descending order of
 *   their position on the converged diagonal);  rank = #{ j : lambda_j > (d 2^-24) lambda_1 }.
 *   variances [B][r] float64, r = `components`: lambda_0 .. lambda_{r-1}, as computed (zero and negative values included).
 *   directions [B][r][d] float64: for j < rank u_j = (sum_k (sqrt(w_k) p_kj) v_k) / sqrt(W lambda_j), k ascending: G-orthonormal;
 *     the component of largest magnitude is positive (lowest index on ties).  For j >= rank: 0.  The slice of a group is also its
 *     workgroup's working storage during the launch, like covectors.
 *   scores [B][K][r] float64: for j < rank (sqrt(W lambda_j) p_kj) / sqrt(w_k) = u_j^T G v_k, with the sign of u_j.  Else 0.
 *   covectors [B][K][d] float64 = y_k;  norm2 [B][K] float64 = q_kk = v_k^T G v_k;  total [B] float64 = (sum_k w_k q_kk) / W.
 *   rank, sweeps [B] int32 (sweeps: those executed, the final rotation-free one included);
 *   info [B] int32: 0 ok; 1 sweep cap reached; 2 a non-finite value in the lower triangle of jtj or in vectors, or a weight that is
 *     not finite and > 0 (every float64 output of the group is NaN, rank and sweeps 0).  Other groups are unaffected.
 * A group's outputs are a function of its own inputs and of (d, K, r) alone: no atomics, independent of B, of the group's position
 * and of completion order, and they repeat bit for bit.
 * 1 <= d <= 128, 1 <= arms <= 64, 1 <= components <= arms, B >= 1, no pointer NULL, float64 pointers 8-byte aligned, the others
 * 4-byte.  Anything else: CMF_EINVAL, nothing is written.  No allocation, no synchronisation.                                   */
int cmf_tangent_pca(const float* jtj, const double* vectors, const double* weights, int d, int arms, int components, int B,
                    double* variances, double* directions, double* scores, double* covectors, double* norm2, double* total,
                    int* rank, int* sweeps, int* info, void* stream);
/* The second fundamental form of the manifold in a latent frame: per sample, in float64 (no contraction), from the centre
 * sweep's Jacobian stack, its metric, a frame of m unit latent directions u_0 .. u_{m-1}, the step h and a sweep at the 2 m shifted
 * latents z +- h u_a.  q = m (m + 1) / 2 pairs p = (a, b), a <= b, in a-major order.
 *   t, t_b, t_r, n_rows, nc: the centre stack as cmf_gram_cholesky takes it (both layouts through the two strides); columns d .. nc - 1
 *     are padding whose contents influence no output.
 *   jtj [B][d][d] float32: the Gram matrix as ONE cmf_gram_cholesky attempt leaves it; only the lower triangle i >= j is read,
 *     nothing is written.
 *   s, s_b, s_r: the shifted stack of 2 m B samples of n_rows rows and 16 columns; sample (b m + a) 2 + sign (sign 0: + h u_a, 1:
 *     - h u_a) begins at s + ((b m + a) 2 + sign) s_b, its row r at + r s_r; column c < m holds J(z_b +- h u_a) u_c, columns m .. 15 are
 *     padding whose contents influence no output.
 *   frame [B][m][d] float64;  step [B] float64, h > 0.
 * With delta_ab[r] = s(+a)[r][b] - s(-a)[r][b], D_ab = delta_ab / (2 h), H_p = (delta_ab + delta_ba) / (4 h), A = J^T H, S2 = H^T H:
 *   second_gram [B][q][q] = S2 - A^T G^-1 A, whole and mirrored: the Gram matrix of the normal components of the H_p;
 *   christoffel [B][q][d] = G^-1 A_p;  frame_metric [B][m][m] = u_a^T G u_b (j, then r ascending; the lower triangle mirrored);
 *   stats [B][4] = { sum_{a<b} ||D_ab - D_ba||^2, sum_{a<b} ||H_ab||^2, trace S2, trace second_gram };
 *   info [B] int32: 0 ok; 1 a pivot of G was not positive and finite (second_gram, christoffel and stats[3] are NaN, the rest is
 *     valid); 2 a non-finite value in the first d columns of t, the first m columns of s, the lower triangle of jtj or in frame, or a
 *     step that is not finite and > 0 (every float64 output of the sample is NaN; found before anything is written: takes precedence
 *     over 1).  Other samples are unaffected.
 * The sums over the rows run over the raw differences; each folded sum is divided once by 4 h, (4 h)^2 or (2 h)^2.
 * A sample's outputs are a function of its own inputs and of (n_rows, nc, d, m) alone: no atomics, independent of B, of its position
 * in the batch and of completion order, and they repeat bit for bit.
 * 1 <= d <= 128, 1 <= m <= min(d, 4), nc % 16 == 0, d <= nc, t_b and t_r >= nc, s_b and s_r >= 16, all four % 4 == 0, t and s 16-byte
 * aligned, float64 pointers 8-byte aligned, the others 4-byte, no pointer NULL, n_rows, B >= 1.  Anything else: CMF_EINVAL, nothing is
 * written.  No allocation, no synchronisation.                                                                                       */
int cmf_second_form(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int m, int B, const float* jtj,
                    const float* s, long long s_b, long long s_r, const double* frame, const double* step, double* second_gram,
                    double* christoffel, double* frame_metric, double* stats, int* info, void* stream);
/* Reverse of the head above for training (autograd through non_square.py:307-308, :280-294, :87-100):
 *   dt(b, r, :) = 2 * t(b, r, :) * (g_logdet[b] * jtj_b^-1 + g_l1off[b] * sign(jtj_b)[i != j]
 *                                   + g_l1diag[b] * sign(jtj_b)[i == j])
 * jtj is the matrix cmf_gram_cholesky / cmf_cholesky_retry left behind; g_* are [B] or NULL (= 0);
 * dt has nc columns per row like t (columns >= d are written as 0) and may not alias t.            */
int cmf_gram_backward(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B,
                      const float* jtj, const float* g_logdet, const float* g_l1off, const float* g_l1diag,
                      float* dt, long long dt_b, long long dt_r, void* stream);
/* The same for any width nc <= 512 with a caller-owned workspace ws of 2 * B * d * d floats (G^-1 for 128 < nc comes from a
 * Cholesky factorisation of jtj in ws, and the d x d cotangent lives beside it).  nc <= 128 runs cmf_gram_backward (ws unused);
 * cmf_gram_backward itself keeps nc <= 128.  No allocation, no synchronisation.                                              */
int cmf_gram_backward_ws(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B,
                         const float* jtj, const float* g_logdet, const float* g_l1off, const float* g_l1diag,
                         float* dt, long long dt_b, long long dt_r, float* ws, void* stream);
/* The same product for an EXPLICIT cotangent m [B][d][d] of the Gram matrix (not necessarily symmetric), any nc <= 512:
 * dt = t (m + m^T).  Training on the Hutchinson surrogate (non_square.py:203-258): m = mean_s u_s eps_s^T, u detached.   */
int cmf_gram_backward_matrix(const float* t, long long t_b, long long t_r, int n_rows, int nc, int d, int B,
                             const float* m, float* dt, long long dt_b, long long dt_r, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Small per-sample reductions / elementwise maps.                                                 */
/* pre-head chain (wrapper.py:28-30, math.py:41-105): y = a*(x + u) + c; if logit: y = log(y)-log(1-y) and
 * lj[b] = n*log|a| + sum(-log(yc) - log(1-yc)), yc = clamp(a*(x+u)+c, 1e-7, 1-1e-7).  u may be NULL.     */
int cmf_prehead(const float* x, const float* u, float* y, float* lj, float a, float c, int logit, int n,
                int B, void* stream);
/* inverse of the pre-head chain for sampling (math.py:45-46, :83-84, :100-101): x = (sigmoid(y) - c) / a */
int cmf_prehead_inverse(const float* y, float* x, float a, float c, int logit, long long n_total, void* stream);
/* lp[b] += -n/2 log(2 pi) - 1/2 sum z^2      (gaussian.py:9-22 with mean 0, stddev 1)              */
int cmf_gaussian_logprob(const float* z, long long z_b, int n, int B, float* lp, void* stream);
/* 2-D prior AffineBijection (affine.py:24-34): encode u = z*exp(ls)+sh, lj[b] += sum ls; decode inverse */
int cmf_affine_prior(float* z, long long z_b, const float* log_scale, const float* shift, int n, int B,
                     int decode, float* lj, void* stream);
/* rec[b] = sum_r (xh(b,r) - x(b,r))^2        (non_square.py:111-114)                               */
int cmf_recon_sqerr(const float* xh, const float* x, int n, int B, float* rec, void* stream);
/* elbo[b] = wl*(low[b] - logdet[b]/2) - lam*rec[b] - wm*l1[b] + pre[b]; NULL inputs count as 0
 * (non_square.py:85, :126-129 and exact.py:27 for the pre-head log-jacobians)                      */
int cmf_elbo_combine(const float* low, const float* logdet, const float* rec, const float* l1, const float* pre,
                     float wl, float lam, float wm, int B, float* elbo, void* stream);
/* Hutchinson log-det surrogate (non_square.py:203-258) against the EXPLICIT Gram matrix produced by
 * cmf_gram_cholesky (see hutch_cg.hip for why the explicit form is the cheaper one on this hardware):
 *   w(b,:,s) = G(b) eps(b,:,s);  u = CG(G, eps) with x0 = 0, unit-normalised right-hand sides, at least
 *   min_iter and at most max_iter iterations, stopping a sample when the mean over its S probes of the
 *   relative residual 2-norm drops below tol;  val[b] = mean_s sum_k u*w.   eps, u, w: [B][d][S]; S <= 512
 *   (probes beyond 16 run in chunks of 16 with the stopping rule applied per chunk; iters[b] = the slowest chunk).
 * d, S <= 512; d > 128 or S > 128 runs the kernel of head_wide.hip, which reads jtj as a SYMMETRIC matrix (as cmf_gram_cholesky
 * writes it).  The reference's solver (gpytorch linear_cg @ fc2053b) is un-vendored: CG iterates are parity-unpinned. */
int cmf_hutch_cg(const float* jtj, const float* eps, int d, int S, int B, int max_iter, int min_iter, float tol,
                 float* u, float* w, float* val, int* iters, void* stream);
/* Metric term on the Hutchinson product W = (J^T J) eps, [B][d][S] with S == d -- the third return value of
 * non_square.py:253-258 fed to :87-100:  l1_diag[b] = sum_k |W_kk|,  l1_off[b] = sum_{i != j} |W_ij|
 * (the reference's masked_select(~eye).view(B, d(d-1)) exists only for S == d: l1_off must be NULL otherwise; the diagonal branch,
 * torch.diagonal of the (B, d, S) product at :87-92, is valid for any S and sums min(d, S) entries).  Either output may be NULL. */
/* d, S <= 512 here and in the two cotangent entry points below. */
int cmf_hutch_metric(const float* w, int d, int S, int B, float* l1_off, float* l1_diag, void* stream);
/* Cotangent of the Gram matrix for the train-mode Hutchinson objective, u detached (non_square.py:236-247):
 *   M(b) = g_val[b]/S sum_s u_s eps_s^T + sum_s (g_off[b] [i != s] + g_diag[b] [i == s]) sign(W_is) e_i eps_s^T,
 * [B][d][d]; feed it to cmf_gram_backward_matrix (dJ = J (M + M^T)).  g_val / g_off / g_diag: [B] or NULL; the metric
 * terms need w; g_off needs S == d. */
int cmf_hutch_cotangent(const float* u, const float* eps, const float* w, int d, int S, int B, const float* g_val,
                        const float* g_off, const float* g_diag, float* M, void* stream);
/* Low-rank form of the same cotangent for S << d (non_square.py:241-256 builds its graph only through J^T J eps for the S
 * probes): with V = [u_1..u_S | eps_1..eps_S | e_0..e_{K-1}] (K = min(d, S) when g_diag is given, else 0; n = 2S + K columns) and
 * P = J V from ONE n-column tangent sweep, the objective is a sum of inner products of columns of P and its cotangent with
 * respect to P^T P is  cmat[b][s][S+s] = g_val[b]/S,  cmat[b][2S+k][S+k] = g_diag[b] sign(W_kk)  ([B][n][n], zero elsewhere);
 * cmf_gram_backward_matrix(P, cmat) then yields the cotangent of P.  w [B][d][S] is read only with g_diag. */
int cmf_hutch_lowrank_cotangent(const float* w, int d, int S, int B, const float* g_val, const float* g_diag, int n,
                                float* cmat, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused affine-coupling layer with an MLP coupler (2-D / tabular models, low-dimensional prior flows): the whole coupler
 * network (get_mlp, networks.py:206-224; tanh rule jvp_layers.py:38-53) for the primal and all Jacobian columns, and the
 * coupling update (acl.py:101-146), in one persistent launch -- replaces the per-layer cmf_conv_primal / cmf_conv_tangent
 * launches + cmf_acl_tangent + cmf_acl_primal of one coupling layer.  See csrc/mlp_coupler.hip.
 *   t != NULL  TANGENT mode (decode only): tangents feature-major with 16 column slots of which the first `ncols` <= 15 are
 *              Jacobian columns (the rest zero padding): z and the modified rows of t are updated in place exactly as
 *              cmf_acl_primal(decode) + cmf_acl_tangent would.
 *   t == NULL  PRIMAL mode: z updated in place (decode != 0: x = z e^{-s} - t; else z = (x + t) e^{s});
 *              lj[b] += -/+ sum s when lj != NULL.
 * Limits: hidden widths <= 128, 2 cin <= 256, network outputs <= 64, 2 .. CMF_MLP_MAX_LAYERS linear layers.               */
#define CMF_MLP_MAX_LAYERS 8
typedef struct {
  float* z; long long z_b;            /* primal (B, D): element (b, f) at z + b*z_b + f                                   */
  float* t; long long t_f;            /* tangents (D, B, 16): element (f, b, col) at t + f*t_f + b*16 + col; or NULL      */
  const float* w;                     /* layer images (cmf_pack_mlp_layer), layer l at w + w_off[l]; 16-byte aligned      */
  const int* zi; const int* si; const int* ti; int n_mod;   /* coupling maps as for cmf_acl_primal                          */
  int B, cin, chan_off, chan_step;    /* the network reads z[b][chan_off + f*chan_step], f < cin                          */
  int n_layers;                       /* linear layers: tanh after every one but the last                                */
  int width[CMF_MLP_MAX_LAYERS + 1];  /* width[0] = cin, width[l + 1] = output features of layer l                        */
  long long w_off[CMF_MLP_MAX_LAYERS];
  int decode;
  float* lj;
  int ncols;                          /* TANGENT mode: Jacobian columns in use (1 .. 15)                                  */
} cmf_mlp_coupler_args;
int cmf_mlp_coupler(const cmf_mlp_coupler_args* a, void* stream);
/* Layer image for cmf_mlp_coupler from nn.Linear parameters w [out][in], bias [out] (NULL = zeros): MFMA A fragments in the
 * order the kernel's K-steps consume them (first != 0: the layer that reads the gathered input rows) + bias, zero-padded to
 * out_tiles x 16 outputs and in_groups x 16 inputs.  The kernel expects: hidden layers out_tiles = HT, later layers
 * in_groups = HT with HT = cmf_mlp_hidden_tiles(widest hidden layer); first layer in_groups = ceil(cin / 16); last layer
 * out_tiles = ceil(outputs / 16).  Size query: out == NULL returns the number of floats through *out_floats.            */
int cmf_pack_mlp_layer(const float* w, const float* bias, int out_features, int in_features, int first, int out_tiles,
                       int in_groups, float* out, long long* out_floats, void* stream);
int cmf_mlp_hidden_tiles(int max_hidden_width);

/* ---------------------------------------------------------------------------------------------
 * NSF prior of the low-dimensional flow (config/schemas.py:87-103 -> bijections/nsf.py:86-113,
 * bijections/linear.py:12-34).  The arithmetic is jrmcornish/nsf @ 8e3fe75 (un-vendored: PARITY UNPINNED); implemented
 * from Durkan et al., "Neural Spline Flows" (NeurIPS 2019) -- see csrc/nsf.hip.
 * Elementwise monotone rational-quadratic spline with linear tails outside [-tail_bound, tail_bound]:
 *   params [B][D][3 bins - 1] (bins widths, bins heights -- both divided by sqrt(hidden) as the autoregressive transform
 *   does --, bins - 1 inner knot derivatives); out(b, f) = spline(x(b, f)) (inverse != 0: the inverse map);
 *   lj[b] += sum_f log |d out / d x| (NULL to skip).  out may alias x.                                                */
int cmf_rq_spline(const float* x, long long x_b, const float* params, int D, int bins, int hidden, float tail_bound,
                  int inverse, int B, float* out, long long out_b, float* lj, void* stream);
/* Training: cotangents of x and of the spline parameters from dz (B, D) and dlj (B,) (NULL = 0):
 *   dx(b,f) = dz dz/dx + dlj[b] d log|dz/dx| / dx;   dparams [B][D][3 bins - 1] likewise per parameter.  Forward direction only. */
int cmf_rq_spline_backward(const float* x, long long x_b, const float* params, int D, int bins, int hidden, float tail_bound,
                           int B, const float* dz, long long dz_b, const float* dlj, float* dx, long long dx_b,
                           float* dparams, void* stream);
/* LULinear backward from dW [n][n] = sum_b dy (x) x: gradients of the strict triangles and of the unconstrained diagonal
 * (accumulated), including the log-jac term sum_b dlj[b] * d(sum log diag U) (dlj: (B,) or NULL; scratch1: 1 float).      */
int cmf_lu_backward(const float* dW, const float* lower, const float* upper, const float* unconstrained_diag, int n, float eps,
                    const float* dlj, int B, float* scratch1, float* g_lower, float* g_upper, float* g_udiag, void* stream);
/* du(b, f) = -dlow[b] u(b, f): backward of the standard-normal log-density (gaussian.py:9-22)                           */
int cmf_gaussian_backward(const float* u, const float* dlow, int n, int B, float* du, void* stream);
/* LULinear: W [n][n] = L U (L unit lower from `lower`, U upper from `upper` with diagonal softplus(unconstrained_diag) +
 * eps; entry order of np.tril_indices(n, -1) / np.triu_indices(n, 1)); logdet[0] = sum log diag(U).                   */
int cmf_lu_weights(const float* lower, const float* upper, const float* unconstrained_diag, int n, float eps, float* W,
                   float* logdet, void* stream);
/* out [n_out][n_in] = w * MADE mask (random_mask = False).  kind 0: input -> hidden, 1: hidden -> hidden, 2: hidden ->
 * output with `multiplier` consecutive outputs per feature (strict inequality).  features = autoregressive width D.    */
int cmf_made_mask_weight(const float* w, float* out, int n_out, int n_in, int kind, int features, int multiplier,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Non-convolution pieces of the coupler networks' primal backward.
 * ScaledTanh2dModule (networks.py:96-113), y = sw tanh(u) + sb, g = sw (1 - tanh(u)^2); y, g, dy, dg, du: (B, C, HW):
 *   du = dy g - 2 dg tanh(u) g;   dsw[c] += sum dy tanh(u) + dg (1 - tanh(u)^2);   dsb[c] += sum dy
 * dg (cotangent of g, from cmf_acl_cross_terms) may be NULL; dsw / dsb may be NULL.                                */
int cmf_stanh_backward(const float* dy, const float* dg, const float* y, const float* g, const float* sw,
                       const float* sb, float* du, float* dsw, float* dsb, int B, int C, int HW, void* stream);
/* Second-order term of the tanh MLP couplers' tangent pass (get_linear_jvp + the tanh rule, jvp_layers.py:38-53): layer i+1
 * reads phi_i = 1 - h_i^2 of the primal activation h (B, F).  c holds the UNMASKED cotangent W_{i+1}^T c_{i+1} of the rows
 * (element (b, f, col) at c + b*c_b + f*c_r + col), x the saved raw tangent of the same rows:
 *     c <- phi c  (in place: the cotangent of layer i's raw output);   dh[b][f] += -2 h sum_col c_old x                    */
int cmf_tanh_cross_terms(float* c, long long c_b, long long c_r, const float* x, long long x_b, long long x_r,
                         const float* h, float* dh, int F, int B, int nc, void* stream);
/* MLP coupler primal backward, elementwise stage (networks.py:206-224): out = (dh + extra) (1 - a^2) over n floats, a = the
 * tanh output, extra (or NULL) = the tangent pass's second-order term (cmf_tanh_cross_terms).  out may alias dh.          */
int cmf_tanh_backward(const float* dh, const float* a, const float* extra, long long n, float* out, void* stream);
/* AffineBijection backward (affine.py:24-34): g_ls[f] += sum_b dz x e^{ls} + sum_b dlj[b] (dlj may be NULL), g_sh[f] += sum_b dz,
 * dz <- dz e^{ls} in place; dz, x: (B, n) with row strides dz_b, x_b.                                                     */
int cmf_affine_prior_backward(float* dz, long long dz_b, const float* x, long long x_b, const float* log_scale, int n, int B,
                              const float* dlj, float* g_ls, float* g_sh, void* stream);
/* dst[i] += src[i]: the skip connection of the reverse sweep next to the split-precision kernel (16-byte accesses when n % 4 == 0
 * and both pointers are 16-byte aligned, a scalar sweep otherwise: odd-sized gradient tensors). */
int cmf_accumulate(float* dst, const float* src, long long n, void* stream);
/* relu' bit mask of an activation tensor act (B, C, HW), C % 8 == 0, in the CMF_F_RELU_BITS layout: out[B][HW][C/8] bytes,
 * bit j of byte (b, px, o) = [act(b, 8 o + j, px) > 0].                                                                  */
int cmf_relu_bits(const float* act, void* out, int B, int C, int HW, void* stream);
/* out[c] += sum_{n, px, col} t(n, c, px, col) over a tangent-layout tensor (element at n*t_np + c*t_c + px*t_px +
 * (col/16)*t_sl + col%16, t_sl = 0 meaning 16): the bias gradient of nn.Conv2d / nn.Linear.                        */
int cmf_channel_sum(const float* t, long long t_np, long long t_c, long long t_px, long long t_sl, int np, int C,
                    int npx, int nc, float* out, void* stream);
/* n <= CMF_WGRAD_MAX_BATCH tensors of ONE shape in one launch (t, out: HOST arrays of device pointers): out[k][c] += the sums of t[k]. */
int cmf_channel_sum_batched(const float* const* t, float* const* out, int n, long long t_np, long long t_c, long long t_px,
                            long long t_sl, int np, int C, int npx, int nc, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused optimiser step over one flat fp32 buffer: replaces the per-parameter loop of
 * torch.optim.{SGD, Adam, Adamax}(params, lr, weight_decay).step() (experiment.py:515-534) and
 * torch.nn.utils.clip_grad_norm_ (trainer.py:218-219).  `step` counts from 1.                      */
#define CMF_OPT_SGD 0
#define CMF_OPT_ADAM 1
#define CMF_OPT_ADAMAX 2
/* out[0] = sum g^2 (deterministic two-level reduction); ws: 1024 floats of caller-owned workspace   */
int cmf_grad_sqnorm(const float* g, long long n, float* ws, float* out, void* stream);
/* p, g, m, v: n floats each, 16-byte aligned (m, v unused for SGD).  sqnorm != NULL: the gradient is first
 * scaled IN PLACE by min(1, max_norm / (sqrt(sqnorm[0]) + 1e-6)) -- read on the device, no host sync.
 * Hyper-parameters are doubles: torch rounds 1 - beta and lr / (1 - beta^t) to fp32 only after forming them.  */
int cmf_optimizer_step(int kind, float* p, float* g, float* m, float* v, long long n, double lr, double beta1,
                       double beta2, double eps, double weight_decay, int step, const float* sqnorm, float max_norm,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CMF_AMD_H */
