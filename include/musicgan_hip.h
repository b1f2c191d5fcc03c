/*
 * musicgan_hip.h -- C ABI of libmusicgan_hip.so, the MI355X (gfx950) kernels behind the MusicGAN hot path.
 *
 * The reference (Ipsedo/MusicGAN) has no FFI/plugin layer: its hot path is stock torch.nn modules
 * (music_gan/networks/) and torchaudio/torch.stft calls (music_gan/audio/functions.py).  Each entry point below
 * names the reference module/ATen op it replaces (file:line relative to /root/reference/music_gan).  A maintainer binds
 * these with ctypes; musicgan_amd/_lib.py is that binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32, NCHW contiguous, 16-byte aligned (torch allocations are);
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); every call is asynchronous on it;
 *   - functions return 0 on success, a negative MG_E* code otherwise, never throw; mg_last_error() gives the text of the
 *     calling thread's last failure; no hidden global state apart from one-time kernel attribute set-up;
 *   - callable concurrently from several host threads on distinct streams (autograd backward threads do).
 */
#ifndef MUSICGAN_HIP_H
#define MUSICGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mg_stream_t;

#define MG_OK 0
#define MG_EINVAL (-1)  /* bad shape / flag combination */
#define MG_ELAUNCH (-2) /* hip launch error */
#define MG_EWORKSPACE (-3)
#define MG_EIO (-4)      /* a host file operation failed (mg_pt_write_samples): errno text in mg_last_error() */

int mg_version(void);
const char* mg_last_error(void);

/* ------------------------------------------------------------------ 3x3 convolution, stride 1, pad 1
 * Replaces nn.Conv2d(k=3,s=1,p=1) [generator.py:16-22,31-37; discriminator.py:15-21,26-32] fused with what follows it:
 * LeakyReLU(0.2) [generator.py:23,38; discriminator.py:22,33], PixelNorm [layers.py:11-17], and with what precedes it
 * in the generator, nn.Upsample(x2, nearest) [generator.py:26-29].  The same kernel evaluates the data gradient
 * (aten::convolution_backward, input grad) when given weights packed with dgrad=1.
 */
#define MG_CONV_UPS_IN 1   /* logical input = nearest-upsample x2 of x (x is N,Cin,H/2,W/2) */
#define MG_CONV_LRELU 2    /* y = leaky_relu(acc + bias, slope) */
#define MG_CONV_MASK_AUX 4 /* y = acc * (aux > 0 ? 1 : slope): LeakyReLU backward fused on the output (aux: N,Cout,H,W) */
#define MG_CONV_PIXNORM 8  /* also emit p = y * rn and rn = 1/sqrt(mean_c(y^2)+1e-8) (needs MG_CONV_LRELU) */
#define MG_CONV_POOL_OUT 16 /* also emit p = AvgPool2d(2,2)(y) (N,Cout,H/2,W/2) [discriminator.py:24]; excludes PIXNORM */
/* Tile masks (mg_wino3x3 only): what the backward pass of conv -> LeakyReLU -> AvgPool2d [discriminator.py:15-24] needs of the
 * full-resolution activation is its sign, so the forward pass can keep one BYTE per 2x2 tile and out-channel instead of four
 * floats: bit 2i+j set <=> y[2Y+i][2X+j] > 0, tensor (N,Cout,H/2,W/2) of uint8. */
#define MG_CONV_MASK_OUT 32   /* with POOL_OUT|LRELU: y (cast to uint8_t*) receives the tile mask; the fp32 y is not written */
#define MG_CONV_MASK_BYTES 64 /* with MASK_AUX|POOL_OUT: aux (cast to const uint8_t*) is the tile mask of THIS conv's output; only p is written */
#define MG_CONV_UNPOOL 128    /* alone: aux = tile mask with one byte per OUTPUT PIXEL (N,Cout,H,W) of this conv; y is (N,Cout,2H,2W): \
                                 y[2Y+i][2X+j] = 0.25 * acc[Y][X] * (bit 2i+j ? 1 : slope), i.e. AvgPool2d backward and the LeakyReLU \
                                 backward of the layer below fused on the data-gradient conv that feeds them */

/* number of floats of the packed (LDS-image) weight layout for a Cin->Cout conv */
size_t mg_conv3x3_packed_floats(int Cin, int Cout);
/* w is the module weight [Co][Ci][3][3].  dgrad=0: pack for the forward conv Ci->Co.  dgrad=1: pack for the data-gradient
 * conv Co->Ci (taps flipped, channels transposed). */
int mg_conv3x3_pack(const float* w, float* wp, int Co, int Ci, int dgrad, mg_stream_t stream);
/* y[N,Cout,H,W] = epilogue(conv3x3(x, wp) + bias).  bias/aux/p/rn may be NULL when the flag that uses them is unset. */
int mg_conv3x3(const float* x, const float* wp, const float* bias, const float* aux, float* y, float* p, float* rn,
               int N, int Cin, int Cout, int H, int W, int flags, float slope, mg_stream_t stream);

/* Upsample(x2 nearest) -> Conv2d(3x3) [generator.py:26-37] in sub-pixel form: four 2x2 convolutions on the LOW-resolution
 * input (16 instead of 36 multiply-adds per low-res pixel and channel pair; same result up to fp32 summation order).
 * x: (N,Cin,Hin,Win); y/p: (N,Cout,2Hin,2Win); rn: (N,1,2Hin,2Win).  flags: MG_CONV_LRELU, MG_CONV_PIXNORM.  wp from
 * mg_upconv3x3_pack (effective weights, mg_upconv3x3_packed_floats floats).  Cout <= 96 recommended (register budget). */
/* The same layer -- Upsample(x2 nearest) -> Conv2d(3x3) [generator.py:24-39] (+ LeakyReLU + PixelNorm, layers.py:11-17) -- and its
 * data gradient (aten::convolution_backward input + upsample_nearest2d_backward) in Winograd F(2x2,3x3) form on the up-sampled grid
 * without the 7 of 16 components that vanish there: 9 multiply-adds per output tile and channel pair (sub-pixel form: 16, direct on
 * the up-sampled tensor: 36).  up: MG_PACK_WINOUPS filters of the module weight [Cout][Cin][3][3] (mg_pack_multi, dgrad = 0 / 1;
 * mg_winoups3x3_packed_floats floats).  Forward: x (N,Cin,Hin,Win) -> y / p (N,Cout,2Hin,2Win), rn (N,1,2Hin,2Win); flags
 * MG_CONV_LRELU, MG_CONV_PIXNORM (then p is written, y optional).  Data gradient: gy (N,Cout,2Hin,2Win) -> gx (N,Cin,Hin,Win).
 * mg_winoups3x3_supported: Win a multiple of 16, Hin of 8, 16..64 out-channels of the call in whole tiles, the 9-component filter
 * bank within the LDS. */
int mg_winoups3x3_supported(int N, int Cin, int Cout, int Hin, int Win, int dgrad);
size_t mg_winoups3x3_packed_floats(int Cin, int Cout, int dgrad);
int mg_winoups3x3(const float* x, const float* up, const float* bias, float* y, float* p, float* rn, int N, int Cin, int Cout,
                  int Hin, int Win, int flags, float slope, mg_stream_t stream);
int mg_winoups3x3_dgrad(const float* gy, const float* up, float* gx, int N, int Cin, int Cout, int Hin, int Win, mg_stream_t stream);
/* mg_winoups3x3_dgrad with the PixelNorm + LeakyReLU backward of the layer below [generator.py:31-39, layers.py:11-17] in the epilogue:
 * p (N,Cin,Hin,Win) that layer's normalised output, rn (N,1,Hin,Win) its 1/norm; gpre = lrelu'(p) rn (gx - p mean_c(gx p)). */
int mg_winoups3x3_dgrad_pn(const float* gy, const float* up, const float* p, const float* rn, float* gpre, int N, int Cin, int Cout, int Hin,
                           int Win, float slope, mg_stream_t stream);
/* mg_winoups3x3 (LeakyReLU + PixelNorm) with the generator's 1x1 head [generator.py:118-126 ToMagnPhaseLayer] on the normalised
 * activation in the same epilogue: mp = tanh(hw p + hb), hw (2,Cout), hb (2) or NULL, mp (N,2,2Hin,2Win); p, rn as above, y optional. */
int mg_winoups3x3_head_supported(int N, int Cin, int Cout, int Hin, int Win); /* mg_winoups3x3_supported and at most 48 out-channels */
int mg_winoups3x3_head(const float* x, const float* up, const float* bias, float* y, float* p, float* rn, const float* hw, const float* hb,
                       float* mp, int N, int Cin, int Cout, int Hin, int Win, float slope, mg_stream_t stream);
size_t mg_upconv3x3_packed_floats(int Cin, int Cout);
int mg_upconv3x3_pack(const float* w, float* wp, int Co, int Ci, mg_stream_t stream);
int mg_upconv3x3(const float* x, const float* wp, const float* bias, float* y, float* p, float* rn, int N, int Cin, int Cout,
                 int Hin, int Win, int flags, float slope, mg_stream_t stream);

/* The same convolution (no UPS_IN; even H, W) in Winograd F(2x2,3x3) form: 16 instead of 36 multiplies per 2x2 output tile
 * and channel pair, fp32 throughout (rounding within ~1.2x rms of the direct form).  Same arguments, flags and fused epilogues
 * as mg_conv3x3; PIXNORM needs Cout <= 64.  up from mg_wino3x3_pack (dgrad = 1: filters of the data-gradient convolution). */
size_t mg_wino3x3_packed_floats(int Cin, int Cout);
int mg_wino3x3_pack(const float* w, float* up, int Co, int Ci, int dgrad, mg_stream_t stream);
/* whether MG_CONV_MASK_AUX | MG_CONV_MASK_BYTES WITHOUT MG_CONV_POOL_OUT (y = result x lrelu'(tile-mask bytes), full resolution) is
 * available for this shape: an epilogue of the wave-per-tile-block kernel (csrc/wino_strip.hip) only */
int mg_wino3x3_mask_bytes_y_supported(int N, int Cin, int Cout, int H, int W);
int mg_wino3x3(const float* x, const float* up, const float* bias, const float* aux, float* y, float* p, float* rn, int N,
               int Cin, int Cout, int H, int W, int flags, float slope, mg_stream_t stream);

/* The critic's fade-in blend [discriminator.py:111-116: alpha * conv_blocks[curr](start_block(x)) + (1 - alpha) *
 * last_start_block(x)] fused on the Winograd convolution next to it, so that neither the blend nor its backward is a pass of its
 * own.  coef: {alpha, 1 - alpha} in DEVICE memory (a captured graph stays valid while alpha moves); tile masks as above.
 *   MG_FADE_FWD      y = coef[0] * leaky_relu(conv(x) + bias) + coef[1] * other;   out2 (uint8, N,Cout,H/2,W/2) = tile mask of
 *                    the LeakyReLU output (all the backward passes need of it)
 *   MG_FADE_TANGENT  y = coef[0] * (conv(x) * lrelu'(mask_in)) + coef[1] * other   (tangent pass of the gradient penalty)
 *   MG_FADE_BWD      up = data-gradient filters, x = gradient w.r.t. the conv AFTER the blend:
 *                    y = (coef[0] * conv(x)) * lrelu'(mask_in),  out2 (float, N,Cout,H,W) = (coef[1] * conv(x)) * lrelu'(other > 0)
 * Results are bitwise those of mg_wino3x3 followed by mg_axpby / mg_blend_lrelu_bwd. */
#define MG_FADE_FWD 1
#define MG_FADE_TANGENT 2
#define MG_FADE_BWD 3
int mg_wino3x3_fade(const float* x, const float* up, const float* bias, const unsigned char* mask_in, const float* other,
                    const float* coef, float* y, void* out2, int N, int Cin, int Cout, int H, int W, int mode, float slope,
                    mg_stream_t stream);

/* Weight (+ bias) gradient of the same convolution in Winograd F(3x3,2x2) form (even H, W; flags: MG_CONV_UPS_IN): same result as
 * mg_conv3x3_wgrad within fp32 rounding, 2.25x fewer multiplies, split-K slabs reduced in a fixed order (deterministic).
 * gw[Cout][Cin][3][3] (+)= ..., gb[Cout] (+)= sum of gy over samples n < bias_n (0: all; gb may be NULL). */
/* Which kernel mg_wino3x3_wgrad_partial(_multi) runs for a layer (accounting of executed FLOPs, tests): 0 = chunk-staged forms
 * (16 Winograd products per tile), 1 = row-staged form, 2 = row-staged form for an up-sampled input (MG_CONV_UPS_IN: 9 of the 16
 * products), -1 = shape not supported.  group_max_chunks as passed to mg_wino3x3_wgrad_partial_multi (0: single launches). */
int mg_wino3x3_wgrad_form(int N, int Cin, int Cout, int H, int W, int flags, int group_max_chunks);
size_t mg_wino3x3_wgrad_ws_bytes(int N, int Cin, int Cout, int H, int W);
int mg_wino3x3_wgrad(const float* x, const float* gy, float* gw, float* gb, void* ws, size_t ws_bytes, int N, int Cin, int Cout,
                     int H, int W, int flags, int accumulate, int bias_n, mg_stream_t stream);
/* The same in two halves, so that the slab reductions of several layers run in ONE launch at the end of an update's weight-gradient
 * sweep (each is a ~20 us latency-bound kernel): _partial runs the matrix kernel into `ws` (one workspace PER LAYER, alive until
 * the reduce) and fills `job`; _reduce sums the slabs of n jobs in a fixed order, applies G^T . G and writes gw / gb. */
typedef struct {
  const float* slab;
  const float* slab_b;
  float* gw;
  float* gb;
  int32_t nsplit, Cout, Cin, CoutP, CinP, accumulate;
} mg_wgrad_job_t;
int mg_wino3x3_wgrad_partial(const float* x, const float* gy, float* gw, float* gb, void* ws, size_t ws_bytes, int N, int Cin,
                             int Cout, int H, int W, int flags, int accumulate, int bias_n, mg_wgrad_job_t* job,
                             mg_stream_t stream);
int mg_wino3x3_wgrad_reduce(const mg_wgrad_job_t* jobs, int n, mg_stream_t stream);
/* _partial for the n layers of a sweep at once (the weight gradients of one backward pass: convolution_backward of every
 * nn.Conv2d(3x3) in generator.py:9-40 / discriminator.py:8-34).  Layers of at most group_max_chunks x (number of CUs) units of work
 * (8-tile chunks x channel blocks) whose channel blocks have the same shape share ONE launch, with their splits sized so that the
 * group -- not every layer -- fills the chip: fewer launches, fewer and smaller slabs for the reduce.  group_max_chunks <= 0:
 * one launch per layer, exactly as n calls of _partial.  jobs[i] belongs to d[i]; results are bitwise independent of the grouping
 * only up to the split count (the slabs are summed in a fixed order either way: deterministic for a given grouping). */
typedef struct {
  const float* x;
  const float* gy;
  float* gw;
  float* gb;
  void* ws;
  size_t ws_bytes;
  int32_t N, Cin, Cout, H, W, flags, accumulate, bias_n;
} mg_wgrad_desc_t;
int mg_wino3x3_wgrad_partial_multi(const mg_wgrad_desc_t* d, int n, int group_max_chunks, mg_wgrad_job_t* jobs, mg_stream_t stream);
/* the same split of mg_conv3x3_wgrad (the direct form's jobs carry CoutP = CinP = 0 and go to their own reduce) */
int mg_conv3x3_wgrad_partial(const float* x, const float* gy, float* gw, float* gb, void* ws, size_t ws_bytes, int N, int Cin,
                             int Cout, int H, int W, int flags, int accumulate, int bias_n, mg_wgrad_job_t* job,
                             mg_stream_t stream);
int mg_conv3x3_wgrad_reduce(const mg_wgrad_job_t* jobs, int n, mg_stream_t stream);

/* Data gradient of Upsample(x2) -> Conv3x3 w.r.t. the LOW-resolution input: one stride-2 convolution with the 4x4 effective
 * kernel over gy (N,Cout,2Hin,2Win) -> gx (N,Cin,Hin,Win); replaces conv-dgrad at 2Hx2W + the 2x2 block sums of Upsample's
 * backward.  wp from mg_upconv3x3_dgrad_pack(w [Co][Ci][3][3]). */
size_t mg_upconv3x3_dgrad_packed_floats(int Cin, int Cout);
int mg_upconv3x3_dgrad_pack(const float* w, float* wp, int Co, int Ci, mg_stream_t stream);
int mg_upconv3x3_dgrad(const float* gy, const float* wp, float* gx, int N, int Cin, int Cout, int Hin, int Win,
                       mg_stream_t stream);

/* weight/bias gradient of the same conv (aten::convolution_backward, weight+bias grads):
 *   gw[Cout][Cin][3][3] (+)= sum_{n,y,x} gy[n,o,y,x] * xin[n,c,y+ky-1,x+kx-1],  gb[Cout] (+)= sum gy   (gb may be NULL)
 * flags: MG_CONV_UPS_IN as above; accumulate!=0 adds to gw/gb instead of overwriting.  bias_n: only samples n < bias_n feed
 * gb (<= 0: all N) -- lets one launch over a concatenated batch sum weight gradients of all samples but bias gradients of a
 * leading sub-batch (the gradient-penalty part has no bias gradient).  ws: scratch of mg_conv3x3_wgrad_ws_bytes() bytes
 * (split-K partial slabs, reduced in a fixed order => deterministic). */
size_t mg_conv3x3_wgrad_ws_bytes(int N, int Cin, int Cout, int H, int W);
int mg_conv3x3_wgrad(const float* x, const float* gy, float* gw, float* gb, void* ws, size_t ws_bytes, int N, int Cin,
                     int Cout, int H, int W, int flags, int accumulate, int bias_n, mg_stream_t stream);

/* the same on 1x1 maps (the last critic conv after the final AvgPool2d, discriminator.py:14-34): x (N,Cin,1,1), gy (N,Cout,1,1);
 * only the centre tap is non-zero.  No workspace, no reduce; float64 accumulation in sample order (deterministic). */
int mg_conv3x3_wgrad_1x1map(const float* x, const float* gy, float* gw, float* gb, int N, int Cin, int Cout, int accumulate,
                            int bias_n, mg_stream_t stream);

/* ------------------------------------------------------------------ 1x1 convolutions (stem 2->C, head C->2)
 * Replaces MagPhaseLayer [discriminator.py:37-50] and ToMagnPhaseLayer [generator.py:43-52].  One of Cin/Cout must be <= 4.
 */
#define MG_C1_LRELU 1      /* y = leaky_relu(.) */
#define MG_C1_TANH 2       /* y = tanh(.) */
#define MG_C1_MASK_AUX 4   /* Cin<=4: y = acc * (aux > 0 ? 1 : slope), aux is N,Cout,HW (output side);
                            * Cout<=4 (Cin>4): x is first multiplied by (aux > 0 ? 1 : slope), aux is N,Cin,HW (input side) */
#define MG_C1_TRANSPOSED 8 /* use w^T: w is [Cin][Cout] in memory (data gradient of the forward conv) */
#define MG_C1_TANH_BWD_IN 16 /* input is gy*(1-aux_in^2): tanh backward fused on the INPUT side (aux_in: N,Cin,HW) */
#define MG_C1_ACCUM 32       /* Cin<=4: y += result (two gradient branches joining: generator.py:118-124 backwards) */
int mg_conv1x1(const float* x, const float* w, const float* bias, const float* aux, float* y, int N, int Cin, int Cout,
               int HW, int flags, float slope, mg_stream_t stream);
/* gw[Cout][Cin] (+)= sum gy*x, gb (+)= sum gy; if tanh_y != NULL gy is first multiplied by (1 - tanh_y^2).
 * bias_n (as for the 3x3 weight gradients): only samples n < bias_n feed gb (0: all) -- the penalty's tangent samples of the
 * fused critic step have no bias gradient. */
size_t mg_conv1x1_wgrad_ws_bytes(int N, int Cin, int Cout, int HW);
int mg_conv1x1_wgrad(const float* x, const float* gy, const float* tanh_y, float* gw, float* gb, void* ws,
                     size_t ws_bytes, int N, int Cin, int Cout, int HW, int accumulate, int bias_n, mg_stream_t stream);

/* The two-channel ends of both networks while a block fades in, one launch each (csrc/fade_ends.hip).
 * mg_stem_pair [discriminator.py:107-113 forward]: h0 = act(ws x + bs) (N,C0,H,W); xp = AvgPool2d(x) (N,2,H/2,W/2; may be NULL);
 *   o = act(wo xp + bo) (N,C1,H/2,W/2).  flags: MG_C1_LRELU, or MG_C1_MASK_AUX = bias-free results times the LeakyReLU derivative of
 *   the activations h0 / o hold, written over them (the penalty's tangent pass).  ws (C0,2), wo (C1,2).  H even, W % 4 == 0.
 *   h0_mask (optional, forward form): the tile mask of h0 in mg_wino3x3's format (N,C0,H/2,W/2 uint8, bit 2i+j <-> h0[2Y+i][2X+j] > 0),
 *   what the data-gradient conv in front of the stem reads instead of h0 itself (MG_CONV_MASK_AUX | MG_CONV_MASK_BYTES).
 * mg_stem_pair_gx [the same lines, backward to x]: gx = ws^T gs + 0.25 * up2(wo^T go), gs (N,C0,H,W), go (N,C1,H/2,W/2), gx (N,2,H,W).
 * mg_head_pair [generator.py:118-126]: mp = tanh(wh x + bh) (N,2,H,W), old = tanh(wo xl + bo) (N,2,H/2,W/2), out = a mp + b up2(old);
 *   (a, b) = coef[0..1] from device memory if coef != NULL, else (ca, cb); mp / old may be NULL (not kept).  wh (2,C), wo (2,Cl).
 * mg_blend_up_bwd: gx = a g, gy = b * (2x2 block sums of g): the blend's backward (g: (NC,H,W), gy: (NC,H/2,W/2)).
 * mg_gen_head_bwd [generator.py:118-126 backward + layers.py:11-17 / generator.py:31-39 backward of the block in front]: from the
 *   gradient g_mp (N,2,H,W) at the head's tanh output mp: t = g_mp (1 - mp^2); gw (2,C) (+)= sum t p, gb (2) (+)= sum t (autograd's
 *   convolution_backward of the 1x1 head, x = p (N,C,H,W) the last block's PixelNorm output); g = w^T t; gpre = lrelu'(p) rn
 *   (g - p mean_c(g p)) (N,C,H,W) = the gradient at the last conv's pre-activation (PixelNorm + LeakyReLU backward, rn (N,1,H,W) the
 *   stored 1/norm).  One read of p, one write of gpre.  g_in (optional, (N,C,H,W)): a second gradient arriving at p, added to g (the old
 *   head of a fading-in level: p is also the input of the last block's first conv, g_in that conv's data gradient).
 *   C in {16, 32, 48, 64}, or any multiple of 4 up to 128 on small maps (N H W <= 32 768); ws: mg_gen_head_bwd_ws_floats(N, C, HW) floats. */
int mg_stem_pair(const float* x, const float* ws, const float* bs, const float* wo, const float* bo, float* h0, float* xp, float* o,
                 unsigned char* h0_mask, int N, int C0, int C1, int H, int W, int flags, float slope, mg_stream_t stream);
int mg_stem_pair_gx(const float* gs, const float* ws, const float* go, const float* wo, float* gx, int N, int C0, int C1, int H, int W,
                    mg_stream_t stream);
int mg_head_pair(const float* x, const float* wh, const float* bh, const float* xl, const float* wo, const float* bo, const float* coef,
                 float ca, float cb, float* mp, float* old, float* out, int N, int C, int Cl, int H, int W, mg_stream_t stream);
int mg_blend_up_bwd(const float* g, const float* coef, float ca, float cb, float* gx, float* gy, int NC, int H, int W,
                    mg_stream_t stream);
/* mg_head_pair with mp given (written by mg_winoups3x3_head): old = tanh(wo xl + bo), out = a mp + b up2(old). */
int mg_head_pair_from_mp(const float* mp, const float* xl, const float* wo, const float* bo, const float* coef, float ca, float cb,
                         float* old, float* out, int N, int Cl, int H, int W, mg_stream_t stream);
int mg_gen_head_bwd_supported(int C, int Cout);                      /* C in {16, 32, 48, 64}: any size */
int mg_gen_head_bwd_supported_at(int C, int Cout, int N, int HW);     /* ... or a multiple of 4 up to 128 on at most 32 768 pixels */
size_t mg_gen_head_bwd_ws_floats(int N, int C, int HW);
int mg_gen_head_bwd(const float* g_mp, const float* mp, const float* w, const float* p, const float* rn, const float* g_in, float* gpre,
                    float* gw, float* gb, float* ws, size_t ws_floats, int N, int C, int HW, float slope, int accumulate, mg_stream_t stream);

/* ------------------------------------------------------------------ element-wise / small ops */
/* PixelNorm forward [layers.py:11-17]: p = y*rn, rn[n,hw] = 1/sqrt(mean_c y^2 + 1e-8) */
int mg_pixelnorm_fwd(const float* y, float* p, float* rn, int N, int C, int HW, mg_stream_t stream);
/* backward through PixelNorm then LeakyReLU: gpre = mask(y) * rn * (gp - p * mean_c(gp * p)), p = y*rn.
 * from_p != 0: the `y` argument is the normalised output p itself (the pre-norm activation need not be kept). */
int mg_pixelnorm_lrelu_bwd(const float* gp, const float* y, const float* rn, float* gpre, int N, int C, int HW,
                           float slope, int from_p, mg_stream_t stream);
/* nn.Upsample(x2 nearest) forward / backward (sum of each 2x2 block) [generator.py:26-29,99-102] */
int mg_upsample2x_fwd(const float* x, float* y, int NC, int Hin, int Win, mg_stream_t stream);
int mg_upsample2x_bwd(const float* gy, float* gx, int NC, int Hin, int Win, mg_stream_t stream);
/* nn.AvgPool2d(2,2) forward [discriminator.py:24,131]; backward fused with the LeakyReLU mask of the layer below:
 * gx = 0.25 * gy[.., h/2, w/2] * (act > 0 ? 1 : slope)   (act NULL => no mask) */
int mg_avgpool2_fwd(const float* x, float* y, int NC, int H, int W, mg_stream_t stream);
int mg_avgpool2_bwd(const float* gy, const float* act, float* gx, int NC, int H, int W, float slope,
                    mg_stream_t stream);
/* the same with the mask given as tile bytes (MG_CONV_MASK_OUT above: (NC,H/2,W/4*2) uint8, bit 2i+j <-> act[2h+i][2w+j] > 0);
 * W must be a multiple of 4 */
int mg_avgpool2_bwd_tilemask(const float* gy, const unsigned char* mask, float* gx, int NC, int H, int W, float slope,
                             mg_stream_t stream);
/* out = g * (act > 0 ? 1 : slope) */
int mg_lrelu_bwd(const float* g, const float* act, float* out, size_t n, float slope, mg_stream_t stream);
/* backward of the critic's fade-in blend [discriminator.py:111-113] and of the two LeakyReLUs feeding it, in one pass:
 * out_a = ca*g*(act_a > 0 ? 1 : slope), out_o = co*g*(act_o > 0 ? 1 : slope)  (rounded as (c*g)*mask, like axpby + lrelu_bwd) */
int mg_blend_lrelu_bwd(const float* g, const float* act_a, const float* act_o, float ca, float co, float* out_a, float* out_o,
                       size_t n, float slope, mg_stream_t stream);
/* out = a*x + b*y (fade-in blend [generator.py:124, discriminator.py:113]); y may be NULL (out = a*x) */
int mg_axpby(float a, const float* x, float b, const float* y, float* out, size_t n, mg_stream_t stream);
/* out[n,c,h,w] = a*x[n,c,h,w] + b*up2(y)[n,c,h,w], y is (NC, H/2, W/2) */
int mg_blend_up(float a, const float* x, float b, const float* y, float* out, int NC, int H, int W,
                mg_stream_t stream);
/* The three fade-in kernels with their coefficients (a, b) = coef[0], coef[1] read from DEVICE memory (y == NULL: coef[0] only):
 * alpha changes every iteration of a fade-in (utils.py:62-68); as launch arguments it would be baked into a captured HIP graph
 * of the update.  Same values, same results as the scalar forms. */
int mg_axpby_dev(const float* coef, const float* x, const float* y, float* out, size_t n, mg_stream_t stream);
int mg_blend_up_dev(const float* coef, const float* x, const float* y, float* out, int NC, int H, int W, mg_stream_t stream);
int mg_blend_lrelu_bwd_dev(const float* g, const float* act_a, const float* act_o, const float* coef, float* out_a, float* out_o,
                           size_t n, float slope, mg_stream_t stream);
/* Linear(K -> 1) [discriminator.py:103-105]: y[n] = b + sum_k w[k] x[n,k] */
int mg_linear1_fwd(const float* x, const float* w, const float* b, float* y, int N, int K, mg_stream_t stream);
/* gx[n,k] = gy[n]*w[k]; gw[k] (+)= sum_n gy[n] x[n,k]; gb (+)= sum_{n < bias_n} gy[n] (0: all n)   (gx/gw/gb may be NULL) */
int mg_linear1_bwd(const float* x, const float* w, const float* gy, float* gx, float* gw, float* gb, int N, int K,
                   int accumulate, int bias_n, mg_stream_t stream);
/* gradient-penalty helpers [discriminator.py:166-184] */
int mg_gp_interp(const float* x_real, const float* x_fake, const float* eps, float* out, int N, size_t chw,
                 mg_stream_t stream); /* out = eps[n]*real + (1-eps[n])*fake */
int mg_sumsq_per_sample(const float* g, float* out, int N, size_t chw, mg_stream_t stream);
int mg_scale_per_sample(const float* g, const float* coef, float* out, int N, size_t chw, mg_stream_t stream);
/* tiny: from sumsq[N] compute penalty = factor*mean((sqrt(ss)-1)^2) and coef[n] = upstream*factor*2*(norm-1)/(N*norm) */
int mg_gp_finish(const float* sumsq, float* penalty, float* coef, int N, float factor, float upstream,
                 mg_stream_t stream);
/* mg_gp_finish + mg_scale_per_sample in one launch: out = g * coef[n] with coef as above, penalty (may be NULL) as above */
int mg_gp_apply(const float* g, const float* sumsq, float* penalty, float* out, int N, size_t chw, float factor, float upstream,
                mg_stream_t stream);
/* sum over (n, hw) of a per-channel tensor: out[c] (+)= sum x[n,c,hw] */
int mg_channel_sum(const float* x, float* out, int N, int C, int HW, int accumulate, mg_stream_t stream);

/* Wasserstein losses [criterion.py:12-18] and the score means train.py:180-186 logs, one launch: out[g] = mean of the g-th group of
 * n consecutive critic scores (g < groups <= 8), out[groups] = groups >= 2 ? out[1] - out[0] (= wasserstein_discriminator_loss
 * with group 0 = real, 1 = fake) : -out[0] (= wasserstein_generator_loss).  out has groups + 1 floats. */
int mg_group_means(const float* x, int groups, int n, float* out, mg_stream_t stream);

/* ------------------------------------------------------------------ multi-tensor weight re-packing
 * All of mg_conv3x3_pack / mg_wino3x3_pack / mg_upconv3x3_pack / mg_upconv3x3_dgrad_pack for a list of weights in ONE launch (the
 * reference has no counterpart: these layouts replace what MIOpen / oneDNN re-derive from nn.Conv2d.weight inside every call).
 * descs is a HOST array; `out` buffers are sized by the matching *_packed_floats(). */
enum { MG_PACK_CONV3X3 = 0, MG_PACK_WINO3X3 = 1, MG_PACK_UPCONV3X3 = 2, MG_PACK_UPCONV3X3_DGRAD = 3, MG_PACK_SMALLNET = 4, MG_PACK_WINOUPS = 5 };
typedef struct {
  const float* w; /* module weight [Co][Ci][3][3] */
  float* out;
  int32_t kind, Co, Ci, dgrad; /* dgrad: data-gradient variant (kinds 0, 1, 4 and 5 only) */
} mg_pack_desc_t;
int mg_pack_multi(const mg_pack_desc_t* descs, int n, mg_stream_t stream);

/* ------------------------------------------------------------------ fused Adam [train.py:64-70,175,214]
 * Multi-tensor torch.optim.Adam step (amsgrad off, weight_decay 0).  desc is a HOST array of n_tensors records (device pointers
 * inside); the records are passed to the kernel by value, so the call neither copies nor synchronises. */
typedef struct {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
  float step_size;  /* lr / (1 - beta1^step), step = count AFTER this update (>= 1) */
  float bc2_sqrt;   /* sqrt(1 - beta2^step) */
} mg_adam_tensor_t;
int mg_adam_step(const mg_adam_tensor_t* desc, int n_tensors, float beta1, float beta2, float eps, float grad_scale,
                 mg_stream_t stream);
/* Same update with the per-parameter step count in DEVICE memory (int32, count BEFORE this update; advanced by the call): the
 * bias corrections are formed on the device, so the launch carries nothing that changes from step to step and can be captured
 * in a HIP graph and replayed (torch.optim.Adam(capturable=True) semantics). */
typedef struct {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
  int32_t* step;
} mg_adam_tensor_dev_t;
int mg_adam_step_dev(const mg_adam_tensor_dev_t* desc, int n_tensors, float lr, float beta1, float beta2, float eps,
                     float grad_scale, mg_stream_t stream);
/* mg_adam_step_dev with an exponential running average of the weights kept in the same pass: after the update of `param`,
 * ema = ema + (param - ema) * ema_weight, ema_weight = 1 - decay in (0, 1].  param, exp_avg, exp_avg_sq and the step counters
 * come out bit for bit as from mg_adam_step_dev; the average costs no launch of its own. */
typedef struct {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
  int32_t* step;
  float* ema;
} mg_adam_tensor_dev_ema_t;
int mg_adam_step_dev_ema(const mg_adam_tensor_dev_ema_t* desc, int n_tensors, float lr, float beta1, float beta2, float eps,
                         float grad_scale, float ema_weight, mg_stream_t stream);

/* ------------------------------------------------------------------ STFT [audio/functions.py:38-62]
 * wav: mono fp32 [L]; out_re/out_im: [512][T] (freq-major, Nyquist row dropped), T = 1 + L/256.  Periodic Hann(1024),
 * centre reflect padding, hop 256, divided by sqrt(sum w^2).  If out_im == NULL, out_re is interleaved complex64 [512][T][2]. */
int mg_stft_1024(const float* wav, float* out_re, float* out_im, int64_t L, mg_stream_t stream);
/* The same transform straight from a file's PCM frames [functions.py:43-49: th_audio.load (normalised to [-1, 1]) and
 * raw_audio.mean(0)]: pcm holds L frames of `channels` interleaved samples as a WAV file stores them (kind: MG_PCM_*), the
 * scaling (int16: / 32768, int32: / 2^31, uint8: (v - 128) / 128) and the mono mean happen inside the STFT kernel's loads for
 * float32 / int16 with one or two channels; other formats take one conversion pass through `ws` (mg_stft_1024_pcm_ws_bytes). */
enum { MG_PCM_F32 = 0, MG_PCM_I16 = 1, MG_PCM_I32 = 2, MG_PCM_U8 = 3 };
/* the conversion alone: mono[L] float32 = mean over channels of the normalised samples [functions.py:43-49] */
int mg_pcm_to_mono(const void* pcm, int kind, int channels, float* mono, int64_t L, mg_stream_t stream);
/* wav_to_stft's other arguments [functions.py:38-41: nperseg, stride]: the same definition for any power-of-two n_fft in
 * [64, 8192] and any hop (periodic Hann(n_fft), reflect padding n_fft/2, / sqrt(sum w^2), rows 0 .. n_fft/2 - 1);
 * out_c64: interleaved complex64 [n_fft/2][1 + L/hop].  An untuned radix-2 path: the drivers only use 1024 / 256. */
int mg_stft_generic(const float* wav, float* out_c64, int64_t L, int n_fft, int hop, mg_stream_t stream);
size_t mg_stft_1024_pcm_ws_bytes(int64_t L, int channels, int kind);
int mg_stft_1024_pcm(const void* pcm, int kind, int channels, float* out_re, float* out_im, void* ws, size_t ws_bytes, int64_t L,
                     mg_stream_t stream);

/* ------------------------------------------------------------------ resampling [torchaudio.functional.resample with its defaults]
 * What a user of the reference calls in front of wav_to_stft for a file that is not at 44.1 kHz (functions.py:45 accepts no other
 * rate): sinc_interp_hann, lowpass_filter_width = lpw, rolloff.  With o / n = orig_freq / new_freq reduced by their gcd,
 * base = min(o, n) * rolloff, w = ceil(lpw * o / base), output m = T n + p is sum_k xpad[T o + k] h_p[k] over the 2w + o taps of
 * torchaudio's row p (xpad = x zero-padded by (w, w + o)), truncated to ceil(n L / o) outputs; orig_freq == new_freq is the identity.
 * Only 2w + 1 consecutive taps per row differ from a rounding of zero (<= 1.3e-49 at the defaults): the bank keeps those.
 * mg_resample_len: ceil(n L / o) (L when the rates are equal); -1 for bad arguments.  Host only. */
int64_t mg_resample_len(int64_t L, int orig_freq, int new_freq);
/* bytes of the compact bank: float32 taps [phases = n][taps = 2w + 1], then int32 start[n] = floor(o p / n), the index in
 * torchaudio's row p of compact tap 0 (equal rates: one phase, one unit tap).  0 for bad arguments.  Host only. */
size_t mg_resample_bank_size(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int* phases, int* taps);
/* fills the bank in HOST memory: computed in float64 with torchaudio's order of operations, rounded once to float32. */
int mg_resample_bank(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, void* bank, size_t bank_bytes);
/* out[r][m], m < mg_resample_len(L, ..): the resampled mono signal of `rows` rows of L PCM frames each (row r starts at frame
 * r * row_stride; frames of `channels` interleaved samples of kind MG_PCM_*), normalised and averaged over channels on load
 * exactly as mg_pcm_to_mono does; bank: the device copy of mg_resample_bank's output for the same arguments.  One launch.
 * Taps per output are accumulated in a fixed order (x_0 h_0, then FMAs j = 1 .. 2w), so equal inputs give equal bits. */
int mg_resample_pcm(const void* pcm, int kind, int channels, int rows, int64_t row_stride, int64_t L, int orig_freq, int new_freq,
                    int lowpass_filter_width, double rolloff, const void* bank, size_t bank_bytes, float* out, mg_stream_t stream);

/* ------------------------------------------------------------------ FLAC decoding [torchaudio.load of a .flac file: functions.py:43,
 * th_audio.load]
 * RFC 9639 streams of 1-8 channels, 4-24 bits, any block size, fixed or variable blocking.  The host parses the metadata blocks and
 * passes the AUDIO REGION (the bytes from the first frame header to the end of the stream) as a device buffer that is 16-byte aligned
 * and readable, zero filled past nbytes, up to mg_flac_padded_bytes(nbytes).  Offsets below are bytes into that region.
 * Workspace (mg_flac_ws_bytes, for at most cand_cap frame-header candidates) starts with int64 status[16]:
 *   [0] candidates found (more than cand_cap: nothing was decoded, call again with a larger cap), [1] frames, [2] samples,
 *   [3] chain error (0 ok, 1 no valid header where frame [4] must start, at byte [5]; 3 candidates over cap), [6] blocking,
 *   [7] first frame with a problem (INT64_MAX: none), [8] its MG_FLAC_F* flags, [9] its start, [10] its decoded end (after the
 *   CRC-16), [11] the next frame's start in the chain.
 * Host-only size queries: */
#define MG_FLAC_F_CRC 1    /* the CRC-16 of the frame as decoded does not check */
#define MG_FLAC_F_END 2    /* the decoded end is not where the chain put the next frame (a false sync code was taken) */
#define MG_FLAC_F_HDR 4    /* header rate / depth / channels disagree with STREAMINFO */
#define MG_FLAC_F_SYNTAX 8 /* invalid subframe fields, or the frame runs past the region */
#define MG_FLAC_F_RANGE 16 /* samples beyond out_frames */
size_t mg_flac_padded_bytes(int64_t nbytes);
size_t mg_flac_ws_bytes(int64_t nbytes, int64_t cand_cap);
/* frame-header scan of every byte offset (sync code, fields, CRC-8), candidates in offset order, and the frame chain from byte 0 */
int mg_flac_scan(const void* data, int64_t nbytes, void* ws, size_t ws_bytes, int64_t cand_cap, mg_stream_t stream);
/* keeps frames 0 .. frame - 1 and chains again from a header at byte `offset` (the decoded end of frame - 1) */
int mg_flac_rechain(const void* data, int64_t nbytes, void* ws, size_t ws_bytes, int64_t cand_cap, int64_t frame, int64_t offset,
                    mg_stream_t stream);
/* decodes the chained frames into out (out_frames, channels): int16 (bits <= 16) or int32, samples left-justified in the container
 * (v << (16 - bits) or v << (32 - bits)), as wav / aiff PCM is stored; planar: int32 [channels][out_frames] scratch.  channels,
 * bits and sample_rate come from STREAMINFO and are checked against every frame header. */
int mg_flac_decode(const void* data, int64_t nbytes, void* ws, size_t ws_bytes, int64_t cand_cap, int channels, int bits,
                   int sample_rate, int32_t* planar, void* out, int64_t out_frames, mg_stream_t stream);

/* ------------------------------------------------------------------ Ogg Vorbis decoding [torchaudio.load of a .ogg file:
 * functions.py:43, th_audio.load]
 * Vorbis I streams of 1-8 channels, blocksizes 64-8192, floor 1, residues 0 / 1 / 2.  The host walks the Ogg pages, checks the
 * header pages, parses the headers and packs the setup (musicgan_amd/audio/vorbis.py pack_setup: `setup` int32 records, `fsetup`
 * float32 VQ values, dB table, IMDCT twiddles and window slopes), all on the device.  `file`: the whole file on the device;
 * `pages`: int64 [npages][4] (file offset, body offset, body bytes, payload offset); pages from `crc_from` on have their CRC-32
 * checked; `packets`: int64 [npk][5] (payload offset, bytes, spectrum offset in floats, first returned frame before trimming,
 * blockflag); `payload` (mg_vorbis_payload_bytes of the page bodies, 4-byte aligned) receives the page bodies back to back.
 * out: (out_frames, channels) float32, frames trim_start .. trim_start + out_frames of the overlap-added stream.  `phases`: bit
 * mask of the launches (1 pages, 2 packets, 4 spectrum, 8 imdct, 16 overlap, 32 status; 63 all).  Workspace (mg_vorbis_ws_bytes)
 * starts with int64 status: [0] first page whose CRC does not check (-1: none), [1] first packet the device refused (-1: none),
 * [2] its reason (1 not an audio packet, 2 mode out of range, 3 blockflag differs from the host's). */
size_t mg_vorbis_payload_bytes(int64_t nbytes);
size_t mg_vorbis_ws_bytes(int64_t packets, int64_t pages, int64_t spec_floats, int channels, int64_t cls_stride);
int mg_vorbis_decode(const void* file, int64_t file_bytes, const int64_t* pages, int64_t npages, int64_t crc_from,
                     const int32_t* setup, const float* fsetup, int channels, int blocksize0, int blocksize1, const int64_t* packets,
                     int64_t npk, void* payload, int64_t payload_bytes, void* ws, size_t ws_bytes, int64_t spec_floats,
                     int64_t cls_stride, float* out, int64_t out_frames, int64_t trim_start, int phases, mg_stream_t stream);

/* ------------------------------------------------------------------ FLAC encoding [torchaudio.save of a .flac path: functions.py:139,
 * th_audio.save]
 * 1-8 channels of `samples` samples at 16 or 24 bits, fixed blocking (4096), STREAMINFO-only streams.  The device writes the frames;
 * the host prepends "fLaC" and STREAMINFO (its MD5 is hashed on the host from `pcm`).  Workspace (mg_flac_enc_ws_bytes) starts
 * with int64 status[16]: [0] bytes of the frames, [1] smallest and [2] largest frame, [3] non-finite input values (nothing written
 * is meaningful when non-zero), [4] the first one's index (channel * samples + sample), [5] non-zero when a frame's packed size
 * disagrees with its analysis (an internal error).
 * Host-only size queries: the workspace, and a bound on the whole file (header + STREAMINFO + frames, every subframe no larger
 * than VERBATIM); the frames' output buffer needs mg_flac_enc_max_bytes - 42 bytes. */
size_t mg_flac_enc_ws_bytes(int64_t samples, int channels);
size_t mg_flac_enc_max_bytes(int64_t samples, int channels, int bits);
/* x: (channels, samples) with rows row_stride elements apart, kind 0 float32 / 1 float64 / 2 int16 (bits 16 only).  Floats are
 * quantised to clamp(rint(x 2^(bits-1)), -2^(bits-1), 2^(bits-1) - 1); writes planar int32 [channels][samples] and pcm, the
 * interleaved little-endian samples of bits / 8 bytes each (STREAMINFO's MD5 input), and resets the status. */
int mg_flac_enc_quantise(const void* x, int kind, int64_t row_stride, int channels, int64_t samples, int bits, int32_t* planar,
                         void* pcm, void* ws, size_t ws_bytes, mg_stream_t stream);
/* analyses and packs every frame of `planar` into out (4-byte aligned, ZERO FILLED, out_bytes >= mg_flac_enc_max_bytes - 42):
 * the frames from byte 0, status [0] bytes long; each frame's CRC-8 and CRC-16 included. */
int mg_flac_enc_frames(const int32_t* planar, int channels, int64_t samples, int bits, int sample_rate, void* ws, size_t ws_bytes,
                       void* out, size_t out_bytes, mg_stream_t stream);

/* ------------------------------------------------------------------ Ogg Vorbis encoding [torchaudio.save of a .ogg path:
 * functions.py:139, th_audio.save]
 * 1-8 channels of `samples` samples, long blocks (2048) only.  The host builds the setup (musicgan_amd/audio/vorbis_encode.py:
 * `tables` int32 codewords / floor posts, `ftables` float32 window, DCT-IV twiddles and dB table, both on the device) and writes
 * the header pages; the device writes the audio pages, numbered from `first_seq`, into out (out_bytes >= mg_vorbis_enc_max_bytes).
 * x: (channels, samples) with rows row_stride elements apart, kind 0 float32 / 1 float64 / 2 int16.  s_db: the floor offset S(q).
 * max_packet_bytes: the longest packet the setup's books can produce.  `phases`: bit mask of the launches (1 analysis, 2 count,
 * 4 layout, 8 pack, 16 pages; 31 all).  Workspace (mg_vorbis_enc_ws_bytes) starts with int64 status[16]: [0] first non-finite
 * input value (channel * samples + sample), [1] first coefficient beyond the books' range ((packet * channels + channel) * 1024
 * + bin), -1 none; [2] packet bytes, [3] bytes of the audio pages, [4] pages, [5] / [6] internal errors (not -1 / 0: page table
 * full, a packet longer than max_packet_bytes). */
size_t mg_vorbis_enc_ws_bytes(int64_t samples, int channels, int64_t max_packet_bytes);
size_t mg_vorbis_enc_max_bytes(int64_t samples, int channels, int64_t max_packet_bytes);
int mg_vorbis_encode(const void* x, int kind, int64_t row_stride, int channels, int64_t samples, float s_db, const int32_t* tables,
                     const float* ftables, int64_t max_packet_bytes, int first_seq, void* ws, size_t ws_bytes, void* out,
                     size_t out_bytes, int phases, mg_stream_t stream);

/* ------------------------------------------------------------------ multi-layer chains on small maps
 * The <= 4x4 ends of both networks -- the generator's first blocks [generator.py:15-40,67-76: conv3x3 -> LeakyReLU -> PixelNorm
 * -> Upsample -> conv3x3 -> LeakyReLU -> PixelNorm] and the critic's last blocks + classifier [discriminator.py:14-34,60-70,
 * 94-101: conv3x3 -> LeakyReLU -> AvgPool2d -> conv3x3 -> LeakyReLU ... -> Flatten -> Linear(160, 1)] -- are ~0.1 GFLOP of work
 * behind 6-10 dependent launches per pass at one launch per layer.  mg_smallnet runs such a chain as ONE launch: a workgroup
 * carries `imgs_per_wg` images through a list of ops with the activations in LDS ([pixel incl. a zero halo ring][channel]), the
 * 3x3 filters streamed from L2 straight into MFMA operand registers (layout of MG_PACK_SMALLNET / mg_smallnet_packed_floats:
 * [Cin/16][9 taps][Cout/16][64 lanes][4], dgrad = 1: the flipped / transposed filters of the data gradient) and every tensor a
 * later pass needs (activations, masks' sources, masked gradients) written to global memory on the way.  The same op list
 * serves the forward passes, the data-gradient chains and the tangent pass of the gradient penalty; weight gradients stay
 * per-layer launches on the stored tensors.  Ops (global tensors are (N, C, H, W) fp32; `src` / `dst` = LDS buffer 0..2):
 *   MG_SN_LOAD     dst <- in                                             (C, H, W)
 *   MG_SN_STORE    out <- src
 *   MG_SN_CONV     dst <- act(conv3x3(src, w) + bias), also -> out       (C -> C2 at H x W; flags MG_SN_LRELU | MG_SN_MASK: act =
 *                  LeakyReLU, or multiplication by lrelu'(aux) = (aux > 0 ? 1 : slope): the tangent pass / LeakyReLU backward)
 *                  1x1 maps take the centre tap in fp64 accumulation (what mg_conv3x3 does there)
 *   MG_SN_MASK     src <- src * lrelu'(aux), also -> out                 (LeakyReLU backward on its own)
 *   MG_SN_PIXNORM  src <- src * rn, rn = 1/sqrt(mean_c src^2 + 1e-8); p -> out, rn -> out2 (N,1,H,W)        [layers.py:11-17]
 *   MG_SN_PNBWD    src <- lrelu'(p) * rn * (src - p * mean_c(src * p)), also -> out;  p = in, rn = aux (PixelNorm + LeakyReLU backward)
 *   MG_SN_POOL     dst <- AvgPool2d(2,2)(src), also -> out               (H, W = input size)
 *   MG_SN_POOLBWD  dst <- 0.25 * up2(src) * lrelu'(aux), also -> out     (H, W = input size; MG_SN_NOLDS: only -> out)
 *   MG_SN_UP       dst <- nearest-upsample x2 of src                     (H, W = input size)
 *   MG_SN_UPBWD    dst <- 2x2 block sums of src                          (H, W = input size)
 *   MG_SN_LINEAR   out[n] <- sum_c w[c] * src[c] + bias[0]               (1x1 map; w = in, bias = aux; fp64 accumulation)
 *   MG_SN_LINBWD   dst[c] <- in[n] * aux[c]                              (in = upstream (N,1), aux = classifier weight)
 * Limits: H, W <= 8 and imgs_per_wg * H * W <= 64 at every CONV, C <= 192, lds_floats_per_buffer * 12 bytes <= 160 KB
 * (mg_smallnet_buffer_floats gives the size one tensor needs).  descs is a HOST array of at most MG_SN_MAX_OPS records. */
enum { MG_SN_LOAD = 0, MG_SN_STORE, MG_SN_CONV, MG_SN_MASK, MG_SN_PIXNORM, MG_SN_PNBWD, MG_SN_POOL, MG_SN_POOLBWD, MG_SN_UP,
       MG_SN_UPBWD, MG_SN_LINEAR, MG_SN_LINBWD };
#define MG_SN_LRELU 1
#define MG_SN_MASK_AUX 2
#define MG_SN_NOLDS 4
#define MG_SN_MAX_OPS 32
typedef struct {
  int32_t op, src, dst, C, C2, H, W, flags;
  const float* in;  /* LOAD: tensor; CONV: packed filters; PNBWD: p; LINEAR: weight; LINBWD: upstream */
  const float* aux; /* CONV: mask source (MG_SN_MASK_AUX); MASK / POOLBWD: mask source; PNBWD: rn; LINEAR: bias; LINBWD: weight */
  const float* bias; /* CONV */
  float* out;
  float* out2; /* PIXNORM: rn */
} mg_sn_op_t;
size_t mg_smallnet_packed_floats(int Cin, int Cout);
size_t mg_smallnet_buffer_floats(int imgs_per_wg, int C, int H, int W);
int mg_smallnet(const mg_sn_op_t* ops, int nops, int N, int imgs_per_wg, size_t lds_floats_per_buffer, float slope,
                mg_stream_t stream);

/* One 3x3 convolution (the nn.Conv2d(3x3) + LeakyReLU / AvgPool2d / Upsample neighbours of mg_conv3x3 above) on maps of at
 * most 16x16 as a latency-optimised launch: a workgroup takes a few images x ONE 16-out-channel tile, its waves split the input
 * channels and have their whole filter share in flight at once (one memory round trip instead of Cin / 8 dependent ones).
 * wpk: MG_PACK_SMALLNET filters (dgrad = 1 for the data gradient).  y (N,Cout,H,W) unless noted; flags:
 *   MG_CONV_UPS_IN     x is (N,Cin,H/2,W/2), nearest-upsampled on the way in [generator.py:26-29]
 *   MG_CONV_LRELU      y = leaky_relu(conv + bias);   MG_CONV_MASK_AUX   y = conv * lrelu'(aux), aux (N,Cout,H,W) (may alias y)
 *   MG_CONV_POOL_OUT   also p (N,Cout,H/2,W/2) = AvgPool2d(2,2)(y) [discriminator.py:24];  y may be NULL
 *   MG_CONV_UPSUM_OUT  also p = 2x2 block SUMS of y (backward of the nearest upsampling in front of the forward conv)
 *   MG_CONV_UNPOOL     alone: y is (N,Cout,2H,2W) = 0.25 * up2(conv) * lrelu'(aux), aux fp32 of that shape (AvgPool2d backward +
 *                      LeakyReLU backward of the layer below; mg_wino3x3's flag of this name takes tile-mask bytes instead) */
#define MG_CONV_UPSUM_OUT 256
int mg_conv3x3_small_supported(int N, int Cin, int Cout, int H, int W);
int mg_conv3x3_small(const float* x, const float* wpk, const float* bias, const float* aux, float* y, float* p, int N, int Cin,
                     int Cout, int H, int W, int flags, float slope, mg_stream_t stream);
/* The same launch with the PixelNorm of the layer in front [layers.py:11-17; generator.py:22-23,38-39: ... LeakyReLU -> PixelNorm
 * -> (Upsample ->) Conv2d] folded into its input staging: x_raw is the UN-normalised activation, y = act(conv(PixelNorm(x_raw)) +
 * bias); pn_p (N,Cin,Hin,Win) and pn_rn (N,1,Hin,Win) receive the normalised activation and 1 / norm (what the backward pass keeps;
 * may be NULL).  flags: MG_CONV_UPS_IN, MG_CONV_LRELU. */
int mg_conv3x3_small_pn(const float* x_raw, const float* wpk, const float* bias, float* y, float* pn_p, float* pn_rn, int N, int Cin,
                        int Cout, int H, int W, int flags, float slope, mg_stream_t stream);

/* ------------------------------------------------------------------ magnitude/phase codec + inverse STFT
 * mg_codec_fwd: stft_to_phase_magn [audio/functions.py:65-94].  stft_c64: interleaved complex64 [512][T] (mg_stft_1024 output);
 * bark_scale: [512] unit-norm bark vector (functions.py:26-35); outputs [S][512][nb_vec], S = (T-1)/nb_vec, both in [-1,1].
 * mg_codec_inv: magn_phase_to_wav [audio/functions.py:97-139] without the file write.  magn_phase: [N][2][512][W];
 * wav_out: [256*(N*W-1)].  The forward unwrap's cumulative sum [functions.py:23] is torch.cumsum's: a float64 running sum
 * rounded to float32 per frame, evaluated as an exact blocked scan (T <= 2^24); the inverse's cumulative phase
 * [functions.py:117-118] is the reference's sequential float32 loop.
 * mg_codec_fwd_strided: the same with consecutive images `img_stride` floats apart (>= 512*nb_vec): with
 * phase_out = magn_out + 512*nb_vec and img_stride = 2*512*nb_vec the outputs ARE the (S, 2, 512, nb_vec) tensor that
 * create_dataset stacks [create_dataset.py:52-58], written once. */
size_t mg_codec_fwd_ws_bytes(int T);
int mg_codec_fwd(const float* stft_c64, const float* bark_scale, float* magn_out, float* phase_out, void* ws,
                 size_t ws_bytes, int T, int nb_vec, mg_stream_t stream);
int mg_codec_fwd_strided(const float* stft_c64, const float* bark_scale, float* magn_out, float* phase_out, size_t img_stride,
                         void* ws, size_t ws_bytes, int T, int nb_vec, mg_stream_t stream);
size_t mg_codec_inv_ws_bytes(int N, int W);
int mg_codec_inv(const float* magn_phase, const float* bark_scale, float* wav_out, void* ws, size_t ws_bytes, int N, int W,
                 mg_stream_t stream);

/* ------------------------------------------------------------------ inverse STFT and Griffin-Lim phase refinement (csrc/griffinlim.hip)
 * What torchaudio.functional.griffinlim (power = 1, rand_init = False) does for users of the reference, on spectra in
 * mg_stft_1024's layout: 512 x TT interleaved complex64, frequency-major, TT = N * W >= 4 frames (definition: DESIGN.md).
 * mg_codec_inv_spectrum: the front half of mg_codec_inv (the same four launches, the same bits).  magn_out [512][TT] receives the
 *   target magnitude M = m / (max m - min m), z_c64 the spectrum mg_codec_inv inverts, or M + 0i if zero_phase != 0 (the phase image
 *   is then not read).
 * mg_istft_1024: the inverse of mg_stft_1024 -- Nyquist row zero, the imaginary part of DC ignored, periodic Hann(1024), hop 256,
 *   times sqrt(sum w^2), overlap-add / window envelope, centre trimmed.  wav_out: [256 * (TT - 1)], 16-byte aligned.  One launch, no
 *   workspace.
 * mg_griffin_lim: with mu = momentum / (1 + momentum) and R_0 = 0, n_iter times: R_k = STFT(ISTFT(Z)), c = R_k - mu R_(k-1),
 *   Z = M c / (|c| + 1e-16); then wav_out = ISTFT(Z).  z_c64 is read (the start) and rewritten (the last Z) if n_iter > 0;
 *   convergence (may be NULL): [n_iter] float64, entry k = || |R_k| - M ||_2 / || M ||_2, float64 sums in a fixed order.  Three
 *   launches per iteration and two at the end, all on `stream`, no allocation and no synchronisation: the call can be captured in
 *   a graph (a single chain) once the library has run on the device.  All pointers 16-byte aligned; 0 <= momentum < 1.
 *   ws_bytes: two spectra (R of the even and of the odd iterations) and the partial sums of every iteration. */
size_t mg_codec_inv_spectrum_ws_bytes(int N, int W);
int mg_codec_inv_spectrum(const float* magn_phase, const float* bark_scale, float* magn_out, float* z_c64, int zero_phase, void* ws,
                          size_t ws_bytes, int N, int W, mg_stream_t stream);
int mg_istft_1024(const float* z_c64, float* wav_out, int TT, mg_stream_t stream);
size_t mg_griffin_lim_ws_bytes(int TT, int n_iter);
int mg_griffin_lim(const float* magn, float* z_c64, float* wav_out, double* convergence, void* ws, size_t ws_bytes, int TT,
                   int n_iter, float momentum, mg_stream_t stream);

/* ------------------------------------------------------------------ phase vocoder (csrc/phasevocoder.hip)
 * torchaudio.functional.phase_vocoder for spectra in mg_stft_1024's layout (512 x frames interleaved complex64, frequency-major,
 * hop 256 of 1024) with a rational rate p / q in [1/8, 8] (above 1: faster and shorter); definition and precision: DESIGN.md.
 * mg_phase_vocoder_len: host only; the output's frames ceil(frames q / p), or -1 for p < 1, q < 1, a rate outside [1/8, 8],
 *   frames < 1 or frames p >= 2^62.
 * mg_phase_vocoder_ws_bytes: host only; 8 bytes per input bin (|X| and arg X, float32) and one float64 per row and tile of 256
 *   output frames; 0 for bad arguments or 2^31 frames and more on either side.
 * mg_phase_vocoder: out_c64 [512][len] receives the re-timed spectrum.  |X| and arg X are torch's float32 values, everything between
 *   them and the final sine / cosine is float64, the phase advance pi k / 2 per frame is applied modulo 2 pi as exact quarter turns
 *   and only the wrapped deviations are summed, in a fixed order: the same bits on every run.  Four launches on `stream`, no
 *   allocation, no synchronisation, no atomics: the call can be captured in a graph.  Spectra 8-byte aligned, ws 16-byte aligned. */
int64_t mg_phase_vocoder_len(int64_t frames, int p, int q);
size_t mg_phase_vocoder_ws_bytes(int64_t frames, int p, int q);
int mg_phase_vocoder(const float* x_c64, float* out_c64, void* ws, size_t ws_bytes, int64_t frames, int p, int q, mg_stream_t stream);
/* The same with identity phase locking (Laroche & Dolson 1999; definition: DESIGN.md, "Phase locking"): every bin follows the
 * nearest peak of its output frame's magnitude and keeps against it the phase difference of the analysis frame.
 * mg_phase_vocoder_locked_ws_bytes: host only; 8 bytes per input bin, 18 per output bin (the peak each bin follows, int16; its phase
 *   step and its magnitude, float64) and 20 per row and tile of 256 output frames; 0 where mg_phase_vocoder_ws_bytes gives 0.
 * mg_phase_vocoder_locked: arguments, checks and error codes of mg_phase_vocoder.  Five launches on `stream` (four up to 256 output
 *   frames), no allocation, no synchronisation, no atomics, one order for every sum: the same bits on every run. */
size_t mg_phase_vocoder_locked_ws_bytes(int64_t frames, int p, int q);
int mg_phase_vocoder_locked(const float* x_c64, float* out_c64, void* ws, size_t ws_bytes, int64_t frames, int p, int q,
                            mg_stream_t stream);

/* ------------------------------------------------------------------ loudness and true peak (csrc/loudness.hip)
 * Programme loudness after ITU-R BS.1770-4 / EBU R128 of a waveform x: C <= 8 rows of L float32 samples, `row_stride` floats apart
 * (definitions: DESIGN.md).  seg = the samples of 100 ms; nseg = L / seg whole segments, the tail is dropped.
 * mg_loudness_chunk: host only; the samples per chunk of the carried filter state.
 * mg_loudness_ws_bytes: host only; four float64 per channel and chunk and one per channel, chunk and segment; 0 for bad arguments.
 * mg_loudness_energy: S [C][nseg] float64 receives the sum of squares of the K-weighted channel over every segment.  coef is a HOST
 *   array of ten float64: b0 b1 b2 a1 a2 of the shelf stage, then of the high-pass stage (a0 = 1); the filter starts from zero state
 *   at sample 0.  States, products and sums are float64; the filtered signal is never written.  Four launches (zero-state end state
 *   of every chunk, the carry s <- A^CHUNK s + z along each channel, the chunks again from their true state, the segments), no
 *   atomics, one order for every sum: the same bits on every run.  nseg == 0: nothing is launched.  ws 16-byte aligned.
 * mg_loudness_gate: weights is a HOST array of C finite non-negative float64.  Block i = segments i .. i + 3, z_i = sum_c
 *   weights[c] (S[c][i] + .. + S[c][i+3]) / (4 seg), l_i = -0.691 + 10 log10 z_i.  record [4] float64 receives: the integrated
 *   loudness -0.691 + 10 log10(mean z over the blocks with l_i > -70 and l_i > G), G = -0.691 + 10 log10(mean z over the blocks
 *   with l_i > -70) - 10, or -inf when nseg < 4 or no block passes -70; max l_i (-inf when nseg < 4); the number of blocks above
 *   -70; the number above both gates.  One launch of one workgroup.
 * mg_true_peak_ws_bytes: host only; one float32 per channel and 2048 samples; 0 for bad arguments.
 * mg_true_peak: peak [1] float32 receives max over channels and samples of max(|x|, |u|), linear, u = x interpolated 4x by the bank
 *   of mg_resample_bank(1, 4, 6, 0.99) (`bank`, on the device) with zeros beyond both ends: the values mg_resample_pcm writes, bit
 *   for bit, reduced without being written.  L >= 1.  Two launches.
 * mg_loudness_normalize: gain [1] float32 receives min(10^((target - record[0]) / 20), 10^(ceiling / 20) / peak[0]) computed in
 *   float64 and rounded once, 1 where record[0] = -inf; out [n] = x [n] * gain (contiguous).  Two launches; record, peak and gain
 *   are device memory.
 * Everything runs on `stream`, allocates nothing and synchronises nothing. */
int mg_loudness_chunk(void);
size_t mg_loudness_ws_bytes(int C, int64_t L, int seg);
int mg_loudness_energy(const float* x, int C, int64_t L, int64_t row_stride, int seg, const double* coef, double* S, void* ws,
                       size_t ws_bytes, mg_stream_t stream);
int mg_loudness_gate(const double* S, const double* weights, int C, int64_t nseg, int seg, double* record, mg_stream_t stream);
size_t mg_true_peak_ws_bytes(int C, int64_t L);
int mg_true_peak(const float* x, int C, int64_t L, int64_t row_stride, const void* bank, size_t bank_bytes, float* peak, void* ws,
                 size_t ws_bytes, mg_stream_t stream);
int mg_loudness_normalize(const float* x, float* out, int64_t n, const double* record, const float* peak, double target,
                          double ceiling, float* gain, mg_stream_t stream);

/* ------------------------------------------------------------------ look-ahead true-peak limiter (csrc/limiter.hip)
 * One gain curve g [L] for all C <= 8 rows of x (L float32 samples, `row_stride` floats apart) that keeps every sample of x G g at
 * or under the ceiling c (definition, steps 1 - 6: DESIGN.md).  A = look-ahead in samples, 0 .. 2047; rho in (0, 1) = release
 * factor per sample; G = pregain[0], one float64 in DEVICE memory, read by the kernels.  `bank`: mg_resample_bank(1, 4, 6, 0.99)
 * on the device.
 * mg_limiter_tile: host only; the samples per workgroup of the hold, release and output kernels.
 * mg_limiter_ws_bytes: host only; one float32 per sample (m), one float64 per tile of L + A positions and one per position (q), each
 *   part rounded up to 16 bytes, + 16; 0 for bad arguments.
 * mg_limiter_envelope: m [L] float32 receives max over the channels of max(|x[n]|, |u[4n - 3 .. 4n + 3]|), u = x interpolated 4x by
 *   the bank with zeros beyond both ends (the values mg_resample_pcm writes, bit for bit; u outside [0, 4 L) does not count).  One
 *   launch.
 * mg_limiter: out [C][L] float32 (contiguous) receives float32(double(x) G g), rounded once; gain_out (optional) [L] float64 receives
 *   g.  r = c / (G m) where G m > c, else 1; h[n] = min r[n .. n + A]; d[n] = max(1 - h[n], rho d[n - 1]) from d = 0 A samples before
 *   the file, carried along the whole file; g[n] = min(r[n], mean of 1 - d over n - A .. n).  Everything but m is float64.  Five
 *   launches (envelope, end state of every tile from zero state, the carry along the tiles, the tiles again from their true state,
 *   window means and output), no atomics, one order for every scan and sum: the same bits on every run.  |out| <= c (1 + 2^-23);
 *   where G m <= c everywhere g is exactly 1.  L == 0: nothing is launched.  ws 16-byte aligned, pregain and gain_out 8-byte.
 * mg_limiter_trim: out [n] = float32(double(y [n]) min(1, ceiling / peak[0])), peak the float32 of mg_true_peak on the device.
 * mg_limiter_pregain: pregain [1] float64 receives prev[0] 10^((target - record[0]) / 20) (prev == NULL: 1), the factor 1 where
 *   record[0] = -inf; record of mg_loudness_gate, all of it device memory.  One launch of one thread.
 * Everything runs on `stream`, allocates nothing and synchronises nothing: the calls can be captured in a graph. */
int mg_limiter_tile(void);
size_t mg_limiter_ws_bytes(int C, int64_t L, int A);
int mg_limiter_envelope(const float* x, int C, int64_t L, int64_t row_stride, const void* bank, size_t bank_bytes, float* m,
                        mg_stream_t stream);
int mg_limiter(const float* x, int C, int64_t L, int64_t row_stride, const void* bank, size_t bank_bytes, const double* pregain,
               double ceiling, int A, double rho, float* out, double* gain_out, void* ws, size_t ws_bytes, mg_stream_t stream);
int mg_limiter_trim(const float* y, float* out, int64_t n, const float* peak, double ceiling, mg_stream_t stream);
int mg_limiter_pregain(const double* record, double target, const double* prev, double* pregain, mg_stream_t stream);

/* CRC-32 (zip / zlib) of the float64 widening of float32 samples: crc_out[i] = crc32 of the little-endian bytes of
 * x[i*floats_per_sample ...].astype(float64) -- the checksum the zip container of `th.save(sample.to(th.float64))`
 * [create_dataset.py:52-62] stores for its payload, which the reference's writer computes on one host core per sample.
 * floats_per_sample = 8192 x a power of two <= 256 (a (2,512,512) sample: 524 288).  ws: mg_crc32_f64_ws_bytes. */
size_t mg_crc32_f64_ws_bytes(int n, int64_t floats_per_sample);
int mg_crc32_f64(const float* x, uint32_t* crc_out, void* ws, size_t ws_bytes, int n, int64_t floats_per_sample, mg_stream_t stream);

/* HOST function (no GPU work): the writer threads' per-sample work of create_dataset [create_dataset.py:52-62, th.save(magn_phase.to(
 * th.float64), path)] for n consecutive float32 samples `rows` (row_floats each, e.g. a slice of a pinned chunk): widen to float64 and
 * write file i as  prefix | float64 payload | suffixes[i*suffix_len ...]  (the zip container of th.save around the payload, from
 * musicgan_amd.fast_pt.PtTemplate) to the i-th NUL-terminated path in `paths`; side_fd >= 0: also pwrite the float32 row at
 * side_off + i * row_floats * 4 of that file (the fast loader's side-car).  Thread-safe; bound through ctypes it runs without the
 * interpreter lock. */
int mg_pt_write_samples(const float* rows, int n, int64_t row_floats, const char* paths, const unsigned char* prefix, int64_t prefix_len,
                        const unsigned char* suffixes, int64_t suffix_len, int side_fd, int64_t side_off);
/* Measurement helper (bench.py `host_io_probe`, no GPU work): what one writer thread's sample costs the host as plain system calls
 * -- n x { new file of file_bytes from a zero buffer; pwrite of side_bytes } and n x { row_floats float32 -> float64 } -- timed
 * separately; called from several threads at once.  The files <dir>/probe_raw_<tid>_<i>.bin, probe_rawside_<tid>.bin are left. */
int mg_host_io_probe(const char* dir, int tid, int n, int64_t file_bytes, int64_t side_bytes, const float* src, int64_t row_floats,
                     double* write_seconds, double* widen_seconds);

/* Per-batch input transform of the training loop, fused: ChannelMinMaxNorm -> ChangeRange(-1,1) -> Resize(S) (bilinear with
 * anti-aliasing, align_corners = False: torchvision's tensor path) [audio/transforms.py:4-40, utils.py:70-86, train.py:138-140].
 * x (N,2,H,W) float64 (x_is_f64 != 0: cast to float32 on read, == x.to(th.float)) or float32; out (N,2,S,S) float32, S <= H, W. */
size_t mg_input_transform_ws_bytes(int N, int H, int W, int S);
int mg_input_transform(const void* x, int x_is_f64, float* out, void* ws, size_t ws_bytes, int N, int H, int W, int S, float eps,
                       mg_stream_t stream);
/* The same transform on windows cut out of a resident array: base holds `rows` samples (2,H,W) float32; row_a, row_b, off are DEVICE
 * int32 arrays of length N.  Sample n is, for each channel and row, columns [off[n], W) of base[row_a[n]] followed by columns
 * [0, off[n]) of base[row_b[n]] (where off[n] == 0, row_b[n] is never read and may be -1); out (N,2,S,S) is bit for bit what
 * mg_input_transform gives on that window laid out in memory.  Two launches, no host read: the indices may be uploaded long before.
 * The kernels TRUST the indices (0 <= row < rows, 0 <= off < W): the caller validates them on the host.  All addressing is 64-bit. */
size_t mg_input_transform_windows_ws_bytes(int N, int H, int W, int S);
int mg_input_transform_windows(const float* base, int64_t rows, const int32_t* row_a, const int32_t* row_b, const int32_t* off,
                               float* out, void* ws, size_t ws_bytes, int N, int H, int W, int S, float eps, mg_stream_t stream);

/* Sliced Wasserstein distance between patches of Laplacian-pyramid levels (Karras et al., ICLR 2018): the evaluation metric of
 * musicgan_amd/metrics.py, which the reference does not have (definition: DESIGN.md).  All float32 unless said otherwise.
 * pyr_down: x (NC,H,W) -> out (NC,H/2,W/2), the 5x5 binomial filter with mirrored borders sampled at even positions.
 * pyr_lap:  out = x - up(coarse), coarse (NC,H/2,W/2); up = zero-stuffing then 4x the same filter.  H, W even and >= 4.
 * gather:   level (N,C,H,W) + centres (N,P,2) int32 (row, column; clamped to the legal range) -> rows row0 .. row0 + N*P of the
 *           (rows_total, C*patch*patch) descriptor buffer, and (sum, sum of squares) of every image and channel in float64 at
 *           stats[(row0/P + n), c, 0..1]; row0 a multiple of P.
 * stats_finish: the (images, C, 2) float64 pairs -> norm (C,3) = (mean, 1/std, std) over images*per_image values per channel.
 * project:  out (D,M), out[d][m] = sum_k ((desc[m][k] - mean_c) * rstd_c) * dirs[d][k], dirs (D,K), K = C*patch*patch.
 * sort_segments: ascending in-place sort of S contiguous segments of M keys; finite values and +-inf (NaN: unspecified order).
 * distance: out[0] = mean |a[i] - b[i]| over n values, summed in float64 in an order that depends on n alone. */
int mg_swd_pyr_down(const float* x, float* out, int NC, int H, int W, mg_stream_t stream);
int mg_swd_pyr_lap(const float* x, const float* coarse, float* out, int NC, int H, int W, mg_stream_t stream);
int mg_swd_gather(const float* level, const int32_t* centres, float* desc, double* stats, int N, int C, int H, int W, int P, int patch,
                  int64_t row0, int64_t rows_total, mg_stream_t stream);
int mg_swd_stats_finish(const double* stats, float* norm, int64_t images, int C, int64_t per_image, mg_stream_t stream);
int mg_swd_project(const float* desc, const float* norm, const float* dirs, float* out, int64_t M, int C, int patch, int D,
                   mg_stream_t stream);
int mg_swd_sort_segments(float* x, int S, int64_t M, mg_stream_t stream);
size_t mg_swd_distance_ws_bytes(int64_t n);
int mg_swd_distance(const float* a, const float* b, int64_t n, float* out, void* ws, size_t ws_bytes, mg_stream_t stream);

/* Multi-scale structural similarity between pairs of images a, b (N,C,H,W) float32 in [-1, 1]: the sample-diversity metric of
 * musicgan_amd/metrics.py, which the reference does not have (definition: DESIGN.md).  HOST queries (no GPU work): scales (0 when a
 * side is below 11), window (the 11 float32 taps), tiles (workgroups per channel plane of an H x W level), scratch_bytes (the slots
 * of every scale plus both images of every coarser scale).
 * scale:  one scale of N pairs.  slots (N,C,tiles(H,W),2) float64 receives every tile's sums of cs and of ssim over its valid
 *         pixels; a_next / b_next (N,C,H/2,W/2), both or none, receive the 2x2 means (H, W even), the next scale's input.
 * finish: slots = the regions of the scales 0 .. S-1 of an H x W image one after the other, slot_doubles values in all -> values[row0
 *         + n] = prod_s max(mean_s, 0)^w_s and, where terms != NULL, terms[(row0 + n), s] = mean_s (the CS mean of every scale but
 *         the last, whose SSIM mean it is), in float64; added in index order.
 * mean:   out[0] = the mean of n float64 values, added in an order that depends on n alone. */
int mg_ssim_scales(int H, int W);
int mg_ssim_window(float* taps);
int64_t mg_ssim_tiles(int H, int W);
size_t mg_ssim_scratch_bytes(int64_t N, int C, int H, int W);
int mg_ssim_scale(const float* a, const float* b, float* a_next, float* b_next, double* slots, int64_t N, int C, int H, int W,
                  mg_stream_t stream);
int mg_ssim_finish(const double* slots, size_t slot_doubles, int64_t N, int C, int H, int W, double* values, double* terms,
                   int64_t row0, int64_t rows_total, mg_stream_t stream);
int mg_ssim_mean(const double* values, int64_t n, double* out, mg_stream_t stream);

/* ---- nearest neighbours in pixel space (csrc/nn.hip): squared L2 distances between rows of D float32 numbers, the kernels behind
 * musicgan_amd/nn_ops.py and metrics.NearestNeighbours, which the reference does not have (definition: DESIGN.md).  HOST queries (no
 * GPU work): chunk (the components one wave accumulates in float32, a compile-time constant), ws_bytes (the float32 partial sums of
 * one sqdist launch: chunks x nq x nr).
 * sqnorm: out[n] = sum_d x[n][d]^2 in float64, added in an order that depends on D alone.
 * sqdist: dist[i][j] = max(0, qn[i] + rn[j] - 2 sum_d q[i][d] r[j][d]) in float64; q (nq,D), r (nr,D) row-major, qn / rn their
 *         sqnorm.  The dot product is accumulated in float32 (exact-fp32 MFMA) inside chunks of D and in float64 across them, in
 *         an order that depends on D alone: a pair's value does not depend on nq, nr or the rows around it.  Any nq, nr, D >= 1.
 * merge:  best_d / best_i (nq,k): every query's k nearest so far, ascending by (distance, id); an empty slot is (DBL_MAX, -1).  The
 *         nr candidates of dist (nq,nr) with the ids rid[nr] are inserted; a candidate whose id equals qid[i] >= 0 is skipped (qid
 *         may be NULL: no query has an id).  1 <= k <= 16. */
int mg_nn_chunk(void);
size_t mg_nn_ws_bytes(int64_t nq, int64_t nr, int64_t D);
int mg_nn_sqnorm(const float* x, int64_t n, int64_t D, double* out, mg_stream_t stream);
int mg_nn_sqdist(const float* q, const float* r, const double* qn, const double* rn, int64_t nq, int64_t nr, int64_t D, double* dist,
                 void* ws, size_t ws_bytes, mg_stream_t stream);
int mg_nn_merge(const double* dist, const int64_t* qid, const int64_t* rid, double* best_d, int64_t* best_i, int64_t nq, int64_t nr,
                int k, mg_stream_t stream);

/* ---- precision / recall / density / coverage (csrc/prdc.hip): the kernels behind nn_ops.nn_sqdist_tiled / prdc_scan and
 * metrics.PRDC, which the reference does not have (definition: DESIGN.md 4.14).
 * tiled_ws_bytes: HOST query, the float64 slice sums of one sqdist_tiled launch: 16 x nq x nr, whatever D is.
 * sqdist_tiled:   mg_nn_sqdist's arguments and, bit for bit, its output for any nq, nr, D >= 1 and any alignment of the rows: the same
 *                 float32 chains inside chunks and the same float64 order across them, with the operand rows staged in LDS and shared
 *                 by 128 x 128 pairs.  All of dist (nq,nr) is written; ws must be 8-byte aligned.
 * scan:           for every row i of dist (nq,nr) float64: count[i] += #{ j : dist[i][j] <= radius[j] } (int64) and rowmin[i] =
 *                 min(rowmin[i], min_j dist[i][j]), both accumulated in place, so a matrix may go through in column blocks.  One
 *                 writer per row, no atomics: counts are integers and the minimum is exact, so the blocking does not show. */
size_t mg_nn_tiled_ws_bytes(int64_t nq, int64_t nr, int64_t D);
int mg_nn_sqdist_tiled(const float* q, const float* r, const double* qn, const double* rn, int64_t nq, int64_t nr, int64_t D,
                       double* dist, void* ws, size_t ws_bytes, mg_stream_t stream);
int mg_prdc_scan(const double* dist, const double* radius, int64_t* count, double* rowmin, int64_t nq, int64_t nr, mg_stream_t stream);

/* ---- DiffAugment (csrc/diffaug.hip, csrc/diffaug_plan.h): one random translation with zero fill and one random cutout per sample,
 * applied to every image the critic sees, and the adjoint for the generator's gradient (definition: DESIGN.md 4.13; the kernels behind
 * musicgan_amd/aug_ops.py).  x, y, gy, gx are (n, c, h, w) float32; u is (n, 8) float32 in [0, 1) in DEVICE memory, read by the kernel:
 * nothing about it is known to the host, so a captured launch follows whatever u holds when it is replayed.  Columns of u: 0 translation
 * on iff < p, 1 / 2 its dy / dx, 3 cutout on iff < p, 4 / 5 its centre, 6 / 7 reserved.  ops: MG_DIFFAUG_* bits; 0 <= p <= 1.
 * fwd:    y = T x.  One launch; any n, c, h, w >= 1; all of y is written.
 * bwd:    gx = T^t gy, likewise.
 *         Every output element is a copy of one input element or +0.0 (a select): both are bit-exact, and NaN / inf that the mask or
 *         the border drops never reach the output.  Source and destination (and u and the destination) must not overlap: MG_EINVAL
 *         before anything is launched.
 * decode: HOST only, u in host memory: out[i] = {dy, dx, y0, y1, x0, x1} of sample i -- T x[i, j] = x[i - dy, j - dx], rows [y0, y1) x
 *         columns [x0, x1) zeroed (all 0: no box) -- through the function the kernels call. */
#define MG_DIFFAUG_TRANSLATION 1
#define MG_DIFFAUG_CUTOUT 2
int mg_diffaug_fwd(const float* x, const float* u, int n, int c, int h, int w, int ops, float p, float* y, mg_stream_t stream);
int mg_diffaug_bwd(const float* gy, const float* u, int n, int c, int h, int w, int ops, float p, float* gx, mg_stream_t stream);
int mg_diffaug_decode(const float* u_host, int n, int h, int w, int ops, float p, int32_t* out);

/* ---- k-means bins for NDB / JSD (csrc/kmeans.hip): the kernels behind musicgan_amd/km_ops.py and metrics.KMeans / metrics.NDB, which
 * the reference does not have (definition: DESIGN.md 4.15).  The distances of a Lloyd iteration are mg_nn_sqdist_tiled's; these are the
 * rest.  1 <= k <= 1024 everywhere; labels are int32 bin numbers; nothing is read back to the host and nothing is allocated.
 * assign:          for every row i of dist (n,k) float64: label[i] = the column of the row's smallest entry (ties: the smaller column),
 *                  mind[i] = that entry; changed[0] (int64) = the number of rows whose label was rewritten with a different value,
 *                  overwritten, not accumulated.
 * order:           the positions 0 .. n-1 sorted by (label, position) into order (n,) int32, and the exclusive prefix sums of the bin
 *                  sizes into start (k+1,) int32; every element of both is written (positions whose label is outside 0 .. k-1 come
 *                  last, behind start[k]).  n <= 2^20, MG_EINVAL beyond.
 * update_ws_bytes: HOST query, the float64 partial sums of one update: (n / 32 + k) x d.
 * update:          centroid[j] (k,d) float32 = the float64 sum of x's rows order[start[j] .. start[j+1]) in that order, in chunks of 32
 *                  members added in chunk order, divided in float64 by the member count and rounded once to float32; a bin without
 *                  members keeps its centroid.  A centroid depends on its ordered member list alone.  16-byte loads when d % 4 == 0 and
 *                  x is 16-byte aligned, element-wise loads otherwise.  n <= 2^20.
 * count:           count[label[i]] += 1 for every i (count (k,) int64, accumulated in place; labels outside 0 .. k-1 are skipped). */
int mg_km_assign(const double* dist, int64_t n, int k, int32_t* label, double* mind, int64_t* changed, mg_stream_t stream);
int mg_km_order(const int32_t* label, int64_t n, int k, int32_t* start, int32_t* order, mg_stream_t stream);
size_t mg_km_update_ws_bytes(int64_t n, int64_t d, int k);
int mg_km_update(const float* x, int64_t n, int64_t d, const int32_t* order, const int32_t* start, int k, float* centroid, void* ws,
                 size_t ws_bytes, mg_stream_t stream);
int mg_km_count(const int32_t* label, int64_t n, int k, int64_t* count, mg_stream_t stream);

/* ---- multi-scale L2 loss with its gradient (csrc/pyrloss.hip, plan: csrc/pyrloss_plan.h): the kernels behind
 * musicgan_amd/proj_ops.py, networks.PyramidL2 and the latent projector, which the reference does not have (definition: DESIGN.md 4.16).
 * x, t (n, c, h, w) float32; `levels` L in 1 .. 7, h and w multiples of 2^(L-1); weights: HOST array of L finite floats >= 0, read
 * before the call returns and passed to the kernels by value.
 *   d_0 = x - t;  d_{s+1} = AvgPool2d(2)(d_s) in mg_avgpool2_fwd's float32 expression
 *   loss[i] = sum_s weights[s] / (c h_s w_s) * sum (double)d_s^2 over sample i     (n,) float64; fixed order, no atomics
 *   grad    = d loss[i] / d x = ((weights[L-1] d_{L-1}, then fmaf(weights[s], d_s, .) for s = L-2 .. 0) * (float)(2 / (c h w)))
 *             (n, c, h, w) float32, or NULL: the loss alone.  It must not overlap x or t (x and t may be the same buffer).
 * Two launches on `stream`, nothing read back, capturable.  A sample's loss and gradient depend on that sample alone and have the
 * same bits in every run and for every split of the batch.  ws: mg_pyramid_l2_ws_bytes (0: the shape is refused) at an 8-byte
 * boundary, fully written. */
size_t mg_pyramid_l2_ws_bytes(int n, int c, int h, int w, int levels);
int mg_pyramid_l2(const float* x, const float* t, int n, int c, int h, int w, int levels, const float* weights, double* loss,
                  float* grad, void* ws, size_t ws_bytes, mg_stream_t stream);

/* ---- harmonic / percussive separation and overlap-add re-timing (csrc/hpss.hip): the kernels behind musicgan_amd/hpss_ops.py,
 * audio.hpss / harmonic / percussive and the transient-preserving time stretch, which the reference does not have (definition:
 * DESIGN.md 4.17).  x_c64 (512, frames) interleaved complex64 in mg_stft_1024's layout, frames >= 1.
 *   S = |x| (float32, torch's bits);  Hm[k,t] = median of S[k, t - (lh-1)/2 .. t + (lh-1)/2];  Pm[k,t] = median of
 *   S[k - (lp-1)/2 .. k + (lp-1)/2, t];  indices past an end reflected (j -> r = j mod 2 n, r < n ? r : 2 n - 1 - r);
 *   softmask(A, B) = A > B for power = infinity; else with Z = max(A, B): Z < 2^-126 ? (both margins 1 ? 1/2 : 0) :
 *   (A/Z)^power / ((A/Z)^power + (B/Z)^power);   mask_h = softmask(Hm, margin_h Pm),  mask_p = softmask(Pm, margin_p Hm);
 *   harm = x mask_h,  perc = x mask_p.
 * lh, lp odd in [3, 63]; power 1, 2 or INFINITY; margins finite and >= 1.  Each of the six outputs (harm, perc (512, frames)
 * complex64; H, P, mask_h, mask_p (512, frames) float32) is written when its pointer is given, at least one must be; none may overlap
 * x.  One launch on `stream`, no workspace, no allocation, no synchronisation, no atomics: capturable.  A median is a selection and
 * a bin depends on its own windows alone: the same bits in every run, whatever surrounds the windows.
 * mg_ola_stretch: y[256 m + j] = w[j] xz[a_m + j] + w[j + 256] xz[a_{m-1} + j + 256] for 0 <= j < 256 and 256 m + j < out_length, with
 *   a_m = floor(256 m p / q) in 64-bit integers, a_{-1} = -256, xz = x inside [0, length) and 0 outside, w[i] = (1 - cos(2 pi i /
 *   512)) / 2 computed in float64 and rounded once.  p / q in [1/8, 8], length >= 1, out_length >= 0, out_length p < 2^62.  One
 *   launch, a gather: nothing is accumulated across threads. */
int mg_hpss(const float* x_c64, float* harm_c64, float* perc_c64, float* H, float* P, float* mask_h, float* mask_p, int64_t frames,
            int lh, int lp, float power, float margin_h, float margin_p, mg_stream_t stream);
int mg_ola_stretch(const float* x, int64_t length, float* y, int64_t out_length, int p, int q, mg_stream_t stream);

/* ---- log-mel feature rows and float64 moments (csrc/logmel.hip, csrc/moments.hip): the kernels behind musicgan_amd/mel_ops.py,
 * metrics.LogMel and metrics.Frechet, which the reference does not have (definition: DESIGN.md 4.19).
 * logmel_rows: x (n, channels, h, w) float32, rows = frequency, columns = time; scale (h,), weight (bands, h) float32 on the device;
 *   lo, hi: HOST arrays of `bands` row limits, 0 <= lo <= hi <= h, read before the call returns and passed to the kernel by value
 *   (MG_EINVAL otherwise: no row index depends on device memory); bands <= 256; `pools` divides w, w / pools <= 1024; floor > 0.
 *     p[h,t] = (x[i,c,h,t] scale[h] + scale[h])^2                  float32, every operation rounded
 *     s[m,t] = sum_{h = lo[m]}^{hi[m]-1} weight[m,h] p[h,t]         float32, ascending h, product and sum rounded apart
 *     v[m,t] = log((double)s[m,t] + floor)                          float64
 *     out[i, m pools + j] = (float)(sum of v[m,t] over the w / pools columns of pool j in ascending t, / (w / pools))
 *   out (n, bands pools) float32, every element written; weights outside [lo, hi) are not read.  One launch per 32 768 images on
 *   `stream`, no workspace, no atomics, capturable.  A row of out depends on its image and on the shapes alone.
 * moments_ws_bytes: HOST query, the float64 partial sums of mg_moments: ceil(n / 1024) x (d + d d) x 8 (0: the shape is refused).
 * moments: rows (n, d) float32, 2 <= n <= 2^24, 1 <= d <= 4096 -> mean (d,) and cov (d, d) float64, two passes in float64:
 *     mean_j = (sum_i x_ij) / n;   cov_jk = sum_i (x_ij - mean_j)(x_ik - mean_k) / (n - 1)
 *   Sums run over chunks of 1024 rows in ascending order from +0.0 and the chunk sums are added in chunk order: the same bits in every
 *   run.  All of cov is written and cov[j,k] and cov[k,j] hold the same bits.  Four launches on `stream`, no atomics, capturable; ws
 *   at an 8-byte boundary; the part of it that is read was written by the same call. */
int mg_logmel_rows(const float* x, int n, int channels, int c, int h, int w, const float* scale, const float* weight,
                   const int32_t* lo, const int32_t* hi, int bands, double floor, int pools, float* out, mg_stream_t stream);
size_t mg_moments_ws_bytes(int64_t n, int64_t d);
int mg_moments(const float* rows, int64_t n, int64_t d, double* mean, double* cov, void* ws, size_t ws_bytes, mg_stream_t stream);

/* ---- Kernel Inception Distance (csrc/kid.hip): the kernels behind musicgan_amd/kid_ops.py, metrics.poly_mmd2 and metrics.KID, which
 * the reference does not have (definition and error bound: DESIGN.md 4.20).
 * standardise_rows: x (n, d) float32, mean (d,) and sd (d,) float64 -> out (n, d) float32, every element written:
 *     out[i,j] = (float)(((double)x[i,j] - mean[j]) / sd[j]), and 0 where sd[j] is 0, infinite or NaN.
 *   One launch, one element per thread; bit-equal to the float64 definition.
 * polyk_ws_bytes: HOST query, the partial row sums of mg_polyk_rowsums: subsets x ceil(mb / 128) x ma x 8 (0: the shape is refused).
 * polyk_rowsums: a (na, d) and b (nb, d) float32, d <= 4096; ia (subsets, ma) and ib (subsets, mb) int32 row numbers in DEVICE
 *   memory, NULL = 0 .. m - 1 for every subset (then m <= n); the rows are gathered while they are staged.  A row number outside its
 *   operand is clamped into it, so no list can make a read leave a or b.  out (subsets, ma) float64, every element written:
 *     out[s,i] = sum over j = 0 .. mb - 1 of k(a[ia[s,i]], b[ib[s,j]]),   k(x, y) = (x.y / d + 1)^3,
 *   without the pairs j = i if skip_diag (which needs ma = mb).  x.y is taken in chunks of 256 components, each a float32 chain from
 *   zero on v_mfma_f32_16x16x4_f32 (the chunk discipline of mg_nn_sqdist_tiled), the chunks are added in float64 in ascending
 *   order, and the division, the cube and every sum over pairs are float64 in an order the column positions alone fix: out[s,i] is
 *   a function of its row of a, the ordered list of b rows of subset s, d and skip_diag (and, with skip_diag, of i) -- not of ma,
 *   of `subsets`, of the other subsets or of the other rows of a -- and the same bits in every run.  The kernel matrix is never
 *   stored.  Two launches on `stream` (tiles, then the sum over the column blocks), no atomics, capturable; subsets <= 65535;
 *   ws at an 8-byte boundary; the part of it that is read was written by the same call. */
int mg_standardise_rows(const float* x, int64_t n, int64_t d, const double* mean, const double* sd, float* out, mg_stream_t stream);
size_t mg_polyk_ws_bytes(int64_t subsets, int64_t ma, int64_t mb);
int mg_polyk_rowsums(const float* a, int64_t na, const float* b, int64_t nb, const int32_t* ia, const int32_t* ib, int64_t subsets,
                     int64_t ma, int64_t mb, int64_t d, int skip_diag, double* out, void* ws, size_t ws_bytes, mg_stream_t stream);

/* ---- mel power spectrogram of waveforms and pooled log rows (csrc/melspec.hip): the kernels behind mel_ops.mel_power,
 * mel_ops.logmel_pool, audio.mel_spectrogram and metrics.WaveLogMel, which the reference does not have (definition and error bound:
 * DESIGN.md 4.21).
 * mel_power: wave holds `rows` signals of `length` float32 mono samples, row_stride >= length samples apart; length > 512; weight
 *   (bands, 512) float32 on the device; lo, hi: HOST arrays of `bands` bin limits, 0 <= lo <= hi <= 512, read before the call returns
 *   and passed to the kernel by value (MG_EINVAL otherwise: no index depends on device memory); bands <= 256.  With
 *   T = 1 + length / 256 and X[k,t] the value of mg_stft_1024 for the row (reflect padding by 512, periodic Hann / sqrt(384),
 *   k = 0 .. 511, Nyquist dropped):
 *     p[k,t] = re re + im im                                          float32, every operation rounded, no fma
 *     s[m,t] = sum_{k = lo[m]}^{hi[m]-1} weight[m,k] p[k,t]           float32, ascending k from +0.0, product and sum rounded apart
 *   out (rows, bands, T) float32, every element written (an empty band: +0.0); weights outside [lo, hi) are not read.  One launch
 *   on `stream`; the spectrum is never written; no workspace, no atomics, capturable.  A row of out depends on its signal alone.
 * logmel_pool: power (rows, bands, frames) float32; windows of `win` frames every `hop` frames, W = (frames - win) / hop + 1 per
 *   row (win <= frames; the tail is dropped); `pools` divides win; floor > 0.  out (rows W, bands pools) float32, every element written:
 *     out[b W + n, m pools + j] = (float)(sum of log((double)power[b,m,t] + floor) over the win / pools frames
 *                                         t = n hop + j win / pools .. of pool j, in ascending t, / (win / pools))
 *   in float64, rounded once.  One launch, one thread per number, no workspace, no atomics, capturable. */
int mg_mel_power(const float* wave, int64_t rows, int64_t length, int64_t row_stride, const float* weight, const int32_t* lo,
                 const int32_t* hi, int bands, float* out, mg_stream_t stream);
int mg_logmel_pool(const float* power, int64_t rows, int bands, int64_t frames, int win, int hop, int pools, double floor, float* out,
                   mg_stream_t stream);

/* ---- perceptual path length (csrc/ppl.hip): the kernels behind musicgan_amd/ppl_ops.py and metrics.PPL, which the reference does
 * not have (definition and error bounds: DESIGN.md 4.22).
 * slerp_pairs: z0, z1 (n, d) float32, t (n) float64, any d >= 1.  za[i] = slerp(z0[i], z1[i], t[i]) and zb[i] = slerp(z0[i], z1[i],
 *   t[i] + eps), both (n, d) float32, with slerp the definition of project.slerp: each row one flat vector, float64 arithmetic, the
 *   straight line (1 - t) a + t b below an angle of 1e-6 (equal or nearly parallel rows, a zero row), one rounding to float32;
 *   t[i] = 0 gives za[i] = z0[i] bit for bit.  flag (n) int32: 1 where the angle is within 1e-6 of pi (no single shortest arc), and
 *   za[i], zb[i] are then +0.0; else 0.  Every element of za, zb and flag is written.  |z0|^2, |z1|^2 and z0.z1 are float64 sums in
 *   an order that depends on d alone (lane l of the pair's wave adds the components 4 l .. 4 l + 3, 4 l + 256 .. in ascending order,
 *   then one butterfly over the 64 lanes), the same whether the rows are 16-byte aligned or not; the same bits in every run and for
 *   any n.  One launch, one wave per pair, no workspace, no atomics, capturable.
 * rows_sqdist: a, b (n, d) float32 -> out (n) float64, every element written:
 *     out[i] = scale * sum_j ((double)a[i,j] - (double)b[i,j])^2
 *   in the same fixed order (one wave per pair): out[i] is a function of its two rows, d and scale alone -- not of n or of the other
 *   rows -- and the same bits in every run; exactly 0 for equal finite rows; a NaN or an infinity stays in its pair.  One launch, no
 *   workspace, no atomics, capturable. */
int mg_slerp_pairs(const float* z0, const float* z1, const double* t, int64_t n, int64_t d, double eps, float* za, float* zb,
                   int32_t* flag, mg_stream_t stream);
int mg_rows_sqdist(const float* a, const float* b, int64_t n, int64_t d, double scale, double* out, mg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
