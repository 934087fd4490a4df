/*
 * vits_amd.h — C-ABI of the MI355X (gfx950) VITS hot path.
 *
 * Every entry point takes plain device pointers, sizes and a hipStream_t
 * passed as `void*` (NULL = default stream).  No torch types cross this
 * boundary; ownership of every buffer stays with the caller (the PyTorch
 * caching allocator on the Python side).  All calls are asynchronous on the
 * given stream, never synchronise the host, and return 0 on success or a
 * negative VITS_E* code on a shape/argument error (checked on the host
 * before anything is launched) or a hipError_t (positive) from the launch.
 *
 * Reference interfaces replaced (paths relative to emotional-vits/):
 *   vits_maximum_path        monotonic_align.maximum_path, call site
 *                            models.py:498 (external Cython package
 *                            `monotonic-align`, not vendored)
 *   vits_neg_cent            the alignment scores of SynthesizerTrn.forward
 *                            (models.py:483-490: exp, 2 matmuls, 2 sums)
 *   vits_conv1d_forward      nn.Conv1d / ConvTranspose1d forward of
 *                            modules.WN (modules.py:130-182),
 *                            modules.ResBlock2 (modules.py:250-260),
 *                            models.Generator (models.py:306-318),
 *                            ResidualCouplingLayer.infer (modules.py:362-375)
 *                            with their elementwise tails fused in
 *   vits_linear_forward      per-utterance nn.Linear conditioning of
 *                            WN.cond_layer (modules.py:109-110,139),
 *                            ResBlock2.conds (modules.py:243-245,253),
 *                            FFN2.cond (attentions.py:143,152)
 *   vits_expand_prior        the prior-expansion matmuls + noise of
 *                            SynthesizerTrn.infer_p2 (models.py:569-571)
 *   vits_conv_post_tanh      Generator tail: leaky_relu(0.01) -> conv_post
 *                            -> tanh (models.py:315-317)
 *   vits_stft_mag_forward /  TorchSTFT.stft + STFTLoss.spec2mag
 *   vits_stft_mag_backward   (modules.py:386-392, stft_loss.py:22-23);
 *   (_multi)                 all resolutions of MultiResolutionSTFTLoss
 *                            (stft_loss.py:47-95) in one launch
 *   vits_layer_norm_channels modules.LayerNorm (modules.py:41-44)
 *   vits_attention_forward   MultiHeadAttention.attention core
 *                            (attentions.py:85-100)
 *   vits_attention_train_forward /  the same core in training, with its
 *   vits_attention_backward         dropout (attentions.py:97) and gradients
 *   vits_resample_poly /     the output stage of VITSWrap.speaking
 *   vits_pcm16               (vits_wrap.py:186-197): librosa.resample for
 *                            pitch and sampling rate, clip, int16, tail pad
 *   vits_resample_poly_span  a span of that stage's output from a window of
 *                            its input: the chunks of a streamed utterance
 *                            (no counterpart: the reference sends whole files)
 *   vits_draw_starts        the np.random.randint slice starts of
 *                            consecutive EmoVITS.infer calls (infer.py:173),
 *                            for a whole batch in call order
 *   vits_pack_pcm            the segment concatenation of VITSWrap.speaking
 *                            (vits_wrap.py:198,212-214), on the device
 *   vits_*_rows              the four above with the speed, the ratio, the
 *                            volume and the tail per row: requests with
 *                            different controls behind one graph replay
 *   vits_duration_plan       per-token durations under a caller's controls
 *                            (pins, per-token scales, a total to fit), the
 *                            attn argument of infer_p2 (models.py:568) built
 *                            on the device
 *   vits_*_int               vits_expand_durations / vits_draw_starts from
 *                            those integer durations
 *   vits_retime_plan /       a recording's own latents resampled along time,
 *   vits_retime_warp         token by token (no counterpart: the reference
 *                            converts a recording at its own length only)
 */
#ifndef VITS_AMD_H
#define VITS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VITS_OK 0
#define VITS_E_ARG (-1)     /* bad pointer / non-positive size */
#define VITS_E_SHAPE (-2)   /* inconsistent shapes / strides */
#define VITS_E_UNSUP (-3)   /* configuration outside the compiled kernels */

/* ---------------------------------------------------------------------- */
/* conv1d: implicit-GEMM dilated 1-D convolution on fp32 MFMA             */
/* ---------------------------------------------------------------------- */

/* epilogue kinds */
#define VITS_EPI_STORE 0     /* y = act(acc + bias + cond) [+res] [accumulate] */
#define VITS_EPI_GATE 1      /* y[p] = tanh(v[2p]) * sigmoid(v[2p+1])           */
                             /* (+ out1.y set: the pre-activation acc + bias,   */
                             /* no cond, to out1 channels p and m/2 + p - the   */
                             /* training gate's saved input)                    */
#define VITS_EPI_UPSAMPLE 2  /* polyphase ConvTranspose1d output scatter        */

/* activations applied to v before residual/accumulate (STORE epilogue) */
#define VITS_ACT_NONE 0
#define VITS_ACT_RELU 1
#define VITS_ACT_TANH 2
#define VITS_ACT_EXP 3

/* tile configurations (rows x cols of one workgroup) */
#define VITS_TILE_128x128 0
#define VITS_TILE_64x256 1
#define VITS_TILE_32x256 2
#define VITS_TILE_64x128 3  /* chosen by the library for small grids of 128x128 layers */

typedef struct vits_conv_out {
  float* y;               /* output [B][*][y_cstride]                        */
  int64_t y_bstride;      /* elements between utterances                     */
  int32_t y_cstride;      /* elements between channels                       */
  int32_t act;            /* VITS_ACT_*                                      */
  const float* res;       /* optional residual (may alias y)                 */
  int64_t res_bstride;
  int32_t res_cstride;
  float res_scale;        /* y = res + res_scale * v                         */
  int32_t accumulate;     /* y = y_old + (...)                               */
  float post_div;         /* y /= post_div when != 1                         */
} vits_conv_out;

typedef struct vits_conv1d_desc {
  /* input x: element (b, c, t) at b*x_bstride + c*x_cstride + t*x_tstride   */
  /* ([B][C][T] activations: x_tstride = 1; time-major [B][T][C]: x_cstride */
  /* = 1, x_tstride = C, used for the text-embedding Linear)                */
  const float* x;
  int64_t x_bstride;
  int32_t x_cstride;
  int32_t x_tstride;
  int32_t cin;
  int32_t tin;            /* valid input positions; outside reads as 0        */
  float in_slope;         /* prologue leaky-relu slope on x; 1.0 = identity   */
  /* packed weights: [cin_pad][k][m_pad] fp32, see vits_amd/engine.py       */
  const float* w;
  int32_t m;              /* GEMM rows actually produced                      */
  int32_t m_pad;          /* row stride of the packed weights                 */
  int32_t cin_pad;        /* multiple of kc                                    */
  int32_t kc;             /* input channels staged per K-chunk (even)         */
  int32_t k;              /* taps                                             */
  int32_t dil;            /* tap dilation                                      */
  int32_t pad_left;       /* input position of column n, tap j: n-pad+j*dil   */
  int32_t n_out;          /* GEMM columns (output positions)                  */
  int32_t tile;           /* VITS_TILE_*                                      */
  /* epilogue */
  int32_t epi;            /* VITS_EPI_*                                       */
  const float* bias;      /* logical-order bias or NULL                       */
  const float* cond;      /* [B][cond_bstride] logical-order add, or NULL     */
  int64_t cond_bstride;
  int32_t split;          /* STORE: rows [0,split)->out0, [split,m)->out1     */
  int32_t up_u;           /* UPSAMPLE: stride u                               */
  int32_t up_pad;         /* UPSAMPLE: ConvTranspose padding                  */
  int32_t t_out;          /* UPSAMPLE: output length                          */
  const int32_t* lengths; /* [B]: zero output columns t >= lengths[b]; NULL   */
  vits_conv_out out0;
  vits_conv_out out1;
  /* weight / MFMA type: VITS_WDT_F32 (w as above, exact-f32 MFMA) or      */
  /* VITS_WDT_BF16 / VITS_WDT_F16 (w = 16-bit [cin_pad/kc][k][kc/8][m_pad]  */
  /* [8], kc % 16 == 0; activations stay fp32 in HBM and are rounded to the */
  /* 16-bit type when staged; fp32 accumulation:                           */
  /* v_mfma_f32_32x32x16_bf16 / _f16), or VITS_WDT_F32S (w = the fp32     */
  /* [cin_pad/16][k][2][m_pad][8] slab image, kc % 16 == 0: fp32 operands  */
  /* split exactly into three bf16 terms in registers, six bf16 MFMAs per  */
  /* 16-deep k-step (hi*hi, hi*mid, mid*hi, mid*mid, hi*lo, lo*hi), fp32   */
  /* accumulation; error vs fp64 at the exact-fp32 kernel's level)         */
  int32_t wdtype;
  /* single-output STORE only (the input gradient of a conv whose forward   */
  /* fused a leaky-relu prologue): v *= gmask[b][row][n] > 0 ? 1 : slope    */
  /* before residual / accumulate; gmask = the forward's input, NULL = off  */
  const float* gmask;
  int64_t gmask_bstride;
  int32_t gmask_cstride;
  float gmask_slope;
  /* io16 != 0 (16-bit wdtype only): x, out0/out1 y and res, and gmask are  */
  /* tensors of the 16-bit operand type (strides in elements); fp32 I/O    */
  /* otherwise.  The fp16-autocast training convs keep fp16 activations   */
  /* (io16 = 1); io16 = 2 marks the 16-bit inference decoder, whose groups */
  /* with a >= 5-tap member read weight fragments from global memory.    */
  int32_t io16;
  /* with lengths: > 0 = workgroups whose first output position is at or    */
  /* past lengths[b] + len_skip exit without computing or writing (the      */
  /* bucketed whole-utterance infer: work follows the utterance, not the     */
  /* bucket; consumers never read past lengths[b] + halo, halo < len_skip,  */
  /* and [lengths[b], lengths[b] + len_skip) is written as zeros); 0 = off  */
  int32_t len_skip;
} vits_conv1d_desc;

#define VITS_WDT_F32 0
#define VITS_WDT_BF16 1
#define VITS_WDT_F16 2
#define VITS_WDT_F32S 3
/* VITS_WDT_F32P: the F32S arithmetic with w = the host-split bf16 planes   */
/* [cin_pad/16][k][2][3][m_pad][8] (plane 0 = hi, 1 = mid, 2 = lo of each   */
/* fp32 weight, x == hi + mid + lo exactly), kc 16 or 32; A fragments are  */
/* read from global memory, so only the input window is staged in LDS.     */
#define VITS_WDT_F32P 4

int vits_conv1d_forward(const vits_conv1d_desc* d, int batch, void* stream);

/* Run `n` conv descriptors back to back on one stream (one host call). */
int vits_conv1d_forward_seq(const vits_conv1d_desc* d, int n, int batch, void* stream);

/* Run `ngroups` groups of consecutive descriptors (sizes[i] each, <= 3):  */
/* the members of a group are independent convs (no member reads another's */
/* output; the three ResBlock2 branches of one Generator stage,            */
/* models.py:311-313 / modules.py:250-260) and share ONE launch when they  */
/* have the same tile, epilogue and staging kind, else run in order.       */
/* Groups run in order.                                                    */
int vits_conv1d_forward_groups(const vits_conv1d_desc* d, const int32_t* sizes, int ngroups,
                               int batch, void* stream);

/* ---------------------------------------------------------------------- */
/* per-utterance conditioning GEMV: y[b][n] = W[n][:] . g[b][:] + bias[n] */
/* ---------------------------------------------------------------------- */
int vits_linear_forward(const float* g, int64_t g_bstride, const float* w, const float* bias,
                        float* y, int64_t y_bstride, int batch, int n_out, int n_in,
                        void* stream);

/* ---------------------------------------------------------------------- */
/* prior expansion: z[b][c][t] = sum_x attn[b][t][x] m[b][c][x]           */
/*                    + noise[b][c][t] * sum_x attn[b][t][x] s[b][c][x]   */
/* ---------------------------------------------------------------------- */
int vits_expand_prior(const float* attn, const float* m, const float* s, const float* noise,
                      float* z, int batch, int channels, int t_y, int t_x, int exp_s,
                      float noise_scale, void* stream);
/* exp_s = 0: z = A.m + noise * (A.s)                 (infer_p2, models.py:569-571) */
/* exp_s = 1: z = A.m + noise * exp(A.s) * noise_scale  (inference, models.py:529-532) */

/* ---------------------------------------------------------------------- */
/* Generator tail: y[b][t] = tanh(sum_{c,j} w[c][j] lrelu(x[b][c][t-3+j], 0.01)) */
/* w: [channels][7] (conv_post, no bias)                                  */
/* ---------------------------------------------------------------------- */
/* ---------------------------------------------------------------------- */
/* durations -> lengths + expanded prior, on the device (replaces the       */
/* w = exp(logw)*rate -> ceil -> y_len .item() -> infer_path -> attn @ m /  */
/* attn @ s -> z_p sequence of models.py:544-553, infer.py:169-176 and     */
/* commons.py:143-155 without a host sync, over a static bucket t_y):       */
/*   w_ceil[x] = ceil(exp(logw[b][x]) * rate) (x < x_len[b], else 0;        */
/*   half_round: fp16 roundings of the half model), y_len = max(sum, 1),   */
/*   z[b][c][t] = m[b][c][x(t)] + noise(c,t) * s[b][c][x(t)] * noise_scale  */
/*   for t < y_len (x(t): cum[x-1] <= t < cum[x]), 0 for y_len <= t < t_y;  */
/*   lens[i][b] = y_len * stage_mult[i].  noise_mode 0: noise [B][C][t_y];  */
/*   1: element (c, t) at noise[s + c*y_len + t] (EmoVITS's buffer slice,   */
/*   infer.py:172-175), s = np.random.randint(noise_len - C*y_len) drawn on */
/*   the device exactly as numpy's legacy RandomState does (masked         */
/*   rejection) from noise_start = [B][VITS_ED_DRAWS] raw MT19937 uint32    */
/*   words; lens must then have n_stage + 1 rows: lens[n_stage][b] = words  */
/*   consumed (the host re-advances its generator by that many), -1 when   */
/*   the slice does not fit (the reference's randint raises), -2 when all  */
/*   VITS_ED_DRAWS words were rejected (the host advances by the pool and  */
/*   calls again with the next words); z = 0 and no noise read for both.  */
/*   t_x <= 4096, n_stage <= 8.                                             */
#define VITS_ED_DRAWS 32
/* ---------------------------------------------------------------------- */
int vits_expand_durations(const float* logw, int64_t logw_bstride, const int32_t* x_len, int t_x,
                          float rate, int half_round, const float* m, const float* s,
                          int64_t ms_bstride, int32_t ms_cstride, const float* noise,
                          int noise_mode, const int32_t* noise_start, int64_t noise_len,
                          float noise_scale, float* z,
                          int batch, int channels, int t_y, int32_t* lens,
                          const int32_t* stage_mult, int n_stage, void* stream);

/* noise_mode 2: the slice start of row b is read from noise_start taken as  */
/* the int64 [batch] `starts` of vits_draw_starts (8-byte aligned); a       */
/* negative start, or one whose slice would leave the buffer, gives z = 0   */
/* and reads no noise.  lens has n_stage rows, as in mode 0.                */

/* ---------------------------------------------------------------------- */
/* The noise-slice starts of a batch as consecutive EmoVITS.infer calls     */
/* draw them (infer.py:173): one launch of one workgroup computes y_len[b]  */
/* of every row with vits_expand_durations' arithmetic, then draws row b's  */
/* np.random.randint(noise_len - channels * y_len[b]) from ONE shared pool  */
/* of raw MT19937 words (uint32 [pool_n]), starting where row b - 1's       */
/* masked rejection stopped.  starts int64 [batch]; meta int32 [2 * batch   */
/* + 1] = y_len [batch] | status [batch] | used_total.  status: words       */
/* consumed (0 when the range has one value: numpy draws nothing), -1 when  */
/* the slice does not fit (nothing consumed), -2 when the pool ran out at   */
/* this row; starts[b] = -1 for a negative status.  Rows at or past         */
/* *n_rows (device int32, NULL = batch: the padding of a batch bucket) draw */
/* nothing: status 0, start 0.  t_x <= 4096, batch <= 1024.                 */
/* ---------------------------------------------------------------------- */
int vits_draw_starts(const float* logw, int64_t logw_bstride, const int32_t* x_len, int t_x,
                     float rate, int half_round, int channels, int64_t noise_len,
                     const uint32_t* pool, int pool_n, const int32_t* n_rows, int batch,
                     int64_t* starts, int32_t* meta, void* stream);

/* Per-row speed: vits_expand_durations / vits_draw_starts with row b's rate */
/* read on the device from rates[b] (fp32 [batch]) in place of the scalar,  */
/* so that one captured graph serves every mix of speeds.  The arithmetic   */
/* is the scalar entry points' (one fp32 multiply, then the half_round      */
/* roundings): a row with rates[b] == rate is bit for bit the scalar call.  */
int vits_expand_durations_rows(const float* logw, int64_t logw_bstride, const int32_t* x_len,
                               int t_x, const float* rates, int half_round, const float* m,
                               const float* s, int64_t ms_bstride, int32_t ms_cstride,
                               const float* noise, int noise_mode, const int32_t* noise_start,
                               int64_t noise_len, float noise_scale, float* z, int batch,
                               int channels, int t_y, int32_t* lens, const int32_t* stage_mult,
                               int n_stage, void* stream);
int vits_draw_starts_rows(const float* logw, int64_t logw_bstride, const int32_t* x_len, int t_x,
                          const float* rates, int half_round, int channels, int64_t noise_len,
                          const uint32_t* pool, int pool_n, const int32_t* n_rows, int batch,
                          int64_t* starts, int32_t* meta, void* stream);

/* ---------------------------------------------------------------------- */
/* Duration control.  vits_duration_plan turns the duration predictor's     */
/* logw and a caller's controls into integer durations on the device (one   */
/* 256-thread workgroup per row, no host sync, safe under stream capture):  */
/*   given     int32 [batch][t_x] or NULL: >= 0 pins the token to exactly    */
/*             that many frames (0 allowed), < 0 leaves it free              */
/*   tok_scale fp32 [batch][t_x] or NULL: per-token factor (>= 0) on w       */
/*   target    int32 [batch] or NULL: > 0 = the row must last exactly that   */
/*             many frames, <= 0 = no target                                 */
/*   rate / rates: the scalar speed, or fp32 [batch] per-row speeds when     */
/*             rates != NULL (rate is then ignored)                          */
/* A free token x < x_len[b] (x_len NULL: t_x) has w = exp(logw) * rate with */
/* vits_expand_durations' fp16 roundings under half_round, then * tok_scale  */
/* (one more fp16 rounding under half_round).  Without a target d = (int)    */
/* ceil(w).  With a target T the rate is not applied (w = exp(logw) *        */
/* tok_scale) and the free tokens F are fitted in integer arithmetic: P =    */
/* the sum of the pins, E = T - P - |F|,                                     */
/*   q[x] = max(llrint(min(max(w, 2^-8), 2^15) * 256) - 128, 1)   (int64)    */
/*   Q[x] = inclusive prefix sum of q over F in token order, Qtot = the last */
/*   B[x] = (Q[x] * E + Qtot / 2) / Qtot                    (int64 division) */
/*   d[x] = 1 + B[x] - B[previous free token]             (B = 0 before F)   */
/* so every free token gets >= 1 frame, pins are untouched and the row sums  */
/* to exactly T, whatever the order of summation.  (A NaN w counts as 2^-8.) */
/* Domain: a pin above 2^18 counts as 2^18 and ceil(w) is clamped to [0,     */
/* 2^18] (an Inf or huge w saturates, a NaN or negative w gives 0 frames):   */
/* the clamp of the _int entry points below, so `total` and their y_len      */
/* always agree.                                                             */
/* dur int32 [batch][t_x]: 0 at and past x_len.  meta int32 [2][batch]:      */
/* total (the plain integer sum of the row: no fp16 rounding of the sum, no  */
/* max(., 1)) and status: 1 when the target cannot   */
/* be met (E < 0, or no free token and T != P, or T > 2^24, the range of     */
/* the int64 fit): the row then gets the no-target durations; else 0.        */
/* w_out fp32 [batch][t_x] or NULL: the w behind each free token's duration  */
/* (rate applied unless the row was fitted), 0 for pinned and padded tokens. */
/* VITS_E_ARG: NULL logw / dur / meta, batch <= 0, t_x <= 0; VITS_E_SHAPE:   */
/* logw_bstride < t_x; VITS_E_UNSUP: t_x > 4096.                             */
/* ---------------------------------------------------------------------- */
int vits_duration_plan(const float* logw, int64_t logw_bstride, const int32_t* x_len, int t_x,
                       float rate, const float* rates, int half_round, const int32_t* given,
                       const float* tok_scale, const int32_t* target, int32_t* dur, int32_t* meta,
                       float* w_out, int batch, void* stream);

/* vits_expand_durations / vits_draw_starts reading integer durations dur    */
/* int32 [batch] rows of dur_bstride (>= t_x) in place of logw / rate /      */
/* half_round: token x < x_len[b] lasts min(max(dur[b][x], 0), 2^18) frames  */
/* (0: the token gets no frame), y_len = max(sum, 1) as a plain integer sum. */
/* Everything else (noise modes 0 / 1 / 2, stage_mult, n_rows, the -1 / -2   */
/* statuses, zeros past y_len) is the logw entry points' rule, and with dur  */
/* = ceil(exp(logw) * rate) they compute bit for bit what those compute      */
/* (fp32 model; the half model's fp16 sum differs above 2048 frames).        */
int vits_expand_durations_int(const int32_t* dur, int64_t dur_bstride, const int32_t* x_len,
                              int t_x, const float* m, const float* s, int64_t ms_bstride,
                              int32_t ms_cstride, const float* noise, int noise_mode,
                              const int32_t* noise_start, int64_t noise_len, float noise_scale,
                              float* z, int batch, int channels, int t_y, int32_t* lens,
                              const int32_t* stage_mult, int n_stage, void* stream);
int vits_draw_starts_int(const int32_t* dur, int64_t dur_bstride, const int32_t* x_len, int t_x,
                         int channels, int64_t noise_len, const uint32_t* pool, int pool_n,
                         const int32_t* n_rows, int batch, int64_t* starts, int32_t* meta,
                         void* stream);

int vits_conv_post_tanh(const float* x, int64_t x_bstride, int32_t x_cstride, const float* w,
                        float* y, int batch, int channels, int t_len, int ksize, void* stream);
/* Same on a 16-bit last-stage activation (xdtype VITS_WDT_BF16 / _F16; the
 * 16-bit model's decoder with 16-bit activations, as the reference's .half()
 * model holds them); VITS_WDT_F32 = vits_conv_post_tanh. */
int vits_conv_post_tanh_lowp(const void* x, int64_t x_bstride, int32_t x_cstride, const float* w,
                             float* y, int batch, int channels, int t_len, int ksize, int xdtype,
                             void* stream);

/* ---------------------------------------------------------------------- */
/* Monotonic alignment search (VITS DP + backtrack), bit-exact vs the     */
/* Cython core.  neg_cent [B][t_t][t_s] fp32 (the reference casts to fp32 */
/* before the DP); mask [B][t_t][t_s] of mask_dtype: lengths are taken as */
/* t_t[b] = sum_y mask[b][y][0], t_s[b] = sum_x mask[b][0][x] exactly as  */
/* monotonic_align/__init__.py does.  path [B][t_t][t_s] of path_dtype is */
/* written in full (1 on the path, 0 elsewhere).                          */
/* dtype codes: VITS_DT_*.                                                */
/* ---------------------------------------------------------------------- */
#define VITS_DT_F32 0
#define VITS_DT_F16 1
#define VITS_DT_BF16 2
#define VITS_DT_I32 3
int vits_maximum_path(const float* neg_cent, const void* mask, int mask_dtype, void* path,
                      int path_dtype, int batch, int t_t, int t_s, void* workspace,
                      int64_t workspace_bytes, void* stream);
/* same, with explicit per-utterance lengths (int32 [B] each, on device) */
int vits_maximum_path_lengths(const float* neg_cent, const int32_t* t_t_len,
                              const int32_t* t_s_len, void* path, int path_dtype, int batch,
                              int t_t, int t_s, void* workspace, int64_t workspace_bytes,
                              void* stream);
/* bytes of workspace the two calls above need (0 when the backtrack bits */
/* fit in LDS)                                                            */
int64_t vits_maximum_path_workspace(int batch, int t_t, int t_s);
/* Forced alignment: the same DP and backtrack as vits_maximum_path_lengths  */
/* (same neg_cent, lengths and workspace), but no path is written.  From the */
/* path of row b:                                                            */
/*   durations[b][x]   frames y < t_t_len[b] on token x; 0 for x >=          */
/*                     t_s_len[b]                                            */
/*   scores[b][x]      (or NULL) the fp32 sum of neg_cent[b][y][x] over the  */
/*                     token's frames, added one by one in increasing y from */
/*                     0.0f (no FMA, no tree: a float32 loop reproduces it   */
/*                     exactly); 0 for x >= t_s_len[b]                       */
/*   frame_token[b][y] (or NULL) the token of frame y; -1 for y >=           */
/*                     t_t_len[b]                                            */
/* A row with t_t_len[b] == 0, t_s_len[b] == 0 or t_t_len[b] < t_s_len[b]    */
/* has no alignment: durations 0, scores 0 and tokens -1 over the whole row. */
/* Lengths are clamped to [0, t_t] / [0, t_s].  Returns VITS_E_ARG for a     */
/* null neg_cent / length / durations pointer, a non-positive size or a      */
/* workspace of fewer than vits_maximum_path_workspace bytes, VITS_E_UNSUP   */
/* for t_s beyond the widest kernel (2048).                                  */
int vits_maximum_path_durations(const float* neg_cent, const int32_t* t_t_len,
                                const int32_t* t_s_len, int32_t* durations, float* scores,
                                int32_t* frame_token, int batch, int t_t, int t_s,
                                void* workspace, int64_t workspace_bytes, void* stream);

/* Forced alignment of long recordings: the DP, backtrack and reductions of  */
/* vits_maximum_path_durations, bit for bit, over a score matrix that is fed */
/* in panels of `panel` frames (a multiple of 32) by all t_s tokens and is   */
/* never held as a whole; t_s has no limit.  A panel's row is processed in   */
/* strips of `strip` tokens (64 * 2^k, k <= 5).  The sequence of one job, on */
/* one stream:                                                               */
/*   vits_mas_long_panel      for y0 = 0, panel, 2 panel, ... in this order  */
/*   vits_mas_long_backtrack  durations and frame_token (or NULL)            */
/*   vits_mas_long_gather     for every panel again, in any order (scores)   */
/*   vits_mas_long_scores     the per-token sums                             */
/* `scores` of _panel / _gather points at row y0 of the matrix: [batch] x    */
/* [rows][t_s] fp32, `batch_stride` elements from one recording to the next  */
/* (>= rows * t_s).  rows <= panel, and rows < panel only for the last       */
/* panel (y0 + rows == t_t).  The gather must see the same values as the     */
/* forward step.  t_t_len / t_s_len, the outputs and the rows without an     */
/* alignment are those of vits_maximum_path_durations; all five calls of a   */
/* job take the same batch, t_t, t_s, strip, panel and workspace.  The       */
/* workspace holds the job's state between the calls, in sections rounded up */
/* to 256 bytes each, with Ws = ceil(t_s / strip) * strip:                   */
/*   float    carry[2][batch][Ws]               V[y0 - 1][.]: a panel reads  */
/*                                              half (y0 / panel) & 1 and    */
/*                                              writes the other             */
/*   uint32_t words[batch][ceil(t_t / 32)][Ws]  decision bits, bit y mod 32  */
/*   int32_t  frame_token[batch][t_t]                                        */
/*   int32_t  start[batch][Ws + 1]              first frame of every token   */
/*   float    val[batch][t_t]                   the path's own scores        */
/* It needs no initialisation and must be 16-byte aligned.  The calls are    */
/* asynchronous and capture-safe and depend on each other through stream     */
/* order alone.  Each returns VITS_E_ARG, before any launch, for a null      */
/* pointer (frame_token excepted), a non-positive size, a panel that is no   */
/* multiple of 32, a strip that is not 64 * 2^k with k <= 5, a y0 that is    */
/* negative, no multiple of panel or >= t_t, rows outside the above, or a    */
/* workspace of fewer than vits_mas_long_workspace bytes; VITS_E_UNSUP for a */
/* panel whose column buffers do not fit the LDS beside the strip's ring.    */
/* vits_mas_long_workspace returns 0 for sizes the calls would refuse.       */
int64_t vits_mas_long_workspace(int batch, int t_t, int t_s, int strip, int panel);
int vits_mas_long_panel(const float* scores, int64_t batch_stride, const int32_t* t_t_len,
                        const int32_t* t_s_len, int batch, int t_t, int t_s, int strip, int panel,
                        int y0, int rows, void* workspace, int64_t workspace_bytes, void* stream);
int vits_mas_long_backtrack(const int32_t* t_t_len, const int32_t* t_s_len, int32_t* durations,
                            int32_t* frame_token, int batch, int t_t, int t_s, int strip,
                            int panel, void* workspace, int64_t workspace_bytes, void* stream);
int vits_mas_long_gather(const float* scores, int64_t batch_stride, const int32_t* t_t_len,
                         const int32_t* t_s_len, int batch, int t_t, int t_s, int strip,
                         int panel, int y0, int rows, void* workspace, int64_t workspace_bytes,
                         void* stream);
int vits_mas_long_scores(const int32_t* t_t_len, const int32_t* t_s_len, float* token_scores,
                         int batch, int t_t, int t_s, int strip, int panel, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------- */
/* MAS scores (models.py:483-490): neg_cent[b][y][x] = sum_d(-0.5 log 2pi */
/* - logs_p - 0.5 z_p^2 s + z_p m_p s - 0.5 m_p^2 s), s = exp(-2 logs_p). */
/* z_p [B][C][t_t], m_p / logs_p [B][C][t_s], neg_cent [B][t_t][t_s], all */
/* contiguous fp32.  Computed in fp32 over every (padded) position, as    */
/* the reference does before its mask.                                    */
/* ---------------------------------------------------------------------- */
int vits_neg_cent(const float* z_p, const float* m_p, const float* logs_p, float* neg_cent,
                  int batch, int channels, int t_t, int t_s, void* stream);

/* ---------------------------------------------------------------------- */
/* STFT magnitude and its adjoint.  x [B][L] fp32; the signal is reflect- */
/* padded by `pad` samples on both sides (pad = n_fft/2 reproduces        */
/* torch.stft(center=True, pad_mode='reflect'); mel_processing pads       */
/* (n_fft-hop)/2 itself and calls center=False), then framed with `hop`,  */
/* windowed by `window` (length win, centred in n_fft as torch.stft does) */
/* and transformed: frames = (L + 2 pad - n_fft)/hop + 1, and none when   */
/* L + 2 pad < n_fft: the transforms then return VITS_E_SHAPE and         */
/* vits_stft_workspace returns 0.                                         */
/* mag [B][n_fft/2+1][frames] = sqrt(re^2 + im^2 + eps); re/im (optional, */
/* needed by the backward) same layout.                                   */
/* ---------------------------------------------------------------------- */
int vits_stft_mag_forward(const float* x, int batch, int length, const float* window,
                          int n_fft, int hop, int win, int pad, float eps, float* mag,
                          float* re, float* im, void* stream);
/* grad_x [B][L] = d(sum grad_mag * mag)/dx.  workspace: frames*n_fft*B   */
/* floats (vits_stft_workspace).                                          */
int vits_stft_mag_backward(const float* grad_mag, const float* mag, const float* re,
                           const float* im, const float* window, int batch, int length,
                           int n_fft, int hop, int win, int pad, float* grad_x,
                           float* workspace, int64_t workspace_floats, void* stream);
int64_t vits_stft_workspace(int batch, int length, int n_fft, int hop, int pad);

/* Several transforms in one launch (the 2 signals x 5 resolutions of the */
/* MR-STFT loss, stft_loss.py:47-95): up to 16 jobs, each with its own    */
/* signal batch, resolution and outputs.  Forward uses x, window, sizes,  */
/* eps, mag, re, im; backward uses grad_mag, mag, re, im, window, sizes,  */
/* grad_x and a workspace of vits_stft_workspace_multi floats.  layout 1: */
/* mag / re / im / grad_mag are [B][frames][n_fft/2+1] (frame-major: a    */
/* workgroup's frames are one contiguous run - coalesced stores); 0: the  */
/* torch.stft layout [B][n_fft/2+1][frames].                              */
typedef struct vits_stft_job {
  const float* x;
  const float* window;
  const float* grad_mag;
  float* mag;
  float* re;
  float* im;
  float* grad_x;
  int32_t batch;
  int32_t length;
  int32_t n_fft;
  int32_t hop;
  int32_t win;
  int32_t pad;
  float eps;
  int32_t layout;
} vits_stft_job;
int vits_stft_mag_forward_multi(const vits_stft_job* jobs, int njobs, void* stream);
int vits_stft_mag_backward_multi(const vits_stft_job* jobs, int njobs, float* workspace,
                                 int64_t workspace_floats, void* stream);
int64_t vits_stft_workspace_multi(const vits_stft_job* jobs, int njobs);

/* Magnitude STFT of a ragged batch, each row's length read on the device  */
/* (inference only: no re / im, layout [B][n_fft/2+1][frames_cap]), so the  */
/* wave -> spectrogram step of voice conversion sits in a captured graph.   */
/* x [B][cap] fp32 with row stride x_bstride; lens int32 [B] (device).      */
/* Row b: L_b = clamp(lens[b], 0, cap); the reflect padding folds at the    */
/* row's own end L_b - 1, and nothing at or past L_b is read.  frames_b =   */
/* min((L_b + 2 pad - n_fft)/hop + 1, frames_cap) when L_b > pad and L_b +  */
/* 2 pad >= n_fft, else 0; columns >= frames_b are written as 0;            */
/* frames_out (int32 [B], optional) receives frames_b.  The first frames_b  */
/* columns of row b are bit for bit vits_stft_mag_forward of that row alone */
/* at length L_b.  VITS_E_ARG for a null x / mag / lens / window;           */
/* VITS_E_SHAPE for frames_cap <= 0, x_bstride < cap, pad >= cap, win >     */
/* n_fft, or a cap no frame fits (cap + 2 pad < n_fft).                     */
int vits_stft_mag_forward_rows(const float* x, int64_t x_bstride, int batch, int cap,
                               const int32_t* lens, const float* window, int n_fft, int hop,
                               int win, int pad, float eps, float* mag, int frames_cap,
                               int32_t* frames_out, void* stream);

/* ---------------------------------------------------------------------- */
/* Tail of the posterior encoder over a bucket (models.py:273-279 with the */
/* mask of models.py:262-271): z[b][c][t] = m + (noise * s) * noise_scale   */
/* for t < lens[b], 0 for lens[b] <= t < t_len.  m, s: the two outputs of   */
/* the proj conv (s already through the ACT_EXP epilogue), rows of          */
/* ms_cstride floats; noise [B][C][t_len] contiguous or NULL (z = m, the    */
/* posterior mean); z [B][C][t_len] contiguous.  stage_lens (optional,      */
/* int32 [n_stage][B]): stage_lens[i][b] = clamp(lens[b], 0, t_len) *       */
/* stage_mult[i], the layout of vits_expand_durations' lens. n_stage <= 8.  */
/* ---------------------------------------------------------------------- */
int vits_posterior_sample(const float* m, const float* s, int64_t ms_bstride, int32_t ms_cstride,
                          const float* noise, float noise_scale, const int32_t* lens, float* z,
                          int batch, int channels, int t_len, int32_t* stage_lens,
                          const int32_t* stage_mult, int n_stage, void* stream);

/* ---------------------------------------------------------------------- */
/* channel LayerNorm over dim 1 of [B][C][T]:                             */
/*   v = LN(x + r) * gamma + beta                (r, gamma, beta optional) */
/*   v = (v + post_add[b][c]) * scale + pos[t][c] * (*pos_alpha)           */
/*   y = (t < lengths[b]) ? v : 0                (lengths optional)        */
/* post_add / pos / pos_alpha optional (NULL); pos is [T][C] (sin table);  */
/* pos_alpha is a device scalar (the learnable TextEncoder.alpha).        */
/* ---------------------------------------------------------------------- */
int vits_layer_norm_channels(const float* x, const float* r, const float* gamma,
                             const float* beta, float* y, int batch, int channels, int t_len,
                             float eps, const int32_t* lengths, const float* post_add,
                             int64_t post_add_bstride, float scale, const float* pos,
                             const float* pos_alpha, void* stream);

/* ---------------------------------------------------------------------- */
/* scaled-dot-product attention over [B][H*D][T] channel-major q/k/v      */
/* (batch stride qkv_bstride, e.g. slices of one fused q|k|v buffer), key */
/* mask from lengths (fill -1e4), out [B][H*D][T] with out_bstride;        */
/* head_dim in {16, 32, 48, 64, 96, 128}, else VITS_E_UNSUP              */
/* ---------------------------------------------------------------------- */
int vits_attention_forward(const float* q, const float* k, const float* v, float* out,
                           int batch, int heads, int head_dim, int t_len,
                           int64_t qkv_bstride, int64_t out_bstride, const int32_t* lengths,
                           void* stream);

/* ---------------------------------------------------------------------- */
/* The same attention for training (MultiHeadAttention.forward,           */
/* attentions.py:79-100 incl. self.drop): layout, mask and padding rules  */
/* of vits_attention_forward; q / k / v / out (and the gradients) of      */
/* `dtype` (VITS_DT_F32: fp32 MFMA; VITS_DT_F16 / _BF16: 16-bit MFMA,     */
/* fp32 accumulation and softmax).                                        */
/*   lse   fp32 [B][H][T]: log-sum-exp of each query's masked scores      */
/*         (saved for the backward)                                       */
/*   p_drop, seed: dropout of the normalised probabilities,               */
/*         out = (P * keep / (1 - p_drop)) V, keep a counter-based hash   */
/*         of (*seed, b, h, query, key).  seed is a DEVICE int64 read by  */
/*         the kernel (capture-safe); p_drop == 0 never reads it (may be  */
/*         NULL) and computes exactly vits_attention_forward's result.    */
/* 0 <= p_drop < 1, else VITS_E_ARG; head_dim as above, else VITS_E_UNSUP. */
/* ---------------------------------------------------------------------- */
int vits_attention_train_forward(const void* q, const void* k, const void* v, void* out,
                                 float* lse, int batch, int heads, int head_dim, int t_len,
                                 int64_t qkv_bstride, int64_t out_bstride,
                                 const int32_t* lengths, int dtype, float p_drop,
                                 const int64_t* seed, void* stream);

/* Backward of vits_attention_train_forward: dq / dk / dv [B][H*D][T] of   */
/* `dtype` with batch stride dqkv_bstride (e.g. the channel slices of one */
/* [B][3C][T] gradient buffer) from q, k, v, out, dout (batch strides     */
/* qkv_bstride / out_bstride / dout_bstride), the saved lse and the same  */
/* p_drop / seed.  S and P are recomputed from lse; dS = P * (keep /      */
/* (1 - p) * (dout . V) - delta), delta[q] = sum_d dout * out, and dS = 0  */
/* wherever the score was filled with -1e4 (dv still receives those       */
/* rows' uniform P).  Two launches, no atomics, fixed reduction order:     */
/* dq (+ delta, an fp32 [B][H][T] workspace the caller provides) by       */
/* query tile, then dk / dv by key tile.                                  */
int vits_attention_backward(const void* q, const void* k, const void* v, const void* out,
                            const void* dout, const float* lse, void* dq, void* dk, void* dv,
                            float* delta, int batch, int heads, int head_dim, int t_len,
                            int64_t qkv_bstride, int64_t out_bstride, int64_t dout_bstride,
                            int64_t dqkv_bstride, const int32_t* lengths, int dtype,
                            float p_drop, const int64_t* seed, void* stream);

/* The dropout keep mask of the two calls above as uint8 [B][H][T][T]     */
/* ([query][key]; 1 = kept) - for tests.                                  */
int vits_attention_dropout_mask(const int64_t* seed, uint8_t* mask, int batch, int heads,
                                int t_len, float p_drop, void* stream);

/* ---------------------------------------------------------------------- */
/* Training-step convs (backward of every stride-1 nn.Conv1d the          */
/* train_stft.py step runs under fp16 autocast, train_stft.py:165-236:    */
/* WN modules.py:130-182, ResBlock2 modules.py:250-260, couplings         */
/* modules.py:357-375, PosteriorEncoder models.py:268-279, Generator      */
/* models.py:306-318, WaveDiscriminator mrd.py:15-55).  The forward and   */
/* the input gradient run through vits_conv1d_forward on a 16-bit image   */
/* of the weight; the weight gradient has its own kernel.                 */
/* ---------------------------------------------------------------------- */
/* fp32 W [cout][cin][k] -> 16-bit image [cin_pad/16][k][2][m_pad][8] of   */
/* wdtype (VITS_WDT_F16 / _BF16).  transpose = 0: rows = co, channels =   */
/* ci (forward).  transpose = 1: rows = ci, channels = co, taps reversed  */
/* (input gradient: dX = conv(dY, W', pad_left = (k-1)*dil - pad)).       */
/* zero / zero_n: optional fp32 buffer the same launch clears (the weight- */
/* gradient accumulator of the backward that follows; NULL / 0 = none).   */
int vits_conv1d_pack16(const float* w, int cout, int cin, int k, int transpose, void* out,
                       int m_pad, int cin_pad, int wdtype, float* zero, int64_t zero_n,
                       void* stream);
/* Both images in one launch: `out` as transpose = 0 ([cin_pad/16][k][2]   */
/* [m_pad][8], rows cout) and `out_t` as transpose = 1 (rows cin, channels  */
/* cout) -- the training forward packs its backward's image with it.       */
int vits_conv1d_pack16_pair(const float* w, int cout, int cin, int k, void* out, int m_pad,
                            int cin_pad, void* out_t, int m_pad_t, int cin_pad_t, int wdtype,
                            void* stream);
/* Both images of many layers in few launches (48 layers per launch): the  */
/* training step packs every HIP conv of a network once per forward, right  */
/* after the weight / spectral norm launch that produced the weights,       */
/* instead of one vits_conv1d_pack16_pair launch per conv call.             */
typedef struct vits_pack16_layer {
  const float* w;   /* fp32 [cout][cin][k] */
  int32_t cout, cin, k;
  void* img;        /* [cin_pad/16][k][2][m_pad][8], rows cout */
  int32_t m_pad, cin_pad;
  void* img_t;      /* [cin_pad_t/16][k][2][m_pad_t][8], rows cin, taps reversed */
  int32_t m_pad_t, cin_pad_t;
  int32_t gate;     /* 1: img rows gate-interleaved (row 2q = output q, row 2q+1 = */
                    /* output cout/2 + q: VITS_EPI_GATE); img_t stays natural      */
} vits_pack16_layer;
int vits_conv1d_pack16_pairs(const vits_pack16_layer* layers, int n, int wdtype, void* stream);

typedef struct vits_conv1d_wgrad_desc {
  const float* dy;        /* output gradient [B][cout][n_out], t contiguous  */
  int64_t dy_bstride;
  int32_t dy_cstride;
  int32_t cout;
  const float* x;         /* forward input [B][cin][tin], t contiguous       */
  int64_t x_bstride;
  int32_t x_cstride;
  int32_t cin;
  int32_t tin;
  int32_t n_out;
  int32_t k;
  int32_t dil;
  int32_t pad_left;       /* forward: output t reads x[t - pad_left + j*dil] */
  float in_slope;         /* forward's leaky-relu prologue slope (1 = none)  */
  float* dw_t;            /* += dW as [k][cout][cin] fp32 (caller zeroes)    */
  float* dbias;           /* += sum_{b,t} dY [cout] fp32, or NULL            */
  int32_t wdtype;         /* MFMA operand type: VITS_WDT_F16 / VITS_WDT_BF16, */
                          /* or VITS_WDT_F32 (fp32 dy / x, exact-fp32 MFMA,  */
                          /* split mode only; the fp32 training step)        */
  int32_t reserved;       /* > 0: (b, t)-chunks of 64 steps per workgroup    */
                          /* (tuning override), 0 = automatic                */
  int32_t io16;           /* dy / x are tensors of the 16-bit operand type   */
                          /* (strides in elements)                           */
  int32_t reserved2;
} vits_conv1d_wgrad_desc;
/* dW[co][ci][j] = sum_{b,t} dY[b][co][t] * act(x[b][ci][t - pad_left + j*dil]) */
/* (operands rounded to wdtype, fp32 accumulation; VITS_E_UNSUP when       */
/* 64 + (k-1)*dil > 128 or k not in {1,2,3,4,5,7,9,11})                  */
int vits_conv1d_wgrad(const vits_conv1d_wgrad_desc* d, int batch, void* stream);
/* Same weight gradient without atomics (deterministic): every (b, t)-split */
/* workgroup stores its partial tile into `workspace`, a second launch sums */
/* the splits and WRITES d->dw_t in the parameter layout [cout][cin][k]    */
/* and d->dbias [cout] (no zeroing needed).  workspace_floats >=           */
/* vits_conv1d_wgrad_workspace(d, batch).  Replaces the weight-gradient    */
/* half of torch's conv backward under autocast (train_stft.py:206,232).   */
int64_t vits_conv1d_wgrad_workspace(const vits_conv1d_wgrad_desc* d, int batch);
int vits_conv1d_wgrad_split(const vits_conv1d_wgrad_desc* d, int batch, float* workspace,
                            int64_t workspace_floats, void* stream);

/* WaveNet gate of WN (modules.py:139-146) / ResBlock2 (modules.py:253-255) */
/* in training: y[b][p][t] = tanh(x[b][p][t] + g[b][p]) *                 */
/*                           sigmoid(x[b][H+p][t] + g[b][H+p]),  p < H     */
/* g optional ([B][>= 2H] with g_bstride).  Backward: dx [B][2H][T] and   */
/* (optional) dg[b][c] = sum_t dx[b][c][t] as a dense [B][2H].            */
int vits_gate_forward(const float* x, int64_t x_bstride, int32_t x_cstride, const float* g,
                      int64_t g_bstride, float* y, int64_t y_bstride, int32_t y_cstride,
                      int batch, int half_channels, int t_len, void* stream);
int vits_gate_backward(const float* dy, int64_t dy_bstride, int32_t dy_cstride, const float* x,
                       int64_t x_bstride, int32_t x_cstride, const float* g, int64_t g_bstride,
                       float* dx, int64_t dx_bstride, int32_t dx_cstride, float* dg, int batch,
                       int half_channels, int t_len, void* stream);
/* The same with x / g / y (and dy / x / g / dx) of the 16-bit type wdtype */
/* (VITS_WDT_F16 / _BF16: the fp16 activations of the autocast training    */
/* step), fp32 math, dg fp32.                                              */
int vits_gate_forward_io16(const void* x, int64_t x_bstride, int32_t x_cstride, const void* g,
                           int64_t g_bstride, void* y, int64_t y_bstride, int32_t y_cstride,
                           int batch, int half_channels, int t_len, int wdtype, void* stream);
int vits_gate_backward_io16(const void* dy, int64_t dy_bstride, int32_t dy_cstride, const void* x,
                            int64_t x_bstride, int32_t x_cstride, const void* g,
                            int64_t g_bstride, void* dx, int64_t dx_bstride, int32_t dx_cstride,
                            float* dg, int batch, int half_channels, int t_len, int wdtype,
                            void* stream);

/* Up to 4 independent vits_gate_backward_io16 jobs of one batch and length */
/* as ONE launch (the three ResBlock2 branches of a Generator stage,         */
/* modules.py:253-255 under train_stft.py:165's autocast); dg of job i at    */
/* dg[b * dg_bstride + c] (a column slice of the stage's cond gradient).     */
typedef struct vits_gate_bwd_job {
  const void* dy;
  int64_t dy_bstride;
  int64_t dy_cstride;
  const void* x;
  int64_t x_bstride;
  int64_t x_cstride;
  const void* g;         /* 16-bit cond [B][g_bstride], or NULL */
  int64_t g_bstride;
  void* dx;
  int64_t dx_bstride;
  int64_t dx_cstride;
  float* dg;             /* fp32, or NULL */
  int64_t dg_bstride;
  int32_t half_channels;
  int32_t reserved;
} vits_gate_bwd_job;
int vits_gate_backward_io16_multi(const vits_gate_bwd_job* jobs, int n, int batch, int t_len,
                                  int wdtype, void* stream);

/* ---------------------------------------------------------------------- */
/* One ResBlock2 dilation pair of the Generator as ONE kernel              */
/* (modules.py:250-260, fp32):                                             */
/*   y = x + c2(tanh(a + sa) * sigmoid(b + sb)),  (a|b) = c1(lrelu(x,.1)) */
/* c1 = Conv1d(C, C, k, dil) packed as vits_conv1d_forward's GATE layout  */
/* ([cin_pad1][k][m_pad1], rows (a_p, b_p) interleaved), c2 = Conv1d(C/2, */
/* C, k, dil 1, pad (k-1)/2) packed [cin_pad2][k][m_pad2]; b1 / cond are  */
/* in logical order ([a | b], cond already offset to this pair), b2 [C].  */
/* accumulate: y += result (then / post_div) - the branch mean of a stage.*/
/* x: [B][C][T] fp32, T % 4 == 0, 16-byte aligned; y must not alias x.    */
/* C in {32, 64} (the 64- and 32-channel Generator stages).  Up to 3      */
/* independent pairs (same C) run as one launch.  kc1 / kc2 from          */
/* vits_resblock_pair_kc.                                                 */
/* ---------------------------------------------------------------------- */
typedef struct vits_resblock_pair_desc {
  const float* x;
  int64_t x_bstride;
  int32_t x_cstride;
  int32_t t_len;
  int32_t channels;
  float in_slope;
  const float* w1;
  int32_t m_pad1;
  int32_t cin_pad1;
  int32_t kc1;
  int32_t k;
  int32_t dil;
  int32_t kc2;
  const float* b1;
  const float* cond;
  int64_t cond_bstride;
  const float* w2;
  int32_t m_pad2;
  int32_t cin_pad2;
  const float* b2;
  float* y;
  int64_t y_bstride;
  int32_t y_cstride;
  int32_t accumulate;
  float post_div;
  int32_t len_skip;      /* as vits_conv1d_desc.len_skip                     */
  /* [B] valid lengths or NULL: the gated tensor is zero and the output 0  */
  /* at t >= lengths[b] (the utterance ends there, as the convs' masks)    */
  const int32_t* lengths;
} vits_resblock_pair_desc;
int vits_resblock_pair_forward(const vits_resblock_pair_desc* d, int n, int batch, void* stream);
int vits_resblock_pair_kc(int channels, int k, int dil, int* kc1, int* kc2);
/* The same pair for 16-bit models (csrc/resblock16.hip; modules.py:250-  */
/* 260 of a model.half() / bf16 Generator): wdtype VITS_WDT_BF16 / F16;   */
/* x and y are [B][C][T] tensors of that type (the float pointers of the  */
/* descriptor reinterpreted), w1 / w2 the 16-bit images                   */
/* [cin_pad/16][k][2][m_pad][8] of vits_conv1d_desc (w1's rows gate-      */
/* interleaved); kc1 / kc2 are ignored.  C = 32, 64, 128 or 256 (the    */
/* 256-channel pairs run csrc/resblock_f32p.hip's streamed-K tile in its  */
/* 16-bit mode; not for the _mean variant), odd k, (k - 1) * dil <= 96,  */
/* T % 4 == 0.                                                            */
int vits_resblock_pair16_forward(const vits_resblock_pair_desc* d, int n, int batch, int wdtype,
                                 void* stream);
/* The last pairs of a stage's n branches as ONE launch: d[0].y receives  */
/* (sum_i pair_i(d[i].x)) / n (models.py:311-313's branch mean; each      */
/* workgroup runs every member on its time tile and sums in registers);   */
/* the members share t_len and lengths; accumulate / post_div ignored.    */
int vits_resblock_pair16_mean_forward(const vits_resblock_pair_desc* d, int n, int batch,
                                      int wdtype, void* stream);
/* The same pair for the split-fp32 (VITS_WDT_F32P) 64-, 128- and 256-  */
/* channel stages of an fp32 Generator (csrc/resblock_f32p.hip;           */
/* modules.py:250-260): x / y fp32 [B][C][T], w1 / w2 the pre-split       */
/* images [cin_pad/16][k][2][3][m_pad][8] bf16 of vits_conv1d_desc (w1's  */
/* rows gate-interleaved); kc1 / kc2 ignored.  Bitwise the two-conv path  */
/* (c1 with the gate epilogue, c2 with the residual one).  Odd k,         */
/* (k - 1) * dil <= 96, T % 4 == 0, 16-byte aligned x rows.               */
int vits_resblock_pair_f32p_forward(const vits_resblock_pair_desc* d, int n, int batch,
                                    void* stream);
/* The last split-fp32 pairs of a 32-channel stage's n branches as ONE     */
/* launch: d[0].y receives ((pair_0 + pair_1) + pair_2) / n, bitwise the   */
/* accumulating launches (accumulate on members > 0, post_div = n on the   */
/* last) without their reads and writes of y.  The members share t_len,    */
/* lengths and y; accumulate / post_div are ignored.  C = 32 only.         */
int vits_resblock_pair_f32p_mean_forward(const vits_resblock_pair_desc* d, int n, int batch,
                                         void* stream);

/* ---------------------------------------------------------------------- */
/* One WN layer (modules.py:130-182) of an fp32 model as ONE kernel, in    */
/* the split-fp32 arithmetic (VITS_WDT_F32P; csrc/wn_f32p.hip):            */
/*   g = tanh(a) * sigmoid(b),  (a|b) = in_layer(h) + b1 + cond            */
/*   rs = res_skip(g) + b2;  h_out = h + rs[:H];  skip (+)= rs[H:]         */
/*   last layer: res_skip has H rows, skip (+)= rs, h_out = NULL           */
/* w1 = Conv1d(H, 2H, k, dil, 'same' padding) in the GATE row layout, w2   */
/* the 1x1 res_skip: the pre-split images [cin_pad/16][k][2][3][m_pad][8]  */
/* bf16 of vits_conv1d_desc; b1 / cond in logical order ([a | b], cond     */
/* already offset to this layer).  Bitwise the two launches it replaces    */
/* (in_layer with the gate epilogue, res_skip with the res + skip one).    */
/* h, h_out, skip: [B][H][T] fp32, time-contiguous; h 16-byte aligned with */
/* strides % 4 == 0, T % 4 == 0.  h_out and skip must not alias h: other   */
/* workgroups read h's halo columns.  hidden == 256, odd k, (k - 1) * dil  */
/* <= 64.  lengths: outputs are 0 at t >= lengths[b] (g is not masked, as  */
/* the gate conv); len_skip as vits_conv1d_desc.len_skip.  ng: columns per */
/* workgroup, 32 or 64; 0 = chosen by grid size (no bit depends on it).    */
/* ---------------------------------------------------------------------- */
typedef struct vits_wn_layer_desc {
  const float* h;
  int64_t h_bstride;
  int32_t h_cstride;
  int32_t t_len;
  int32_t hidden;
  int32_t k;
  int32_t dil;
  int32_t last;
  const void* w1;
  int32_t m_pad1;
  int32_t cin_pad1;
  const float* b1;
  const float* cond;
  int64_t cond_bstride;
  const void* w2;
  int32_t m_pad2;
  int32_t cin_pad2;
  const float* b2;
  float* h_out;
  int64_t ho_bstride;
  int32_t ho_cstride;
  int32_t accumulate;    /* skip += (every layer but the first)              */
  float* skip;
  int64_t skip_bstride;
  int32_t skip_cstride;
  int32_t len_skip;
  int32_t ng;
  int32_t reserved;
  const int32_t* lengths;
} vits_wn_layer_desc;
/* n layers in order (a WN stack), one host call.  Every descriptor is     */
/* checked before the first launch.                                        */
int vits_wn_layers_f32p_forward(const vits_wn_layer_desc* d, int n, int batch, void* stream);
/* Convs and fused WN layers in one ordered host call (a coupling's pre /  */
/* WN stack / post): kinds[i] = 0 takes the next of convs, 1 the next of   */
/* wn; n items in all, nconv + nwn == n.  Every descriptor is checked      */
/* before the first launch.                                                */
int vits_conv1d_wn_seq_forward(const vits_conv1d_desc* convs, int nconv,
                               const vits_wn_layer_desc* wn, int nwn, const int32_t* kinds, int n,
                               int batch, void* stream);

/* Fused RAdam step (radam.py:35-99, the D optimizer of train_stft.py:97) */
/* over a list of fp32 tensors, one launch per VITS_RADAM_MAX tensors.     */
/* scal: device float[8] state (scal[0] = step count, the rest scratch);  */
/* found_inf: device flag of GradScaler's unscale (NULL = never skip);    */
/* when set, nothing is updated (GradScaler's skip rule, no host sync).   */
/* grad_scale: device scalar the grads are still multiplied by (NULL =    */
/* already unscaled).  lr_dev: optional device double read at run time   */
/* instead of lr (an lr scheduler's in-place update then reaches a        */
/* captured hipGraph, train_stft.py:127-139 ExponentialLR).               */
#define VITS_RADAM_MAX 96
typedef struct vits_radam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
} vits_radam_tensor;
int vits_radam_step(const vits_radam_tensor* tensors, int n, float* scal, const float* found_inf,
                    const float* grad_scale, double lr, const double* lr_dev, double beta1,
                    double beta2, double eps, double weight_decay, void* stream);

/* ---------------------------------------------------------------------- */
/* Weight normalisation of many layers in one launch (legacy             */
/* torch.nn.utils.weight_norm, dim 0: the generator's convs, upsamplers   */
/* and conditioning Linears, modules.py:58-109, models.py:233; replaces   */
/* the per-layer torch._weight_norm / its backward of every forward).     */
/* Each layer is [rows][cols] (rows = size of dim 0), fp32, contiguous.  */
/* forward: w = v * (g / ||v_row||), norms[row] written (global row      */
/* index over all layers of the call, in order); backward (same layers,  */
/* same norms): dg = <dw,v>/n, dv = (g/n)(dw - v <dw,v>/n^2).            */
/* ---------------------------------------------------------------------- */
#define VITS_WNORM_MAX 56
typedef struct vits_wnorm_layer {
  const float* v;
  const float* g;
  float* w;        /* forward output */
  const float* dw; /* backward input */
  float* dv;       /* backward outputs */
  float* dg;
  int32_t rows;
  int32_t cols;
} vits_wnorm_layer;
int vits_weight_norm_forward(const vits_wnorm_layer* layers, int n, float* norms, void* stream);
int vits_weight_norm_backward(const vits_wnorm_layer* layers, int n, const float* norms,
                              void* stream);

/* ---------------------------------------------------------------------- */
/* Spectral normalisation of many layers at once (torch.nn.utils.        */
/* spectral_norm, dim 0, one power iteration per training forward, the   */
/* discriminators of mrd.py; replaces the per-layer forward pre-hooks).  */
/* forward (5 launches for all layers): training: v = normalize(W^T u),  */
/* u = normalize(W v), u / v updated in place; sigma = u . (W v);        */
/* w_sn = W / sigma; saved = [sigma, u (rows), v (cols)] of this call.   */
/* backward (2 launches): dw = dw_sn / sigma - (<dw_sn, W> / sigma^2)    */
/* u v^T, with a workspace of vits_spectral_norm_workspace floats.       */
/* emu16 = 1: the hook inside an fp16 autocast region (mv operands and   */
/* result rounded to fp16, as the reference's autocast mv).              */
/* ---------------------------------------------------------------------- */
#define VITS_SNORM_MAX 48
typedef struct vits_snorm_layer {
  const float* w;     /* weight_orig viewed [rows][cols] */
  float* u;           /* [rows] buffer */
  float* v;           /* [cols] buffer */
  float* w_sn;        /* forward output */
  const float* dw_sn; /* backward input */
  float* dw;          /* backward output */
  float* saved;       /* [1 + rows + cols] */
  int32_t rows;
  int32_t cols;
  float eps;
  int32_t cl_channels; /* 0: w_sn / dw_sn fp32 like w; C > 0: fp16 channels-  */
                       /* last [O][kh][kw][C] images of a Conv2d weight       */
                       /* [O][C][kh][kw] (the autocast MIOpen conv's operand) */
} vits_snorm_layer;
int vits_spectral_norm_supported(int rows, int cols);
int vits_spectral_norm_forward(const vits_snorm_layer* layers, int n, int training, int emu16,
                               void* stream);
int64_t vits_spectral_norm_workspace(const vits_snorm_layer* layers, int n);
int vits_spectral_norm_backward(const vits_snorm_layer* layers, int n, int emu16,
                                float* workspace, int64_t ws_floats, void* stream);

/* ---------------------------------------------------------------------- */
/* The residual / skip update between two WN layers of the fp16-autocast  */
/* training step (modules.py:93-182): x' = (x + rs[:, :H]) * mask (fp32), */
/* x16' = x' rounded to the 16-bit type (the next conv's input), out' =   */
/* out + rs[:, H:] (out NULL = 0); rs [B][2H][T] of the 16-bit type, x /  */
/* out / x' / out' [B][H][T] fp32, mask [B][1][T] fp32, all contiguous.   */
/* backward: G = dx' + dx16' (either NULL = 0), dx = G * mask, drs =      */
/* [G * mask ; dout'] rounded to the 16-bit type (dout' NULL = 0).        */
/* ---------------------------------------------------------------------- */
int vits_wn_update_forward(const float* x, const void* rs, const float* mask, const float* out,
                           float* x_new, void* x16_new, float* out_new, int batch, int H, int T,
                           int wdtype, void* stream);
int vits_wn_update_backward(const float* gx, const void* gx16, const float* gout,
                            const float* mask, float* dx, void* drs, int batch, int H, int T,
                            int wdtype, void* stream);

/* ---------------------------------------------------------------------- */
/* Mean-only coupling layer glue of the fp16-autocast training step       */
/* (ResidualCouplingLayer.forward modules.py:314-360, WN output           */
/* modules.py:182, Flip folded in: ResidualCouplingBlock models.py:219-235).*/
/* mask_cast: h = y * mask (fp32) and h16 = h in the 16-bit type;          */
/*   backward: dy = 16-bit((gh + gh16) * mask) (either NULL = 0).         */
/* wn_final: o16 = 16-bit((out + rs) * mask) (out NULL = 0); backward:    */
/*   d = g16 * mask, dout = d (fp32, NULL = skip), drs = 16-bit(d).       */
/* coupling: x [B][2h][T] fp32, p = post conv output [B][h][T] 16-bit,    */
/*   m = p * mask; out = cat(x0, reverse ? (x1 - m) * mask :              */
/*   m + x1 * mask), channel-reversed when flip; backward: gx0 = g0, gx1 = */
/*   g1 * mask, gp = 16-bit(+-g1 * mask) (g read through the same flip).  */
/* ---------------------------------------------------------------------- */
int vits_mask_cast_forward(const void* y, const float* mask, float* h, void* h16, int batch,
                           int C, int T, int wdtype, void* stream);
int vits_mask_cast_backward(const float* gh, const void* gh16, const float* mask, void* dy,
                            int batch, int C, int T, int wdtype, void* stream);
int vits_wn_final_forward(const float* out, const void* rs, const float* mask, void* o16,
                          int batch, int C, int T, int wdtype, void* stream);
int vits_wn_final_backward(const void* g16, const float* mask, float* dout, void* drs, int batch,
                           int C, int T, int wdtype, void* stream);
int vits_coupling_forward(const float* x, const void* p, const float* mask, float* out,
                          int batch, int half, int T, int reverse, int flip, int wdtype,
                          void* stream);
int vits_coupling_backward(const float* g, const float* mask, float* gx, void* gp, int batch,
                           int half, int T, int reverse, int flip, int wdtype, void* stream);

/* ---------------------------------------------------------------------- */
/* STFT-discriminator glue of the fp16-autocast training step             */
/* (mrd.py:94-156, STFTDiscriminator.forward: Conv2d -> LeakyReLU ...).   */
/* join_to_cl: the first layer's joined-row conv output y [B][C][F_out*L] */
/* (row f's T outputs at columns f*L + p1 ..) -> out [B][F_out][T][C]     */
/* (NHWC) = leaky_relu(y, slope); backward: dy [B][C][F_out*L] =          */
/* lrelu'(out) * g at output columns, 0 at pad columns.                   */
/* bias_lrelu: out = leaky_relu(y + fp16(bias), slope) on NHWC rows of C  */
/* channels (the MIOpen conv runs without bias); backward: dy = lrelu'(out)*g */
/* and db[c] = fp16-rounded fp32 sum of dy (deterministic: per-workgroup  */
/* partials in `workspace`, added in workgroup order by a second launch; */
/* db NULL: the data gradient only, one launch, no workspace).           */
/* 16-bit tensors of `wdtype`; C % 8 == 0, C <= 512 (bias_lrelu backward: */
/* 256 % (C/8) == 0).                                                      */
/* ---------------------------------------------------------------------- */
int vits_stftd_join_to_cl_forward(const void* y, void* out, int batch, int C, int F_out, int L,
                                  int p1, int T, float slope, int wdtype, void* stream);
int vits_stftd_join_to_cl_backward(const void* g, const void* out, void* dy, int batch, int C,
                                   int F_out, int L, int p1, int T, float slope, int wdtype,
                                   void* stream);
int vits_bias_lrelu_forward(const void* y, const float* bias, void* out, int64_t rows, int C,
                            float slope, int wdtype, void* stream);
int vits_bias_lrelu_workspace(int64_t rows, int C);
int vits_bias_lrelu_backward(const void* g, const void* out, void* dy, float* db,
                             float* workspace, int ws_floats, int64_t rows, int C, float slope,
                             int wdtype, void* stream);

/* ---------------------------------------------------------------------- */
/* PCM output stage of VITSWrap.speaking (vits_wrap.py:186-197): the pitch */
/* / sampling-rate resampling and the int16 conversion, on the device.     */
/* vits_resample_poly = scipy.signal.resample_poly(x, up, down) with its   */
/* defaults (Kaiser 5.0, zero extension), per row of x [batch][x_cap]      */
/* (`x_dtype` VITS_DT_F32 / _F16 / _BF16, row stride x_bstride elements):  */
/*   out[n] = sum_i x[i] * h[n*down - i*up + half_len], n < n_out =        */
/*   ceil(n_in * up / down), fp32 accumulation in a fixed order.           */
/* up / down are used as given: reduce them by their gcd to get scipy's    */
/* filter.  half_len = 10 * max(up, down); h has 2 * half_len + 1 taps     */
/* (float32(firwin(...)) * float32(up)) and is passed by phase: `table`    */
/* [table_rows = up][table_k = ceil((2 * half_len + 1) / up)] fp32,        */
/* table[r][k] = h[r + k * up], 0 past the last tap.  up == down == 1 is a */
/* copy (table ignored, may be NULL).                                      */
/* Row length n_in: `lens` NULL -> n_host for every row (then n_host >     */
/* x_cap or n_out > out_cap is VITS_E_SHAPE); else lens[b] * len_scale,    */
/* int32 [batch] read on the device and clamped to [0, x_cap] (n_out to    */
/* out_cap).  x at or past n_in counts as zero whatever the buffer holds.  */
/* Exactly one output, [batch][out_cap] with row stride out_bstride:       */
/* `out` fp32, or `pcm` int16 = clip(float32(float32(v * volume) * 32767), */
/* -32768, 32767) truncated toward zero (the host expression, bit for      */
/* bit).  Either is written as zero from n_out to out_cap.  `out_lens`     */
/* (int32 [batch], NULL = skip) receives n_out, so that a second pass can  */
/* take its lengths from the device.                                       */
/* vits_pcm16: the int16 conversion alone (n_out = n_in).                  */
/* ---------------------------------------------------------------------- */
int vits_resample_poly(const void* x, int x_dtype, int64_t x_bstride, int x_cap,
                       const int32_t* lens, int len_scale, int n_host, const float* table,
                       int table_rows, int table_k, int up, int down, int half_len, float* out,
                       int16_t* pcm, int64_t out_bstride, int out_cap, float volume,
                       int32_t* out_lens, int batch, void* stream);
int vits_pcm16(const void* x, int x_dtype, int64_t x_bstride, int x_cap, const int32_t* lens,
               int len_scale, int n_host, float volume, int16_t* pcm, int64_t out_bstride,
               int out_cap, int batch, void* stream);

/* vits_resample_poly_span: one row, one pass of the output stage over a   */
/* SPAN of the whole signal's output, from a WINDOW of its input (streamed */
/* synthesis).  x holds the samples [x_lo, x_lo + x_len) of  */
/* a signal of n_in samples; out[j], j < out_len, is output sample out_lo  */
/* + j of vits_resample_poly over the whole signal, bit for bit: the phase */
/* follows the global index and the sum is the same fp32 FMA chain in      */
/* ascending k over the inputs in [0, n_in) (the zero taps that pad a      */
/* phase row are not read).  Samples at or past n_out = ceil(n_in * up /   */
/* down) are written as zero up to out_len (the tail silence).  table,     */
/* table_rows, table_k, up, down, half_len, out / pcm and volume as for    */
/* vits_resample_poly; up == down == 1 is the copy (vits_pcm16 over a      */
/* span).  All offsets and lengths are host integers, counted in samples   */
/* of the whole signal.  VITS_E_ARG: a null pointer (x may be NULL only    */
/* with x_len == 0), a negative offset or size, both or neither output.    */
/* VITS_E_SHAPE: a table that is not this ratio's, an index beyond int64,  */
/* or a tap of a requested output that needs an input in [0, n_in) outside */
/* the window: that input range is, for the outputs [out_lo, e), e =       */
/* min(out_lo + out_len, n_out), [max(0, ceil((out_lo * down - half_len) / */
/* up)), min(n_in, floor(((e - 1) * down + half_len) / up) + 1)), or       */
/* [out_lo, e) for the copy.  Nothing outside x[0, x_len) is read; out_len */
/* == 0 launches nothing.                                                  */
int vits_resample_poly_span(const void* x, int x_dtype, int64_t x_lo, int64_t x_len, int64_t n_in,
                            const float* table, int table_rows, int table_k, int up, int down,
                            int half_len, float* out, int16_t* pcm, int64_t out_lo,
                            int64_t out_len, float volume, void* stream);

/* Ragged pack behind the last pass (a request's segments in one copy):    */
/* rows int16 [batch][cap] (row stride bstride) -> out int16 [out_cap]:     */
/* row b's first n_out[b] samples at out + offsets[b], then `tail` zeros;   */
/* n_out[b] = y_len[b] * hop passed through ceil(n * up[i] / down[i]) for   */
/* each of the n_passes <= 2 (reduced) ratios, offsets[b + 1] = offsets[b]  */
/* + n_out[b] + tail.  y_len int32 [batch] and *n_rows (NULL = batch) are   */
/* read on the device; rows at or past *n_rows add nothing.  offsets int32  */
/* [batch + 1].  Nothing is written at or past out_cap; samples past a      */
/* row's cap read as zero.  batch <= 64.                                    */
int vits_pack_pcm(const int16_t* rows, int64_t bstride, int cap, const int32_t* y_len, int hop,
                  const int32_t* up, const int32_t* down, int n_passes, int tail,
                  const int32_t* n_rows, int batch, int32_t* offsets, int16_t* out,
                  int64_t out_cap, void* stream);

/* ---------------------------------------------------------------------- */
/* Per-row output stage: the rows of one launch belong to different         */
/* requests, each with its own pitch, output rate, volume and tail.         */
/* vits_resample_poly_rows is vits_resample_poly with the ratio, filter and */
/* volume of row b taken from rows[b] (a HOST array of `batch` records,     */
/* copied into the kernel arguments: the call keeps no pointer to it):      */
/* up / down reduced, half_len = 10 * max(up, down), table [up][table_k]    */
/* with table_k = ceil((2 * half_len + 1) / up) as above, on the device; up */
/* == down == 1 is the copy (table ignored).  Every output sample is        */
/* computed exactly as vits_resample_poly computes it for that ratio.  The  */
/* row length is lens[b] * len_scale (device int32 [batch], required); out  */
/* / pcm is [batch][out_cap] for ONE shared out_cap, each row zero from its */
/* own n_out = ceil(n_in * up / down) (clamped to out_cap) to out_cap;      */
/* out_lens (NULL = skip) receives n_out.  batch <= 64.                     */
/* ---------------------------------------------------------------------- */
typedef struct {
  const float* table; /* device, [up][table_k]; NULL for up == down == 1 */
  int32_t up, down, half_len, table_k;
  float volume;       /* int16 output only */
  int32_t reserved;
} vits_post_row;
int vits_resample_poly_rows(const void* x, int x_dtype, int64_t x_bstride, int x_cap,
                            const int32_t* lens, int len_scale, const vits_post_row* rows,
                            float* out, int16_t* pcm, int64_t out_bstride, int out_cap,
                            int32_t* out_lens, int batch, void* stream);

/* vits_pack_pcm with per-row ratios and tails: up / down are HOST int32    */
/* [batch][2] (1 / 1 in a slot the row does not use), tail HOST int32       */
/* [batch] (>= 0); n_out[b] = y_len[b] * hop through ceil(n * up[b][i] /    */
/* down[b][i]), i = 0, 1; offsets[b + 1] = offsets[b] + n_out[b] + tail[b]. */
/* Everything else as vits_pack_pcm.                                        */
int vits_pack_pcm_rows(const int16_t* rows, int64_t bstride, int cap, const int32_t* y_len,
                       int hop, const int32_t* up, const int32_t* down, const int32_t* tail,
                       const int32_t* n_rows, int batch, int32_t* offsets, int16_t* out,
                       int64_t out_cap, void* stream);

/* ---------------------------------------------------------------------- */
/* Window copy of long-recording voice conversion: n_jobs <= 64 ranges of   */
/* fp32 elements in ONE launch.  For job j and channel r < channels:        */
/*   dst[dst_off + r * dst_rstride + i] = src[src_off + r * src_rstride + i]*/
/*                                                          for i < len,    */
/*   dst[dst_off + r * dst_rstride + i] = 0       for len <= i < fill_len,  */
/* and nothing else is written.  Offsets, lengths and strides count         */
/* elements; src_numel / dst_numel are the sizes of the two buffers, and a  */
/* job that reads or writes outside them is refused.  jobs is a HOST array, */
/* copied into the kernel arguments: the call keeps no pointer to it and    */
/* can be captured.  Accesses are 16 bytes wide where the source and the    */
/* destination of a (job, channel) are co-aligned, single elements          */
/* otherwise.  VITS_E_ARG: a null pointer, a pointer off a 4-byte boundary, */
/* n_jobs < 1, channels < 1, a negative offset, stride, size or length,     */
/* fill_len < len.  VITS_E_SHAPE: n_jobs > 64, channels > 65535, a job      */
/* outside its buffers, channels > 1 with dst_rstride < fill_len.           */
/* ---------------------------------------------------------------------- */
typedef struct {
  int64_t src_off, dst_off, len, fill_len;
} vits_window_job;
int vits_copy_windows(const float* src, int64_t src_numel, int64_t src_rstride, float* dst,
                      int64_t dst_numel, int64_t dst_rstride, const vits_window_job* jobs,
                      int n_jobs, int channels, void* stream);

/* ---------------------------------------------------------------------- */
/* Speech editing: tokens [a, b_old) of a recording's text   */
/* are replaced by tokens [a, b_new) of a new text; spans int32 [batch][3]  */
/* = a | b_old | b_new.  All lengths are read on the device, no call keeps  */
/* a host pointer, all three can be captured.  Durations are taken as       */
/* min(max(d, 0), 2^18), the clamp of the _int entry points.                */
/*                                                                          */
/* vits_edit_pins (one 256-thread workgroup per row): from the recording's  */
/* durations dur_old int32 [batch] rows of dur_old_bstride (token x <       */
/* x_len_old[b]), cum = their prefix sums, f0 = cum[a), f1 = cum[b_old):    */
/*   given[b][t] = dur_old[t]                 t < a                         */
/*               = span_given[b][t] (NULL: -1)   a <= t < b_new             */
/*               = dur_old[t - b_new + b_old]    b_new <= t < x_len_new[b]  */
/*               = -1                            x_len_new[b] <= t < t_x_new*/
/*   target[b]   = 0                           span_target NULL or [b] == 0 */
/*               = y_len_old[b] - (f1 - f0) + span_target[b]      [b] > 0   */
/*               = y_len_old[b]                 [b] < 0 (keep the length)   */
/*   meta int32 [3][batch] = f0 | f1 | status                               */
/* the inputs of vits_duration_plan over the new text.  status 1: a length  */
/* outside [0, t_x], a span that is not 0 <= a <= b_old <= x_len_old, a <=  */
/* b_new <= x_len_new with x_len_old - b_old == x_len_new - b_new, tokens   */
/* whose durations are all 0 (no alignment), or sum(dur_old) != y_len_old:  */
/* the row then gets given = 0 everywhere, target 0 and f0 = f1 = 0.        */
/* VITS_E_ARG: a NULL pointer other than span_given / span_target, batch <= */
/* 0, t_x <= 0; VITS_E_SHAPE: dur_old_bstride < t_x_old; VITS_E_UNSUP: a    */
/* t_x > 4096.                                                              */
/* ---------------------------------------------------------------------- */
int vits_edit_pins(const int32_t* dur_old, int64_t dur_old_bstride, const int32_t* x_len_old,
                   int t_x_old, const int32_t* x_len_new, int t_x_new, const int32_t* spans,
                   const int32_t* span_given, const int32_t* span_target,
                   const int32_t* y_len_old, int32_t* given, int32_t* target, int32_t* meta,
                   int batch, void* stream);

/* vits_edit_splice: the prior expansion of the new span and the splice in  */
/* one pass.  dur_new int32 [batch] rows of dur_bstride (the plan's, token  */
/* x < x_len_new[b], NULL: t_x), cum = their prefix sums, total = the last; */
/* the pins make the prefix and the suffix of dur_new the old durations, so */
/*   f0 = cum[a), n_new = cum[b_new) - f0, f1 = y_len_old - (total -        */
/*   cum[b_new)), y_new = total = f0 + n_new + (y_len_old - f1)             */
/*   z[b][c][t] = z_p_rec[b][c][t]                          t < f0          */
/*              = m[b][c][x(t)] + noise[b][c][t] * s[b][c][x(t)]            */
/*                                             f0 <= t < f0 + n_new         */
/*              = z_p_rec[b][c][t - n_new + (f1 - f0)]                      */
/*                                             f0 + n_new <= t < y_new      */
/*              = 0                                     y_new <= t < t_y    */
/* x(t) = the token with cum[x - 1] <= t < cum[x]; the product and the sum  */
/* are two rounded fp32 operations, vits_expand_durations_int's expression  */
/* at noise_scale 1.  m, s: [batch] of ms_bstride, channel rows of          */
/* ms_cstride; noise [batch][channels][t_y] is indexed by output frame and  */
/* read on the new span only; z_p_rec [batch][channels][t_rec] is read      */
/* below y_len_old only.  Every element of z is written.  lens int32        */
/* [n_stage][batch] = y_new * stage_mult[i]; meta int32 [4][batch] = f0 |   */
/* n_new | f1 | status.  status -1: y_new > t_y (f0, n_new, f1 are still    */
/* reported); status 1: not 0 <= a <= b_new <= x_len_new, b_old < a,        */
/* y_len_old outside [0, t_rec] or f1 < f0 (f0 = n_new = f1 = 0); either    */
/* way the row is zero and its lengths are 0.  Kept frames move as 16-byte  */
/* vectors where source and destination are co-aligned (z and z_p_rec on a  */
/* 16-byte boundary, t_y, t_rec and the suffix shift multiples of four; the */
/* zero fill past y_new needs z and t_y alone), else one by one.            */
/* VITS_E_ARG: a NULL pointer other than x_len_new, a z or z_p_rec off a    */
/* 4-byte boundary, a size <= 0, n_stage outside [1, 8]; VITS_E_SHAPE:      */
/* dur_bstride or ms_cstride < t_x, ms_bstride < 0, batch > 65535;          */
/* VITS_E_UNSUP: t_x > 4096.                                                */
int vits_edit_splice(const int32_t* dur_new, int64_t dur_bstride, const int32_t* x_len_new,
                     int t_x, const int32_t* spans, const int32_t* y_len_old, const float* m,
                     const float* s, int64_t ms_bstride, int32_t ms_cstride, const float* noise,
                     const float* z_p_rec, int t_rec, float* z, int batch, int channels, int t_y,
                     int32_t* lens, const int32_t* stage_mult, int n_stage, int32_t* meta,
                     void* stream);

/* vits_edit_patch: the waveform side.  orig [batch] rows of orig_bstride    */
/* (orig_cap samples, the recording at the model rate), o likewise (the     */
/* synthesis of the spliced latents), splice_meta = vits_edit_splice's      */
/* meta.  With Ty = y_len_old[b], y_new = f0 + n_new + Ty - f1, L = y_new * */
/* hop, margin in frames and fade in samples:                               */
/*   lo = max(f0 - margin, 0) * hop, hi = min(f0 + n_new + margin, y_new) * */
/*   hop, shift = (y_new - Ty) * hop;                                       */
/*   fade > 0 and lo - fade < 0: lo = 0 and no fade in; fade > 0 and hi +   */
/*   fade > L: hi = L and no fade out (the synthesis runs to that end);     */
/*   out[i] = orig[i]                                      i < lo - fade    */
/*          = orig[i] * (1 - w) + o[i] * w, w = (j + 0.5f) / fade,          */
/*            j = i - (lo - fade)                    lo - fade <= i < lo    */
/*          = o[i]                                         lo <= i < hi     */
/*          = orig[i - shift] * (1 - w) + o[i] * w, w = (j + 0.5f) / fade,  */
/*            j = hi + fade - 1 - i                  hi <= i < hi + fade    */
/*          = orig[i - shift]                        hi + fade <= i < L     */
/*          = 0                                      L <= i < out_cap       */
/* j + 0.5f, the division, 1 - w, the two products and their sum are six    */
/* separately rounded fp32 operations (no contraction).  out_len int32      */
/* [batch] = L.  A row whose splice status is not 0, or whose Ty * hop >    */
/* orig_cap or L > o_cap or L > out_cap, is zero with out_len 0.            */
/* VITS_E_ARG: a NULL pointer, batch / cap / hop <= 0, margin or fade < 0;  */
/* VITS_E_SHAPE: a row stride below its cap, batch > 65535.                 */
int vits_edit_patch(const float* orig, int64_t orig_bstride, int orig_cap, const float* o,
                    int64_t o_bstride, int o_cap, const int32_t* y_len_old,
                    const int32_t* splice_meta, int hop, int margin, int fade, float* out,
                    int64_t out_bstride, int out_cap, int32_t* out_len, int batch, void* stream);

/* ---------------------------------------------------------------------- */
/* Retiming a recording: the recording's own latents are     */
/* resampled along time, token by token.  All lengths are read on the       */
/* device, no call keeps a host pointer, both can be captured.  Durations   */
/* and pins are taken as min(max(d, 0), 2^18), the clamp of the _int entry  */
/* points.                                                                  */
/*                                                                          */
/* vits_retime_plan (one 256-thread workgroup per row): a row's old         */
/* durations dur_old int32 [batch] rows of dur_old_bstride (token x <       */
/* x_len[b], NULL: t_x) to its new ones.  Optional (NULL = none): given     */
/* int32 [batch][t_x] (>= 0 pins the token to that many frames, < 0 leaves  */
/* it free), tok_scale fp32 [batch][t_x] (NULL: 1), rate fp32 [batch]       */
/* (NULL: 1), target int32 [batch] (> 0: the row lasts exactly that many    */
/* frames, <= 0: none).  With F = the free tokens and P = the sum of the    */
/* pins, in token order over F:                                             */
/*   s[x]  = fminf(fmaxf(tok_scale[x] * rate, 2^-8), 2^8)   one fp32        */
/*           product; rate is taken as 1 when the row has a target; a NaN   */
/*           becomes 2^-8                                                   */
/*   q[x]  = llrint((double)dur_old[x] * (double)s[x] * 256.0)   (exact: 42 */
/*           significant bits; ties to even)                                */
/*   Q[x]  = inclusive prefix sum of q over F, Qtot = its last (int64)      */
/*   E     = target ? target - P : (Qtot + 128) >> 8                        */
/*   B[x]  = (Q[x] * E + Qtot / 2) / Qtot       (int64 division; Qtot == 0: */
/*           every B is 0)                                                  */
/*   d[x]  = B[x] - B[previous free token]      (B = 0 before the first)    */
/*   dur_new[x] = pin, or d[x]; 0 for x_len <= x < t_x                      */
/* so that the free tokens sum to E exactly, a free token may get 0 frames, */
/* nothing depends on a summation order, and with no control q = 256 *      */
/* dur_old, E = sum(dur_old) and dur_new == dur_old.  A consistent row has  */
/* Qtot <= 2^34 and E <= 2^26 (2^24 with a target): Q * E <= 2^60.          */
/* meta int32 [2][batch] = total (the sum of dur_new) | status.  status 1   */
/* (the row gets dur_new = dur_old): sum(dur_old[:x_len]) != y_len_old,     */
/* y_len_old > 2^18, E < 0, target > 2^24, or a target with Qtot == 0 and   */
/* E != 0.                                                                  */
/* VITS_E_ARG: NULL dur_old / y_len_old / dur_new / meta, batch <= 0, t_x   */
/* <= 0; VITS_E_SHAPE: dur_old_bstride < t_x; VITS_E_UNSUP: t_x > 4096.     */
/* ---------------------------------------------------------------------- */
int vits_retime_plan(const int32_t* dur_old, int64_t dur_old_bstride, const int32_t* x_len,
                     int t_x, const int32_t* y_len_old, const int32_t* given,
                     const float* tok_scale, const float* rate, const int32_t* target,
                     int32_t* dur_new, int32_t* meta, int batch, void* stream);

/* vits_retime_warp (256 threads per 64 output frames of a row): z_p_rec    */
/* fp32 [batch][channels][t_rec], read below y_len_old only, to z fp32      */
/* [batch][channels][t_y], every element written.  c_old / c_new = the      */
/* exclusive prefix sums of dur_old / dur_new (rows of their bstride, token */
/* x < x_len[b], NULL: t_x), y_new = sum(dur_new).  For t < y_new, with i   */
/* the token that owns frame t (c_new[i] <= t < c_new[i] + dur_new[i];      */
/* tokens of 0 new frames own nothing), k = t - c_new[i], dn = dur_new[i],  */
/* do = dur_old[i], in int64:                                               */
/*   num = (2k + 1) * do - dn, den = 2 * dn                                 */
/*   qf = floor(num / den), r = num - qf * den                              */
/*   j0 = clamp(c_old[i] + qf, 0, y_len_old - 1)                            */
/*   j1 = clamp(c_old[i] + qf + 1, 0, y_len_old - 1)                        */
/*   w  = (float)r / (float)den        (exact operands, one correctly       */
/*        rounded fp32 division)                                            */
/*   z[t] = (r == 0 || j0 == j1) ? z_p_rec[j0]                              */
/*        : z_p_rec[j0] + w * (z_p_rec[j1] - z_p_rec[j0])                   */
/* a rounded subtraction, product and sum (no contraction); z[t] = 0 for    */
/* y_new <= t < t_y.  This is the centre-aligned piecewise-linear map of    */
/* each token's new frames onto its old ones ((k + 1/2) * do / dn - 1/2),   */
/* continuous across token boundaries, the exact copy where dn == do.       */
/* lens int32 [n_stage][batch] = y_new * stage_mult[i] (NULL with n_stage   */
/* 1: 1); meta int32 [2][batch] = y_new | status.  status -1: y_new > t_y,  */
/* y_len_old <= 0 or y_len_old > t_rec; the row is then zero and its lens   */
/* are 0, meta still reports y_new.                                         */
/* VITS_E_ARG: a NULL pointer other than x_len, a z or z_p_rec off a 4-byte */
/* boundary, a size <= 0, n_stage outside [1, 8]; VITS_E_UNSUP: t_x > 4096, */
/* t_rec or t_y > 2^18; VITS_E_SHAPE: a bstride < t_x, batch > 65535.       */
int vits_retime_warp(const float* z_p_rec, int t_rec, const int32_t* dur_old,
                     int64_t dur_old_bstride, const int32_t* dur_new, int64_t dur_new_bstride,
                     const int32_t* x_len, int t_x, const int32_t* y_len_old, float* z, int batch,
                     int channels, int t_y, int32_t* lens, const int32_t* stage_mult, int n_stage,
                     int32_t* meta, void* stream);

/* library introspection */
const char* vits_amd_version(void);
int vits_amd_device_arch(char* buf, int len);

/* Dispatch counters: how many kernel launches each family of entry points */
/* has issued since the last reset (host-side counts, one per launched     */
/* kernel, incremented only when the launch was accepted).  Tests use them */
/* to prove that a step ran on this library's kernels (not a torch path).  */
#define VITS_CNT_CONV_F32 0      /* vits_conv1d_forward*: exact fp32 MFMA    */
#define VITS_CNT_CONV_SPLIT 1    /*   split fp32 (VITS_WDT_F32S / F32P)     */
#define VITS_CNT_CONV_16 2       /*   bf16 / fp16 operands                  */
#define VITS_CNT_WGRAD_F32 3     /* vits_conv1d_wgrad(_split), fp32 operands */
#define VITS_CNT_WGRAD_16 4      /*   16-bit operands                       */
#define VITS_CNT_GATE_F32 5      /* vits_gate_forward / _backward           */
#define VITS_CNT_GATE_16 6       /* vits_gate_*_io16                        */
#define VITS_CNT_RESBLOCK 7      /* vits_resblock_pair*_forward             */
#define VITS_CNT_PACK 8          /* vits_conv1d_pack*                       */
#define VITS_CNT_ATTN 9          /* vits_attention_train_forward / _backward */
#define VITS_CNT_N 10
int64_t vits_dispatch_count(int which);
void vits_dispatch_count_reset(void);

/* Test hook: which conv kernel vits_conv1d_forward / one shared-grid group */
/* of vits_conv1d_forward_groups would launch for d[0..n) at `batch`.  It   */
/* runs the launch path itself (descriptor checks, global-A choice, small-  */
/* grid fallback, staging kind, budgets) up to the launch and stops there:  */
/* a plain host function - no device needed, no pointer dereferenced (their */
/* values are read for alignment only), no dispatch counter bumped.         */
/* Returns what the launch would: VITS_OK with *out filled, or the refusal */
/* (VITS_E_UNSUP for mixed staging kinds or an over-budget chunk, ...).     */
#define VITS_PLAN_EPI_STORE2 3  /* plan.epi: STORE with two outputs (split < m) */
typedef struct vits_conv1d_plan_t {
  int32_t wdtype;    /* VITS_WDT_* of the kernel                             */
  int32_t ga;        /* 16-bit kinds: weight fragments read from global memory */
  int32_t bm, bn;    /* workgroup tile (after the small-grid fallback)       */
  int32_t waves_m, waves_n;
  int32_t v4;        /* 16-byte-block X staging (else element-wise)          */
  int32_t io16;      /* 16-bit activations                                    */
  int32_t epi;       /* VITS_EPI_*, or VITS_PLAN_EPI_STORE2                  */
  int32_t up_lds;    /* UPSAMPLE: the LDS-staged plain store is taken        */
  int32_t lds_bytes; /* dynamic LDS of the launch                            */
  int32_t grid[3];
} vits_conv1d_plan_t;
int vits_conv1d_plan(const vits_conv1d_desc* d, int n, int batch, vits_conv1d_plan_t* out);

#ifdef __cplusplus
}
#endif
#endif /* VITS_AMD_H */
