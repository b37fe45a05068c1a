/*
 * stylemc_hip.h -- C ABI of the MI355X (gfx950) kernels for StyleMC's find_direction hot path.
 *
 * Conventions (all entry points):
 *   - extern "C", plain device pointers + explicit sizes, fp32 NCHW-contiguous tensors.
 *   - `stream` is a hipStream_t passed as void* (NULL = legacy default stream).  Kernels are
 *     enqueued asynchronously; nothing synchronises the host.
 *   - Return SMC_OK (0) or an SMC_ERR_* code; smc_last_error() returns a thread-local message.
 *   - The caller owns every buffer.  Nothing allocates device memory internally: ops that need
 *     scratch space take a `workspace` whose size the matching *_workspace_size() query returns.
 *   - Pointers documented "may be NULL" mean "absent" (the reference passes empty tensors for that,
 *     torch_utils/ops/bias_act.py:39,150-157).
 *
 * Each entry point cites the reference interface it replaces.
 */
#ifndef STYLEMC_HIP_H
#define STYLEMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMC_ABI_VERSION 6

#define SMC_OK 0
#define SMC_ERR_INVALID 1     /* bad argument / shape (reference: TORCH_CHECK -> RuntimeError)   */
#define SMC_ERR_UNSUPPORTED 2 /* valid request this build has no kernel for                       */
#define SMC_ERR_LAUNCH 3      /* hipGetLastError() after a launch was not hipSuccess             */

/* activation codes: identical to the reference's cuda_idx (torch_utils/ops/bias_act.py:23-33) */
#define SMC_ACT_LINEAR 1
#define SMC_ACT_RELU 2
#define SMC_ACT_LRELU 3
#define SMC_ACT_TANH 4
#define SMC_ACT_SIGMOID 5
#define SMC_ACT_ELU 6
#define SMC_ACT_SELU 7
#define SMC_ACT_SOFTPLUS 8
#define SMC_ACT_SWISH 9

int smc_abi_version(void);

/* Batch-invariant planning.  Split-K factors, tile configurations and channel splits are normally chosen per call
 * to fill the chip, so the same image computed in a batch of 2 and in a batch of 4 may be summed in a different fp32
 * order.  After smc_set_plan_batch(plan, local) every such decision for a call on n images (m rows of a token-major
 * GEMM) is made as for n * plan / local images (m * plan / local rows): a data-parallel shard of `local` images of
 * a `plan`-image batch then computes each image bit for bit as the whole batch does.  (0, 0) restores the default.
 * Process-wide; set it from the thread that enqueues the work, before enqueueing it. */
int smc_set_plan_batch(int plan, int local);
const char* smc_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * bias_act -- replaces the pybind `_plugin.bias_act(x, b, xref, yref, dy, grad, dim, act, alpha,
 * gain, clamp)` of torch_utils/ops/bias_act.cpp:32-90 (called at bias_act.py:153,182,201).
 *   bias index of element i = (i / step_b) % size_b   (step_b = x.stride(dim), size_b = b.numel())
 *   grad 0: y = clamp(act(x + b) * gain)
 *   grad 1: y = d/dx   (x holds the incoming gradient, xref/yref the saved forward tensors)
 *   grad 2: second-order term (only for activations with a 2nd derivative)
 * b, xref, yref, dy may be NULL.  clamp < 0 disables clamping.
 */
int smc_bias_act_f32(const float* x, const float* b, const float* xref, const float* yref, const float* dy,
                     float* y, int64_t numel, int64_t size_b, int64_t step_b, int grad, int act, float alpha,
                     float gain, float clamp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * upfirdn2d -- replaces `_plugin.upfirdn2d(x, f, upx, upy, downx, downy, padx0, padx1, pady0, pady1,
 * flip, gain)` of torch_utils/ops/upfirdn2d.cpp:16-94 (called at upfirdn2d.py:237-240).
 *   x [major, in_h, in_w], f [fh, fw] (device fp32), y [major, out_h, out_w] with
 *   out_h = (in_h*upy + pady0 + pady1 - fh + downy) / downy  (checked).
 *   flip = 0: convolution (taps flipped), 1: correlation.  Negative padding crops.
 */
int smc_upfirdn2d_f32(const float* x, const float* f, float* y, int64_t major, int in_h, int in_w, int out_h,
                      int out_w, int fh, int fw, int upx, int upy, int downx, int downy, int padx0, int padx1,
                      int pady0, int pady1, int flip, float gain, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Modulated convolution (replaces the cuDNN grouped F.conv2d / F.conv_transpose2d of
 * torch_utils/ops/conv2d_resample.py:29-54,125-147 driven by the upstream modulated_conv2d).
 * The build uses the non-fused form: x*s -> shared-weight conv -> *d[n,o] -> +noise -> bias_act,
 * mathematically identical to the reference's fused grouped conv, without per-sample weights.
 *
 * smc_conv_gemm_f32 is an implicit-GEMM "gather convolution" on MFMA (v_mfma_f32_32x32x2_f32):
 *   for every phase p, output position (a, b) in [0,out_h) x [0,out_w) of sample n:
 *     acc[n,o,a,b] = sum_{t < ntaps, i < cin} W_p[t][i][o] * s[n,i] * x[n, i, a*in_stride + tap_dy[t],
 *                                                                      b*in_stride + tap_dx[t]]
 *   (out-of-range input reads are 0), written to y[n, o, out_oy + out_sy*a, out_ox + out_sx*b]
 *   through the epilogue.  One phase = a plain (strided) conv; four phases = the polyphase
 *   stride-2 transposed conv of the up=2 layers.
 */
typedef struct {
    int ntaps;            /* 1..9                                             */
    int tap_dy[9];
    int tap_dx[9];
    int in_stride;        /* 1 or 2                                           */
    int out_h, out_w;     /* output grid of this phase                        */
    int out_oy, out_ox;   /* offset of the grid in y                          */
    int out_sy, out_sx;   /* stride of the grid in y                          */
    const float* wk;      /* [ntaps][cin][cout] packed weights                */
    const float* wino_u;  /* optional (IR-SE50 executor): Winograd F(2x2) taps of a 9-tap 3x3 stride-1 'same'
                             phase from smc_wino_taps_f32, used for its <= 16x16 planes; NULL = none        */
    const void* wk_x3;    /* optional: wk split into three bf16 terms (smc_conv_weights_x3).  When every phase of a
                             call has them, the LDS-DMA GEMM runs the fp32 products as split-bf16 MFMAs (each
                             operand a = a0 + a1 + a2 exactly, the six products a_i b_j with i + j <= 2: error per
                             product <= 2^-23 |a b|, fp32-class) at 6/16 of the fp32 MFMA's cost; the per-sample
                             weights of a style-scaled call are split on the fly.  NULL = exact-fp32 MFMA        */
} smc_conv_phase;

/* Bytes of the split-bf16 planes of a phase's [ntaps][cin][cout] weights (cin % 16 == 0; 0 = unsupported), and
 * the planes themselves: layout [ntaps][cin/16][3 terms][2 octets][cout][8] bf16, term s of wk[t][16c + 8q + e][o]
 * at ((((t*(cin/16) + c)*3 + s)*2 + q)*cout + o)*8 + e; wk_x3 16-B aligned. */
int64_t smc_conv_weights_x3_bytes(int ntaps, int cin, int cout);
int smc_conv_weights_x3(const float* wk, int ntaps, int cin, int cout, void* wk_x3, void* stream);

#define SMC_EPI_STORE 0   /* y = acc                                                           */
#define SMC_EPI_MODACT 1  /* u = acc; y = clamp(act(u*d[n,o] + noise*strength + bias[o])*gain)  */
/* modes of the IR-SE50 (ArcFace) convolutions, id_loss/model_irse.py:                           */
#define SMC_EPI_PRELU 2      /* z = acc*scale_c[o] + bias[o]; u_save = z; y = z >= 0 ? z : alpha_c[o]*z */
#define SMC_EPI_PRELU_GRAD 3 /* y = acc * (act_ref >= 0 ? 1 : alpha_c[o])  (PReLU backward)          */
#define SMC_EPI_AFFINE 4     /* y = acc*scale_c[o] + bias[o]  (eval-mode BatchNorm)                  */

typedef struct {
    int mode;                      /* SMC_EPI_*                                                  */
    const float* d;                /* [n][cout] demodulation coefficients, may be NULL (=1)       */
    const float* noise;            /* may be NULL; element = noise[n*noise_nstride + y*W + x]     */
    int64_t noise_nstride;         /* 0 for the const [H, W] noise buffer                          */
    const float* noise_strength;   /* device scalar, may be NULL (=1)                             */
    const float* bias;             /* [cout], may be NULL                                          */
    int act;                       /* SMC_ACT_* (linear / relu / lrelu on this path)               */
    float alpha, gain, clamp;      /* clamp < 0: none                                              */
    float* u_save;                 /* may be NULL: stores u (pre-demod acc), layout of y            */
    const float* scale_c;          /* [cout] per-channel scale (multiplies d in MODACT), may be NULL */
    const float* alpha_c;          /* [cout] PReLU slopes (PRELU / PRELU_GRAD)                      */
    const float* act_ref;          /* PRELU_GRAD: the saved pre-activation, layout of y             */
    const float* residual;         /* may be NULL: added last, [n][cout][y_h/rs][y_w/rs] at the      */
    int residual_stride;           /*   positions with y % rs == 0 and x % rs == 0 (rs 0 -> 1)      */
    int grad_from_y;               /* MODACT backward entry points (act_bwd, blur_act_bwd): their `u`
                                    * argument holds the forward OUTPUT y instead of u -- the
                                    * activation mask needs only y, so a layer whose styles need no
                                    * gradient saves no u -- and dd must be NULL (it needs u)         */
} smc_conv_epilogue;

/* bytes of workspace smc_conv_gemm_f32 needs for these sizes (0 = none). */
/* nonzero if the last smc_conv_gemm_f32 call of this thread launched the split-bf16 kernels (the phases carried wk_x3
 * and the LDS-DMA tiles took the shape; 2: the 256-channel wide tile), 0 if it ran exact-fp32 products (timing /
 * roofline attribution, tests). */
int smc_conv_gemm_last_x3(void);
int64_t smc_conv_gemm_workspace_size(int n, int cin, int cout, int y_h, int y_w, const smc_conv_phase* phases,
                                     int nphases);

/* Route report of the last smc_conv_gemm_f32 / smc_conv_gemm_aux_f32 call of this thread (tests, attribution; no
 * launch decision reads it).  A route is one kernel instantiation of the dispatcher, numbered 1 ..
 * smc_conv_gemm_route_count() - 1 and named by its kernel template and parameters (smc_conv_gemm_route_name; NULL
 * outside the range); 0 ("none") when the call failed before its launch.  The names are the stable identity of a
 * route; the numbers are an index into the names for one build of the library and shift when a route is added or
 * removed, so compare names, never numbers, across builds.  The flags are the modifiers of that launch: */
#define SMC_ROUTE_SPLIT_K 1     /* split-K partial planes, summed by the epilogue pass                  */
#define SMC_ROUTE_PER_SAMPLE 2  /* tiles restarted per image (style-scaled input, straddling tiles)      */
#define SMC_ROUTE_PRESCALE 4    /* x * s written to the workspace, shared weights                        */
#define SMC_ROUTE_WSAMPLE 8     /* per-sample weights W * s built in the workspace                       */
int smc_conv_gemm_last_route(void);
int smc_conv_gemm_last_route_flags(void);
int smc_conv_gemm_route_count(void);
const char* smc_conv_gemm_route_name(int route);

int smc_conv_gemm_f32(const float* x, int n, int cin, int in_h, int in_w, float* y, int cout, int y_h, int y_w,
                      const smc_conv_phase* phases, int nphases, const float* s_in, const smc_conv_epilogue* epi,
                      float* workspace, int64_t workspace_bytes, void* stream);

/* The IR-SE50 executor's planning (its own split-K target and its TAG-1 kernel instantiations), exported so its
 * instantiations can be verified directly: same arguments and semantics as smc_conv_gemm_workspace_size /
 * smc_conv_gemm_f32. */
int64_t smc_conv_gemm_aux_workspace_size(int n, int cin, int cout, int y_h, int y_w, const smc_conv_phase* phases,
                                         int nphases);
int smc_conv_gemm_aux_f32(const float* x, int n, int cin, int in_h, int in_w, float* y, int cout, int y_h, int y_w,
                          const smc_conv_phase* phases, int nphases, const float* s_in, const smc_conv_epilogue* epi,
                          float* workspace, int64_t workspace_bytes, void* stream);

/* Convolution weight gradient (replaces the weight-gradient calls of torch_utils/ops/conv2d_gradfix.py, the cuDNN
 * conv2d_weight / conv_transpose2d weight gradient behind its Conv2dGradWeight), an implicit GEMM on the exact-fp32
 * MFMA with M = cout, N = cin x taps, K = n * out_h * out_w:
 *   dw[o][i][ky][kx] = sum_{n,a,b} grad[n,o,a,b] * inp[n, i, a*stride + ky - pad_y, b*stride + kx - pad_x]
 * (reads outside inp are 0): the weight gradient of the cross-correlation F.conv2d computes.  inp [n][cin][in_h][in_w],
 * grad [n][cout][out_h][out_w], dw [cout][cin][kh][kw].  With the roles swapped -- inp = the gradient of a stride-2
 * transposed conv's output [n][cout][2h+1][2w+1], grad = that layer's input x [n][cin][h][w], stride 2, pad 0 -- the
 * result [cin][cout][kh][kw] is conv_transpose2d's weight gradient in its own layout.
 * Supported: kh == kw in {1, 3}, stride in {1, 2}, pads in 0..2, any cin, cout >= 1 (tile edges are masked), any
 * n, in_h, in_w >= 1 with out = (in + 2 pad - k) / stride + 1 and every tensor below 2 GiB; anything else returns
 * SMC_ERR_INVALID from host-side validation, before any launch.  K is split across workgroups to fill the chip: each
 * split writes a partial dw into `workspace` (smc_conv_wgrad_workspace_size() bytes, 0: no split) and a second kernel
 * sums the partials in split order -- no atomics, bit-identical from run to run.  smc_conv_wgrad_last_nsplit(): the
 * split count of this thread's last successful call (a record; no launch decision reads it).
 * Added under ABI version 6 without a version bump: callers detect these three entry points by symbol. */
int64_t smc_conv_wgrad_workspace_size(int n, int cin, int cout, int in_h, int in_w, int out_h, int out_w, int kh,
                                      int kw, int stride);
int smc_conv_wgrad_f32(const float* inp, int n, int cin, int in_h, int in_w, const float* grad, int cout, int out_h,
                       int out_w, int kh, int kw, int stride, int pad_y, int pad_x, float* dw, float* workspace,
                       int64_t workspace_bytes, void* stream);
int smc_conv_wgrad_last_nsplit(void);

/* Winograd F(2x2, 3x3) form of the 3x3 stride-1 pad-1 convolution (the SynthesisLayer conv1 forward and its
 * data gradient -- the one-phase smc_conv_gemm_f32 call with taps (dy, dx) in {-1,0,1}^2), same operands and
 * epilogue semantics (modes STORE / MODACT / PRELU / PRELU_GRAD / AFFINE, no split-K workspace):
 *   acc[n,o,y,x] = sum_{c,dy,dx} W[o][c][dy+1][dx+1] * s[n,c] * x[n, c, y+dy, x+dx]
 * uw holds the transformed taps written by smc_wino_weights_f32 (flip 0 for this forward form).
 * smc_conv3x3_wino_supported() says whether a shape has a kernel: n >= 1, cin % 8 == 0 (>= 8), cout % 32 == 0
 * (>= 32), the input n cin h w below 2 GiB, and a block of 64 tiles (2 x 2 outputs each) that divides the image's
 * tile grid -- 2 tile rows x 32 tile columns (w % 64 == 0 and h % 4 == 0) or, failing that, 4 x 16 (w % 32 == 0 and
 * h % 8 == 0).  (h even, w % 4 == 0 and w >= 32 are implied but do not suffice: h = 6, w = 64 has no kernel.)
 * Unsupported shapes return SMC_ERR_UNSUPPORTED. */
int smc_conv3x3_wino_supported(int n, int cin, int cout, int h, int w);
int smc_conv3x3_wino_f32(const float* x, int n, int cin, int h, int w, float* y, int cout, const float* uw,
                         const float* s_in, const smc_conv_epilogue* epi, void* stream);
/* The same conv with split K for grids too small to fill the chip (smc_conv3x3_wino_workspace_size() > 0: fewer than
 * 512 work items): K splits write raw partial tiles into `workspace` and smc_modconv_epilogue_f32 sums them and
 * applies `epi`.  A NULL / too small workspace runs the single-pass kernel.
 * smc_conv3x3_wino_workspace_size() = split bytes + fold bytes (0 for an unsupported shape):
 *   split: with items = n * (h w / 256) * (cout / 32) work items (n: the planning batch, smc_set_plan_batch) and
 *     cin / 8 K steps, the split count doubles from 1
 *     while items * splits < 512 and the steps divide into 2 * splits parts of at least 8; splits > 1 take
 *     splits * n * cout * h * w * 4 bytes rounded up to 256, else 0;
 *   fold: n * cin * cout * 64 bytes of per-image taps with the style s[n, c] folded in when cin * cout <= 128 * 128
 *     (used by a call that passes s_in and the workspace), else 0. */
int64_t smc_conv3x3_wino_workspace_size(int n, int cin, int cout, int h, int w);
int smc_conv3x3_wino_ws_f32(const float* x, int n, int cin, int h, int w, float* y, int cout, const float* uw,
                            const float* s_in, const smc_conv_epilogue* epi, float* workspace, int64_t workspace_bytes,
                            void* stream);
/* Route report of the last smc_conv3x3_wino_f32 / smc_conv3x3_wino_ws_f32 call of this thread, as for
 * smc_conv_gemm_f32 (tests, attribution; no launch decision reads it): the kernel instantiation, numbered 1 ..
 * smc_conv3x3_wino_route_count() - 1 and named as written in its launch -- wino_kernel<TC,SM,EK> (TC tile columns of
 * the block; SM 1: style scale in the kernel, 2: none; EK 0: generic epilogue, 1: MODACT lrelu + clamp, 2: MODACT
 * linear, 3: split-K partials), wino_x3r_kernel<EK> -- by smc_conv3x3_wino_route_name (NULL outside the range; the
 * names are the stable identity, the numbers an index into them for one build); 0 ("none") when the call failed
 * before its launch.  Flags: SMC_ROUTE_SPLIT_K, and
 * SMC_ROUTE_WINO_FOLD when the style was folded into per-image taps in the workspace first (the launch then runs
 * SM = 2).  smc_conv3x3_wino_last_nsplit(): the K splits of that launch (1: one pass).
 * Added under ABI version 6 without a version bump: callers detect these entry points by symbol. */
#define SMC_ROUTE_WINO_FOLD 16
int smc_conv3x3_wino_last_route(void);
int smc_conv3x3_wino_last_route_flags(void);
int smc_conv3x3_wino_last_nsplit(void);
int smc_conv3x3_wino_route_count(void);
const char* smc_conv3x3_wino_route_name(int route);
/* The plan of a smc_conv3x3_wino_ws_f32 call, without the call (host only, no device call): the route, flags and K
 * splits that a call of this shape would report, with a style scale or not (has_style), this epilogue (NULL: the plain
 * store) and a workspace of workspace_bytes (0: none).  Of epi only the fields are read, no memory behind its
 * pointers.  Returns SMC_ERR_UNSUPPORTED (route 0) where smc_conv3x3_wino_supported() is 0.  Any of route, flags,
 * nsplit may be NULL.  Added under ABI version 6 without a version bump, as the route report. */
int smc_conv3x3_wino_plan(int n, int cin, int cout, int h, int w, int has_style, const smc_conv_epilogue* epi,
                          int64_t workspace_bytes, int* route, int* flags, int* nsplit);
/* Experimental split-bf16 F(2x2) for cin = cout = 32, w % 64 == 0, h % 4 == 0 (the r = 1024 conv1), taken by
 * smc_conv3x3_wino_ws_f32 with its workspace when enabled: mode 0 off (the default: slower in the full step,
 * profiles/r06/wino_x3/README), 1 for the MODACT lrelu form, 2 also for the linear form.  Process-wide; returns the
 * previous mode.  The workspace size follows the mode in force. */
int smc_set_wino_x3(int mode);
/* w [cout][cin][3][3] -> uw [K][4][N][4] floats (16 * cin * cout, 16-B aligned), U = G g G^T per (k, n):
 * flip = 0: K = cin, N = cout, g = w[n][k] (the forward correlation);
 * flip = 1: K = cout, N = cin, g = w[k][n] rotated 180 degrees (the data gradient, conv^T). */
int smc_wino_weights_f32(const float* w, int cout, int cin, int flip, float* uw, void* stream);

/* Winograd F(4x4, 3x3) form of the same convolution (4x4 output tiles, 36 multiplies per channel pair instead of
 * 144; interpolation points 0, +-1, +-2), same operands and epilogue semantics as smc_conv3x3_wino_f32 and the same
 * C-ABI contract (replaces the same grouped conv2d of conv2d_resample.py:147-154).  uw holds the taps written by
 * smc_wino4_weights_f32.  smc_conv3x3_wino4_supported(): n >= 1, cin % 4 == 0 (>= 4), w % 64 == 0 (>= 64),
 * h % 8 == 0 (>= 8), cout % 64 == 0 (>= 64); the input n cin h w and the taps 36 cin cout below 2 GiB.  x, y, uw, u_save and noise
 * 16-B aligned (noise_nstride % 4 == 0). */
int smc_conv3x3_wino4_supported(int n, int cin, int cout, int h, int w);
int smc_conv3x3_wino4_f32(const float* x, int n, int cin, int h, int w, float* y, int cout, const float* uw,
                          const float* s_in, const smc_conv_epilogue* epi, void* stream);
/* Route report of the last smc_conv3x3_wino4_f32 call of this thread, as smc_conv3x3_wino_last_route: one of the six
 * wino4_kernel<SM,EK> (SM, EK as above; no split-K form), 0 ("none") when the call failed before its launch.  Added
 * under ABI version 6 without a version bump: callers detect these entry points by symbol. */
int smc_conv3x3_wino4_last_route(void);
int smc_conv3x3_wino4_route_count(void);
const char* smc_conv3x3_wino4_route_name(int route);
/* The plan of a smc_conv3x3_wino4_f32 call, as smc_conv3x3_wino_plan: the route it would report (SM by has_style, EK
 * by epi); SMC_ERR_UNSUPPORTED (route 0) where smc_conv3x3_wino4_supported() is 0.  Host only. */
int smc_conv3x3_wino4_plan(int n, int cin, int cout, int h, int w, int has_style, const smc_conv_epilogue* epi,
                           int* route);
/* w [cout][cin][3][3] -> uw [K][9][N][4] floats (36 * cin * cout, 16-B aligned), U = G g G^T (6x6) per (k, n) computed
 * in fp64 and rounded once, element (a, b) at xi = 6 b + a; flip as for smc_wino_weights_f32. */
int smc_wino4_weights_f32(const float* w, int cout, int cin, int flip, float* uw, void* stream);

/* Small-plane Winograd F(2x2, 3x3) with split-K for the IR-SE50 14x14 / 7x7 stages (id_loss/model_irse.py,
 * helpers.py:86-119): the 3x3 stride-1 'same' conv of a 9-tap phase, x [n][cin][h][w] -> y [n][cout][h][w], any
 * smc_conv_epilogue mode applied by the split-K reduction (smc_modconv_epilogue_f32).  uw from smc_wino_taps_f32
 * ([cin][4][cout][4]).  Supported: h, w in [2, 16], cin % 8 == 0 (>= 16), cout % 32 == 0. */
int smc_wino_sp_supported(int n, int cin, int cout, int h, int w);
int64_t smc_wino_sp_workspace_size(int n, int cin, int cout, int h, int w);
int smc_wino_taps_f32(const smc_conv_phase* phase, int cin, int cout, float* uw, void* stream);
int smc_conv3x3_wino_sp_f32(const float* x, int n, int cin, int h, int w, float* y, int cout, const float* uw,
                            const smc_conv_epilogue* epi, float* workspace, int64_t workspace_bytes, void* stream);

/* Apply the modconv epilogue to a raw accumulator tensor, summing `nsplit` partial planes
 * (src + k*split_stride).  src/y/u_save: [n, c, h, w]. */
int smc_modconv_epilogue_f32(const float* src, int nsplit, int64_t split_stride, float* y, int n, int c, int h,
                             int w, const smc_conv_epilogue* epi, void* stream);

/* Fused conv0 epilogue: U = upfirdn2d(T, f, pad=(padx0,pady0 on both sides), gain=fgain) (1:1 FIR),
 * then the modconv epilogue (u_save receives U).  T: [n, c, t_h, t_pitch] of which the first t_w columns
 * are the image (t_pitch = 0: t_w; a pitch that is a multiple of 4 -- the transposed conv's odd 2h + 1
 * width padded -- takes the 16-B load path), may be `nsplit` partial planes; y: [n, c, y_h, y_w].  Only
 * 4x4 filters have the fast kernels; any other size up to 8x8 runs a generic tile kernel, larger ones return
 * SMC_ERR_UNSUPPORTED.  f = NULL (fh = fw = 4): the built-in setup_filter([1,3,3,1]) taps as compile-time constants
 * (bit-identical to passing that filter; the kernel then holds no taps in registers).  epi must not be NULL (pass
 * mode SMC_EPI_STORE for the bare FIR): SMC_ERR_INVALID otherwise. */
int smc_modconv_blur_act_f32(const float* t, int nsplit, int64_t split_stride, float* y, int n, int c, int t_h,
                             int t_w, int t_pitch, int y_h, int y_w, const float* f, int fh, int fw, int padx0,
                             int pady0, float fgain, int flip, const smc_conv_epilogue* epi, void* stream);

/* The whole up=2 modconv layer in one launch: the 4-phase stride-2 transposed 3x3 conv of smc_conv_gemm_f32 (same
 * `phases`, split-bf16 planes wk_x3 required, s_in may be NULL), the 4x4 FIR (pad 1) and the MODACT epilogue of
 * smc_modconv_blur_act_f32, with the raw conv output T = [n, cout, 2h+1, 2w+1] kept on chip.  x: [n, cin, h, w];
 * y, epi->u_save: [n, cout, 2h, 2w]; epi->noise indexes y.  y (and u_save) are bit-identical to the unsplit
 * smc_conv_gemm_f32 (STORE) + smc_modconv_blur_act_f32 pair.  Only the built-in [1,3,3,1] filter at gain 4 (f = NULL,
 * fh = fw = 4, fgain = 4) and only the shapes smc_modconv_up2_supported() accepts (host logic: cin % 16 == 0,
 * cout 32 or 64, input < 2 GiB); anything else returns SMC_ERR_UNSUPPORTED.  `workspace` holds the per-sample
 * weights when s_in is set: the bytes smc_conv_gemm_workspace_size(n, cin, cout, 2h+1, 2w+1, phases, 4) reports
 * suffice.  smc_modconv_up2_plan_ok(): whether the two-launch pair would run that shape as the fused kernel computes
 * it -- without split-K at the planning batch (where it splits, the fused grid under-fills the chip too and the
 * pair is the faster form) and with style-scaled weights (planes of at most 9 cout super-pixels may take a
 * prescaled input instead, which rounds differently): the shapes at which the bit-identity above holds.
 * Route report of the last call of this thread, as for smc_conv_gemm_f32: 0 ("none") when it failed before its
 * launch, else the kernel instantiation (smc_modconv_up2_route_name; NULL outside the range). */
int smc_modconv_up2_supported(int n, int cin, int cout, int h, int w);
int smc_modconv_up2_plan_ok(int n, int cin, int cout, int h, int w);
int smc_modconv_up2_f32(const float* x, int n, int cin, int h, int w, float* y, int cout,
                        const smc_conv_phase* phases, int nphases, const float* s_in, const float* f, int fh, int fw,
                        float fgain, const smc_conv_epilogue* epi, float* workspace, int64_t workspace_bytes,
                        void* stream);
int smc_modconv_up2_last_route(void);
const char* smc_modconv_up2_route_name(int route);

/* A 32-channel synthesis block's conv1 and the ToRGB layer that reads its output, in one launch: the 3x3 Winograd
 * F(2x2) conv of smc_conv3x3_wino_ws_f32 (same x, uw, s_in, epi) whose MODACT epilogue also forms
 *   rgb[n, k, p] = clamp_rgb(sum_c w_rgb[k, c] * s_rgb[n, c] * y[n, c, p] + b_rgb[k])
 * (the expression of smc_torgb_fwd_f32; replaces the same ToRGBLayer.forward call, utils.py:47) from the fp32 y values
 * in its registers.  rgb: [n, cout_rgb, h, w]; w_rgb: [cout_rgb, cout]; s_rgb: [n, cout]; b_rgb: [cout_rgb] or NULL.
 * y: [n, cout, h, w], bit-identical to the unsplit smc_conv3x3_wino_ws_f32 launch of the same style form -- or NULL,
 * and only rgb is written (a block whose output nothing else reads).  The dot product is one FMA chain over the
 * channels in ascending order at every plane size, so a launch is bit-reproducible; on planes above 4096 positions that
 * is smc_torgb_fwd_f32's order and rgb is bit-identical to it (its small-plane kernel sums in another order).
 * smc_modconv_conv1_torgb_supported(): cout == 32, cout_rgb in 1..4, a shape smc_conv3x3_wino_supported() accepts
 * that the two-launch path runs in one pass at the planning batch (no split-K), and -- where epi is not NULL -- the
 * MODACT lrelu epilogue (0 <= alpha <= 1, clamp >= 0) without u_save or residual (epi NULL asks about the shape
 * alone).  Anything else returns SMC_ERR_UNSUPPORTED and the caller keeps the two launches; so does the launch with
 * epi NULL, the STORE default of smc_conv3x3_wino_ws_f32, which has no fused form.
 * `workspace`: smc_modconv_conv1_torgb_workspace_size() bytes (16-B aligned) hold the per-image taps with s_in folded
 * in (the launch then runs the SM = 2 form, as SMC_ROUTE_WINO_FOLD of smc_conv3x3_wino_ws_f32); without it the style
 * scale is applied in the kernel (SM = 1).
 * Route report of the last call of this thread: 0 ("none") when it failed before its launch, else
 * wino_rgb_kernel<TC,SM> by smc_modconv_conv1_torgb_route_name (NULL outside 0 .. route_count() - 1).
 * Added under ABI version 6 without a version bump: callers detect these entry points by symbol. */
int smc_modconv_conv1_torgb_supported(int n, int cin, int cout, int h, int w, int cout_rgb,
                                      const smc_conv_epilogue* epi);
int64_t smc_modconv_conv1_torgb_workspace_size(int n, int cin, int cout, int h, int w);
int smc_modconv_conv1_torgb_f32(const float* x, int n, int cin, int h, int w, float* y, int cout, const float* uw,
                                const float* s_in, const smc_conv_epilogue* epi, const float* w_rgb,
                                const float* s_rgb, const float* b_rgb, float clamp_rgb, int cout_rgb, float* rgb,
                                float* workspace, int64_t workspace_bytes, void* stream);
int smc_modconv_conv1_torgb_last_route(void);
int smc_modconv_conv1_torgb_route_count(void);
const char* smc_modconv_conv1_torgb_route_name(int route);

/* Backward of smc_modconv_blur_act_f32 in one pass: du = bias_act'(g; y re-derived from u) * d[n,o],
 * dt = adjoint FIR of du (pad (pady0, padx0) = (fh-1-p, fw-1-p) of the forward pad p, flip, gain fgain;
 * upfirdn2d.py:245-264 rule), and if dd != NULL: dd[n,o] += sum_hw dz*u.  g/u: [n,c,u_h,u_w],
 * dt: [n,c,t_h,t_pitch] (t_pitch = 0: t_w; columns >= t_w are not written).  dt: any adjoint pad >= 0 (a
 * negative one is SMC_ERR_INVALID).  dd: adjoint pads 0 .. 3 in both axes (below 2, t is smaller than u: dd still sums
 * the whole u plane); dd != NULL with a pad above 3 is SMC_ERR_UNSUPPORTED.  4x4 filters only
 * (SMC_ERR_UNSUPPORTED otherwise); f = NULL: the built-in [1,3,3,1] taps (as smc_modconv_blur_act_f32). */
int smc_modconv_blur_act_bwd_f32(const float* g, const float* u, float* dt, float* dd, int n, int c, int u_h, int u_w,
                                 int t_h, int t_w, int t_pitch, const float* f, int fh, int fw, int padx0, int pady0,
                                 float fgain, int flip, const smc_conv_epilogue* epi, void* workspace,
                                 int64_t workspace_bytes, void* stream);
/* Workspace smc_modconv_blur_act_bwd_f32 needs when dd != NULL (0: none; the per-tile dd partials of planes wider
 * than two FIR tiles, summed per plane in a fixed order -- bit-reproducible dd). */
int64_t smc_modconv_blur_act_bwd_workspace_size(int n, int c, int u_h, int u_w, int t_h, int t_w);

/* Loss-head row reductions, one wave per row in a fixed order: the same row gives the same bits in any batch
 * (PyTorch's row reductions pick their block shape from the row count).  out[r] = sum_k a[r,k] * b[r,k]; ldb = 0
 * broadcasts b's first row.  Replaces the sums / norms of clip_loss.py:28-34, id_loss.py:26-39, model_irse.py:48. */
int smc_row_dot_f32(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int rows, int len,
                    void* stream);

/* The directional CLIP head (clip_loss.py:28-34) per row: f = e - src, u = f / |f|,
 * loss[r] = 1 - cosine_similarity(u, t) (eps as torch's), grad[r] = d loss[r] / d e[r] = (cos uh - th) / |f|
 * ([rows, len], dense).  t: one row (the normalised text direction).  len <= 1024. */
int smc_direction_head_f32(const float* e, int64_t lde, const float* src, int64_t lds, const float* t, float* loss,
                           float* grad, int rows, int len, float eps, void* stream);

/* d[n,o] = rsqrt(sum_i s[n,i]^2 * wsq[o,i] + eps), wsq[o,i] = sum_k W[o,i,k]^2 (demodulation). */
int smc_modconv_demod_f32(const float* s, const float* wsq, float* d, int n, int cin, int cout, float eps,
                          void* stream);

/* Backward of the modconv epilogue: recompute y from u, dz = bias_act grad (CUDA-kernel semantics,
 * bias_act.cu:51-142), du = dz * d[n,o]; if dd != NULL: dd[n,o] += sum_hw dz*u. */
int smc_modconv_act_bwd_f32(const float* g, const float* u, float* du, float* dd, int n, int c, int h, int w,
                            const smc_conv_epilogue* epi, void* workspace, int64_t workspace_bytes, void* stream);
/* Workspace smc_modconv_act_bwd_f32 needs when dd != NULL (0: none; per-workgroup dd partials of planes that span
 * more than two workgroups). */
int64_t smc_modconv_act_bwd_workspace_size(int n, int c, int h, int w);

/* out[r] (+)= sum_p a[r,p]*b[r,p] over rows r < rows of length len; if a_scaled != NULL also
 * a_scaled[r,p] = a[r,p]*scale[r] (scale may be NULL only when a_scaled is NULL). */
int smc_channel_dot_f32(const float* a, const float* b, const float* scale, float* out, float* a_scaled,
                        int64_t rows, int64_t len, int accumulate, void* stream);

/* ds[n,i] += -s[n,i] * sum_o dd[n,o] * d[n,o]^3 * wsq[o,i]   (gradient through the demodulation). */
int smc_modconv_demod_bwd_f32(const float* s, const float* d, const float* dd, const float* wsq, float* ds, int n,
                              int cin, int cout, void* stream);

/* ToRGB (1x1 modulated conv without demodulation + linear bias_act with clamp), replacing the
 * [upstream] ToRGBLayer.forward path (utils.py:47):  y[n,c,p] = clamp(sum_i w[c,i]*s[n,i]*x[n,i,p] + b[c]).
 * w: [cout][cin], s: [n][cin] (already multiplied by the layer's weight_gain), b: [cout] or NULL. */
int smc_torgb_fwd_f32(const float* x, const float* w, const float* s, const float* b, float* y, int n, int cin,
                      int cout, int h, int w_, float clamp, void* stream);

/* dx[n,i,p] (+)= (scale ? s[n,i] : 1) * sum_c w[c,i] * g[n,c,p] * [|y[n,c,p]| < clamp] */
int smc_torgb_bwd_f32(const float* g, const float* y, const float* w, const float* s, float* dx, int n, int cin,
                      int cout, int h, int w_, float clamp, int scale, int accumulate, void* stream);

/* Block-tail backward (the synthesis block output y = conv1's output feeds this block's ToRGB and the next block's
 * conv0): du[n,k,p] = act'(g_next[n,k,p] + (ToRGB^T g_rgb)[n,k,p]; y[n,k,p]) * d[n,k] with conv1's MODACT epilogue
 * `epi` (grad_from_y must be set: y is conv1's output; its d/act/alpha/gain/clamp), ToRGB^T as smc_torgb_bwd_f32
 * with scale = 1 (g_rgb masked by |y_rgb| < clamp_rgb), g_next may be NULL (the last block).  Bit-identical to
 * smc_torgb_bwd_f32 + the sum + smc_modconv_act_bwd_f32 (grad_from_y).  Replaces the autograd sum of the two
 * gradients of [upstream] SynthesisBlock's `x` (utils.py:47 torgb + the next block's conv0). */
int smc_torgb_act_bwd_f32(const float* g_rgb, const float* y_rgb, const float* w, const float* s, float clamp_rgb,
                          const float* g_next, const float* y, float* du, int n, int cin, int cout, int h, int w_,
                          const smc_conv_epilogue* epi, void* stream);

/* Launch report of the memory-bound companion kernels: this thread's last call to smc_modconv_epilogue_f32,
 * smc_modconv_blur_act_f32 / _bwd_f32, smc_modconv_demod_f32 / _bwd_f32, smc_modconv_act_bwd_f32, smc_channel_dot_f32
 * or smc_torgb_fwd_f32 / _bwd_f32 / _act_bwd_f32 (tests, attribution; no launch decision reads it; a dispatcher that
 * calls one of them -- the Winograd split-K reduction -- records here too).  As smc_conv3x3_wino_last_route: 0
 * ("none") when the call failed before its launch, else the kernel instantiation, numbered 1 ..
 * smc_modconv_aux_route_count() - 1 and named as written in its launch (smc_modconv_aux_route_name; NULL outside the
 * range; compare names, never numbers, across builds).  Flags: SMC_ROUTE_DD_PARTIALS when the two-level dd sum ran
 * (per-tile partials in the workspace, then dd_sum_kernel).  smc_modconv_aux_last_nsplit: the grid.z channel split of
 * smc_torgb_act_bwd_f32, 1 for every other entry point. */
#define SMC_ROUTE_DD_PARTIALS 32
int smc_modconv_aux_last_route(void);
int smc_modconv_aux_last_route_flags(void);
int smc_modconv_aux_last_nsplit(void);
int smc_modconv_aux_route_count(void);
const char* smc_modconv_aux_route_name(int route);

/* IDLoss face crop (id_loss.py:20-23): y[p] = adaptive_avg_pool(crop(adaptive_avg_pool(x[p], (pool_h, pool_w)),
 * [crop_y0 : crop_y0+crop_h, crop_x0 : crop_x0+crop_w]), (out_h, out_w)) for `planes` planes; the first pool
 * must be an integer factor (in = pool * k, else SMC_ERR_UNSUPPORTED).  The backward writes the whole input
 * gradient dx [planes][in_h][in_w] (zeros outside the crop). */
int smc_face_crop_f32(const float* x, int64_t planes, int in_h, int in_w, int pool_h, int pool_w, int crop_y0,
                      int crop_x0, int crop_h, int crop_w, int out_h, int out_w, float* y, void* stream);
int smc_face_crop_bwd_f32(const float* dy, int64_t planes, int in_h, int in_w, int pool_h, int pool_w, int crop_y0,
                          int crop_x0, int crop_h, int crop_w, int out_h, int out_w, float* dx, void* stream);

/* CLIP input preprocessing (find_direction.py:49-52): y = (bicubic(clamp(img*127.5+128, 0, 255), out) / 255
 * - mean[c]) / std[c], bicubic = F.interpolate(mode='bicubic', align_corners=False) (A = -0.75).  img
 * [n][channels][in_h][in_w] -> y [n][channels][out_h][out_w]; mean/std: `channels` floats on the device.
 * The backward writes the whole image gradient dimg (downsampling, in >= out, only). */
int smc_clip_unprocess_f32(const float* img, int n, int channels, int in_h, int in_w, int out_h, int out_w,
                           const float* mean, const float* std_, float* y, void* stream);
int smc_clip_unprocess_bwd_f32(const float* img, const float* dy, int n, int channels, int in_h, int in_w, int out_h,
                               int out_w, const float* mean, const float* std_, float* dimg, void* stream);
/* StyleGAN-NADA CLIP preprocessing (clip_loss_nada.py:72-75 `preprocess`, applied at :109-111 and :225):
 * torchvision Normalize(mean=-1, std=2) -> Resize(out, BICUBIC) -> CenterCrop(out) -> Normalize(CLIP mean, std),
 * no clamp: y = (bicubic((img + 1) / 2, out) - mean[c]) / std[c].  Same shapes / backward contract as
 * smc_clip_unprocess_f32 (square input, so the crop is the identity). */
int smc_clip_preprocess_nada_f32(const float* img, int n, int channels, int in_h, int in_w, int out_h, int out_w,
                                 const float* mean, const float* std_, float* y, void* stream);
int smc_clip_preprocess_nada_bwd_f32(const float* img, const float* dy, int n, int channels, int in_h, int in_w,
                                     int out_h, int out_w, const float* mean, const float* std_, float* dimg,
                                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * CLIP ViT image tower (replaces the third-party openai/CLIP VisionTransformer that the reference
 * calls through CLIPLoss.encode_image, clip_loss.py:21,25-26; weights frozen -> data gradient only).
 *
 * smc_linear_f32: C[M][N] = epi(A[M][K] . B[K][N]) on fp32 MFMA (row-major, leading dimensions in
 * floats; K % 32 == 0, N % 4 == 0, A and B 16-B aligned).  B is the frozen weight stored K-major
 * (nn.Linear weight^T for a forward product, the weight itself for its data gradient).
 * Epilogue order: + bias[n]; * act'(dact_pre[m][n]); pre_save = v, v = act(v); + residual[m][n]
 * (residual may alias C).  Workspace: smc_linear_workspace_size() bytes (split-K partial tiles).
 */
#define SMC_LIN_ACT_NONE 0
#define SMC_LIN_ACT_QUICKGELU 1 /* x * sigmoid(1.702 x), CLIP's QuickGELU */

typedef struct {
    const float* bias;      /* [N] or NULL                                                    */
    const float* dact_pre;  /* multiply by QuickGELU'(dact_pre[m*ld_dact+n]) or NULL           */
    int ld_dact;
    int act;                /* SMC_LIN_ACT_*                                                   */
    float* pre_save;        /* pre-activation store when act != NONE, may be NULL              */
    int ld_pre;
    const float* residual;  /* added last, may be NULL or alias C                              */
    int ld_res;
} smc_linear_epilogue;

int64_t smc_linear_workspace_size(int M, int N, int K);
int smc_linear_f32(const float* a, int lda, const float* b, int ldb, float* c, int ldc, int M, int N, int K,
                   const smc_linear_epilogue* epi, float* workspace, int64_t workspace_bytes, void* stream);

/* smc_linear_ex_f32: smc_linear_f32 with the three optional operands the tower's executor hands the same launch
 * (tests, attribution), each NULL or:
 *   bt       the same B transposed, [N][K] row-major with row pitch K, 16-B aligned: N % 64 == 0 && K % 64 == 0 shapes
 *            stage the B tile k-fastest (lin_gemm2_kernel<true>);
 *   planes   the split-bf16 planes of the same [K][N] (smc_linear_x3_planes, 16-B aligned): those shapes run the fp32
 *            products as three-term bf16 splits (lin_gemm2_x3_kernel; planes take precedence over bt);
 *   counters smc_linear_counter_ints(M, N) zeroed ints: a split-K call sums its partial tiles in the GEMM launch itself
 *            (the workgroup that finishes a tile last; the counters are left non-zero), NULL: in a second kernel.
 * Other shapes ignore bt and planes (the 32 x 128 exact-fp32 kernel). */
int64_t smc_linear_counter_ints(int M, int N);
int smc_linear_ex_f32(const float* a, int lda, const float* b, int ldb, float* c, int ldc, int M, int N, int K,
                      const smc_linear_epilogue* epi, float* workspace, int64_t workspace_bytes, const float* bt,
                      const void* planes, int* counters, void* stream);
/* Split-bf16 planes of a row-major [K][N] fp32 matrix (ldb floats per row; K % 32 == 0): b = t0 + t1 + t2 exactly,
 * each term the top 16 bits of what the terms before it leave (truncation); term s of b[k][n] is the bf16 at element
 * ((((k / 32) * 3 + s) * 4 + (k % 32) / 8) * N + n) * 8 + k % 8.  smc_linear_x3_planes_bytes: the buffer's size. */
int64_t smc_linear_x3_planes_bytes(int K, int N);
int smc_linear_x3_planes(const float* b, int ldb, int K, int N, void* planes, void* stream);

/* Route report of this thread's last GEMM launch through smc_linear_f32, smc_linear_ex_f32 or the tower's executor
 * (smc_vit_forward_f32 / smc_vit_backward_f32: their last projection); written at the launch site, no launch
 * decision reads it.  Route: 0 ("none") when the call failed before its launch, otherwise the kernel, 1 ..
 * smc_linear_route_count() - 1, named by smc_linear_route_name (NULL outside the range).  nsplit: the split-K factor
 * of that launch (0 with route 0).  reduce: how its partial tiles were summed, */
#define SMC_LIN_REDUCE_NONE 0     /* nsplit == 1: a single pass                 */
#define SMC_LIN_REDUCE_KERNEL 1   /* the separate reduction kernel              */
#define SMC_LIN_REDUCE_INLAUNCH 2 /* the in-launch hand-off (counters given)    */
int smc_linear_last_route(void);
int smc_linear_last_nsplit(void);
int smc_linear_last_reduce(void);
int smc_linear_route_count(void);
const char* smc_linear_route_name(int route);

/* LayerNorm over the last dim (nn.LayerNorm: biased variance, y = (x-mean)*rstd*w + b), one row per
 * wave; dim % 64 == 0, dim <= 1024.  mean/rstd [rows] may be NULL.  Row strides in floats. */
int smc_layernorm_fwd_f32(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t ldy,
                          float* mean, float* rstd, int rows, int dim, float eps, void* stream);
/* dx = LN'(dy) (+ dres if not NULL); dx may alias dres. */
int smc_layernorm_bwd_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* mean,
                          const float* rstd, const float* w, const float* dres, int64_t ldres, float* dx,
                          int64_t lddx, int rows, int dim, void* stream);

/* Multi-head softmax attention over qkv [batch*tokens][3*heads*64] (q | k | v, nn.MultiheadAttention
 * in_proj order) -> out [batch*tokens][heads*64]; p_save [batch][heads][tokens][tokens] may be NULL.
 * head_dim must be 64.  The backward writes dqkv [batch*tokens][3*heads*64] and needs qkv and dout 16-byte
 * aligned. */
int smc_attention_fwd_f32(const float* qkv, float* out, float* p_save, int batch, int tokens, int heads,
                          int head_dim, float scale, void* stream);
int smc_attention_bwd_f32(const float* dout, const float* qkv, const float* p_save, float* dqkv, int batch,
                          int tokens, int heads, int head_dim, float scale, void* stream);
/* The same forward with the causal mask of CLIP's text transformer (openai/CLIP model.py
 * build_attention_mask: -inf above the diagonal), used once per prompt by the CLIPLoss text side
 * (clip_loss.py:15-18 encode_text).  Forward only. */
int smc_attention_causal_fwd_f32(const float* qkv, float* out, int batch, int tokens, int heads, int head_dim,
                                 float scale, void* stream);

/* Non-overlapping patch extraction (conv kernel == stride): img [batch][channels][grid*patch]^2 <->
 * patches [batch*grid*grid][channels*patch*patch]; inverse = 1 writes img from patches. */
int smc_patch_im2col_f32(const float* img, float* patches, int batch, int channels, int grid, int patch,
                         int inverse, void* stream);

typedef struct {
    int width, layers, heads, patch, grid, out_dim, in_ch; /* ViT-B/32: 768, 12, 12, 32, 7, 512, 3 */
    float ln_eps;                                          /* 1e-5 (nn.LayerNorm default)          */
    int products;  /* 0: exact-fp32 MFMA; 1: split-bf16 (three bf16 terms per fp32 operand, the six products above
                      2^-23 |a b|; the packed buffer then ends with every projection's planes, smc_vit_pack_x3) */
} smc_vit_config;

/* Packed frozen weights: one fp32 buffer, segments in this order, each padded to 64 floats:
 *   conv_wt [C*p*p][D], conv_w [D][C*p*p], class_embedding [D], positional_embedding [L][D],
 *   ln_pre.{w,b} [D],
 *   per layer: ln_1.{w,b}, in_proj_weight^T [D][3D], in_proj_weight [3D][D], in_proj_bias [3D],
 *              out_proj.weight^T [D][D], out_proj.weight [D][D], out_proj.bias [D], ln_2.{w,b},
 *              c_fc.weight^T [D][4D], c_fc.weight [4D][D], c_fc.bias [4D],
 *              c_proj.weight^T [4D][D], c_proj.weight [D][4D], c_proj.bias [D],
 *   ln_post.{w,b} [D], proj [D][E], proj^T [E][D]
 * (the segment sizes of one layer are padded individually; see stylemc_amd/vit_hip.py). */
int64_t smc_vit_packed_floats(const smc_vit_config* cfg);
/* Activations the backward needs, per batch size (floats). */
int64_t smc_vit_saved_floats(const smc_vit_config* cfg, int batch);
/* products = 1: fill the planes region at the end of `packed` from its fp32 segments (after they are written). */
int smc_vit_pack_x3(const smc_vit_config* cfg, float* packed, void* stream);
int64_t smc_vit_workspace_bytes(const smc_vit_config* cfg, int batch);
/* image [batch][in_ch][grid*patch][grid*patch] -> out [batch][out_dim]; saved may be NULL (no backward). */
int smc_vit_forward_f32(const smc_vit_config* cfg, const float* packed, const float* image, int batch, float* out,
                        float* saved, float* workspace, int64_t workspace_bytes, void* stream);
/* dimage = d out / d image applied to dout, from the forward's saved activations (laid out for `batch`
 * images); only the leading batch_run <= batch images are differentiated: dout [batch_run][out_dim],
 * dimage [batch_run][in_ch][..][..] (the original-image half of a batched pair needs no gradient). */
int smc_vit_backward_f32(const smc_vit_config* cfg, const float* packed, const float* dout, int batch, int batch_run,
                         const float* saved, float* dimage, float* workspace, int64_t workspace_bytes,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * ArcFace IR-SE50 (id_loss/model_irse.py:10-49, helpers.py:56-119; run by IDLoss.extract_feats,
 * id_loss/id_loss.py:20-24): forward and input gradient (frozen, eval-mode weights).
 * The caller describes the network once (packed conv phases as for smc_conv_gemm_f32, eval-mode
 * BatchNorms as per-channel scale a / shift b); see stylemc_amd/irse_hip.py for the packing.
 */
typedef struct {
    int cin, depth, stride, in_h, in_w;  /* unit input [n][cin][in_h][in_w] -> [n][depth][in_h/s][in_w/s]   */
    const float* bn1_a;                  /* [cin] res_layer BatchNorm2d (before conv1) as x*a + b              */
    const float* bn1_b;
    smc_conv_phase c1_fwd;               /* 3x3 stride 1, cin -> depth                                         */
    smc_conv_phase c1_bwd;               /* its adjoint depth -> cin, bn1_a folded into the weights            */
    const float* prelu;                  /* [depth]                                                            */
    smc_conv_phase c2_fwd;               /* 3x3 stride s, depth -> depth                                       */
    smc_conv_phase c2_bwd[4];            /* its adjoint (4 polyphase phases when s == 2), bn2_a folded         */
    int c2_bwd_nphases;
    const float* bn2_a;                  /* [depth]                                                            */
    const float* bn2_b;
    const float* se_w1;                  /* SE fc1 [hidden][depth]                                             */
    const float* se_w2;                  /* SE fc2 [depth][hidden]                                             */
    int se_hidden;
    int sc_conv;                         /* shortcut: 0 = MaxPool2d(1, s) (cin == depth), 1 = conv1x1(s) + BN  */
    smc_conv_phase sc_fwd;               /* 1 tap, in_stride s                                                 */
    smc_conv_phase sc_bwd;               /* adjoint on the compact grid, sc_a folded                          */
    const float* sc_a;
    const float* sc_b;
} smc_irse_unit;

typedef struct {
    int n_units;
    const smc_irse_unit* units;
    int in_h, in_w;                      /* 112 x 112                                                          */
    int img_ch;                          /* 3                                                                  */
    int stem_cin;                        /* img_ch padded to a multiple of 16 (zero channels / weights)        */
    int stem_cout;                       /* 64                                                                 */
    smc_conv_phase stem_fwd;             /* input_layer conv3x3                                                */
    smc_conv_phase stem_bwd;             /* its adjoint, stem_bn_a folded                                      */
    const float* stem_bn_a;
    const float* stem_bn_b;
    const float* stem_prelu;
    int feat;                            /* 512                                                                */
    int flat;                            /* 512*7*7                                                            */
    const float* fc_wt;                  /* [flat][feat]: output BatchNorm2d + Linear + BatchNorm1d folded     */
    const float* fc_w;                   /* [feat][flat] (data gradient)                                       */
    const float* fc_b;                   /* [feat]                                                             */
} smc_irse_net;

int64_t smc_irse_saved_floats(const smc_irse_net* net, int n);
int64_t smc_irse_workspace_bytes(const smc_irse_net* net, int n);
/* img [n][img_ch][in_h][in_w] -> feat [n][feat] (before the l2 normalisation); saved may be NULL. */
int smc_irse_forward_f32(const smc_irse_net* net, const float* img, int n, float* feat, float* saved,
                         float* workspace, int64_t workspace_bytes, void* stream);
/* input gradient of the leading n <= n_saved faces of a forward that ran (and saved) n_saved faces:
 * dfeat [n][feat] -> dimg [n][img_ch][in_h][in_w]. */
int smc_irse_backward_f32(const smc_irse_net* net, const float* dfeat, int n_saved, int n, const float* saved,
                          float* dimg, float* workspace, int64_t workspace_bytes, void* stream);

/* The squeeze-and-excite stage of one unit on its own: exactly the two launches each that smc_irse_forward_f32 /
 * smc_irse_backward_f32 make per unit (the same host code), for tests at shapes the network never reaches.  Added
 * under ABI version 6 without a version bump.  Limits, checked on the host before any launch (SMC_ERR_INVALID): n >= 1,
 * C % 16 == 0, C <= 512, 1 <= hid <= 256, stride 1 or 2, in_h and in_w >= stride and divisible by it, n*C*oh*ow below
 * 2^31, no NULL pointer but where one is allowed below.
 *
 * Forward, oh = in_h / stride, ow = in_w / stride:
 *   m[n][C] = mean_hw r;  h[n][hid] = relu(w1 m);  g[n][C] = sigmoid(w2 h);  out = r * g[.., None, None] + shortcut;
 *   xbn = out * a[c] + b[c]
 *   r, out, xbn [n][C][oh][ow];  w1 [hid][C];  w2 [C][hid];  a, b [C].
 *   shortcut: exactly one of sc [n][C][oh][ow] (the conv shortcut's output) and x [n][C][in_h][in_w] (the unit's input,
 *   read at [stride*y][stride*x]: MaxPool2d(1, stride)) is non-NULL.  xbn, a and b are all NULL or all given. */
int smc_irse_se_fwd_f32(const float* r, const float* sc, const float* x, int stride, int in_h, int in_w, int n, int C,
                        const float* w1, const float* w2, int hid, const float* a, const float* b, float* out,
                        float* xbn, float* h, float* g, float* m, void* stream);
/* Backward of the same stage for dout [n][C][oh][ow], from the forward's r, g and h:
 *   dg[n][C] = sum_hw dout * r;  dz = dg g (1 - g);  dh = (h > 0) w2^T dz;  dm = w1^T dh / (oh ow);
 *   dr = dout * g[.., None, None] + dm[.., None, None]       dg [n][C], dr [n][C][oh][ow]. */
int smc_irse_se_bwd_f32(const float* dout, const float* r, const float* g, const float* h, const float* w1,
                        const float* w2, int n, int C, int hid, int oh, int ow, float* dg, float* dr, void* stream);

/* ---------------------------------------------------------------------------------------------
 * e4e / pSp encoder (encoder4editing/models/encoders/psp_encoders.py:58-200, helpers.py:123-140): the IR-SE50 trunk
 * with feature taps, the FPN's upsample-add and the grouped stride-2 convolution of the 18 map2style heads.
 * Inference only, fp32.  Added under ABI version 6 without a version bump: callers detect these entry points by symbol.
 *
 * smc_irse_trunk_f32 runs the stem and the units of a net exactly as smc_irse_forward_f32 does (nothing saved), without
 * the output layer: feat, flat and the fc_* fields are not read and may be 0 / NULL (the adjoint phases are still
 * sized for the workspace and must be described).  The outputs of the units tap_units[0 .. ntaps) (1 <= ntaps <= 3,
 * ascending, host array) are written to the caller's buffers tap_out[t] (host array of device pointers), each
 * [n][depth][in_h/s][in_w/s] of that unit.  e4e taps units 6, 20 and 23 (psp_encoders.py:177-184).
 */
int64_t smc_irse_trunk_workspace_bytes(const smc_irse_net* net, int n);
int smc_irse_trunk_f32(const smc_irse_net* net, const float* img, int n, const int* tap_units, float* const* tap_out,
                       int ntaps, float* workspace, int64_t workspace_bytes, void* stream);

/* y = bilinear(x -> out_h x out_w, align_corners = True) + lat  (helpers.py:123-140 _upsample_add):
 * x [planes][in_h][in_w], lat and y [planes][out_h][out_w]; any sizes >= 1, every tensor below 2 GiB. */
int smc_upsample_add_f32(const float* x, int64_t planes, int in_h, int in_w, const float* lat, float* y, int out_h,
                         int out_w, void* stream);

/* `groups` independent 3x3 stride-2 pad-1 convolutions in one launch (GradualStyleBlock, psp_encoders.py:41-47):
 *   y[g][s][o][a][b] = lrelu(bias[g][o] + sum_{t < ntaps, i < cin} wk[g][t][i][o] * x_g[s][i][2a - 1 + ky_t][2b - 1 + kx_t],
 *                            alpha)
 * with out = (in - 1) / 2 + 1 for any h, w >= 1 (odd, non-square and 1 x 1 planes included), reads outside the plane 0,
 * lrelu(z, alpha) = z > 0 ? z : alpha z (alpha 0.01: nn.LeakyReLU(); alpha 1: linear).
 *   x_g[s] = x + g * x_group_stride + s * x_sample_stride (floats), a contiguous [cin][h][w] block: group stride 0 lets
 *     every group read the same feature map, and strides of a wider tensor select channel slices of it.
 *   taps: host array of the ntaps (1..9) taps summed, each ky*3 + kx, ascending; wk [groups][ntaps][cin][cout] holds
 *     only those.  The caller drops the taps that can only touch padding at this plane size (2x2 -> 1x1 keeps 4,
 *     1x1 -> 1x1 keeps the centre: with alpha = 1 that is a grouped Linear, the heads' EqualLinear).
 *   bias [groups][cout], may be NULL.  y [groups][n][cout][oh][ow].
 * Per group a GEMM on the exact-fp32 MFMA (M = n*oh*ow, N = cout, K = ntaps*cin).  Where tiles x groups cannot fill
 * the chip, K is split across workgroups into partial planes in `workspace` (smc_conv_s2_grouped_workspace_size()
 * bytes, 0: no split; -1: unsupported shape) that a second kernel sums in split order: no atomics, bit-identical from
 * run to run.  Limits (smc_conv_s2_grouped_supported(); otherwise SMC_ERR_INVALID from host-side validation, before
 * any launch): 1 <= groups <= 65535, cin % 16 == 0, cout % 32 == 0, groups*n*cin*h*w, groups*n*cout*oh*ow and
 * groups*9*cin*cout floats each below 2 GiB, the strided input span below 2 GiB, wk 16-byte aligned. */
int smc_conv_s2_grouped_supported(int groups, int n, int cin, int cout, int h, int w);
int64_t smc_conv_s2_grouped_workspace_size(int groups, int n, int cin, int cout, int h, int w, int ntaps);
int smc_conv_s2_grouped_f32(const float* x, int64_t x_sample_stride, int64_t x_group_stride, int groups, int n, int cin,
                            int h, int w, const float* wk, const int* taps, int ntaps, const float* bias, float alpha,
                            float* y, int cout, float* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Face landmarks (MTCNN detector, MobileNet-GDConv regressor): depthwise convolution, ceil-mode max-pool and the
 * crop + bilinear resize + normalise of a face box.  Inference only, fp32, no atomics and a fixed summation order
 * (bit-identical from run to run), 64-bit plane offsets.  Added under ABI version 6 without a version bump: callers
 * detect these entry points by symbol.  Every limit below is checked on the host before any launch (SMC_ERR_INVALID).
 *
 * smc_dwconv_f32:  y[n][c] = act(scale_c[c] * (w[c] * x[n][c]) + shift_c[c])   (cross-correlation, as nn.Conv2d with
 * groups = channels; eval-mode BatchNorm folded into scale_c / shift_c, either may be NULL = 1 / 0).
 *   x [n][c][in_h][in_w], w [c][k][k], y [n][c][oh][ow].  Two forms:
 *     k = 3, pad = 1, stride 1 or 2: any plane >= 1 x 1, out = (in + 2 - 3) / stride + 1;
 *     pad = 0, stride 1, k == in_h == in_w, 2 <= k <= 8 (the "global" depthwise layer of MobileNet_GDConv): out 1 x 1.
 *   n * c <= 2^31 - 1, sides <= 32768.  16-byte loads and stores are used where x and y are 16-byte aligned and in_w is
 *   a multiple of 4 * stride; the results do not depend on that. */
#define SMC_DW_ACT_LINEAR 0
#define SMC_DW_ACT_RELU6 1 /* min(max(z, 0), 6) */
int smc_dwconv_supported(int n, int c, int in_h, int in_w, int k, int stride, int pad);
int smc_dwconv_f32(const float* x, int n, int c, int in_h, int in_w, const float* w, int k, int stride, int pad,
                   const float* scale_c, const float* shift_c, int act, float* y, void* stream);

/* nn.MaxPool2d(k, stride, ceil_mode = True), pad 0, for (k, stride) = (2, 2) or (3, 2) (MTCNN/get_nets.py):
 * x [planes][in_h][in_w] -> y [planes][oh][ow], out = ceil((in - k) / stride) + 1, the last window clipped at the
 * border; in_h, in_w >= k.  NaN propagates as in torch. */
int smc_maxpool2d_f32(const float* x, int64_t planes, int in_h, int in_w, int k, int stride, float* y, void* stream);

/* One face crop per image, from a generator image to the regressor's input, in one launch:
 *   v   = denorm ? clamp(img * 127.5 + 128, 0, 255) : img            (denorm_img, float: no uint8 step)
 *   r   = bilinear(v[:, y1:y2, x1:x2] -> out_size x out_size)        (align_corners = False, no antialias; the source
 *                                                                     coordinate as torch computes it in fp32)
 *   out = (r / 255 - mean[c]) / std[c],  or r itself where mean3 and std3 are both NULL (crop_face's own output)
 * img [n][3][in_h][in_w], boxes [n][4] int32 ON THE DEVICE as (x1, y1, x2, y2) with exclusive ends, out
 * [n][3][out_size][out_size]; mean3 / std3: HOST arrays of 3 floats (std != 0), both or neither.  A box is clipped to
 * the image by the kernel (at least one pixel is kept), so no box can make it read outside the planes. */
int smc_crop_bilinear_norm_f32(const float* img, int n, int in_h, int in_w, const int* boxes, int out_size, int denorm,
                               const float* mean3, const float* std3, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STYLEMC_HIP_H */
