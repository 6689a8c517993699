/*
 * hyres_hip.h — C-ABI of libhyres_hip.so, the MI355X (gfx950) kernels behind HyRES's
 * residual-codec hot path.  Plain pointers and sizes only: every tensor argument is a device
 * pointer to fp32 data laid out NHWC ([B][H][W][ld] with the channel slice starting at the
 * pointer), every entry point takes the caller's HIP stream as an opaque handle and returns
 * 0 on success or a nonzero HYRES_E_* / hipError_t code (message: hyres_last_error_string()).
 * The library never allocates, frees or synchronises: scratch is caller-supplied (query with the
 * *_workspace_bytes functions), so every call is stream-ordered and hipGraph-capturable.
 *
 * The reference has no native operator API — its "operator interface" is nn.Module.forward +
 * autograd.  Each entry point below names the reference code it replaces
 * (paths relative to the reference repo root).
 */
#ifndef HYRES_HIP_H
#define HYRES_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hyres_stream_t; /* hipStream_t */

#define HYRES_OK 0
#define HYRES_E_SHAPE 1001     /* inconsistent or unsupported shape / stride */
#define HYRES_E_ALIGN 1002     /* pointer or leading dimension not 16-byte aligned where needed */
#define HYRES_E_ARG 1003       /* invalid enum / NULL pointer */
#define HYRES_E_WORKSPACE 1004 /* workspace too small */

#define HYRES_MAX_TAPS 49

/* ------------------------------------------------------------------------------------------ */
/* library                                                                                    */
/* ------------------------------------------------------------------------------------------ */
int hyres_version(void);
const char* hyres_last_error_string(void);


/* ------------------------------------------------------------------------------------------ */
/* convolution geometry (implicit GEMM, NHWC).                                                */
/* One launch computes Y[b, i*osh+oph[p], j*osw+opw[p], co] for every phase p < nphase and base */
/* pixel (i,j) < (Hq,Wq):  bias[co] + sum over taps t of phase p and ci < Ci of                 */
/*   X[b, i*ish + dh[t], j*isw + dw[t], ci] * W2[co*ldw + t*Ci + ci]   (zero outside X).        */
/* Phases express ConvTranspose2d / strided-conv input-gradients as sub-pixel convolutions.    */
/* ------------------------------------------------------------------------------------------ */
typedef struct hyres_conv_geom {
    int B, Hi, Wi, Ci, ldx;   /* input: NHWC, pixel stride ldx floats */
    int Ho, Wo, Co, ldy;      /* output tensor dims, pixel stride ldy floats */
    int nphase, Hq, Wq;       /* base grid per phase */
    int osh, osw, ish, isw;   /* output / input stride of the base grid */
    int oph[4], opw[4];       /* output offset of each phase */
    int ntap[4], tap0[4];     /* taps of each phase: global tap indices tap0[p] .. tap0[p]+ntap[p]-1 */
    int ntaps;                /* total taps (rows of W2 = ntaps*Ci per output channel) */
    int dh[HYRES_MAX_TAPS], dw[HYRES_MAX_TAPS];
    int kh[HYRES_MAX_TAPS], kw[HYRES_MAX_TAPS]; /* kernel element each tap reads (weight re-layout) */
} hyres_conv_geom;

/* Keep only the taps whose kernel element (kh, kw) has keep[kh*KW + kw] != 0 (order preserved).
 * CheckboardMaskedConv2d's forward/dgrad run on its 12 live taps of 25. */
int hyres_geom_filter_taps(hyres_conv_geom* g, const unsigned char* keep, int KW);

/* nn.Conv2d(k, stride, pad, dil) forward (models/layers/common.py:4-11, compressai conv()). */
int hyres_geom_conv2d(hyres_conv_geom* g, int B, int H, int W, int Ci, int ldx, int Co, int ldy,
                      int KH, int KW, int stride, int pad, int dil);
/* input-gradient of that Conv2d: a conv over dY (stride 1) or a 4-phase sub-pixel conv (stride 2).
 * (B,H,W,Ci,Co,...) describe the ORIGINAL conv; ld_dx / ld_dy are the gradients' pixel strides. */
int hyres_geom_conv2d_dgrad(hyres_conv_geom* g, int B, int H, int W, int Ci, int ld_dx, int Co,
                            int ld_dy, int KH, int KW, int stride, int pad, int dil);
/* nn.ConvTranspose2d(k, s=2, p, output_padding=1) forward (compressai deconv()) as 4 phases. */
int hyres_geom_deconv2d(hyres_conv_geom* g, int B, int H, int W, int Ci, int ldx, int Co, int ldy,
                        int K, int pad);
/* input-gradient of that ConvTranspose2d: a stride-2 conv over dY. */
int hyres_geom_deconv2d_dgrad(hyres_conv_geom* g, int B, int H, int W, int Ci, int ld_dx, int Co,
                              int ld_dy, int K, int pad);

/* Weight re-layout for a geometry built by the helpers above.  ``w`` is the PyTorch parameter
 * (Conv2d: [Co][Ci][KH][KW]; ConvTranspose2d: [Ci][Co][K][K]); ``w2`` gets [rows][ntaps*cols] in
 * the geometry's tap order.  ``mask`` (same shape as w, or NULL) multiplies w on the fly
 * (CheckboardMaskedConv2d, models/layers/checkerboard.py:46-47). (Ci, Co) are the ORIGINAL layer's. */
#define HYRES_WPREP_CONV 0        /* Conv2d forward:  rows = Co, cols = Ci */
#define HYRES_WPREP_CONV_DGRAD 1  /* Conv2d dgrad:    rows = Ci, cols = Co, taps flipped as geom */
#define HYRES_WPREP_DECONV 2      /* ConvT forward:   rows = Co, cols = Ci, phase tap order */
#define HYRES_WPREP_DECONV_DGRAD 3/* ConvT dgrad:     rows = Ci(in), cols = Co(out) */
int hyres_conv_weight_prep(const hyres_conv_geom* g, const float* w, float* w2, int mode, int Ci,
                           int Co, int KH, int KW, int pad, const float* mask, hyres_stream_t s);
/* Batched re-layout: every conv weight of a model in ONE launch per optimiser step.
 * hyres_prep_desc_fill writes one descriptor (hyres_prep_desc_bytes() bytes, host memory) for the same
 * arguments as hyres_conv_weight_prep, covering output elements [begin, begin + rows*ntaps*cols);
 * hyres_conv_weight_prep_batch runs n device-resident descriptors (sorted by begin, total elements). */
long long hyres_prep_desc_bytes(void);
int hyres_prep_desc_fill(void* desc, const hyres_conv_geom* g, const float* w, float* w2, int mode, int Ci, int Co,
                         int KH, int KW, long long begin, long long* count);
int hyres_conv_weight_prep_batch(const void* descs, int n, long long total, hyres_stream_t s);

/* epilogue of the convolution GEMM */
#define HYRES_EPI_BIAS 0      /* y = act(acc + bias + res) */
#define HYRES_EPI_GDN 1       /* n = acc + bias(beta');  y = aux0 * rsqrt(n); out2 = n   (GDN)  */
#define HYRES_EPI_IGDN 2      /* n = acc + bias(beta');  y = aux0 * sqrt(n);  out2 = n   (IGDN) */
#define HYRES_EPI_GDN_BWD 3   /* y = 2*aux0*acc + aux1 * rsqrt(aux2)                              */
#define HYRES_EPI_IGDN_BWD 4  /* y = 2*aux0*acc + aux1 * sqrt(aux2)                               */
#define HYRES_EPI_ROWSCALE 5  /* y = act(aux1[pix * ld1] * acc + bias (+ res)): a per-output-pixel scale of the
                               * input folded into the GEMM (SpatialAttention's x * attn ahead of MultiScaleRefine's
                               * fusion 1x1, enhancement.py:105-109)                                          */
#define HYRES_EPI_SA_BWD 6    /* y = acc + aux0[pix * ld0] + (n == ((const int*)aux2)[pix] ? aux0[pix * ld0 + 1] : 0):
                               * SpatialAttention's channel-mean / channel-max backward (enhancement.py:14-20)
                               * folded into the input-gradient of MultiScaleRefine's fusion 1x1 (training with
                               * the ROWSCALE forward): aux0 = [P][2] (d mean / C, d max), aux2 = argmax [P]  */
#define HYRES_ACT_NONE 0
#define HYRES_ACT_RELU 1
#define HYRES_ACT_PRELU 2     /* single shared slope (nn.PReLU()), read from device pointer */
#define HYRES_ACT_RELU_MASK 3 /* ReLU backward fused into an input-gradient: y = (aux0 > 0) ? y : 0,
                                 aux0 = the ReLU output of the layer whose gradient is produced */
#define HYRES_ACT_PRELU_MASK 4 /* PReLU backward fused into an input-gradient (round 6; the 3x3 Ci = Co = 64 layers on
                                * conv3x3_wres_bf6_kernel only, HYRES_E_ARG elsewhere): y = (aux0 > 0) ? v : slope[0] * v,
                                * aux0 = the saved pre-activation (fp32, pitch ld0), and the slope gradient
                                * sum_{aux0 <= 0} aux0 * v is ADDED to ((float*)aux1)[0] — per-block partials in aux2
                                * (capacity ld2 floats >= HYRES_PRELU_PARTIALS), summed in a fixed order by a second
                                * kernel of the same call (deterministic). kind BIAS, accumulate 0, fp32 IO.
                                * Replaces prelu_bwd of MultiScaleRefine's scale blocks (enhancement.py:44-51,
                                * 89-95): the dilation-2 conv's input-gradient writes the PReLU'd gradient directly.
                                * With kind HYRES_EPI_SA_BWD (round 6, the streaming 64 -> 192 input-gradients only):
                                * output channels [0, 64) get the PReLU backward — aux1 = their pre-activation (Y's
                                * dtype, pitch ld1), slope gradient ADDED to ((float*)res)[0], partials in out2
                                * (ldo2 >= HYRES_PRELU_PARTIALS); no accumulate. Replaces MultiScaleRefine scale 1's
                                * prelu_bwd (its PReLU output is multi[..., 0:64], enhancement.py:113-115) */
#define HYRES_PRELU_PARTIALS 2048

#define HYRES_IO_X16 1   /* hyres_epilogue.io_f16 bits; X16 / Y16 also hyres_add2d's io */
#define HYRES_IO_Y16 2
#define HYRES_IO_AUX16 4
typedef struct hyres_epilogue {
    int kind, act, accumulate;    /* accumulate: y += result (gradient accumulation) */
    int square_input;             /* GEMM A-operand prologue x -> x*x (GDN norm) */
    const float* bias;            /* [Co] or NULL */
    const float* res; int ldres;  /* added before act, or NULL */
    const float* slope;           /* PReLU slope (device, 1 float) */
    const float* aux0; int ld0;
    const float* aux1; int ld1;
    const float* aux2; int ld2;
    float* out2; int ldo2;
    int f16_operands;             /* 1: X and W2 rounded to fp16 in the LDS staging, v_mfma_f32_32x32x16_f16
                                   * with fp32 accumulation and fp32 epilogue (autocast-fp16 inference,
                                   * BASELINE configs[4]); ignored on the small-Ci and narrow paths */
    int io_f16;                   /* fp16 activations in HBM (autocast, configs[4] and AMP training): bit 0 =
                                   * X is fp16, bit 1 = Y and the epilogue's activation operands (res, aux0,
                                   * out2) are fp16 (bias/slope stay fp32); bits 0/1: no accumulate, no
                                   * GDN-backward kinds. X-fp16 needs Ci % 32 == 0 (or the narrow Co <= 4
                                   * kernel, whose Y stays fp32). Bit 2 (HYRES_IO_AUX16, backward convs with
                                   * fp32 X/Y): the saved activations the epilogue reads — aux0 (the ReLU
                                   * mask's y, GDN-backward's x) and aux2 (GDN-backward's norm) — are fp16. */
} hyres_epilogue;

/* Y = conv(X, W2) with the epilogue — nn.Conv2d / nn.ConvTranspose2d / GDN forward and their
 * input-gradients (replaces torch's cuDNN/MIOpen conv dispatch at every conv call site on the hot
 * path: models/checkerboard.py:35-88, models/layers/attention.py:11-39,
 * models/layers/enhancement.py:17,44-51,65-82, compressai GDN/RBB).  fp32 MFMA (v_mfma_f32_32x32x2f32). */
int hyres_conv_forward(const hyres_conv_geom* g, const float* x, const float* w2, int ldw, float* y,
                       const hyres_epilogue* e, void* workspace, long long ws_bytes, hyres_stream_t s);
/* Scratch for split-K on small-M layers (0 = none needed).  Passing a NULL / short workspace is
 * valid: the launch then runs unsplit (same result, fewer blocks in flight). */
long long hyres_conv_workspace_bytes(const hyres_conv_geom* g);
/* Name of the kernel hyres_conv_forward launches for (g, e) — split != 0 when a workspace of
 * hyres_conv_workspace_bytes(g) is passed — as rocprof prints it, e.g.
 * "conv_fwd_kernel<2, 1, 2, 2, 0, false, false>" (16B-aligned operands assumed).  Host-only, no
 * launch: the profiling label of bench.py's roofline line comes from the launcher's own choice. */
int hyres_conv_kernel_name(const hyres_conv_geom* g, const hyres_epilogue* e, int split, char* buf, int n);
/* The same for the launch hyres_conv_forward would make with these operands: the route sees their real alignment
 * (x, w2, y, the epilogue's pointers, the workspace), ldw and the workspace size, and says itself whether it splits K.
 * A split launch is named "<tiles kernel>+conv_splitk_reduce4_kernel<Y fp16>" or "...+conv_splitk_reduce_kernel<...>",
 * whichever reduce follows. *vec4 (may be NULL) gets the route's float4-epilogue flag. Host-only: no launch, no device
 * access, the pointers are never dereferenced. */
int hyres_conv_kernel_name_at(const hyres_conv_geom* g, const hyres_epilogue* e, const void* x, const void* w2,
                              int ldw, const void* y, const void* ws, long long ws_bytes,
                              int* vec4, char* buf, int n);
/* Tuning override of the conv planners (sweeps only; not used by the product path). key 0: tile
 * (0 = 128x128, 1 = 128x64, 2 = 128x32, 3 = 64x128, 4 = 64x64), 1: split-K target block count,
 * 2: minimum K chunks per split; value -1 restores the built-in heuristic. *old (may be NULL) gets the
 * previous value. Not thread-safe against concurrent launches. */
/* The launcher's choice for (g, e): *tile = 0..4 as above (-1: the narrow VALU kernel), *nsplit = split-K
 * factor (1 = fused epilogue). Pure host function. */
int hyres_conv_plan(const hyres_conv_geom* g, const hyres_epilogue* e, int* tile, int* nsplit);
#define HYRES_TUNE_TILE 0
#define HYRES_TUNE_SPLIT_BLOCKS 1
#define HYRES_TUNE_SPLIT_MINCHUNKS 2
#define HYRES_TUNE_WGRAD_BLOCKS 3     /* weight gradients: split-K target block count */
#define HYRES_TUNE_WGRAD_MINCHUNKS 4  /* minimum 32-pixel chunks per split */
#define HYRES_TUNE_WGRAD_NT 5         /* 1: no tap grouping (one tap per block column group) */
#define HYRES_TUNE_WGRAD_MAXSPLIT 6   /* maximum split count (default 256; 64 on <= 16384-pixel grids) */
#define HYRES_TUNE_F32_GEMM 7         /* GEMM of the fp32 convolutions (forward, input-gradient, and the halo-staged /
                                       * 1x1 weight gradients): 1 bf16x6 (default: each fp32 operand split into 3 bf16
                                       * pieces, the 6 cross products with i + j <= 2, fp32 accumulation — per-product
                                       * error <= ~2^-25, i.e. fp32-accurate, on the 16x faster bf16 MFMA; DESIGN §4
                                       * "bf16x6"), 0 the native fp32 MFMA */
#define HYRES_TUNE_STREAM_H 8         /* 1 (default): fp16-activation 1x1 convs with K, Co <= 128 on >= 16384 pixels on the
                                       * streaming kernel (conv1x1_stream_h_kernel); 0: the tiled kernel (A/B) */
#define HYRES_TUNE_WRES_BF6_GUARD 9   /* 1 (default): the bf16x6 weight-resident 3x3 conv and the fused f16 ResidualUnit declare the whole VGPR file of
                                       * its SIMDs, so no other kernel's wave shares them; 0: DIAGNOSTIC ONLY, the
                                       * allocation under which co-resident waves computed wrong values (DESIGN §4
                                       * "Cross-kernel interference") */
#define HYRES_TUNE_STREAM_B6 10       /* 1 (default): the fp32 1x1 convs with (Ci, Co) in {(64,64), (64,128), (128,64)} on
                                       * >= 65536 pixels on the bf16x6 streaming kernel (conv1x1_stream_b6_kernel, any of
                                       * residual / ReLU mask / accumulate); 0: the tiled implicit GEMM (A/B) */
#define HYRES_TUNE_STREAM_CE 11       /* 1 (default): conv1x1_stream_b6_kernel stages each co tile's accumulator through LDS
                                       * so its epilogue reads / writes whole 128-byte pixel-row pieces; 0: the MFMA
                                       * lane layout straight to HBM (32 B per pixel row per wave instruction; A/B) */
#define HYRES_TUNE_WRES_BF6_V 12      /* conv3x3_wres_bf6_kernel variant: bit 0 (default 1) each tap's fragments read
                                       * one tap ahead, bit 1 static priority 1 for waves 4..7; 0: reads as the compiler
                                       * schedules them (A/B) */
#define HYRES_TUNE_NARROW_STRIP 13    /* 1 (default): Co <= 4 convs whose phases' taps are <= 3x3 grids, Wq % 4 == 0, on
                                       * conv_narrow_strip_kernel (4-pixel strips, weights in VGPRs); 0: conv_narrow_kernel */
#define HYRES_TUNE_WRES32 14          /* 1 (default): fp32 3x3 Ci = 64 convs on the weight-resident kernels
                                       * (conv3x3_wres_bf6 / _f32); 0: the implicit GEMM (A/B) */
#define HYRES_TUNE_WGRAD_PF 15        /* bf16x6 1x1 weight gradients: 2 (default) = operand loads two chunks ahead
                                       * (wgrad1x1_bf6_pf2_kernel), 1 = one chunk ahead (wgrad1x1_bf6_kernel) */
#define HYRES_TUNE_WGRAD_HALO_PF 16   /* bf16x6 3x3 halo weight gradients (one kernel row of 3 taps per block): 2
                                       * (default) = operand loads two chunks ahead (wgrad_halo_bf6_pf2_kernel), 1 = one
                                       * chunk ahead; the 5x5s stay on wgrad_halo_bf6_kernel (slower two ahead) */
#define HYRES_TUNE_STREAM_HF 17       /* 1 (default): fp16-IO 1x1 convs (Ci, Co in {64, 128}, >= 16384 px) with a residual /
                                       * ReLU-mask / accumulate operand on conv1x1_stream_hf_kernel; 0: the f16 tiles */
#define HYRES_TUNE_SMALL_TILE 18      /* 1 (default): fp32 implicit-GEMM tiles on <= 65536-pixel grids by the round-6 rule
                                       * (64x64 for the short-K 1x1s with Co <= 192, 128x128 for Co >= 512;
                                       * profiles/r6g_tile32.txt); 0: the round-5 rule (A/B) */
#define HYRES_TUNE_B6_SWIZZLE 19      /* 1 (default): the bf16x6 implicit GEMM stages its split planes in 64-B LDS rows with the
                                       * 16-B slots XOR-swizzled by row (conflict-free stores and reads); 0: 80-B padded rows
                                       * (2-way store conflicts), A/B; bit-identical */
#define HYRES_TUNE_B6_DB 20           /* the bf16x6 implicit GEMM's 64x64 tile staging K chunks in two LDS buffers (one barrier
                                       * per chunk, conv_fwd_b6db_kernel): 1 always, -1 on grids of <= 16384 output pixels,
                                       * 0 (default) never (one buffer, two barriers; faster in the graphed step); bit-identical */
#define HYRES_TUNE_STREAM_SAB 21      /* 1 (default): the SA_BWD input-gradient of MultiScaleRefine's fusion 1x1 (64 -> 192 on
                                       * >= 65536 pixels) on conv1x1_stream_b6_kernel<6, 4, 8 | acc>, its ROWSCALE forward
                                       * (192 -> 64) on <2, 12, 16>, and under AMP the SA_BWD input-gradient on
                                       * conv1x1_stream_hf_kernel<6, 4, 8 | acc>; 0: the implicit GEMMs */
#define HYRES_TUNE_WGRAD_HALO5_PF 22  /* 1: the 5-tap-row halo weight gradients (5x5, stride 1 / 2) also on the two-chunks-
                                       * ahead kernel (with key 16 = 2; bit-identical); 0 (default): one chunk ahead — no
                                       * gain per launch or in the step (profiles/r6v_wg5.txt, r6v_wg5_step_ab.txt) */
#define HYRES_TUNE_THIN_WINDOW 23     /* 1 (default): the thin (3-channel) 3x3 weight gradients keep each pixel's 3 x 3 Q window
                                       * in registers, sliding one column per pixel (bit-identical); 0: nine LDS reads per pixel */
#define HYRES_TUNE_BWD1X1_FUSED 24    /* bit 0 (default 1): the backward of the fp32 1x1 layers with a 128-channel output
                                       * gradient and a 64-channel input on >= 65536 pixels in one kernel
                                       * (conv1x1_bwd_fused_b6_kernel: input gradient + weight / bias gradient partials from
                                       * one read of the output gradient); 0: conv1x1_stream_b6_kernel +
                                       * wgrad1x1_bf6_pf2_kernel (A/B). Bit 1 (default 0, tests): no pixel floor for it and
                                       * for conv1x1_stream_b6_kernel's BIAS forms. Bit 2 (default 0): also the 64-channel
                                       * gradient / 128-channel input layers (measured no faster than the two kernels) */
#define HYRES_TUNE_KEYS 25
int hyres_conv_tuning(int key, int value, int* old);

/* Weight gradient:  dW[t][m][n] = sum_q P[q][m] * Q[shift_t(q)][n]  over a base grid q (B,Hq,Wq).
 * Conv2d: P = dY (output grid), Q = X;  ConvTranspose2d: P = X (input grid), Q = dY.
 * Result written (or accumulated) into the PyTorch-layout gradient dst[m*sm + n*sn + t*st]. */
typedef struct hyres_wgrad_desc {
    int B, Hq, Wq;               /* base grid (P's pixel grid) */
    int M, ldp;                  /* P channels / pixel stride */
    int N, ldq, Hqq, Wqq;        /* Q channels / pixel stride / Q spatial dims */
    int sq;                      /* Q stride of the base grid */
    int ntaps;
    int dh[HYRES_MAX_TAPS], dw[HYRES_MAX_TAPS];
    int sm, sn, st;              /* destination strides (floats) */
    int square_q;                /* Q -> Q*Q (GDN gamma gradient) */
    int accumulate;
    int f16_operands;            /* AMP: P, Q rounded to fp16 on the f16 MFMA, fp32 accumulation */
    int io_f16;                  /* fp16 operands in HBM (AMP training, fp16 saved activations): bit 0 = P is
                                  * fp16, bit 1 = Q is fp16; read natively by the f16 weight-gradient kernels
                                  * and the thin kernel (P), converted to fp32 scratch for the others */
} hyres_wgrad_desc;
int hyres_wgrad_desc_conv2d(hyres_wgrad_desc* d, int B, int H, int W, int Ci, int ldx, int Co,
                            int ldy, int KH, int KW, int stride, int pad, int dil);
int hyres_wgrad_desc_deconv2d(hyres_wgrad_desc* d, int B, int H, int W, int Ci, int ldx, int Co,
                              int ldy, int K, int pad);
long long hyres_wgrad_workspace_bytes(const hyres_wgrad_desc* d);
/* Name of the kernel hyres_conv_wgrad launches for d as rocprof prints it, every template argument spelled out,
 * e.g. "wgrad_halo_bf6_pf2_kernel<3, 1, 1, 2>" (16B-aligned operands and workspace assumed).  Host-only, no
 * launch: the launcher's own choice function. */
int hyres_wgrad_kernel_name(const hyres_wgrad_desc* d, char* buf, int n);
/* The same for a launch whose P / Q / workspace pointers are (non-zero) or are not (0) 16-byte aligned: a misaligned
 * operand reroutes the 1x1 and thin kernels to wgrad_kernel and clears its float4 flags.  Where hyres_conv_wgrad
 * refuses the launch (a halo / f16 descriptor off the vector path) the name is that of the planned kernel. */
int hyres_wgrad_kernel_name_at(const hyres_wgrad_desc* d, int p_aligned, int q_aligned, int ws_aligned, char* buf,
                               int n);
/* The launcher's plan for d under the same assumption: the split count, the grid (blocks, rounded up to a multiple
 * of 8; the thin kernel's row blocks x tap groups as they are), the block size and the lanes of the split reduce.
 * Any output may be NULL.  Pure host function. */
int hyres_wgrad_plan(const hyres_wgrad_desc* d, int* nsplit, int* blocks, int* threads, int* lanes);
/* dbias (optional, may be NULL): dbias[m] (+)= sum_q P[q][m] — the Conv2d bias gradient when P = dY
 * (replaces the separate colsum for conv layers; fused into the weight-gradient kernel). */
int hyres_conv_wgrad(const hyres_wgrad_desc* d, const float* p, const float* q, float* dst,
                     float* dbias, void* workspace, long long ws_bytes, hyres_stream_t s);

/* Deferred split-K reduce (same reference operation as hyres_conv_wgrad: the weight / bias gradient of
 * one conv in loss.backward(), src/utils/engine.py:63 via models/checkerboard.py:35-88). A weight
 * gradient is a GEMM over the batch's pixels, split over pixel ranges into [nsplit][ntaps][M][N]
 * partial slabs; hyres_conv_wgrad reduces them with one launch per layer. The deferred form launches
 * only the GEMM kernel and returns the reduce as up to two jobs (weight, then bias); the caller keeps
 * the workspace untouched and the destinations unread until hyres_wgrad_reduce_jobs has run them on the
 * same stream, where one launch reduces up to HYRES_WGRAD_MAX_JOBS jobs (a gradient segment of many
 * layers). Jobs of one launch must not write overlapping destinations. The result is bit-identical to
 * hyres_conv_wgrad's (same split plan, same per-output summation order). */
#define HYRES_WGRAD_MAX_JOBS 48
typedef struct hyres_wgrad_job {
    const float* slab;   /* [nsplit][ntaps][M][N] partials in the workspace */
    float* dst;          /* dst[m*sm + n*sn + t*st] (+)= sum over the nsplit partials */
    int nsplit, ntaps, M, N;
    int sm, sn, st, accumulate;
    int lanes;           /* reduce layout the launcher chose (4, 8 or 16): fixes the summation order */
    int reserved;
} hyres_wgrad_job;
int hyres_conv_wgrad_deferred(const hyres_wgrad_desc* d, const float* p, const float* q, float* dst,
                              float* dbias, void* workspace, long long ws_bytes, hyres_wgrad_job* jobs,
                              int* njobs, hyres_stream_t s);
int hyres_wgrad_reduce_jobs(const hyres_wgrad_job* jobs, int n, hyres_stream_t s);

/* Fused backward of a plain fp32 1x1 Conv2d (bf16x6, HYRES_TUNE_BWD1X1_FUSED): the input gradient
 * hyres_conv_forward(g, gp, w2, ldw, gx, e) computes (bit-identical to conv1x1_stream_b6_kernel's) and the partials of
 * the weight / bias gradient hyres_conv_wgrad_deferred(d, gp, q, dw, dbias) computes, in one launch that reads the
 * output gradient gp once. The split reduce comes back as jobs, as from hyres_conv_wgrad_deferred.
 * hyres_conv1x1_bwd_fused_ok: whether (g, e, d) and the operands' alignment (a NULL pointer: assumed aligned) are
 * eligible; otherwise the caller launches the two kernels. */
int hyres_conv1x1_bwd_fused_ok(const hyres_conv_geom* g, const hyres_epilogue* e, const hyres_wgrad_desc* d,
                               const void* gp, const void* q, const void* w2, int ldw, const void* gx);
long long hyres_conv1x1_bwd_fused_workspace_bytes(const hyres_wgrad_desc* d);
int hyres_conv1x1_bwd_fused_kernel_name(const hyres_conv_geom* g, const hyres_epilogue* e, const hyres_wgrad_desc* d,
                                        char* buf, int n);
int hyres_conv1x1_bwd_fused(const hyres_conv_geom* g, const float* gp, const float* w2, int ldw, float* gx,
                            const hyres_epilogue* e, const hyres_wgrad_desc* d, const float* q, float* dw, float* dbias,
                            void* workspace, long long ws_bytes, hyres_wgrad_job* jobs, int* njobs, hyres_stream_t s);

/* Fused ResidualUnit / ResidualBottleneckBlock forward, autocast inference with fp16 activations (round 4):
 * y = [relu](x + W3 * relu(W2 (*) relu(W1 * x + b1) + b2) + b3) in ONE launch, t1 / t2 kept on chip (fp16, the
 * unfused path's rounding points). Replaces the three-conv chain of the ResidualUnit in models/layers/attention.py:11-30
 * (final_relu = 1) and of compressai's ResidualBottleneckBlock at models/checkerboard.py:38,42,51,56 (final_relu = 0).
 * x, y: [B][H][W][N] fp16, N = 128, W % 64 == 0 (hyres_ru_fused_f16_ok); weights / biases fp32 in the PyTorch
 * layouts (w1 [N/2][N], w2 [N/2][N/2][3][3], w3 [N][N/2]), converted to fp16 on load; 16-byte aligned. */
int hyres_ru_fused_f16_ok(int B, int H, int W, int N);
int hyres_ru_fused_f16(const void* x, void* y, int B, int H, int W, int N, const float* w1, const float* b1,
                       const float* w2, const float* b2, const float* w3, const float* b3, int final_relu,
                       void* t1, void* t2, hyres_stream_t s);
/* t1, t2: NULL (inference), or [B][H][W][N/2] fp16 outputs receiving the two intermediates (AMP training: the
 * backward of the three convs reads them). */

/* ------------------------------------------------------------------------------------------ */
/* operand dtypes of the element-wise and MultiScaleRefine entry points                       */
/* ------------------------------------------------------------------------------------------ */
/* The activation / gradient operands of these entry points are ``void*``: fp32, or fp16 in HBM (autocast inference
 * and AMP training) with fp32 arithmetic either way. Their last argument before the stream says which:
 *  - ``int dt`` (entry points with both operand classes), a mask of
 *      HYRES_DT_ACT16:  the SAVED activations the forward wrote (y, x, pre, a / b, the GDN norm) are fp16;
 *      HYRES_DT_GRAD16: the gradients in and out (g, gy, gx, ga / gb, dn, gs) are fp16 — autocast's own semantics
 *                       inside the f16 region (the gradient of an fp16 tensor is fp16, src/utils/engine.py:32,50-53).
 *    Kernels exist for 0, ACT16 and ACT16 | GRAD16; GRAD16 alone (fp16 gradients of fp32 activations) and any other
 *    value are HYRES_E_ARG — except hyres_bilinear_bwd_prelu, which has all four.
 *  - ``int f16`` (entry points with one operand class): 0 = fp32, 1 = fp16; anything else is HYRES_E_ARG.
 *  - hyres_add2d's two-sided ``int io``: HYRES_IO_X16 | HYRES_IO_Y16.
 * The value is checked first, before any pointer and before any launch. Parameters, weight gradients and the saved
 * fp32 side tensors (pooled, attn, ...) stay ``float*``. Vector paths need 4-element alignment of the operand: 16 B
 * as fp32, 8 B as fp16; where an fp32 entry falls back to a scalar kernel on a ragged / misaligned operand and the
 * fp16 form has no scalar kernel, that is said at the entry point. */
#define HYRES_DT_ACT16 1
#define HYRES_DT_GRAD16 2

/* column sums over pixels: dst[c] (+)= sum_p x[p*ld + c]  (bias gradients); x fp32 / fp16 (f16), fp32 sums */
int hyres_colsum(const void* x, int P, int C, int ld, float* dst, int accumulate, void* workspace,
                 long long ws_bytes, int f16, hyres_stream_t s);
long long hyres_colsum_workspace_bytes(int P, int C);

/* ------------------------------------------------------------------------------------------ */
/* layout / elementwise                                                                       */
/* ------------------------------------------------------------------------------------------ */
int hyres_nchw_to_nhwc(const float* x, float* y, int B, int C, int H, int W, int ldy, hyres_stream_t s);
int hyres_nhwc_to_nchw(const float* x, int ldx, float* y, int B, int C, int H, int W, hyres_stream_t s);
/* y = a + alpha*b over n contiguous floats (hyres.py:48,62 glue) */
int hyres_axpby(const float* a, const float* b, float alpha, float* y, long long n, hyres_stream_t s);
/* x_hat = clamp(x0 + r, 0, 1)  (models/hyres.py:66-67); bwd: g passes where 0 < x0+r < 1 */
int hyres_add_clamp01(const float* x0, const float* r, float* y, long long n, hyres_stream_t s);
int hyres_add_clamp01_bwd(const float* pre, const float* g, float* gx, int accumulate, long long n,
                          hyres_stream_t s);
/* g_out = g * (y > 0)   (ReLU backward), optional accumulate into dst */
int hyres_relu_bwd(const float* y, const float* g, float* gx, long long n, hyres_stream_t s);
/* strided variant over NHWC slices (dtypes: "operand dtypes" above; y is the saved activation) */
int hyres_relu_bwd_2d(const void* y, int ldy_, const void* g, int ldg, void* gx, int ldgx, long long P,
                      int C, int dt, hyres_stream_t s);
/* PReLU backward from the saved pre-activation x: gx = g*(x>0 ? 1 : a); dslope += sum(g*x*(x<=0))
 * (enhancement.py nn.PReLU). ws: hyres_reduce_workspace_bytes(P*C). */
int hyres_prelu_bwd(const void* x, int ldx, const void* g, int ldg, void* gx, int ldgx, long long P,
                    int C, const float* slope, float* dslope, void* ws, long long ws_bytes, int dt,
                    hyres_stream_t s);
/* AttentionBlock gate (models/layers/attention.py:44-47): out = a*sigmoid(b) + x. f16 (autocast inference: a, b, x,
 * out fp16) needs n % 4 == 0 and has no scalar kernel; fp32 falls back to one on a ragged n or a misaligned operand. */
int hyres_attn_gate_fwd(const void* a, const void* b, const void* x, void* out, long long n, int f16,
                        hyres_stream_t s);
/* a, b are the saved activations, g / ga / gb the gradients; a ragged n or a misaligned operand runs the scalar kernel */
int hyres_attn_gate_bwd(const void* a, const void* b, const void* g, void* ga, void* gb, long long n, int dt,
                        hyres_stream_t s);
/* The same with the ReLU backward of a folded in (a = the last ResidualUnit's ReLU output, models/layers/attention.py:
 * 11-30, 44-47): ga = (a > 0) ? g * sigmoid(b) : 0. n % 4 == 0 and every operand aligned are REQUIRED (round 6). */
int hyres_attn_gate_bwd_relu(const void* a, const void* b, const void* g, void* ga, void* gb, long long n, int dt,
                             hyres_stream_t s);
/* y (+)= x  (gradient fan-in); f16: both fp16 */
int hyres_accumulate(const void* x, void* y, long long n, int f16, hyres_stream_t s);
/* y[p*ldy + c] (+)= x[p*ldx + c]  over P pixels x C channels (strided gradient fan-in / copy), fp32 add;
 * io: HYRES_IO_X16 = x fp16, HYRES_IO_Y16 = y fp16, 0 = both fp32 */
int hyres_add2d(const void* x, int ldx, void* y, int ldy, long long P, int C, int accumulate, int io,
                hyres_stream_t s);
/* NHWC x [B][Hs][Ws][C] (pixel stride ldx) -> y [B][Hd][Wd][C] (ldy), both anchored at the top-left corner:
 * y[b][h][w][c] (+)= h < Hs && w < Ws ? x[b][h][w][c] : 0. Hd >= Hs, Wd >= Ws is a zero pad at the bottom and
 * right, Hd <= Hs, Wd <= Ws the crop that is its gradient (and the other way round); accumulate: gradient fan-in
 * (outside the source y keeps its value). io as hyres_add2d. ResidualJPEGCompression pads the residual of an
 * image whose sides are not multiples of the transforms' stride with it and crops residual_hat back. */
int hyres_pad2d(const void* x, int ldx, int Hs, int Ws, void* y, int ldy, int Hd, int Wd, int B, int C,
                int accumulate, int io, hyres_stream_t s);
/* y = a * b elementwise (in-place allowed: CheckboardMaskedConv2d's weight.data *= mask) */
int hyres_mul(const float* a, const float* b, float* y, long long n, hyres_stream_t s);
/* stream-ordered memset 0 (hipMemsetAsync) */
int hyres_zero(void* p, long long bytes, hyres_stream_t s);
/* y (+)= (coef ? coef[0] : 1) * scale * x */
int hyres_scale(const float* x, const float* coef, float scale, float* y, long long n, int accumulate,
                hyres_stream_t s);

/* GDN reparametrisation (compressai NonNegativeParametrizer + LowerBound):
 * beta' = max(beta, bb)^2 - ped,  gamma' = max(gamma, gb)^2 - ped;  and backward. */
int hyres_gdn_reparam_fwd(const float* beta, const float* gamma, float* beta_p, float* gamma_p, int C,
                          hyres_stream_t s);
int hyres_gdn_reparam_bwd(const float* beta, const float* gamma, const float* dbeta_p,
                          const float* dgamma_p, float* dbeta, float* dgamma, int C, int accumulate,
                          hyres_stream_t s);
/* GDN backward helper: dn = g * y / n * (-0.5 GDN | +0.5 IGDN); y, n the saved activations, g, dn the gradients */
int hyres_gdn_dnorm(const void* g, const void* y, const void* n, void* dn, long long P, int C,
                    int inverse, int dt, hyres_stream_t s);

/* ------------------------------------------------------------------------------------------ */
/* quantisation, checkerboard context, entropy models                                         */
/* ------------------------------------------------------------------------------------------ */
/* U(-0.5, 0.5) noise (counter-based hash RNG), replaces torch.empty_like().uniform_() in
 * models/utils/quantization.py:6-10 and compressai EntropyModel.quantize("noise") */
int hyres_uniform_noise(float* out, long long n, unsigned long long seed, unsigned long long offset,
                        hyres_stream_t s);
/* Same distribution with the seed in device memory: draws with seed = mix(*seed_dev ^ salt), then
 * advances *seed_dev (stream-ordered), so a captured HIP graph draws fresh noise on every replay. */
int hyres_uniform_noise_dev(float* out, long long n, unsigned long long* seed_dev, unsigned long long salt,
                            hyres_stream_t s);
/* Quantizer.quantize (models/utils/quantization.py:11-14): mode 0 = "ste" value round(x)-x+x,
 * mode 1 = round (half-to-even) */
int hyres_quantize(const float* x, int mode, float* y, long long n, hyres_stream_t s);
/* Anchor pass (models/checkerboard.py:106-122): y_a = y*[(h+w) even];
 * y_a_hat = STE(y_a - m_a) + m_a  or  y_a + noise. Writes y_a_hat (NHWC [B,H,W,C]). */
int hyres_ckbd_anchor_fwd(const float* y, const float* means_a, int ldm, const float* noise,
                          float* y_a_hat, int B, int H, int W, int C, hyres_stream_t s);
/* Non-anchor pass + combine + GaussianConditional (checkerboard.py:132-142, compressai GC):
 * y_na_hat, y_hat = y_a_hat + y_na_hat, scales = s_a + s_na, means = m_a + m_na,
 * y_q = round(y - means) + means (eval) or y + noise_gc (train), lik = LB(GC(y_q; scales, means)).
 * Also accumulates sum(log lik) per block into ws (bpp partial). */
int hyres_ckbd_nonanchor_gc_fwd(const float* y, const float* y_a_hat, const float* params_a, int lda,
                                const float* params_na, int ldn, const float* noise_q,
                                const float* noise_gc, float* y_hat, float* scales, float* means,
                                float* y_q, float* lik, int B, int H, int W, int C, hyres_stream_t s);
/* backward of the above: g_y = g_yhat (+ GC term in training); [g_scales | g_means] written to
 * both param-aggregation gradient buffers (scales = s_a + s_na, means = m_a + m_na).  The STE /
 * noise quantisers pass the gradient straight to y and give none to the means. */
int hyres_ckbd_gc_bwd(const float* y_q, const float* scales, const float* means, const float* g_lik,
                      const float* g_yhat, int training, float* g_y, float* g_params_a, int lda,
                      float* g_params_na, int ldn, int B, int H, int W, int C, hyres_stream_t s);
/* g_y[anchor positions] += g_ya (context-model path back into the anchor quantiser) */
int hyres_ckbd_anchor_bwd(const float* g_ya, float* g_y, int B, int H, int W, int C, hyres_stream_t s);

/* EntropyBottleneck forward (compressai 1.2.6): z NHWC [P][C]; params packed per channel
 * (see hyres_eb_pack); z_q = z + noise (train) | round(z - med) + med (eval); lik = LB(sig(u)-sig(l));
 * z_hat_ste = quantize_ste(z - med) + med (checkerboard.py:98-101). */
int hyres_eb_fwd(const float* z, const float* packed, const float* noise, int training, float* z_q,
                 float* lik, float* z_hat_ste, long long P, int C, hyres_stream_t s);
int hyres_eb_bwd(const float* z_q, const float* packed, const float* lik, const float* g_lik,
                 const float* g_zhat, int training, int noisequant, float* g_z, float* g_packed_ws,
                 long long P, int C, hyres_stream_t s);
long long hyres_eb_workspace_bytes(long long P, int C);
/* pack EB parameters (softplus(matrices), biases, tanh(factors), quantile medians) per channel */
#define HYRES_EB_REC 64
int hyres_eb_pack(const float* const* mats, const float* const* biases, const float* const* factors,
                  const float* quantiles, float* packed, int C, hyres_stream_t s);
/* reduce the per-block packed gradients of hyres_eb_bwd into the parameter gradients */
int hyres_eb_unpack_grad(const float* g_packed_ws, int nblocks, const float* const* mats,
                         const float* const* factors, float* const* g_mats, float* const* g_biases,
                         float* const* g_factors, float* g_quantiles, int C, int accumulate,
                         hyres_stream_t s);
/* EntropyBottleneck.loss (aux loss) and its gradient wrt quantiles */
int hyres_eb_aux_loss(const float* packed, const float* quantiles, const float* target, float* loss,
                      float* g_quantiles, int C, hyres_stream_t s);

/* ------------------------------------------------------------------------------------------ */
/* MultiScaleRefine pieces (models/layers/enhancement.py)                                     */
/* ------------------------------------------------------------------------------------------ */
/* bilinear, align_corners=False, torch source-index rule (scale = in/out, or 1/scale_factor). f16 (x / y, or the
 * gradients gy / gx, fp16): the forward then needs C % 4 == 0, ld % 4 == 0, 8B-aligned x / y and takes no accumulate
 * (HYRES_E_ARG); the fp32 forward and both backward forms have scalar kernels. */
int hyres_bilinear_fwd(const void* x, int ldx, void* y, int ldy, int B, int Hi, int Wi, int Ho, int Wo,
                       int C, float scale_h, float scale_w, int accumulate, int f16, hyres_stream_t s);
int hyres_bilinear_bwd(const void* gy, int ldgy, void* gx, int ldgx, int B, int Hi, int Wi, int Ho,
                       int Wo, int C, float scale_h, float scale_w, int accumulate, int f16, hyres_stream_t s);
/* SEBlock (enhancement.py:25-40): s = sigmoid(W2 relu(W1 mean_hw(x))); y = x*s. pooled / hidden / sgate fp32.
 * f16 (x, y fp16) needs C % 4 == 0, 256 % (C/4) == 0 and 8B-aligned x / y (no scalar kernels). */
int hyres_se_fwd(const void* x, const float* w1, const float* w2, void* y, float* pooled,
                 float* hidden, float* sgate, int B, int HW, int C, int Cr, void* ws, long long ws_bytes, int f16,
                 hyres_stream_t s);
/* x the saved activation, gy / gx the gradients; weight gradients fp32 */
int hyres_se_bwd(const void* x, const void* gy, const float* w1, const float* w2,
                 const float* pooled, const float* hidden, const float* sgate, void* gx, float* gw1,
                 float* gw2, int B, int HW, int C, int Cr, void* ws, long long ws_bytes, int dt, hyres_stream_t s);
/* hyres_se_bwd with the backward of the PReLU that produced x folded in (round 6; MultiScaleRefine's
 * SE(PReLU(conv_in(x))), enhancement.py:107-110): gx = PReLU'(pre) * dL/dx, the slope gradient
 * sum_{pre <= 0} pre * dL/dx ADDED to dslope[0] (block partials in the workspace, fixed-order sum). pre has x's
 * dtype; with fp16 gradients the gradient is rounded to fp16 before the PReLU, as the unfused chain stores it.
 * C % 4 == 0 and aligned gy / gx / pre are required; the workspace is hyres_se_workspace_bytes + B*C*4 + 2048*4
 * bytes. Replaces prelu_bwd after the SE backward. */
int hyres_se_bwd_prelu(const void* x, const void* gy, const float* w1, const float* w2, const float* pooled,
                       const float* hidden, const float* sgate, void* gx, float* gw1, float* gw2, int B, int HW, int C,
                       int Cr, const void* pre, const float* slope, float* dslope, void* ws, long long ws_bytes, int dt,
                       hyres_stream_t s);
long long hyres_se_workspace_bytes(int B, int HW, int C);
/* SpatialAttention (enhancement.py:7-21) fused: a = sigmoid(conv7x7([mean_c, max_c])); y = x * a.
 * pooled2 [P][2] and argmax [P] (first maximal channel, torch.max semantics) are saved for backward, fp32 / int
 * like attn. C % 4 == 0, aligned x/y/gy/gx. y == NULL: the attention map only. */
int hyres_spatial_attn_fwd(const void* x, const float* w, float* pooled2, int* argmax, float* attn,
                           void* y, int B, int H, int W, int C, int f16, hyres_stream_t s);
int hyres_spatial_attn_bwd(const void* x, const float* w, const float* pooled2, const int* argmax,
                           const float* attn, const void* gy, void* gx, float* gw, int B, int H, int W,
                           int C, void* ws, long long ws_bytes, int dt, hyres_stream_t s);
long long hyres_spatial_attn_workspace_bytes(int B, int H, int W);
/* Training with SpatialAttention's multiply folded into MultiScaleRefine's fusion 1x1 (HYRES_EPI_ROWSCALE forward,
 * enhancement.py:105-109): h = PReLU(attn[p] * (W multi)[p] + b), ``pre`` its pre-activation [P][C] (C = fusion
 * width, ldpre), gy = dL/dh [P][ldg]. Writes gs = attn[p] * gp (gp = PReLU-backward of gy: the fusion 1x1's weight-
 * and input-gradient operand), glogit[p] = (1 - attn[p]) * sum_o gp[p,o] * (pre[p,o] - b[o]) (= the gradient at the
 * attention logit: attn * z = pre - b, no division), and ADDS dbias += sum_p gp, dslope += sum_{pre <= 0} gy * pre
 * (deterministic per-block partials). ``pre`` is the saved activation, gy / gs the gradients; attn, bias, glogit, dbias,
 * dslope fp32. C % 4 == 0 (fp16 pre: C, ldpre, ldg % 8 == 0), C <= 64, 16B-aligned rows;
 * ws >= hyres_sa_fold_workspace_bytes(P, C). */
long long hyres_sa_fold_workspace_bytes(long long P, int C);
int hyres_sa_fold_bwd(const void* pre, int ldpre, const void* gy, int ldg, const float* attn, const float* bias,
                      const float* slope, void* gs, float* glogit, float* dbias, float* dslope, long long P, int C,
                      void* ws, long long ws_bytes, int dt, hyres_stream_t s);
/* SpatialAttention's map backward from the logit gradient: gw += d conv7x7 weight, gpooled2 = [P][2] gradients of
 * the channel mean (already divided by C, as HYRES_EPI_SA_BWD reads it) and the channel max. ws as
 * hyres_spatial_attn_workspace_bytes(B, H, W). */
int hyres_spatial_attn_bwd_map(const float* glogit, const float* pooled2, const float* w, float* gpooled2, float* gw,
                               int B, int H, int W, int C, void* ws, long long ws_bytes, hyres_stream_t s);
/* Round 6: the up-sample's backward with the PReLU backward of the layer that produced its input folded in
 * (MultiScaleRefine scales 2 / 3: conv + PReLU, then the bilinear up-sample, enhancement.py:89-103): writes
 * gx = pre > 0 ? g : slope * g (g = the gather sum, rounded to fp16 first with fp16 gradients) — NOT accumulated, the
 * caller is the first writer — and ADDS dslope += sum_{pre <= 0} pre * g (deterministic block partials in ws).
 * dt: HYRES_DT_GRAD16 gy / gx fp16, HYRES_DT_ACT16 pre fp16 (all four masks). C % 4 == 0, aligned rows;
 * ws >= hyres_bilinear_bwd_prelu_workspace_bytes. */
long long hyres_bilinear_bwd_prelu_workspace_bytes(int B, int Hi, int Wi, int C);
int hyres_bilinear_bwd_prelu(const void* gy, int ldgy, void* gx, int ldgx, int B, int Hi, int Wi, int Ho, int Wo, int C,
                             float scale_h, float scale_w, const void* pre, int ldpre, const float* slope, float* dslope,
                             void* ws, long long ws_bytes, int dt, hyres_stream_t s);

/* ------------------------------------------------------------------------------------------ */
/* losses and optimiser (src/losses/rd_loss.py:18-44, src/utils/engine.py:56-90)              */
/* ------------------------------------------------------------------------------------------ */
/* out[0] (+)= sum(log(x)) over n floats (two-pass deterministic) */
int hyres_sum_log(const float* x, long long n, float* out, void* ws, long long ws_bytes,
                  hyres_stream_t s);
/* out[0] = sum((a-b)^2) */
int hyres_sum_sqdiff(const float* a, const float* b, long long n, float* out, void* ws,
                     long long ws_bytes, hyres_stream_t s);
long long hyres_reduce_workspace_bytes(long long n);
/* g = coef / x  (d/dx of coef*log x) ; g = coef*(a-b) */
int hyres_scale_recip(const float* x, const float* coef, float scale, float* g, long long n,
                      hyres_stream_t s);
int hyres_scale_diff(const float* a, const float* b, const float* coef, float scale, float* g,
                     long long n, hyres_stream_t s);
/* RateDistortionLoss scalars from sums = [sum log lik_y, sum log lik_z, sum sq err]:
 * *out[i] = [loss, bpp, residual_bpp, y_bpp, z_bpp, mse][i]  (rd_loss.py:23-42, alpha = 0) */
int hyres_rd_finalize(const float* sums, const float* jpeg_bpp, float lmbda, long long npx,
                      long long nel, float* const* out, hyres_stream_t s);
/* backward coefficients from the six output gradients: coef = [c_y, c_z, c_mse] */
int hyres_rd_bwd_coef(const float* g0, const float* g1, const float* g2, const float* g3,
                      const float* g4, const float* g5, float lmbda, long long npx, long long nel,
                      float* coef, hyres_stream_t s);
/* sum of squares of a flat buffer, accumulated and returned in fp64 -> out[0] (device double): a finite
 * gradient never overflows it, so !isfinite(out[0]) <=> some element is inf/NaN (GradScaler found_inf is
 * element-wise, torch/amp/grad_scaler.py) and the clip norm of engine.py:76 stays exact; ws >= 8 bytes per
 * block (hyres_reduce_workspace_bytes). */
int hyres_sumsq(const float* x, long long n, double* out, void* ws, long long ws_bytes, hyres_stream_t s);
/* fused Adam over a flat parameter buffer: torch.optim.Adam (foreach, amsgrad=False, weight_decay=0)
 * replacing src/utils/engine.py:68-82 (clip_grad_norm_ -> [GradScaler] -> Adam.step). Hyper-parameters
 * are doubles: 1-beta, the bias corrections, step_size and sqrt(bc2) are formed in double precision as
 * torch does in Python, then used as fp32 scalars. step_dev: device float = completed steps (incremented
 * on device unless the step is skipped). sumsq (device, may be NULL): sum of squares of ``grad``;
 * with max_norm > 0 the clip_grad_norm_ factor min(1, max_norm/(||g*gscale||+1e-6)) is applied on the
 * fly. gscale (device, may be NULL): GradScaler unscale factor 1/scale. skip: 0 never, 1 skip when
 * sumsq is not finite (GradScaler.step's found_inf), 2 skip when sumsq is NaN (engine.py:60-74). */
int hyres_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                    double lr, double beta1, double beta2, double eps, float* step_dev,
                    const double* sumsq, double max_norm, const float* gscale, int skip,
                    hyres_stream_t s);
/* torch GradScaler.update on the device (engine.py:73,80): found_inf = !isfinite(sumsq[0]) of the
 * scaled gradients; scale *= backoff on inf, *= growth after growth_interval clean steps;
 * inv_scale = 1/scale. */
int hyres_grad_scaler_update(const double* sumsq, float* scale, float* inv_scale, int* growth_tracker,
                             double growth_factor, double backoff_factor, int growth_interval,
                             hyres_stream_t s);

/* ------------------------------------------------------------------------------------------ */
/* VGG16 perceptual loss (src/losses/vgg16.py, rd_loss.py:40), NHWC           */
/* ------------------------------------------------------------------------------------------ */
/* torchvision Normalize: y = (x - mean[c]) / std[c], C <= 4; mean / stdv are HOST arrays
 * (vgg16.py:35-38, 50-51) */
int hyres_normalize_fwd(const float* x, float* y, long long P, int C, const float* mean, const float* stdv,
                        hyres_stream_t s);
int hyres_normalize_bwd(const float* g, float* gx, long long P, int C, const float* mean, const float* stdv,
                        int accumulate, hyres_stream_t s);
/* y = max(x, 0) (nn.ReLU at a slice boundary, vgg16.py:29-33) */
int hyres_relu_fwd(const float* x, float* y, long long n, hyres_stream_t s);
/* nn.MaxPool2d(2, 2): argmax in {0..3} ((0,0),(0,1),(1,0),(1,1)), first maximum wins, NaN propagates */
int hyres_maxpool2_fwd(const float* x, float* y, unsigned char* argmax, int B, int H, int W, int C, hyres_stream_t s);
int hyres_maxpool2_bwd(const float* g, const unsigned char* argmax, float* gx, int B, int H, int W, int C,
                       int accumulate, hyres_stream_t s);
/* out[0] (+)= mean |a - b| (two-pass deterministic), its backward ga (+)= coef[0] * sign(a - b) / n
 * (vgg16.py:58 torch.abs(x - y).mean()) */
long long hyres_absdiff_workspace_bytes(long long n);
int hyres_absdiff_mean(const float* a, const float* b, long long n, float* out, int accumulate, void* ws,
                       long long ws_bytes, hyres_stream_t s);
int hyres_absdiff_bwd(const float* a, const float* b, const float* coef, long long n, float* ga, int accumulate,
                      hyres_stream_t s);

/* ------------------------------------------------------------------------------------------ */
/* entropy coding (compress / decompress): compressai 1.2.6 semantics            */
/* ------------------------------------------------------------------------------------------ */
/* GaussianConditional.build_indexes(scales) + quantize(y, "symbols", means) of one checkerboard pass
 * (models/checkerboard.py:159-161): params NHWC [B,H,W,ldp] with scales in channels [0,M) and means in
 * [M,2M); y NHWC masked by parity (0 anchor, 1 non-anchor, -1 none); sym/idx int32 NCHW. y == NULL:
 * indexes only (decoder side). */
int hyres_gc_symbols(const float* y, int ldy, const float* params, int ldp, int M, int B, int H, int W, int parity,
                     const float* scale_table, int nt, int* sym, int* idx, hyres_stream_t s);
/* GaussianConditional.decompress's dequantize: out[NHWC] (+)= sym + means (checkerboard.py:162-164) */
int hyres_gc_dequant(const int* sym, const float* params, int ldp, int M, int B, int H, int W, float* out, int ldo,
                     int accumulate, hyres_stream_t s);
/* EntropyBottleneck.compress/decompress symbolisation around the channel medians (checkerboard.py:170-171):
 * dequant = 0: sym = round(z - med); 1: zhat = sym + med */
int hyres_eb_symbols(const float* z, int ldz, const float* medians, int B, int H, int W, int C, int* sym,
                     float* zhat, int ldo, int dequant, hyres_stream_t s);
/* compressai pmf_to_quantized_cdf (cpp_exts/ops/ops.cpp): n probabilities -> n+1 CDF entries summing to
 * 2^precision with every symbol frequency >= 1 (host) */
int hyres_pmf_to_quantized_cdf(const float* pmf, int n, int precision, int* cdf_out);
/* compressai RansEncoder.encode_with_indexes / RansDecoder.decode_with_indexes (cpp_exts/rans): 64-bit
 * rANS, 16-bit CDFs [ncdf][cdf_stride], bypass escape for out-of-range symbols (host). out == NULL:
 * *out_len = the string length only. */
int hyres_rans_encode_with_indexes(const int* symbols, const int* indexes, long long n, const int* cdfs,
                                   int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf,
                                   unsigned char* out, long long out_cap, long long* out_len);
int hyres_rans_decode_with_indexes(const unsigned char* in, long long in_len, const int* indexes, long long n,
                                   const int* cdfs, int cdf_stride, const int* cdf_sizes, const int* offsets,
                                   int ncdf, int* symbols_out);

/* ------------------------------------------------------------------------------------------ */
/* Device rANS coder (opt-in, HYRES_ENTROPY_CODER=device): the wave-interleaved string format HRW1 (csrc/wrans_core.h,
 * DESIGN.md). One string per image and pass: "HRW1", n, n_esc, n_words, 64 lane states, the escape values, the payload
 * words. The coded symbols of a [C,H,W] latent are the positions, in (c, h, w) order, that the checkerboard ``parity``
 * (0 anchor, 1 non-anchor, -1 all) owns; ``sym`` / ``idx`` are the full [B][C][H][W] arrays of hyres_gc_symbols /
 * hyres_eb_symbols (idx == NULL: the CDF of position (c, h, w) is row c). CDF tables as for the host coder, on the
 * device for the device calls. Not compressai's wire format: hyres_rans_* keeps that. */
/* ------------------------------------------------------------------------------------------ */
/* coded symbols of one string, or -1 on a bad shape (host) */
long long hyres_wrans_count(int C, int H, int W, int parity);
/* the most bytes one string can take: 528 + 8 per coded symbol, or -1 (host) */
long long hyres_wrans_max_string_bytes(int C, int H, int W, int parity);
/* workspace of hyres_wrans_encode for B strings, or -1 (host) */
long long hyres_wrans_workspace_bytes(int B, int C, int H, int W, int parity);
/* Encodes B strings and packs them one after the other into ``out`` (capacity out_cap >= B * max_string_bytes behind
 * the start offset; a write past it is dropped). offs[0..B] (device) receives the byte offsets: offs[b + 1] - offs[b]
 * is string b's length. chain = 0 starts at offs[0] = 0; chain = 1 starts at the offs[0] an earlier call on the
 * stream left there, so several calls fill one buffer and one offset table (pass offs + B of the previous call).
 * Two kernels on ``s``, no host sync. */
int hyres_wrans_encode(const int* sym, const int* idx, int B, int C, int H, int W, int parity, const int* cdfs,
                       int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf, unsigned char* out,
                       long long out_cap, long long* offs, int chain, void* ws, long long ws_bytes,
                       hyres_stream_t s);
/* Decodes string b at strings + offs[b] (4-byte aligned, offs[0..B] on the device; validate every string with
 * hyres_wrans_validate on the host first) into the full symbol array sym_out [B][C][H][W]: owned positions from the
 * stream, the others (int)rintf(0.f - mean) with mean = params[pixel * ldp + M + c] (NHWC params [.., scales | means];
 * params may be NULL for parity -1). Reads are clamped to each string's end and to the tables. One kernel on ``s``. */
int hyres_wrans_decode(const unsigned char* strings, const long long* offs, const int* idx, int B, int C, int H, int W,
                       int parity, const int* cdfs, int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf,
                       const float* params, int ldp, int M, int* sym_out, hyres_stream_t s);
/* one string holds the coded symbols of a [C,H,W] latent under ``parity``: magic, n, lengths consistent with the byte
 * count; HYRES_E_ARG with the reason otherwise (host) */
int hyres_wrans_validate(const unsigned char* in, long long in_len, int C, int H, int W, int parity);
/* the same coder on host memory, one string (csrc/wrans_core.h); out == NULL: *out_len only. No GPU call (host) */
int hyres_wrans_encode_host(const int* sym, const int* idx, int C, int H, int W, int parity, const int* cdfs,
                            int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf, unsigned char* out,
                            long long out_cap, long long* out_len);
int hyres_wrans_decode_host(const unsigned char* in, long long in_len, const int* idx, int C, int H, int W, int parity,
                            const int* cdfs, int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf,
                            const float* params, int ldp, int M, int* sym_out);

/* ------------------------------------------------------------------------------------------ */
/* Segmented device rANS format HRW2 (a second opt-in on top of HRW1): one string is cut into S = max(1, ceil(n / 64R))
 * segments of R = ``seg_rows`` rows of 64 coded symbols, each coded exactly as HRW1 codes a whole string, so one
 * wave64 codes one segment and a string takes S waves. "HRW2", n, R, S; S x {esc_end, words_end} (cumulative); S x 64
 * lane states; the escapes; the payload words (csrc/wrans_core.h). Everything else is as for
 * hyres_wrans_*: the coded symbols, the arrays, the tables, ``chain``. hyres_wrans_validate refuses an HRW2 string
 * and hyres_wrans2_validate an HRW1 string. */
/* ------------------------------------------------------------------------------------------ */
/* segments of one string, or -1 on a bad shape or seg_rows < 1 (host) */
long long hyres_wrans2_segments(int C, int H, int W, int parity, int seg_rows);
/* the most bytes one string can take: 16 + 520 per segment + 8 per coded symbol, or -1 (host) */
long long hyres_wrans2_max_string_bytes(int C, int H, int W, int parity, int seg_rows);
/* workspace of hyres_wrans2_encode for B <= 65535 strings, or -1 (host) */
long long hyres_wrans2_workspace_bytes(int B, int C, int H, int W, int parity, int seg_rows);
/* As hyres_wrans_encode, in HRW2 with seg_rows rows per segment (out_cap >= B * max_string_bytes behind the start
 * offset). Three kernels on ``s`` (encode and pack on a (segments, B) grid, a scan of one wave per string between
 * them), no host sync; bad arguments are refused before any launch. */
int hyres_wrans2_encode(const int* sym, const int* idx, int B, int C, int H, int W, int parity, const int* cdfs,
                        int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf, int seg_rows,
                        unsigned char* out, long long out_cap, long long* offs, int chain, void* ws, long long ws_bytes,
                        hyres_stream_t s);
/* As hyres_wrans_decode for HRW2 strings that all have ``seg_rows`` rows per segment (validate every string with
 * hyres_wrans2_validate on the host first and compare the R it returns). Grid and loop bounds come from the shape and
 * seg_rows alone; reads are clamped to each string's end, to the directory's counts and to the tables. One kernel. */
int hyres_wrans2_decode(const unsigned char* strings, const long long* offs, const int* idx, int B, int C, int H, int W,
                        int parity, int seg_rows, const int* cdfs, int cdf_stride, const int* cdf_sizes,
                        const int* offsets, int ncdf, const float* params, int ldp, int M, int* sym_out,
                        hyres_stream_t s);
/* one HRW2 string of a [C,H,W] latent under ``parity``: magic, n, R >= 1 and S, a non-decreasing directory whose steps
 * fit their segments, the byte count (checked in this order); *seg_rows_out (may be NULL) receives R. HYRES_E_ARG with
 * the reason otherwise (host) */
int hyres_wrans2_validate(const unsigned char* in, long long in_len, int C, int H, int W, int parity,
                          int* seg_rows_out);
/* the same coder on host memory, one string; out == NULL: *out_len only. decode_host validates the string and takes
 * R from it. No GPU call (host) */
int hyres_wrans2_encode_host(const int* sym, const int* idx, int C, int H, int W, int parity, const int* cdfs,
                             int cdf_stride, const int* cdf_sizes, const int* offsets, int ncdf, int seg_rows,
                             unsigned char* out, long long out_cap, long long* out_len);
int hyres_wrans2_decode_host(const unsigned char* in, long long in_len, const int* idx, int C, int H, int W,
                             int parity, const int* cdfs, int cdf_stride, const int* cdf_sizes, const int* offsets,
                             int ncdf, const float* params, int ldp, int M, int* sym_out);

/* ------------------------------------------------------------------------------------------ */
/* JPEG 4:2:2 base layer: bit-exact with libjpeg-turbo at PyTurboJPEG's defaults */
/* ------------------------------------------------------------------------------------------ */
/* libjpeg's quality-scaled baseline quantisation tables (entries 1..255) in zigzag order, i.e. the two DQT
 * payloads of the file (host) */
int hyres_jpeg_quant_tables(int quality, unsigned char* lum64, unsigned char* chr64);
/* workspace of hyres_jpeg_roundtrip for a [B,3,H,W] batch (H % 8 == 0, W % 16 == 0), or -1 (host) */
long long hyres_jpeg_workspace_bytes(int B, int H, int W);
/* bytes one image's file can take at most: the 623-byte header, the entropy segment at the worst case of 1664
 * bits per 8x8 block with every byte stuffed, EOI; the minimum ``file_stride`` below (host) */
long long hyres_jpeg_stream_bytes(int H, int W);
/* Encode -> decode round trip of x [B,3,H,W] fp32 (channel 0 read as B; bytes = (clamp(x,0,1)*255) truncated):
 * decoded [B,3,H,W] fp32 = decoded byte / 255, sizes[b] = byte count of image b's file, and if files != NULL the
 * file itself at files + b * file_stride. All device pointers; kernels on ``s`` only — no host sync, allocation
 * or copy, so the call can be captured into a graph. */
int hyres_jpeg_roundtrip(const float* x, int B, int H, int W, int quality, float* decoded, int* sizes,
                         unsigned char* files, long long file_stride, void* ws, long long ws_bytes,
                         hyres_stream_t s);
/* the same round trip on host memory with the same arithmetic (csrc/jpeg_core.h); ws and s are ignored, no GPU
 * call is made (host) */
int hyres_jpeg_roundtrip_host(const float* x, int B, int H, int W, int quality, float* decoded, int* sizes,
                              unsigned char* files, long long file_stride, void* ws, long long ws_bytes,
                              hyres_stream_t s);

/* Decoding foreign 4:2:2 files on the device: a self-synchronising parallel Huffman decoder (csrc/jpeg_core.h),
 * bit-exact with libjpeg-turbo's decode. */
typedef struct hyres_jpeg_info {
    int supported;          /* 1: the device decoder takes the file */
    int H, W;               /* valid when supported */
    long long scan_off;     /* the entropy-coded segment inside the file: after the SOS header ... */
    long long scan_len;     /* ... up to the trailing EOI */
    unsigned char qtab[128]; /* luminance then chrominance quantiser, zigzag order (the DQT payloads) */
} hyres_jpeg_info;
/* Parses the marker segments of a JPEG file (host). supported = baseline SOF0, 8-bit, three components sampled
 * 2x1 / 1x1 / 1x1 in one interleaved scan (Ss = 0, Se = 63, Ah = Al = 0), no restart interval, 8-bit DQT tables of
 * any values, the four Annex K Huffman tables, H % 8 == 0 and W % 16 == 0; APPn / COM segments anywhere. Returns
 * HYRES_OK for every readable argument; when supported == 0, hyres_last_error_string() gives the reason. */
int hyres_jpeg_parse(const unsigned char* file, long long nbytes, hyres_jpeg_info* info);
/* workspace of hyres_jpeg_decode for B files of H x W whose entropy segments take at most scan_capacity bytes each
 * (1 <= scan_capacity < 2^28), valid for every sub_bits, or -1 (host) */
long long hyres_jpeg_decode_workspace_bytes(int B, int H, int W, long long scan_capacity);
/* Decodes B files of one size. scans: the raw (still stuffed) entropy segments, image b's at scans + scan_off[b],
 * scan_len[b] <= scan_capacity bytes; qtabs [B][2][64]: the files' quantisers in zigzag order; sub_bits: bits per
 * subsequence, a multiple of 32 in 32 .. 8192, 0 = the default; block_threads: threads of the work-group that
 * decodes one image, a multiple of 64 in 64 .. 1024, 0 = the default. decoded [B,3,H,W] fp32 = byte / 255 (channel
 * 0 = B); status[b] = 0 for a valid file, else bits 1 marker inside the segment, 2 invalid code or run past index
 * 63, 4 block count, 8 end position or padding, 16 segment longer than scan_capacity — the image's output is then
 * unspecified, every access stays inside the workspace; rounds (may be NULL): rounds[b] = sync rounds run, at
 * most the number of subsequences - 1. All device pointers; seven launches on ``s`` whose grids depend on
 * (B, H, W, scan_capacity, block_threads) alone — no host sync, allocation or copy: capture-legal. */
int hyres_jpeg_decode(const unsigned char* scans, const long long* scan_off, const int* scan_len,
                      const unsigned char* qtabs, int B, int H, int W, long long scan_capacity, int sub_bits,
                      int block_threads, float* decoded, int* status, int* rounds, void* ws, long long ws_bytes,
                      hyres_stream_t s);
/* the host twin: the same symbol step, rounds, write pass, DC scan and IDCT (csrc/jpeg_core.h) on host memory, a
 * plain loop over subsequences where the kernel has threads; decoded is zero-filled where status[b] != 0;
 * block_threads, ws and s are ignored, no GPU call is made (host) */
int hyres_jpeg_decode_host(const unsigned char* scans, const long long* scan_off, const int* scan_len,
                           const unsigned char* qtabs, int B, int H, int W, long long scan_capacity, int sub_bits,
                           int block_threads, float* decoded, int* status, int* rounds, void* ws, long long ws_bytes,
                           hyres_stream_t s);

/* Any H x W (1 <= H, W < 65536): the *_any twins of the entry points above take the same arguments and run the
 * same kernels with the same properties (device pointers, kernels on ``s`` only, no host sync, allocation or copy,
 * grids a function of the shape alone: capture-legal), for images that are not whole 16x8 MCUs as well, still
 * bit-exact with libjpeg-turbo. The file carries the true H x W in SOF0 and ceil(H/8) * ceil(W/16) MCUs of
 * Y0 Y1 Cb Cr. Encode: each component's last real row / sample is replicated down / to the right before the
 * transform (for chroma: before the h2v1 average); when ceil(W/8) is odd the last MCU's second luminance block is a
 * dummy block (AC zero, DC = the quantised DC of the block before it). Decode: every block of the scan is decoded
 * (status bit 4 counts the ragged grid), samples outside H x W are dropped, fancy upsampling puts its last-column
 * rule at chroma column ceil(W/2) - 1, and a chroma row of one or two samples (W <= 4) is replicated as libjpeg
 * does. The u8 planes and coefficients in the workspace have the padded extents; decoded [B,3,H,W] the true ones.
 * The strict entry points keep refusing such shapes and files; on whole MCUs both run the same code. */
long long hyres_jpeg_workspace_bytes_any(int B, int H, int W);
long long hyres_jpeg_stream_bytes_any(int H, int W);
int hyres_jpeg_roundtrip_any(const float* x, int B, int H, int W, int quality, float* decoded, int* sizes,
                             unsigned char* files, long long file_stride, void* ws, long long ws_bytes,
                             hyres_stream_t s);
int hyres_jpeg_roundtrip_any_host(const float* x, int B, int H, int W, int quality, float* decoded, int* sizes,
                                  unsigned char* files, long long file_stride, void* ws, long long ws_bytes,
                                  hyres_stream_t s);
int hyres_jpeg_parse_any(const unsigned char* file, long long nbytes, hyres_jpeg_info* info);
long long hyres_jpeg_decode_any_workspace_bytes(int B, int H, int W, long long scan_capacity);
int hyres_jpeg_decode_any(const unsigned char* scans, const long long* scan_off, const int* scan_len,
                          const unsigned char* qtabs, int B, int H, int W, long long scan_capacity, int sub_bits,
                          int block_threads, float* decoded, int* status, int* rounds, void* ws, long long ws_bytes,
                          hyres_stream_t s);
int hyres_jpeg_decode_any_host(const unsigned char* scans, const long long* scan_off, const int* scan_len,
                               const unsigned char* qtabs, int B, int H, int W, long long scan_capacity, int sub_bits,
                               int block_threads, float* decoded, int* status, int* rounds, void* ws,
                               long long ws_bytes, hyres_stream_t s);

/* ------------------------------------------------------------------------------------------ */
/* MS-SSIM / SSIM metric: pytorch_msssim's ms_ssim at its defaults (11-tap sigma-1.5 window, valid filtering,     */
/* K = (0.01, 0.03), 2x2 average pooling with padding side % 2 between levels)                                   */
/* ------------------------------------------------------------------------------------------ */
/* workspace of hyres_msssim for two [B,C,H,W] batches, or -1 on a bad shape (host) */
long long hyres_msssim_workspace_bytes(int B, int C, int H, int W, int levels);
/* x, y: contiguous NCHW fp32 on the device; 1 <= levels <= 5 and min(H, W) > 10 * 2^(levels - 1) (HYRES_E_SHAPE
 * otherwise); weights: ``levels`` floats on the HOST, passed to the kernel by value. out[b] = mean over c of
 * prod_l relu(m[l][b][c])^weights[l], where m is the spatial mean of cs_map for l < levels - 1 and of ssim_map for
 * the last level; per_level (may be NULL) receives m itself, [levels][B][C], before the relu — levels = 1 gives
 * plain SSIM. levels + 1 launches on ``s``; no host sync, allocation, copy, memset or atomic, every sum in a fixed
 * order: capture-legal, and the same input gives the same bits, alone or inside a batch. */
int hyres_msssim(const float* x, const float* y, int B, int C, int H, int W, int levels, const float* weights,
                 float data_range, float* out, float* per_level, void* ws, long long ws_bytes, hyres_stream_t s);
/* the same on host memory with the same arithmetic (csrc/msssim_core.h); ws and s are ignored, no GPU call is made
 * (host) */
int hyres_msssim_host(const float* x, const float* y, int B, int C, int H, int W, int levels, const float* weights,
                      float data_range, float* out, float* per_level, void* ws, long long ws_bytes,
                      hyres_stream_t s);
/* workspace of hyres_msssim_bwd, or -1 on a bad shape (host) */
long long hyres_msssim_bwd_workspace_bytes(int B, int C, int H, int W, int levels);
/* grad_y [B,C,H,W] = d (sum_b grad_out[b] * out[b]) / d y for the ``out`` of hyres_msssim on the same arguments;
 * grad_out: B floats on the device. The function is symmetric in x and y: the gradient towards x is the same call with
 * the two images swapped. Self-contained: it runs hyres_msssim's launches again into its own workspace, then one
 * small kernel and two kernels per level (3 * levels + 2 launches). A channel in which any level's mean is <= 0 gets
 * exactly 0. Gather only; no host sync, allocation, copy, memset or atomic, every sum in a fixed order: capture-legal,
 * and the same input gives the same bits, alone or inside a batch. */
int hyres_msssim_bwd(const float* x, const float* y, int B, int C, int H, int W, int levels, const float* weights,
                     float data_range, const float* grad_out, float* grad_y, void* ws, long long ws_bytes,
                     hyres_stream_t s);
/* the same on host memory with the same arithmetic; ws and s are ignored, no GPU call is made (host) */
int hyres_msssim_bwd_host(const float* x, const float* y, int B, int C, int H, int W, int levels,
                          const float* weights, float data_range, const float* grad_out, float* grad_y, void* ws,
                          long long ws_bytes, hyres_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* HYRES_HIP_H */
