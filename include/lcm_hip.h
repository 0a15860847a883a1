/*
 * lcm_hip.h -- C ABI of the MI355X (gfx950) LCM Stable-Diffusion-1.5 hot path.
 *
 * The reference has no FFI of its own: its hot path is one Python call,
 *   self.pipe(prompt=..., width=..., height=..., num_inference_steps=..., guidance_scale=..., generator=...)
 * at backends/cuda_worker.py:221-229 (diffusers StableDiffusionPipeline + LCMScheduler), behind the
 * PipelineWorker Protocol of backends/base.py:29-39.  This header is the boundary a maintainer binds
 * (ctypes stub in INTEGRATION.md) to replace the arithmetic under that call.  Each entry point names the
 * operator of the reference's op graph it replaces (diffusers module, reached from the call site above;
 * numpy twin of the glue in backends/rknnlcm.py where one exists).
 *
 * Conventions
 *   - all device pointers; activations are fp16 "pixel-major" (NHWC == [B*H*W, C] row major) unless stated;
 *     latents / noise / eps-state are fp32 NCHW (the request-side layout of backends/rknnlcm.py:424).
 *   - weights are fp16, row = output channel, k-contiguous; 3x3 weights are [Cout][ky][kx][Cin].
 *   - every function enqueues on `stream` (hipStream_t passed as void*), never synchronises, and
 *     returns 0 on success or a negative LCM_E* / positive hipError_t code; lcm_last_error() gives text.
 *   - nothing here allocates: callers own all buffers (graph-capture safe).
 */
#ifndef LCM_HIP_H
#define LCM_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LCM_OK 0
#define LCM_EINVAL (-1)   /* shape / alignment precondition violated */
#define LCM_ENODEV (-2)   /* no gfx950 device */
#define LCM_EUNSUPPORTED (-3)   /* a well-formed input of a kind the library leaves to another decoder (JPEG input) */

#define LCM_EPI_NONE 0
#define LCM_EPI_GEGLU 1   /* out[m][j] = x*gelu(g); weight rows interleaved x/g in blocks of 16 */
#define LCM_EPI_QUICK_GELU 2  /* x * sigmoid(1.702 x) after bias (CLIPMLP, hidden_act quick_gelu) */
#define LCM_EPI_GELU 3        /* exact gelu after bias */

const char* lcm_last_error(void);
int lcm_version(void);
/* device_count / arch string of device `dev` (buf >= 64 bytes) */
int lcm_device_info(int dev, char* arch_buf, int buf_len, int* cu_count, uint64_t* hbm_bytes);

/* ---- dense contraction (torch.nn.Linear / 1x1 Conv2d inside UNet2DConditionModel, AutoencoderKL) ----
 * out[z][m][n] = out_scale * sum_k A[z][m][k] * W[z][n][k]  (+bias[n]) (+rowadd[m / rows_per_batch][n]) (+res[m][n])
 * A may be split along k over two sources (fused torch.cat of the up-block skip: k < K1 from A, else A2).
 * Preconditions: K % 64 == 0, K1 % 64 == 0, N % 64 == 0 (N % 32 for GEGLU pairs), 16-byte aligned rows.
 */
int lcm_gemm_f16(const void* A, int lda, const void* A2, int lda2, int K1,
                 const void* W, const void* bias, const void* rowadd, int ld_rowadd, int rows_per_batch,
                 const void* res, int ldr, void* out, int ldo,
                 int M, int N, int K, int epilogue, float out_scale,
                 int batch, int64_t strideA, int64_t strideW, int64_t strideO, int img_rows,
                 void* stats_out, int64_t stats_bytes, int* slabs_per_image, void* stream);
/* img_rows = output rows PER IMAGE when the M rows stack several independent requests (M % img_rows == 0; 0: M is
 * one image).  It keys everything that decides the fp32 summation order (see "Determinism" below).
 *
 * Fused GroupNorm statistics (all three contraction entry points): stats_out != NULL asks the epilogue to also
 * write the per-channel (sum, sum of squares) of the fp16 values it stores, per CANONICAL 32-pixel slab of the
 * output (32 consecutive rows of a GEMM; a 2x16 -- 4x8 for images up to 16 wide -- pixel patch of a 3x3 convolution;
 * a split-K reduce slab): fp32 [B * slabs_per_image][N][2].  Slabs are a property of the output tensor, never of
 * the tile shape.  *slabs_per_image returns how many slabs each image got; 0 means the launch could not produce them
 * (img_rows % 32 != 0, GEGLU/batched launch, N > 2048): use lcm_groupnorm_f16 on the output instead.
 * Consumer: lcm_groupnorm_from_stats_f16.  stats_bytes = size of the buffer behind stats_out: a launch whose slabs would not
 * fit is refused with LCM_EINVAL BEFORE anything is enqueued (round 2 wrote past an undersized buffer: a GPU memory fault on
 * odd image sizes).  lcm_stats_bytes(M, N, img_rows) returns a size that always suffices. */
int64_t lcm_stats_bytes(int M, int N, int img_rows);

/* fp32 scratch for deterministic split-K (deep-K, small-M layers).  The caller owns the memory; it is
 * registered per current device and must outlive every later launch (graph replays included).  With no workspace
 * registered the library never splits (a deployment either registers one, always, or never: the pipeline always
 * does).  With one registered, a launch whose canonical K partition does not fit FAILS (LCM_EINVAL) -- it is never
 * silently run with fewer parts, because that would change the numbers.  bytes >= 4*splits*M*N of the largest split
 * layer (64 MiB covers SD1.5 at batch 1, 384 MiB batch 8). */
int lcm_set_workspace(void* ptr, int64_t bytes);
/* a workspace of its own for the launches of one stream: two sampler passes in flight on two streams ("lanes") must not share
 * split-K slabs.  Looked up before the device-wide workspace.  An entry is OWNED by the pointer that registered it:
 * (ptr, bytes > 0) registers -- LCM_EINVAL if the stream already carries another owner's workspace; (ptr, 0) forgets the entry
 * only if it still holds ptr; (NULL, 0) forgets it whoever owns it. */
int lcm_set_stream_workspace(void* stream, void* ptr, int64_t bytes);
/* a hipStream_t of the caller's own (hipStreamNonBlocking).  Frameworks hand streams out of small recycled pools (torch: 32 per
 * device), so two long-lived owners can end up keyed on one handle; a lane of the sampler takes its streams from here. */
int lcm_stream_create(void** stream_out);
int lcm_stream_destroy(void* stream);

/* launch heuristics of the contraction kernels (0 keeps a value): workgroups a split-K launch aims for, the
 * maximum number of K splits, and the workgroup count below which a larger tile is passed over.  These feed the
 * canonical-partition heuristic: changing them changes fp32 summation order for shapes without a plan entry. */
int lcm_set_tuning(int target_wgs, int max_splits, int min_wgs);
/* where the canonical K partition may have more than one part: images of at most `max_rows_per_image` output rows
 * (default 4096), at most `max_parts` parts (default 8).  A deployment-wide constant: it is part of what decides the
 * fp32 summation order. */
int lcm_set_split_policy(int max_rows_per_image, int max_parts);
/* How a launch whose canonical partition has several parts runs: split over workgroups + reduce launch (fp32 slabs), or
 * SEGMENTED in one workgroup (the parts accumulated separately and added in part order, in registers).  Same bits either
 * way; 0 (default) = segmented when the unsplit launch already fills the chip (batched requests), 1 = always segmented,
 * 2 = always split. */
int lcm_set_seg_mode(int mode);

/* Determinism.  The fp32 summation order of every output element is fixed by the K partition of its layer, and
 * that partition is a function of the PER-IMAGE problem only: (kind, rows per image, N, K[, output width]) ->
 * splits, from the plan entry of that per-image shape if one was set, else from a fixed heuristic.  Tile shape,
 * pipeline depth and kernel variant (the plan entry of the TOTAL shape, or the occupancy heuristic) never change a
 * bit of the result, and the fused statistics are slab-canonical.  Hence: same request + seed => same bytes, alone
 * or inside a batch of any size, in any process, under any tuning of tile / variant (the reference contract
 * tests/test_sdxl_worker.py:171-198, extended to micro-batches).
 *
 * Per-shape launch plans, normally loaded from the table shipped with the package (tuned offline): kind 0 =
 * lcm_gemm_f16 (aux = batch), 1 = row-gather conv (aux = 1), 2 = LDS-halo conv (aux = (W_out << 1) | has_gn).
 * bm in {64,128}, bn in {64,128,160}; variant as below (-1 = auto).  `splits` is honoured only through the entry
 * whose M equals the rows per image of a launch (it then IS that shape's canonical partition). */
int lcm_plan_set(int kind, int M, int N, int K, int aux, int bm, int bn, int splits, int variant);
int lcm_plan_clear(void);
/* the K partition a contraction of this per-image shape runs with (ph = 1: phase-decomposed upsample conv) */
int lcm_canonical_splits(int kind, int m_img, int N, int K, int aux, int ph);

/* Narrow tiles: a second, exact-shape table for batch-1 launches whose only real work is streaming weights (the 16^2 and
 * 8^2 UNet levels: 64 / 256 rows x 1280 channels put 80-200 workgroups on 256 CUs).  A 64 x 32 tile halves the weight
 * bytes each workgroup streams and doubles the workgroups.  Keys are those of the plan table, on the TOTAL shape of the
 * launch: kind 0 = (0, M, N, K, batch), kind 2 = (2, M, N, K, (W_out << 1) | has_gn).  Only bn = 32 with N % 32 == 0 is
 * accepted (LCM_EINVAL otherwise).  A hit replaces the tile width of the launch and nothing else -- the K partition, the
 * ring depth / taps per step and the statistics slabs are those of the wide launch, so results are bit-identical
 * (Determinism, above) -- and only where the launch is unbatched in z, has no GEGLU / activation epilogue, is not segmented
 * and not GroupNorm-fused; every other launch ignores the table.  The package installs narrow_plans_gfx950.json (shapes
 * measured faster cold on an MI355X, tools/make_narrow_plans.py) when the library is loaded; LCM_TUNED_PLANS=0 skips it. */
int lcm_narrow_set(int kind, int M, int N, int K, int aux, int bn);
int lcm_narrow_clear(void);
/* process-wide switch over the whole narrow table (A/B runs); default on */
int lcm_set_narrow_tiles(int on);

/* ---- LayerNorm -> Linear as one contraction (BasicTransformerBlock: norm1 -> attn1.to_q|k|v, norm2 -> attn2.to_q,
 * norm3 -> ff.net.0.proj) ----
 *   LN(x) W^T + b  =  rstd[m] * (sum_k x[m][k] W'[n][k] - mean[m] * ln_g[n]) + ln_c[n]
 * with W' = gamma (*) W in fp16, ln_g[n] = sum_k W'[n][k] and ln_c[n] = sum_k beta[k] W[n][k] + b[n] in fp32 (packed once
 * by the host).  The row statistics (sum, sum of squares over K, fp32) are accumulated from the A fragments while the
 * kernel walks K, so the normalisation costs no launch and no extra pass over the activations.  K is never split.
 * epilogue: LCM_EPI_NONE or LCM_EPI_GEGLU (ln_g / ln_c in the packed row order of W).  img_rows as lcm_gemm_f16. */
int lcm_gemm_ln_f16(const void* A, int lda, const void* W, const void* ln_g, const void* ln_c, float eps,
                    void* out, int ldo, int M, int N, int K, int epilogue, int img_rows, void* stream);

/* FeedForward of a BasicTransformerBlock in ONE launch:  out = x + Linear_2( GEGLU( Linear_1( LayerNorm(x) ) ) )
 * = lcm_gemm_ln_f16(epilogue GEGLU) followed by lcm_gemm_f16(bias b2, residual x), bit for bit, with the [M, 4C] intermediate
 * kept in registers (replaces diffusers' FeedForward(activation_fn="geglu") under norm3 and the residual add).
 * W1 [8C][C]: gamma (*) W of ff.net.0.proj, value / gate rows interleaved in blocks of 16; ln_g / ln_c [8C] fp32 as for
 * lcm_gemm_ln_f16; W2 [C][4C]: ff.net.2 with its columns in the stored order of the GEGLU output ("operand order": channel
 * 16 P + 4 q + j at column 32 (P >> 1) + 8 q + 4 (P & 1) + j -- the order in which lcm_gemm_*_f16's GEGLU epilogue stores it).
 * out may alias x (every workgroup reads and writes only its own 128 rows).  C = 320 only; a layer whose canonical K
 * partition of the second product has parts (img_rows small) is refused with LCM_EINVAL: use the two launches. */
int lcm_mlp_geglu_f16(const void* x, int ldx, const void* W1, const void* ln_g, const void* ln_c, float eps,
                      const void* W2, const void* b2, void* out, int ldo, int M, int C, int img_rows, void* stream);
/* refresh ln_g (= row sums of the live fp16 W') and ln_c (= c_base + alpha * c_delta; c_out / c_delta may be NULL) after
 * a style LoRA re-merged W' in place */
int lcm_ln_fold_refresh(const void* W, int N, int K, const void* c_base, const void* c_delta, float alpha,
                        void* g_out, void* c_out, void* stream);

/* 1: short-K GEMM launches with more tiles than the chip holds let each workgroup walk several n-tiles with a
 * continuous LDS-DMA pipeline (no ramp / drain per tile); 0 (default): one tile per workgroup.  Bit-identical. */
int lcm_set_persist_n(int on);

/* contraction kernel variant: 0 = register-staged double buffer, 2/3/4 = LDS-DMA pipeline with that many stages */
int lcm_set_kernel_variant(int variant);

/* tile shape the contraction kernels use for an [M x N] output (BM*1000 + BN); for profiling / docs */
int lcm_gemm_tile_config(int M, int N, int batch);

/* ---- 3x3 convolution, padding 1 (ResnetBlock2D.conv1/conv2, Downsample2D, Upsample2D.conv) ----
 * implicit GEMM over K = 9*Cin on MFMA; in: [B,Hin,Win,Cin]; stride 1|2; ups=1 reads the input through a
 * nearest-2x upsample (F.interpolate(scale_factor=2) fused into the loader).  ups=2 computes the same
 * Upsample2D (interpolate -> conv) as four 2x2 PHASE convolutions on the low-resolution input -- output pixel
 * (2y+py, 2x+px) only sees input rows {y-1+py, y+py} / columns {x-1+px, x+px} -- with W the phase-packed weights
 * [4 = py*2+px][Cout][2][2][Cin] (3x3 taps that land on one input pixel pre-summed): 16 instead of 36 multiply-adds
 * per output element and input channel.  Epilogue as lcm_gemm_f16.
 * Odd targets (Upsample2D called with output_size = an odd-sized skip: F.interpolate(size=(2h-1, 2w-1), nearest),
 * which is the 2x result minus its last row / column, then conv with ZERO padding of that cropped image): ups = 1 | 4
 * (output height 2*Hin-1) | 8 (output width 2*Win-1), with the plain 3x3 weights -- the pre-summed phase weights of
 * ups=2 do not hold for the border outputs, ups=2 with a crop flag is refused.
 * Preconditions: Cin % 64 == 0, Cout % 64 == 0.
 */
int lcm_conv3x3_f16(const void* in, const void* W, const void* bias,
                    const void* rowadd, int ld_rowadd, const void* res, void* out,
                    int B, int Hin, int Win, int Cin, int Cout, int stride, int ups,
                    void* stats_out, int64_t stats_bytes, int* slabs_per_image, void* stream);

/* ---- AutoencoderKL encoder Downsample2D: F.pad(x, (0, 1, 0, 1)) -> 3x3 convolution, stride 2, padding 0 ----
 * One zero row below / one zero column right of the image only: Ho = (Hin + 1 - 3) / 2 + 1, Wo likewise, and output (oy, ox)
 * reads input rows 2 oy .. 2 oy + 2.  (lcm_conv3x3_f16 with stride 2 pads symmetrically and is another function.)
 * in fp16 [B,Hin,Win,Cin], W fp16 [Cout][9][Cin], out fp16 [B,Ho,Wo,Cout]; bias only.  The row-gather implicit GEMM
 * (csrc/vae_enc.hip): the canonical K partition of the per-image shape (lcm_canonical_splits, kind 1: Determinism, above), run
 * as split launch + ordered reduce at every batch size; fused statistics per canonical 32-row slab as lcm_conv3x3_f16.
 * Preconditions: Cin % 64 == 0, Cout % 64 == 0, Hin >= 2, Win >= 2. */
int lcm_conv3x3_down_f16(const void* in, const void* W, const void* bias, void* out, int B, int Hin, int Win, int Cin, int Cout,
                         void* stats_out, int64_t stats_bytes, int* slabs_per_image, void* stream);

/* ---- fused GroupNorm(+SiLU) -> 3x3 convolution, stride 1 (ResnetBlock2D norm1->act->conv1, norm2->act->conv2) ----
 * LDS-halo implicit GEMM (csrc/conv_halo.hip).  Input = channel concat [in | in2] (in2 NULL: single source; fused
 * torch.cat of the skip).  gn_scale/gn_shift: fp32 [B][C1+C2] from lcm_groupnorm_affine_f16 (NULL: plain conv);
 * silu=1 applies SiLU after the affine; zero padding is applied AFTER the normalisation, as in the reference
 * graph.  ups=1 reads the (raw) input through a nearest-2x upsample; ups=2 as in lcm_conv3x3_f16 (gn_scale must be NULL).
 * Epilogue as lcm_gemm_f16.
 * Preconditions: C1, C2, Cout multiples of 64.
 */
int lcm_conv3x3_gn_f16(const void* in, int C1, const void* in2, int C2, const void* gn_scale, const void* gn_shift,
                       int silu, const void* W, const void* bias, const void* rowadd, int ld_rowadd, const void* res,
                       void* out, int B, int Hin, int Win, int Cout, int ups, void* stats_out, int64_t stats_bytes,
                       int* slabs_per_image, void* stream);
/* GroupNorm statistics folded into per-(image, channel) fp32 scale/shift tables [B][C1+C2] for the call above;
 * ws as for lcm_groupnorm_f16. */
int lcm_groupnorm_affine_f16(const void* x, int C1, const void* x2, int C2, const void* gamma, const void* beta,
                             void* scale_out, void* shift_out, int B, int HW, int groups, float eps, void* ws,
                             void* stream);
/* launches of the LDS-halo conv with fewer workgroups than this use its pipelined variant (3-stage weight ring,
 * double-buffered halo) instead of the single-buffer high-occupancy one; default 768 */
int lcm_set_halo_pipe_threshold(int wgs);
/* GroupNorm-fused convolution (lcm_conv3x3_gn_f16 with scale / shift): 1 = the raw halo of the next 64-channel chunk
 * is fetched into registers under the taps of the current one (measured slower: 202 VGPRs, two workgroups per CU instead of three), 0 (default) = fetched where it is consumed.  Bit-neutral. */
int lcm_set_halo_prefetch(int on);
/* bit 0 (default on): the LDS-halo convolution's plain (unsplit) launches with a residual fetch the residual tile by LDS-DMA and
 * store the result tile in whole rows through an LDS image of the tile; bit 1 (default off: measured neutral): plain GEMMs with a
 * residual too; 0: 8-byte pieces per lane everywhere.  Bit-neutral. */
int lcm_set_staged_epilogue(int on);
/* 1 (default): stride-1 3x3 convolutions use the LDS-halo kernel; 0: the row-gather implicit GEMM everywhere */
int lcm_set_conv_impl(int impl);

/* ---- 3x3 convolution from the fp32 NCHW latent (UNet conv_in; VAE post_quant_conv+decoder.conv_in) ----
 * in: fp32 [B,4,H,W]; optional pre-transform z = pre_w(4x4 fp32, row=out) * (in * in_scale) + pre_b
 * (AutoencoderKL: latents / scaling_factor -> post_quant_conv, backends/rknnlcm.py:614).
 * W: fp16 [Cout][9][4]; out: fp16 [B,H,W,Cout].  Cout % 16 == 0.  The fp32 input enters the MFMA as fp16 hi + fp16 lo parts
 * (two K slots per value against the same weight): input precision ~22 bits, fp32 accumulation.
 */
int lcm_conv3x3_c4_f32in(const void* in, const void* pre_w, const void* pre_b, float in_scale,
                         const void* W, const void* bias, void* out, int B, int H, int Wd, int Cout, void* stream);

/* The same with a residual: out = conv(in) + bias + res, res fp16 [B,H,W,Cout] added in fp32 before the one fp16 rounding
 * (ControlNet: conv_in(latents) + hint embedding).  No pre-transform. */
int lcm_conv3x3_c4_res_f32in(const void* in, const void* W, const void* bias, const void* res, void* out, int B, int H,
                             int Wd, int Cout, void* stream);

/* ---- ControlNet hint stack (ControlNetConditioningEmbedding): narrow 3x3 convolutions, csrc/controlnet.hip ----
 * lcm_hint_conv_u8: in uint8 RGB [B,H,W,3], x / 255 applied in the kernel and carried as fp16 hi + lo (~22 bits);
 *   W fp16 [Cout][9][3]; out fp16 [B,H,W,Cout]; Cout % 16 == 0.
 * lcm_hint_conv_f16: in fp16 [B,H,W,Cin], Cin in {16, 32, 96}; W fp16 [Cout][9][Cin]; out fp16 [B,Ho,Wo,Cout];
 *   stride 1 or 2 (padding 1: Ho = ceil(H / 2)); Cout % 16 == 0.
 * Both: fp32 accumulation in one chain per output (no K split: a pixel's bits depend on its own inputs only),
 * bias then optional SiLU in fp32, one fp16 rounding.  Any H, W >= 1. */
int lcm_hint_conv_u8(const void* in, const void* W, const void* bias, void* out, int B, int H, int Wd, int Cout, int silu,
                     void* stream);
int lcm_hint_conv_f16(const void* in, const void* W, const void* bias, void* out, int B, int H, int Wd, int Cin, int Cout,
                      int stride, int silu, void* stream);

/* ---- 3x3 convolution to a few channels (UNet conv_out -> eps; VAE decoder.conv_out -> RGB) ----
 * in: fp16 [B,H,W,Cin], W: fp16 [Cout][9][Cin], Cout <= 4, Cin % 8 == 0.
 * mode 0: out fp32 [B,H,W,Cout];  mode 1: out u8 [B,H,W,Cout] = rint(clamp(y/2+0.5,0,1)*255)
 * (VaeImageProcessor.postprocess; backends/rknnlcm.py:223,232-236,259); out_f32 optional float copy (NHWC).
 */
int lcm_conv3x3_smalln(const void* in, const void* W, const void* bias, void* out, void* out_f32,
                       int B, int H, int Wd, int Cin, int Cout, int mode, void* stream);
/* The same behind a fused GroupNorm-apply (+SiLU when silu != 0): in is the RAW tensor, gn_scale / gn_shift fp32 [B][Cin] the
 * tables of lcm_groupnorm_from_stats_f16 (out == NULL form) -- conv_norm_out -> SiLU -> conv_out of the UNet and of the
 * AutoencoderKL decoder without the normalised tensor in memory.  Cin % 64 == 0 (MFMA kernel; the choice of kernel depends on
 * Cin only).  gn_scale == NULL: identical to lcm_conv3x3_smalln. */
int lcm_conv3x3_smalln_gn(const void* in, const void* gn_scale, const void* gn_shift, int silu, const void* W,
                          const void* bias, void* out, void* out_f32, int B, int H, int Wd, int Cin, int Cout,
                          int mode, void* stream);

/* ---- GroupNorm (+SiLU) over [B,HW,C1(+C2)] (ResnetBlock2D.norm1/2, Transformer2DModel.norm, conv_norm_out) ----
 * x2 != NULL normalises the channel concatenation [x | x2] (fused torch.cat of the skip) and writes the
 * concatenated tensor.  ws: fp32 workspace of lcm_groupnorm_ws_bytes().  Deterministic (no atomics).
 */
int64_t lcm_groupnorm_ws_bytes(int B, int HW, int C, int groups);
int lcm_groupnorm_f16(const void* x, int C1, const void* x2, int C2, const void* gamma, const void* beta,
                      void* out, int B, int HW, int groups, float eps, int silu, void* ws, void* stream);

/* GroupNorm (+SiLU) of [x | x2] from producer-written statistics (see lcm_gemm_f16): stats1 = [B*P1][C1][2],
 * stats2 = [B*P2][C2][2] (x2/stats2 NULL: single source).  ws: >= 8*B*(C1+C2) bytes.  No pass over the data for
 * the statistics: one finalize launch (per image x group) + the apply launch.  out == NULL stops after the finalize
 * and leaves the folded per-(image, channel) fp32 tables in ws (scale [B][C1+C2], then shift [B][C1+C2]) for
 * lcm_conv3x3_gn_f16, which applies them while staging its input (x / x2 may then be NULL; C2 is taken as given). */
/* Tensors of at most this many bytes (default 8 MiB) run lcm_groupnorm_from_stats_f16 as ONE launch (each workgroup
 * re-derives its group's statistics, then applies its pixel slice): small-batch passes are launch-latency bound. */
int lcm_set_gn_fused_bytes(int64_t bytes);
int lcm_groupnorm_from_stats_f16(const void* x, int C1, const void* x2, int C2, const void* stats1, int P1,
                                 const void* stats2, int P2, const void* gamma, const void* beta, void* out,
                                 int B, int HW, int groups, float eps, int silu, void* ws, void* stream);

/* ---- LayerNorm over the last dim (BasicTransformerBlock.norm1/2/3) ---- */
int lcm_layernorm_f16(const void* x, const void* gamma, const void* beta, void* out, int M, int C, float eps,
                      void* stream);

/* ---- fused attention softmax(scale*Q K^T) V (Attention in BasicTransformerBlock.attn1/attn2) ----
 * Q: rows b*Sq+s, element (h*d + i) at Q[row*ldq + ...]; K,V likewise with Sk rows per batch; out [B*Sq][ldo].
 * d in {40, 64, 80, 160} (UNet / CLIP heads: 32x32x16-MFMA kernel, O for the whole head in registers) or, without causal
 * mask, d = 512 (AutoencoderKL mid-block attention, one head of 512: 16x16x32-MFMA kernel, 16 query rows per wave,
 * V^T fragments by ds_read_b64_tr_b16).  Online softmax in fp32, no S x S matrix in memory; a query row's result does not
 * depend on B or on the other rows.  scale > 0: the softmax scale (diffusers: d^-0.5).  scale <= 0: Q already carries
 * scale * log2(e) (the caller folded both into the projection that produced Q) and the logits are used as they are.
 */
int lcm_attention_f16(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* out, int ldo,
                      int B, int heads, int Sq, int Sk, int d, float scale, int causal, void* stream);
/* query rows per attention workgroup: 0 = by grid size, 4 = 128, 8 = 256 (streaming kernel only), 2 = 64 (register-staged
 * kernel only; measured slower at batch 1: every workgroup re-stages all K/V tiles).  Bit-neutral within a kernel. */
int lcm_set_attention_waves(int waves);
/* Which kernel serves the long non-causal sequences (Sk >= 128, d in {40, 64, 80}: the UNet's self-attention at the 64^2 / 32^2
 * levels, SDXL): 1 (default) = the streaming kernel (K/V tiles by LDS-DMA into a double buffer, Q pre-scaled, running max
 * carried in the padding k-slots of the QK^T MFMA for d = 40, deferred rescale), 0 = the register-staged kernel that serves
 * everything else.  Which kernel runs is a function of (d, Sk, causal) only -- never of B -- so a request's bits do not depend
 * on the batch; the two kernels differ in rounding (Q scaling in fp16, deferred max). */
int lcm_set_attention_impl(int impl);
/* 1 (default): self-attention over 1024..4096 keys splits the keys of a query block over two wave groups of the workgroup
 * (merged at the end; keyed on the sequence length alone, so batch-invariant); 0: never (A/B switch, changes those bits). */
int lcm_set_attention_ksplit(int on);
/* causal != 0: keys after the query are masked (CLIPTextModel's causal attention mask, transformers; the text
 * encoder call of the pipeline, twin backends/rknnlcm.py:266-367). */

/* ---- CLIPTextEmbeddings: out[b*S+s] = token_embedding[ids[b*S+s]] + position_embedding[s]; ids int32 ---- */
int lcm_embed_tokens_f16(const void* ids, const void* tok_emb, const void* pos_emb, void* out, int B, int S, int D,
                         int vocab, void* stream);

/* ---- prompt emphasis: per-token weights on the text encoder's output, chunk mean restored (csrc/prompt.hip) ----
 * z fp16 [n_chunks*S][D]: the encoder's output after the final LayerNorm, one 77-token chunk after the other; w fp32 [n_chunks*S]
 * (device): the weight of every token, 1.0 at BOS, EOS and padding.  Per chunk c, with sums over ALL S x D elements e of the chunk,
 *     S0 = sum z[e],   S1 = sum z[e] w[row(e)],   r = S1 != 0 ? S0 / S1 : 1      (= mean(z_c) / mean(z_c w): the counts cancel)
 *     out[(c S + s) ldo + i] = fp16( (float(z) * w[c S + s]) * r )               (two fp32 products, one rounding to fp16)
 * -- "Original" emphasis as written after A1111 (equality unverified), the mean taken per chunk of one request.  out rows have leading
 * dimension ldo >= D (a multiple of 8), so the chunks of a request land concatenated in their slot of a wider destination; columns
 * past D are not written.  S = 77, D in {768, 1024, 1280}; anything else is LCM_EINVAL.
 * Reduction order (fp32; fixed, so a chunk's bits depend on neither n_chunks nor its place in the launch).  One workgroup of 512
 * threads per chunk; the chunk's elements are numbered e = s D + i.  Thread t adds the elements 8 (t + 512 k) + j in the order
 * k = 0, 1, ... then j = 0 .. 7:  s0 <- s0 + z,  s1 <- fma(z, w, s1).  The 64 thread sums of a wave are combined by the xor butterfly
 * 32, 16, 8, 4, 2, 1 (v <- v + v[lane ^ o]), the 8 wave sums are then added in wave order 0 .. 7 starting from 0.  Both sums come
 * from ONE read of the chunk (it stays in registers for the scaling).  With all weights of a chunk exactly 1.0 every fma(z, 1, s1)
 * equals s0 + z, hence S1 == S0 bit for bit, r == 1 and out == z exactly; callers that know this on the host copy instead.
 * No host read-back: capturable. */
int lcm_prompt_emphasis_f16(const void* z, const void* w, void* out, int ldo, int n_chunks, int S, int D, void* stream);

/* ---- row softmax in place over [rows][n] fp16 (AutoencoderKL mid-block attention, d=512 single head) ---- */
int lcm_softmax_rows_f16(void* x, int rows, int n, int ld, void* stream);
/* ---- [z][R][C] -> [z][C][R] transpose, fp16 ---- */
int lcm_transpose_f16(const void* in, int ldi, void* out, int ldo, int R, int C, int batch,
                      int64_t stride_in, int64_t stride_out, void* stream);

/* ---- small-M linear (TimestepEmbedding, ResnetBlock2D.time_emb_proj): M <= 16 ----
 * out[m][n] = act_out( sum_k act_in(x[m][k]) W[n][k] + bias[n] + res[m][n] ), act = SiLU when flagged.
 */
int lcm_linear_smallm_f16(const void* x, int ldx, const void* W, const void* bias, const void* res, int ldr,
                          void* out, int ldo, int M, int N, int K, int silu_in, int silu_out, void* stream);
/* The same with any M and with x / res given for fewer rows than M: row m reads x[m % x_rows] and res[m % res_rows]
 * (the time-embedding MLP of all sampler steps in one launch per layer: rows step-major (step, image), the guidance embedding
 * and SDXL's added embedding given once per image).  A row's result does not depend on M. */
int lcm_linear_rows_f16(const void* x, int ldx, int x_rows, const void* W, const void* bias, const void* res, int ldr,
                        int res_rows, void* out, int ldo, int M, int N, int K, int silu_in, int silu_out, void* stream);

/* ---- Timesteps(flip_sin_to_cos=True, freq_shift=0): out fp16 [B][dim] = [cos | sin](t * f) ---- */
int lcm_timestep_embedding(float t, void* out, int B, int dim, void* stream);
/* nsteps <= 64 timesteps (host array) at once: out fp16 [nsteps][B][dim] */
int lcm_timestep_embedding_steps(const float* t_host, int nsteps, void* out, int B, int dim, void* stream);

/* ---- LCMScheduler.step (backends/rknnlcm.py:596-599), epsilon prediction, fp32 state ----
 * eps: fp32 NHWC [B,h,w,4] (conv_out); eps_uncond != NULL applies classifier-free guidance first.
 * lat (in/out): fp32 NCHW [B,4,h,w]; noise fp32 NCHW (ignored when last).  coef = {sqrt_alpha_t, sqrt_beta_t,
 * c_skip, c_out, sqrt_alpha_prev, sqrt_beta_prev}.
 */
int lcm_scheduler_step(const void* eps, const void* eps_uncond, float guidance, void* lat, const void* noise,
                       const float* coef6, int last, int B, int h, int w, void* stream);

/* The same step for any prediction type of the model output m (after CFG, applied to m exactly as above):
 *   LCM_PRED_EPSILON  x0 = (x - sqrt_beta_t m) / sqrt_alpha_t      (lcm_scheduler_step: identical kernel, identical bits)
 *   LCM_PRED_V        x0 = sqrt_alpha_t x - sqrt_beta_t m          (v-prediction: SD 2.x-768 and most SD2 fine-tunes)
 *   LCM_PRED_SAMPLE   x0 = m
 * then den = c_out x0 + c_skip x, and x <- last ? den : sqrt_alpha_prev den + sqrt_beta_prev noise (diffusers'
 * LCMScheduler.step).  Any other prediction_type returns LCM_EINVAL before anything is enqueued. */
#define LCM_PRED_EPSILON 0
#define LCM_PRED_V 1
#define LCM_PRED_SAMPLE 2
int lcm_scheduler_step_ex(const void* eps, const void* eps_uncond, float guidance, void* lat, const void* noise,
                          const float* coef6, int last, int prediction_type, int B, int h, int w, void* stream);

/* ---- multi-pass refinement in latent space ----
 * lat_out = fmaf(sqrt_b, noise, sqrt_a * x0) over fp32 NCHW [B,4,h,w] in one launch (16-byte accesses: every pointer 16-byte
 * aligned).  dup != 0: lat_out is [2B,4,h,w] and both halves (the two classifier-free-guidance rows of each request) get the
 * value.  Starts a chain from denoised latents of an earlier pass. */
int lcm_latents_renoise(const void* x0, const void* noise, float sqrt_a, float sqrt_b, void* lat_out, int B, int h, int w,
                        int dup, void* stream);
/* The last step of a pass that another pass follows, as one launch: den as lcm_scheduler_step_ex(last = 1) forms it (bit-equal),
 * stored to xk (fp32 NCHW [B,4,h,w]); lat <- fmaf(next_sqrt_b, noise, next_sqrt_a * den), the next pass's first state -- the
 * same bits lcm_latents_renoise gives for (xk, noise).  dup != 0: lat points at the second half of a [2B,4,h,w] state (as the
 * CFG call of lcm_scheduler_step_ex does) and the first half receives the same values.  coef6[4..5] are unused. */
int lcm_scheduler_step_handover(const void* eps, const void* eps_uncond, float guidance, void* lat, const void* noise, void* xk,
                                const float* coef6, float next_sqrt_a, float next_sqrt_b, int prediction_type, int B, int h, int w,
                                int dup, void* stream);

/* ---- samplers: Euler, Euler a, DDIM and DPM++ 2M as one step launch (csrc/sampler.hip, samplers.py) ----
 * Definitions.  abar[t] = alphas_cumprod[t], sigma[t] = sqrt((1 - abar[t]) / abar[t]) for t = 0..999.  For a noise level s:
 * sa(s) = 1 / sqrt(1 + s^2), sb(s) = s sa(s).  The sampler state is the variance-preserving one the UNet reads (with k-diffusion's
 * state X, x = sa(s) X): nothing scales the UNet's input.
 *   t_to_sigma(t), fractional t: linear in log sigma between floor(t) and ceil(t).  sigma_to_t(s): the inverse on the same table,
 *   the weight clipped to [0, 1].
 *   Schedules of n steps, both with s_n = 0 appended:  "normal"  s_i = t_to_sigma(t_i), t_i = linspace(999, 0, n), the UNet is
 *   evaluated at the fractional t_i;  "karras"  s_i = (smax^(1/7) + i/(n-1) (smin^(1/7) - smax^(1/7)))^7 with smax = sigma[999],
 *   smin = sigma[0] (n = 1: smax), the UNet is evaluated at t_i = sigma_to_t(s_i).
 *   Every step is x' = cx x + c0 x0 + c1 x0_prev + cn noise, then x0_prev <- x0, with m the model output after guidance and x0
 *   from m by the prediction type as lcm_scheduler_step_ex states it (sqrt_alpha_t = sa, sqrt_beta_t = sb).  With s = s_i,
 *   s' = s_(i+1), S = sa:
 *     Euler     cx = S(s') s' / (S(s) s), c0 = S(s') (1 - s'/s).
 *     Euler a   sup = min(s', sqrt(s'^2 (s^2 - s'^2) / s^2)), sdn = sqrt(s'^2 - sup^2): Euler towards sdn scaled by S(s'),
 *               cx = S(s') sdn / (S(s) s), c0 = S(s') (1 - sdn/s), cn = S(s') sup; the last step (s' = 0) is x' = x0, no noise.
 *     DPM++ 2M  h = ln s - ln s', e = -expm1(-h), cx = S(s') s' / (S(s) s); first step c0 = S(s') e; later steps with
 *               r = h_prev / h: c0 = S(s') e (1 + 1/(2r)), c1 = -S(s') e / (2r); the last step (s' = 0) is x' = x0.
 *     DDIM      diffusers' DDIMScheduler, eta 0, "leading" spacing, steps_offset 1: integer t_i = (n-1-i) (1000 / n) + 1,
 *               prev = t_i - 1000 / n (integer division; prev < 0 uses final_alpha_cumprod); cx = sb_prev / sb_t,
 *               c0 = sa_prev - sb_prev sa_t / sb_t.
 *   Initial state: x = noise sb(s_0) for Euler, Euler a and DPM++ 2M, x = noise for DDIM.
 *   These are written after the published formulas of k-diffusion, A1111 and diffusers; none of them was at hand to compare
 *   with, so equality with any of them is unverified.
 * lcm_sampler_step: eps / eps_uncond fp32 NHWC [B,h,w,4] (16-byte aligned; eps_uncond NULL: no guidance); lat fp32 NCHW
 * [B,4,h,w], updated in place; x0_prev fp32 NCHW [B,4,h,w], read only when c1 != 0 and always written; noise fp32 NCHW, read
 * only when cn != 0 (cn != 0 with noise NULL is LCM_EINVAL).  dup != 0: lat points at the second half of a [2B,4,h,w] state and
 * the first half receives the same values (as lcm_scheduler_step_handover).  Operation order per element, every operation
 * rounded to fp32 once (rn):
 *   m  = eps_uncond ? fma(guidance, eps - eps_uncond, eps_uncond) : eps
 *   x0 = epsilon: fma(-sb, m, x) / sa;  v: fma(-sb, m, sa * x);  sample: m
 *   r  = fma(cx, x, c0 * x0);  c1 != 0: r = fma(c1, x0_prev, r);  cn != 0: r = fma(cn, noise, r)
 * An element reads its own operands only: a request's bits depend neither on the batch size nor on its position.  A null or
 * misaligned pointer, a bad shape (B*4*h*w < 2^30) or an unknown prediction type returns LCM_EINVAL before anything is enqueued. */
int lcm_sampler_step(const void* eps, const void* eps_uncond, float guidance, void* lat, void* x0_prev, const void* noise, float sa,
                     float sb, float cx, float c0, float c1, float cn, int prediction_type, int B, int h, int w, int dup,
                     void* stream);

/* ---- hires fix: the hand-over between two sizes ----
 * lat_out = fmaf(sqrt_b, noise, sqrt_a * up(x0)) in one launch: x0 fp32 NCHW [B,4,h,w] (the denoised latents of the
 * low-resolution pass) is upscaled to [B,4,H,W] with one of A1111's latent upscalers and re-noised like lcm_latents_renoise.
 * All modes are torch.nn.functional.interpolate(..., align_corners=False, antialias=False):
 *   LCM_UPSCALE_BILINEAR       "Latent"                  bilinear, source coordinate clamped at 0
 *   LCM_UPSCALE_BICUBIC        "Latent (bicubic)"        bicubic, A = -0.75, indices clamped, coordinate not clamped
 *   LCM_UPSCALE_NEAREST_EXACT  "Latent (nearest-exact)"  source index floor((dst + 0.5) in / out)
 * A source coordinate is the exact rational ((2 dst + 1) in - out) / (2 out): integer floor, and a fraction that is one
 * correctly rounded fp32 division -- the weights depend on (dst, in, out) only (Determinism, above).  Taps of weight 0 are
 * left out, so H == h, W == w gives lcm_latents_renoise's bits.  x_up != NULL also receives up(x0) (fp32 [B,4,H,W]).
 * dup != 0: lat_out is [2B,4,H,W] and both halves get the value.  Any 1 <= h <= H <= 4h, 1 <= w <= W <= 4w with H, W <= 16384
 * and B*4*H*W < 2^30; no alignment requirement.  Anything else is LCM_EINVAL before anything is enqueued. */
#define LCM_UPSCALE_BILINEAR 0
#define LCM_UPSCALE_BICUBIC 1
#define LCM_UPSCALE_NEAREST_EXACT 2
int lcm_latents_upscale_renoise(const void* x0, int h, int w, const void* noise, float sqrt_a, float sqrt_b, int mode, void* x_up,
                                void* lat_out, int B, int H, int W, int dup, void* stream);

/* ---- image-to-image: the two ends of the AutoencoderKL encoder (csrc/vae_enc.hip) ----
 * lcm_vae_enc_conv_in_u8: encoder.conv_in from the picture.  in uint8 RGB [B,H,W,3]; x = 2 u8 / 255 - 1 is formed in the
 *   kernel and carried as fp16 hi + lo (~22 bits); the zero padding applies to x (a border pixel's neighbours are 0, not -1).
 *   W fp16 [Cout][9][3], out fp16 [B,H,W,Cout], Cout % 16 == 0 and <= 512; one fp32 chain per output, no K split; any H, W >= 1.
 * lcm_vae_posterior_renoise: pre_mean / pre_logvar fp32 [B,h,w,4] (rows 0..3 / 4..7 of encoder.conv_out), quant_w fp32 [8][8],
 *   quant_b fp32 [8], e0 / e1 fp32 [B,4,h,w].  moments = quant_w pre + quant_b (fp32);
 *   z = (mean + exp(0.5 clamp(logvar, -30, 20)) e0) scaling_factor -> z_out fp32 [B,4,h,w];
 *   lat_out = sqrt_a z + sqrt_b e1 (lcm_latents_renoise's expression); dup != 0: lat_out is [2B,4,h,w], both halves written;
 *   moments_out: optional fp32 [B,8,h,w].  B*8*h*w < 2^30. */
int lcm_vae_enc_conv_in_u8(const void* in, const void* W, const void* bias, void* out, int B, int H, int Wd, int Cout, void* stream);
int lcm_vae_posterior_renoise(const void* pre_mean, const void* pre_logvar, const void* quant_w, const void* quant_b,
                              const void* e0, const void* e1, float scaling_factor, float sqrt_a, float sqrt_b, void* z_out,
                              void* lat_out, void* moments_out, int B, int h, int w, int dup, void* stream);

/* ---- inpainting: the mask on the device, the masked step, the overlay (csrc/inpaint.hip) ----
 * Everything about the mask is integer arithmetic, so each result below is defined bit for bit.
 * lcm_inpaint_mask_prepare: mask uint8 [B,H,W] (255 = repaint) -> alpha uint8 [B,H,W] and, when latmask_out != NULL, the
 *   binary latent mask uint8 [B,H/8,W/8] (then H and W must be multiples of 8; alpha alone takes any H, W >= 1).
 *   Blur: weights_u32 is a DEVICE array of 2 radius + 1 uint32 that sum to exactly 65536 (the caller's Gaussian, centre tap
 *   last adjusted); t[y,x] = (sum_k w_k m[y, clamp(x + k - radius, 0, W - 1)] + 32768) >> 16 into scratch_u8 [B,H,W], then the
 *   same down the columns of t into alpha; uint32 sums (at most 255 * 65536 + 32768).  The edge is replicated, so a radius
 *   beyond the picture's side is fine; radius <= 80.  radius == 0: alpha = mask (a device copy, no blur launch; weights and
 *   scratch may be NULL).  Latent mask: M = 1 where 2 * (sum of the 8 x 8 block of alpha) >= 64 * 255, else 0.
 *   At most three launches.  Planes 8-byte aligned; B*H*W < 2^31.
 * lcm_scheduler_step_inpaint: one LCMScheduler.step and the select, one launch.  Arguments as lcm_scheduler_step_ex, plus
 *   z / e1 fp32 [B,4,h,w] (the init picture's clean latents and the re-noise draw) and latmask uint8 [B,h,w].  Per element
 *   lat <- latmask ? stepped : kept, where stepped has the bits lcm_scheduler_step_ex gives for the same operands (both the
 *   last and the non-last form) and kept = last ? z : the bits of lcm_latents_renoise(z, e1, next_sqrt_a, next_sqrt_b).
 *   noise and e1 may be NULL when last != 0.  dup != 0: lat points at the second half of a [2B,4,h,w] state and the first
 *   half receives the same values (as lcm_scheduler_step_handover).  eps / eps_uncond 16-byte aligned; B*4*h*w < 2^30.
 * lcm_inpaint_composite_rgb8: rgb <- (alpha rgb + (255 - alpha) init + 127) / 255 per pixel and channel, integer division,
 *   in place on rgb uint8 [B,H,W,3]; init uint8 [B,H,W,3], alpha uint8 [B,H,W].  alpha 255 keeps rgb, alpha 0 gives init,
 *   exactly.  Pointers 16-byte aligned; B*H*W*3 < 2^31.
 * Anything else is LCM_EINVAL before anything is enqueued. */
int lcm_inpaint_mask_prepare(const void* mask_u8, const void* weights_u32, int radius, void* alpha_u8_out, void* scratch_u8,
                             void* latmask_out, int B, int H, int W, void* stream);
int lcm_scheduler_step_inpaint(const void* eps, const void* eps_uncond, float guidance, void* lat, const void* noise, const void* z,
                               const void* e1, const void* latmask, const float* coef6, int last, float next_sqrt_a,
                               float next_sqrt_b, int prediction_type, int B, int h, int w, int dup, void* stream);
int lcm_inpaint_composite_rgb8(void* rgb_inout, const void* init_u8, const void* alpha_u8, int B, int H, int W, void* stream);

/* ---- ControlNet preprocessors: Canny edges and inversion (csrc/canny.hip, DESIGN.md sections 3 and 6) ----
 * The text below DEFINES the edge picture; all of it is int32 arithmetic, so every result is defined bit for bit.  It was
 * written to be OpenCV's cv2.Canny(rgb, low, high) on a three-channel picture with apertureSize = 3, L2gradient = False, as
 * recalled; equality with OpenCV is UNVERIFIED (OpenCV was not available to compare against).
 *   Input uint8 [B,H,W,3], output uint8 [B,H,W,3] with every pixel 0,0,0 or 255,255,255; B, H, W >= 1, B*H*W < 2^29.
 *   Thresholds: lo = floor(low), hi = floor(high), swapped if lo > hi.
 *   Gradients, per channel, borders replicated (p(y,x) with y, x clamped to the picture):
 *     dx = (p(y-1,x+1) - p(y-1,x-1)) + 2 (p(y,x+1) - p(y,x-1)) + (p(y+1,x+1) - p(y+1,x-1))
 *     dy = (p(y+1,x-1) - p(y-1,x-1)) + 2 (p(y+1,x) - p(y-1,x)) + (p(y+1,x+1) - p(y-1,x+1))
 *     n = |dx| + |dy|
 *   Channel pick: the channel with the largest n, the lowest channel index on a tie; its (dx, dy, m = n) are the pixel's.
 *   Non-maximum suppression, with m outside the picture 0 (not replicated).  Let x = |dx|, y = |dy| << 15, t22 = x * 13573,
 *   t67 = t22 + (x << 16).
 *     y < t22:  peak iff m > m(y,x-1) && m >= m(y,x+1)
 *     y > t67:  peak iff m > m(y-1,x) && m >= m(y+1,x)
 *     else:     s = ((dx ^ dy) < 0) ? -1 : 1;  peak iff m > m(y-1,x-s) && m > m(y+1,x+s)
 *   Class: 0 unless peak && m > lo; then 2 (strong) if m > hi, else 1 (weak).
 *   Linking: a pixel is an edge iff its class is > 0 and its 8-connected component of class > 0 pixels holds a class-2 pixel.
 *   Components never cross the pictures of a batch.
 * lcm_canny_ws_bytes: the device workspace a call needs (class map, labels, marks: 16-byte padded B*H*W + 8 B*H*W bytes); 0
 *   for a bad shape.
 * lcm_canny_classes_u8: picture -> class map uint8 [B,H,W]; lo / hi are the integer thresholds (swapped if lo > hi).  One launch.
 * lcm_canny_link: class map (any non-zero value other than 2 counts as weak) -> edge picture.  ws 16-byte aligned, ws_bytes >=
 *   lcm_canny_ws_bytes; cls may be the front of ws.  Exact for every input in FOUR launches whatever the content: tile-local
 *   union-find in LDS, a seam pass of integer atomic min over tile borders, a flatten pass that carries the strong marks to
 *   the roots, the picture.  No workgroup waits for another and nothing is read back.  The result does not depend on the
 *   order in which workgroups run.
 * lcm_canny_rgb8: both stages, five launches; out_rgb may be in_rgb (in place); neither may overlap ws.
 * lcm_invert_u8: out[i] = 255 - in[i] for n bytes (the "invert" preprocessor); in place allowed.  One launch.
 * Nothing allocates or synchronises; the calls are capturable.  Anything else is LCM_EINVAL before anything is enqueued. */
long long lcm_canny_ws_bytes(int B, int H, int W);
int lcm_canny_classes_u8(const void* in_rgb, void* cls_out, int B, int H, int W, int lo, int hi, void* stream);
int lcm_canny_link(const void* cls, void* out_rgb, void* ws, long long ws_bytes, int B, int H, int W, void* stream);
int lcm_canny_rgb8(const void* in_rgb, void* out_rgb, void* ws, long long ws_bytes, int B, int H, int W, float low, float high,
                   void* stream);
int lcm_invert_u8(const void* in, void* out, long long n, void* stream);

/* ---- variation seeds: subseed blend and seed-resize paste of the initial latents (csrc/variation.hip, DESIGN.md sections 3, 6) ----
 * The text below DEFINES the result.  It was written after A1111's create_random_tensors / slerp as recalled; equality with A1111
 * is UNVERIFIED, and two deviations are deliberate (below).
 *   lat0 fp32 [B][4][h][w]: the requests' initial latents (the target).  Slot b has a descriptor d = descs[b] (a HOST array of B,
 *   copied into the kernel's arguments: nothing of it is read after the call returns):
 *     active == 0: the slot is not touched and the other fields are not read.
 *     low, high fp32 [4][hs][ws] (device): the base noise and the subseed's noise at the SOURCE shape; t in [0, 1].
 *   Blend, per channel c and source column x, over the hs values down the HEIGHT axis (A1111's quirk, kept: the sphere is per
 *   column), all in fp32:
 *     S_ll = sum low^2,  S_hh = sum high^2,  S_lh = sum low high    -- each s <- fma(a, b, s) from 0 over y = 0, 1, ..., hs - 1
 *     d = S_lh / sqrt(S_ll * S_hh)
 *     if S_ll > 0 and S_hh > 0 and |d| <= 0.9995 (false for a NaN):   w = acos(d), so = sin(w),
 *         a = sin((1 - t) w) / so,  b = sin(t w) / so                 (IEEE division: b == 1 exactly at t == 1, a == 1 at t == 0)
 *     else  a = 1 - t,  b = t                                         (zero, parallel and antiparallel columns: linear)
 *     r[c][y][x] = fma(a, low[c][y][x], b * high[c][y][x])
 *   t == 0: nothing is blended and high is not read (may be NULL): r = low bit for bit.
 *   Deviations from A1111: it takes the linear branch for the WHOLE tensor on mean(d) > 0.9995, with the two weights swapped, and
 *   returns NaN for an exactly parallel column; here the rule is per column, the weights are the right way round and no finite
 *   input gives a NaN.
 *   Paste (seed-resize): r is centred into the slot.  dx = floor((w - ws) / 2), dy = floor((h - hs) / 2).  On an axis where the
 *   source is not larger, the whole of r lands at offset dx (dy); where it is larger, its window from -dx (-dy) of the target's
 *   size fills the whole axis.  The axes are independent.  The sums always run over ALL hs rows of the source column, also those
 *   the paste crops.  Cells of the slot outside the window keep their value.
 *   In place: low may be the slot itself (then hs == h and ws == w are required): every thread owns whole columns and has read a
 *   cell before it writes it.  Otherwise low and high must not overlap the slot.
 * One launch for the whole batch: one wave of 64 threads per (slot, 64 (channel, column) pairs); a thread walks its column twice
 * (sums, then blend), lanes are neighbouring columns, so loads coalesce across x.  No workgroup waits for another, no LDS.  A
 * column's bits depend on its own low, high and t only -- not on B, the slot, the lane or the other requests.
 * LCM_EINVAL before anything is enqueued: null lat0 / descs, B outside 1..8, h, w, hs or ws outside 1..256, t outside [0, 1] or NaN,
 * a null or non-4-byte-aligned low (or high with t > 0), a low that overlaps the slot without being it.  No active slot: LCM_OK
 * and no launch.  Nothing allocates or synchronises; capturable. */
typedef struct lcm_variation_desc {
    const void* low;           /* fp32 [4][hs][ws]; the slot itself for a blend in place */
    const void* high;          /* fp32 [4][hs][ws]; not read when t == 0 */
    int hs, ws;                /* source shape, 1..256 each */
    float t;                   /* subseed strength in [0, 1] */
    int active;                /* 0: the slot is left alone */
} lcm_variation_desc;
#define LCM_VARIATION_MAX_BATCH 8
int lcm_noise_variation_f32(void* lat0, int B, int h, int w, const lcm_variation_desc* descs, void* stream);

/* ---- Lanczos resampler: fitting an upload to the request's size (csrc/resize.hip, csrc/resize.cpp) ----
 * The text below DEFINES the fitted picture bit for bit.  It is PIL's ImagingResample for 8-bit pixels with the Lanczos filter:
 * Image.resize((out_w, out_h), Image.LANCZOS) of an "L" or "RGB" picture gives the same bytes (verified against Pillow 12.2.0 by
 * tests/test_resize_cpu.py and tests/test_resize_gpu.py; other Pillow versions are unverified).
 *   Tables, per axis with source size `in` and output size `out`, in IEEE double on the host, no fused or reordered operation:
 *     scale = in / out;  fs = max(scale, 1.0);  support = 3.0 * fs;  ksize = (int)ceil(support) * 2 + 1;  ss = 1.0 / fs
 *     for output xx:  center = (xx + 0.5) * scale
 *       xmin = max(0, (int)(center - support + 0.5));  xmax = min(in, (int)(center + support + 0.5));  n = xmax - xmin
 *       w[x] = L((x + xmin - center + 0.5) * ss) for x < n;  ww = the sum of w in index order;  w[x] /= ww if ww != 0
 *     L(x) = sinc(x) * sinc(x / 3) for -3 <= x < 3, else 0;  sinc(0) = 1, otherwise sinc(x) = sin(pi x) / (pi x), libm's sin
 *     k[x] = (int)(w[x] * 2^22 + 0.5) for w[x] >= 0, (int)(w[x] * 2^22 - 0.5) otherwise (truncation towards zero)
 *   One pass along an axis:  acc = 2^21 + sum_{x<n} pix[xmin + x] * k[x]  in int32 (|acc| < 2^31 always);
 *     out = clamp(acc >> 22, 0, 255), arithmetic shift.
 *   Order: the horizontal pass first, into a uint8 intermediate (rounded and clipped), then the vertical pass over it.  A pass
 *   whose axis keeps its size does not run (PIL skips it too; its table would be the identity).  Only the source rows the
 *   vertical tables read are resampled horizontally.
 *   Window: a call computes the w x h pixels at (x0, y0) of the full out_w x out_h grid and nothing else.  A window position
 *   outside the grid takes the nearest grid position on that axis (edge replication: the bands of "resize and fill").
 *   Domain: C = 1 or 3 interleaved channels; source sides 1..8192; output and window sides 1..4096; x0, y0 in -4096..4096.
 *   (Image.resize runs the vertical pass FIRST for height > 100 * width && out_h < height: callers that want PIL's bytes keep
 *   such pictures away from this path -- backends/hip_worker.resize does.)
 * Host-only, no device needed:
 *   lcm_resize_ksize: ksize of an axis;  lcm_resize_table_bytes: bytes of the table of n outputs of an axis, 16-byte padded:
 *     int32 [n][2] (xmin, taps), then int32 [n][ksize] coefficients, zero behind the taps;  0 for a bad axis.
 *   lcm_resize_tables: that table for outputs o0 .. o0 + n - 1 (each clamped to the grid) into host memory.
 *   lcm_resize_span: the source range [first, last) those outputs read;  lcm_resize_max_span: the most source pixels that `tile`
 *     neighbouring outputs read together.
 *   lcm_resize_passes: bit 0 the horizontal pass runs, bit 1 the vertical one (both sizes kept: the horizontal pass copies).
 *   lcm_resize_plan_table_bytes / lcm_resize_plan_tables: the tables of a whole call -- the horizontal pass's, then the vertical
 *     pass's, each only if it runs -- as the head of the workspace holds them.
 * lcm_resize_ws_bytes: the device workspace of a call: those tables, then the intermediate (16-byte padded); 0 for bad geometry.
 * lcm_resize_lanczos_u8: src uint8 [sh][sw][C] with row stride src_stride bytes -> the window into dst, rows dst_stride bytes
 *   apart (so a slot of a batch tensor is written in place).  The CALLER has put lcm_resize_plan_tables' bytes at the front of
 *   ws (16-byte aligned) on the same stream before the call.  At most one launch per pass; rows need no alignment; no
 *   workgroup waits for another; nothing allocates, synchronises or is read back; capturable.  src, dst and ws must not
 *   overlap.  Anything else is LCM_EINVAL before anything is enqueued. */
int lcm_resize_ksize(int in, int out);
long long lcm_resize_table_bytes(int in, int out, int n);
int lcm_resize_tables(int in, int out, int o0, int n, void* host_dst, long long dst_bytes);
int lcm_resize_span(int in, int out, int o0, int n, int* first, int* last);
int lcm_resize_max_span(int in, int out, int o0, int n, int tile);
int lcm_resize_passes(int sw, int sh, int out_w, int out_h);
long long lcm_resize_plan_table_bytes(int sw, int sh, int out_w, int out_h, int w, int h);
int lcm_resize_plan_tables(int sw, int sh, int out_w, int out_h, int x0, int y0, int w, int h, void* host_dst, long long dst_bytes);
long long lcm_resize_ws_bytes(int C, int sw, int sh, int out_w, int out_h, int x0, int y0, int w, int h);
int lcm_resize_lanczos_u8(const void* src, long long src_stride, int C, int sw, int sh, int out_w, int out_h, int x0, int y0, int w,
                          int h, void* dst, long long dst_stride, void* ws, long long ws_bytes, void* stream);

/* ---- tile grid combine: the overlapping tiles of an SD-upscale request blended into one picture (csrc/grid.hip, DESIGN.md
 * sections 3, 6; backends/sdupscale.py) ----
 * The text below DEFINES the result bit for bit.  It is A1111's combine_grid, that is PIL's paste with an "L" mask, per channel
 * byte (byte-equal to Pillow 12.2.0's paste in A1111's paste order at the geometries of tests/test_sdupscale_cpu.py; equality
 * with A1111 itself is UNVERIFIED).
 *   tiles_u8 uint8 [rows*cols][tile_h][tile_w][3], tile k = r * cols + c at offset (xs[c], ys[r]) of the picture;
 *   out_u8 uint8 [H][W][3].  The descriptor is read during the call only and travels in the kernel's arguments.
 *   m(i) = (255 * i) / overlap, integer division, for 0 <= i < overlap.
 *   blend(p, t, m) = DIV255(p * (255 - m) + t * m),  DIV255(a) = ((a + 128) + ((a + 128) >> 8)) >> 8.
 *   Row picture R_r(x, yy), 0 <= yy < tile_h: start at 0, then for c = 0 .. cols-1 in order, i = x - xs[c], t = tile (r, c) at (i, yy):
 *     c == 0: if x < tile_w the value becomes t;
 *     otherwise, if 0 <= i < overlap the value becomes blend(value, t, m(i));
 *     otherwise, if overlap <= i < tile_w the value becomes t.
 *   Output O(x, y): start at 0, then for r = 0 .. rows-1 in order, j = y - ys[r]:
 *     r == 0: if y < tile_h the value becomes R_0(x, y);
 *     otherwise, if 0 <= j < overlap the value becomes blend(value, R_r(x, j), m(j));
 *     otherwise, if overlap <= j < tile_h the value becomes R_r(x, j).
 *   overlap == 0: no blend region (A1111 divides by zero there: a stated deviation).
 *   The offsets of an axis obey four facts (v = xs, n = cols, tile = tile_w, size = W; likewise ys): v[0] == 0; v strictly
 *   increasing; v[k+1] - v[k] <= tile - overlap; v[n-1] + tile == size.  So every pixel lies under a tile's non-blend part and a
 *   pixel may lie under three or more tiles of an axis.
 * One launch, a pure gather: a thread owns four neighbouring pixels of one output row (dword stores where the row allows it), finds
 * the covering rows and columns from the by-value offsets and folds forward from the last non-blend cover.  No LDS, no atomics, no
 * workgroup waits for another; nothing allocates, synchronises or is read back; capturable.  tiles and out must not overlap.
 * LCM_EINVAL before anything is enqueued: null pointers; cols or rows outside 1..32; tile_w or tile_h outside 1..4096; W or H
 * outside tile..4096; overlap outside 0 .. min(tile_w, tile_h) - 1; xs / ys that break the four facts;
 * rows * cols * tile_h * tile_w * 3 >= 2^31. */
#define LCM_GRID_MAX_AXIS 32
typedef struct lcm_grid_desc {
    int W, H, tile_w, tile_h, overlap, cols, rows;
    int xs[LCM_GRID_MAX_AXIS];
    int ys[LCM_GRID_MAX_AXIS];
} lcm_grid_desc;
int lcm_grid_combine_rgb8(const void* tiles_u8, void* out_u8, const lcm_grid_desc* desc, void* stream);

/* ---- adaptive_avg_pool2d(lat,(8,8)) -> fp16 [B,4,8,8] (run_job_with_latents, backends/cuda_worker.py:299-304) */
int lcm_latents_pool8(const void* lat, void* out_f16, int B, int h, int w, void* stream);

/* Live per-launch timing of the MFMA kernels: between begin/end every contraction / attention launch is bracketed by
 * HIP events on its launch stream (main kernel only).  lcm_profile_end synchronises those events and writes one
 * "kernel instantiation<TAB>milliseconds" line per launch, in launch order; returns the number of lines. */
int lcm_profile_begin(int max_launches);
int lcm_profile_end(char* out, int64_t cap);
/* profiling aid: hold the stream busy for `usec` (<= 2 s) so queued launches run back to back */
int lcm_debug_spin(int usec, void* stream);
/* measurement only (tools/seam_cost.py): n_barriers grid-wide seams (release, one monotonic counter, bounded relaxed poll, acquire,
 * re-read of another workgroup's 128-byte record) inside ONE launch of `workgroups` <= 256 co-resident workgroups; state = device
 * memory of >= 16 + workgroups * 128 bytes (word 1 reads 1 afterwards if a spin gave up).  Never on the product path. */
int lcm_debug_grid_barrier(int workgroups, int n_barriers, void* state, void* stream);

/* ---- RGB8 -> PNG on the host (no GPU work): the ``img.save(buf, format="PNG")`` that closes run_job
 * (backends/cuda_worker.py:234-239).  rgb = `height` scanlines of `width` RGB8 pixels `pitch` bytes apart; the image is cut into
 * `stripes` deflate segments (dynamic Huffman over literals + distance-1 runs, filter "Up") compressed in parallel; the bytes
 * written depend on (image, stripes) only.  out must hold lcm_png_bound(width, height, stripes) bytes. */
long long lcm_png_bound(int width, int height, int stripes);
int lcm_png_encode_rgb8(const void* rgb, int width, int height, long long pitch, int stripes, void* out, long long out_cap,
                        long long* out_len);

/* ---- AutoencoderKL.tiled_decode glue (vae.enable_tiling(), backends/cuda_worker.py:91): decoded tiles are fp32
 * pixel-major [B,h,w,3].  blend: vertical=1 -> b[y] = a[ah-extent+y]*(1-y/extent) + b[y]*(y/extent) for y < extent (aw == bw);
 * vertical=0 -> the same along x (ah == bh).  place_tile: crop [0:ch, 0:cw] of a tile into the RGB8 image at (oy, ox) with
 * the (x/2+0.5).clamp * 255 -> rint conversion (optional fp32 copy). */
int lcm_vae_blend_f32(const void* a, int ah, int aw, void* b, int bh, int bw, int B, int extent, int vertical, void* stream);
int lcm_vae_place_tile(const void* tile, int th, int tw, void* out_u8, void* out_f32, int H, int W, int B,
                       int oy, int ox, int ch, int cw, void* stream);

/* ---- LoRA style merge: out = base + alpha * delta over n fp16 elements (n % 8 == 0); out may alias the live weight.
 * Replaces pipe.set_adapters([name],[weight]) / disable_lora() of backends/cuda_worker.py:165-196 (weights are
 * re-merged in place, so captured graphs stay valid). */
int lcm_axpy_f16(const void* base, const void* delta, float alpha, void* out, int64_t n, void* stream);

/* ---- super-resolution post-process (server/lcm_sr_server.py SuperResWorker, upscale_once): the ONNX model zoo's
 * super-resolution-10 (conv1 5x5 1->64, conv2 3x3 64->64, conv3 3x3 64->32, each + ReLU; conv4 3x3 32->r*r; pixel shuffle r;
 * r = 3 is the only factor the kernels implement) on the luma plane, plus PIL's bicubic xr of Cb / Cr and the merge.
 * Images are RGB8 [H][W][3], planes uint8 row major.  A pass cuts the W x H image into tile_w x tile_h tiles: x starts
 * min(i * tile_w, W - tile_w) for i < ceil(W / tile_w), y likewise, numbered row-major (y outer).  Each tile is an independent
 * network input, zero padded at ITS OWN border.  Tile activations are fp16 NHWC [T][tile_h][tile_w][C] for the T tiles
 * [t0, t0 + T) of the plan (any split of the plan into such chunks gives the same bits).  Weights are fp16: conv1 [25 taps][64],
 * conv2 / conv3 [Cout][ky][kx][Cin = 64], conv4 [ky][kx][Cin = 32][r*r]; biases fp32.
 *   conv1:          RGB8 -> Y = PIL's integer luma, fp16(Y / 255), conv1 + bias + ReLU -> [T][th][tw][64]
 *   conv3x3:        cout 64 (conv2) or 32 (conv3), 3x3 pad 1 per tile + bias + ReLU; in [T][th][tw][64]; 16-byte aligned
 *   conv4_shuffle:  y_out[r*gy + i][r*gx + j] = uint8(clip(255 * (conv4[i*r + j] + bias), 0, 255)) (truncation), written
 *                   only for the input pixels (gx, gy) the tile OWNS -- the tile with the largest covering x start and y
 *                   start, i.e. the one a row-major overwrite leaves on top -- so each of the rW x rH bytes is written
 *                   once by exactly one tile; y_out [rH][rW]
 *   chroma_h:       Cb / Cr of RGB8 (PIL's 6-bit tables, within 1 of PIL), PIL's 8-bit bicubic (a = -0.5) along x to rW
 *                   columns -> cbcr_h [H][rW][2] (uint8 as PIL keeps its intermediate)
 *   merge:          PIL's bicubic along y to rH rows of cbcr_h, merged with y_plane, YCbCr -> RGB8 (PIL's tables, within 1)
 *                   -> rgb_out [rH][rW][3] */
int lcm_sr_conv1(const void* rgb, int W, int H, int tile_w, int tile_h, int t0, int ntiles, const void* w1, const void* b1,
                 void* out, void* stream);
int lcm_sr_conv3x3(const void* in, int T, int th, int tw, int cout, const void* w, const void* bias, void* out, void* stream);
int lcm_sr_conv4_shuffle(const void* in, int W, int H, int tile_w, int tile_h, int t0, int ntiles, const void* w4,
                         const void* b4, int r, void* y_out, void* stream);
int lcm_sr_chroma_h(const void* rgb, int W, int H, int r, void* cbcr_h, void* stream);
int lcm_sr_merge(const void* y_plane, const void* cbcr_h, int W, int H, int r, void* rgb_out, void* stream);

/* ---- RGB8 -> baseline JPEG (the ``img.save(buf, format="JPEG", quality=q)`` of the super-resolution worker,
 * server/lcm_sr_server.py upscale_once): a device front end and a host entropy coder.  4:2:0, 16x16 MCUs, W, H in 1..65535.
 *   dct_rgb8 (device, one launch, capturable): rgb = H rows of W RGB8 pixels `pitch` bytes apart (any alignment) ->
 *     coefs int16 [ceil(H/16)][ceil(W/16)][6][64], blocks Y00 Y01 Y10 Y11 Cb Cr, each in zigzag order; coefs is 16-byte
 *     aligned and coefs_bytes >= lcm_jpeg_coef_bytes(W, H).  Arithmetic: libjpeg's 16-bit fixed point colour conversion
 *       Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *       Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *       Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 *     chroma = (a + b + c + d + bias) >> 2 over 2x2 with bias 1 for an even output column, 2 for an odd one; the last pixel /
 *     row replicated up to whole MCUs; level shift -128; fp32 8x8 DCT-II with JPEG normalisation (DC = sum / 8); multiply by
 *     the fp32 reciprocal of the table entry, round to nearest, clamp DC to +-2047 and AC to +-1023.
 *   quant_tables: out[0..63] luma, out[64..127] chroma, natural (row-major) order: the Annex K tables scaled as libjpeg's
 *     jpeg_set_quality(quality, force_baseline = TRUE) does; quality 1..100.
 *   encode_coefs (host, no GPU work): coefficients of that layout -> a JFIF file: SOI, APP0, two DQT, SOF0, four DHT (the
 *     Annex K tables), DRI, one interleaved scan, EOI.  The restart interval is one MCU row for every `threads` (rows are
 *     coded `threads` at a time on the pool the PNG writer owns), so the bytes depend on (coefs, W, H, quality) only.
 *     out_cap >= lcm_jpeg_bound(W, H).  A DC difference outside +-2047 or an AC value outside +-1023 is LCM_EINVAL. */
long long lcm_jpeg_coef_bytes(int W, int H);
long long lcm_jpeg_bound(int W, int H);
int lcm_jpeg_quant_tables(int quality, uint8_t* out);
int lcm_jpeg_dct_rgb8(const void* rgb, int W, int H, long long pitch, int quality, void* coefs, long long coefs_bytes,
                      void* stream);
int lcm_jpeg_encode_coefs(const void* coefs, int W, int H, int quality, int threads, void* out, long long out_cap,
                          long long* out_len);

/* ---- JPEG file -> RGB8 on the device (the ``Image.open(io.BytesIO(image_bytes)).convert("RGB")`` of the super-resolution
 * worker): a host marker parser and entropy decoder, and a device back end.  The pixels equal libjpeg-turbo's default decode
 * (PIL's) byte for byte.
 *   Supported: baseline and extended sequential Huffman (SOF0, SOF1), 8 bit, ONE interleaved scan, Y only (sampling 1x1) or
 *     Y Cb Cr with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1 (4:4:4, 4:2:2, 4:2:0), any DHT tables, with or without DRI;
 *     APPn / COM are skipped.  Everything else -- progressive, lossless, arithmetic coding, 12 bit, 4 components, 3 components
 *     that are not YCbCr (an Adobe marker whose transform is not 1; ids other than 1 2 3 without a JFIF marker), other sampling
 *     factors, several scans or a marker other than RSTn / EOI after the scan, 16-bit DQT, a height given by DNL -- returns
 *     LCM_EUNSUPPORTED: the caller gives the file to another decoder.  Malformed input is LCM_EINVAL.
 *   dec_info (host): fills lcm_jpeg_info from the markers; nothing is decoded.
 *   dec_coefs (host, no GPU work): Huffman-decodes the scan into
 *       coefs int16 [mcus_y][mcus_x][blocks_per_mcu][64]
 *     blocks in the order of the file (the luma blocks of the MCU row by row, then Cb, then Cr), every block in ZIGZAG order as
 *     stored -- for 4:2:0 exactly the layout of lcm_jpeg_dct_rgb8 / lcm_jpeg_encode_coefs, [my][mx][6][64] Y00 Y01 Y10 Y11 Cb Cr.
 *     An MCU is 8 hmax x 8 vmax pixels; grayscale is one block per MCU.  With a restart interval the intervals are found by
 *     scanning for FFD0..FFD7 and decoded `threads` at a time on the pool the PNG writer owns, DC prediction starting from 0 in
 *     each: the result does not depend on `threads`.  Without DRI the scan is one interval on one thread.  A bad code, a run
 *     past the end of a block, a missing / surplus / out-of-sequence RSTn, an interval that ends early or leaves a byte or more
 *     unread, no EOI, a DC value outside +-2047 or an AC value outside +-1023 are LCM_EINVAL.
 *   idct_rgb8 (device, two launches on `stream`, capturable; nothing is allocated or synchronised): coefs of that layout (16-byte
 *     aligned, coefs_bytes >= info->coefs_bytes) -> H rows of W RGB8 pixels `pitch` bytes apart at rgb_out (any alignment); only
 *     those 3 W bytes of a row are written.  work: 16-byte aligned device scratch of info->work_bytes (the sample planes between
 *     the launches).  Of info it reads width, height, ncomp, sampling and qt.  Arithmetic, all integer:
 *       dequantise: coefficient x table entry.  Inverse DCT: the "slow integer" 8x8 transform (Loeffler-Ligtenberg-Moschytz,
 *       13-bit constants FIX(x) = round(x * 8192): 0.298631336 0.390180644 0.541196100 0.765366865 0.899976223 1.175875602
 *       1.501321110 1.847759065 1.961570560 2.053119869 2.562915447 3.072711026), columns first with the result
 *       (x + 2^10) >> 11 (PASS1_BITS = 2 extra bits kept), then rows with (x + 2^17) >> 18, in 32-bit two's complement that
 *       wraps (it cannot for coefficients of 8-bit samples), arithmetic shifts; + 128; clamp to 0..255.
 *       Chroma of a 2x2 file ("fancy" upsampling; C = the component's own ceil(W/2) x ceil(H/2) samples, indices clamped to
 *       them): v[r][c] = 3 C[r >> 1][c] + C[(r >> 1) -+ 1][c] (- for even r, + for odd r); out[r][2c] = (3 v[r][c] + v[r][c-1] +
 *       8) >> 4, out[r][2c+1] = (3 v[r][c] + v[r][c+1] + 7) >> 4.  Of a 2x1 file: out[2c] = (3 C[c] + C[c-1] + 1) >> 2,
 *       out[2c+1] = (3 C[c] + C[c+1] + 2) >> 2, except that the first and the last output column are C[0] and C[last].  A
 *       component of one or two samples' width is replicated instead (out[r][x] = C[r >> 1][x >> 1], resp. C[r][x >> 1]).
 *       Colour, with b = Cb - 128, r = Cr - 128:  R = Y + ((91881 r + 32768) >> 16),  G = Y + ((-22554 b - 46802 r + 32768) >> 16),
 *       B = Y + ((116130 b + 32768) >> 16), clamped.  Grayscale: R = G = B = Y. */
typedef struct lcm_jpeg_info {
    int width, height;
    int ncomp;                 /* 1 (Y) or 3 (Y Cb Cr) */
    int sampling;              /* luma sampling: 0 = 1x1 (4:4:4 and grayscale), 1 = 2x1 (4:2:2), 2 = 2x2 (4:2:0) */
    int restart_interval;      /* MCUs per restart interval, 0 = none */
    int mcus_x, mcus_y;
    int blocks_per_mcu;        /* 1, 3, 4 or 6 */
    long long coefs_bytes;     /* mcus_y * mcus_x * blocks_per_mcu * 128 */
    long long work_bytes;      /* mcus_y * mcus_x * blocks_per_mcu * 64 */
    uint8_t qt[3][64];         /* quantisation table of every component, natural (row-major) order */
} lcm_jpeg_info;
int lcm_jpeg_dec_info(const void* data, long long len, lcm_jpeg_info* info);
int lcm_jpeg_dec_coefs(const void* data, long long len, int threads, void* coefs, long long coefs_bytes);
int lcm_jpeg_idct_rgb8(const void* coefs, long long coefs_bytes, const lcm_jpeg_info* info, void* work, long long work_bytes,
                       void* rgb_out, long long pitch, void* stream);

/* ---- hipGraph capture of the 4-step sampler loop + VAE ---- */
int lcm_graph_begin(void* stream);
int lcm_graph_end(void* stream, void** graph_exec_out);
int lcm_graph_launch(void* graph_exec, void* stream);
int lcm_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif
