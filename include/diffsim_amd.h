/*
 * diffsim_amd.h -- C ABI of the MI355X-native DiffSim scoring engine (libdiffsim_amd.so).
 *
 * The reference (showlab/DiffSim) has no FFI: its seam is Python.  These entry points are
 * what a binding for the reference's hot path would call; each cites the reference
 * interface it replaces.  Conventions:
 *   - plain pointers and sizes only; every tensor (including the workspace) is allocated
 *     by the caller (PyTorch-ROCm in the shipped wrapper) and passed as a device pointer;
 *   - the callee never allocates after dsim_unet_finalize(), never frees caller memory,
 *     never synchronises the stream and never throws: it returns 0 or a negative
 *     dsim_status code (dsim_strerror() gives the text);
 *   - one handle per device, one host thread per handle, re-entrant across handles (per-kernel launch attributes
 *     are cached per device, so handles on several devices may live in one process);
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).
 *
 * Layouts: activations are token-major ("NHWC"): [batch][pixel][channel].  Q/K/V leave the
 * engine as [batch][token][head*head_dim] -- the same memory the reference's non-contiguous
 * (B,H,N,D) views alias (diffsim/hacked_attn.py:74-77).
 */
#ifndef DIFFSIM_AMD_H
#define DIFFSIM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSIM_ABI_VERSION 7

typedef enum dsim_status {
    DSIM_OK = 0,
    DSIM_ERR_INVALID = -1,      /* bad argument / unsupported shape */
    DSIM_ERR_MISSING_WEIGHT = -2,
    DSIM_ERR_WORKSPACE = -3,    /* workspace too small */
    DSIM_ERR_HIP = -4,          /* a HIP runtime call failed */
    DSIM_ERR_STATE = -5,        /* call order violated (e.g. qkv before finalize) */
    DSIM_ERR_NO_DEVICE = -6
} dsim_status;

typedef enum dsim_dtype { DSIM_F32 = 0, DSIM_BF16 = 1, DSIM_F16 = 2 } dsim_dtype;

/* where the hooked attn1 sits: diffsim/diffsim.py:122-145
 *   DOWN: unet.down_blocks[:-1][layer]   MID: unet.mid_block   UP: unet.up_blocks[1:][layer]
 * always ...attentions[-1].transformer_blocks[-1].attn1                                   */
typedef enum dsim_tap_block { DSIM_TAP_DOWN = 0, DSIM_TAP_MID = 1, DSIM_TAP_UP = 2 } dsim_tap_block;

#define DSIM_MAX_LEVELS 4

/* Subset of diffusers' unet/config.json the path depends on. */
typedef struct dsim_unet_cfg {
    int32_t in_channels;                          /* 4 */
    int32_t n_levels;                             /* 4 */
    int32_t block_out_channels[DSIM_MAX_LEVELS];  /* 320,640,1280,1280 */
    int32_t down_has_attn[DSIM_MAX_LEVELS];       /* 1,1,1,0  (CrossAttnDownBlock2D vs DownBlock2D) */
    int32_t up_has_attn[DSIM_MAX_LEVELS];         /* 0,1,1,1 */
    int32_t layers_per_block;                     /* 2 */
    int32_t num_heads;                            /* 8 */
    int32_t cross_attention_dim;                  /* 768 */
    int32_t norm_num_groups;                      /* 32 */
    float   norm_eps;                             /* 1e-5 (ResnetBlock2D); Transformer2D GN uses 1e-6 */
    int32_t sample_size;                          /* latent side: 64 for 512 px */
    int32_t ctx_len;                              /* 77 */
    int32_t compute_dtype;                        /* dsim_dtype: DSIM_F32 (parity mode) or DSIM_BF16 */
    int32_t tap_block;                            /* dsim_tap_block */
    int32_t tap_layer;                            /* ABSOLUTE index into down_blocks / up_blocks (the wrapper
                                                     resolves the reference's slices: SD1.5 down[:-1]/up[1:],
                                                     SDXL down[1:]/up[:-1]); ignored for DSIM_TAP_MID */
    int32_t tap_attn;                             /* attention index inside the block, -1 = last (SD1.5) */
    int32_t tap_tfm;                              /* transformer_block index inside it, -1 = last (SD1.5) */
    /* SDXL deltas; zero = SD1.5 behaviour */
    int32_t heads_per_level[DSIM_MAX_LEVELS];     /* 5,10,20 ; 0 = num_heads everywhere */
    int32_t depth_per_level[DSIM_MAX_LEVELS];     /* transformer blocks per Transformer2DModel: 1,2,10 ; 0 = 1 */
    int32_t addition_embed;                       /* 1: "text_time" added conditioning (add_embedding.*) */
    int32_t addition_time_embed_dim;              /* 256 */
    int32_t pooled_dim;                           /* 1280 */
} dsim_unet_cfg;

typedef struct dsim_unet dsim_unet;

int         dsim_version(void);
const char* dsim_strerror(int status);
/* number of visible HIP devices (does not initialise a context beyond the count query) */
int         dsim_device_count(void);

/* ---- U-Net-to-tap engine: replaces DiffSimPipeline.step()'s `self.unet(...)` call
 *      (diffsim/diffsim_pipeline.py:213-221) plus the pre-hook that stashes q,k,v
 *      (diffsim/diffsim.py:43-56 -> diffsim/hacked_attn.py:61-77). ---------------------- */
int  dsim_unet_create(const dsim_unet_cfg* cfg, dsim_unet** out);
void dsim_unet_destroy(dsim_unet* h);

/* Hand one parameter over under its diffusers state-dict key (e.g.
 * "down_blocks.0.resnets.0.conv1.weight").  `dev_ptr` is borrowed until dsim_unet_finalize()
 * returns; src dtype may be f32, bf16 or f16; shape is the diffusers shape.  Parameters
 * that lie after the tap are accepted and ignored. */
int  dsim_unet_load_weight(dsim_unet* h, const char* key, const void* dev_ptr, int dtype,
                           const int64_t* shape, int ndim);
/* Repack every parameter up to the tap into the engine's own device buffers (conv weights
 * [Cout][3][3][Cin], fused QKV / KV, GEGLU-interleaved FF).  Allocates; synchronises `stream`. */
int  dsim_unet_finalize(dsim_unet* h, void* stream);
/* Diffusion timestep t (an actual timestep, not the reference's --target_step index; the
 * wrapper maps index -> t through the PNDM table, diffsim/diffsim_pipeline.py:153-157).
 * Pre-computes the time embedding and every ResnetBlock2D time_emb_proj (t is constant over a
 * run).  Enqueues on `stream`. */
int  dsim_unet_set_timestep(dsim_unet* h, int t, void* stream);
/* SDXL: timestep plus the added conditioning of DiffSimXLPipeline.step (diffsim/diffsim_xl_pipeline.py:231-262,
 * 312): text_embeds f32 device [2][pooled_dim] = [negative, positive] pooled prompt embeddings, time_ids f32
 * device [2][6] = (original_size, crop_top_left, target_size).  The two CFG halves get different time
 * embeddings; every ResnetBlock2D bias is prepared once per half. */
int  dsim_unet_set_conditioning(dsim_unet* h, int t, const float* text_embeds, const float* time_ids, void* stream);

/* Bytes of workspace one dsim_unet_qkv call over n_images needs; 0 when the call is impossible: handle not
 * finalized, or some activation of that batch would reach 2 GiB (tensors are addressed with 32-bit offsets) --
 * split the batch then. */
size_t dsim_unet_workspace_bytes(const dsim_unet* h, int n_images);

/* One noised U-Net forward to the tap for n_images latents, each duplicated for
 * classifier-free guidance ([uncond, cond], diffsim/diffsim_pipeline.py:208):
 *   latents, noise : f32 [n_images][C_in][s][s]  (NCHW, as the reference holds them)
 *   x_t = sqrt_abar*latents + sqrt_1m_abar*noise  (scheduler.add_noise, pipeline :177-183)
 *   ctx            : f32 [2][ctx_len][cross_attention_dim] = [uncond, cond] prompt embeddings
 *   q,k,v (out)    : compute_dtype [n_images][2][tokens][heads*head_dim]
 */
int  dsim_unet_qkv(dsim_unet* h, const float* latents, const float* noise, float sqrt_abar,
                   float sqrt_1m_abar, const float* ctx, int n_images, void* q, void* k, void* v,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Measurement aid (bench.py's roofline leg): while enabled, dsim_unet_qkv brackets every kernel
 * launch with a pair of HIP events recorded on the launch stream.  After the caller has
 * synchronised the stream, dsim_unet_profile_get returns, per launch: the kernel family name
 * (e.g. "gemm_bf16_256x160_conv3"), its ALGORITHMIC flops and bytes, and the elapsed ms.
 * dsim_unet_profile(h, enable) clears earlier records.  Not for use inside a timed region. */
int  dsim_unet_profile(dsim_unet* h, int enable);
int  dsim_unet_profile_count(const dsim_unet* h);
int  dsim_unet_profile_get(dsim_unet* h, int i, char* name, int name_cap, double* flops,
                           double* bytes, double* ms);

/* geometry of the tap for the current cfg: tokens, heads, head_dim */
int  dsim_unet_tap_shape(const dsim_unet* h, int* tokens, int* heads, int* head_dim);

/* Move the tap of a finalized handle (same meaning as the cfg fields of the same names): the packed weights are
 * shared by every tap, only the point where the walk stops changes -- one weight copy serves
 * --target_block/--target_layer sweeps (diffsim/diffsim.py:122-145, diffsim/diffsim_xl.py:88-107).
 * DSIM_ERR_MISSING_WEIGHT when a parameter needed before the new tap was never loaded (the old tap stays). */
int  dsim_unet_set_tap(dsim_unet* h, int tap_block, int tap_layer, int tap_attn, int tap_tfm);

/* ---- tap sweeps: the q,k,v of several taps from ONE forward --------------------------------------------------------
 * A tap named per call; the fields mean what the dsim_unet_cfg fields of the same names mean (block: dsim_tap_block,
 * layer: absolute block index, attn / tfm: -1 = the last). */
typedef struct dsim_tap { int32_t block, layer, attn, tfm; } dsim_tap;
/* geometry of `tap` (tokens, heads, head_dim) at the handle's current latent side; DSIM_ERR_INVALID for a tap the graph has not */
int    dsim_unet_tap_shape_at(const dsim_unet* h, const dsim_tap* tap, int* tokens, int* heads, int* head_dim);
/* Workspace of one dsim_unet_qkv_taps call: never more than the deepest tap's dsim_unet_workspace_bytes (the captures go to the
 * caller's tensors).  0 when the call is impossible: an invalid, duplicate or unloaded tap, or an activation or a tap output of
 * n_images that would reach 2 GiB. */
size_t dsim_unet_taps_workspace_bytes(const dsim_unet* h, int n_images, int n_taps, const dsim_tap* taps);
/* dsim_unet_qkv for n_taps taps (any order) in ONE walk to the deepest of them: q[i], k[i], v[i] receive what dsim_unet_qkv writes
 * with its tap at taps[i], bit for bit.  At each shallower tap the walk runs that block's norm1 and q/k/v projection as a walk that
 * stops there does (DSIM_FUSE_TAPQKV when q[i], k[i], v[i] lie at equal distances), then carries on exactly as a walk that passes
 * the block (its own projection into its own buffer).  The handle's tap is neither read nor moved; CFG de-duplication is off when
 * any tap lies in the first down block.  Checked before anything is enqueued: DSIM_ERR_INVALID for n_taps < 1, a duplicate or an
 * invalid tap, DSIM_ERR_MISSING_WEIGHT for a parameter missing before the deepest tap, DSIM_ERR_WORKSPACE for a short workspace.
 * Profile records (dsim_unet_profile) cover every launch of the call. */
int    dsim_unet_qkv_taps(dsim_unet* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar,
                          const float* ctx, int n_images, int n_taps, const dsim_tap* taps, void* const* q, void* const* k,
                          void* const* v, void* workspace, size_t workspace_bytes, void* stream);
/* Opt-in: compute what the two classifier-free-guidance halves share once.  The reference runs torch.cat([latents] * 2)
 * through the whole U-Net (diffsim_pipeline.py:208-221); conv_in, the first ResnetBlock2D and the first transformer up to its
 * cross-attention query see two bit-identical halves (one time embedding: SD1.5 graphs only; ignored for SDXL and when the tap
 * lies in the first down block).  Scores are bit-identical to the default; 6 % fewer FLOPs are executed. */
int  dsim_unet_set_cfg_dedup(dsim_unet* h, int enable);
/* Which multi-operator kernels replace their unfused chains (bf16 handles; default DSIM_FUSE_ALL).  0 runs every layer as its own
 * launch -- the A/B switch of bench.py --fusion and of the parity tests; results agree to bf16 rounding, not bit for bit.
 * DSIM_FUSE_FF: norm3 -> ff.net.0.proj (GEGLU) -> ff.net.2 -> + residual of a 320-channel BasicTransformerBlock as one launch
 * (hacked_modules.py:118-132).
 * DSIM_FUSE_LNPROJ: the normalisation in front of a projection runs inside the projection's row-resident launch, at 320 and 640
 * channels: the LayerNorm of a block's self-attention q/k/v projection (norm1 -> to_q|to_k|to_v) and of its cross-attention query
 * (norm2 -> attn2.to_q) (hacked_modules.py:88-116), and the Transformer2DModel's GroupNorm -> proj_in, whose GroupNorm then is a
 * statistics pass only (hacked_modules.py:336-339).  The 640-channel forms and the GroupNorm form engage where a level's map has
 * HW % 128 == 0 rows -- decided by the map size, never by the batch.
 * DSIM_FUSE_TAPQKV: the tapped layer's to_q / to_k / to_v (hacked_attn.py:61-69) as ONE N = 3C launch whose column runs go to the
 * three output tensors -- taken when q, k, v lie at equal distances in memory (one [3][...] allocation); bit-identical to the
 * three launches, any compute dtype. */
#define DSIM_FUSE_FF     1
#define DSIM_FUSE_LNPROJ 2
#define DSIM_FUSE_TAPQKV 4
#define DSIM_FUSE_ALL    7
int  dsim_unet_set_fusion(dsim_unet* h, int mask);
/* Latent side of the next dsim_unet_qkv calls (cfg.sample_size is only the default): the reference runs any
 * --image_size through the same weights (argprocess.py:8: default 512 px, SDXL native 1024 px).  `side` must be a
 * multiple of 2^(n_levels-1). */
int  dsim_unet_set_sample_size(dsim_unet* h, int side);

/* ---- many prompts in one forward: a context table ----------------------------------------------------------------------------
 * dsim_unet_qkv / dsim_unet_qkv_taps with one prompt per IMAGE instead of one per call:
 *   ctx       : f32 device [n_ctx][2][ctx_len][cross_attention_dim], n_ctx [uncond, cond] pairs
 *   ctx_index : int32 device [n_images], image i's row of ctx; values must lie in [0, n_ctx).  The index stays on the device (no
 *               check on the host side of the call); the gather kernel clamps every value into [0, n_ctx), so a bad index reads
 *               some row of the table, never memory outside it.  Not read when n_ctx == 1 (may be NULL then).
 * Batch element 2 i + cfg attends to ctx[ctx_index[i]][cfg].  Every cross-attention projects the K / V of each batch element's own
 * context (2 n_images ctx_len rows instead of 2 ctx_len) and attends per element; no other layer depends on the prompt.  Row for
 * row, the q / k / v are bit for bit those of a dsim_unet_qkv call whose ctx is that image's row.  n_ctx == 1 runs exactly the
 * launches of dsim_unet_qkv with ctx.  Checked before anything is enqueued: DSIM_ERR_INVALID for n_ctx < 1, a NULL ctx_index with
 * n_ctx > 1, or n_ctx > 1 on a handle with added conditioning (SDXL: the pooled prompt embedding enters every resnet through the
 * per-CFG-half time embedding), then what dsim_unet_qkv / dsim_unet_qkv_taps check. */
size_t dsim_unet_ctx_workspace_bytes(const dsim_unet* h, int n_images, int n_ctx);
size_t dsim_unet_taps_ctx_workspace_bytes(const dsim_unet* h, int n_images, int n_ctx, int n_taps, const dsim_tap* taps);
int    dsim_unet_qkv_ctx(dsim_unet* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar,
                         const float* ctx, int n_ctx, const int32_t* ctx_index, int n_images, void* q, void* k, void* v,
                         void* workspace, size_t workspace_bytes, void* stream);
int    dsim_unet_qkv_taps_ctx(dsim_unet* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar,
                              const float* ctx, int n_ctx, const int32_t* ctx_index, int n_images, int n_taps, const dsim_tap* taps,
                              void* const* q, void* const* k, void* const* v, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the tapped block's cross-attention operands: what the text attention maps are made of -----------------------------------
 * The reference declares `--use_text_attn`, "use the cross-attention results of text to guide conditional similarity"
 * (argprocess.py:17), and builds nothing behind it.  dsim_unet_qkv_text is dsim_unet_qkv_ctx on the handle's own tap whose walk does
 * not stop at the tap: the tapped BasicTransformerBlock runs on through its self-attention (on the captured q, k, v themselves),
 * attn1.to_out + residual, norm2 and attn2.to_q, and the block's attn2.to_k | to_v of the prompt context:
 *   q,k,v : as dsim_unet_qkv, bit for bit (the launches up to the tap are the same)
 *   xq    : dtype [2 n_images][tokens][heads*head_dim]: the cross-attention query of every batch element
 *   xkv   : dtype [n_kv][ctx_len][2*heads*head_dim], K in columns [0, C) and V in [C, 2C); n_kv = 2 ([uncond, cond]) when
 *           n_ctx == 1, 2 n_images (batch element e's own context in row e) with a context table
 * An image's rows do not depend on the other images of the call.  Checks, all before anything is enqueued: DSIM_ERR_INVALID for a
 * NULL xq or xkv, then what dsim_unet_qkv_ctx checks; DSIM_ERR_WORKSPACE below dsim_unet_text_workspace_bytes (0: an impossible
 * call, as its siblings).  SDXL handles take the call with n_ctx == 1. */
size_t dsim_unet_text_workspace_bytes(const dsim_unet* h, int n_images, int n_ctx);
int    dsim_unet_qkv_text(dsim_unet* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar,
                          const float* ctx, int n_ctx, const int32_t* ctx_index, int n_images, void* q, void* k, void* v,
                          void* xq, void* xkv, void* workspace, size_t workspace_bytes, void* stream);

/* ---- score tail: replaces diffsim/diffsim.py:177-197 (4x F.scaled_dot_product_attention,
 *      2x F.cosine_similarity or F.mse_loss, mean).  Fused: the O tensors never reach HBM. --
 *   q,k,v       : dtype [n_feat][B][N][H*D]   (features of n_feat images, B = CFG batch = 2)
 *   idx_a,idx_b : device int32 [n_pairs]; pair p scores image idx_a[p] against idx_b[p]
 *   similarity  : 0 cosine, 1 mse
 *   out_scores  : device f32 [n_pairs]
 */
size_t dsim_pair_score_workspace_bytes(int n_pairs, int B, int H, int N, int D);
int    dsim_pair_score(const void* q, const void* k, const void* v, const int32_t* idx_a,
                       const int32_t* idx_b, int n_pairs, int B, int H, int N, int D, int dtype,
                       int similarity, float* out_scores, void* workspace, size_t workspace_bytes,
                       void* stream);
/* The same call with a per-pair status: status[p] = 0 when score p is finite, 1 when it is NaN or infinite
 * (non-finite features: an overflowed activation or a corrupt weight; the reference would print the NaN and
 * count the triplet as wrong, cute_main.py:201-205).  status: device int32 [n_pairs]. */
int    dsim_pair_score_status(const void* q, const void* k, const void* v, const int32_t* idx_a,
                              const int32_t* idx_b, int n_pairs, int B, int H, int N, int D, int dtype,
                              int similarity, float* out_scores, int32_t* status, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- score matrix: every image of set A against every image of set B (retrieval: queries x gallery) --
 * out[a][b] is what dsim_pair_score returns for the pair (image a of set A, image b of set B), but each image's
 * self-attention O_ii = SDPA(Q_i, K_i, V_i) is computed once per call instead of once per pair: a cell costs the two
 * cross attentions, the self attentions cost n_a + n_b.  The sets are separate tensors, so a retained query set can be
 * scored against fresh gallery chunks without copying.
 *   qa,ka,va    : dtype [n_a][B][N][H*D]   (set A: the query images, 16-byte aligned)
 *   qb,kb,vb    : dtype [n_b][B][N][H*D]   (set B: the gallery images)
 *   similarity  : 0 cosine, 1 mse
 *   out         : device f32 [n_a][n_b]
 *   status      : NULL, or device int32 [n_a][n_b]: 1 where the score is NaN or infinite (as dsim_pair_score_status)
 * DSIM_ERR_INVALID for an unsupported shape or dtype, DSIM_ERR_WORKSPACE when workspace_bytes is short of
 * dsim_score_matrix_workspace_bytes (which returns 0 for an invalid shape).  Deterministic: a cell's value does not
 * depend on the other cells of the call. */
size_t dsim_score_matrix_workspace_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype);
int    dsim_score_matrix(const void* qa, const void* ka, const void* va, int n_a,
                         const void* qb, const void* kb, const void* vb, int n_b,
                         int B, int H, int N, int D, int dtype, int similarity,
                         float* out, int32_t* status, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- similarity maps: the score tail kept per query token ----------------------------------------------
 * The score of direction a->b breaks down over a's query tokens: cos(O_ab, O_aa) = sum_i dot_i / (|O_ab| |O_aa|), and
 * mse = sum_i sqd_i / (B H N D), where dot_i / sqd_i sum over the CFG batch, the heads and d at token i.
 *   q,k,v, idx_a, idx_b, similarity : as dsim_pair_score
 *   score       : device f32 [n_pairs], the pair's score (within float rounding of dsim_pair_score's)
 *   local       : NULL, or device f32 [n_pairs][2][N]: the token's own cosine of its O_ab and O_aa vectors (over B, H, D),
 *                 or their mean squared difference
 *   contrib     : NULL, or device f32 [n_pairs][2][N]: the token's term of the direction's score, so that
 *                 score[p] = 0.5 (sum_i contrib[p][0][i] + sum_i contrib[p][1][i])
 *   status      : NULL, or device int32 [n_pairs] (as dsim_pair_score_status)
 * Row [p][0] lies on image idx_a[p]'s token grid, row [p][1] on idx_b[p]'s.  Deterministic, and a pair's values do not
 * depend on the other pairs of the call.  dsim_pair_score_maps_workspace_bytes returns 0 for an invalid shape. */
size_t dsim_pair_score_maps_workspace_bytes(int n_pairs, int B, int H, int N, int D);
int    dsim_pair_score_maps(const void* q, const void* k, const void* v, const int32_t* idx_a,
                            const int32_t* idx_b, int n_pairs, int B, int H, int N, int D, int dtype,
                            int similarity, float* score, float* local, float* contrib, int32_t* status,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- token alignments: which token of the other image each token attends to -----------------------------
 * The score tail is built on the cross-attention of image A's queries over image B's keys; this call returns that attention.
 * For pair p and direction 0 (a = idx_a[p], b = idx_b[p]; direction 1 is the mirror, b's queries over a's keys):
 *   P_bh[i][j] = softmax_j(Q_a[b,h,i,:] . K_b[b,h,j,:] / sqrt(D)),   Pm[i][j] = mean of P_bh[i][j] over the B CFG halves and H heads.
 * Token j sits at row j / grid_w, column j % grid_w of its image's token grid.
 *   q,k         : dtype [n_feat][B][N][H*D], as dsim_pair_score (no v)
 *   grid_w      : width of the token grid; must divide N
 *   match       : NULL, or device int32 [n_pairs][2][N]: argmax_j Pm[i][j], ties to the lowest j
 *   weight      : NULL, or device f32 [n_pairs][2][N]: Pm[i][match]
 *   expect      : NULL, or device f32 [n_pairs][2][N][2]: sum_j Pm[i][j] (row_j, col_j), the soft-argmax position on the other grid
 *   attn        : NULL, or device f32 [n_pairs][2][N][N] (16-byte aligned when N % 4 == 0): Pm itself; below 2 GiB per call (chunk the pairs)
 *   status      : NULL, or device int32 [n_pairs]: 1 when any probability of the pair is non-finite (as dsim_pair_score_status)
 * Row [p][0] lies on image idx_a[p]'s token grid and points into idx_b[p]'s; row [p][1] the other way round.
 * The logits are computed from the stored q and k without rescaling q; the scale enters in f32 after the matrix product and
 * nothing is rounded to 16 bits on the way to Pm.  (dsim_pair_score's attentions pre-scale q and round it to the compute
 * dtype: its probabilities differ from these in the last bits.)  Deterministic, no atomics; a pair's values do not depend on the
 * other pairs of the call, and do not depend on which outputs are requested.  The workspace holds only the softmax statistics
 * per (pair, direction, b, h, row).  DSIM_ERR_INVALID (workspace query: 0) for an unsupported D, n_pairs < 1 or a grid_w that
 * does not divide N, and for an attn of 2 GiB or more; DSIM_ERR_WORKSPACE for a short workspace. */
size_t dsim_pair_align_workspace_bytes(int n_pairs, int B, int H, int N, int D);
int    dsim_pair_align(const void* q, const void* k, const int32_t* idx_a, const int32_t* idx_b, int n_pairs,
                       int B, int H, int N, int D, int dtype, int grid_w,
                       int32_t* match, float* weight, float* expect, float* attn, int32_t* status,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- region scores: the score restricted to a token region per image --------------------------------------
 * Every feature image i carries a token region R_i, a subset of its N tokens, given as a byte mask (non-zero = on).  The region
 * score of pair p (a = idx_a[p], b = idx_b[p]) is dsim_pair_score's tail applied to the sub-tensors Q_a[:, :, R_a, :], K_a[R_a],
 * V_a[R_a] and Q_b[R_b], K_b[R_b], V_b[R_b], rows in ascending token order:
 *   direction a->b: O_ab = SDPA(Q_a[R_a], K_b[R_b], V_b[R_b]),  O_aa = SDPA(Q_a[R_a], K_a[R_a], V_a[R_a]), both rounded to the
 *   pipeline dtype as dsim_pair_score rounds them; cosine over the flattened (B, H, |R_a|, D) tensors (eps 1e-8), or mse
 *   dividing by B H |R_a| D; direction b->a is the mirror over R_b; the score is the mean of the two directions.
 * The softmax scale stays 1/sqrt(D).  With every region full this is the pair score.  Off tokens are neither queries nor keys:
 * their rows are never read.
 *   q,k,v, idx_a, idx_b, similarity : as dsim_pair_score (index entries are not range-checked)
 *   mask        : device uint8 [n_feat][N]
 *   out_scores  : device f32 [n_pairs]
 *   status      : NULL, or device int32 [n_pairs]: 0, 1 where the score is NaN or infinite, 2 where a region of the pair is
 *                 empty (the score is then NaN; the other pairs of the call are not affected)
 *   counts      : NULL, or device int32 [n_feat]: |R_i|
 * Deterministic, no atomics.  A pair's value does not depend on the other pairs of the call, nor on anything outside its two
 * regions: not on the off tokens' features, and not on where in the image the region's rows lie.
 * DSIM_ERR_INVALID (workspace query: 0) for a bad dtype, similarity or head dim, n_pairs < 1, n_feat < 1, 2 n_pairs > 65535 or
 * B H > 65535; DSIM_ERR_WORKSPACE for a short workspace; both are decided on the host before anything is enqueued. */
size_t dsim_pair_score_regions_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);
int    dsim_pair_score_regions(const void* q, const void* k, const void* v, const uint8_t* mask /* [n_feat][N] */,
                               int n_feat, const int32_t* idx_a, const int32_t* idx_b, int n_pairs,
                               int B, int H, int N, int D, int dtype, int similarity,
                               float* out_scores, int32_t* status /* NULL or [n_pairs]: 0, 1 non-finite, 2 empty region */,
                               int32_t* counts /* NULL or [n_feat] */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- soft region scores: a weight per token instead of an on/off mask (additive to ABI v7) ---------------------------------------
 * Every feature image i carries a byte weight per token, m_i[t] in 0 .. 255, with w_i[t] = m_i[t] / 255.  For the direction a -> b,
 * with s(t, u) = Q_a[t] . K_x[u] / sqrt(D) per (CFG half, head):
 *   O_ab[t] = sum_u softmax_u( s(t,u) + ln w_b[u] ) V_b[u]        (a key of weight 0 takes part in no softmax)
 *   O_aa[t] = sum_u softmax_u( s(t,u) + ln w_a[u] ) V_a[u]
 * both rounded to the pipeline dtype exactly where dsim_pair_score and dsim_pair_score_regions round them;
 *   cosine: sum_t w_a[t] <O_ab[t], O_aa[t]> / max(sqrt(sum_t w_a[t] |O_ab[t]|^2) sqrt(sum_t w_a[t] |O_aa[t]|^2), eps), the sums also
 *           over both CFG halves, all heads and D, eps = 1e-8 under each norm as dsim_pair_score's;
 *   mse:    sum_t w_a[t] |O_ab[t] - O_aa[t]|^2 / (B H D sum_t w_a[t]), sum_t w_a[t] taken exactly as (sum of bytes) / 255;
 * the direction b -> a is the mirror and the score is the mean of the two.  The weights are fractional multiplicities: a token of
 * byte 2c is indistinguishable from two identical tokens of byte c.  With every byte 0 or 255 this is dsim_pair_score_regions on the
 * mask m != 0, bit for bit; with every byte 255 it is the pair score.  The biases are log2(m / 255) from a 256-entry f32 table
 * built in double and rounded once (entry 255 is 0.0f), added to the logits in f32 before the softmax; a query row's f32 sums are
 * multiplied by (float)m / 255.0f.
 *   q,k,v, idx_a, idx_b, similarity : as dsim_pair_score (index entries are not range-checked)
 *   weights     : device uint8 [n_feat][N]
 *   out_scores  : device f32 [n_pairs]
 *   status      : NULL, or device int32 [n_pairs]: 0, 1 where the score is NaN or infinite, 2 where an image of the pair has byte
 *                 sum 0 (the score is then NaN; the other pairs of the call are not affected)
 *   weight_sums : NULL, or device int32 [n_feat]: the images' byte sums
 * Deterministic, no atomics.  A pair's value depends on its two images and their weights alone; rows of weight 0 are never read.
 * Refusals as dsim_pair_score_regions, and N >= 2^31 / 255: DSIM_ERR_INVALID (workspace query: 0) or DSIM_ERR_WORKSPACE, decided on
 * the host before anything is enqueued. */
size_t dsim_pair_score_weights_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);
int    dsim_pair_score_weights(const void* q, const void* k, const void* v, const uint8_t* weights /* [n_feat][N] */,
                               int n_feat, const int32_t* idx_a, const int32_t* idx_b, int n_pairs,
                               int B, int H, int N, int D, int dtype, int similarity,
                               float* out_scores, int32_t* status /* NULL or [n_pairs]: 0, 1 non-finite, 2 zero weight */,
                               int32_t* weight_sums /* NULL or [n_feat] */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- region score matrices: every masked query image against every masked gallery image -------------------------------------------
 * Set A has n_a feature images and set B has n_b (q, k, v of a set: [n][B][N][H*D], as dsim_score_matrix); each image carries a
 * byte mask [N] (non-zero = on) with region R_i.  Cell (i, j) is exactly the region score of the pair (A_i, B_j) as
 * dsim_pair_score_regions defines it: rows in ascending token order, both SDPAs over the regions' rows only, outputs rounded to the
 * pipeline dtype, cosine with F.cosine_similarity's eps or mse divided by B H |R_query| D, the mean of the two directions.  Each
 * image's self-attention over its region is computed once; a cell costs one attention per direction.
 * With all masks full it is dsim_score_matrix's cell.  A cell with an empty region on either side is NaN with status 2, and no
 * other cell is disturbed.  Rows outside a region are never read.
 *   out         : device f32 [n_a][n_b]
 *   status      : NULL, or device int32 [n_a][n_b]: 0, 1 where the score is NaN or infinite, 2 where a region of the cell is empty
 *   counts      : NULL, or device int32 [n_a + n_b]: |R_i| of set A's images, then of set B's
 * Deterministic, no atomics; a cell depends on its two images and their regions alone.
 * DSIM_ERR_INVALID (workspace query: 0) for a bad dtype, similarity or head dim, n_a < 1 or n_b < 1, n_a + n_b > 65535,
 * B H > 65535, ceil(N/128) n_a n_b 2 >= 2^31, or any tensor or list of 2^31 elements or more; DSIM_ERR_WORKSPACE for a short
 * workspace; both are decided on the host before anything is enqueued. */
size_t dsim_score_matrix_regions_workspace_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype);
int    dsim_score_matrix_regions(const void* qa, const void* ka, const void* va, const uint8_t* mask_a, int n_a,
                                 const void* qb, const void* kb, const void* vb, const uint8_t* mask_b, int n_b,
                                 int B, int H, int N, int D, int dtype, int similarity,
                                 float* out /* [n_a][n_b] */, int32_t* status /* NULL or [n_a][n_b]: 0 | 1 | 2 */,
                                 int32_t* counts /* NULL or [n_a + n_b] */,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- soft score matrices: every weighted query image against every weighted gallery image (additive to ABI v7) -------------------
 * dsim_score_matrix_regions with weight bytes for the masks: set A's images carry weights_a [n_a][N], set B's weights_b [n_b][N],
 * w = byte / 255.  Cell (i, j) is dsim_pair_score_weights of the pair (A_i, B_j), bit for bit, in every dtype and at every head
 * dim: tokens of byte 0 are dropped, every softmax carries the key image's biases log2(byte / 255) (the same 256-entry table), a
 * query row's f32 sums are multiplied by (float)byte / 255.0f, and the mse count of a direction is B H D (byte sum) / 255 in f64.
 * Each image's self-attention (with its own biases) is computed once; a cell costs one attention per direction.
 * With bytes 0 / 255 only the cell is dsim_score_matrix_regions' on m != 0, bit for bit; with every byte 255 dsim_score_matrix's
 * tiled cell.  A cell with an image of byte sum 0 is NaN with status 2, and no other cell is disturbed.
 *   out         : device f32 [n_a][n_b]
 *   status      : NULL, or device int32 [n_a][n_b]: 0, 1 where the score is NaN or infinite, 2 where an image of the cell has byte sum 0
 *   weight_sums : NULL, or device int32 [n_a + n_b]: the byte sums of set A's images, then of set B's
 * Deterministic, no atomics; a cell depends on its two images and their weights alone; rows of weight 0 are never read.
 * Refusals as dsim_score_matrix_regions, and N 255 >= 2^31 or (n_a + n_b) (N rounded up to 64) >= 2^31: DSIM_ERR_INVALID (workspace
 * query: 0) or DSIM_ERR_WORKSPACE, decided on the host before anything is enqueued. */
size_t dsim_score_matrix_weights_workspace_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype);
int    dsim_score_matrix_weights(const void* qa, const void* ka, const void* va, const uint8_t* weights_a, int n_a,
                                 const void* qb, const void* kb, const void* vb, const uint8_t* weights_b, int n_b,
                                 int B, int H, int N, int D, int dtype, int similarity,
                                 float* out /* [n_a][n_b] */, int32_t* status /* NULL or [n_a][n_b]: 0 | 1 | 2 */,
                                 int32_t* weight_sums /* NULL or [n_a + n_b] */,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- region maps: the region score per query token (additive to ABI v7) ---------------------------------------------------------
 * dsim_pair_score_maps for dsim_pair_score_regions: the region tail's own attentions, rounding and products, kept per query token.
 * Outputs lie on the full token grid.  For direction 0 (image idx_a[p] over idx_b[p]; direction 1 the mirror) and an on token i:
 * local[p][0][i] is the token's own cosine (or its mean squared difference over the B H D values) and contrib[p][0][i] its term of
 * the direction's value, so that 0.5 (sum contrib[p][0] + sum contrib[p][1]) is the pair's region score; the mse count of a direction
 * is B H D times the query image's own |R|.  Off tokens: local = contrib = 0 exactly (the caller holds the mask).
 *   q,k,v, mask, idx_a, idx_b, similarity, counts : as dsim_pair_score_regions
 *   score       : device f32 [n_pairs]
 *   local, contrib : NULL, or device f32 [n_pairs][2][N] each
 *   status      : NULL, or device int32 [n_pairs]: 0, 1 where the score is NaN or infinite, 2 where a region of the pair is empty
 *                 (score NaN, both maps all zero; the other pairs of the call are not affected)
 * With every region full the outputs are dsim_pair_score_maps' bits.  Deterministic, no atomics; rows outside a region are never
 * read.  Refusals as dsim_pair_score_regions, and n_feat N >= 2^31. */
size_t dsim_pair_score_maps_regions_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);
int    dsim_pair_score_maps_regions(const void* q, const void* k, const void* v, const uint8_t* mask /* [n_feat][N] */,
                                    int n_feat, const int32_t* idx_a, const int32_t* idx_b, int n_pairs,
                                    int B, int H, int N, int D, int dtype, int similarity,
                                    float* score, float* local, float* contrib,
                                    int32_t* status /* NULL or [n_pairs]: 0, 1 non-finite, 2 empty region */,
                                    int32_t* counts /* NULL or [n_feat] */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- region alignments: the cross-attention of one region over the other (additive to ABI v7) -------------------------------------
 * dsim_pair_align with the background out of the softmax.  For direction a->b and query token i in R_a,
 * Pm[i][j] = softmax over j in R_b ONLY of Q_a[i] . K_b[j] / sqrt(D), averaged over the B CFG halves and the H heads (dsim_pair_align's
 * arithmetic on the regions' rows in ascending token order).  Outputs lie on the full grid; for an on query token i:
 *   match  [n_pairs][2][N] int32 : argmax over j in R_b, as the token index on b's full grid (ties: the lowest j)
 *   weight [n_pairs][2][N] f32   : that probability
 *   expect [n_pairs][2][N][2] f32: sum_j Pm[i][j] (j / grid_w, j % grid_w), full-grid coordinates
 *   attn   [n_pairs][2][N][N] f32: Pm, zero outside R_a x R_b; fewer than 2 GiB per call
 * each of which may be NULL.  Off query tokens: match -1, weight 0, expect (-1, -1).
 *   status      : NULL, or device int32 [n_pairs]: 0, 1 where a probability is non-finite, 2 where a region of the pair is empty
 *                 (every row of the pair then carries the off values)
 *   counts      : NULL, or device int32 [n_feat]: |R_i|
 * With every region full the outputs are dsim_pair_align's bits.  Deterministic, no atomics; rows outside a region are never read.
 * Refusals as dsim_pair_align (N % grid_w, an attn of 2 GiB or more) and dsim_pair_score_regions (n_feat < 1, n_feat N >= 2^31). */
size_t dsim_pair_align_regions_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);
int    dsim_pair_align_regions(const void* q, const void* k, const uint8_t* mask /* [n_feat][N] */, int n_feat,
                               const int32_t* idx_a, const int32_t* idx_b, int n_pairs,
                               int B, int H, int N, int D, int dtype, int grid_w,
                               int32_t* match, float* weight, float* expect, float* attn,
                               int32_t* status /* NULL or [n_pairs]: 0 | 1 | 2 */, int32_t* counts /* NULL or [n_feat] */,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- soft region maps: the soft region score per query token (additive to ABI v7) ------------------------------------------------
 * dsim_pair_score_maps_regions for dsim_pair_score_weights: weights [n_feat][N] bytes, w = byte / 255, in place of the mask.  For the
 * direction a -> b and a query token t with w_a[t] > 0, both attentions are biased as in the soft score and rounded where the tails
 * round; with dot_t, x2_t, y2_t (cosine) or sqd_t (mse) the token's sums over B, H, D:
 *   local[t]   = the token's own value, not weighted by its own weight: dot_t / (|x_t| |y_t|) with the finish's eps rule, or
 *                sqd_t / (B H D)
 *   contrib[t] = its term of the direction's soft value: w_a[t] dot_t / (sqrt(sum w x2) sqrt(sum w y2)), or
 *                w_a[t] sqd_t / (B H D sum w_a), sum w_a taken as (byte sum) / 255
 * so that 0.5 (sum contrib[p][0] + sum contrib[p][1]) is score[p], which agrees with dsim_pair_score_weights within
 * 1e-6 max(1, |s|).  The weight enters in f64 in the finish; the per-token partials are unweighted.  Tokens of weight 0 hold +0.0f in
 * both maps.  With bytes 0 / 255 the three outputs are dsim_pair_score_maps_regions' bits.
 *   status      : NULL, or device int32 [n_pairs]: 0, 1 non-finite score, 2 an image of byte sum 0 (score NaN, maps zero)
 *   weight_sums : NULL, or device int32 [n_feat]: the images' byte sums
 * Deterministic, no atomics, every output element has one writer.  Refusals as dsim_pair_score_maps_regions and
 * dsim_pair_score_weights, decided before anything is enqueued. */
size_t dsim_pair_score_maps_weights_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);
int    dsim_pair_score_maps_weights(const void* q, const void* k, const void* v, const uint8_t* weights /* [n_feat][N] */,
                                    int n_feat, const int32_t* idx_a, const int32_t* idx_b, int n_pairs,
                                    int B, int H, int N, int D, int dtype, int similarity,
                                    float* score, float* local, float* contrib,
                                    int32_t* status /* NULL or [n_pairs]: 0, 1 non-finite, 2 zero weight */,
                                    int32_t* weight_sums /* NULL or [n_feat] */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- soft region alignments (additive to ABI v7) -------------------------------------------------------------------------------
 * dsim_pair_align_regions with weights for the mask: Pm[i][j] is the mean over B, H of the softmax over the listed j (w_b[j] > 0) of
 * Q_a[i] . K_b[j] / sqrt(D) + ln w_b[j].  A query token's own weight does not enter; a token of weight 0 is an off token: match -1,
 * weight 0, expect (-1, -1).  match, weight, expect and attn are as the region alignments', over these probabilities.  The bias is
 * log2(byte / 255) from the soft score's table, added to the exponent's argument in f32 with the raw running maximum as the
 * reference point.  With bytes 0 / 255 the outputs are dsim_pair_align_regions' bits.
 *   status      : NULL, or device int32 [n_pairs]: 0, 1 non-finite probability, 2 an image of byte sum 0 (every row off)
 *   weight_sums : NULL, or device int32 [n_feat]: the images' byte sums
 * Refusals as dsim_pair_align_regions and dsim_pair_score_weights. */
size_t dsim_pair_align_weights_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);
int    dsim_pair_align_weights(const void* q, const void* k, const uint8_t* weights /* [n_feat][N] */, int n_feat,
                               const int32_t* idx_a, const int32_t* idx_b, int n_pairs,
                               int B, int H, int N, int D, int dtype, int grid_w,
                               int32_t* match, float* weight, float* expect, float* attn,
                               int32_t* status /* NULL or [n_pairs]: 0 | 1 | 2 */, int32_t* weight_sums /* NULL or [n_feat] */,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- text attention maps and text-guided regions: the prompt's cross-attention picks the tokens --------------------------------
 * What `--use_text_attn` (argprocess.py:17 of the reference) names.  For image i, on the conditional CFG half only (batch element
 * e = 2 i + 1 of xq; context row 1 when n_kv == 2, row e when n_kv == 2 n_images):
 *   P_h[n][l] = softmax_l(xq_h[n,:] . xk_h[l,:] / sqrt(D)),   T_i[n][l] = mean of P_h[n][l] over the H heads (ascending),
 *   s_i[n]    = sum_l w_i[l] T_i[n][l]                         (saliency: f32 fma, l ascending),
 *   m_i       = mean of s_i over the N tokens (summed in f64 in an order that depends on N alone),
 *   token n is on iff (double)s_i[n] >= (double)rel_threshold * m_i; if no token passes (a threshold above every token, or
 *   non-finite saliency) every token is on: the whole image.
 *   xq          : dtype [n_images][2][N] rows of ldq elements, head h in columns [h D, (h + 1) D)   (dsim_unet_qkv_text's xq: ldq = H D)
 *   xk          : dtype [n_kv][L] rows of ldk elements, likewise                                     (its xkv: ldk = 2 H D)
 *   token_weight: device f32 [n_w][L], n_w = 1 (shared) or n_images; may be NULL when only attn / status are asked for
 *   attn        : NULL, or device f32 [n_images][N][L]: T
 *   saliency    : NULL, or device f32 [n_images][N]
 *   mask        : NULL, or device uint8 [n_images][N]: 1 = on (the mask dsim_pair_score_regions takes)
 *   counts      : NULL, or device int32 [n_images]: the mask's sum
 *   status      : NULL, or device int32 [n_images]: 1 when any probability of the image is non-finite
 * The logits come from the stored values without pre-scaling xq, the scale enters in f32 after the matrix product and nothing is
 * rounded to 16 bits on the way to T (dsim_pair_align's arithmetic).  Deterministic, no atomics; an image's values do not depend on
 * the other images of the call, nor on which outputs are requested.  All checks before anything is enqueued: DSIM_ERR_INVALID
 * (workspace query: 0 for n_images outside [1, 65535], N < 1 or L outside [1, 128]) for a bad dtype or head dim, H < 1, n_kv not 2
 * or 2 n_images, ldq / ldk below H D or not whole 16-byte chunks, xq / xk not 16-byte aligned, a negative or non-finite
 * rel_threshold, and -- when saliency, mask or counts is asked for -- a NULL token_weight or n_w not 1 or n_images;
 * DSIM_ERR_WORKSPACE for a short workspace. */
size_t dsim_text_attention_workspace_bytes(int n_images, int N, int L);
int    dsim_text_attention(const void* xq, int ldq, const void* xk, int ldk, int n_images, int n_kv, int H, int N, int L, int D,
                           int dtype, const float* token_weight, int n_w, float rel_threshold,
                           float* attn, float* saliency, uint8_t* mask, int32_t* counts, int32_t* status,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- region transfer: the attention mass a token sends into the other image's region -------------------------------------------
 * Every feature image i carries a byte m_i[t] in 0 .. 255 per token, w = m / 255 (the soft regions' convention).  With Pm exactly
 * as dsim_pair_align defines it (softmax over ALL keys, logits from the stored un-rescaled q and k, the scale entering in f32,
 * nothing rounded to 16 bits, the mean over the B CFG halves and H heads), for pair p (a = idx_a[p], b = idx_b[p]):
 *   mass[p][0][i] = sum_j Pm_ab[i][j] w_b[j]   (on a's grid: a's queries over b's keys)
 *   mass[p][1][u] = sum_t Pm_ba[u][t] w_a[t]   (on b's grid: b's queries over a's keys)
 * The weights enter the sum only; no bias joins the logits.  A mass lies in [0, 1] and is 1 where every key byte is 255.
 *   q,k         : dtype [n_feat][B][N][H*D], as dsim_pair_align (no v)
 *   weights     : device uint8 [n_feat][N]
 *   directions  : 1: rows [p][0] only, 2: rows [p][1] only, 3: both; rows of a direction not asked for are not written
 *   mass        : device f32 [n_pairs][2][N]
 *   status      : NULL, or device int32 [n_pairs]: 1 where a probability of the pair (in a direction asked for) is non-finite
 * One pass over the keys, Pm is never formed: per query row and (b, h) the online maximum and two running f32 sums,
 * l = sum_j e_ij and num = sum_j e_ij w_j (fma) with e_ij = exp2(fma(s, c, -m c)), r_bh = num / l; mass = (sum over (b, h) ascending
 * of r_bh) * (1 / (B H)).  The workspace holds r_bh, f32 [n_pairs][2][B H][N], folded in that fixed order by a second launch.
 * Deterministic, no atomics; a pair's values do not depend on the other pairs of the call, on the directions asked for, or on the
 * weights of images other than the row's key image.  All checks before anything is enqueued: DSIM_ERR_INVALID (workspace query: 0)
 * as dsim_pair_align for the dtype, head dim and shape, for n_feat < 1 or n_feat N >= 2^31; DSIM_ERR_INVALID for directions
 * outside 1 .. 3 and a NULL weights or mass; DSIM_ERR_WORKSPACE for a short workspace. */
size_t dsim_pair_region_transfer_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);
int    dsim_pair_region_transfer(const void* q, const void* k, const uint8_t* weights /* [n_feat][N] */, int n_feat,
                                 const int32_t* idx_a, const int32_t* idx_b, int n_pairs, int B, int H, int N, int D, int dtype,
                                 int directions /* 1: rows [p][0], 2: rows [p][1], 3: both */,
                                 float* mass /* [n_pairs][2][N] */, int32_t* status /* NULL or [n_pairs] */,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- transfer matrix: the mass every gallery image sends into every query's weighted tokens (additive to ABI v7) ------------------
 * Set A has n_a feature images with weight bytes weights_a [n_a][N] (w = byte / 255), set B has n_b images and no weights; the sets
 * are separate tensors, as dsim_score_matrix's.  Cell (i, j) is dsim_pair_region_transfer's mass[p][1] of the pair (a = A_i, b = B_j):
 *   mass[i][j][u] = sum_t Pm_ba[u][t] w_a[t]   (on B_j's grid: B_j's queries over A_i's keys, weighted by A_i's bytes)
 * bit for bit, in every dtype and at every head dim: the same logits, online maximum, l and num with the same fma order,
 * r_bh = num / l, and the fold over (b, h) ascending times 1 / (B H).
 *   qa,ka       : dtype [n_a][B][N][H*D];  qb,kb: dtype [n_b][B][N][H*D] (no v; the kernel reads qb and ka only)
 *   weights_a   : device uint8 [n_a][N]
 *   mass        : device f32 [n_a][n_b][N]
 *   status      : NULL, or device int32 [n_a][n_b]: 1 where a probability of the cell is non-finite
 * The workspace holds r_bh, f32 [n_a n_b][B H][N]: one direction only.  Deterministic, no atomics, one writer per element; a cell's
 * row depends on its two images and A_i's weights alone.  All checks before anything is enqueued: DSIM_ERR_INVALID (workspace query:
 * 0) for a bad dtype or head dim, n_a < 1 or n_b < 1, n_a + n_b > 65535, B H > 65535, ceil(N/128) n_a n_b >= 2^31, or any tensor
 * (features, weights, masses, workspace) of 2^31 elements or more; DSIM_ERR_INVALID for a NULL pointer other than status;
 * DSIM_ERR_WORKSPACE for a short workspace. */
size_t dsim_region_transfer_matrix_workspace_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype);
int    dsim_region_transfer_matrix(const void* qa, const void* ka, const uint8_t* weights_a /* [n_a][N] */, int n_a,
                                   const void* qb, const void* kb, int n_b, int B, int H, int N, int D, int dtype,
                                   float* mass /* [n_a][n_b][N] */, int32_t* status /* NULL or [n_a][n_b] */,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- cell-region score matrices: set B's region belongs to the cell, not to the image (additive to ABI v7) ------------------------
 * dsim_score_matrix_regions / dsim_score_matrix_weights with one change: set B's masks or weights are [n_a][n_b][N], one row per
 * cell; set A's stay [n_a][N].  Cell (i, j) is dsim_pair_score_regions (dsim_pair_score_weights) of the pair (A_i, B_j) under the
 * rows (mask_a[i], mask_b[i][j]), bit for bit: the same lists over the non-zero bytes in ascending order, the same rounding points,
 * the same bias table and (float)m / 255.0f factors, the same partial layout and f64 fold.  With mask_b[i][j] equal for all i it is
 * dsim_score_matrix_regions' (dsim_score_matrix_weights') cell, bit for bit.
 * A_i's self-attention over its region is computed once per query image; B_j's depends on the cell and runs with the cell's cross
 * attention in one workgroup: a cell costs three attentions.
 *   out         : device f32 [n_a][n_b]
 *   status      : NULL, or device int32 [n_a][n_b]: 0, 1 where the score is NaN or infinite, 2 where mask_a[i] or mask_b[i][j] is
 *                 empty (weights: has byte sum 0); such a cell is NaN and disturbs no other cell
 *   counts / weight_sums : NULL, or device int32 [n_a + n_a n_b]: set A's region sizes (byte sums), then the cells' in cell order
 * Deterministic, no atomics; a cell depends on its two images and its two rows alone; rows outside a region are never read.
 * Refusals as dsim_score_matrix_regions (dsim_score_matrix_weights) with n_a + n_a n_b rows where those have n_a + n_b:
 * DSIM_ERR_INVALID (workspace query: 0) or DSIM_ERR_WORKSPACE, decided on the host before anything is enqueued. */
size_t dsim_score_matrix_cell_regions_workspace_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype);
int    dsim_score_matrix_cell_regions(const void* qa, const void* ka, const void* va, const uint8_t* mask_a /* [n_a][N] */, int n_a,
                                      const void* qb, const void* kb, const void* vb, const uint8_t* mask_b /* [n_a][n_b][N] */, int n_b,
                                      int B, int H, int N, int D, int dtype, int similarity,
                                      float* out /* [n_a][n_b] */, int32_t* status /* NULL or [n_a][n_b]: 0 | 1 | 2 */,
                                      int32_t* counts /* NULL or [n_a + n_a n_b] */,
                                      void* workspace, size_t workspace_bytes, void* stream);
size_t dsim_score_matrix_cell_weights_workspace_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype);
int    dsim_score_matrix_cell_weights(const void* qa, const void* ka, const void* va, const uint8_t* weights_a /* [n_a][N] */, int n_a,
                                      const void* qb, const void* kb, const void* vb, const uint8_t* weights_b /* [n_a][n_b][N] */,
                                      int n_b, int B, int H, int N, int D, int dtype, int similarity,
                                      float* out /* [n_a][n_b] */, int32_t* status /* NULL or [n_a][n_b]: 0 | 1 | 2 */,
                                      int32_t* weight_sums /* NULL or [n_a + n_a n_b] */,
                                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- VAE encoder: replaces `pipe.vae.encode(image)` in
 *      DiffSim.prepare_image_latents (diffsim/diffsim.py:92-96).  Sampling
 *      z = mean + exp(0.5*clamp(logvar,-30,20))*eps and the 0.18215 scaling stay with the caller,
 *      which owns the generator whose draw order defines the score. ------------------------------ */
typedef struct dsim_vae_cfg {
    int32_t in_channels;                          /* 3 */
    int32_t latent_channels;                      /* 4 */
    int32_t n_levels;                             /* 4 */
    int32_t block_out_channels[DSIM_MAX_LEVELS];  /* 128,256,512,512 */
    int32_t layers_per_block;                     /* 2 */
    int32_t norm_num_groups;                      /* 32 */
    int32_t compute_dtype;                        /* DSIM_F32 or DSIM_BF16 */
} dsim_vae_cfg;
typedef struct dsim_vae dsim_vae;

int    dsim_vae_create(const dsim_vae_cfg* cfg, dsim_vae** out);
void   dsim_vae_destroy(dsim_vae* h);
/* diffusers AutoencoderKL keys: "encoder.*" and "quant_conv.*" (decoder keys are not needed) */
int    dsim_vae_load_weight(dsim_vae* h, const char* key, const void* dev_ptr, int dtype,
                            const int64_t* shape, int ndim);
int    dsim_vae_finalize(dsim_vae* h, void* stream);
/* Workspace of one dsim_vae_encode call; 0 for a call it refuses: an image size the encoder does not take, or a batch one of whose
 * activations would reach 2 GiB (32-bit tensor offsets), which dsim_vae_encode refuses with DSIM_ERR_INVALID before it enqueues */
size_t dsim_vae_workspace_bytes(const dsim_vae* h, int n_images, int image_size);
/* images: f32 [n][3][S][S] in [-1,1] (process_image output); moments (out): f32 [n][2*latent][S/8][S/8]
 * = cat(mean, logvar) exactly as AutoencoderKL's quant_conv output */
int    dsim_vae_encode(dsim_vae* h, const float* images, int n_images, int image_size, float* moments,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Measurement aid (ABI v7), same contract and record format as dsim_unet_profile / _count / _get: per launch of the next
 * dsim_vae_encode calls, the kernel family, its algorithmic FLOPs / bytes and its HIP-event duration on the launch stream */
int    dsim_vae_profile(dsim_vae* h, int enable);
int    dsim_vae_profile_count(const dsim_vae* h);
int    dsim_vae_profile_get(dsim_vae* h, int i, char* name, int name_cap, double* flops, double* bytes, double* ms);

/* ---- DiT-XL/2 scorer backbone: replaces `diffusion.p_sample(model, latents, t,
 *      model_kwargs=dict(y=[1, 1000]))` + the pre-hook on model.blocks[L].attn of diffsim/diffsim_dit.py:93-114.
 *      Weights under the reference's own state-dict keys (DiT/modelsdit.py): pos_embed, x_embedder.proj.*,
 *      t_embedder.mlp.{0,2}.*, y_embedder.embedding_table.weight, blocks.N.{attn.qkv,attn.proj,mlp.fc1,mlp.fc2,
 *      adaLN_modulation.1}.* -------------------------------------------------------------------------------- */
typedef struct dsim_dit_cfg {
    int32_t input_size;        /* latent side: 32 for 256 px */
    int32_t patch_size;        /* 2 */
    int32_t in_channels;       /* 4 */
    int32_t hidden_size;       /* 1152 */
    int32_t depth;             /* 28 */
    int32_t num_heads;         /* 16 */
    int32_t mlp_ratio;         /* 4 */
    int32_t num_classes;       /* 1000 (embedding table has num_classes + 1 rows) */
    int32_t freq_dim;          /* 256 */
    int32_t compute_dtype;     /* DSIM_F32 or DSIM_BF16 */
    int32_t tap_layer;         /* block index L of the hooked attention */
} dsim_dit_cfg;
typedef struct dsim_dit dsim_dit;

int    dsim_dit_create(const dsim_dit_cfg* cfg, dsim_dit** out);
void   dsim_dit_destroy(dsim_dit* h);
int    dsim_dit_load_weight(dsim_dit* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim);
int    dsim_dit_finalize(dsim_dit* h, void* stream);
/* t_model = the timestep the MODEL sees = SpacedDiffusion.timestep_map[1000 - target_step]
 * (DiT/diffusion/respace.py:117-129); y0,y1 = class labels of the two batch halves (1 and num_classes = null) */
int    dsim_dit_set_conditioning(dsim_dit* h, int t_model, int y0, int y1, void* stream);
/* Attention arithmetic of the DiT blocks: 0 = the handle's compute dtype (default), 1 = fp8 (OCP e4m3) MFMAs for
 * both QK^T and PV with f32 softmax (BASELINE.json config 5; bf16 handles, head_dim 72 or 32 only).  The
 * reference's timm Attention (DiT/modelsdit.py:103-124, F.scaled_dot_product_attention in fp16) has no such mode:
 * it is an opt-in accuracy/throughput trade, compared with the oracle under a stated looser tolerance. */
int    dsim_dit_set_attention(dsim_dit* h, int mode);
/* Measurement aid, same contract and record format as dsim_unet_profile / _count / _get */
int    dsim_dit_profile(dsim_dit* h, int enable);
int    dsim_dit_profile_count(const dsim_dit* h);
int    dsim_dit_profile_get(dsim_dit* h, int i, char* name, int name_cap, double* flops, double* bytes, double* ms);
/* Workspace of one dsim_dit_qkv call; 0 for a batch one of whose activations would reach 2 GiB (32-bit tensor offsets), which
 * dsim_dit_qkv refuses with DSIM_ERR_INVALID before it enqueues anything */
size_t dsim_dit_workspace_bytes(const dsim_dit* h, int n_images);
/* Move the tap (the block whose attention q,k,v are emitted) without re-packing: ONE weight copy serves every
 * --target_layer of diffsim_DiT.diffsim_score (diffsim/diffsim_dit.py:100-104 hooks model.blocks[target_layer[0]].attn).
 * DSIM_ERR_MISSING_WEIGHT if a block up to the new tap was never loaded (the old tap stays).  dsim_dit_set_conditioning
 * prepares the modulation vectors of every loaded block, so the conditioning survives a move of the tap. */
int    dsim_dit_set_tap(dsim_dit* h, int tap_layer);
/* x_t = sqrt_abar*latents + sqrt_1m_abar*noise (DDIM add_noise at t = target_step, diffsim_dit.py:63-72);
 * q,k,v (out): compute dtype [n_images][2][tokens][heads*head_dim] */
int    dsim_dit_qkv(dsim_dit* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar,
                    int n_images, void* q, void* k, void* v, void* workspace, size_t workspace_bytes, void* stream);
/* Tap sweep: dsim_dit_qkv for the blocks layers[0..n_taps) (any order) in ONE walk to the deepest, q[i], k[i], v[i] bit for bit
 * what dsim_dit_qkv writes with its tap at layers[i].  A shallower tap is captured by the three row-block projections of the tap
 * path; the block then runs its fused qkv projection as usual.  The handle's tap is neither read nor moved.  Errors as
 * dsim_unet_qkv_taps (a layer outside [0, depth) or a duplicate: DSIM_ERR_INVALID); the workspace query returns 0 for them and
 * for a tap output of n_images that would reach 2 GiB. */
size_t dsim_dit_taps_workspace_bytes(const dsim_dit* h, int n_images, int n_taps, const int* layers);
int    dsim_dit_qkv_taps(dsim_dit* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar,
                         int n_images, int n_taps, const int* layers, void* const* q, void* const* k, void* const* v,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- ViT scorer backbones (additive to ABI v7): the reference's clip_cross and dino_cross metrics.  Replaces the forward of HF
 *      CLIPVisionModel up to encoder layer L with the hook of metrics/hooks.py:3-17 on it (metrics/clip_i.py:113-141), and of HF
 *      Dinov2Model up to layer L's attention with the hook of metrics/hooks.py:19-32 on it (metrics/dino.py:120-146): q, k, v are
 *      the hooked layer's own q / k / v Linear layers applied to the hook's input.
 *      Weights under one neutral naming (the Python side maps the HF keys): pos_embed [N][C] (already interpolated to the
 *      handle's side), cls_token [C], x_embedder.proj.weight [C][3][p][p] (+ .bias with patch_bias), pre_norm.{weight,bias}
 *      (with pre_norm), blocks.N.{norm1,norm2}.{weight,bias}, blocks.N.attn.qkv.{weight,bias} ([3C][C] = q ; k ; v),
 *      blocks.N.attn.proj.*, blocks.N.mlp.{fc1,fc2}.*, blocks.N.{ls1,ls2} [C] (with layer_scale). ------------------------- */
#define DSIM_VIT_ACT_GELU 0          /* erf form (F.gelu's default): DINOv2 */
#define DSIM_VIT_ACT_QUICK_GELU 1    /* x * sigmoid(1.702 x): CLIP */
typedef struct dsim_vit_cfg {
    int32_t image_size;        /* side of the (square) input in pixels: 224 */
    int32_t patch_size;        /* 32 (CLIP-B/32), 14 (DINOv2) */
    int32_t hidden_size;       /* C: 768, 384 */
    int32_t depth;             /* 12 */
    int32_t num_heads;         /* 12, 6 (head dim 64) */
    int32_t mlp_dim;           /* 3072, 1536 */
    int32_t act;               /* DSIM_VIT_ACT_* */
    int32_t pre_norm;          /* 1: LayerNorm on the embedded tokens (CLIP's pre_layrnorm) */
    int32_t patch_bias;        /* 1: the patch conv has a bias (DINOv2) */
    int32_t layer_scale;       /* 1: LayerScale vectors on both residual branches (DINOv2) */
    int32_t tap_input;         /* 0: q/k/v from norm1's output (DINOv2's hook); 1: from the block's raw input (CLIP's hook) */
    float   ln_eps;            /* 1e-5 (CLIP), 1e-6 (DINOv2) */
    int32_t compute_dtype;     /* DSIM_F32, DSIM_BF16 or DSIM_F16 */
    int32_t tap_layer;         /* block index L of the hooked layer */
} dsim_vit_cfg;
typedef struct dsim_vit dsim_vit;

/* Life cycle, error codes and "every check before the first launch" as the dsim_dit_* calls of the same names. */
int    dsim_vit_create(const dsim_vit_cfg* cfg, dsim_vit** out);
void   dsim_vit_destroy(dsim_vit* h);
int    dsim_vit_load_weight(dsim_vit* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim);
int    dsim_vit_finalize(dsim_vit* h, void* stream);
int    dsim_vit_set_tap(dsim_vit* h, int tap_layer);        /* moves the tap without re-packing (as dsim_dit_set_tap) */
int    dsim_vit_profile(dsim_vit* h, int enable);
int    dsim_vit_profile_count(const dsim_vit* h);
int    dsim_vit_profile_get(dsim_vit* h, int i, char* name, int name_cap, double* flops, double* bytes, double* ms);
size_t dsim_vit_workspace_bytes(const dsim_vit* h, int n_images);
/* pixels: f32 [n_images][3][S][S], already normalised (the image processor's output); q,k,v (out): compute dtype
 * [n_images][1][N][heads*head_dim], N = 1 + (S / patch)^2, the class token first.  An image's rows do not depend on the other
 * images of the call beyond the GEMM tile choice. */
int    dsim_vit_qkv(dsim_vit* h, const float* pixels, int n_images, void* q, void* k, void* v, void* workspace,
                    size_t workspace_bytes, void* stream);
/* Tap sweep, as dsim_dit_qkv_taps: the layers (any order, no duplicates) in ONE walk to the deepest, bit for bit what
 * dsim_vit_qkv writes with its tap at layers[i]. */
size_t dsim_vit_taps_workspace_bytes(const dsim_vit* h, int n_images, int n_taps, const int* layers);
int    dsim_vit_qkv_taps(dsim_vit* h, const float* pixels, int n_images, int n_taps, const int* layers, void* const* q,
                         void* const* k, void* const* v, void* workspace, size_t workspace_bytes, void* stream);

/* ---- projected score tail: replaces CLIPScore.attention_calc of metrics/clip_i.py:143-159 (4x SDPA, each followed by the hooked
 *      layer's out_proj, then 2x cosine, mean).  Arguments as dsim_pair_score_status, plus
 *   w_out       : compute dtype [C][C], C = H*D, rows = output features (nn.Linear's weight)
 *   bias        : f32 [C]
 * Per pair and direction the cross and the self attention outputs are rounded to the compute dtype as dsim_pair_score rounds them
 * and kept in the workspace; P = O w_out^T + bias with f32 accumulation, rounded to the compute dtype; the cosine (eps 1e-8) or mse
 * (over B*N*C values) sums are f32 per workgroup and f64 across workgroups in a fixed order: deterministic, no atomics, and a
 * pair's score does not depend on the other pairs of the call.  status may be NULL.
 * DSIM_ERR_INVALID (workspace query: 0) for a head dim outside the supported list, a bad dtype or similarity, n_pairs < 1,
 * 2 n_pairs > 65535, 2 B H > 65535 or C > 1024 (16 rows of C f32 values fill 64 KiB of LDS); DSIM_ERR_WORKSPACE for
 * a short workspace; both decided on the host before anything is enqueued. */
size_t dsim_pair_score_proj_workspace_bytes(int n_pairs, int B, int H, int N, int D, int dtype);
int    dsim_pair_score_proj(const void* q, const void* k, const void* v, const int32_t* idx_a, const int32_t* idx_b, int n_pairs,
                            int B, int H, int N, int D, int dtype, int similarity, const void* w_out, const float* bias,
                            float* out_scores, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---- feature-cosine metrics: the reference's `diffeats` (metrics/diffeats.py:136-205) and `dinofeats` (metrics/dino.py:163-183):
 *      the plain cosine of the tapped self-attention's OWN output, the ablation beside the attention scores above.
 * dsim_attn_features: per image i, O_i = SDPA(q_i, k_i, v_i) per (b, h) on the tiled attention core, rounded to the compute dtype as
 *   dsim_pair_score rounds its outputs and merged to [B][N][C] rows, C = H*D.
 *     q,k,v       : dtype [n][B][N][H*D] (16-byte aligned);  L = B*N*H*D, an image's elements (stated so that the call and its
 *                   consumers below agree on it)
 *     w_out, bias : both NULL (F = O: dinofeats, the context layer as it is), or the tapped layer's output projection, compute dtype
 *                   [C][C] (rows = output features) and f32 [C]: F = O w_out^T + bias on the matrix cores, f32 accumulation in an
 *                   order fixed by the tile shape, rounded once (diffeats: attn1.to_out.0; no residual, no rescale)
 *     minmax      : non-zero: G = (F - mn) / (mx - mn) in f32, rounded to the compute dtype, mn / mx the exact minimum / maximum of
 *                   the image's rounded F over all B N C values (diffeats.py:136-140).  mx == mn makes every value of that image NaN,
 *                   as the reference's division does.  Zero: G = F.
 *     feats (out) : dtype [n][B][N][C], G
 *     stats (out) : f32 [n][4] = { sum of G^2, mn, mx, 0 } (mn, mx: of F); the sum is f32 per workgroup and f64 across workgroups in
 *                   a fixed order
 *   No atomics; an image's features and stats do not depend on the other images of the call.
 * dsim_feature_pair_score: out[p] = cosine_similarity(flat G of image idx_a[p], flat G of image idx_b[p]), eps 1e-8 under each norm
 *   (the eps arithmetic of dsim_pair_score): the dot product over L in f32 per workgroup and f64 across in a fixed order, the norms
 *   from stats.  status: NULL, or device int32 [n_pairs], 1 where the score is NaN or infinite.  A pair's score does not depend on
 *   the other pairs of the call.
 * dsim_feature_matrix: out[a][b] = the same cosine of (image a of set A, image b of set B), as a Gram product on the matrix cores in
 *   the 16-bit modes (f32: exact-f32 MFMAs): 32 x 128 tiles, K split over workgroups in 16384 elements, the f32 partials folded in
 *   f64 in ascending K order.  No atomics.  A cell's value depends on its two images alone: not on n_a, n_b, its position or the other
 *   cells (edge tiles are zero-padded; a NaN image poisons only its own row or column), and out[a][b] of (A, B) equals out[b][a] of
 *   (B, A).  A matrix cell and the pair score of the same two images are NOT bit-equal: the matrix cores and the vector unit round a
 *   long dot product differently; both are deterministic and hold the same bound against float64.
 *     status      : NULL, or device int32 [n_a][n_b], as above
 * Every check is made before anything is enqueued.  DSIM_ERR_INVALID (workspace query: 0) for a bad dtype, a head dim outside the
 * supported list, n < 1, n > 65535, n_pairs > 65535, B H > 65535, L != B N H D, L % 8 != 0, L > 2^30, n_a n_b >= 2^31, or one of
 * w_out / bias without the other; DSIM_ERR_WORKSPACE for a short workspace. */
size_t dsim_attn_features_workspace_bytes(int n, int B, int H, int N, int D, int L, int dtype, int proj);
int    dsim_attn_features(const void* q, const void* k, const void* v, int n, int B, int H, int N, int D, int L, int dtype,
                          const void* w_out, const float* bias, int minmax, void* feats, float* stats, void* workspace,
                          size_t workspace_bytes, void* stream);
size_t dsim_feature_pair_score_workspace_bytes(int n_pairs, int L, int dtype);
int    dsim_feature_pair_score(const void* feats, const float* stats, const int32_t* idx_a, const int32_t* idx_b, int n_pairs, int L,
                               int dtype, float* out_scores, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
size_t dsim_feature_matrix_workspace_bytes(int n_a, int n_b, int L, int dtype);
int    dsim_feature_matrix(const void* fa, const float* stats_a, int n_a, const void* fb, const float* stats_b, int n_b, int L,
                           int dtype, float* out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* dsim_feature_matrix with the caller's K chunk (additive to ABI v7): the same kernels and the same f64 fold, the f32 partial sums
 * ending every k_chunk elements instead of every 16384 (k_chunk a multiple of 64 in [64, 16384]; 16384 is dsim_feature_matrix bit
 * for bit, and so is any k_chunk >= L).  For long descriptors whose terms are all of one sign -- the Gram descriptors below -- where a
 * 16384-term f32 chain rounds a cell to about 4e-6 and 1024-term chains to about 2e-7.  The workspace grows with ceil(L / k_chunk).
 * Refusals as dsim_feature_matrix, and for a k_chunk outside the list or ceil(L / k_chunk) > 65535. */
size_t dsim_feature_matrix_chunked_workspace_bytes(int n_a, int n_b, int L, int dtype, int k_chunk);
int    dsim_feature_matrix_chunked(const void* fa, const float* stats_a, int n_a, const void* fb, const float* stats_b, int n_b, int L,
                                   int dtype, int k_chunk, float* out, int32_t* status, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* ---- VGG Gram style metric (additive to ABI v7): the reference's `gram` (metrics/vgg_gram.py).  Replaces torchvision's
 *      vgg19().features run up to module '28' (conv5_1 BEFORE its ReLU), gram_matrix (G = X X^T over the spatial axis, not
 *      normalised) and, with dsim_feature_pair_score / dsim_feature_matrix on the f32 rows, the cosine of line 81.
 *      A conv-only stack: 3x3 convs (stride 1, padding 1, bias), a ReLU behind every conv but the last, 2x2 max-pools of stride 2 in
 *      floor mode.  Weights under one neutral naming (the Python side maps torchvision's features.N keys): convs.I.weight
 *      [Cout][Cin][3][3] and convs.I.bias [Cout], I = 0, 1, ... counting the plan's convs. */
#define DSIM_VGG_MAX_PLAN 32
typedef struct dsim_vgg_cfg {
    int32_t in_channels;                /* 3 (1 .. 4: the first conv runs on a direct kernel from the NCHW pixels) */
    int32_t plan[DSIM_VGG_MAX_PLAN];    /* > 0: a conv's output channels (% 8 == 0; the input channels of every conv but the first
                                           must be a multiple of 64, the implicit GEMM's K tile); 0: a 2x2 max-pool (only behind a
                                           conv); -1 ends it.  The first and the last entry are convs; the tap is the last conv's
                                           output, without ReLU.  VGG-19 to conv5_1: 64,64,0,128,128,0,256 x4,0,512 x4,0,512,-1 */
    int32_t compute_dtype;              /* DSIM_F32, DSIM_BF16 or DSIM_F16 */
} dsim_vgg_cfg;
typedef struct dsim_vgg dsim_vgg;

/* Life cycle, error codes and "every check before the first launch" as the dsim_vit_* calls of the same names.  dsim_vgg_create:
 * DSIM_ERR_INVALID for a plan that breaks the rules above or has no terminator, and for a dtype outside the three. */
int    dsim_vgg_create(const dsim_vgg_cfg* cfg, dsim_vgg** out);
void   dsim_vgg_destroy(dsim_vgg* h);
int    dsim_vgg_load_weight(dsim_vgg* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim);
int    dsim_vgg_finalize(dsim_vgg* h, void* stream);
int    dsim_vgg_profile(dsim_vgg* h, int enable);
int    dsim_vgg_profile_count(const dsim_vgg* h);
int    dsim_vgg_profile_get(dsim_vgg* h, int i, char* name, int name_cap, double* flops, double* bytes, double* ms);
/* the tap's geometry for H x W inputs: H' = H >> pools, W' = W >> pools, C = the last conv's channels; DSIM_ERR_INVALID for an
 * image smaller than the pools allow */
int    dsim_vgg_out_shape(const dsim_vgg* h, int H, int W, int* out_h, int* out_w, int* out_c);
/* One call is one batch of n equally sized images; H and W are independent and need not be even (a pool drops an odd last row or
 * column without reading it).  pixels: f32 [n][in_channels][H][W], already normalised; out: compute dtype [n][H'][W'][C],
 * channel-last.  The implicit GEMM addresses tensors with 32-bit offsets: a batch whose largest activation would reach 2 GiB (64
 * channels at 512 x 768 are 50 MB per image in 16 bits) is refused with DSIM_ERR_INVALID, and dsim_vgg_workspace_bytes returns 0 for
 * it; split the batch.  DSIM_ERR_INVALID for n < 1 or a NULL pointer, DSIM_ERR_STATE before finalize, DSIM_ERR_WORKSPACE for a short
 * workspace: all before anything is enqueued.  The executor does not rescale: with real VGG-19 weights fp16 activations can
 * overflow, bf16 is the mode for this metric. */
size_t dsim_vgg_workspace_bytes(const dsim_vgg* h, int n_images, int H, int W);
int    dsim_vgg_features(dsim_vgg* h, const float* pixels, int n_images, int H, int W, void* out, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The stack's two element-wise kernels alone (tests): x = relu(x) in place over n_elems elements (a multiple of 16 bytes), and
 * out [n][H/2][W/2][C] = maxpool2x2(relu(in [n][H][W][C])) (C % 8 == 0, H, W >= 2); NaN propagates through both, as in torch. */
int    dsim_op_relu(void* x, size_t n_elems, int dtype, void* stream);
int    dsim_op_relu_pool2(const void* in, void* out, int n, int H, int W, int C, int dtype, void* stream);
/* dsim_gram_rows: out[i][r - row0][c] = sum_p X_i[p][r] X_i[p][c] for r in [row0, row0 + n_rows), X_i = feat[i] ([P][C],
 *   channel-last, P = H' W'): rows of the Gram matrix of image i, both operands from the same tile.
 *     feat        : dtype [n][P][C], 16-byte aligned, C % 8 == 0
 *     out         : f32 [n][n_rows][C], ALWAYS f32 (Gram entries of real VGG features exceed fp16's range)
 *     stats (out) : f32 [n][4] = { sum of out^2 (accumulated in f64), min, max, 0 }: what dsim_feature_pair_score /
 *                   dsim_feature_matrix expect beside out as DSIM_F32 features of L = n_rows C
 *   16-bit dtypes with n_rows >= 8 and row0 % 8 == 0 run on the matrix cores (32 x 128 tiles, f32 accumulation); f32 features and
 *   the other row ranges (the reference's single row) on the vector unit with one fma per position, p ascending.  P is split over
 *   workgroups in 512 positions; the f32 partials fold in ascending p order.  No atomics; an image's rows and stats do not depend
 *   on the other images of the call.  DSIM_ERR_INVALID (workspace query: 0) for a bad dtype, n < 1, P < 1, C % 8 != 0, a row
 *   range outside [0, C), n ceil(P / 512) > 65535, n_rows > 65535 or n_rows C > 2^30; DSIM_ERR_WORKSPACE for a short workspace;
 *   decided on the host before anything is enqueued. */
size_t dsim_gram_rows_workspace_bytes(int n, int P, int C, int row0, int n_rows, int dtype);
int    dsim_gram_rows(const void* feat, int n, int P, int C, int row0, int n_rows, int dtype, float* out, float* stats,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- the arithmetic either side of the VAE encoder, on the device (the host only decodes and resizes) ----
 * dsim_image_preprocess: what process_image does after its Lanczos resize (diffsim/diffsim.py:31-41): pixels u8 [n][H][W][3] ->
 *   f32 [n][3][H][W] = (p / 255 - 0.5) / 0.5 in IEEE f32, bit-identical to the numpy path; to_half = 1 additionally rounds
 *   through fp16 (the SD1.5 pipeline's `image.to(dtype=float16)`, diffsim.py:93).
 * dsim_latent_sample: `scaling_factor * latent_dist.sample()` of prepare_image_latents (diffsim.py:92-96): out[j] =
 *   sf * (mean + exp(0.5 clamp(logvar, -30, 20)) * eps) for image first + j * stride of `moments` ([n][2C][hw], dsim_vae_encode's
 *   output); eps f32 [eps_n][C][hw] drawn by the CALLER's generator (eps_n = 1: one draw shared by all, as every reference call
 *   reseeds; or one per output image); round_fp16 = 1 rounds the latents through fp16 (diffsim_xl.py:63, the fp16 pipelines). */
int dsim_image_preprocess(const unsigned char* pixels_hwc, float* out, int n, int H, int W, int to_half, void* stream);
int dsim_latent_sample(const float* moments, const float* eps, float* out, int n_out, int first, int stride, int C, int hw,
                       int eps_n, float scaling_factor, int round_fp16, void* stream);

/* ---- the resize in front of it, on the device: PIL's 8-bit resampling, bit for bit ----
 * dsim_resize_u8: `image.resize((S, S), LANCZOS)` of process_image (diffsim/diffsim.py:27-33), and the image processors' bicubic
 *   resize + centre crop of the ViT metrics, for packed RGB u8 over a ragged batch: n images of their own sizes, one output size.
 *   Pillow's two passes in Pillow's integer arithmetic: horizontally over the source rows the vertical pass reads, into u8, then
 *   vertically, each as clamp((2^21 + sum_i p[min + i] k[i]) >> 22, 0, 255) in int32 with an arithmetic shift.  An axis whose
 *   source extent equals the output extent is skipped (both: a copy).  Only the window [oy, oy + ch) x [ox, ox + cw) of the
 *   out_h x out_w result is computed and stored: out u8 [n][ch][cw][3].
 *     src        : device bytes; image i is u8 [h][w][3] at images[i].src_offset (a multiple of 16), src_bytes the buffer's length
 *     images     : HOST array [n] (read and copied by the call; free on return).  The call turns it into device descriptors with one
 *                  hipMemcpyAsync from pageable host memory, which the runtime may complete before it returns: a call can block
 *                  the calling thread until the stream has reached that copy
 *     table_data : device int32 [table_ints]; table t, at tables[t].offset: out_size pairs (min, n), then out_size rows of ksize
 *                  coefficients (22-bit fixed point; those past n unread).  One table per distinct (source extent, output extent,
 *                  filter); h_table / v_table = -1 where the pass is skipped (and only there)
 *     tables     : HOST array [n_tables] describing table_data
 *     y_first, rows : the source rows the vertical pass reads, [v-table min(oy), v-table min(oy+ch-1) + n(oy+ch-1)), or [oy, oy + ch)
 *                  without a vertical pass; temp_offset (a multiple of 16, unread without a horizontal pass): where the image's
 *                  rows x round_up(3 cw, 16) temp bytes lie in the workspace's temp area; images must not overlap there
 *   Deterministic, no atomics, 64-bit offsets; an image's bytes do not depend on the other images of the call.
 *   The table CONTENTS live in device memory and are the caller's contract: min >= 0, 1 <= n <= ksize, min + n <= the source extent,
 *   min and min + n non-decreasing (the kernels clamp every window to the image's rows and columns, so a table that breaks this
 *   gives wrong bytes, not a wild access).  Refusals, all decided on the host before anything is enqueued: DSIM_ERR_INVALID
 *   (workspace query: 0) for n < 1 or n > 65535, an output or crop extent < 1, a crop outside the resized image, an image extent < 1,
 *   ksize < 1, any NULL pointer, a source offset + 3 w h beyond src_bytes, a table id >= n_tables or a table beyond table_ints, a
 *   table whose in_size / out_size are not the image's and the output's extent (or -1 where they differ), rows outside the image,
 *   a misaligned offset, or more than ~300 source pixels per output pixel; DSIM_ERR_WORKSPACE for a short workspace. */
typedef struct dsim_resize_image {
    int64_t src_offset;
    int32_t w, h;
    int32_t h_table, v_table;
    int32_t y_first, rows;
    int64_t temp_offset;
} dsim_resize_image;
typedef struct dsim_resize_table {
    int64_t offset;                     /* int32 index into table_data */
    int32_t in_size, out_size, ksize, reserved;
} dsim_resize_table;
size_t dsim_resize_u8_workspace_bytes(const dsim_resize_image* images, int n, const dsim_resize_table* tables, int n_tables,
                                      size_t table_ints, int out_w, int out_h, int ox, int oy, int cw, int ch, size_t src_bytes);
int    dsim_resize_u8(const unsigned char* src, size_t src_bytes, const dsim_resize_image* images, int n, const int32_t* table_data,
                      size_t table_ints, const dsim_resize_table* tables, int n_tables, int out_w, int out_h, int ox, int oy, int cw,
                      int ch, unsigned char* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- single-operator entry points (kernel-level parity tests and micro-benchmarks) -----
 * x: dtype [M][K] (or NHWC image for the conv forms); w: diffusers-layout f32 weight.      */
int dsim_op_linear(const void* x, const float* w /*[N][K]*/, const float* bias /*[N] or NULL*/,
                   const void* residual /*[M][N] or NULL*/, void* out /*[M][N]*/, int M, int N,
                   int K, int dtype, int geglu /* w is [2*N][K], out = h*gelu(g) */, void* stream);
int dsim_op_conv3x3(const void* x /*[B][H][W][Cin]*/, const float* w /*[Cout][Cin][3][3]*/,
                    const float* bias, const void* residual, void* out, int B, int H, int W,
                    int Cin, int Cout, int stride, int upsample, int dtype, void* stream);
int dsim_op_groupnorm(const void* x0, int C0, const void* x1, int C1, const float* gamma,
                      const float* beta, void* out, int B, int HW, int groups, float eps,
                      int silu, int dtype, void* stream);
int dsim_op_layernorm(const void* x, const float* gamma, const float* beta, void* out, int M,
                      int C, float eps, int dtype, void* stream);
/* LayerNorm without affine, then the adaLN modulation y = LN(x) * (1 + scale2[half]) + shift2[half], half = (row / rows_per_batch) & 1
 * (DiT blocks: the two CFG halves of a batch alternate every rows_per_batch rows); scale2 / shift2: f32 [2][C]; in place allowed. */
int dsim_op_layernorm_mod(const void* x, const float* scale2, const float* shift2, void* out, int M, int C, int rows_per_batch,
                          float eps, int dtype, void* stream);
/* What dsim_op_groupnorm (pre = 0) / dsim_op_groupnorm_pre (pre = 1) launch for a shape: the launcher's own decision (it calls the
 * same function).  Host code only, runs without a device; DSIM_ERR_INVALID where the launch would refuse the shape. */
typedef struct dsim_gn_plan {
    int form;                                   /* 0 one-pass (gn_onepass_kernel), 1 two-pass (gn_stats_kernel + gn_apply_kernel),
                                                   2 pre (gn_fold_kernel + gn_apply_kernel) */
    int NS, UNR;                                /* 16-byte channel slots per thread and rows in flight per thread (one-pass: 1, 0) */
    int CS;                                     /* channels a workgroup covers: the one-pass slab width, else C */
    int tpr, R;                                 /* threads per row and rows in flight per workgroup (R = 256 / tpr) */
    int chunks;                                 /* statistic slabs per image (one-pass: 0; pre: 1, the folded pair) */
    int rb;                                     /* row blocks per image of the apply pass (one-pass: 0) */
} dsim_gn_plan;
int dsim_groupnorm_plan(int C0, int C1, int B, int HW, int groups, int dtype, int pre, dsim_gn_plan* plan);
/* The same for dsim_op_layernorm (mod = 0) / dsim_op_layernorm_mod (mod = 1). */
typedef struct dsim_ln_plan {
    int form;                                   /* 0 lanes-per-row (layernorm_rows_kernel<CPL>), 1 wave-per-row (layernorm_kernel<MAXS, RPW>) */
    int LPR, CPL, passes;                       /* form 0: lanes per row, 16-byte chunks per lane, wave passes per workgroup (else 0) */
    int MAXS, RPW;                              /* form 1: chunk slots per lane, rows per wave (else 0) */
    int blocks;                                 /* workgroups */
} dsim_ln_plan;
int dsim_layernorm_plan(int M, int C, int dtype, int mod, dsim_ln_plan* plan);
/* q: [B][Nq][ldq] at column offset h*D; k,v: [Bkv][Nk][ldk]; batch b reads kv batch b % Bkv */
int dsim_op_attention(const void* q, int ldq, const void* k, const void* v, int ldk, void* out,
                      int ldo, int B, int Bkv, int H, int Nq, int Nk, int D, int dtype,
                      void* stream);
/* the same attention on bf16 tensors with fp8 (e4m3) MFMAs -- the kernel behind dsim_dit_set_attention(h, 1); D = 72 or 32 */
int dsim_op_attention_fp8(const void* q, int ldq, const void* k, const void* v, int ldk, void* out,
                          int ldo, int B, int Bkv, int H, int Nq, int Nk, int D, void* stream);

/* The attention kernels (what dsim_op_attention starts; DSIM_ATTN_FP8 is dsim_op_attention_fp8's):
 *   P160       sdpa160_kernel: 256 queries x 256 keys at d = 160, B == Bkv, 16-byte aligned pointers and ld's (16-bit types)
 *   SHORT      attn_short_kernel<D, false>: Nk <= 96 at d = 40 / 64 / 80 / 160, keys resident in LDS (16-bit types)
 *   SHORT_K80  attn_short_kernel<D, true>: the same for 64 < Nk <= 80 (the 77-key prompt context)
 *   LONG       attn_long_kernel: d = 40, Nk >= 2048, Nk % 64 == 0 (16-bit types)
 *   Q2 / Q2FAST attn_q2_kernel<64, false | true>: d = 64, Nk > 96, Nq >= 256; FAST from Nk >= 1024 on (16-bit types)
 *   FAST       attn_kernel<T, D, true>: the fixed-reference softmax, Nk >= 1024 (16-bit types)
 *   EXACT      attn_kernel<T, D, false>: the exact running maximum (every other 16-bit problem; every f32 problem)
 *   FP8        attn_fp8_kernel<D>: bf16 in / out, e4m3 MFMAs, D = 72 or 32 */
typedef enum dsim_attn_kind {
    DSIM_ATTN_P160 = 0, DSIM_ATTN_SHORT = 1, DSIM_ATTN_SHORT_K80 = 2, DSIM_ATTN_LONG = 3, DSIM_ATTN_Q2 = 4, DSIM_ATTN_Q2FAST = 5,
    DSIM_ATTN_FAST = 6, DSIM_ATTN_EXACT = 7, DSIM_ATTN_FP8 = 8
} dsim_attn_kind;
/* What one attention launch ran, recorded where the kernel was launched (not derived from the dispatch rule). */
typedef struct dsim_attn_launch {
    int kind;                                   /* dsim_attn_kind */
    int D;                                      /* the instantiation's head dim */
    int dtype;                                  /* its element type: DSIM_F32, DSIM_BF16 or DSIM_F16 (FP8: DSIM_BF16, the in / out type) */
    int k80;                                    /* 1: attn_short_kernel<D, true> */
    int qit;                                    /* SHORT / SHORT_K80: query blocks per workgroup, else 0 */
    int grid;                                   /* workgroups launched */
    char family[64];                            /* the profile family the executors name it by: attention_<dtype>_d<D><suffix>, or attention_fp8_d<D> */
} dsim_attn_launch;
/* dsim_op_attention (fp8 = 0) or dsim_op_attention_fp8 (fp8 = 1: dtype must be DSIM_BF16) with every stride and pointer as the
 * executors pass them (the fused q | k | v rows: ldq = ldk = 3C, k = q + C, v = q + 2C; the cross-attention's k | v rows: ldk = 2C,
 * v = k + C); launched (may be NULL) receives the record of the kernel that ran.  Synchronises. */
int dsim_op_attention_ex(const void* q, int ldq, const void* k, const void* v, int ldk, void* out, int ldo, int B, int Bkv, int H,
                         int Nq, int Nk, int D, int dtype, int fp8, dsim_attn_launch* launched, void* stream);
/* The dsim_attn_kind dsim_op_attention_ex would launch for the same arguments, into *kind.  Host code only: launches nothing and
 * reads no pointer (it looks at their alignment), so it runs without a device.  DSIM_ERR_INVALID where the launch would refuse. */
int dsim_attention_plan(const void* q, int ldq, const void* k, const void* v, int ldk, const void* out, int ldo, int B, int Bkv,
                        int H, int Nq, int Nk, int D, int dtype, int fp8, int* kind);
/* out[r][:] = softmax(x[r][:] * scale) over cols (the VAE mid-block's softmax; cols % 8 == 0 in 16-bit types, % 4 in f32; in place
 * allowed).  Synchronises. */
int dsim_op_softmax_rows(const void* x, void* out, int rows, int cols, float scale, int dtype, void* stream);

/* One BasicTransformerBlock feed-forward as a single launch (bf16, C = 320): out = x + ff.net.2(GEGLU(ff.net.0.proj(LayerNorm(x))))
 * -- the chain /root/reference/diffsim/hacked_modules.py:118-132 runs as norm3 -> ff -> + hidden_states.  w1: [8C][C] f32 (diffusers
 * ff.net.0.proj.weight, rows [h ; g]), b1: [8C], w2: [C][4C], b2: [C]; x / out: bf16 [M][C] (out may alias x).
 * Returns DSIM_ERR_INVALID for a width the fused kernel does not cover.                                                   */
int dsim_op_ff_fused(const void* x, const float* ln_gamma, const float* ln_beta, const float* w1, const float* b1,
                     const float* w2, const float* b2, void* out, int M, int C, float eps, void* stream);
/* LayerNorm + bias-free Linear as a single launch (bf16, C = 320 or 640, N a multiple of 64 up to 3 C): out[M][N] = LayerNorm(x) W^T --
 * norm1 -> to_q|to_k|to_v and norm2 -> attn2.to_q of /root/reference/diffsim/hacked_modules.py:88-116.  w: [N][C] f32;
 * ln_gamma = ln_beta = NULL skips the LayerNorm.  Returns DSIM_ERR_INVALID for a shape the kernel does not cover.            */
int dsim_op_ln_linear(const void* x, const float* ln_gamma, const float* ln_beta, const float* w, void* out, int M, int C,
                      int N, float eps, void* stream);

/* dsim_op_ff_fused / dsim_op_ln_linear in either 16-bit compute dtype (DSIM_BF16: the two above; DSIM_F16: the fp16 twins the
 * engines run in fp16 mode); x / out in that dtype. */
int dsim_op_ff_fused_dt(const void* x, const float* ln_gamma, const float* ln_beta, const float* w1, const float* b1,
                        const float* w2, const float* b2, void* out, int M, int C, float eps, int dtype, void* stream);
int dsim_op_ln_linear_dt(const void* x, const float* ln_gamma, const float* ln_beta, const float* w, void* out, int M, int C,
                         int N, float eps, int dtype, void* stream);
/* GroupNorm -> Linear (a Transformer2DModel's norm -> proj_in, hacked_modules.py:336-339) as a statistics pass and ONE row-resident
 * launch that normalises the rows on arrival: out[B][HW][N] = GroupNorm(x[B][HW][C]) W^T + bias, bit for bit dsim_op_groupnorm
 * followed by this operator with gamma = beta = NULL (no normalisation: the plain row-resident Linear + bias).  16-bit dtypes,
 * C = 320 or 640, N a multiple of 64 up to C, w [N][C] f32, bias [N] f32 or NULL; with a GroupNorm HW % 128 == 0 (a 128-row tile
 * lies inside one image).  DSIM_ERR_INVALID for anything else. */
int dsim_op_gn_linear_dt(const void* x, const float* gamma, const float* beta, int groups, float eps, const float* w, const float* bias,
                         void* out, int B, int HW, int C, int N, int dtype, void* stream);

/* The implicit GEMM with every epilogue field the engines use, as one operator (parity tests of each tile and epilogue).
 *   out[m][n] = epi(sum_k A(m,k) W[n][k] + bias[n]); the A0 | A1 channel concatenation along K (linear), or the 3x3 conv of
 *   the [M / (Hout Wout)][H][W][C0] image A0 (stride 1 | 2, ups: nearest 2x upsample folded in, pad 0: the VAE downsample's
 *   F.pad(x, (0, 1, 0, 1)) then no padding).  N counts WEIGHT rows: 2 x the output columns for GEGLU.
 *   w: diffusers-layout f32 -- linear [N][K] (GEGLU rows [h ; g]), conv [N][C0][3][3]; wb_rows > 0 (linear): [M / wb_rows][N][K],
 *      matrix i multiplying rows [i wb_rows, (i + 1) wb_rows), packed wb_stride bytes apart (>= N K x element size, % 16 == 0).
 *   bias / bias2: [N] f32 (bias2, which needs bias, for the rows with odd m / rows_per_batch > 0); act 1: tanh-GELU; gate / gate2:
 *      f32 scales of the output columns before the residual add (gate2, which needs gate: odd m / rows_per_batch).
 *   epi: 0 none, 1 residual ([M][ldo] in dtype), 2 GEGLU (out = h * gelu(g)).
 *   out: [M][ldo] in dtype, ldo >= the output columns (out_split > 0: >= out_split, column run j going to out + j out_split_stride
 *      bytes); DSIM_ERR_INVALID otherwise.
 *   gn_part (16-bit power-of-two 3x3 convs on the 256 x 128 / 256 x 256 / 512 x 128 tiles): [M / gn_hw][gn_hw / 64][N / 4][2] f32
 *      (sum, sum of squares) of the stored output per (64 rows, 4-channel quad).
 * launched receives the instantiation that ran (recorded where it was launched) and family the profile name of the instantiation
 * planned for the same arguments (gemm_family() from gemm_plan(): "gemm[_small]_<dtype>_<bm>x<bn>_<linear | conv3 | conv3p>" +
 * "_geglu" | "_res" | "_act" (act without gate or residual) | "_dit" (a gate, or act with a residual: no "_res" on these) | "", +
 * "_gn" with gn_part, + "|M.. N.. K..").  Allocates and synchronises. */
typedef struct dsim_gemm_op {
    int mode;                                   /* 0 linear, 1 3x3 conv */
    int H, W, stride, ups, pad;                 /* conv: stored input map, stride 1 | 2, upsample 0 | 1, pad 1 | 0 */
    const void* A0; int C0;
    const void* A1; int C1;
    int M, N, K;
    const float* w;
    int wb_rows; unsigned wb_stride;
    const float* bias; const float* bias2; int rows_per_batch;
    int act; const float* gate; const float* gate2;
    int epi;
    const void* residual; void* out; int ldo;
    int out_split; long long out_split_stride;
    int force_big;
    float* gn_part; int gn_hw;
    int dtype;
} dsim_gemm_op;
typedef struct dsim_gemm_launch {
    int bm, bn;
    int kind;                                   /* 0 linear, 1 conv3, 2 conv3p (power-of-two output maps) */
    int geglu;
    int ek;                                     /* 0 plain, 1 residual, 2 DiT gate, 3 tanh-GELU only, 4 / 5 plain / residual + GN statistics */
    int small;                                  /* 1: the small-batch kernel */
    char family[128];                           /* the profile name of the planned instantiation (above) */
} dsim_gemm_launch;
int dsim_op_gemm(const dsim_gemm_op* op, dsim_gemm_launch* launched, void* stream);
/* GroupNorm (+ SiLU) of x [B][HW][C] whose statistics come from a conv epilogue's gn_part (part32, chunks = HW / 64 per image: any
 * other count is DSIM_ERR_INVALID) */
int dsim_op_groupnorm_pre(const void* x, int C, const float* gamma, const float* beta, void* out, int B, int HW, int groups,
                          float eps, int silu, int dtype, const float* part32, int chunks, void* stream);

/* ---- the kernels in front of the models, one operator each: noising + conv_in, the time-embedding primitives, the weight packs,
 * the data movers, DiT's patch embedding, the VAE's quant_conv fold and its output transpose.  Each validates its arguments
 * (DSIM_ERR_INVALID), launches on the stream, synchronises, and writes only into the caller's buffers.
 *
 * dsim_op_conv_in: x = sa * lat + sb * noise (noise NULL: x = lat; NCHW f32 [n_img][Cin][S][S]), then the 3x3 conv with zero padding:
 *   out[(img * dup + d)][S * S][Cout] in dtype for d < dup (dup 1 | 2: the CFG copies).  w: diffusers-layout f32 [Cout][Cin][3][3],
 *   bias f32 [Cout] (16-byte aligned for the eight-wide and row kernels).  force: 0 the executors' choice (the row kernel where it
 *   applies -- Cin 3, Cout 128, S % 64 == 0, no noise, dup 1 --, else what the U-Net's launch picks), or a dsim_conv_in_kernel to run;
 *   a forced kernel that does not apply is DSIM_ERR_INVALID.  gn_part (NULL, or f32 [n_img][S * S / 64][Cout / 4][2]: the row kernel in
 *   the 16-bit dtypes only) receives the GroupNorm partial sums of the stored values, dsim_gemm_op.gn_part's layout.  *kernel (may be
 *   NULL) receives the dsim_conv_in_kernel that ran. */
typedef enum dsim_conv_in_kernel {
    DSIM_CONV_IN_GENERIC = 1,                   /* prep_conv_in_kernel: one output channel per thread, 16 pixels per workgroup */
    DSIM_CONV_IN_EIGHT = 2,                     /* prep_conv_in8_kernel: eight channels per thread; Cout % 8 == 0, Cout <= 2048, staging <= 48 KB */
    DSIM_CONV_IN_ROWS = 3                       /* conv_in_rows_kernel: the VAE's 3 -> 128 conv at image resolution */
} dsim_conv_in_kernel;
int dsim_op_conv_in(const float* lat, const float* noise, float sa, float sb, const float* w, const float* bias, void* out, int dtype,
                    int n_img, int Cin, int S, int Cout, int dup, float* gn_part, int force, int* kernel, void* stream);
/* diffusers Timesteps(dim, flip_sin_to_cos = True, downscale_freq_shift = 0): out f32 [dim] = [cos | sin](t f_i), f_i =
 * exp(-ln(10000) i / (dim / 2)); dim even.  dsim_op_sincos_values: the same for count f32 values on the device, out [count][dim]. */
int dsim_op_timestep_sincos(float* out, int dim, int t, void* stream);
int dsim_op_sincos_values(float* out, int dim, const float* vals, int count, void* stream);
/* y[N] = W[N][K] act(x[K]) + bias[N] in f32: W in w_dtype, bias NULL or in b_dtype, x / y f32; act 0 identity, 1 SiLU on x. */
int dsim_op_gemv_f32(const void* W, int w_dtype, const void* bias, int b_dtype, const float* x, float* y, int N, int K, int act,
                     void* stream);
/* One weight pack from a checkpoint dtype into an engine layout, each value rounded once to dst_dtype:
 *   LINEAR  [rows = N][cols = K] -> [N][K], geglu 0, or 16 / 32 (N % (2 geglu) == 0): the [h ; g] rows interleaved in blocks
 *   CONV3   [rows = Cout][cols = Cin][3][3] -> [Cout][tap][Cin]
 *   CONV_IN [rows = Cout][cols = Cin][3][3] -> f32 [tap * Cin + ci][Cout]          (dst_dtype must be DSIM_F32)
 *   VECTOR  [rows = N] (cols = 1) -> f32 [N], geglu as LINEAR                      (dst_dtype must be DSIM_F32) */
typedef enum dsim_pack_kind { DSIM_PACK_LINEAR = 0, DSIM_PACK_CONV3 = 1, DSIM_PACK_CONV_IN = 2, DSIM_PACK_VECTOR = 3 } dsim_pack_kind;
int dsim_op_pack(int kind, const void* src, int src_dtype, void* dst, int dst_dtype, int rows, int cols, int geglu, void* stream);
/* out[2 b], out[2 b + 1] = in[b] for b < n_batch, elements of bytes_per_elem bytes (% 16 == 0) */
int dsim_op_dup_batch(const void* in, void* out, int n_batch, size_t bytes_per_elem, void* stream);
/* token-major nearest resize [B][Hin][Win][row_bytes] -> [B][Hout][Wout][row_bytes] as F.interpolate(mode = "nearest"); row_bytes % 16 == 0 */
int dsim_op_resize_nearest(const void* in, void* out, int B, int Hin, int Win, int Hout, int Wout, size_t row_bytes, void* stream);
/* dst[(2 img + cfg)][per] = ctx[clamp(index[img], 0, n_ctx - 1)][cfg][per] in dtype; ctx f32 [n_ctx][2][per], index int32 [n_images] */
int dsim_op_gather_ctx(const float* ctx, int n_ctx, const int32_t* index, void* dst, int dtype, int n_images, size_t per, void* stream);
/* DiT's x_embedder + pos_embed on the noised latent: out[(img * 2 + cfg)][T][D] in dtype, T = (S / p)^2, token (ty, tx) =
 * sum_k w[d][k] x[c][ty p + py][tx p + px] + bias[d] + pos[T][D], k = (c p + py) p + px; w f32 [D][Cin p p]; noise is required. */
int dsim_op_patch_embed(const float* lat, const float* noise, float sa, float sb, const float* w, const float* bias, const float* pos,
                        void* out, int dtype, int n_img, int Cin, int S, int p, int D, void* stream);
/* The VAE's quant_conv folded into conv_out: out_w[Cm][K] = wq wco in dtype (wq f32 [Cm][Cm], wco [Cm][K] in dtype), out_b[Cm] =
 * wq bco + bq in f32.  Either output may be NULL.  The bias launch is one workgroup sized from Cm: Cm > 1024 with out_b is
 * DSIM_ERR_INVALID. */
int dsim_op_fold_quant(const float* wq, const void* wco, const float* bco, const float* bq, void* out_w, float* out_b, int Cm, int K,
                       int dtype, void* stream);
/* token-major [n][HW][C] in dtype -> f32 NCHW [n][C][HW] */
int dsim_op_to_nchw_f32(const void* x, float* out, int n, int HW, int C, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSIM_AMD_H */
