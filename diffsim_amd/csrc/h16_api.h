// The host entry points of the sources that are compiled once per 16-bit type (gemm / gemm_skinny / rowres / attention / tails /
// align / regions / soft_regions / region_matrix / region_maps / textattn / transfer / attn160 .hip).  Declarations only and no include guard: common.h includes this file inside `inline namespace DSIM_H16_NS`, the including
// object's own type, and the bf16 objects of the product build once more inside `namespace f16`, which declares the fp16 twins with
// the same signatures and default arguments.  The argument structs and enums are plain dsim types (common.h, above the include).

// implicit GEMM -- gemm.hip, gemm_skinny.hip
int launch_gemm(const GemmArgs& a, int dtype, hipStream_t s);
// The instantiation launch_gemm starts for these arguments: the one place that decides it (host only, launches nothing, any of the
// three dtypes); DSIM_ERR_INVALID where launch_gemm would refuse them
int gemm_plan(const GemmArgs& a, int dtype, GemmLaunchRec* plan);
int gemm_fill_extents(GemmArgs& g, size_t es);                       // operand byte extents for the buffer descriptors
// small-batch kernel (gemm_skinny.hip): same arithmetic, deep ring; g prepared by launch_gemm, the tile / mode / epilogue from its plan
int launch_gemm_skinny(const GemmArgs& g, const GemmLaunchRec& plan, hipStream_t s);
int gemm_band_width(int tilesM, int tilesN, size_t w_tile_bytes);   // tile-order band width (L2 reuse of the weight tiles)

// row-resident Linear and fused feed-forward -- rowres.hip
size_t rowlin_stream_bytes(int C, int N);       // 0: shape not covered
int pack_rowlin_stream(const void* w_packed /*[N][C] h16*/, void* stream, int C, int N, hipStream_t s);
int launch_rowlin(const RowLinArgs& a, hipStream_t s);
size_t ff_stream_bytes(int C);                  // 0: no fused kernel for this width
// w1_packed: the GEGLU-interleaved [8C][C] h16 weight (pack_linear with geglu_interleave = 1); w2_packed: [C][4C] h16
int pack_ff_stream(const void* w1_packed, const void* w2_packed, void* stream, int C, hipStream_t s);
int launch_ff_fused(const FFArgs& a, hipStream_t s);

// attention -- attention.hip; the fused score tail of any shape -- tails.hip
int launch_attention(const AttnArgs& a, int dtype, hipStream_t s);
const char* attention_kernel_kind(const AttnArgs& a, int dtype);      // "_p160" / "_short" / "_long" / "_q2" / "_q2fast" / "_fast" / "": the kernel it picks
// the dsim_attn_kind launch_attention would start for these arguments (host only, launches nothing); DSIM_ERR_INVALID where it
// would refuse them
int attention_plan(const AttnArgs& a, int dtype);
// the pair launchers (PairArgs, common.h) serve this shape; tiled = false: for a persistent grid (pair_args_check, common.h, asks)
bool pair_shape_served(int n_pairs, int B, int H, int N, int D, bool tiled = true);
size_t pair_score_scratch_bytes(int n_pairs, int B, int H, int N, int D);
int launch_pair_score(const PairArgs& a, int dtype, float* out, int32_t* status, hipStream_t s);      // status may be NULL
// the score tail at SD1.5's default tap (256 tokens, head dim 160, 16-bit types): persistent workgroups, K / V streamed once per
// 256 queries through an LDS-DMA ring -- attn160.hip
bool pair_score160_applies(int N, int D, int dtype);
size_t pair_score160_scratch_bytes(int n_pairs, int B, int H);
int launch_pair_score160(const PairArgs& a, float* out, int32_t* status, hipStream_t s);
// similarity maps: the score tail kept per query token (pair_map_kernel: pair_tail_kernel's body with a per-token epilogue, any
// shape and dtype) -- tails.hip
//   score [n_pairs]; local, contrib (each may be NULL) [n_pairs][2][N]; status (may be NULL) [n_pairs]
size_t pair_score_maps_scratch_bytes(int n_pairs, int B, int H, int N);
int launch_pair_score_maps(const PairArgs& a, int dtype, float* score, float* local, float* contrib, int32_t* status, hipStream_t s);
// token alignments: softmax(Q_a K_b^T / sqrt(D)) averaged over the CFG halves and heads, per query token its argmax, weight and
// soft-argmax position, and on request the probabilities (align_stats_kernel + align_kernel, any shape and dtype) -- align.hip
//   match, weight [n_pairs][2][N]; expect [n_pairs][2][N][2]; attn [n_pairs][2][N][N]; status [n_pairs]; each may be NULL
size_t pair_align_scratch_bytes(int n_pairs, int B, int H, int N, int D);      // 0: shape not served
int launch_pair_align(const PairArgs& a, int dtype, int grid_w, int32_t* match, float* weight, float* expect, float* attn,
                      int32_t* status, hipStream_t s);
// region scores: the score tail restricted to a token region per feature image (mask [n_feat][N] bytes, non-zero = on): the
// tail's arithmetic on the regions' rows, taken through ascending token lists built on the device -- regions.hip
//   out [n_pairs]; status (may be NULL) [n_pairs]: 0, 1 non-finite, 2 empty region; counts (may be NULL) [n_feat]
size_t pair_score_regions_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);      // 0: call not served
int launch_pair_score_regions(const PairArgs& a, int dtype, const uint8_t* mask, int n_feat, float* out, int32_t* status,
                              int32_t* counts, hipStream_t s);
// the masks [n_feat][N] as ascending token lists [n_feat][N] and counts [n_feat] (also to counts, unless NULL): region_lists_kernel
int launch_region_lists(const uint8_t* mask, int n_feat, int N, int32_t* list, int32_t* cnt, int32_t* counts, hipStream_t s);
// soft region scores: the region score with a byte weight per token (weights [n_feat][N], w = byte / 255) -- a weight-0 token is
// dropped, a listed key's logit carries the bias ln w, a query row's terms the factor w -- soft_regions.hip
//   out [n_pairs]; status (may be NULL) [n_pairs]: 0, 1 non-finite, 2 an image of byte sum 0; weight_sums (may be NULL) [n_feat]
size_t pair_score_weights_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);      // 0: call not served
int launch_pair_score_weights(const PairArgs& a, int dtype, const uint8_t* weights, int n_feat, float* out, int32_t* status,
                              int32_t* weight_sums, hipStream_t s);
// region maps: launch_pair_score_maps' outputs for the region score -- the region tail kept per query token, on the full token grid,
// zeros at the off tokens -- region_maps.hip
//   score [n_pairs]; local, contrib (each may be NULL) [n_pairs][2][N]; status (may be NULL): 0, 1 non-finite, 2 empty region
size_t pair_score_maps_regions_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);      // 0: call not served
int launch_pair_score_maps_regions(const PairArgs& a, int dtype, const uint8_t* mask, int n_feat, float* score, float* local,
                                   float* contrib, int32_t* status, int32_t* counts, hipStream_t s);
// region alignments: launch_pair_align's outputs with the softmax over the key image's region only, on the full token grid; off query
// tokens carry match -1, weight 0, expect (-1, -1) and attn is zero outside R_a x R_b -- region_maps.hip
//   status (may be NULL) [n_pairs]: 0, 1 non-finite probability, 2 empty region; counts (may be NULL) [n_feat]
size_t pair_align_regions_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);      // 0: call not served
int launch_pair_align_regions(const PairArgs& a, int dtype, const uint8_t* mask, int n_feat, int grid_w, int32_t* match, float* weight,
                              float* expect, float* attn, int32_t* status, int32_t* counts, hipStream_t s);
// region score matrix: cell (i, j) is the region score of (A_i over mask_a[i], B_j over mask_b[j]); each image's self attention over
// its region once, at compacted positions, then one listed attention per cell and direction -- region_matrix.hip
//   out [n_a][n_b]; status (may be NULL) [n_a][n_b]: 0, 1 non-finite, 2 empty region; counts (may be NULL) [n_a + n_b]
size_t score_matrix_regions_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype);      // 0: call not served
int launch_score_matrix_regions(const MatrixArgs& a, int dtype, float* out, int32_t* status, int32_t* counts, hipStream_t s);
// soft score matrix: cell (i, j) is the soft region score of (A_i, B_j) with a.mask as the two sets' weight bytes -- the region
// matrix's launches with weighted rows -- soft_matrix.hip
//   out [n_a][n_b]; status (may be NULL) [n_a][n_b]: 0, 1 non-finite, 2 an image of byte sum 0; weight_sums (may be NULL) [n_a + n_b]
size_t score_matrix_weights_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype);      // 0: call not served
int launch_score_matrix_weights(const MatrixArgs& a, int dtype, float* out, int32_t* status, int32_t* weight_sums, hipStream_t s);
// soft region maps and soft region alignments: the two region forms above with a byte weight per token (weights [n_feat][N]) -- the
// soft tail's biased attentions per query token, the finish applying the query weight; the alignments' softmax with the key image's
// biases -- soft_maps.hip
//   status (may be NULL) [n_pairs]: 0, 1 non-finite, 2 an image of byte sum 0; weight_sums (may be NULL) [n_feat]
size_t pair_score_maps_weights_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);      // 0: call not served
int launch_pair_score_maps_weights(const PairArgs& a, int dtype, const uint8_t* weights, int n_feat, float* score, float* local,
                                   float* contrib, int32_t* status, int32_t* weight_sums, hipStream_t s);
size_t pair_align_weights_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);      // 0: call not served
int launch_pair_align_weights(const PairArgs& a, int dtype, const uint8_t* weights, int n_feat, int grid_w, int32_t* match, float* weight,
                              float* expect, float* attn, int32_t* status, int32_t* weight_sums, hipStream_t s);
// region transfer: the attention mass each token sends into the other image's weighted tokens, sum_j Pm[i][j] w[j] with launch_pair_align's
// Pm (softmax over all keys; weights [n_feat][N] bytes, w = byte / 255, in the sum only), in one pass over the keys without Pm or
// statistics (transfer_part_kernel + transfer_fold_kernel, any shape and dtype) -- transfer.hip
//   directions 1: rows [p][0], 2: rows [p][1], 3: both; mass [n_pairs][2][N] (rows not asked for are not written); status (may be NULL)
size_t pair_region_transfer_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D);      // 0: call not served
int launch_pair_region_transfer(const PairArgs& a, int dtype, const uint8_t* weights, int n_feat, int directions, float* mass,
                                int32_t* status, hipStream_t s);
// transfer matrix: launch_pair_region_transfer's mirror row for every cell (A_i, B_j) of two sets, a.mask[0] set A's weight bytes
// (a.q[1], a.k[0] are what it reads) -- transfer_matrix.hip
//   mass [n_a][n_b][N]; status (may be NULL) [n_a][n_b]
size_t region_transfer_matrix_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype);      // 0: call not served
int launch_region_transfer_matrix(const MatrixArgs& a, int dtype, float* mass, int32_t* status, hipStream_t s);
// cell-region score matrices: the region / soft matrix with set B's rows per cell, a.mask[1] [n_a][n_b][N]; set A's self attention
// once per image, set B's with the cell's cross attention in one workgroup -- cell_matrix.hip
//   out [n_a][n_b]; status (may be NULL) [n_a][n_b]: 0, 1, 2; counts / weight_sums (may be NULL) [n_a + n_a n_b]
size_t score_matrix_cell_regions_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype);      // 0: call not served
int launch_score_matrix_cell_regions(const MatrixArgs& a, int dtype, float* out, int32_t* status, int32_t* counts, hipStream_t s);
size_t score_matrix_cell_weights_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype);      // 0: call not served
int launch_score_matrix_cell_weights(const MatrixArgs& a, int dtype, float* out, int32_t* status, int32_t* weight_sums, hipStream_t s);
// text attention maps: the tapped block's cross-attention on the conditional CFG half, averaged over the heads; its weighted sum over
// the prompt tokens (saliency) and the token region above rel_threshold x the image's mean saliency (text_attn_kernel,
// text_region_kernel, any head dim and dtype, 1 <= L <= 128) -- textattn.hip
//   xq [n_images][2][N] rows of ldq; xk [n_kv][L] rows of ldk (n_kv = 2 or 2 n_images); weight f32 [n_w][L] (n_w = 1 or n_images)
//   attn [n_images][N][L]; saliency [n_images][N]; mask [n_images][N] bytes; counts, status [n_images]; each may be NULL
size_t text_attention_scratch_bytes(int n_images, int N, int L);      // 0: shape not served
int launch_text_attention(const void* xq, int ldq, const void* xk, int ldk, int n_images, int n_kv, int H, int N, int L, int D, int dtype,
                          const float* weight, int n_w, float rel_threshold, float* attn, float* saliency, uint8_t* mask, int32_t* counts,
                          int32_t* status, void* scratch, size_t scratch_bytes, hipStream_t s);
// the same core as a plain SDPA (256 queries = 256 keys, head dim 160, 16-bit types): the U-Net's 16 x 16-level self-attentions
bool sdpa160_applies(const AttnArgs& a);
int launch_sdpa160(const AttnArgs& a, hipStream_t s);
// score matrix (every image of set A against every image of set B; q, k, v of a set: [n][B][N][H*D]): the self attentions once per
// image into the workspace, then two cross attentions per cell -- tails.hip (any shape), attn160.hip (the default tap, 16-bit).
// The launchers take MatrixArgs (common.h).  matrix_shape_served: the one answer to which matrix calls are served, for the workspace
// queries (0 exactly where it refuses), the launchers and the entry points (matrix_args_check, common.h); listed: the region matrix
bool matrix_shape_served(int n_a, int n_b, int B, int H, int N, int D, int dtype, bool listed);
size_t score_matrix_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype);      // 0: call not served
int launch_score_matrix(const MatrixArgs& a, int dtype, float* out, int32_t* status, hipStream_t s);
size_t score_matrix160_scratch_bytes(int n_a, int n_b, int B, int H);
int launch_score_matrix160(const MatrixArgs& a, float* out, int32_t* status, hipStream_t s);
