/*
 * sfcvit.h -- C ABI of the MI355X (gfx950) SFC-ViT hot path.
 *
 * The reference (RemcoHoger/Space-Filling-Curves-for-Vision-Transformers) is pure
 * Python on PyTorch and has no FFI of its own: these entry points
 * are what a binding for the path would bind.  Each one names the reference
 * interface it replaces (paths relative to the reference root; `torch:` = the
 * installed torch the reference calls into).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.  Unless marked HOST every
 *     pointer is a device (HBM) pointer and must be 16-byte aligned.
 *   - bf16 tensors are passed as `const void*` to raw bf16 bits, row-major.
 *   - `stream` is a hipStream_t (NULL = default stream).  No entry point
 *     synchronises, allocates or copies to the host: all are graph-capturable.
 *   - return value: 0 = launched / done, nonzero = rejected (see sfcvit_last_error()).
 *     Nothing is launched when an argument check fails.
 *   - inputs are never written; outputs are fully overwritten.
 */
#ifndef SFCVIT_H
#define SFCVIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFCVIT_ABI_VERSION 1

enum sfcvit_status {
    SFCVIT_OK = 0,
    SFCVIT_EINVAL = 1,   /* bad argument (shape, alignment, enum) */
    SFCVIT_ELAUNCH = 2,  /* HIP reported an error at launch */
    SFCVIT_ENODEV = 3    /* no usable gfx950 device */
};

int sfcvit_abi_version(void);
/* HOST: message of the last failing call on this thread ("" if none). */
const char *sfcvit_last_error(void);
/* HOST: number of visible HIP devices, <0 on error (does not create a context). */
int sfcvit_device_count(void);

/* ------------------------------------------------------------------------
 * Curve index tables (host, integer, bit-exact with the reference)
 * ---------------------------------------------------------------------- */
enum sfcvit_curve {
    SFCVIT_CURVE_HILBERT = 0, /* src/curves/space_filling_curves.py:168-202 */
    SFCVIT_CURVE_Z = 1,       /* :134-165 */
    SFCVIT_CURVE_MOORE = 2,   /* :205-251 */
    SFCVIT_CURVE_PEANO = 3,   /* :74-131  */
    SFCVIT_CURVE_RASTER = 4,  /* identity order (RasterScan1DEmbedding, zigzag_embedding1D.py:30-39) */
    SFCVIT_CURVE_SPIRAL = 5,  /* inward spiral from the bottom-left cell: OnionEmbedding1D.onion_indices,
                                 src/tokenizers/_1D/onion_embedding1D.py:35-53 = multiscale/multi_onion.py:68-87 */
    SFCVIT_CURVE_HILBERT_T = 6 /* the private generator of _2D/HilbertEmbedding (src/tokenizers/_2D/
                                 hilbert_embedding.py:30-78): Hilbert without the (x,y) swap; n a power of two */
};

/* HOST. embed_and_prune_sfc(curve, n, n) (space_filling_curves.py:471-491) as the
 * flat table r*n+c that SFCEmbedding1D._sfc_indices builds (multi_hilbert.py:68-72).
 * out_flat: n*n int32. */
int sfcvit_curve_table(int curve, int n, int32_t *out_flat);
/* HOST. Same points as (row, col) int64 pairs: the `hilbert_indices` / `z_indices`
 * buffers of HilbertEmbedding1D / MortonEmbedding1D (hilbert_embedding1D.py:20-28).
 * out_rc: n*n*2 int64. */
int sfcvit_curve_table_rc(int curve, int n, int64_t *out_rc);

/* HOST. Per-token pixel offsets for the fused tokenizer kernel.
 * Token t of SFCEmbedding1D(img, p, g) (multi_hilbert.py:74-84) is made of
 * P = g*p*p pixels; pixel kk = gi*p*p + p1*p + p2 is at
 * (row, col) = ((flat[t*g+gi] / grid)*p + p1, (flat[t*g+gi] % grid)*p + p2), grid = img/p.
 * The 1-D tokenizers are the case p = 1, g = patch_size with `flat` = r*img+c.
 * flat: grid*grid int32 (curve table); out_pix: (grid*grid/g) * P int32 = img*img entries. */
int sfcvit_pixel_table(const int32_t *flat, int img, int p, int g, int32_t *out_pix);

/* ------------------------------------------------------------------------
 * Fused SFC gather + patchify + linear projection
 *   replaces HilbertEmbedding1D.forward / MortonEmbedding1D.forward
 *   (src/tokenizers/_1D/hilbert_embedding1D.py:30-44), RasterScan1DEmbedding.forward
 *   (zigzag_embedding1D.py:30-39) and SFCEmbedding1D.forward (multi_hilbert.py:74-84).
 * ---------------------------------------------------------------------- */
typedef struct sfcvit_patch_embed_args {
    const void *x;      /* [B, C, H*W] image, fp32 (x_is_bf16 = 0) or bf16 */
    const int32_t *pix; /* [N, P] pixel offsets (sfcvit_pixel_table), device copy */
    const void *w;      /* [D, P*C] bf16, feature index = kk*C + c (reference layout) */
    const void *bias;   /* [D] bf16 or NULL */
    void *y;            /* fwd: out [B*N, D] bf16 ; bwd: in, dY [B*N, D] bf16 */
    void *dw;           /* bwd: out [D, P*C] fp32 */
    void *dbias;        /* bwd: out [D] fp32 (NULL = skip) */
    void *workspace;    /* sfcvit_patch_embed_workspace(...) bytes, 16-byte aligned */
    int64_t workspace_bytes;
    int32_t B, C, HW, N, P, D; /* N*P = H*W; D a multiple of 8; P*C arbitrary (padded to 8 inside; the
                                  vectorised table reads need P % 8 == 0, other P take a scalar gather) */
    int32_t x_is_bf16;
    /* Optional tile descriptor (device copy of what sfcvit_tile_descriptors wrote; NULL = generic kernels).  With it,
     * P = 256 and D % 256 == 0 the forward runs the tiled kernel (csrc/patch_embed_tiled.hip: whole 16-pixel row
     * segments loaded with 16-byte vectors straight into the LDS tile, the intra-tile curve order folded into a
     * per-class permuted weight).  desc_ncls / desc_cnt = its classes and tokens per class (host copies);
     * the forward workspace must then hold desc_ncls * D * C * 256 bf16. */
    const int32_t *desc;
    int32_t desc_ncls;
    int32_t desc_cnt[8];
} sfcvit_patch_embed_args;

/* HOST: analyse a pixel table (host copy of sfcvit_pixel_table's output): > 0 = number of int32 written to `desc`
 * (every token is a 16 x 16 pixel tile or a strip of 256 consecutive pixels), 0 = not tileable, < 0 = error.
 * Capacity 16 + 2 N + 2 * 8 * 256 always suffices. */
int sfcvit_tile_descriptors(const int32_t *pix, int N, int P, int img_w, int32_t *desc, int capacity);

/* HOST: workspace bytes for fwd (bwd = 0) / bwd (bwd = 1). */
int64_t sfcvit_patch_embed_workspace(int B, int C, int N, int P, int D, int bwd);

int sfcvit_patch_embed_fwd(const sfcvit_patch_embed_args *a, void *stream);
/* The gather alone: tokens[b * N + n][kk * C + c] = bf16(x[b, c, pix[n][kk]]) -- the reference's
 * `x_flat[:, :, perm].reshape(B, N, P * C)` (src/tokenizers/_1D/hilbert_embedding1D.py:36-41) as one pass: the image is read
 * once (every 16 x 16 tile of a Hilbert / Z token by one workgroup), rows are written whole.  tokens is [B * N, ld] bf16 with
 * ld >= P * C, ld % 8 == 0 (columns P * C .. ld - 1 are zeroed).  order (device, [N], or NULL) = the tokens sorted by their
 * lowest pixel offset: workgroups then take horizontally adjacent 16 x 16 tiles in pairs, whose 64-byte rows share
 * 128-byte lines (a performance hint only; any permutation of 0 .. N - 1 gives the same tokens).  Two-stage patch embed = this + sfcvit_gemm (round 3: at
 * ViT-B the persistent GEMMs run the projection and its weight gradient 2-3x faster than the fused gather kernels). */
int sfcvit_tokens_gather(const void *x, int x_is_bf16, const int32_t *pix, const int32_t *order, int B, int C, int HW, int N, int P,
                         void *tokens, int ld, void *stream);
/* The same tokens for pixel tables whose tokens are 16 x 16 pixel tiles of an fp32 image (sfcvit_tile_descriptors mode 1:
 * every Hilbert / Z tokenizer at 256 pixels per token): whole 128-byte image lines by 16-byte loads, the curve order applied on
 * the way out of LDS (round 4; csrc/patch_embed.hip tokens_gather_tiles_kernel).  origin (device, [N]) = flat offset of each
 * token's top-left pixel (descriptor words [16 + N, 16 + 2 N)); order as above; ld must be 256 * C, 1 <= C <= 4, x fp32. */
int sfcvit_tokens_gather_tiles(const void *x, const int32_t *pix, const int32_t *order, const int32_t *origin, int B, int C, int H,
                               int W, int N, void *tokens, int ld, void *stream);
/* dW = sum_{b,t} dY[b,t,:]^T tokens[b,t,:] with the tokens re-gathered from x
 * (nothing but x is saved for backward); the image receives no gradient. */
int sfcvit_patch_embed_bwd(const sfcvit_patch_embed_args *a, void *stream);

/* ------------------------------------------------------------------------
 * MixUp / CutMix on the device
 *   replaces mixup_data / cutmix_data (src/training/train.py:7-47) and the soft-target construction + accuracy
 *   bookkeeping of train_with_mixup_or_cutmix (train.py:148-172).
 *
 * One batch's mix is described by two DEVICE buffers, so that a captured graph picks up new values on every replay:
 *   perm  int32[B]: the partner image of each image (the reference's `idx`).  An entry outside [0, B) means "no
 *         partner" (the image itself): no kernel reads outside the batch whatever the buffer holds.
 *   rec   eight 32-bit words, 16-byte aligned:
 *         [0] mode: 0 = none, 1 = MixUp, 2 = CutMix
 *         [1] r0 [2] r1 [3] c0 [4] c1: the CutMix box [r0, r1) x [c0, c1) on tensor dims 2 and 3
 *         [5] lam  [6] 1 - lam: fp32 bit patterns; 1 - lam is formed on the host in double and rounded once, which is
 *             what torch does with the Python scalar `1 - lam`
 *         [7] reserved (0)
 *   The reference's quirk is kept: rand_bbox derives bbx* from W and bby* from H, and cutmix_data then applies bbx to
 *   dim 2 (rows) and bby to dim 3 (columns) (train.py:41-42).  The record stores the box AS IT IS APPLIED -- r = bbx,
 *   c = bby -- not as it is named.
 * Per pixel of image b, with q = perm[b]:
 *   MixUp   fadd(fmul(lam, x[b]), fmul(1 - lam, x[q])): three separately rounded fp32 operations, never a fused
 *           multiply-add (bit-identical to torch's lam * x + (1 - lam) * x[idx])
 *   CutMix  x[q] inside the box, x[b] outside; the source is the un-mixed batch, so cycles in perm are exact
 *   mode 0  x[b]
 * Images are fp32.
 * ---------------------------------------------------------------------- */
/* sfcvit_tokens_gather / sfcvit_tokens_gather_tiles with the mix applied on the way to bf16: tokens[b * N + n][kk * C + c] =
 * bf16(mix(x)[b, c, pix[n][kk]]) -- one more read of the image, no extra pass, and backward (which keeps the tokens) is
 * unchanged.  origin != NULL: the 16 x 16-tile kernel (P must be 256 and the arguments those of sfcvit_tokens_gather_tiles;
 * a wave loads the partner's lines next to the image's own, and a tile pair the box does not touch loads no partner);
 * origin == NULL: the per-pixel kernels (any P; ld as in sfcvit_tokens_gather).  Mode 0 gives the unmixed gather's bits. */
int sfcvit_tokens_gather_mix(const void *x, const int32_t *pix, const int32_t *order, const int32_t *origin, const int32_t *perm,
                             const uint32_t *rec, int B, int C, int H, int W, int N, int P, void *tokens, int ld, void *stream);
/* out[B, C, H, W] = the mixed batch (fp32 in and out): one read of x[b] and x[perm[b]], one write, 16-byte accesses when
 * H * W % 4 == 0.  For the paths that never materialise tokens (the fused gather-GEMM kernels, the hierarchical kernel, the
 * Conv2d-weight tokenizers, altvit).  out must not overlap x. */
int sfcvit_mix_images(const void *x, const int32_t *perm, const uint32_t *rec, void *out, int B, int C, int H, int W, void *stream);
/* sfcvit_soft_ce on the targets lam * onehot(y_a) + (1 - lam) * onehot(y_b) without building them: y_a, y_b int64 [B]
 * (device), lam / 1 - lam from rec (mode 0: lam = 1).  Same max / sum-of-exponentials loop as sfcvit_soft_ce, so the same
 * lse; where y_a == y_b the single target is fadd(lam, 1 - lam), as the dense row holds.  loss_rows, dlogits (may be NULL)
 * as in sfcvit_soft_ce.  hit_rows (fp32 [B] or NULL) = lam * (argmax == y_a) + (1 - lam) * (argmax == y_b), the lowest
 * index winning ties: per row, no atomics, so an epoch's sum is the same from run to run.  A label outside [0, C) is a
 * label without a target: it adds nothing to loss, gradient or hits, and nothing is read or written through it. */
int sfcvit_soft_ce_pair(const void *logits, const int64_t *y_a, const int64_t *y_b, const uint32_t *rec, float *loss_rows,
                        void *dlogits, float *hit_rows, int B, int C, int ld, float gscale, void *stream);

/* ------------------------------------------------------------------------
 * Train / test image transforms on the device: uint8 batch in, normalized images out
 *   replaces the per-sample transform stack of the reference's loaders (main.py:169-188):
 *     train  RandomResizedCrop(size) -> RandomHorizontalFlip -> ColorJitter(0.4, 0.4, 0.4, 0.1) -> ToImage /
 *            ToDtype(float32, scale=True) -> RandomErasing(p=0.2) -> Normalize(mean, std)
 *     test   ToDtype -> Normalize
 *   in two steps: a HOST draw of one 16-word record per image (plain C++, no HIP), and ONE capturable launch that
 *   reads the uint8 batch [B, C, H, W] and the device copy of the records and writes the augmented, scaled,
 *   normalized batch [B, C, S, S] (fp32 or bf16).
 *
 * Record, 16 words of 32 bits per image:
 *   [0]      flags: bit 0 flip, bit 1 erase, bits 2-5 = brightness / contrast / saturation / hue enabled
 *   [1..4]   crop top, left, h, w (ints, inside the H x W source)
 *   [5]      jitter order: four 2-bit fields, field i = the op applied i-th (0 brightness, 1 contrast, 2 saturation,
 *            3 hue), a permutation of 0..3
 *   [6..9]   brightness, contrast, saturation, hue factors (fp32 bit patterns)
 *   [10..13] erase top, left, h, w on the S x S OUTPUT grid
 *   [14..15] 0
 * Every random number of the draw is a pure function of (seed, step, sample_base + b, draw index), so a sample's
 * record does not depend on batch size, rank or call order (csrc/augment.cpp states the stream).
 * ---------------------------------------------------------------------- */
#define SFCVIT_AUG_WORDS 16
#define SFCVIT_AUG_FLAGS 0
#define SFCVIT_AUG_CROP 1
#define SFCVIT_AUG_ORDER 5
#define SFCVIT_AUG_FACTORS 6
#define SFCVIT_AUG_ERASE 10
#define SFCVIT_AUG_FLIP_BIT 1u
#define SFCVIT_AUG_ERASE_BIT 2u
#define SFCVIT_AUG_JITTER_SHIFT 2     /* flags bit (2 + op) = op enabled */
#define SFCVIT_AUG_ORDER_IDENTITY 0xE4u

typedef struct sfcvit_augment_cfg {
    int32_t S;            /* output size (S x S); the apply needs S >= H and S >= W (upsampling or identity) */
    int32_t crop;         /* draw a RandomResizedCrop box (0 = the whole image) */
    int32_t flip;         /* draw a horizontal flip with probability 1/2 */
    int32_t out_is_bf16;  /* output dtype of the apply: 0 fp32, 1 bf16 (round to nearest even) */
    double scale[2];      /* crop: area fraction range, torchvision's default (0.08, 1) */
    double ratio[2];      /* crop: aspect range, default (3/4, 4/3) */
    double brightness, contrast, saturation, hue;   /* ColorJitter ranges; 0 disables the op */
    double erase_p;       /* RandomErasing probability; 0 disables it (area 0.02-0.33 of S x S, aspect 0.3-3.3) */
    float mean[3], std[3]; /* Normalize, per channel (the apply refuses a zero std) */
} sfcvit_augment_cfg;

/* HOST. Fills rec_host[B * 16] for samples sample_base .. sample_base + B - 1 of step `step`.  Every switch off
 * (a zeroed cfg with S = H = W) gives the test transform's record: flags 0, the whole image, identity order. */
int sfcvit_augment_draw(uint32_t *rec_host, int B, int H, int W, const sfcvit_augment_cfg *cfg, uint64_t seed, uint64_t step,
                        int64_t sample_base);
/* x uint8 [B, C, H, W], rec_dev the device copy of the records, out [B, C, S, S] fp32 or bf16; cfg is a HOST pointer
 * read before the call returns.  Per output pixel, in fp32 on v / 255: bilinear crop + resize (align_corners = False,
 * taps inside the crop box, the output column mirrored under flip), the jitter ops in the record's order (contrast
 * blends with the image's gray mean AS IT STANDS before that op: a per-image reduction in a fixed order, so two runs
 * give the same bits), the erase box set to 0, (x - mean) / std.  1 <= C <= 3, and C == 3 when a colour op is enabled.
 * A record that was never filled in is clamped into the image: no read leaves the batch whatever the buffer holds. */
int sfcvit_augment_apply(const uint8_t *x, const uint32_t *rec_dev, void *out, int B, int C, int H, int W,
                         const sfcvit_augment_cfg *cfg, void *stream);

/* ------------------------------------------------------------------------
 * Fused hierarchical tokenizer, forward
 *   replaces HierarchicalHilbertEmbedding.forward (src/tokenizers/multiscale/multi_hilbert.py:31-40) and its
 *   siblings multi_morton.py / multi_moore.py / multi_peano.py / multi_onion.py / multi_zigzag.py (same lines) when
 *   every level has the same token count N (true of every configuration the reference ships, main.py:269-274; the
 *   F.interpolate(mode='linear') to N tokens is then the identity):
 *       h[m, l*D:(l+1)*D] = bf16( W_l tokens_l[m, :] + b_l )      level l = SFCEmbedding1D (multi_hilbert.py:74-84)
 *       y[m, :]           = bf16( Wf h[m, :] + bf )               fusion  = nn.Linear(L*D, L*D)
 *   in ONE kernel: tokens gathered through the per-level pixel tables, level outputs kept in LDS as the A operand
 *   of the fusion GEMM.  h is also written out (the fusion weight gradient needs it); backward composes
 *   sfcvit_gemm (dh, dWf) and sfcvit_patch_embed_bwd per level.
 *   wf = NULL: the kernel stops after the first line -- gather + every level projection + the concatenation (each
 *   level writes its own columns of h; no torch.cat pass) -- and the caller runs the fusion Linear as sfcvit_gemm.
 *   That pair is the faster one at the reference's shape (the all-in-one kernel re-streams Wf once per
 *   64 token rows and is bound by L2 -> CU delivery); both are kept, bit-identical in h.
 * ---------------------------------------------------------------------- */
#define SFCVIT_HIER_MAX_LEVELS 4
typedef struct sfcvit_hier_args {
    const void *x;                               /* [B, C, H*W] image, fp32 (x_is_bf16 = 0) or bf16 */
    const int32_t *pix[SFCVIT_HIER_MAX_LEVELS];  /* level l: [N, P[l]] pixel offsets (sfcvit_pixel_table), device */
    const void *w[SFCVIT_HIER_MAX_LEVELS];       /* level l: [D, P[l]*C] bf16, feature index kk*C + c, 16-byte aligned */
    const void *b[SFCVIT_HIER_MAX_LEVELS];       /* level l: [D] bf16 or NULL */
    const void *wf;                              /* [L*D, L*D] bf16; NULL = levels + concatenation only (y unused) */
    const void *bf;                              /* [L*D] bf16 or NULL */
    void *h;                                     /* out [B*N, L*D] bf16: concatenated level outputs */
    void *y;                                     /* out [B*N, L*D] bf16 */
    int32_t P[SFCVIT_HIER_MAX_LEVELS];           /* pixels per token of level l; N * P[l] = H*W for every level */
    int32_t B, C, HW, N, L, D;
    int32_t x_is_bf16;
} sfcvit_hier_args;

/* HOST: 1 if (L, D, C, P[0..L)) is inside the fused kernel's envelope: 1..4 levels, D % 64 == 0, L*D % 256 == 0,
 * P[l]*C % 8 == 0, and 64 rows of (L*D + sum of P[l]*C) bf16 fit the 160 KiB LDS; else 0 (compose the level calls). */
int sfcvit_hier_tokenizer_supported(int L, int D, int C, const int32_t *P);
/* SFCVIT_EINVAL outside that envelope or when the levels do not share the token count. */
int sfcvit_hier_tokenizer_fwd(const sfcvit_hier_args *a, void *stream);
/* Levels with different token counts: the reference resamples every coarser level to the first level's length with
 * F.interpolate(mode="linear", align_corners=False) and concatenates on the feature axis
 * (src/tokenizers/multiscale/multi_hilbert.py:33-38).  Both in one pass over bf16 level outputs:
 *   levels[l] (device) = y_l [B, n_tokens[l], D];  out = [B, N0, L * D], N0 = n_tokens[0];  `levels` / `n_tokens` are HOST arrays.
 * _bwd: dlevels[l] [B, n_tokens[l], D] = the transposed resampling of dout's column block l (fixed summation order). */
int sfcvit_hier_resample_concat(const void *const *levels, const int32_t *n_tokens, int L, int B, int N0, int D, void *out, void *stream);
int sfcvit_hier_resample_concat_bwd(const void *dout, const int32_t *n_tokens, int L, int B, int N0, int D, void *const *dlevels,
                                    void *stream);
/* HOST: name of the tokenizer kernel the calling thread launched last through any entry point of the three sections above
 * (patch embed, token gathers, hierarchical tokenizer), "none" before any -- what rocprofv3 would show, for tests that must
 * know which path ran: pe_fwd_kernel<fp32|bf16>, pe_bwd_kernel<..>, pe2_fwd_kernel<..>, pe2_bwd_kernel<..> (the tiled
 * forms; sfcvit_patch_embed_fwd / _bwd run the generic ones without a descriptor, or when P, D or its class count do not
 * fit), tokens_gather_kernel<fp32|bf16|mix>, tokens_gather_p256_kernel<..>, tokens_gather_tiles_kernel<C, fp32|mix>,
 * hier_fwd_kernel<fp32|bf16, fuse|levels>, hier_resample_concat_kernel, hier_resample_concat_bwd_kernel.  The helper
 * launches (weight permutation, split reduction, column sum) are not named.  SFCVIT_EINVAL for a null buffer or n <= 0. */
int sfcvit_last_tokenizer_kernel(char *buf, int n);

/* ------------------------------------------------------------------------
 * bf16 MFMA GEMM with fused epilogue
 *   replaces nn.Linear forward/backward at every site of the path:
 *   in_proj / out_proj (torch:nn/functional.py:5822-5833,6632-6637), linear1/linear2
 *   (torch:nn/modules/transformer.py:980-982), MixerBlock.channel_mix (src/models/vit.py:262-266),
 *   FactorisedLinear's two einsums (vit.py:289-292) and the classifier (vit.py:319).
 *
 *   C[M,N] = epilogue( sum_k A(m,k) * B(n,k) )
 *   a_kmajor = 0: A is [M, lda] with k contiguous;  1: A is [K, lda] with m contiguous
 *   b_kmajor = 0: B is [N, ldb] with k contiguous;  1: B is [K, ldb] with n contiguous
 *   epilogue, in this order (fp32):  v += bias[n];  aux_out[m,n] = bf16(v);
 *   v = act(v);  v = dropout(v);  v += residual[m,n];  v *= dact(aux_in[m,n]) * dact_scale;  C[m,n] = v
 * ---------------------------------------------------------------------- */
enum sfcvit_act { SFCVIT_ACT_NONE = 0, SFCVIT_ACT_RELU = 1, SFCVIT_ACT_GELU = 2 };
/* dact: 0 none; RELU: (aux_in > 0); GELU: gelu'(aux_in) (erf form, nn.GELU default) */

typedef struct sfcvit_gemm_args {
    const void *a, *b;
    void *c;
    const void *bias;      /* [N] bf16 or NULL */
    const void *residual;  /* [M, ldr] bf16 or NULL */
    const void *aux_in;    /* [M, ldaux] bf16, needed when dact != 0 */
    void *aux_out;         /* [M, ldaux] bf16 or NULL */
    int32_t M, N, K;
    int32_t lda, ldb, ldc, ldr, ldaux;
    int32_t a_kmajor, b_kmajor;
    int32_t act, dact;
    int32_t c_is_f32;      /* 0: C is bf16, 1: C is fp32 */
    int32_t splitk;        /* >1: split K over that many workgroups per tile (weight-gradient
                              shapes); needs `workspace`, allows no epilogue */
    void *workspace;       /* fp32 slabs, sfcvit_gemm_workspace(M, N, splitk) bytes */
    int64_t workspace_bytes;
    int32_t force_generic; /* kernel choice, for tests and benchmarks: 0 = automatic (persistent 8-phase kernel when
                              both operands are k-contiguous and the shape sits on its tile grid, else the LDS-DMA
                              ring kernel, else the generic 128 x 128 kernel); 1 = generic only; 4 / 6 / 7 = ring
                              kernel (heuristic / 256 x 128 / 256 x 256); 8 / 9 / 10 = persistent kernel with
                              256- / 224- / 192-row tiles (EINVAL when not eligible); SFCVIT_GEMM_* below */
#define SFCVIT_GEMM_AUTO 0
#define SFCVIT_GEMM_GENERIC 1
#define SFCVIT_GEMM_RING 4
#define SFCVIT_GEMM_RING_256x128 6
#define SFCVIT_GEMM_RING_256x256 7
#define SFCVIT_GEMM_P8_256 8
#define SFCVIT_GEMM_P8_224 9
#define SFCVIT_GEMM_P8_192 10
    float dropout_p;       /* > 0: after act, before residual: v = keep(m, n) ? v / (1 - p) : 0 (nn.Dropout, training) */
    uint32_t dropout_seed;
    float dact_scale;      /* multiplies v together with dact (0 = 1): 1/(1-p) of a dropout that followed the ReLU */
    int32_t row_offset;    /* dropout mask row of C row m is m + row_offset (a GEMM computed as row slices
                              keeps one mask) */
    void *colsum_out;      /* NULL, or [N]: column sums over m of the epilogue's result (the bias gradient of the Linear
                              that produced the A operand's gradient chain, e.g. db1 = colsum(dh)): fp32, or bf16 when
                              colsum_bf16 != 0.  Fused into the persistent kernel's epilogue when that kernel runs
                              (partials of the fp32 values in `workspace`, then a fixed-order reduce); otherwise a
                              separate pass over the stored bf16 C.  Needs workspace_bytes >=
                              sfcvit_gemm_colsum_workspace(M, N); not with split-K or fp32 C. */
    int32_t colsum_bf16;
    const uint32_t *seed_off; /* NULL, or a device word added to dropout_seed when the kernel RUNS (sfcvit_step_advance):
                                 lets a captured graph draw a new mask per replay */
    void *actmask;         /* NULL, or a bit matrix [M][ld_actmask bytes], bit (n & 7) of byte n >> 3 of row m <-> C[m, n] > 0:
                              with act = RELU it is WRITTEN (fused into the persistent kernel's epilogue, a separate pass
                              over C otherwise); with dact = RELU it MAY be read in place of aux_in (the persistent kernel
                              does: 2 bytes instead of 32 per lane and row; aux_in must be valid all the same).
                              linear2's dX through ReLU + dropout needs only the sign pattern of the stored activation
                              (torch:nn/modules/transformer.py:980-982): 19 MB instead of 308 MB per ViT-B layer.
                              N % 16 == 0, ld_actmask even and >= N / 8, 2-byte aligned. */
    int32_t ld_actmask;
} sfcvit_gemm_args;

int sfcvit_gemm(const sfcvit_gemm_args *a, void *stream);
/* HOST: workspace bytes for a call with colsum_out. */
int64_t sfcvit_gemm_colsum_workspace(int M, int N);
/* HOST: name of the kernel the calling thread's last sfcvit_gemm launched, as rocprofv3 prints it (without the
 * namespace), e.g. "gemm8p_kernel<7, 6, true>" -- lets a benchmark key its live timings by kernel symbol. */
int sfcvit_last_gemm_kernel(char *buf, int n);
/* HOST: bytes of workspace sfcvit_gemm needs for this split (0 when splitk <= 1). */
int64_t sfcvit_gemm_workspace(int M, int N, int splitk);

/* dst[c, r] = src[r, c] (bf16; R, C, lds, ldd multiples of 8).  One transposed copy of a weight per
 * step lets dX = dY W run with both operands k-contiguous (sfcvit_gemm's fastest layout). */
int sfcvit_transpose(const void *src, int R, int C, int lds, void *dst, int ldd, void *stream);

/* The same for many contiguous matrices in ONE launch (every weight of a model at the start of its backward pass: 51 launches
 * of 5 us become one).  `tiles` is a DEVICE array with one entry per 64 x 64 tile; matrix i occupies src_base + src_off
 * elements as [R, C] and its transpose dst_base + dst_off as [C, R]; R and C multiples of 8, offsets multiples of 8. */
typedef struct sfcvit_transpose_tile {
    int64_t src_off, dst_off;   /* in bf16 elements */
    int32_t R, C;               /* the matrix this tile belongs to */
    int32_t r0, c0;             /* first row / column of the tile */
} sfcvit_transpose_tile;
int sfcvit_transpose_batched(const void *src_base, void *dst_base, const sfcvit_transpose_tile *tiles, int n_tiles, void *stream);

/* Deferred partial-sum reductions.  Every column-sum-like result of this library (sfcvit_colsum, the bias sums of
 * sfcvit_gemm / sfcvit_attention_bwd, dgamma / dbeta / column sums of sfcvit_layernorm_bwd) is a main kernel that writes
 * fp32 partial rows into the caller's workspace and a small fixed-order reduction over them.  While deferral is on
 * (process-wide switch), calls queue that reduction instead of launching it; sfcvit_reduce_flush launches everything
 * queued as ONE kernel on `stream` (which must be the stream the calls used).  The caller keeps the workspaces and the
 * outputs alive and unread until the flush.  sfcvit_reduce_defer returns the previous setting; _pending the queue length;
 * _discard empties the queue without launching (after an aborted pass). */
int sfcvit_reduce_defer(int on);
int sfcvit_reduce_pending(void);
int sfcvit_reduce_flush(void *stream);
int sfcvit_reduce_discard(void);

/* Column sums: out[n] = sum_m x[m, n] (bias gradients). x bf16 [M, ld]; out fp32 [N] (overwritten).
 * Two passes through `workspace` (sfcvit_colsum_workspace bytes, HOST query) instead of float atomics, so the
 * result is bit-reproducible from run to run. */
int64_t sfcvit_colsum_workspace(int M, int N);
int sfcvit_colsum(const void *x, int M, int N, int ld, void *out, int out_bf16, void *workspace, int64_t workspace_bytes,
                  void *stream);   /* out: fp32 [N], or bf16 [N] when out_bf16 != 0 */

/* ------------------------------------------------------------------------
 * LayerNorm (biased variance, affine) -- nn.LayerNorm at norm1/norm2
 * (torch:nn/modules/transformer.py:951-958), channel_mix_ln (vit.py:254,272), mlp_head.0 (vit.py:303)
 * ---------------------------------------------------------------------- */
/* y = (x - mean) * rstd * gamma + beta ; mean, rstd fp32 [M] saved for backward. */
int sfcvit_layernorm_fwd(const void *x, const void *gamma, const void *beta, void *y,
                         float *mean, float *rstd, int M, int D, float eps, void *stream);
/* dx (bf16) ; dgamma, dbeta fp32 [D].  If dx_add != NULL, dx = dx_add + LN-backward
 * (gradient arriving over the residual branch).  ws: fp32 workspace of
 * sfcvit_layernorm_bwd_ws(M, D) bytes. */
int sfcvit_layernorm_bwd(const void *dy, const void *x, const float *mean, const float *rstd,
                         const void *gamma, const void *dx_add, void *dx, float *dgamma,
                         float *dbeta, int M, int D, void *ws, void *stream);
/* Same, plus (dx_drop != NULL) dx_drop[m, d] = keep(m, d) ? dx / (1 - p) : 0 (bf16): the gradient
 * entering a sub-layer whose output went through nn.Dropout(p) before the residual add (dropout1 /
 * dropout2, torch:nn/modules/transformer.py:953-957), mask regenerated from `seed`; and
 * (dcol != NULL) dcol[d] = sum_m of that outgoing gradient (dx_drop if given, else dx), fp32 [D]: the
 * bias gradient of the sub-layer's last Linear, for free in the same pass. */
int sfcvit_layernorm_bwd_drop(const void *dy, const void *x, const float *mean, const float *rstd,
                              const void *gamma, const void *dx_add, void *dx, void *dx_drop, float p,
                              uint32_t seed, const uint32_t *seed_off, void *dgamma, void *dbeta, void *dcol, int grads_bf16, int M, int D,
                              void *ws, void *stream);
/* grads_bf16 != 0: dgamma / dbeta / dcol are bf16 [D] instead of fp32 -- the caller passes views of its flat
 * gradient buffer and no cast / accumulate pass follows. */
int64_t sfcvit_layernorm_bwd_ws(int M, int D);
/* HOST: name of the main kernel the calling thread's last sfcvit_layernorm_bwd / _bwd_drop / _bwd_path or
 * sfcvit_add_layernorm_path_fwd launched, as rocprofv3 prints
 * it (e.g. "ln_bwd_cols_kernel<4, true>"): tests assert through it that a width ran on the column-sum kernel. */
int sfcvit_last_rowwise_kernel(char *buf, int n);

/* Stochastic depth (DropPath, timm's drop_path with scale_by_keep) on a residual site of the post-norm encoder layer:
 *   s = bf16(x + c[b] * branch),  y = LayerNorm(s),  c[b] = keep(b) / (1 - rate),  b = row / N, one flag per image.
 * keep(b) is element (b, 0) of the mask sfcvit_dropout_mask writes for `seed` at p = rate (seed_off: the device word the
 * dropout sites add, NULL = 0); nothing is stored, backward regenerates it.  branch, x, s, y: bf16 [B * N, D]; branch is the
 * sub-layer's output after its own dropout, WITHOUT the residual; a dropped image's rows of branch are not read and its rows
 * of s are the bits of x.  mean, rstd fp32 [B * N] are those of the rounded s.  D % 8 == 0, D <= 4096; s and y overlap
 * neither an input nor each other.  Notes its kernel ("add_ln_path_kernel<2>") for sfcvit_last_rowwise_kernel. */
int sfcvit_add_layernorm_path_fwd(const void *branch, const void *x, const void *gamma, const void *beta, void *s, void *y,
                                  float *mean, float *rstd, int B, int N, int D, float eps, float rate,
                                  uint32_t seed, const uint32_t *seed_off, void *stream);
/* sfcvit_layernorm_bwd_drop over M = B * rows_per_image rows with the branch scale of the site above in the outgoing gradient:
 *   dx_drop[m, d] = keep_path(m / rows_per_image) && keep(m, d) ? dx / ((1 - p) (1 - path_rate)) : 0
 * dx_drop is required and written at p = 0 too; dcol sums it as stored, i.e. rounded to bf16 (nothing from dropped images); dx, dgamma and dbeta are those of
 * sfcvit_layernorm_bwd_drop.  Same workspace (sfcvit_layernorm_bwd_ws(B * rows_per_image, D)), deferral and grads_bf16 forms. */
int sfcvit_layernorm_bwd_path(const void *dy, const void *x, const float *mean, const float *rstd, const void *gamma,
                              const void *dx_add, void *dx, void *dx_drop, float p, uint32_t seed,
                              const uint32_t *seed_off, void *dgamma, void *dbeta, void *dcol, int grads_bf16, int B,
                              int rows_per_image, int D, void *ws, float path_rate, uint32_t path_seed, void *stream);

/* LayerScale residual site (CaiT / DeiT-III) of the pre-norm encoder layer, with or without stochastic depth: the site above
 * with a per-channel scale lam (bf16 [D], like gamma) on the branch,
 *   s = bf16(x + (c[b] * lam[d]) * branch),  y = LayerNorm(s),  c[b] = keep(b) / (1 - rate).
 * rate = 0: no DropPath, c = 1, no flag is evaluated (seed is unused).  Everything else is sfcvit_add_layernorm_path_fwd's
 * contract: a dropped image's rows of branch are not read and its rows of s are the bits of x; mean / rstd are those of the
 * rounded s; D % 8 == 0, D <= 4096; no in-place form.  Notes its kernel as "add_ln_scale_kernel<2>". */
int sfcvit_add_layernorm_scale_fwd(const void *branch, const void *x, const void *lam, const void *gamma, const void *beta, void *s,
                                   void *y, float *mean, float *rstd, int B, int N, int D, float eps, float rate, uint32_t seed,
                                   const uint32_t *seed_off, void *stream);
/* sfcvit_layernorm_bwd_path plus the channel scale.  dx = dx_add + LayerNorm backward is the gradient of s (and of x);
 *   dx_drop[m, d] = keep_path(m / rows_per_image) && keep(m, d) ? dx * lam[d] / ((1 - p) (1 - path_rate)) : 0   (always written)
 *   dcol[d] = sum_m dx_drop as stored (rounded);   dlam[d] = sum_m dx[m, d] as stored (rounded) * c[b] * branch[m, d]
 * branch (bf16 [M, D]) is the forward's branch; rows of dropped images are not read and add nothing to dlam.  dlam is required
 * (fp32 or bf16 [D] like the others: it may be a row of a [2, D] parameter's gradient slot); dcol may be NULL.  dgamma, dbeta
 * and dx are those of sfcvit_layernorm_bwd_drop on the same grid.  path_rate = 0: no flag is evaluated.  Four reductions are
 * queued under sfcvit_reduce_defer.  Workspace: sfcvit_layernorm_bwd_scale_ws(M, D) bytes (four partial rows per workgroup,
 * 4/3 of sfcvit_layernorm_bwd_ws).  D % 8 == 0, D <= 2048.  The kernel form is sfcvit_layernorm_bwd_drop's for the width:
 * "ln_bwd_scale_kernel<2, true>" (vectors per lane, dx_add given), "ln_bwd_cols_scale_kernel<3, false>" at D = 768 / 1024. */
int sfcvit_layernorm_bwd_scale(const void *dy, const void *x, const float *mean, const float *rstd, const void *gamma,
                               const void *dx_add, const void *branch, const void *lam, void *dx, void *dx_drop, float p,
                               uint32_t seed, const uint32_t *seed_off, void *dgamma, void *dbeta, void *dcol, void *dlam,
                               int grads_bf16, int B, int rows_per_image, int D, void *ws, float path_rate, uint32_t path_seed,
                               void *stream);
int64_t sfcvit_layernorm_bwd_scale_ws(int M, int D);

/* QK-norm (ViT-22B; timm's qk_norm=True): a LayerNorm over the head dim on the queries and keys of every head of a packed
 * projection qkv [M, 3 * H * hp] bf16 (q | k | v thirds, head h at columns h * hp .. of each third), IN PLACE, before q k^T:
 *   q[m, h, :hd] <- LayerNorm_hd(q[m, h, :hd]; P[0], P[1], eps),  k likewise with P[2], P[3];  q, k[m, h, hd:hp] <- +0;  v untouched
 * hp: the kernel head dim (64 / 128 / 192 / 256); 1 <= hd <= hp: the model's head dim, columns hd .. hp - 1 being zero padding
 * that stays out of the statistics.  params P: bf16 [4, hd], rows q_weight, q_bias, k_weight, k_bias, shared by all heads.
 * Biased variance, centred, fp32 from the bf16 inputs; one rounding to bf16.  eps >= 0, finite.  raw [M, 2 * H * hp] bf16
 * receives the bits of q | k as they were: the backward recomputes mean and rstd from it with the forward's own device
 * function, nothing else is stored.  Notes its kernel ("qk_norm_fwd_kernel<64>") for sfcvit_last_rowwise_kernel. */
int sfcvit_qk_norm_fwd(void *qkv, void *raw, const void *params, int M, int H, int hd, int hp, float eps, void *stream);
/* Its backward, in place on the q and k thirds of dqkv [M, 3 * H * hp] as the attention backward left them (v untouched):
 *   dx = rstd * (g - mean(g) - xh * mean(g * xh)),  g = dy * gamma, over the hd real columns; padded columns are written +0
 * whatever they held.  dparams [4, hd] (fp32, or bf16 with dparams_is_bf16: a gradient slot): dgamma = sum dy * xh and dbeta =
 * sum dy over all M * H head rows, q and k apart.  colsum (optional; fp32 or bf16) [2 * H * hp]: the column sums of the stored
 * dq | dk over the M rows, the q and k part of the in_proj bias gradient.  vsum (optional, needs colsum): fp32 [H * hp], the v
 * third's column sums from the attention backward; colsum is then [3 * H * hp] and its last third receives them, so one slot
 * ends up holding the whole bias gradient.  Deterministic: per-workgroup partials in ws (sfcvit_qk_norm_bwd_ws(M, H, hp)
 * bytes), one fixed-order second-stage launch, no atomics, a grid that depends on the shape alone.  Never queued under
 * sfcvit_reduce_defer.  Notes "qk_norm_bwd_kernel<64>". */
int sfcvit_qk_norm_bwd(void *dqkv, const void *raw, const void *params, void *dparams, int dparams_is_bf16, void *colsum,
                       int colsum_is_bf16, const float *vsum, void *ws, int M, int H, int hd, int hp, float eps, void *stream);
int64_t sfcvit_qk_norm_bwd_ws(int M, int H, int hp);
/* HOST: the launch geometry of both directions: out[0] = token rows per workgroup, out[1] = slot groups (of 8 head slots) per
 * row, out[2] = workgroups = out[1] * ceil(M / out[0]), out[3] = 16-byte vectors per lane. */
int sfcvit_qk_norm_plan(int M, int H, int hp, int32_t *out);

/* RoPE (rotary position embedding; RoPE-ViT, EVA-02, timm's rope blocks) on the queries and keys of every head of a packed
 * projection qkv [M = B * N, 3 * H * hp] bf16 (q | k | v thirds, head h at columns h * hp .. of each third), IN PLACE, after
 * QK-norm and before q k^T.  Channel pairs are interleaved: pair p of a head row is its columns (2 p, 2 p + 1).
 *   table [N, hd / 2, 2] fp32: row n, pair p holds (c, s); shared by the heads, the batch, q and k; row m uses n = m mod N
 *   y0 = x0 * c - x1 * s,  y1 = x0 * s + x1 * c          (fp32 from the bf16 inputs, one rounding to bf16)
 * The map [c -s; s c] is applied as given: c * c + s * s = 1 is not assumed.  hp: the kernel head dim (64 / 128 / 192 / 256);
 * hd: the model's head dim, EVEN, 2 <= hd <= hp; columns hd .. hp - 1 are padding and are written +0 whatever they held.  v is
 * neither read nor written and nothing is saved for the backward.  Notes its kernel ("rope_fwd_kernel<64>") for
 * sfcvit_last_rowwise_kernel. */
int sfcvit_rope_fwd(void *qkv, const float *table, int B, int N, int H, int hd, int hp, void *stream);
/* Its backward, in place on the q and k thirds of dqkv [B * N, 3 * H * hp] as the attention backward left them (v untouched):
 * the transposed map, dx0 = g0 * c + g1 * s, dx1 = -g0 * s + g1 * c; padded columns are written +0 even when they held NaN.
 * colsum (optional; fp32, or bf16 with colsum_is_bf16) [2 * H * hp]: the column sums of the stored dq | dk over the M rows, the q
 * and k part of the in_proj bias gradient; needs ws (sfcvit_rope_bwd_ws(B, N, H, hp) bytes).  vsum (optional, needs colsum):
 * fp32 [H * hp], the v third's column sums from the attention backward; colsum is then [3 * H * hp] and its last third
 * receives them.  Deterministic: per-workgroup fp32 partials, one fixed-order second-stage launch, no atomics, a grid that
 * depends on the shape alone.  Without colsum: one launch, no workspace, the same dq | dk bits.  Never queued under
 * sfcvit_reduce_defer.  Notes "rope_bwd_kernel<64>". */
int sfcvit_rope_bwd(void *dqkv, const float *table, void *colsum, int colsum_is_bf16, const float *vsum, void *ws, int B, int N,
                    int H, int hd, int hp, void *stream);
int64_t sfcvit_rope_bwd_ws(int B, int N, int H, int hp);
/* HOST: the launch geometry of both directions: out[0] = tokens per workgroup (one per wave), out[1] = images per workgroup (a
 * wave walks them), out[2] = slot groups (of 8 head slots) per row, out[3] = workgroups = out[2] * ceil(N / out[0]) *
 * ceil(B / out[1]), out[4] = 16-byte vectors per lane. */
int sfcvit_rope_plan(int B, int N, int H, int hp, int32_t *out);

/* ------------------------------------------------------------------------
 * Multi-head self-attention core (no mask; the masked form is the next section) on the packed projection
 *   replaces F.scaled_dot_product_attention as reached from nn.MultiheadAttention
 *   (torch:nn/functional.py:6623-6631); qkv is the in_proj output [B, N, 3*H*hd]
 *   with q | k | v in thirds, head h at columns h*hd .. h*hd+hd-1 of each third.
 * ---------------------------------------------------------------------- */
typedef struct sfcvit_attn_args {
    const void *qkv; /* [B, N, 3*H*hd] bf16 */
    void *out;       /* fwd: out [B, N, H*hd] bf16 ; bwd: in */
    float *lse;      /* [B, H, N] fp32 log-sum-exp of the scaled scores: fwd out, bwd in */
    const void *dout; /* bwd: [B, N, H*hd] bf16 */
    void *dqkv;       /* bwd: out [B, N, 3*H*hd] bf16 */
    float *delta;     /* bwd: workspace [B, H, N] fp32 */
    int32_t B, N, H, hd;
    float scale;      /* 1/sqrt(hd) */
    float dropout_p;  /* > 0: dropout on the attention probabilities (SDPA dropout_p, training mode);
                         row = (b*H + h)*N + q, col = key of the mask function */
    uint32_t dropout_seed;
    const uint32_t *seed_off; /* as in sfcvit_gemm_args */
    /* backward only, optional: column sums of dqkv over all B * N rows (= the in_proj bias gradient,
     * torch:nn/functional.py:5822-5833) written to colsum_out ([3 D], fp32 or bf16).  colsum_part = workspace of
     * sfcvit_attention_colsum_workspace(B, N, H, hd) bytes.  The one-pass kernel (hd = 64, N <= 224) emits the sums
     * itself; the other paths run sfcvit_colsum over the dqkv they wrote. */
    float *colsum_part;
    int64_t colsum_part_bytes;
    void *colsum_out;
    int32_t colsum_bf16;
} sfcvit_attn_args;
int64_t sfcvit_attention_colsum_workspace(int B, int N, int H, int hd);

int sfcvit_attention_fwd(const sfcvit_attn_args *a, void *stream);
int sfcvit_attention_bwd(const sfcvit_attn_args *a, void *stream);
/* The same for any sequence length: head dims 128 / 192 / 256 whose whole sequence does not fit one CU's LDS (N > 256,
 * or 192 / 160 for hd 192 / 256), where sfcvit_attention_fwd / _bwd refuse, run on streaming kernels that loop over
 * 64-row blocks (attn_wide_stream_*); every other shape runs exactly what sfcvit_attention_fwd / _bwd run.  Column sums
 * (colsum_out) work as there. */
int sfcvit_attention_fwd_any(const sfcvit_attn_args *a, void *stream);
int sfcvit_attention_bwd_any(const sfcvit_attn_args *a, void *stream);
/* HOST: the plan of sfcvit_attention_fwd (bwd = 0) / _bwd (bwd != 0), or of their _any forms (any_length != 0), for
 * these arguments and the current environment switches, without touching a device: writes the name of the main kernel
 * (as sfcvit_last_attn_kernel would report it) into buf and returns SFCVIT_OK, or returns the refusal's code with the
 * message in sfcvit_last_error().  Tensors are checked for null / alignment only, never read. */
int sfcvit_attention_plan(const sfcvit_attn_args *a, int bwd, int any_length, char *buf, int n);
/* HOST: name of the main kernel the calling thread's last sfcvit_attention_fwd / _bwd launched, as rocprofv3 prints it
 * (e.g. "attn_seq_bwd_fused_kernel<13, true>"): tests assert through it that a shape ran on the production kernel. */
int sfcvit_last_attn_kernel(char *buf, int n);

/* ------------------------------------------------------------------------
 * Masked / windowed self-attention core (head dim 64)
 *   replaces F.scaled_dot_product_attention(attn_mask=...) as reached from nn.TransformerEncoder.forward(src, mask)
 *   and the reference's CustomTransformerEncoder (src/models/vit.py:152-174), which passes src_mask to every layer.
 *
 *   A mask is an additive fp32 matrix M [N, N] shared by all batches and heads; entries are finite or -inf:
 *       s_ij = scale * q_i . k_j + M_ij,   P = softmax_j(s),   lse_i = log sum_j exp(s_ij)   (lse includes the mask)
 *   Dropout acts on P with the mask function of sfcvit_attn_args: with an all-zero M the same elements are dropped as
 *   in sfcvit_attention_fwd.  Preconditions (enforced by sfcvit_attention_mask_blocks, assumed by the kernels): no NaN,
 *   no +inf, and every row has at least one finite entry.
 *
 *   The block map says, per (64-query block, 64-key block), whether the kernels visit it: a workgroup owns 64 queries
 *   (forward, dQ) or 64 keys (dK / dV) and walks its row / column of the map, so a banded mask costs its band.  No
 *   atomics: every output element is written once after sums in a fixed order (two runs, same bits); key blocks no
 *   query sees get dK = dV = 0 written.
 * ---------------------------------------------------------------------- */
#define SFCVIT_MASK_BLOCK 64
#define SFCVIT_MASK_MAX_N 4096
/* HOST, no HIP call: validates mask_host [N, N] and writes map_host [nb][nb], nb = ceil(N / 64):
 *   0 = no finite entry (skipped), 1 = mixed (the kernels read the mask), 2 = every entry 0.0f (no mask read).
 * SFCVIT_EINVAL (reason in sfcvit_last_error()): null pointer, N < 1 or N > 4096, a NaN or +inf entry, a row without a
 * finite entry (the message names the row). */
int sfcvit_attention_mask_blocks(const float *mask_host, int N, uint8_t *map_host);
typedef struct sfcvit_attn_mask_args {
    /* the fields of sfcvit_attn_args, same meaning */
    const void *qkv;
    void *out;
    float *lse;
    const void *dout;
    void *dqkv;
    float *delta;
    int32_t B, N, H, hd; /* hd = 64 only, 1 <= N <= 4096 */
    float scale;
    float dropout_p;
    uint32_t dropout_seed;
    const uint32_t *seed_off;
    float *colsum_part;  /* workspace of sfcvit_attention_colsum_workspace(B, N, H, hd) bytes, with colsum_out */
    int64_t colsum_part_bytes;
    void *colsum_out;    /* bwd, optional: sfcvit_colsum over the dqkv written */
    int32_t colsum_bf16;
    /* the mask */
    const float *mask;        /* device, [N, N] fp32 */
    const uint8_t *block_map; /* device, [nb][nb] as written by sfcvit_attention_mask_blocks for this mask */
} sfcvit_attn_mask_args;
/* Argument checks (null, 16-byte alignment of the bf16 tensors, N, hd, dropout_p in [0, 1)) run before any HIP call.
 * sfcvit_last_attn_kernel reports "attn_masked_fwd_kernel" / "attn_masked_bwd_kv_kernel". */
int sfcvit_attention_masked_fwd(const sfcvit_attn_mask_args *a, void *stream);
int sfcvit_attention_masked_bwd(const sfcvit_attn_mask_args *a, void *stream);

/* ------------------------------------------------------------------------
 * Self-attention core with a learned relative position bias per head (head dim 64)
 *   the bias of Swin / BEiT windows: softmax(q k^T / sqrt(hd) + b_h[offset(i, j)]) v
 *
 *       s[b,h,i,j]  = scale * q_i . k_j + bias(h,i,j)
 *       bias(h,i,j) = table[h, index[i,j]]   if index[i,j] >= 0
 *                   = -inf                   if index[i,j] == -1   (pair hidden: a window lives in the index itself)
 *       P = softmax_j(s),   lse_i = log sum_j exp(s_ij)   (lse includes the bias)
 *       dTable[h,t] = sum over b and over (i,j) with index[i,j] == t of  P_ij * (keep_ij * dP_ij - delta_i)
 *   index: int32 [N, N], values in [-1, T), shared by all batches and heads, static.  table: fp32 [H, T].  Dropout acts on
 *   P with the mask function of sfcvit_attn_args, keep_ij = 1 / (1 - p) or 0: an all-zero table over an all-visible index
 *   drops what sfcvit_attention_fwd drops.  The bias sits after the scale: dTable carries no scale factor.  Preconditions
 *   (enforced by sfcvit_attention_bias_blocks, assumed by the kernels): every entry in [-1, T), every row has an entry >= 0.
 *
 *   The kernels are the masked ones with head h's table row staged in LDS once per workgroup and looked up per score;
 *   the block map says which 64 x 64 blocks hold a visible pair.  The table gradient takes no atomics: a workgroup owns
 *   one visited block of one head and a chunk of the batch, recomputes S and dP per image, sums P (keep dP - delta) in
 *   fp32 registers over its chunk and stores the block into the workspace [chunks][H][visited blocks][64][64]; the
 *   chunks are summed in ascending order, and one wave per dTable element then sums its bucket's positions in the fixed
 *   order of the inverted index.  Two runs give the same bits.
 * ---------------------------------------------------------------------- */
#define SFCVIT_BIAS_MAX_N 1024
#define SFCVIT_BIAS_MAX_BUCKETS 4096 /* one head's table row in LDS: 16 KiB */
/* HOST, no HIP call: validates index_host [N, N] and writes
 *   map_host [nb][nb], nb = ceil(N / 64): 0 = every entry -1 (skipped), 1 = visited;
 *   the inverted index as CSR: offsets_host [T + 1], positions_host [number of entries >= 0, at most N * N]:
 *   positions_host[offsets_host[t] .. offsets_host[t + 1]) are the i * N + j with index[i,j] == t, ascending.
 * SFCVIT_EINVAL (reason in sfcvit_last_error()): null pointer, N outside 1 .. 1024, T outside 1 .. 4096, an entry < -1 or
 * >= T (the message names row and column), a row without an entry >= 0 (the message names the row). */
int sfcvit_attention_bias_blocks(const int32_t *index_host, int N, int T, uint8_t *map_host, int32_t *offsets_host,
                                 int32_t *positions_host);
/* Bytes of the table gradient's workspace for a map with `visited_blocks` non-zero entries. */
int64_t sfcvit_attention_bias_workspace(int B, int N, int H, int visited_blocks);
typedef struct sfcvit_attn_bias_args {
    /* the fields of sfcvit_attn_mask_args without the mask, same meaning */
    const void *qkv;
    void *out;
    float *lse;
    const void *dout;
    void *dqkv;
    float *delta;
    int32_t B, N, H, hd; /* hd = 64 only, 1 <= N <= 1024 */
    float scale;
    float dropout_p;
    uint32_t dropout_seed;
    const uint32_t *seed_off;
    float *colsum_part;
    int64_t colsum_part_bytes;
    void *colsum_out;
    int32_t colsum_bf16;
    const uint8_t *block_map; /* device, [nb][nb] as written by sfcvit_attention_bias_blocks for this index */
    /* the bias */
    const int32_t *index;     /* device, [N, N] */
    const float *table;       /* device, [H, T] fp32 */
    int32_t T;
    int32_t visited_blocks;   /* bwd: number of non-zero entries of block_map */
    const int32_t *offsets;   /* bwd: device, [T + 1] */
    const int32_t *positions; /* bwd: device, [offsets[T]] */
    float *dtable;            /* bwd: out, device, [H, T] fp32; every element is written.  NULL: a frozen table -- its gradient
                                 is not computed, and visited_blocks, offsets, positions and the workspace are not looked at */
    void *workspace;          /* bwd: sfcvit_attention_bias_workspace(B, N, H, visited_blocks) bytes, 16-byte aligned */
    int64_t workspace_bytes;
} sfcvit_attn_bias_args;
/* Argument checks (null, alignment, N, T, hd, dropout_p, workspace size) run before any HIP call.
 * sfcvit_last_attn_kernel reports "attn_bias_fwd_kernel" / "attn_bias_bwd_kv_kernel".  colsum_out as in the masked backward. */
int sfcvit_attention_bias_fwd(const sfcvit_attn_bias_args *a, void *stream);
int sfcvit_attention_bias_bwd(const sfcvit_attn_bias_args *a, void *stream);

/* ------------------------------------------------------------------------
 * Attention maps and attention-distance statistics
 *   replaces the `(output, [attn_weights per layer])` path of CustomTransformerEncoderLayer / CustomTransformerEncoder
 *   (src/models/vit.py:48-174, commented out there; average_attn_weights=False) and the need_weights=True branch of
 *   multi_head_attention_forward (torch:nn/functional.py), which leaves the fused SDPA path and materialises
 *   [B, H, N, N] per layer.
 *
 * Both entry points take the packed projection and the lse that sfcvit_attention_fwd / _fwd_any wrote for it (the
 * log-sum-exp of the scaled scores; it does not depend on dropout) and rebuild
 *     P[i, j] = exp(scale * q_i . k_j - lse[i])
 * in one pass over 64-key blocks: no row maximum, no online softmax, LDS use independent of N.  Any N >= 1, head dims
 * 64 / 128 / 192 / 256.  No atomics: every output element is written once by one lane after sums in a fixed order, so
 * two runs give the same bits.
 * ---------------------------------------------------------------------- */
typedef struct sfcvit_attn_probe_args {
    const void *qkv;       /* [B, N, 3*H*hd] bf16 (sfcvit_attn_args.qkv) */
    const float *lse;      /* [B, H, N] fp32, as written by the attention forward */
    int32_t B, N, H, hd;
    float scale;           /* the forward's softmax scale; finite, nonzero */
    /* sfcvit_attention_probs */
    void *probs;           /* head_mean = 0: [B, H, N, N]; head_mean = 1: [B, N, N] = the mean over heads, summed in head
                              order in fp32 and multiplied by 1/H once (average_attn_weights=True) */
    int32_t probs_is_bf16; /* 0: fp32, 1: bf16 (round to nearest even) */
    int32_t head_mean;
    /* sfcvit_attention_stats: per query row, each [B, H, N] fp32 or NULL = skip (at least one must be given) */
    const float *pos;      /* [N, 2] fp32 (row, col) of each token's centre in the image; needed by dist_rows only */
    float *dist_rows;      /* sum_j P[i, j] * ||pos_i - pos_j||_2 : attention distance in image space */
    float *seq_rows;       /* sum_j P[i, j] * |i - j|             : attention distance along the token sequence (the curve) */
    float *ent_rows;       /* sum_j P[i, j] * (lse_i - s_ij)      : entropy in nats (a term with P = 0 adds 0) */
    float *mass_rows;      /* sum_j P[i, j]                       : ~1; how well these scores agree with the forward's lse */
} sfcvit_attn_probe_args;
/* Rows are written with 16-byte stores when N % 4 == 0 (fp32) / N % 8 == 0 (bf16), element by element otherwise. */
int sfcvit_attention_probs(const sfcvit_attn_probe_args *a, void *stream);
int sfcvit_attention_stats(const sfcvit_attn_probe_args *a, void *stream);

/* ------------------------------------------------------------------------
 * Depth-wise convolution along the token sequence
 *   replaces the first stage of TokenAggregator.forward (src/models/vit.py:37-42):
 *   nn.Conv1d(dim, dim, k, s, padding=k//2, groups=dim) between two transposes.  Here the activation stays
 *   [B, N, D] bf16 with D contiguous; the point-wise Conv1d, GELU and LayerNorm that follow are a GEMM,
 *   the GELU pass and the LayerNorm of this library.
 *
 *   x [B, N, D] bf16;  w [D, k] bf16 (dw.weight [D, 1, k] viewed 2-D);  bias [D] bf16 or NULL;  u [B, Nout, D] bf16,
 *   pad = k / 2, Nout = (N + 2 pad - k) / s + 1 (nn.Conv1d's rule: odd k with s = 1 keeps N, even k gives N + 1).
 *   Supported: k in 1..9, s in 1..4, D % 8 == 0, B, N >= 1 (N < k included); everything else is SFCVIT_EINVAL, decided
 *   before any HIP call.  x, u, du, dx and the workspace must be 16-byte aligned; w, bias, dw, db need no alignment.
 *   No atomics: dw / db partial sums go through the workspace and are added in a fixed order (two runs, same bits);
 *   their final reduction joins the deferred reductions above when deferral is on.
 * ---------------------------------------------------------------------- */
/* HOST: Nout, or a negative value for arguments the kernels refuse. */
int sfcvit_dwconv1d_out_len(int N, int k, int s);
/* u[b, n, d] = bf16( bias[d] + sum_t w[d, t] * x[b, n s + t - pad, d] ), rows outside 0 .. N - 1 counted as zero; the
 * sum runs in fp32 in tap order t = 0 .. k - 1 starting from the bias, and is rounded once.  A tap never reaches into
 * image b - 1 or b + 1. */
int sfcvit_dwconv1d_fwd(const void *x, const void *w, const void *bias, void *u, int B, int N, int D, int k, int s, void *stream);
/* HOST: workspace bytes of the backward call (0 for refused arguments). */
int64_t sfcvit_dwconv1d_bwd_workspace(int B, int N, int D, int k, int s);
/* du [B, Nout, D] bf16 in.  Each output may be NULL = skipped (not all three):
 *   dx [B, N, D] bf16: dx[b, m, d] = sum_t w[d, t] * du[b, (m + pad - t) / s, d] over the taps where the division is
 *      exact and in range (fp32 sum in tap order, one rounding); needs w
 *   dw [D, k]:         dw[d, t] = sum_{b, n} du[b, n, d] * x[b, n s + t - pad, d]; needs x
 *   db [D]:            db[d] = sum_{b, n} du[b, n, d]
 * dw and db are summed in fp32 and written as fp32, or as bf16 when grads_bf16 != 0 (views of a flat gradient buffer).
 * The workspace is needed for dw / db only. */
int sfcvit_dwconv1d_bwd(const void *du, const void *x, const void *w, void *dx, void *dw, void *db, int grads_bf16, int B, int N,
                        int D, int k, int s, void *workspace, int64_t workspace_bytes, void *stream);
/* HOST: name of the main kernel the calling thread's last sfcvit_dwconv1d_fwd / _bwd launched, as rocprofv3 prints it
 * (e.g. "dwconv3_bwd_kernel<true, true>"). */
int sfcvit_last_dwconv_kernel(char *buf, int n);

/* ------------------------------------------------------------------------
 * Positional embedding
 *   the reference's commented-out `x = x + self.pos_embed` (src/models/vit.py:360-361, :382; :207-219, :240): one table
 *   row per token index, added to every image directly after the tokenizer.
 *
 *   x, y, dy [B, N, D] bf16, D contiguous;  pos [N, D] bf16 (a [1, N, D] parameter viewed 2-D).
 *   Supported: B, N >= 1, D >= 8 and D % 8 == 0 (16-byte vectors), byte counts within int64; everything else is
 *   SFCVIT_EINVAL, decided before any HIP call.  x, pos, y, dy and the workspace must be 16-byte aligned; dpos needs the
 *   alignment of its element only (a slot of a flat gradient buffer).  Nothing allocates, synchronises or copies to the
 *   host: graph-capturable.  dx of the add is dy itself: there is no kernel for it.
 * ---------------------------------------------------------------------- */
/* y[b, n, :] = bf16( float(x[b, n, :]) + float(pos[n, :]) ): one rounding per element (the bits of torch's bf16 add).
 * y may be x itself (in place). */
int sfcvit_pos_embed_fwd(const void *x, const void *pos, void *y, int B, int N, int D, void *stream);
/* HOST: workspace bytes of the backward call (0 for refused arguments, and 0 wherever the table alone fills the GPU). */
int64_t sfcvit_pos_embed_bwd_workspace(int B, int N, int D);
/* dpos[n, :] = sum_b dy[b, n, :], summed in fp32 in a fixed order (no atomics, one writer per element: two runs, same
 * bits) and written as fp32, or as bf16 when grad_bf16 != 0 (a view of a flat gradient buffer).  Where the plan splits
 * the batch (workspace > 0) the final reduction joins the deferred reductions above when deferral is on. */
int sfcvit_pos_embed_bwd(const void *dy, void *dpos, int grad_bf16, int B, int N, int D, void *workspace, int64_t workspace_bytes,
                         void *stream);
/* HOST: name of the kernel the calling thread's last sfcvit_pos_embed_fwd / _bwd launched, as rocprofv3 prints it
 * (e.g. "pos_embed_bwd_kernel<2>"). */
int sfcvit_last_pos_embed_kernel(char *buf, int n);

/* ------------------------------------------------------------------------
 * CLS token and token pooling
 *   the reference's commented-out learnable [CLS] token (src/models/vit.py:209-210, :237-238: `torch.cat([cls, x], dim=1)`
 *   in front of the encoder), the read-out of token 0 its docstring promises, and the token mean of altvit.py.
 *
 *   Every tensor is bf16 with D contiguous.  Supported: B, N (T) >= 1, D >= 8 and D % 8 == 0 (16-byte vectors), byte counts
 *   within int64; everything else is SFCVIT_EINVAL, decided before any HIP call.  Every tensor and the workspace must be
 *   16-byte aligned, except dcls, which needs the alignment of its element only (a slot of a flat gradient buffer).
 *   Nothing allocates, synchronises or copies to the host: graph-capturable.  No atomics, one writer per output element:
 *   two runs give the same bits.
 * ---------------------------------------------------------------------- */
/* x [B, N, D], cls [D] -> y [B, N + 1, D]:  y[b, 0, :] = cls, y[b, 1 + n, :] = x[b, n, :].  A copy of bits.  y must not
 * overlap x. */
int sfcvit_cls_prepend_fwd(const void *x, const void *cls, void *y, int B, int N, int D, void *stream);
/* HOST: workspace bytes of the backward call (0 for refused arguments, and 0 up to 2048 images). */
int64_t sfcvit_cls_prepend_bwd_workspace(int B, int N, int D);
/* dy [B, N + 1, D] -> dx [B, N, D] = dy[:, 1:, :] (a copy; dx may be NULL: dcls alone) and dcls[d] = sum_b dy[b, 0, d],
 * summed in fp32 in a fixed order and written as fp32, or as bf16 when grad_bf16 != 0 (a view of a flat gradient buffer).
 * Where the plan splits the batch (workspace > 0) the final reduction joins the deferred reductions above when deferral is
 * on. */
int sfcvit_cls_prepend_bwd(const void *dy, void *dx, void *dcls, int grad_bf16, int B, int N, int D, void *workspace,
                           int64_t workspace_bytes, void *stream);
/* x [B, T, D] -> y [B, D]:  y[b, :] = bf16( (sum over t in [first, first + count) of float(x[b, t, :])) / count ): an fp32 sum
 * in a fixed order, one fp32 division, one rounding.  Needs 0 <= first, count >= 1, first + count <= T.  count == 1 copies
 * the row's bits (the CLS read-out: first = 0). */
int sfcvit_token_pool_fwd(const void *x, void *y, int B, int T, int D, int first, int count, void *stream);
/* dy [B, D] -> dx [B, T, D]:  dx[b, t, :] = bf16(float(dy[b, :]) / count) for t in [first, first + count) (the bits of dy
 * when count == 1) and +0 elsewhere: every element of dx is written. */
int sfcvit_token_pool_bwd(const void *dy, void *dx, int B, int T, int D, int first, int count, void *stream);
/* HOST: name of the kernel the calling thread's last sfcvit_cls_prepend_* / sfcvit_token_pool_* launched, as rocprofv3
 * prints it (e.g. "token_pool_fwd_kernel<16>": 16 lanes across columns, 256 / 16 = 16 lanes across the token range). */
int sfcvit_last_token_pool_kernel(char *buf, int n);

/* ------------------------------------------------------------------------
 * Token mixing: GEMMs along the token axis of [B, N, D]
 *   replaces the token-mix branch of MixerBlock.forward (src/models/vit.py:269-271, commented out there):
 *       x = x + token_mix(token_mix_ln(x).transpose(1, 2)).transpose(1, 2)
 *   with token_mix = Linear(N, hid) -> GELU -> Linear(hid, N) (src/models/vit.py:259-263).  The activation stays
 *   [B, N, D] bf16 with D contiguous and the hidden tensor is [B, hid, D]: neither transposed copy exists.  Every
 *   image's matrix is multiplied from the LEFT by a weight shared across the batch; a tile never crosses an image.
 *
 *   Supported: B >= 1, M >= 1, K >= 1, D % 8 == 0, and M % 8 == 0 or K % 8 == 0 (one of the two is the hidden width,
 *   the other the token count, which may be anything: 196, 27, 1); everything else is SFCVIT_EINVAL, decided before
 *   any HIP call.  x, c, bias-free activations (residual, aux_in, aux_out, g) and the workspace must be 16-byte
 *   aligned; w, bias, dw, db need 2-byte alignment only (rows of a [hid, N] weight are 2 N bytes: the weight loader
 *   uses the widest load the row pitch and the pointer allow).  Ragged M, K and D tails are zero-filled on load and
 *   masked on store.  Nothing allocates, synchronises or copies to the host: graph-capturable.
 * ---------------------------------------------------------------------- */
typedef struct sfcvit_tokmix_args {
    const void *w;        /* bf16, dense: [M, K] (k contiguous), or [K, M] when w_transposed != 0 */
    const void *x;        /* bf16 [B, K, D] */
    void *c;              /* bf16 [B, M, D] */
    const void *bias;     /* bf16 [M] or NULL: a ROW bias */
    const void *residual; /* bf16 [B, M, D] or NULL */
    const void *aux_in;   /* bf16 [B, M, D] or NULL: the result is multiplied by gelu'(aux_in) */
    void *aux_out;        /* bf16 [B, M, D] or NULL: the value before the activation */
    int32_t B, M, K, D;
    int32_t w_transposed;
    int32_t act;          /* SFCVIT_ACT_NONE or SFCVIT_ACT_GELU (erf form) */
} sfcvit_tokmix_args;
/* C_b[M, D] = epi( op(W) X_b[K, D] ) for b = 0 .. B-1, fp32 accumulation, epilogue in fp32 in this order:
 *   v += bias[m];  aux_out = bf16(v);  v = gelu(v);  v += residual[b, m, d];  v *= gelu'(aux_in[b, m, d]);  store bf16.
 * The four jobs of the block: fc1 (W1, z -> U, H), fc2 (W2, H, residual x), dH = W2^T dy with the gelu'(U) factor
 * (-> dU), dz = W1^T dU. */
int sfcvit_tokmix_left(const sfcvit_tokmix_args *a, void *stream);
/* HOST: workspace bytes of sfcvit_tokmix_wgrad (0 for refused arguments). */
int64_t sfcvit_tokmix_wgrad_workspace(int B, int M, int K, int D);
/* dW[M, K] = sum_b G_b[M, D] X_b[K, D]^T and db[m] = sum_{b, d} G_b[m, d]; g [B, M, D], x [B, K, D] bf16.  The
 * contraction runs over (b, d): ranges of whole images write fp32 partials into the workspace, the library's ordered
 * column reduction adds them (no atomics: two runs, same bits) and joins the deferred reductions when deferral is on.
 * dw / db are fp32, or bf16 when grads_bf16 != 0 (views of a flat gradient buffer); either may be NULL = skipped
 * (not both). */
int sfcvit_tokmix_wgrad(const void *g, const void *x, void *dw, void *db, int grads_bf16, int B, int M, int K, int D,
                        void *workspace, int64_t workspace_bytes, void *stream);
/* HOST: name of the main kernel the calling thread's last sfcvit_tokmix_left / _wgrad launched, as rocprofv3 prints it
 * (e.g. "tokmix_left_kernel<false, true>"). */
int sfcvit_last_tokmix_kernel(char *buf, int n);

/* ------------------------------------------------------------------------
 * Elementwise / loss / optimizer
 * ---------------------------------------------------------------------- */
/* y = gelu_erf(x) (nn.GELU in MultiLayerPredictor, vit.py:308); bf16, n elements. */
int sfcvit_gelu_fwd(const void *x, void *y, int64_t n, void *stream);
/* dx = dy * gelu'(x) */
int sfcvit_gelu_bwd(const void *dy, const void *x, void *dx, int64_t n, void *stream);
/* GELU followed by nn.Dropout(p) (MultiLayerPredictor, vit.py:308-309) on a [rows, cols] tensor, cols % 8 == 0. */
int sfcvit_gelu_drop_fwd(const void *x, void *y, int rows, int cols, float p, uint32_t seed, const uint32_t *seed_off, void *stream);
int sfcvit_gelu_drop_bwd(const void *dy, const void *x, void *dx, int rows, int cols, float p, uint32_t seed, const uint32_t *seed_off,
                         void *stream);
/* The keep mask itself, as bf16 {0, 1/(1-p)} (tests and debugging): out [rows, cols]. */
int sfcvit_dropout_mask(void *out, int64_t rows, int cols, float p, uint32_t seed, void *stream);

/* SoftTargetCrossEntropy (main.py:45-51), forward and gradient in one pass.
 * logits bf16 [B, ld] (first C columns used), targets fp32 [B, C];
 * loss_rows fp32 [B] = -sum_c t*log_softmax ; dlogits bf16 [B, ld] = (softmax*sum_c t - t) * gscale
 * (columns C..ld-1 are written 0).  The mean over B is gscale = 1/B by the caller. */
int sfcvit_soft_ce(const void *logits, const float *targets, float *loss_rows, void *dlogits,
                   int B, int C, int ld, float gscale, void *stream);

/* Sum of squares of a bf16 (is_f32 = 0) or fp32 buffer, accumulated into *out (fp32, device).  Block partials
 * go through `workspace` (SFCVIT_SUMSQ_WORKSPACE_BYTES, device) and are added in a fixed order: reproducible. */
#define SFCVIT_SUMSQ_WORKSPACE_BYTES 4096
int sfcvit_sumsq_accum(const void *g, int64_t n, int is_f32, float *out, void *workspace, void *stream);

/* Fused clip_grad_norm_ + AdamW step (src/training/train.py:165-166, main.py:288-289) on a
 * flat buffer.  clip coefficient = min(1, max_norm / (sqrt(*sumsq) + 1e-6)) is computed on the
 * device from *sumsq (torch.nn.utils.clip_grad_norm_ semantics).  master: fp32 copy of the
 * parameters (updated), param: bf16 parameters (rewritten from master), grad bf16,
 * m, v fp32.  Decoupled weight decay as torch.optim.AdamW. */
typedef struct sfcvit_adamw_args {
    void *param;       /* bf16 [n] */
    float *master;     /* fp32 [n] */
    const void *grad;  /* bf16 [n] */
    float *m, *v;      /* fp32 [n] */
    const float *sumsq; /* device scalar: sum of squares of ALL grads (NULL = no clipping) */
    int64_t n;
    float lr, beta1, beta2, eps, weight_decay, max_norm;
    float grad_scale;  /* every gradient (and the norm) is multiplied by this first:
                          1/world_size after a SUM all-reduce, else 1 */
    int32_t step;      /* 1-based */
    const float *dev_state; /* NULL, or the device step state of sfcvit_step_advance: lr and the bias corrections are then
                               read from it when the kernel RUNS (lr / step above are ignored) */
} sfcvit_adamw_args;
int sfcvit_adamw_step(const sfcvit_adamw_args *a, void *stream);

/* Model EMA: sfcvit_adamw_step with an exponential moving average of the fp32 master weights updated in the same kernel
 * (timm's --model-ema): per parameter, once the step has produced the new master value w,
 *     e <- e + (1 - d_t) * (w - e)                                   e fp32 [n], every operation in fp32
 * d_t = decay, or with warmup != 0  d_t = min(decay, float(1 + t) / float(10 + t))  (a correctly rounded fp32 division),
 * t = the 1-based step of this update: a->step, or word [1] of a->dev_state when that is set, read when the kernel RUNS --
 * a captured step replays with the right decay.  param, master, m and v get the bits sfcvit_adamw_step gives them; the
 * average costs one more fp32 stream in and out (36 bytes per parameter instead of 28) and no launch.
 * Refused (SFCVIT_EINVAL, before any HIP call): what sfcvit_adamw_step refuses, a null e or ema, an ema that is not 16-byte
 * aligned, a decay outside [0, 1) or NaN, an ema that shares a byte with param, master, grad, m or v. */
typedef struct sfcvit_ema_args {
    float *ema;        /* fp32 [n]: the average (updated) */
    float decay;       /* 0 <= decay < 1 */
    int32_t warmup;    /* != 0: d_t = min(decay, (1 + t) / (10 + t)) */
} sfcvit_ema_args;
int sfcvit_adamw_ema_step(const sfcvit_adamw_args *a, const sfcvit_ema_args *e, void *stream);

/* Gradient accumulation: K micro-batches per optimizer step.  The kernels of a backward pass overwrite the bf16 flat
 * gradient, so the running sum lives next to the optimizer in one fp32 buffer `acc` [n]: after each of the first K - 1
 * backward passes sfcvit_grad_accum folds the flat gradient into it (one elementwise pass, 6 bytes per parameter the first
 * time, 10 after), and after the last one sfcvit_grad_accum_finish forms the averaged gradient in place, with the clip's sum
 * of squares taken in the same pass (8 bytes per parameter; it replaces sfcvit_sumsq_accum's read of the gradient).
 * sfcvit_adamw_step / sfcvit_adamw_ema_step then run as they are.  Every operation is a separate, correctly rounded fp32
 * one; Inf and NaN propagate.
 *
 * acc[i] = float(grad[i])            when first != 0  (acc is not read)
 * acc[i] = acc[i] + float(grad[i])   otherwise: ONE fp32 add per element and call
 * Refused (SFCVIT_EINVAL, before any HIP call): a null grad or acc, n <= 0, a grad or acc that is not 16-byte aligned, an acc
 * that shares a byte with grad. */
int sfcvit_grad_accum(const void *grad /* bf16 [n] */, float *acc /* fp32 [n] */, int64_t n, int first, void *stream);

/* grad[i] = bf16_rne( (acc[i] + float(grad[i])) * scale ): one fp32 add, one fp32 multiply, one rounding, in place.
 * sumsq != NULL: *sumsq += sum_i float(grad_new[i])^2 -- the squares of the STORED bf16 values (what the AdamW kernel
 * will read).  Block partials go through `workspace` (SFCVIT_SUMSQ_WORKSPACE_BYTES) and are added in a fixed order.
 * No atomics: two runs, same bits.  sumsq == NULL: workspace may be NULL.
 * Refused: what sfcvit_grad_accum refuses, a scale that is not finite or <= 0, a sumsq without a workspace, a sumsq or
 * workspace that is not 4-byte aligned or shares a byte with grad or acc. */
int sfcvit_grad_accum_finish(void *grad, const float *acc, int64_t n, float scale, float *sumsq, void *workspace, void *stream);

/* Device-resident step state, 8 words (16-byte aligned): [0] dropout seed offset (uint32), [1] step (int32), [2] learning
 * rate (float, host-written), [3] 1 - beta1^step, [4] 1 / sqrt(1 - beta2^step).  sfcvit_step_advance increments the step
 * and refreshes [0], [3], [4]; run it once per training step before the forward (first node of a captured step).  The
 * reference keeps all of this on the host (torch.optim.AdamW's step counter, torch's Philox offset); on the device a
 * whole training step replays from one hipGraph (main.py:284's torch.compile(mode="reduce-overhead") intent). */
int sfcvit_step_advance(void *state, float beta1, float beta2, uint32_t seed_base, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SFCVIT_H */
