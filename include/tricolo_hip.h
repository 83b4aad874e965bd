/* tricolo_hip.h - C ABI of libtricolo_hip.so: the MI355X (gfx950) kernels under the TriCoLo training step.
 *
 * The reference (3dlg-hcvc/tricolo) is pure Python and has no FFI; its hot path bottoms out in third-party native
 * code (spconv, cuDNN via torchvision / torch.nn, cuBLAS).  This library is what sits under the reference's
 * encoder / loss modules instead (last row).  Each entry point names the reference call site
 * whose native work it replaces (paths relative to /root/reference).
 *
 * Conventions: plain pointers + sizes, all pointers are DEVICE pointers unless noted; `stream` is a hipStream_t
 * passed as void*; every call is asynchronous on that stream, allocates nothing, keeps no global state and returns
 * 0 on success, a hipError_t (>0) or a negative TRI_ERR_* code otherwise (text via tri_last_error()).  Activations
 * are channels-last [B, D, H, W, C] (2D tensors use D = 1), C a multiple of 4, stored as `act_fmt` says:
 * TRI_FMT_F32 (0: bf16x3 mode), TRI_FMT_BF16 (1: bf16 mode) or TRI_FMT_F16 (2: f16 mode; the 16-bit formats move half
 * the bytes of every pass and ARE the MFMA operand type of the conv kernels); accumulation / statistics are fp32 always.
 */
#ifndef TRICOLO_HIP_H
#define TRICOLO_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRI_FMT_F32 0
#define TRI_FMT_BF16 1
#define TRI_FMT_F16 2

int tri_version(void);
const char* tri_last_error(void);

/* Geometry of one convolution / dense layer.  Linear(in,out) is KD=KH=KW=1 on a 1x1x1 grid with B = rows. */
typedef struct TriConvDesc {
    int B, ID, IH, IW, Cin;   /* input grid, stored input channels (multiple of 4; 3-channel inputs are stored as 4) */
    int OD, OH, OW, Cout;     /* output grid, output channels (multiple of 32) */
    int KD, KH, KW, stride, pad_d, pad_h, pad_w;
} TriConvDesc;

/* ---- weight packing -----------------------------------------------------------------------------------------
 * fp32 parameter in the reference's own layout (addressed by element strides) -> MFMA operand rows
 * dst[row][tap * inner_pad + i], bf16 (fmt TRI_FMT_BF16 or 0) or f16 (fmt TRI_FMT_F16), zero padded to
 * tri_conv_kpad(ntaps, inner_pad).  w_lo != NULL (bf16 only) additionally receives the residual x - bf16(x)
 * (3-product split mode, fp32-grade accuracy).
 *   forward operand : rows = Cout, inner = Cin     dgrad operand : rows = Cin, inner = Cout (swap the strides)
 * Layouts: spconv SubMConv3d weight [Cout,kd,kh,kw,Cin] (sparse_cnn.py:12-32), torchvision conv [Cout,Cin,kh,kw]
 * (mv_cnn.py:44), nn.Linear [out,in].
 * frag != 0 (rows % 16 == 0): the same elements in MFMA-FRAGMENT-MAJOR order for the kernels that load their weight fragments straight
 * into registers (TRI_CONV_VOXG / VOXB / S2G): the [16 rows x 32 k] block (row tile rt, k-step ks) is 1 KiB at
 * ((rt * kpad / 32) + ks) * 512 elements, element (r, k) of it at ((k % 32) / 8 * 16 + r % 16) * 8 + k % 8 - lane (r, k / 8) of a
 * 16x16x32 A fragment reads its 8 elements as ONE contiguous 16-byte piece and a wave reads 1 KiB contiguously. */
int tri_conv_kpad(int ntaps, int cin_stored);
/* one packing job; tri_weight_prep_multi runs an array of them (DEVICE memory) in a single launch - one per tower and step */
typedef struct TriPrepDesc {
    const float* w;
    void* hi;
    void* lo;            /* NULL in the single-operand modes (bf16, f16) */
    long s_row, s_tap, s_inner;
    int rows, ntaps, inner, inner_pad, kpad, fmt;
    int frag;            /* 1: fragment-major order (see above) */
} TriPrepDesc;
int tri_weight_prep_multi(const TriPrepDesc* descs_dev, int n, void* stream);
int tri_weight_prep(const float* w, long s_row, long s_tap, long s_inner, int rows, int ntaps, int inner, int inner_pad,
                    void* w_hi, void* w_lo, int fmt, int frag, void* stream);

/* ---- token embedding (bigru.py:10,15) ------------------------------------------------------------------------------
 * fwd: emb[L,B,D] = W[tokens[B,L]] (already in the GRU's time-major order); bwd: dense dW[V,D], occurrences summed in
 * ascending (l, b) order (deterministic), row padding_idx zero (nn.Embedding(padding_idx=0) semantics). */
int tri_embedding_fwd(const int* tokens, const float* weight, int B, int L, int D, float* out, void* stream);
int tri_embedding_bwd(const int* tokens, const float* dout, int B, int L, int V, int D, int padding_idx, float* dweight, void* stream);

/* ---- text -> shape retrieval ------------------------------------------------------------------------
 * Device-side replacement of eval_retrieval.py:70-82,184-187: float64 similarities text[Nq,D] . shape[Ns,D]^T, the k best
 * shapes per query (descending, equal similarities -> higher index first, i.e. numpy's ascending argsort flipped) and the
 * 0-based rank of the query's own shape label[q] in the full ordering (first_hit, may be NULL together with label). */
int tri_retrieval_topk(const float* text, const float* shape, const int* label, int Nq, int Ns, int D, int k, int* topk_idx /* [Nq,k] */,
                       double* topk_sim /* [Nq,k] */, int* first_hit /* [Nq] */, void* stream);
/* The same ranking for a gallery of any size (csrc/gallery.hip): a workgroup owns a tile of queries and streams the shape rows past
 * them, keeping running top-k lists instead of a query's Ns similarities, so there is no limit on Ns.  Every similarity is the
 * float64 value tri_retrieval_topk forms for the pair: wherever both accept a call they return the same bits.  1 <= k <= min(Ns,
 * TRI_GALLERY_MAX_K); D <= 4096 (the float64 query tile takes at most 32 KiB of LDS: 8 queries per loaded shape row up to D = 512,
 * 4 / 2 / 1 up to 1024 / 2048 / 4096).  label and first_hit may be NULL (first_hit needs label); a label outside [0, Ns) gives
 * first_hit -1. */
#define TRI_GALLERY_MAX_K 64
int tri_retrieval_gallery(const float* text /* [Nq,D] */, const float* shape /* [Ns,D] */, const int* label /* [Nq] or NULL */, int Nq, int Ns,
                          int D, int k, int* topk_idx /* [Nq,k] */, double* topk_sim /* [Nq,k] */, int* first_hit /* [Nq] or NULL */,
                          void* stream);
/* Shape -> text: the same ranking (the same kernel, the same float64 bits, the same top k) where SEVERAL candidates are correct for a
 * query.  A query names a class, query_class[q]; the candidate rows of class g are class_rows[class_off[g] .. class_off[g + 1]) (CSR:
 * class_off ascending, class_off[ncls] <= Nc).  With b the row of the query's class that ranks first, first_hit[q] is the number of
 * candidates c != b that rank before (sim(q, b), b): the 0-based position of the first correct candidate.  first_hit[q] = -1 when
 * query_class[q] is outside [0, ncls) or the class holds no row (nothing is read for it); a class_rows entry outside [0, Nc) is
 * skipped, never dereferenced.  With class_off = 0..Nc and class_rows = 0..Nc-1 the three outputs are tri_retrieval_gallery's byte for
 * byte.  Limits and return codes are tri_retrieval_gallery's; first_hit may be NULL (then query_class, class_off and class_rows may be
 * NULL too), first_hit without all three is TRI_ERR_ARG. */
int tri_retrieval_classes(const float* query /* [Nq,D] */, const float* cand /* [Nc,D] */, const int* query_class /* [Nq] */,
                          const int* class_off /* [ncls+1] */, const int* class_rows, int Nq, int Nc, int D, int ncls, int k,
                          int* topk_idx /* [Nq,k] */, double* topk_sim /* [Nq,k] */, int* first_hit /* [Nq] or NULL */, void* stream);

/* ---- dense layers with <= 64 rows (MLP heads at the per-GPU batch) ---------------------------------------------
 * nn.Linear forward / backward of sparse_cnn.py:39-44, mv_cnn.py:21-26, bigru.py:12, clip_text.py:9-14 in three launches,
 * reading the fp32 parameter directly (no packed copy).  x [M,K], w [N,K] (torch layout), y / dout [M,N]; act 0 none /
 * 1 relu / 2 tanh; the backward entry points take the forward OUTPUT y and apply act' themselves.  split3 = bf16x3. */
int tri_linear_small_supported(int M, int K, int N);               /* M <= 64, K % 128 == 0, N % 128 == 0 */
int tri_linear_small_fwd(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int act, int split3, void* stream);
int tri_linear_small_dgrad(const float* dout, const float* y, const float* w, float* dx, int M, int K, int N, int act, int split3,
                           void* stream);
int tri_linear_small_wgrad(const float* x, const float* dout, const float* y, float* dw, float* db /* may be NULL */, int M, int K, int N,
                           int act, int split3, void* stream);
/* tri_linear_small_wgrad + tri_linear_small_dgrad of one layer in a single launch (same results) */
int tri_linear_small_bwd(const float* x, const float* dout, const float* y, const float* w, float* dx, float* dw, float* db, int M, int K,
                         int N, int act, int split3, void* stream);

/* ---- implicit-GEMM convolution on MFMA ------------------------------------------------------------------------
 * tri_conv_fwd replaces spconv.SubMConv3d (sparse_cnn.py:12,17,22,27,32; row_mask = active-site mask gives the
 * submanifold rule), every torchvision conv2d of net_1 (mv_cnn.py:29) and nn.Linear (sparse_cnn.py:39-44,
 * mv_cnn.py:21-26, bigru.py:12, clip_text.py:9-14; bias + act 0 none / 1 relu / 2 tanh fused).
 * stats (optional) receives [tri_conv_num_mtiles][2][Cout] per-tile column sums / sums of squares for BatchNorm.
 * tri_conv_dgrad / tri_conv_wgrad replace the autograd backward of the same call sites; `d` is always the FORWARD
 * descriptor.  wgrad writes dw through element strides, i.e. directly in the reference's parameter layout. */
/* split3: 0 = bf16 operands / fp32 activations, 1 = bf16x3 (hi + lo operands), 2 = 16-bit operands and activation storage (bf16 or f16) */
int tri_conv_num_mtiles(const TriConvDesc* d, int split3);
/* the same for a call that passes a compact row list (row_list = 1: row_pos + row_count): such launches are planned for the voxel
 * grids' occupancy (<= 25 %), so a small level may run split-K over its list where the dense call would not */
int tri_conv_num_records(const TriConvDesc* d, int split3, int row_list);
/* Kernel families of tri_conv_fwd / tri_conv_dgrad.  What each one serves, which calls it refuses or hands to the generic kernel, its
 * BatchNorm record count and its packed-operand order are one table: conv_families[] in csrc/conv_igemm.hip (Python: ops.CONV_FAMILIES). */
typedef enum TriConvFamily {
    TRI_CONV_IGEMM = 0,      /* conv_igemm_kernel: register-staged im2col, every layer and mode */
    TRI_CONV_DMA = 2,        /* conv_dma_kernel: LDS-DMA staging (16-bit storage, 64 | Cin) */
    TRI_CONV_HALO2D = 3,     /* conv_halo2d_kernel: 2D 3x3 / 1 / pad 1 */
    TRI_CONV_STEM = 4,       /* conv_stem_kernel: 4 stored input channels, stride 2, 64 outputs; forward only */
    TRI_CONV_HALO_ROWS = 5,  /* conv_halo_rows_kernel: the row-unit pipeline of the same layers */
    TRI_CONV_VOX0 = 6,       /* conv_vox0_kernel: voxel level 0; forward only; site mask as row_mask, refuses a row list */
    TRI_CONV_C64 = 9,        /* conv_c64_kernel: 64 -> 64 channels 3x3 / 1, both directions (7, 8, 11: A/B partners dropped in round 6) */
    TRI_CONV_S2D = 10,       /* conv_s2d_kernel: data gradient of the 64 -> 128 channel 3x3 / 2 layer */
    TRI_CONV_PW = 12,        /* conv_pw_kernel: 1x1 / 2 shortcuts */
    TRI_CONV_VOXG = 13,      /* conv_voxg_kernel: SubMConv3d on 2^3 / 4^3 / 8^3 grids, both directions; site mask, refuses a row list */
    TRI_CONV_VOXB = 14,      /* conv_voxb_kernel: voxel level 1 on 16^3 / 32^3 grids; forward only; site mask */
    TRI_CONV_S2G = 15        /* conv_s2g_kernel: forward of the 3x3 / 2 layers with >= 128 input channels; refuses row mask / list, bias,
                                activation, accumulate.  13 / 14 / 15 read FRAGMENT-MAJOR packed operands */
} TriConvFamily;
/* the word tri_conv_kernel_family returns: family | tile << 8 | split-K << 16 | samples per unit << 24 */
#define TRI_FAMILY_CODE_MASK 255     /* bits 0..7: TriConvFamily */
#define TRI_FAMILY_TILE_SHIFT 8      /* bits 8..15: output-channel tile width (halo kernels: 64-position blocks per row tile) */
#define TRI_FAMILY_SPLITK_SHIFT 16   /* bit 16 (IGEMM / DMA): the dense call runs split-K, or has more than 256 DMA k-steps: no row list */
#define TRI_FAMILY_SPU_SHIFT 24      /* bits 24..30 (VOXG): samples per unit = per BatchNorm record */
/* the family tri_conv_fwd (transposed = 0) / tri_conv_dgrad (transposed = 1) dispatches for this layer and mode.  For profilers. */
int tri_conv_kernel_family(const TriConvDesc* d, int transposed, int split3);
/* Kernel families of the weight gradient (tri_conv_wgrad, tri_conv_wgrad_partial, tri_conv_stem_wgrad_bn).  Which calls each one takes,
 * its slab layout and its grouping family are one table: wgrad_families[] in csrc/conv_wgrad.hip (Python: ops.WGRAD_FAMILIES). */
typedef enum TriWgradFamily {
    TRI_WGRAD_STAGED = 0,    /* conv_wgrad_kernel: register-staged im2col, every layer and mode */
    TRI_WGRAD_DMA = 2,       /* conv_wgrad_dma_kernel: LDS-DMA staging (16-bit storage, 8 | Cin, whole channel tiles) */
    TRI_WGRAD_STEM = 4,      /* conv_stem_wgrad_kernel: 4 stored input channels, stride 2, 64 outputs; dense calls, fused or not */
    TRI_WGRAD_VOX0 = 6,      /* conv_vox0_wgrad_kernel: voxel level 0; only with the site mask as row_mask */
    TRI_WGRAD_KROW = 7,      /* conv_wgrad_krow_kernel: resolution-keeping 3x3 layers, 64 | channels; dense calls */
    TRI_WGRAD_C64 = 9        /* conv_wgrad_c64_kernel: 64 -> 64 channels 3x3 / 1 from 6 row tiles per compute unit on; dense calls */
} TriWgradFamily;
/* features of a weight-gradient call */
#define TRI_WGRAD_MASK 1             /* row_mask */
#define TRI_WGRAD_ROWS 2             /* compact row list (row_pos + row_count) */
#define TRI_WGRAD_SPLIT3 4           /* 3-product split (fp32 storage) */
#define TRI_WGRAD_BNF 8              /* tri_conv_stem_wgrad_bn: dOut formed from the BatchNorm-backward inputs; no other feature */
/* the word tri_conv_wgrad_route returns: family | grouping family << 8 | tile rows << 12 | tile columns << 21 */
#define TRI_WGRAD_ROUTE_CODE_MASK 255    /* bits 0..7: TriWgradFamily */
#define TRI_WGRAD_ROUTE_GROUP_SHIFT 8    /* bits 8..11: the tri_conv_wgrad_group_info family whose launches this call may join (0: none) */
#define TRI_WGRAD_ROUTE_ROWS_SHIFT 12    /* bits 12..20: output channels of the dW tile one workgroup forms */
#define TRI_WGRAD_ROUTE_COLS_SHIFT 21    /* bits 21..30: its columns of K = (tap, channel); persistent kernels: the whole padded K */
/* the kernel a call with these features runs on this layer in this storage format, or the negative TRI_ERR_* it is refused with (text via
 * tri_last_error).  For profilers and timers. */
int tri_conv_wgrad_route(const TriConvDesc* d, int act_fmt, int features);
/* the layer's class, for callers that choose what to pass: 6 brick layer (conv_vox0_wgrad_kernel when the call passes the site mask),
 * 7 kernel-row layer, 2 DMA-capable, 0 otherwise.  Not the kernel of a particular call: that is tri_conv_wgrad_route. */
int tri_conv_wgrad_kernel_family(const TriConvDesc* d, int act_fmt);
/* split-K scratch a small-M layer needs (0 = none): pass at least this many bytes to tri_conv_fwd / tri_conv_dgrad */
size_t tri_conv_workspace(const TriConvDesc* d, int transposed);
int tri_conv_fwd(const TriConvDesc* d, const void* in, const void* w_hi, const void* w_lo, void* out, const uint8_t* row_mask,
                 const float* bias, int act, int accumulate, float* stats, int act_fmt, void* workspace, size_t workspace_bytes,
                 const int* row_pos /* optional compact row list, see tri_mask_compact */, const int* row_count /* DEVICE int */,
                 void* stream);
int tri_conv_dgrad(const TriConvDesc* d, const void* dout, const void* wt_hi, const void* wt_lo, void* din, const uint8_t* row_mask,
                   int accumulate, int act_fmt, void* workspace, size_t workspace_bytes,
                   const int* row_pos /* optional [B*ID*IH*IW]: a permutation of the input positions, the order in which the
                                         kernel's row tiles visit them.  For stride 2 pass the positions sorted by the parity of
                                         (coordinate + pad) per axis: a tile then only runs the 1-4 taps of 9 its rows can use
                                         (the other products are structurally zero).  Purely an execution-order hint. */,
                   const int* row_count /* optional DEVICE int: row_pos is a COMPACT list, only rows [0, *row_count) are computed
                                           (submanifold layers: the active sites, tri_mask_compact); other rows of din are NOT written */,
                   void* stream);
/* Data gradient that also takes the BatchNorm-backward sums of the BatchNorm whose OUTPUT gradient it produces: din is the gradient
 * w.r.t. relu(bn(y)) (relu_scale / relu_shift: the mask y * scale + shift > 0 is recomputed), w.r.t. relu(bn(y) + shortcut) whose
 * saved output is relu_out (mask relu_out > 0), or w.r.t. bn(y) itself (neither).  partial[records][2][C] receives sum g', sum g' * y
 * over the values AS STORED in din (g' = masked), the layout tri_bn_bwd_reduce writes and tri_bn_bwd_finalize sums: the separate
 * reduce pass over din / y (module/img_encoder/mv_cnn.py:44 BasicBlock backward: one per BatchNorm2d) is not launched at all.
 * tri_conv_dgrad_bn_records: number of records, or 0 when this layer's data-gradient kernel has no fused form (then call
 * tri_conv_dgrad and tri_bn_bwd_reduce). */
typedef struct TriConvBnSums {
    const void* y;            /* [B, ID, IH, IW, Cin] the BatchNorm's input, storage format of din */
    const float* relu_scale;  /* optional [Cin] */
    const float* relu_shift;
    const void* relu_out;     /* optional, shape of y */
    float* partial;           /* out */
} TriConvBnSums;
int tri_conv_dgrad_bn_records(const TriConvDesc* d, int accumulate, int act_fmt);
int tri_conv_dgrad_bn(const TriConvDesc* d, const void* dout, const void* wt_hi, const void* wt_lo, void* din, int accumulate,
                      int act_fmt, void* workspace, size_t workspace_bytes, const int* row_pos, const TriConvBnSums* sums, void* stream);
size_t tri_conv_wgrad_workspace(const TriConvDesc* d);
/* gather plan of a layer geometry (origin offset + tap validity bits per output position): build once, reuse every step */
size_t tri_conv_plan_bytes(const TriConvDesc* d);
int tri_conv_plan_build(const TriConvDesc* d, void* plan, void* stream);
int tri_conv_wgrad(const TriConvDesc* d, const void* in, const void* dout, const uint8_t* row_mask, const void* plan /* required */,
                   void* workspace, size_t workspace_bytes, float* dw, long s_co, long s_tap, long s_ci, int cin_real, int split3,
                   int act_fmt, float out_scale /* dw = out_scale * sum: undoes the f16 mode's gradient scaling */,
                   const int* row_pos, const int* row_count /* optional compact list of the output positions to contract over
                       (tri_mask_compact: the active sites of a submanifold layer) - executed work = active rows; row_mask unused */,
                   void* stream);
/* The same in two halves, so that a tower's backward pays ONE reduce launch instead of one per layer: tri_conv_wgrad_partial runs
 * the position-split partial kernel into `workspace` (which must stay untouched until the reduce) and fills *pending;
 * tri_wgrad_reduce_grouped sums the slabs of n pending layers into their dw (any n; TRI_WGRAD_GROUP_MAX layers per launch).
 * Same arithmetic and summation order as tri_conv_wgrad: results are bitwise identical. */
#ifndef TRI_WGRAD_GROUP_MAX
#define TRI_WGRAD_GROUP_MAX 24
#endif
typedef struct TriWgradReduce {
    const float* slab;
    float* dw;
    long s_co, s_tap, s_ci;
    int splits, Cout, Kpad, ntaps, cin_stored, cin_real, zlanes, nblocks;   /* zlanes 0: row form (one output channel per block, the
                                                                               parameter row written as one contiguous run) */
    float out_scale;
    int kw_real;                       /* 0, or (slabs whose kernel rows are padded to 2^kw_shift taps: stem 8, voxel level 0 4) the real kernel width */
    int kw_shift;
} TriWgradReduce;
int tri_conv_wgrad_partial(const TriConvDesc* d, const void* in, const void* dout, const uint8_t* row_mask, const void* plan /* required */,
                           void* workspace, size_t workspace_bytes, float* dw, long s_co, long s_tap, long s_ci, int cin_real, int split3,
                           int act_fmt, float out_scale, const int* row_pos, const int* row_count, TriWgradReduce* pending /* HOST, out */,
                           void* stream);
int tri_wgrad_reduce_grouped(const TriWgradReduce* pending /* HOST array */, int n, void* stream);
/* Same, and every workgroup that STORED an inf / NaN gradient element flags the optimizer's current attempt in `note` (the int32[4]
 * device record of tri_adam_guard / tri_adam_tick: note[2] = max(note[2], note[0] + note[3] + 1)) - the overflow scan of these tensors
 * (torch.cuda.amp.GradScaler's found_inf; tricolo_amd/optim.py) then needs no pass of its own.  note may be NULL. */
int tri_wgrad_reduce_grouped_noted(const TriWgradReduce* pending /* HOST array */, int n, int* note, void* stream);
/* Several layers' partial kernels in ONE launch (16-bit activation storage).  The launch's resident
 * workgroups are shared by the jobs, so each layer is cut into fewer, longer splits than alone: the fp32 slab traffic of the step
 * (splits x Cout x K per layer, written here and re-read by the reduce) shrinks by about the number of jobs.
 * tri_conv_wgrad_group_info: family 0 = the layer is not groupable (use tri_conv_wgrad_partial), else jobs of equal family may share
 * a launch; tiles = workgroups per split, steps = 64-position steps (the caller's budget: ~448 workgroups per launch).
 * tri_conv_wgrad_partial_group: n <= TRI_WGRAD_JOBS_MAX jobs of one family (dense position ranges or compact row lists, no row mask);
 * workspace sized by tri_conv_wgrad_workspace as before;
 * pending[i] (HOST, out) is job i's reduce descriptor for tri_wgrad_reduce_grouped. */
#define TRI_WGRAD_JOBS_MAX 12
typedef struct TriWgradJob {
    const TriConvDesc* d;
    const void* in;
    const void* dout;
    const void* plan;
    void* workspace;
    size_t workspace_bytes;
    float* dw;
    long s_co, s_tap, s_ci;
    int cin_real;
    float out_scale;
    const int* row_pos;                /* optional compact list of the output positions to contract over (tri_mask_compact) ... */
    const int* row_count;              /* ... and its device-side length, as tri_conv_wgrad_partial takes them */
} TriWgradJob;
/* Stem weight gradient fused with tri_maxpool_bn_bwd_apply (conv 7x7/2 -> BN -> ReLU -> MaxPool2d(3,2,1), mv_cnn.py:44): dW from the
 * conv output y, the pool's winning-tap map / pooled gradient and the BatchNorm-backward coefficients; the gradient w.r.t. the conv
 * output is never stored.  TRI_ERR_UNSUPPORTED when the layer does not run conv_stem_wgrad_kernel (then: apply + tri_conv_wgrad_partial). */
int tri_conv_stem_wgrad_bn(const TriConvDesc* d, const void* in, const void* y, const uint8_t* arg, const void* dpool, const float* c1,
                           const float* c2, const float* c3, const float* relu_scale, const float* relu_shift, void* workspace,
                           size_t workspace_bytes, float* dw, long s_co, long s_tap, long s_ci, int cin_real, int act_fmt, float out_scale,
                           TriWgradReduce* pending /* HOST, out */, void* stream);
int tri_conv_wgrad_group_info(const TriConvDesc* d, int act_fmt, int* family, int* tiles, int* steps);
int tri_conv_wgrad_partial_group(const TriWgradJob* jobs /* HOST array */, int n, int act_fmt, TriWgradReduce* pending /* HOST array, out */,
                                 void* stream);

/* ---- BatchNorm (train-mode statistics, eps / momentum as torch.nn.BatchNorm1d/2d) ----------------------------------
 * Replaces nn.BatchNorm1d over active voxels (sparse_cnn.py:13,18,23,28,33; count from a device counter) and the 20
 * BatchNorm2d of ResNet-18 (mv_cnn.py:29; count_host = N*H*W). */
int tri_bn_finalize(const float* partial, int ntiles, int C, const int* count_dev, int count_host, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked, float momentum,
                    float eps, float* mean, float* invstd, float* scale, float* shift, void* stream);
int tri_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* rm, const float* rv, float eps, float* mean,
                       float* invstd, float* scale, float* shift, void* stream);
int tri_bn_act(const void* y, const float* scale, const float* shift, const void* res, const float* rscale, const float* rshift,
               void* out, long M, int C, int relu, int act_fmt, void* stream);
int tri_relu_bwd(const void* dout, const void* out, void* g, long n, int act_fmt, void* stream);
int tri_bn_bwd_num_blocks(long M);
/* relu_scale / relu_shift (optional): g is the gradient w.r.t. relu(bn(y)); the mask y*scale+shift > 0 is recomputed */
/* relu_out (optional): g is the gradient w.r.t. relu(bn(y) + residual) and relu_out that ReLU's saved output (mask out > 0) */
int tri_bn_bwd_reduce(const void* y, const void* g, long M, int C, float* partial, const float* relu_scale, const float* relu_shift,
                      const void* relu_out, const uint8_t* row_mask /* optional: rows with 0 are skipped (never read) */, int act_fmt,
                      void* stream);
/* BatchNorm backward of a SMALL tensor (accepted up to M = 16,384 rows; the Python gate ops.bn_bwd uses it for M <= 512 only - from
 * ~1 k rows on the three-pass form is faster: this kernel's loads are 16 bytes per cache line) in ONE launch: a workgroup owns 4 / 8 channels for all positions - sums,
 * coefficients (double) and the apply pass without records or a finalize launch.  Arguments as tri_bn_bwd_reduce / _finalize / _apply
 * (dy may alias g); TRI_ERR_UNSUPPORTED for other shapes. */
int tri_bn_bwd_small(const void* y, const void* g, long M, int C, const int* count_dev, int count_host, const float* gamma,
                     const float* mean, const float* invstd, const float* relu_scale, const float* relu_shift, const void* relu_out,
                     void* g_masked, const uint8_t* row_mask, int keep_inactive, void* dy, float* dgamma, float* dbeta, float out_scale,
                     int act_fmt, void* stream);
int tri_bn_bwd_finalize(const float* partial, int nblk, int C, const int* count_dev, int count_host, const float* gamma,
                        const float* mean, const float* invstd, float* dgamma, float* dbeta, float* c1, float* c2, float* c3,
                        float out_scale /* dgamma, dbeta *= out_scale (g carries the f16 mode's gradient scale; dy keeps it) */,
                        void* stream);
int tri_bn_bwd_apply(const void* y, const void* g, const float* c1, const float* c2, const float* c3, const uint8_t* row_mask,
                     void* dy, long M, int C, const float* relu_scale, const float* relu_shift, const void* relu_out,
                     void* g_masked /* optional: receives g * (relu_out > 0), may alias g */,
                     int keep_inactive /* 0: rows with row_mask == 0 come out as zeros (a data gradient gathers them); 1: they are left
                                          untouched - for layers whose dy only feeds a weight gradient over the same mask (voxel level 0) */,
                     int act_fmt, void* stream);
/* BatchNorm backward of TWO tensors of one shape that share their upstream gradient - bn2 and the shortcut's BatchNorm of a down-sampling
 * BasicBlock (mv_cnn.py:20; out = relu(bn_a(ya) + bn_b(yb)), g = gradient of out, relu_out = out): the three passes serve both, g and
 * relu_out are read once.  partial_* [tri_bn_bwd_num_blocks(M)][2][C]; buf_* [5][C] = dgamma, dbeta, c1, c2, c3; g_masked (may alias g)
 * receives g * (out > 0). */
int tri_bn_bwd_pair_reduce(const void* ya, const void* yb, const void* g, const void* relu_out, long M, int C, float* partial_a,
                           float* partial_b, int act_fmt, void* stream);
int tri_bn_bwd_pair_finalize(const float* partial_a, const float* partial_b, int nblk, int C, int count_host, const float* gamma_a,
                             const float* mean_a, const float* invstd_a, float* buf_a, const float* gamma_b, const float* mean_b,
                             const float* invstd_b, float* buf_b, float out_scale, void* stream);
int tri_bn_bwd_pair_apply(const void* ya, const void* yb, const void* g, const void* relu_out, const float* buf_a, const float* buf_b,
                          void* dya, void* dyb, void* g_masked, long M, int C, int act_fmt, void* stream);

/* ---- pooling -------------------------------------------------------------------------------------------------
 * BN + ReLU + mask + spconv.SparseMaxPool3d(2,2) fused (sparse_cnn.py:13-15 ...), its backward routing;
 * nn.MaxPool2d(3,2,1) of the ResNet stem; AdaptiveAvgPool2d + torch.max over views (mv_cnn.py:29-31). */
int tri_bn_relu_pool3d_fwd(const void* y, const float* scale, const float* shift, const uint8_t* mask, int B, int D, int C,
                           void* pooled, uint8_t* mask_out, int act_fmt, void* stream);
/* Row-list forms of the voxel tower's backward passes (round 4): the routing pass over the ACTIVE pooled sites (out_pos / out_count = the
 * next level's tri_mask_compact list) and the whole BatchNorm backward (reduce + finalize + apply, three launches) over the level's own
 * list, rows outside the list neither read nor written (tri_bn_bwd_apply's keep_inactive contract).  Same values as the dense forms. */
int tri_pool3d_bwd_route_rows(const void* y, const float* scale, const float* shift, const uint8_t* mask, const void* pooled,
                              const void* dpooled, int B, int D, int C, void* g, const int* out_pos, const int* out_count, int act_fmt,
                              void* stream);
/* (round 5) the routing walk with the level's BatchNorm-backward sums folded in, as tri_pool3d_bwd_route_reduce does for the dense walk:
 * partial [tri_pool3d_bwd_route_rows_num_blocks][2][C] feeds tri_bn_bwd_finalize; the apply pass is then tri_bn_bwd_apply (site mask) or
 * tri_bn_bwd_apply_rows (dy = c1 * g + c2 + c3 * y on the rows of the level's own list only; dy may alias g).  C / 4 must divide 256.
 * All 2x2x2-window kernels need fewer than 2^31 sites and a 2-byte aligned mask (TRI_ERR_ARG otherwise). */
int tri_pool3d_bwd_route_rows_num_blocks(int B, int D, int C);
int tri_pool3d_bwd_route_rows_reduce(const void* y, const float* scale, const float* shift, const uint8_t* mask, const void* pooled,
                                     const void* dpooled, int B, int D, int C, void* g, const int* out_pos, const int* out_count,
                                     float* partial, int act_fmt, void* stream);
int tri_bn_bwd_apply_rows(const void* y, const void* g, const float* c1, const float* c2, const float* c3, void* dy, int C,
                          const int* row_pos, const int* row_count, long max_rows, int act_fmt, void* stream);
size_t tri_bn_bwd_rows_scratch(int C);
int tri_bn_bwd_rows(const void* y, const void* g, int C, const int* row_pos, const int* row_count, long max_rows, const float* gamma,
                    const float* mean, const float* invstd, void* dy, float* dgamma, float* dbeta, float out_scale, void* scratch,
                    int act_fmt, void* stream);
int tri_pool3d_bwd_route(const void* y, const float* scale, const float* shift, const uint8_t* mask, const void* pooled,
                         const void* dpooled, int B, int D, int C, void* g, int act_fmt, void* stream);
/* the same with the level's BatchNorm-backward sums folded in (sparse_cnn.py:12-35 backward: SparseMaxPool3d -> ReLU -> BatchNorm1d):
 * partial [tri_pool3d_bwd_route_reduce_num_blocks][2][C] = per-workgroup sums of g and g * y over the active sites, what
 * tri_bn_bwd_reduce would produce from a second pass; continue with tri_bn_bwd_finalize / tri_bn_bwd_apply.  C / 4 must divide 256. */
int tri_pool3d_bwd_route_reduce_num_blocks(int B, int D, int C);
int tri_pool3d_bwd_route_reduce(const void* y, const float* scale, const float* shift, const uint8_t* mask, const void* pooled,
                                const void* dpooled, int B, int D, int C, void* g, float* partial, int act_fmt, void* stream);
/* bn_scale / bn_shift (optional, [C]): pools relu(x * scale + shift), i.e. BatchNorm + ReLU + MaxPool2d of the ResNet stem in one pass */
int tri_maxpool2d_fwd(const void* x, int N, int H, int W, int C, void* out, uint8_t* arg /* [N,Ho,Wo,C] winning tap, may be NULL */,
                      const float* bn_scale, const float* bn_shift, int act_fmt, void* stream);
int tri_maxpool2d_bwd(const uint8_t* arg, const void* dout, int N, int H, int W, int C, void* dx, int act_fmt, void* stream);
/* stem backward without materialising the max-pool gradient (conv -> BN -> ReLU -> MaxPool2d(3,2,1), mv_cnn.py:44): the BatchNorm
 * backward passes read (y [N,H,W,C], arg [N,H/2,W/2,C], dpool [N,H/2,W/2,C]) and route the pooled gradient to the winning taps
 * on the fly.  reduce -> tri_bn_bwd_finalize(partial, tri_maxpool_bn_bwd_num_blocks(...), C, count = N*H*W) -> apply.  Same
 * values as tri_maxpool2d_bwd followed by tri_bn_bwd_reduce / _apply with relu_scale / relu_shift.  H, W even. */
int tri_maxpool_bn_bwd_num_blocks(int N, int H, int W);
int tri_maxpool_bn_bwd_reduce(const void* y, const uint8_t* arg, const void* dpool, int N, int H, int W, int C, float* partial,
                              const float* relu_scale, const float* relu_shift, int act_fmt, void* stream);
/* round 4: the same [blocks][2][C] sums from the POOLED tensors (pooled = the forward's max-pool output, which the next layer keeps):
 * sum(g) and sum(g y) are sums over windows, and an active window's winning activation is (pooled - shift) / scale; 50 MB instead of
 * 137 MB read at the bench shape.  Windows whose recovered activation would be ill-conditioned (|pooled| > 64 |gamma|) read the
 * stored y through the tap map.  16-bit storage, C % 8 == 0 and C / 8 a divisor of 256; else TRI_ERR_UNSUPPORTED. */
int tri_maxpool_bn_bwd_pooled_num_blocks(int N, int H, int W);
int tri_maxpool_bn_bwd_reduce_pooled(const void* pooled, const void* dpool, const void* y, const uint8_t* arg, int N, int H, int W, int C,
                                     float* partial, const float* relu_scale, const float* relu_shift, const float* gamma, int act_fmt,
                                     void* stream);
int tri_maxpool_bn_bwd_apply(const void* y, const uint8_t* arg, const void* dpool, int N, int H, int W, int C, const float* c1,
                             const float* c2, const float* c3, const float* relu_scale, const float* relu_shift, void* dy, int act_fmt,
                             void* stream);
int tri_avgpool_viewmax_fwd(const void* x, int B, int V, int HW, int C, float* out, int* arg, int act_fmt, void* stream);
int tri_avgpool_viewmax_bwd(const float* dout, const int* arg, int B, int V, int HW, int C, void* dx, int act_fmt, float scale, void* stream);

/* ---- layout converters (batch layout of tricolo/data/data_module.py:40-65) ---------------------------------------- */
/* dense [B,V,V,V,4] and mask [B*V^3 padded to 32 bytes] are zero-filled by the call (one fill when mask directly follows dense) */
int tri_voxel_scatter(const int* locs, const float* feats, int n, int B, int V, void* dense, uint8_t* mask, int act_fmt, void* stream);
/* the dataset's dense RGBA u8 grids [B,4,V,V,V] straight to the tower input (active <=> alpha != 0, feats =
 * RGB / 255; general_dataset.py:47-51,92-93) - no CPU COO build, no scatter.  mask must hold B*V^3 bytes (padded to 32). */
int tri_voxel_from_rgba_u8(const uint8_t* rgba, int B, int V, void* dense, uint8_t* mask, int act_fmt, void* stream);
int tri_mask_count(const uint8_t* mask, long n, int* count, void* stream);
/* instrumentation: *slot = wall_clock64() (100 MHz) at this point of the stream; tools/step_timeline.py */
int tri_debug_stamp(unsigned long long* slot, void* stream);
/* toolchain regression probe: copies n16 16-byte elements src -> dst through the raw-buffer builtins (form 0 load with a per-lane offset -
 * what the conv kernels use -, 1 load with an SGPR scalar offset, 2 / 3 the same for stores; csrc/misc.hip buffer_b128_probe_kernel) */
int tri_debug_buffer_b128_probe(const void* src, void* dst, long n16, int form, void* stream);
/* active-site list of a submanifold level: row_pos[0 .. *count) = positions with mask != 0, ascending; *count = how many.
 * Hand row_pos + count to tri_conv_fwd / tri_conv_dgrad: they then compute (and write) ONLY those rows - executed work =
 * active work (spconv's rulebook idea on a dense index space).  Split-K layers take the list too (slab row = list row).  scratch: tri_mask_compact_scratch(n) bytes. */
size_t tri_mask_compact_scratch(long n);
int tri_mask_compact(const uint8_t* mask, long n, int* row_pos, int* count, void* scratch, void* stream);
/* (round 5) the voxel tower's five site masks and five row lists up front: tri_mask_pyramid builds the masks of levels 1-4 (2x2x2 OR-pool,
 * what tri_bn_relu_pool3d_fwd writes as mask_out level by level - that argument may now be NULL) from the level-0 mask of [B, V, V, V]
 * grids in one launch (V % 16 == 0; masks[l - 1] holds B * (V >> l)^3 bytes rounded up to 32, padding zeroed); tri_mask_compact_multi is
 * tri_mask_compact of up to 8 masks in two launches (each list <= 2,097,152 sites).  Same masks, same lists, same counts. */
int tri_mask_pyramid(const uint8_t* mask0, int B, int V, uint8_t* const* masks, void* stream);
size_t tri_mask_compact_multi_scratch(const long* n, int nlist);
int tri_mask_compact_multi(const uint8_t* const* masks, const long* n, int nlist, int* const* rows, int* const* counts, void* scratch,
                           void* stream);
int tri_nchw3_to_nhwc4(const float* x, int N, int H, int W, void* out, int act_fmt, void* stream);
/* u8 images [N,3,H,W] -> channels-last [N,H,W,4], (u8/255 - mean[c]) / std[c] as ToTensor + Normalize of
 * general_dataset.py:87-89; mean3 / std3 are HOST pointers to three floats. */
int tri_nchw3_u8_to_nhwc4(const uint8_t* x, int N, int H, int W, const float* mean3, const float* std3, void* out, int act_fmt, void* stream);

/* ---- row ops ------------------------------------------------------------------------------------------------------
 * F.normalize(dim=1) (sparse_cnn.py:51, mv_cnn.py:33, bigru.py:18), bias gradients, activation backward. */
int tri_l2norm_fwd(const float* x, int rows, int D, float eps, float* z, float* norm, void* stream);
int tri_l2norm_bwd(const float* z, const float* norm, const float* dz, int rows, int D, float eps, float* dx, void* stream);
int tri_colsum(const float* g, long M, int C, float* out, void* stream);
int tri_axpy(const float* x, float a, float* y, long n, void* stream);
int tri_act_bwd(const float* dout, const float* out, float* g, long n, int act, void* stream);
/* dst (act_fmt storage) = scale * src (fp32), and back: the fp32 heads <-> 16-bit tower boundary of the voxel tower */
int tri_cast_from_f32(const float* src, void* dst, long n, float scale, int act_fmt, void* stream);
int tri_cast_to_f32(const void* src, float* dst, long n, int act_fmt, void* stream);

/* ---- persistent bidirectional GRU recurrence (nn.GRU(256,128,bidirectional) of text_encoder/bigru.py:11,17) -----------
 * xproj [L][B][768] = x_t W_ih^T + b_ih for both directions (768 = dir*384 + gate*128 + unit, gate order r,z,n);
 * w_hh [2][384][128], b_hh [2][384].  Outputs: hs [2][L][B][128], gates [2][L][B][128][4] (r,z,n,hn per unit) saved for backward,
 * hfinal [B][256] = cat(forward final state, reverse final state) (bigru.py:18).  tri_gru_bwd returns the gate
 * pre-activation gradients dgi [L][B][768], dgh [2][L][B][384] and h_{t-1} rows hprev [2][L][B][128]; the weight
 * gradients are then plain GEMMs (tri_conv_wgrad with 1x1 geometry).
 * split3: MFMA operand mode of the recurrence - 0 single bf16 products, 1 the 3-product bf16 hi/lo split (fp32-grade), 2 single f16
 * products (the f16 mode; the backward carries its gate gradients through LDS times 2^12).
 * Input range of tri_gru_bwd in the f16 mode: every gate gradient must satisfy |dgate| < 65504 / 4096 (~16), or f16(4096 dgate)
 * overflows to inf; with unit-size dhfinal the largest |dgate| is ~2.2, a real NT-Xent step is 2^-7 of that.  Resolution: 2^-24 / 4096
 * (f16 subnormals survive the conversion, the LDS round trip and the f16 MFMA on gfx950 - measured: at 2^-20 of unit scale the backward
 * is 1.4e-4 in relative L2 from float64, where flushing them would cost 2.7e-2; tests/test_gpu_text_tower.py,
 * profiles/r17/NOTES_text_tower.md).  The bf16 modes have fp32's range and scale exactly with powers of two. */
int tri_gru_fwd(const float* xproj, const float* w_hh, const float* b_hh, int B, int L, float* hs, float* gates, float* hfinal,
                int split3, void* stream);
int tri_gru_bwd(const float* dhfinal, const float* w_hh, const float* hs, const float* gates, int B, int L, float* dgi, float* dgh,
                float* hprev, float* dbias /* [ceil(B/16)][2][4][128] per-chunk sums of (dr, dz, dn_input, dn_hidden) */,
                int split3, void* stream);

/* up to 8 contiguous fp32 segments copied in one launch; srcs / dsts / n are HOST arrays of device pointers / element counts
 * (the per-step [w_ih_f; w_ih_r] ... concatenations of the nn.GRU parameters, bigru.py:11) */
int tri_copy_segments(const void* const* srcs, void* const* dsts, const long* n, int count, void* stream);
/* nn.GRU bias gradients from tri_gru_bwd's dbias: db_ih[dir] = (dr, dz, dn_input), db_hh[dir] = (dr, dz, dn_hidden), [384] each */
int tri_gru_bias_grads(const float* dbias, int nchunk, float* db_ih_f, float* db_hh_f, float* db_ih_r, float* db_hh_r, void* stream);

/* ---- NT-Xent loss, forward + backward fused (tricolo/loss/nt_xent.py:24-74) ------------------------------------------ */
/* One pair: loss (device scalar) = alpha * CE_rows(S) + (1 - alpha) * CE_cols(S), S = norm(za) norm(zb)^T / T; dza / dzb (optional,
 * both or neither) = d loss / d za, zb.  1 <= B <= 8192, 1 <= D <= 2048 (TRI_ERR_ARG otherwise).  The M = 2 case of the all-pairs
 * kernels below, with the same workspace layout: tri_ntxent_workspace(B, D) == tri_ntxent_multi_workspace(2, B, D). */
size_t tri_ntxent_workspace(int B, int D);
int tri_ntxent_fwd_bwd(const float* za, const float* zb, int B, int D, float temperature, float alpha, int norm, float* loss,
                       float* dza, float* dzb, void* workspace, size_t workspace_bytes, void* stream);
/* gradient half alone, from the workspace a tri_ntxent_fwd_bwd(dza = dzb = NULL) call filled; dloss (optional DEVICE scalar,
 * NULL = exactly 1) = upstream d(total)/d(loss), folded in */
int tri_ntxent_bwd(const float* za, const float* zb, int B, int D, float temperature, float alpha, int norm, const float* dloss,
                   float* dza, float* dzb, const void* workspace, size_t workspace_bytes, void* stream);
/* All pairs of a step at once (tricolo_net.py:56-63: the loss of every pair of modalities, summed): M = 2 or 3 embeddings
 * z[m] [B, D] (HOST array of device pointers, in the reference's modality order - the earlier one of a pair is the alpha
 * side), 4 launches forward, 1 backward.  losses [P + 1] (device) = the pair losses in itertools.combinations order, then
 * their sum ((l0 + l1) + l2 in fp32, as Python's sum()).  The backward takes the upstream gradients of the pair losses
 * (HOST array of device scalars, NULL entries / NULL array = 0) and of the total (device scalar or NULL) and writes
 * dz[m] = sum over m's pairs.  B <= 512, D % 4 == 0, 4 <= D <= 2048 (TRI_ERR_UNSUPPORTED otherwise: use the per-pair calls, which
 * run the same kernels and past this range a tiled similarity kernel). */
size_t tri_ntxent_multi_workspace(int M, int B, int D);
int tri_ntxent_multi_fwd(const float* const* z, int M, int B, int D, float temperature, float alpha, int norm, float* losses,
                         void* workspace, size_t workspace_bytes, void* stream);
int tri_ntxent_multi_bwd(const float* const* z, int M, int B, int D, float temperature, float alpha, int norm,
                         const float* const* dpair, const float* dtotal, float* const* dz, const void* workspace,
                         size_t workspace_bytes, void* stream);
/* The same four calls with a LEARNABLE temperature (CLIP's logit scale): s = clamp(*logit_scale, 0, max_logit_scale), 1 / T = exp(s),
 * logit_scale a DEVICE scalar that every kernel reads itself - a captured HIP graph follows the parameter from replay to replay.  The
 * backward forms also WRITE (not accumulate) dlogit_scale (device scalar) = d / d logit_scale with the upstreams folded in: exactly 0
 * outside [0, max_logit_scale], the boundaries included in the passing range (torch.clamp); row partials + a fixed-order double sum, no
 * atomics, one launch more than the fixed backward.  Same ranges and dispatch as the fixed twins; workspace
 * tri_ntxent_ls_workspace(M, B, D) (M = 2 for the single-pair calls), larger than the fixed one by [P][B] floats.  TRI_ERR_ARG for a NULL
 * logit_scale, a NULL dlogit_scale in a call that forms gradients, a negative or non-finite max_logit_scale, a smaller workspace. */
size_t tri_ntxent_ls_workspace(int M, int B, int D);
int tri_ntxent_ls_fwd_bwd(const float* za, const float* zb, int B, int D, const float* logit_scale, float max_logit_scale, float alpha,
                          int norm, float* loss, float* dza, float* dzb, float* dlogit_scale, void* workspace, size_t workspace_bytes,
                          void* stream);
int tri_ntxent_ls_bwd(const float* za, const float* zb, int B, int D, const float* logit_scale, float max_logit_scale, float alpha, int norm,
                      const float* dloss, float* dza, float* dzb, float* dlogit_scale, const void* workspace, size_t workspace_bytes,
                      void* stream);
int tri_ntxent_multi_ls_fwd(const float* const* z, int M, int B, int D, const float* logit_scale, float max_logit_scale, float alpha,
                            int norm, float* losses, void* workspace, size_t workspace_bytes, void* stream);
int tri_ntxent_multi_ls_bwd(const float* const* z, int M, int B, int D, const float* logit_scale, float max_logit_scale, float alpha,
                            int norm, const float* const* dpair, const float* dtotal, float* const* dz, float* dlogit_scale,
                            const void* workspace, size_t workspace_bytes, void* stream);

/* ---- Triplet loss, semi-hard with a hard fallback (tricolo/loss/triplet.py) ------------------------------------------------ */
/* loss = mean over S = {(i, j), j != i : d[i][i] < d[i][j] < d[i][i] + margin} of d[i][i] - d[i][j] + margin, over
 * H = {(i, j), j != i : d[i][j] < d[i][i]} when S is empty, NaN (0 / 0, every gradient NaN) when both are;
 * d[i][j] = sqrt(max(|zls[j]|^2 - 2 <zls[i], zis[j]> + |zis[i]|^2, 0)) in float64 from the fp32 rows, gradient 0 where d = 0.
 * Branch and counts are decided on the device.  counts (optional, device int[2]) = (|S|, |H|).  3 launches forward, 1 backward.
 * 2 <= B <= 4096, 1 <= D <= 2048 (TRI_ERR_UNSUPPORTED otherwise).  dloss: DEVICE scalar, upstream d(total)/d(loss), folded in. */
size_t tri_triplet_workspace(int B, int D);
int tri_triplet_fwd(const float* zis, const float* zls, int B, int D, double margin, float* loss, int* counts, void* workspace,
                    size_t workspace_bytes, void* stream);
int tri_triplet_bwd(const float* zis, const float* zls, int B, int D, double margin, const float* dloss, float* dzis, float* dzls,
                    const void* workspace, size_t workspace_bytes, void* stream);
/* All pairs of a step at once, same contract as tri_ntxent_multi_*: pair (a, b) in itertools.combinations order is
 * loss(zis = z[a], zls = z[b]); losses [P + 1] = pair losses, then (l0 + l1) + l2 in fp32; counts (optional) [P][2] = (|S|, |H|) per pair.
 * 2 <= B <= 512, D % 4 == 0, 4 <= D <= 2048 (TRI_ERR_UNSUPPORTED otherwise: use the per-pair calls). */
size_t tri_triplet_multi_workspace(int M, int B, int D);
int tri_triplet_multi_fwd(const float* const* z, int M, int B, int D, double margin, float* losses, int* counts, void* workspace,
                          size_t workspace_bytes, void* stream);
int tri_triplet_multi_bwd(const float* const* z, int M, int B, int D, double margin, const float* const* dpair, const float* dtotal,
                          float* const* dz, const void* workspace, size_t workspace_bytes, void* stream);

/* ---- Shape F1 / chamfer distance on point clouds (calculate_f1.py: knn_points(K=1) both ways, F1 at a distance) -------------- */
/* Batched one-sided nearest neighbour.  P [N][S1][3], Q [N][S2][3] fp32 contiguous (p_shared / q_shared != 0: that side is ONE
 * cloud [S][3] used for every n).  len_p / len_q (optional, device int64 [N]): rows at and beyond a length are padding and are never
 * read.  d2 [N][S1] = the smallest (ax-bx)^2 + (ay-by)^2 + (az-bz)^2 (fp32, formed from the differences) over the valid points of
 * Q[n]; idx (optional, int64 [N][S1]) = the lowest index that attains it.  Padding rows are written as 0 / -1, an empty Q[n]
 * gives +inf / -1.  Any S1, S2 in 0 .. 2^28, any N >= 0 (large batches are split over launches).  Bit-reproducible. */
int tri_nn_dist2(const float* P, const float* Q, const long* len_p, const long* len_q, int N, int S1, int S2, int p_shared, int q_shared,
                 float* d2, long* idx, void* stream);
/* Per cloud n: counts [N][T] (int) = valid points with sqrtf(d2) < thresholds[k] (thresholds: HOST array of T <= 8 floats), sums [N] =
 * fp32 sum of d2 over the valid points in a fixed order.  One launch. */
#define TRI_F1_MAX_THRESHOLDS 8
int tri_f1_counts(const float* d2, const long* lengths, int N, int S, const float* thresholds, int T, int* counts, float* sums, void* stream);
/* precision [T][N] = 100 * (count_p / len_p), recall [T][N] = 100 * (count_q / len_q), f1 = (2 * precision * recall) / (precision +
 * recall + eps), chamfer [N] (optional) = sum_p / len_p + sum_q / len_q: fp32, the reference's order of operations, correctly rounded
 * divisions.  Lengths default to S1 / S2; a length of 0 gives NaN (the mean of nothing), as the reference would. */
int tri_f1_finalize(const int* count_p, const int* count_q, const float* sum_p, const float* sum_q, const long* len_p, const long* len_q,
                    int N, int S1, int S2, int T, float eps, float* precision, float* recall, float* f1, float* chamfer, void* stream);

/* ---- Mesh surface sampling (calculate_f1.py: Meshes.get_bounding_boxes, scale_verts, sample_points_from_meshes) ---------------- */
/* A packed batch of N triangle meshes: verts [sumV][3] fp32, faces [sumF][3] int32 vertex indices LOCAL to their mesh, vert_off /
 * face_off device int64 [N + 1] (first 0, ascending), scale (optional, device fp32 [N]): one factor per mesh, applied to the vertices
 * as fl32(v * scale[n]) before anything else, as the reference scales its meshes before it samples them.  A vertex index outside the
 * mesh is clamped to the mesh's own vertices (callers validate on the host; the kernels never read beyond the mesh).
 *
 * Every mesh call takes the batch as one descriptor (csrc/mesh_batch.h lays the arrays out).  The first eight members are every
 * call's; the sampler's calls and tri_mesh_bbox read no material and take null in those three.  The groups after them are optional
 * and DECLARED, not inferred from null: `fields` names the groups the caller says are there.  A group that `fields` does not name
 * is never read, whatever its members hold.  What every call refuses with TRI_ERR_ARG before anything runs: a null descriptor, a
 * negative N or T, a bit in `fields` that the call does not take, TRI_MESH_MIPS without TRI_MESH_TEXTURES, T > 0 with a null
 * member in a declared texture or pyramid group (T == 0: both groups may be null), a null face_vn / mat_pbr in a declared group. */
#define TRI_MESH_TEXTURES 1u
#define TRI_MESH_MIPS 2u
#define TRI_MESH_NORMALS 4u
#define TRI_MESH_PBR 8u
typedef struct TriMeshBatch {       /* the members of csrc/mesh_batch.h's MeshBatch, in its order, then `fields` */
    const float* verts; const int* faces; const long* vert_off; const long* face_off;
    const int* face_mat; const float* mat_kd; const long* mat_off;
    int N;
    const float* face_uv; const int* mat_tex; const uint8_t* texels; const long* tex_off; const int* tex_size; int T;   /* TRI_MESH_TEXTURES */
    const uint8_t* mip_texels; const long* mip_off;                                                                     /* TRI_MESH_MIPS */
    const float* face_vn;                                                                                               /* TRI_MESH_NORMALS */
    const float* mat_pbr;                                                                                               /* TRI_MESH_PBR */
    unsigned fields;                /* the TRI_MESH_* groups that are there */
} TriMeshBatch;
size_t tri_mesh_batch_size(void);   /* sizeof(TriMeshBatch), for bindings that mirror the struct */

/* tri_mesh_bbox replaces gt_meshes.get_bounding_boxes() (calculate_f1.py:90): bbox [N][3][2] fp32 = per-axis (min, max) over ALL
 * vertices of the mesh, referenced by a face or not; a mesh without vertices gives zeros.  Not scaled.  Reads verts and vert_off. */
int tri_mesh_bbox(const TriMeshBatch* batch, float* bbox, void* stream);
/* The face-area CDF that sample_points_from_meshes (calculate_f1.py:125) draws its faces from: area = 0.5 * |(b - a) x (c - a)| in fp32
 * on the scaled vertices, cdf [sumF] float64 = the inclusive prefix sum of the areas per mesh, total [N] float64 = its last entry (0
 * for a mesh without faces).  Summed in float64 in 2,048-face chunks counted from the mesh's first face (chunk sums, a serial chain
 * over the sums, apply): the bits depend on the mesh alone, the CDF never decreases and a face of area 0 repeats the entry before it
 * exactly.  max_faces: at least the largest face count of the batch (it sizes the grid), below 2^31.  No atomics; bit-reproducible. */
int tri_mesh_face_cdf(const TriMeshBatch* batch, const float* scale, long max_faces, double* cdf, double* total, void* stream);
/* Replaces sample_points_from_meshes(meshes, S) (calculate_f1.py:125; normals are not produced).  For mesh n and sample s:
 * Philox4x32-10, key = (low, high 32 bits of seed), counter = (s, n, 0, 0) -> x0..x3; u_f = (x0 >> 8) * 2^-24, u1, u2 likewise from x1,
 * x2; the face is the smallest f with cdf[f] > u_f * total[n] (float64; a face of area 0 is never chosen); with r = sqrtf(u1) the point is
 * (1 - r) a + r (1 - u2) b + r u2 c in fp32 on the scaled vertices.  points [N][S][3] fp32, face_idx (optional) int64 [N][S], local
 * to the mesh.  A mesh without faces or with total area 0 gives zero rows and -1.  Row (n, s) depends on (seed, n, s) and the mesh
 * only - not on S, the launch shape or the other meshes.  Large batches are split over launches. */
int tri_mesh_sample_points(const TriMeshBatch* batch, const float* scale, const double* cdf, const double* total, int S,
                           unsigned long long seed, float* points, long* face_idx, void* stream);

/* ---- Multi-view rendering (data/preprocess_all_data.py:44-82: the pyrender scene, restated as a rasteriser) -------------------- */
/* The packed batch of the mesh sampler plus: face_mat int32 [sumF], the material of every face, local to its mesh; mat_kd fp32
 * [sumM][3] diffuse colours with mat_off int64 [N + 1]; cam fp32 [N][views][12] = eye[3], then the 3 x 3 world-to-camera rotation row
 * by row (the camera looks down -z, +y up).  image u8 [N][views][3][H][W]; visibility (optional) int32 [N][views][H][W]: the face
 * seen at the pixel centre, local to its mesh, -1 for background.  A perspective projection with vertical field of view yfov on an
 * H x W viewport; a face with a vertex nearer than znear is dropped whole (NO near-plane clipping), vertices snap to 1/256 pixel,
 * coverage by int64 edge functions at the pixel centres with the top-left rule, both sides visible, depth 1 / z interpolated in
 * fp32, the nearest face per pixel by a 64-bit atomic max (at bit-equal depth the lower face index): independent of the order in
 * which faces arrive, bit-reproducible.  Flat Lambert shading, Kd (0.1 + 3 / pi max(n . (0, 1, 0), 0)), white background.  The
 * arithmetic is spelled out at the head of csrc/raster.hip.  samples is 1 or 4 (below; anything else is TRI_ERR_ARG, and a
 * workspace of 0).  workspace: tri_raster_workspace(...) bytes of device memory, 16-byte aligned (0 for sizes tri_raster_render
 * refuses).  Limits of one call: fewer than 2^31 faces, fewer than 2^31 pixels over all meshes and views, at most 65535 views:
 * TRI_ERR_UNSUPPORTED before anything is launched.  Indices outside a mesh are clamped to it.
 *
 * ONE entry point renders every mode; the mode follows from batch->fields and samples, as the paragraphs below say: textured with
 * TRI_MESH_TEXTURES, mip-mapped with TRI_MESH_MIPS beside it, smooth with TRI_MESH_NORMALS, the metallic-roughness BRDF with
 * TRI_MESH_PBR, in any combination and at either sample count. */
size_t tri_raster_workspace(long sumF, int N, int views, int H, int W, int samples);
int tri_raster_render(const TriMeshBatch* batch, const float* cam, long sumF, int views, int H, int W, double yfov, double znear,
                      int samples, void* workspace, uint8_t* image, int* visibility, void* stream);

/* TRI_MESH_TEXTURES: map_Kd textures.  The batch's five texture fields (csrc/mesh_batch.h): face_uv fp32 [sumF][3][2], one (u, v)
 * per face corner, a NaN in face_uv[f][0][0] marks a face without texture coordinates; mat_tex int32 [sumM], a batch-global texture
 * index per material, -1 = none, anything else clamped to T - 1 (T == 0: nothing is textured); texels u8 [sumTexels][4] RGBA (alpha
 * ignored); tex_off int64 [T + 1] texel offsets; tex_size int32 [T][2] = (height, width); row 0 is the top of the image, v = 0 its
 * bottom.  Visibility is the untextured call's, bit for bit; the colour of a textured face is clamp((Kd c) shade, 0, 1) with c the
 * texture at the perspective-correct (u, v) of the pixel centre: repeat wrap, bilinear over the texel centres, NO mip-maps, every
 * operation in fp32 rounded on its own (spelled out at the head of csrc/raster.hip).  An untextured face - by its material, by the NaN
 * marker, or where (u, v) is not finite - is coloured exactly as without textures.  Same workspace, same limits.
 *
 * samples == 4: four coverage samples per pixel, for batches with and without textures.  The sample positions, in 1/256 pixel from
 * the pixel's top-left corner: (96, 32), (224, 96), (32, 160), (160, 224) - the 4x rotated grid, the centre is not among them.
 * Coverage, depth and the 64-bit key of a sample are the one-sample rules at the sample's position instead of the pixel centre (same
 * face set-up, top-left rule, atomic max).  Every sample is coloured as a pixel is with one sample - a textured face from the
 * perspective-correct (u, v) at the sample's own position - and the pixel is (c0 + c1 + c2 + c3 + 2) >> 2 per channel of the four u8
 * colours: a multisample resolve for untextured faces, 4x supersampling for textured ones.  image u8 [N][views][3][H][W];
 * visibility (optional) int32 [N][views][H][W][4]: the face at each sample, -1 for none.  Limits of one call: those of one sample,
 * with fewer than 2^31 SAMPLES (N views H W 4) in place of pixels.  The arithmetic is spelled out at the head of csrc/raster.hip. */

/* The mip pyramid of every texture of a batch (csrc/mesh_batch.h lays it out).  Texture t of size (H0, W0) has
 * L = floor(log2(max(H0, W0))) + 1 levels of size (max(1, H0 >> l), max(1, W0 >> l)); its chain starts at mip_off[t] (int64 [T + 1], the
 * running sum of the chain lengths, formed by the caller) of mip_texels u8 [sum_mip][4], the levels one after the other from level 0,
 * row major.  Level 0 is a copy of the texture; a texel of a level l >= 1 is the area-weighted box mean over the span of LEVEL 0 it
 * covers, in exact integers, (2 S + D) / (2 D) with D = H0 W0 (half rounds up), alpha 255.  One launch, no host synchronisation.
 * sum_texels and sum_mip are the numbers of texels the two arrays hold: no read leaves [0, min(tex_off[T], sum_texels) - 1], no write
 * [0, min(mip_off[T], sum_mip) - 1], whatever the tables say.  T == 0 or sum_mip == 0: nothing runs. */
int tri_texture_mips(const uint8_t* texels, const long* tex_off, const int* tex_size, int T, long sum_texels, const long* mip_off,
                     long sum_mip, uint8_t* mip_texels, void* stream);

/* TRI_MESH_MIPS (beside TRI_MESH_TEXTURES): tri_raster_render with mip-mapped textures, at either sample count: the same visibility,
 * bit for bit, the same workspace and limits.  mip_texels, mip_off: the pyramid of tri_texture_mips for this batch's textures.  A
 * textured face is coloured clamp((Kd c) shade, 0, 1) with c blended from two levels of the pyramid; the level of detail comes from
 * (u, v) at the position itself, one whole pixel to the right and one whole pixel down (the face's plane extended; with four samples
 * the step is still one pixel, no LOD bias).  Where the texture is magnified (rho <= 1) the colour is the one without the pyramid,
 * bit for bit.  The rule is spelled out at the head of csrc/raster.hip; it is a definition of this project, not compared with any
 * other renderer.  T == 0: every face is untextured and the pyramid may be null.
 *
 * TRI_MESH_NORMALS: smooth shading, in any of the six modes above, with the batch's corner normals face_vn fp32 [sumF][3][3]
 * (csrc/mesh_batch.h: one normal per face corner in the order of `faces`, not necessarily of unit length; a NaN in face_vn[f][0][0]
 * marks a face without normals, which is shaded flat exactly as before).  Visibility does not change, bit for bit: only the resolve
 * pass differs.  At the pixel centre - with four samples at each sample's own position - the normal is interpolated with the
 * perspective-correct weights of the textured modes, turned toward the eye by the sign of its dot product with eye - vertex 0, and
 * lit as the flat one is: Kd (0.1 + 3 / pi max(n_y / |n|, 0)); where the interpolated normal is not finite or has no length the
 * position takes the flat shade.  The arithmetic is spelled out at the head of csrc/raster.hip.
 *
 * TRI_MESH_PBR: the glTF 2.0 metallic-roughness BRDF in place of the Lambert shade, in any of the six modes above, flat or smooth,
 * with the batch's mat_pbr fp32 [sumM][2] = (metallic, roughness) per material, indexed like mat_kd (csrc/mesh_batch.h; metallic
 * clamped to [0, 1], roughness to [0.04, 1], a NaN takes the lower bound; a mesh without materials takes (0.2, 0.8)).  Visibility
 * does not change, bit for bit: only the resolve pass differs.  At the pixel centre - with four samples at each sample's own
 * position - the world position p on the winning face comes from the perspective-correct weights, v = (eye - p) / |eye - p|,
 * l = (0, 1, 0), h = (l + v) / |l + v|, n is the unit shading normal of the Lambert modes, base = Kd (times the texel), and
 *   colour = clamp(0.1 base + 3 NL ((1 - F) cdiff / pi + F G D / (4 NL NV)), 0, 1)
 * with Schlick's Fresnel term, the Smith-GGX geometry term and the GGX distribution of the glTF specification and the cosine clamps of
 * the Khronos reference shader; every sum, product and quotient is spelled out at the head of csrc/raster.hip.  A position where a
 * weight, |eye - p| or |l + v| is not finite or zero, or the normal has no finite length, takes the Lambert colour of the same
 * batch without TRI_MESH_PBR, bit for bit. */

/* Vertex normals of a packed batch, written as corner normals face_vn_out fp32 [sumF][3][3] for TRI_MESH_NORMALS.  A
 * definition of this project (head of csrc/mesh_normals.hip): area-weighted - the fp32 cross product of every face, clamped to
 * +-2^16 per component and rounded to fixed point with 36 fractional bits, is summed per VERTEX INDEX of its mesh with 64-bit integer
 * atomics, so the result does not depend on the order of the faces and is bit-reproducible - then normalised in float64 and rounded
 * to fp32.  fill 0: a face whose face_vn_in[f][0][0] is not NaN keeps its nine incoming values bit for bit and only the others are
 * computed (face_vn_in may be null: all are computed); fill 1: every face is computed.  A face with a corner whose sum is (0, 0, 0) is
 * written as nine NaNs.  workspace: tri_mesh_vertex_normals_workspace(sumV) bytes of device memory (24 per vertex), 8-byte aligned.
 * Three launches on the stream, no host synchronisation.  Fewer than 2^31 faces and vertices.  Takes no optional group: the
 * incoming normals are face_vn_in, not the batch's face_vn. */
size_t tri_mesh_vertex_normals_workspace(long sumV);
int tri_mesh_vertex_normals(const TriMeshBatch* batch, long sumV, long sumF, int fill, void* workspace, const float* face_vn_in,
                            float* face_vn_out, void* stream);

/* One colour per face for the voxeliser: colours fp32 [sumF][3] = Kd for an untextured face, else Kd times the mean of four bilinear
 * samples of its texture, at barycentric (1/3, 1/3, 1/3), (2/3, 1/6, 1/6), (1/6, 2/3, 1/6), (1/6, 1/6, 2/3) of the face's UVs (used
 * affinely; summed in this order, times 0.25f).  A face with a sample at a non-finite (u, v) is untextured.  Not clamped.
 * Takes TRI_MESH_TEXTURES and no other group. */
int tri_mesh_face_colours(const TriMeshBatch* batch, long sumF, float* colours, void* stream);

/* ---- Coloured solid voxel grids from meshes (no counterpart in the reference, which reads downloaded NRRD grids) --------------- */
/* The packed batch of tri_raster_render plus frame fp32 [N][4] = (origin x, y, z, cell size) per mesh.  grid u8 [N][4][V][V][V],
 * indexed [channel][x][y][z] (mesh x, y, z -> grid i, j, k); labels (optional) u8 [N][V][V][V]: 0 exterior, 1 surface, 2 interior.
 * Vertices snap to 1/256 voxel; a voxel is a surface voxel when the closed box [256 i, 256 (i + 1)]^3 and a face overlap (thirteen
 * separating-axis tests, exact in int64; touching counts; zero-area faces and faces with a vertex beyond 2^17 units are dropped).
 * Its colour is the rounded mean of floor(255 clamp(Kd, 0, 1) + 0.5) over all overlapping faces, every face weighing the same,
 * summed with integer atomics: independent of the order in which faces arrive, bit-reproducible.  fill 0 = surface only; fill 1 =
 * carve: a non-surface voxel with a surface voxel on all six axis rays is interior and takes the colour of the nearest one (ties in
 * the order -x, +x, -y, +y, -z, +z).  Alpha 255 on surface and interior voxels; everything 0 elsewhere.  A mesh with cell <= 0 or a
 * non-finite frame gives an all-zero grid.  The arithmetic is spelled out at the head of csrc/voxelize.hip.  workspace:
 * tri_voxelize_workspace(...) bytes of device memory, 16-byte aligned (0 for sizes tri_voxelize_meshes refuses).  V must be 32, 64
 * or 128; fewer than 2^24 faces and fewer than 2^31 voxels in one call: TRI_ERR_UNSUPPORTED before anything is launched.  Takes no
 * optional group. */
size_t tri_voxelize_workspace(long sumF, int N, int V);
int tri_voxelize_meshes(const TriMeshBatch* batch, const float* frame, long sumF, int V, int fill, void* workspace, uint8_t* grid,
                        uint8_t* labels, void* stream);

/* ---- Bicubic antialiased resize of u8 renderings (general_dataset.py:63-65: Resize(image_size, BICUBIC, antialias=True)) ------- */
/* in [planes][Hin][Win] u8 -> out [planes][Hout][Wout] u8, both contiguous: cast to fp32, the separable bicubic (a = -0.5) antialias
 * filter of ATen's _upsample_bicubic2d_aa (width pass first; per axis scale = n_in / n_out, support = 2 max(scale, 1), windows clipped
 * at the borders and renormalised), clamp to [0, 255], round half to even.  Any sizes, down and up; Hin == Hout && Win == Wout copies.
 * fp32 accumulation in tap order, no atomics: bit-reproducible.  workspace: tri_resize_bicubic_aa_workspace(...) bytes of device
 * memory, 16-byte aligned (the per-axis window / weight tables, written by the call).  TRI_ERR_UNSUPPORTED when one output row's
 * window and the tables exceed 64 KiB of LDS (nothing is truncated). */
size_t tri_resize_bicubic_aa_workspace(int Hin, int Win, int Hout, int Wout);
int tri_resize_bicubic_aa_u8(const uint8_t* in, int planes, int Hin, int Win, uint8_t* out, int Hout, int Wout, void* workspace,
                             void* stream);

/* ---- Adam (torch.optim.Adam as instantiated by config/config.yaml:50-53, tricolo_net.py:43-44) ------------------------ */
/* `step` is a DEVICE int[4]: [0] optimizer steps applied (the t of the bias corrections; tri_adam_tick adds one), [1] the running count
 * of gradient elements the update kernels skipped because they were inf / NaN (per-element fallback: such an element leaves p, m and v
 * untouched), [2] attempt number of the last step whose gradient tri_adam_guard* found non-finite, [3] steps skipped whole.
 * Per-step overflow guard of the 16-bit modes (torch.cuda.amp.GradScaler's rule, decided on the device so that it replays inside a HIP
 * graph): call tri_adam_guard / tri_adam_guard_segments over the step's gradient BEFORE tri_adam_tick; when it finds an inf / NaN the
 * tick counts a skipped step instead of an applied one and the update kernels return without touching p, m, v. */
int tri_adam_guard(const float* g, long n, int* step, void* stream);
int tri_adam_guard_segments(const void* grad_ptrs, const long* grad_starts, int nseg, long n, int* step, void* stream);
int tri_adam_tick(int* step, void* stream);
/* lr_dev (optional, DEVICE float): when not NULL the learning rate is read from it at run time, so a captured HIP graph
 * follows a schedule (LrDecayCallback of train.py) without re-capture; `lr` is used otherwise.  Bias corrections in double. */
int tri_adam_step(float* p, const float* g, float* m, float* v, long n, const int* step, float lr, const float* lr_dev, float b1, float b2,
                  float eps, float wd, float gscale, void* stream);
/* the same update with the gradients read in place: grad_ptrs = DEVICE array of nseg device pointers (NULL = no gradient: the
 * segment is SKIPPED like torch.optim.Adam skips parameters whose .grad is None), grad_starts = DEVICE array of the flat start offset of each segment (ascending, first 0); segment sizes and n are
 * multiples of 4, gradient tensors 16-byte aligned.  Saves the flat-gradient concatenation pass of the single-GPU step. */
int tri_adam_step_segments(float* p, const void* grad_ptrs, const long* grad_starts, int nseg, float* m, float* v, long n,
                           const int* step, float lr, const float* lr_dev, float b1, float b2, float eps, float wd, float gscale,
                           void* stream);

/* ---- Gradient clipping, decided on the device (torch.nn.utils.clip_grad_norm_ / clip_grad_value_; csrc/adam.hip) -------------- */
/* Launch order of a clipped step: tri_adam_guard*, tri_adam_tick, tri_grad_sumsq*, tri_grad_clip_coef, tri_adam_step*_clipped.  Nothing
 * here uses an atomic or a ticket: the same input gives the same bits, also replayed from a HIP graph.
 * tri_grad_norm_blocks(n): how many doubles ONE tri_grad_sumsq / tri_grad_sumsq_segments call over n elements writes to `partial` - a
 * function of n alone (1 <= blocks <= 4096; no stream, no device memory; n < 0 is TRI_ERR_ARG). */
int tri_grad_norm_blocks(long n);
/* partial[b] = sum of (double)g[i] * (double)g[i] over workgroup b's share of the elements (a function of n and the grid only), for
 * every b < tri_grad_norm_blocks(n); nothing else is written.  Any n >= 0 (n == 0 writes one 0.0; g is not looked at), g 4-byte aligned:
 * scalar head up to the first 16-byte boundary, 16-byte body, scalar tail. */
int tri_grad_sumsq(const float* g, long n, double* partial, void* stream);
/* the same over the pointer table of tri_adam_step_segments (grad_ptrs / grad_starts: DEVICE arrays of nseg entries, 1 <= nseg <= 1024,
 * segment sizes and n multiples of 4, gradients 16-byte aligned; n = the flat size the starts count in).  A NULL segment is NOT part of
 * the norm: the update skips it, as torch.optim.Adam ignores a parameter without a gradient. */
int tri_grad_sumsq_segments(const void* grad_ptrs, const long* grad_starts, int nseg, long n, double* partial, void* stream);
/* One workgroup adds partial[0 .. nblk) in a fixed order (nblk >= 0; several tri_grad_sumsq calls may have filled consecutive parts) and
 * computes, in double:  total = |gscale| * sqrt(sum),  rec[0] = (float)total,  c = max_norm / (total + 1e-6),
 * rec[1] = c < 1 ? (float)c : 1.0f.  A total that is inf / NaN gives rec[1] = 1.0f and rec[0] keeps the non-finite value: that step
 * belongs to the guard.  clipped[0] += 1 (one thread) when and only when rec[1] < 1.  max_norm = +inf measures only (rec[1] = 1.0f).
 * rec: DEVICE float[2], clipped: DEVICE int[1].  TRI_ERR_ARG: max_norm <= 0 or NaN, nblk < 0, rec or clipped NULL (partial NULL with
 * nblk > 0). */
int tri_grad_clip_coef(const double* partial, int nblk, float gscale, float max_norm, float* rec, int* clipped, void* stream);
/* tri_adam_step / tri_adam_step_segments with  gi = clamp(g * (gscale * coef), -clip_value, clip_value) + wd * p.  coef is read from
 * coef_dev at run time (DEVICE float, e.g. rec + 1 of tri_grad_clip_coef; NULL = 1) and gscale * coef is formed once, in fp32.  The clamp
 * exists only in a separate instantiation, launched when clip_value is finite; clip_value = +inf runs the expression of the plain entry
 * points with that one scalar replaced, so coef == 1 gives their bits.  clip_value <= 0 or NaN is TRI_ERR_ARG. */
int tri_adam_step_clipped(float* p, const float* g, float* m, float* v, long n, const int* step, float lr, const float* lr_dev, float b1,
                          float b2, float eps, float wd, float gscale, const float* coef_dev, float clip_value, void* stream);
int tri_adam_step_segments_clipped(float* p, const void* grad_ptrs, const long* grad_starts, int nseg, float* m, float* v, long n,
                                   const int* step, float lr, const float* lr_dev, float b1, float b2, float eps, float wd, float gscale,
                                   const float* coef_dev, float clip_value, void* stream);

/* ---- Dynamic loss scaling, decided on the device (torch.cuda.amp.GradScaler's back-off and growth; csrc/adam.hip) --------------- */
/* The step's backward is seeded with the DEVICE scalar state[0] = s instead of 1 (the loss kernels read their upstream gradient from a
 * device pointer), so every gradient of the step carries s.  Launch order of such a step: tri_adam_guard*, tri_adam_tick,
 * (tri_grad_sumsq*,) tri_loss_scale_step, tri_adam_step*_clipped with coef_dev = rec + 1.  It takes tri_grad_clip_coef's place: one
 * workgroup adds partial[0 .. nblk) in that call's order and computes, in double and with s, 1 / s as state[0], state[1] hold them on entry,
 *     total = |gscale| * (1 / s) * sqrt(sum),  rec[0] = (float)total          (the norm of the TRUE gradient)
 *     c = max_norm / (total + 1e-6) when that is < 1, else 1; 1 when total is inf / NaN or nblk == 0
 *     rec[1] = c * (1 / s),  clipped[0] += 1 when c < 1
 * and then moves the scale the NEXT backward reads.  The step counts as skipped when step[2] == step[0] + step[3] (after the tick):
 *     skipped:  streak = 0;  if s > min_scale: s = max(s / 2, min_scale), backoffs += 1
 *     applied:  streak += 1; if streak >= growth_interval: streak = 0, and if s < max_scale: s = min(2 s, max_scale), growths += 1
 *     state = {s, 1 / s}
 * state: DEVICE float[2]; cnt: DEVICE int[3] = {streak, backoffs, growths}; step: DEVICE int[4], read only; partial may be NULL with
 * nblk == 0 (no norm clipping: pass max_norm = +inf); rec: DEVICE float[2]; clipped: DEVICE int[1].  Every scale is a power of two, so
 * 1 / s, c * (1 / s) and gscale * (1 / s) are exact, and with s = 1 rec holds tri_grad_clip_coef's bits.  No atomics: plain stores by one
 * thread.  TRI_ERR_ARG: a NULL operand, nblk < 0, max_norm <= 0 or NaN, growth_interval < 1, min_scale or max_scale not a power of two in
 * [2^-100, 2^100], min_scale > max_scale (state[0] is the caller's to keep inside them: it is not looked at on the host). */
int tri_loss_scale_step(float* state, int* cnt, const int* step, const double* partial, int nblk, float gscale, float max_norm,
                        int growth_interval, float min_scale, float max_scale, float* rec, int* clipped, void* stream);

/* ---- Counter-based dropout (the Dropout(0.1) of the reference's clip_text.py / clip_img.py heads; csrc/dropout.hip) ------------ */
/* used[0] = step[0]; step[0] += 1   (one thread; device int64 [1] each).  Stream-ordered: every later launch on `stream` that reads
 * `used` sees the value of THIS forward, also when the launches are replayed from a HIP graph. */
int tri_dropout_tick(long long* step, long long* used, void* stream);
/* y[r][c] = x[r][c] * m(r, c),  m = 0 when dropped, `scale` when kept: ONE fp32 multiply per element (inf / NaN propagate as in torch:
 * inf * 0 = NaN).  x, y: contiguous fp32 [rows][cols], distinct buffers, any cols >= 1, 4-byte alignment is all that is assumed
 * (16-byte accesses only where cols % 4 == 0 and both pointers are 16-byte aligned).
 * Element (r, c) is dropped iff  (w >> 8) < threshold,  w = word (c & 3) of Philox4x32-10(key = (seed & 0xffffffff, seed >> 32),
 * counter = (c >> 2, (row0 + r) & 0xffffffff, used[0] & 0xffffffff, tower)).   threshold in [0, 2^24] = round(p * 2^24).
 * Forward and backward are the same call (dx = dy * m).  rows == 0 returns success without a launch (pointers are not looked at);
 * threshold > 2^24, cols < 1, rows < 0 or a null pointer is TRI_ERR_ARG. */
int tri_dropout_apply(const float* x, float* y, long rows, int cols, unsigned threshold, float scale, unsigned long long seed,
                      const long long* used, unsigned long long row0, unsigned tower, void* stream);

#ifdef __cplusplus
}
#endif
#endif
