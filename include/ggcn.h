/* ggcn.h -- C ABI of libggcn_hip.so: the gated graph-convolution hot path of
 * laiviet/ed-gated-gcn as hand-written HIP kernels for MI355X (gfx950).
 *
 * The reference has no native code and no FFI: its boundary for this path is
 * the Python class GraphConvolution (models/gcn.py:9-45) and the ~20 lines of
 * BertAmir55.forward that wrap it (models/bert_amir5.py:621-640).  These entry
 * points are what a binding for that path calls; each one names the reference
 * lines it replaces.  INTEGRATION.md shows the reference-side binding (a ctypes
 * stub behind the unchanged nn.Module signature).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (hipMalloc'd or a torch CUDA/HIP tensor's
 *    data_ptr) unless named host_*; nothing is copied, owned or freed here;
 *  - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*;
 *    NULL = the default stream); no call synchronises, allocates or frees, so
 *    every call may be captured in a hipGraph;
 *  - return 0 on success, a GGCN_E* code otherwise; ggcn_last_error() gives the
 *    message of the calling thread's last failure (never NULL);
 *  - feature matrices are row-major fp32 with an explicit leading dimension in
 *    ELEMENTS; a batch of B graphs of T nodes is the N = B*T rows b*T .. b*T+T-1;
 *  - batched CSR: rowptr int32[N+1], colidx int32[nnz] holding GLOBAL node ids
 *    (block-diagonal: every id of row i lies in i's own graph), vals fp32[nnz]
 *    or NULL for a binary adjacency (all ones);
 *  - row masks (graphs of at most GGCN_MASK_MAX_T = 256 nodes): rowmask uint32[N][W], W = ceil(T/32) words
 *    per node, bit j%32 of word j/32 of node b*T+i set iff adj[b,i,j] != 0 -- the 0/1 adjacency at one bit
 *    per entry (T <= 32: one word per node), consumed by ggcn_layer_fused / ggcn_block_fused.
 */
#ifndef GGCN_H
#define GGCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped when a prototype, struct or enum CHANGES.  Added functions alone do not bump it: a binding that declares a function
 * an older library lacks fails at load time on the missing symbol (14 also covers ggcn_layer_fused_bf16_drop / _wide, ggcn_block_fused_bf16 and ggcn_aggregate_bf16). */
#define GGCN_ABI_VERSION 14
#define GGCN_MASK_MAX_T 256   /* largest graph the row-mask (one-launch) path takes */

typedef void *ggcn_stream_t;

enum ggcn_status {
    GGCN_OK = 0,
    GGCN_EINVAL = 1,       /* bad argument (null pointer, negative size, misaligned, ...) */
    GGCN_ELAUNCH = 2,      /* the HIP runtime refused the launch */
    GGCN_EUNSUPPORTED = 3  /* valid request this build has no kernel for */
};

/* dtype of a dense adjacency handed to ggcn_csr_from_dense (models/gcn.py:33
 * `adj.float()` accepts any real dtype). */
enum ggcn_adj_dtype {
    GGCN_ADJ_F32 = 0,
    GGCN_ADJ_U8 = 1,   /* torch.uint8 and torch.bool */
    GGCN_ADJ_I32 = 2,
    GGCN_ADJ_I64 = 3,
    GGCN_ADJ_F64 = 4,
    GGCN_ADJ_F16 = 5
};

/* bits of the `flags` word written by ggcn_csr_from_dense */
enum ggcn_csr_flags {
    GGCN_FLAG_WEIGHTED = 1 /* some non-zero entry differs from 1: the adjacency carries edge weights */
};

/* arithmetic of the dense linear (models/gcn.py:34 `torch.matmul(text, weight)`) */
enum ggcn_precision {
    GGCN_PREC_BF16X3 = 0,  /* fp32 operands split into bf16 hi+lo, 3 bf16 MFMAs per
                              product, fp32 accumulate: |err| ~ 2^-16 |x||w| per product */
    GGCN_PREC_FP32 = 1,    /* v_mfma_f32_32x32x2_f32: a k-ordered fp32 FMA chain, exact fp32 */
    GGCN_PREC_F16MX8 = 2,  /* operands split into fp16 hi + residual; hi.hi on the fp16 MFMA, both cross
                              terms in ONE block-scaled fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4):
                              2/3 of bf16x3's matrix-core time, |err| ~ 2^-15 |x||w| per product.
                              Needs |x|, |w| < 65504 (fp16 range; larger values saturate to inf) */
    GGCN_PREC_F16 = 3,     /* HALF-PRECISION FEATURES ONLY (ggcn_linear_h): plain fp16 MFMA on the fp16 image of W
                              (the fp16 fragments of the GGCN_PREC_F16MX8 pack), fp32 accumulate; |err| ~ 2^-12 |x||w|
                              per product -- below the rounding of the fp16 output it feeds */
    GGCN_PREC_F16MX6 = 4   /* the F16MX8 scheme with the correction products in fp6 (e2m3): gfx950 runs the block-scaled
                              MFMA twice as fast when both operands are 6-bit, so a product costs 3/4 of F16MX8's
                              matrix-core time.  e2m3 spans 6 binades, so both operands carry TRUE per-(row or column,
                              32 k) power-of-two scales (the activations' are computed in the kernel); |err| as F16MX8
                              (+10 %).  Same range rule.  Taken by ggcn_layer_fused / ggcn_block_fused for graphs of
                              <= 32 nodes with K % 32 == 0 and 16-byte aligned rows; its own ggcn_weight_pack image */
};

int ggcn_abi_version(void);
/* 1 when the library holds the experimental GGCN_PREC_F16MX6 form of the one-launch layer (csrc: make F16MX6=1); the
 * product build does not (measured slower than GGCN_PREC_F16MX8) and refuses that precision with GGCN_EUNSUPPORTED. */
int ggcn_has_f16mx6(void);
const char *ggcn_last_error(void);

/* ---- batched CSR from the reference's dense adjacency ---------------------
 * Replaces models/gcn.py:33 (`adj.float()`) and the structure half of :35/:41.
 * adj is [B,T,T] of `adj_dtype` with strides in ELEMENTS (the reference passes
 * a non-contiguous slice, models/bert_amir5.py:589).  Every non-zero adj[b,i,j]
 * becomes colidx entry b*T+j of row b*T+i (ascending j) with its value in vals
 * (vals may be NULL when the caller knows adj is 0/1).  `capacity` is the
 * number of entries colidx/vals can hold (B*T*T always suffices); entries
 * beyond it are dropped (rowptr still holds the true counts).
 * rowmask (NULL or uint32[B*T*ceil(T/32)], needs T <= GGCN_MASK_MAX_T) receives the row masks; flags (NULL or
 * one device int32) receives ggcn_csr_flags.
 * `workspace` needs ggcn_csr_workspace_bytes(B*T) bytes. */
size_t ggcn_csr_workspace_bytes(int64_t n_rows);
int ggcn_csr_from_dense(const void *adj, int adj_dtype, int B, int T,
                        int64_t stride_b, int64_t stride_r, int64_t stride_c,
                        int32_t *rowptr, int32_t *colidx, float *vals, int64_t capacity,
                        uint32_t *rowmask, int32_t *flags,
                        void *workspace, ggcn_stream_t stream);

/* Row masks straight from the dense adjacency (T <= GGCN_MASK_MAX_T): one pass, no CSR arrays.  This is all
 * ggcn_layer_fused needs, so the drop-in forward(text, adj) builds nothing else. */
int ggcn_rowmask_from_dense(const void *adj, int adj_dtype, int B, int T,
                            int64_t stride_b, int64_t stride_r, int64_t stride_c,
                            uint32_t *rowmask, int32_t *flags, ggcn_stream_t stream);

/* Transposed batched CSR (rows = source nodes): the backward pass applies A^T (train.py:120).  rowptr_t
 * int32[N+1], colidx_t int32[nnz], vals_t fp32[nnz] or NULL together with vals; rows of the result are sorted
 * by column; workspace: 4*B*T bytes.  One workgroup per graph (the adjacency is block-diagonal). */
int ggcn_csr_transpose(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T,
                       int32_t *rowptr_t, int32_t *colidx_t, float *vals_t, void *workspace,
                       ggcn_stream_t stream);

/* Per-graph operand blocks of the one-launch layer / block for graphs of <= 32 nodes, from the row masks
 * (one word per node): GGCN_GRAPH_OPS_BYTES per graph = the 0/1 adjacency laid out as the A operand of the
 * aggregation MFMA (2 x 1 KiB) + 1/(rowsum(adj)+1) of its 32 rows in accumulator order (models/gcn.py:35).
 * Built once per adjacency (it replaces, per column tile and wavefront, the expansion of the masks, 32 IEEE
 * divisions and 16 cross-lane moves per graph).  graph_ops: ggcn_graph_operands_bytes(B) bytes, 16-byte aligned. */
#define GGCN_GRAPH_OPS_BYTES 2176
/* The block's second layer applies the normalised adjacency twice (bert_amir5.py:626,639 without a non-linearity in between):
 * ggcn_graph_operands2 folds the two into ONE operand per graph, M2 = (D.A)^2 with D = diag(1 / (rowsum(A) + 1)) (gcn.py:35),
 * as the A operand of the aggregation MFMA in the launch's plane type (`plane`: 0 = bf16 pairs for GGCN_PREC_BF16X3, 1 = fp16
 * pairs for GGCN_PREC_F16MX8): hi and lo parts of M2 * 2^10 (the scale keeps the lo part out of fp16's subnormals; the
 * epilogue multiplies by 2^-10), two k-steps each, plus rowsum(D.A) per row (the factor of the `mid` bias):
 * GGCN_GRAPH_OPS2_BYTES per graph.  ggcn_block_fused reads it for its W12 column tiles. */
#define GGCN_GRAPH_OPS2_BYTES 4224
/* Graphs of 129..256 nodes (the eight-wavefront one-launch layer): the neighbour sums walk per-row EDGE LISTS.  ggcn_graph_edge_lists
 * makes them once per adjacency tensor from the row masks -- per graph GGCN_EDGE_LISTS_BYTES = the kernel's LDS image: per row up to
 * 16 source rows as byte offsets into its fp32 tile, the degree, 1/(rowsum+1) (models/gcn.py:35), a zero row -- and
 * ggcn_layer_fused takes the blocks in its graph_ops argument (NULL: every (graph, 256 columns) workgroup builds its lists itself,
 * as before; rows with more than 16 neighbours walk their mask words either way, so the row masks stay required). */
#define GGCN_EDGE_LISTS_BYTES 11264
size_t ggcn_graph_edge_lists_bytes(int B);
int ggcn_graph_edge_lists(const uint32_t *rowmask, int B, int T, void *lists, ggcn_stream_t stream);
size_t ggcn_graph_operands_bytes(int B);
int ggcn_graph_operands(const uint32_t *rowmask, int B, int T, void *graph_ops, ggcn_stream_t stream);
size_t ggcn_graph_operands2_bytes(int B);
int ggcn_graph_operands2(const uint32_t *rowmask, int B, int T, int plane, void *graph_ops2, ggcn_stream_t stream);

/* Row masks from an existing batched CSR (T <= GGCN_MASK_MAX_T). */
int ggcn_csr_rowmask(const int32_t *rowptr, const int32_t *colidx, int B, int T,
                     uint32_t *rowmask, ggcn_stream_t stream);

/* ---- dense linear ----------------------------------------------------------
 * Replaces models/gcn.py:34: Y[M,F] = X[M,K] . W[K,F]  (W is in x out, gcn.py:18).
 * GGCN_PREC_BF16X3 and GGCN_PREC_F16MX8 need `wpack`, the split image of W in MFMA
 * fragment order, made once per weight update by ggcn_weight_pack for THAT precision
 * (ggcn_weight_pack_bytes(K,F,precision) bytes; the two images differ); GGCN_PREC_FP32
 * reads W itself and ignores wpack.  transposed != 0 packs W^T instead: W is then
 * [F,K] row-major with ldw >= K, the image is that of the [K,F] matrix W^T (the dX
 * linear of the backward pass, train.py:120, uses it with the forward's weight). */
size_t ggcn_weight_pack_bytes(int K, int F, int precision);
int ggcn_weight_pack(const float *W, int64_t ldw, int K, int F, int precision, int transposed,
                     void *wpack, ggcn_stream_t stream);
int ggcn_linear(const float *X, int64_t ldx, const float *W, int64_t ldw, const void *wpack,
                float *Y, int64_t ldy, int64_t M, int K, int F, int precision,
                ggcn_stream_t stream);

/* ---- gated aggregation: one wavefront per destination node ----------------
 * Replaces models/gcn.py:35-45 and models/bert_amir5.py:627-640 in one pass:
 *   y[i,:]      = ( sum_e vals[e] * Hd[colidx[e],:] ) / ( sum_e vals[e] + 1 ) + bias
 *   out[i,:]    = y[i,:] * store_gate[g(i),:]           (store_gate NULL => 1)
 *   pool_a[g,:] = max over the T rows of graph g of y * pool_gate_a[g,:]
 *   pool_b[g,:] = likewise with pool_gate_b
 * Hd [N,F] is the linear's output; gates and pools are [B,F] contiguous.
 * out may be NULL (pooled outputs only); pool_x NULL disables that pool
 * (pool_gate_x NULL with pool_x set => gate of ones); bias may be NULL.
 * N = B*T.  Layer 1 of the block (bert_amir5.py:626-636): store_gate NULL,
 * pools (gate1,x1) and (gate2,y1).  Layer 2 (:639-640): store_gate = gate2,
 * pool (gate2,out). */
int ggcn_aggregate(const float *Hd, int64_t ldh,
                   const int32_t *rowptr, const int32_t *colidx, const float *vals,
                   const float *bias, int B, int T, int F,
                   const float *store_gate, const float *pool_gate_a, const float *pool_gate_b,
                   float *out, int64_t ldo, float *pool_a, float *pool_b,
                   ggcn_stream_t stream);

/* ---- backward pass of the layer (train.py:115-121 trains through gc1/gc2) ----------------
 * For Y = D.A.(X.W) + b with D = diag(1/(rowsum(A)+1)) and an upstream gradient dY [N,F]:
 *   dH = A^T.(D.dY)   ggcn_aggregate_t on the TRANSPOSED adjacency (CSR of adj^T: rows = source
 *                     nodes), src_scale = the 1/(rowsum+1) of the ORIGINAL rows from
 *                     ggcn_inv_denominators;  out[j] = sum_e vals_t[e]*src_scale[colidx_t[e]]*G[colidx_t[e]]
 *   dX = dH.W^T       ggcn_linear with the image made by ggcn_weight_pack(transposed = 1)
 *                     (packs the transpose of the stored matrix: the packed operand has
 *                     K = F_layer rows and F = K_layer columns)
 *   dW = X^T.dH       ggcn_dweight, split over the node rows, deterministic (fixed-order slab sum):
 *                     GGCN_PREC_FP32  exact fp32 MFMA on the rows as they lie (16-byte row loads when
 *                     aligned, element loads otherwise);
 *                     GGCN_PREC_BF16X3  X is transposed and dH packed once, then the forward's
 *                     bf16x3 main loop runs split-K (about 3x faster at config 2; needs
 *                     ~2 x 4*N*max(K,F) bytes of workspace).  f16mx8 is refused: gradients need
 *                     the fp32 exponent range.  (workspace: ggcn_dweight_workspace_bytes(N, K, F,
 *                     precision) bytes, 16-byte aligned)
 *   db = sum_rows dY  ggcn_gate_pool_backward's d_bsum (per graph) + ggcn_colsum over the graphs. */
/* Backward of the gate / max-pool epilogue (models/bert_amir5.py:627-640): from the stored
 * layer output `out` (= y*store_gate), the gates and the upstream gradients of out and of the
 * two pooled outputs, produce dY (gradient of the ungated layer output y) and the gate gradients:
 *   dY[t] = d_out[t]*sg + [t=argmax_a] d_pa*ga + [t=argmax_b] d_pb*gb
 *   d_sg = sum_t d_out*y,  d_ga = d_pa*y[argmax_a],  d_gb = d_pb*y[argmax_b]
 * Any of store_gate, gate_a/d_pa, gate_b/d_pb, d_out, d_sg, d_ga, d_gb may be NULL. */
int ggcn_gate_pool_backward(const float *out, int64_t ldo,
                            const float *store_gate, const float *gate_a, const float *gate_b,
                            const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb,
                            int B, int T, int F, float *dY, int64_t ldy,
                            float *d_sg, float *d_ga, float *d_gb, float *d_bsum, ggcn_stream_t stream);
/* The same with the gates' dropout keep factors of ggcn_layer_fused_drop (same p, seed and streams as the forward launch):
 * sg, ga, gb become sg*k_store[t], ga*k_a[t], gb*k_b[t].  A token whose store factor is 0 (out[t] = 0) contributes y = 0:
 * exact when the pool gates in use share the store gate's stream or there is no store gate (the block's two layers). */
int ggcn_gate_pool_backward_drop(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                                 const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa,
                                 const float *d_pb, int B, int T, int F, float *dY, int64_t ldy, float *d_sg,
                                 float *d_ga, float *d_gb, float *d_bsum, float p, uint64_t seed, int stream_store,
                                 int stream_a, int stream_b, ggcn_stream_t stream);
/* ggcn_gate_pool_backward[_drop] followed by ggcn_aggregate_t in ONE launch, for graphs of T <= 32 nodes with a 0/1 adjacency
 * given as row masks (ggcn_rowmask_from_dense / _from_csr: one word per node): writes dH = A^T . D . dY (the gradient of
 * hidden = text . W, models/gcn.py:34,41 under train.py:120) straight away -- dY is consumed by nothing else and never
 * reaches memory.  p = 0: no gate dropout.  Needs F % 4 == 0, leading dimensions % 4 == 0, 16-byte aligned pointers
 * (GGCN_EUNSUPPORTED otherwise: take the two calls).  Same sums in the same order as the two calls. */
int ggcn_gate_pool_backward_agg(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                                const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa,
                                const float *d_pb, const uint32_t *rowmask, int B, int T, int F, float *dH, int64_t ldh,
                                float *d_sg, float *d_ga, float *d_gb, float *d_bsum, float p, uint64_t seed,
                                int stream_store, int stream_a, int stream_b, float *dh_amax, ggcn_stream_t stream);
/* dh_amax (NULL, or one device float the caller zeroed): receives max |dH| of the launch (an atomic maximum of bit patterns:
 * +inf when a gradient is not finite).  ggcn_linear_scaled reads it:
 *   Y[M,F] = X[M,K] . W   on the two-unit f16mx8 product (GGCN_PREC_F16MX8 image of W) for rows of ANY magnitude: every
 *   workgroup derives the same power of two s from *amax (|x| * s < 256), multiplies x by s before the split and the result by
 *   1 / s -- both exact -- so gradients far below fp16's range keep the product's ~2^-16 accuracy relative to the largest
 *   entry (values below amax * 2^-32 flush: they cannot matter to a sum the largest entries dominate).  This is the backward's
 *   dX = dH . W^T (train.py:120 through models/gcn.py:34) at 325-335 us instead of the three-product form's 420 at config 2.
 *   Needs K % 32 == 0, F % 4 == 0 and 16-byte aligned rows (GGCN_EUNSUPPORTED otherwise: ggcn_linear with GGCN_PREC_BF16X3).
 *   A non-finite amax leaves the data unscaled (the result is non-finite either way). */
int ggcn_linear_scaled(const float *X, int64_t ldx, const void *wpack, float *Y, int64_t ldy, int64_t M, int K, int F,
                       const float *amax, ggcn_stream_t stream);
/* The same two steps on the matrix cores (no gate dropout): dH_g = A_g^T . (D.dY_g) as one MFMA chain per (graph, 32 columns)
 * -- D.dY split into three bf16 planes (2^-25 of its scale), A^T an exact 0/1 operand -- instead of 1024 scalar bit tests per
 * thread.  graph_ops: the graph's ggcn_graph_operands blocks (their 1/(rowsum+1) table); graph_ops_t: ggcn_graph_operands blocks of
 * the TRANSPOSED row masks (ggcn_rowmask_transpose: bit t of word s = bit s of word t; once per adjacency tensor).  Same results as
 * ggcn_gate_pool_backward_agg up to the order of additions (gate gradients and bias sums: two partial sums per column instead of one
 * sequential sum; arg-max ties go to the smaller row in both).  Needs F % 4 == 0, ldh % 4 == 0, 16-byte aligned dH. */
int ggcn_rowmask_transpose(const uint32_t *rowmask, int B, int T, uint32_t *rowmask_t, ggcn_stream_t stream);
int ggcn_gate_pool_backward_mma(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                                const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb,
                                const void *graph_ops, const void *graph_ops_t, int B, int T, int F, float *dH, int64_t ldh,
                                float *d_sg, float *d_ga, float *d_gb, float *d_bsum, float *dh_amax, ggcn_stream_t stream);
/* d_bsum (NULL or [B,F]) receives sum_t dY per graph; db = sum_rows dY is then ggcn_colsum over its B rows.
 * ggcn_colsum: out[f] = sum_r X[r,f] for X [M, ld], deterministic (fixed-order slab sums);
 * workspace: ggcn_colsum_workspace_bytes(F) bytes. */
size_t ggcn_colsum_workspace_bytes(int F);
int ggcn_colsum(const float *X, int64_t ld, int64_t M, int F, float *out, void *workspace, ggcn_stream_t stream);
size_t ggcn_dweight_workspace_bytes(int64_t n_rows, int K, int F, int precision);
int ggcn_dweight(const float *X, int64_t ldx, const float *dH, int64_t ldg, int64_t n_rows, int K, int F,
                 float *dW, int64_t lddw, int precision, void *workspace, ggcn_stream_t stream);
int ggcn_inv_denominators(const int32_t *rowptr, const float *vals, int64_t n_rows, float *inv,
                          ggcn_stream_t stream);
int ggcn_aggregate_t(const float *G, int64_t ldg,
                     const int32_t *rowptr_t, const int32_t *colidx_t, const float *vals_t,
                     const float *src_scale, int B, int T, int F,
                     float *out, int64_t ldo, ggcn_stream_t stream);
/* Gradient with respect to a REAL-VALUED adjacency (models/gcn.py:33-45 is differentiable in `adj`: a soft or learned graph).
 * Per graph, with H = X.W the layer's `hidden`, inv_i = 1/(sum_k A_ik + 1) (ggcn_inv_denominators) and dY the gradient at the
 * plain layer output y = D.A.H + b (what ggcn_gate_pool_backward[_drop] writes):
 *   G_ij  = inv_i * (dY_i . H_j)          reduction over F
 *   c_i   = inv_i * sum_k A_ik * G_ik     over the row's non-zeros (rowptr / colidx with global node ids / vals, NULL = 0/1)
 *   dA_ij = G_ij - c_i                    for EVERY (i, j): the gradient is dense, zero entries and padding rows included
 * d_adj is [B,T,T] contiguous.  One launch: float32 operands split into bf16 hi / lo in the kernel, three bf16 MFMAs per product
 * with fp32 accumulation (the fp32 exponent range: gradients have no range contract), no atomics, a fixed summation order --
 * results are bit-identical from run to run.  Any T in 1..GGCN_LONG_MAX_T (beyond: GGCN_EUNSUPPORTED), any F >= 1, ldy, ldh >= F;
 * rows that are not 16-byte aligned take element loads.  NULL pointers (vals excepted), ldy or ldh < F, pointers off 4 bytes and
 * negative sizes return GGCN_EINVAL with a message that names the argument, before any launch; B = 0 succeeds without one. */
int ggcn_adjacency_grad(const float *dY, int64_t ldy, const float *hidden, int64_t ldh,
                        const float *inv,
                        const int32_t *rowptr, const int32_t *colidx, const float *vals,
                        int B, int T, int F, float *d_adj, ggcn_stream_t stream);
/* ggcn_gate_pool_backward_mma for a REAL-valued adjacency (a soft or learned graph), graphs of <= 32 nodes, no gate dropout:
 * gate / pool backward and dH = A_w^T . D . dY in ONE launch on the matrix cores -- no transposed CSR, no ggcn_aggregate_t, and
 * dY in memory only when asked for.
 * ggcn_graph_operands_weighted_t turns the batched CSR with its weights (vals; NULL = all ones) into one block of
 * GGCN_GRAPH_OPSWT_BYTES per graph holding N = A_w^T (N[s][t] = A_w[t][s]; row s is the SOURCE node) and nothing else:
 * 1 / (rowsum + 1) stays with dY, as in the 0/1 kernel.  N is stored as three bf16 planes p0 + p1 + p2 (p0 = bf16(N),
 * p1 = bf16(N - p0), p2 = bf16(N - p0 - p1): the residual is at most 2^-24 of the entry); plane p, k-step s lies at byte
 * (2 p + s) * 1024 as 64 lanes x 16 bytes in the A-operand order of v_mfma_f32_32x32x16_bf16, the order of
 * GGCN_GRAPH_OPSW_BLOCK_BYTES blocks (lane l: row l & 31, h = l >> 5; element j of k-step s = column 16 s + 8 (j >> 2) + 4 h +
 * (j & 3)), which is the consuming kernel's register -> row map.  Rows and columns >= T are zero.  Entries of one (t, s) add up.
 * Size: ggcn_graph_operands_weighted_t_bytes(B) = B * 6144 (0 for B <= 0); 16-byte aligned.  *flag (optional, device memory,
 * zeroed by the caller) gets bit 0 when an entry of A_w is not finite -- such an adjacency keeps the two calls.
 * Refusals, before any launch: T > 32 -> GGCN_EUNSUPPORTED; null rowptr / colidx / graph_ops_wt, T < 1, B < 0, blocks off
 * 16 bytes -> GGCN_EINVAL; B = 0 succeeds without a launch.
 * ggcn_gate_pool_backward_weighted: arguments as ggcn_gate_pool_backward_mma, with
 *   graph_ops_wt  the blocks above;   inv  float[B*T] = 1 / (rowsum(A_w) + 1) (ggcn_inv_denominators);
 *   dY            NULL, or [B*T, ldy]: receives the UNSCALED dY (what ggcn_gate_pool_backward writes), for ggcn_adjacency_grad.
 * D.dY is split into three bf16 planes as in the 0/1 kernel and multiplied by the three planes of N; the six products of weight
 * >= 2^-16 of the leading one are kept (n0.y0, n0.y1, n0.y2, n1.y0, n1.y1, n2.y0) and summed smallest first: 12 MFMAs per
 * 32-column tile, dH within a few fp32 ulps of its scale.  The gate gradients and bias sums are the 0/1 kernel's (the same
 * winners: ties go to the smaller row; two partial sums per column).  No atomics, a fixed summation order: bit-identical from run
 * to run.  No max |dH| (dX takes ggcn_linear).
 * Needs T <= 32 (GGCN_EUNSUPPORTED: ggcn_gate_pool_backward + ggcn_aggregate_t), F % 4 == 0, ldo, ldd, ldh, ldy % 4 == 0 and
 * 16-byte aligned dH / dY / blocks (GGCN_EUNSUPPORTED); null out / dH / inv / graph_ops_wt, a leading dimension below F, T or
 * F < 1 -> GGCN_EINVAL; every check comes before the launch, and B = 0 succeeds without one. */
#define GGCN_GRAPH_OPSWT_BYTES 6144
size_t ggcn_graph_operands_weighted_t_bytes(int B);
int ggcn_graph_operands_weighted_t(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T,
                                   void *graph_ops_wt, int32_t *flag, ggcn_stream_t stream);
int ggcn_gate_pool_backward_weighted(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                                     const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb,
                                     const void *graph_ops_wt, const float *inv, int B, int T, int F, float *dH, int64_t ldh,
                                     float *dY, int64_t ldy, float *d_sg, float *d_ga, float *d_gb, float *d_bsum,
                                     ggcn_stream_t stream);

/* ggcn_gate_pool_backward_mma for 0/1 graphs of 33..128 nodes, without gate dropout: gate / pool backward and dH = A^T . D . dY in
 * ONE launch on the matrix cores -- no dY in memory, no transposed CSR, no ggcn_aggregate_t.
 * ggcn_rowmask_transpose_wide: the row masks of the transposed adjacency in the layout of `rowmask` (uint32 [B*T][W],
 * W = ceil(T/32)): bit t % 32 of word t / 32 of row s of rowmask_t = bit s % 32 of word s / 32 of row t of rowmask; bits and words at
 * or beyond T are 0.  Once per adjacency tensor.  32 < T <= 128 (T <= 32: ggcn_rowmask_transpose), else GGCN_EUNSUPPORTED.
 * ggcn_gate_pool_backward_wide: arguments as ggcn_gate_pool_backward_weighted, with
 *   rowmask_t  the masks above (16-byte aligned);   inv  float[B*T] = 1 / (rowsum(A) + 1) (ggcn_inv_denominators);
 *   no dY and no max |dH|: an adjacency gradient keeps ggcn_gate_pool_backward + ggcn_aggregate_t, and so does gate dropout
 *   (ggcn_gate_pool_backward_drop): this launch has no form under it.
 * One workgroup per graph; per 32 columns the winners of both pools are found over all ceil(T/32) row blocks, then D.dY of every
 * source block is split into three bf16 planes (2^-25 of its scale) and multiplied by the 0/1 blocks of A^T that have an edge
 * (6 MFMAs per block, planes smallest first, source blocks in ascending order).  The gate gradients and bias sums are the 32-node
 * kernel's (ties go to the smaller row; two partial sums per column).  No atomics, a fixed summation order: bit-identical from run
 * to run; dH differs from the two calls' in the last bits.
 * Needs 32 < T <= 128, F % 4 == 0, ldh % 4 == 0, 16-byte aligned dH / rowmask_t, a graph's rows (in whole 32-row blocks) below
 * 2 GiB (GGCN_EUNSUPPORTED); null out / dH / rowmask_t / inv, B, T or F < 1, a leading dimension below F -> GGCN_EINVAL; every
 * check comes before the launch. */
int ggcn_rowmask_transpose_wide(const uint32_t *rowmask, int B, int T, uint32_t *rowmask_t, ggcn_stream_t stream);
int ggcn_gate_pool_backward_wide(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                                 const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb,
                                 const uint32_t *rowmask_t, const float *inv, int B, int T, int F, float *dH, int64_t ldh,
                                 float *d_sg, float *d_ga, float *d_gb, float *d_bsum, ggcn_stream_t stream);

/* ggcn_gate_pool_backward_weighted for a REAL-valued adjacency of graphs of 33..128 nodes, without gate dropout: gate / pool
 * backward and dH = A_w^T . D . dY in ONE launch on the matrix cores -- no transposed CSR, no ggcn_aggregate_t.
 * ggcn_graph_operands_weighted_wide_t: N = A_w^T (N[s][t] = A_w[t][s]) per graph as W x W blocks of 32 x 32, W = ceil(T/32), each
 * THREE bf16 planes p0 + p1 + p2 (p0 = RNE bf16 of the entry, p1 of the rest, p2 of what is left: 2^-25 of the entry) of two
 * k-steps of 64 lanes x 16 bytes in A-operand order (lane l = row l % 32 of the block, element j of k-step k = column
 * 16 k + 8 (j >> 2) + 4 (l / 32) + (j & 3)): plane p, k-step k of block (s, t) at ((s W + t) * 6 + 2 p + k) * 1024 bytes of the
 * graph's W^2 * 6144.  Rows and columns >= T are zero; nothing is folded in (1 / (rowsum + 1) stays with dY).  Behind the blocks
 * of all B graphs: one uint32 per graph, bit 4 s + t set when block (s, t) has a non-zero entry.  Built from the batched CSR
 * (entries of one (t, s) add up; ids outside the graph are not followed), once per adjacency tensor.  An entry of -0.0 counts as
 * zero for the summary: a block that holds nothing else is skipped (its products would be zeros of either sign, or NaN against
 * a D.dY that is not finite).  flag (optional, zeroed by the caller): bit 0 is raised when an entry, or the sum of the entries
 * of one (t, s), is not finite OR its magnitude is not below 3.0e38 -- a finite value that close to FLT_MAX would round to an
 * infinite bf16 plane; the caller then keeps the two calls.  ggcn_graph_operands_weighted_wide_t_bytes(B, T) =
 * B * (W^2 * 6144 + 4), or 0 outside 32 < T <= 128.  Null rowptr / colidx / blocks, B or T < 1 -> GGCN_EINVAL; T <= 32
 * (ggcn_graph_operands_weighted_t) or T > 128 -> GGCN_EUNSUPPORTED; the blocks must be 16-byte aligned.
 * ggcn_gate_pool_backward_weighted_wide: arguments exactly as ggcn_gate_pool_backward_weighted, with graph_ops_wwt the blocks
 * above (16-byte aligned) and inv = float[B*T] 1 / (rowsum(A_w) + 1) (ggcn_inv_denominators).  dY (optional): the unscaled dY
 * for ggcn_adjacency_grad; NULL: no dY store, and dH is bit for bit the same.  One workgroup per graph; per 32 columns the
 * winners of both pools are found over all W row blocks, then D.dY of every source block is split into three bf16 planes and
 * multiplied by the non-empty blocks of N: the six plane products of weight >= 2^-16, smallest first (12 MFMAs per block), source
 * blocks in ascending order.  No atomics, a fixed summation order: bit-identical from run to run; dH differs from the two calls'
 * in the last bits.  No form under gate dropout.
 * Needs 32 < T <= 128, F % 4 == 0, ldh % 4 == 0, 16-byte aligned dH / graph_ops_wwt, a graph's rows (in whole 32-row blocks) below
 * 2 GiB (GGCN_EUNSUPPORTED); null out / dH / graph_ops_wwt / inv, B, T or F < 1, a leading dimension below F (ldy where dY is
 * given) -> GGCN_EINVAL; every check comes before the launch. */
size_t ggcn_graph_operands_weighted_wide_t_bytes(int B, int T);
int ggcn_graph_operands_weighted_wide_t(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T,
                                        void *graph_ops_wwt, int32_t *flag, ggcn_stream_t stream);
int ggcn_gate_pool_backward_weighted_wide(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                                          const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb,
                                          const void *graph_ops_wwt, const float *inv, int B, int T, int F, float *dH, int64_t ldh,
                                          float *dY, int64_t ldy, float *d_sg, float *d_ga, float *d_gb, float *d_bsum,
                                          ggcn_stream_t stream);

/* ---- fp16 features (BASELINE configs[3]: 512-token graphs, hidden 1024) ------------------
 * Same operations with X / hidden / out stored as IEEE half and fp32 accumulation; weights
 * (wpack), bias, gates and pooled outputs stay fp32.  The reference cannot run half inputs
 * (models/gcn.py:33-34 raise a dtype mismatch); parity is against the fp32 reference
 * on fp16-rounded inputs.  An fp16 value splits exactly into two bf16 terms, so the linear uses
 * the same three-product scheme as GGCN_PREC_BF16X3. */
int ggcn_linear_h(const void *X, int64_t ldx, const void *wpack, void *Y, int64_t ldy,
                  int64_t M, int K, int F, int precision, ggcn_stream_t stream);
int ggcn_aggregate_h(const void *Hd, int64_t ldh,
                     const int32_t *rowptr, const int32_t *colidx, const float *vals,
                     const float *bias, int B, int T, int F,
                     const float *store_gate, const float *pool_gate_a, const float *pool_gate_b,
                     void *out, int64_t ldo, float *pool_a, float *pool_b,
                     ggcn_stream_t stream);

/* The two calls above as ONE launch for long graphs (T <= GGCN_LONG_MAX_T = 512) with fp16 features: models/gcn.py:34-45
 * (+ the gates and pools of models/bert_amir5.py:627-640) without `hidden` leaving the CU.  A workgroup owns a
 * graph and 128 output columns: plain fp16 MFMA (the arithmetic of GGCN_PREC_F16; wpack from
 * ggcn_weight_pack(..., GGCN_PREC_F16)), `hidden` rounded to fp16 into LDS exactly as ggcn_linear_h stores it, then the
 * CSR neighbour sums out of LDS.  Same arguments and results as ggcn_linear_h(GGCN_PREC_F16) + ggcn_aggregate_h
 * (rounding of the fp32 sums differs by summation order only).  Needs K % 64 == 0, F % 8 == 0, 16-byte aligned
 * X / out / bias / gates with ldx, ldo multiples of 8; anything else returns GGCN_EUNSUPPORTED (use the two calls). */
#define GGCN_LONG_MAX_T 512
int ggcn_layer_fused_h(const void *X, int64_t ldx, const void *wpack,
                       const int32_t *rowptr, const int32_t *colidx, const float *vals,
                       const float *bias, int B, int T, int K, int F,
                       const float *store_gate, const float *pool_gate_a, const float *pool_gate_b,
                       void *out, int64_t ldo, float *pool_a, float *pool_b,
                       ggcn_stream_t stream);

/* ---- one whole gated layer in one launch (graphs of <= GGCN_MASK_MAX_T = 256 nodes, binary adjacency) ----
 * Replaces models/gcn.py:34-45 + models/bert_amir5.py:627-640 without materialising
 * `hidden`: the linear's accumulator tile (one graph x 32 features) is multiplied by
 * the graph's 0/1 adjacency with a second MFMA, then divided, biased, gated, pooled and
 * stored.  Same outputs and argument meaning as ggcn_linear(GGCN_PREC_BF16X3) followed by
 * ggcn_aggregate; X is [B*T, K], wpack from ggcn_weight_pack(K, F, precision); T <= 32 reads graph_ops
 * (ggcn_graph_operands; rowmask may be NULL), T > 32 reads rowmask uint32[B*T][ceil(T/32)] (graph_ops may be
 * NULL); precision is GGCN_PREC_BF16X3 or GGCN_PREC_F16MX8.  T <= 32: one 32x32
 * accumulator tile is one graph.  32 < T <= 128: a graph takes a 64- or 128-row slot of a wavefront's tile and
 * its adjacency is applied as ceil(T/32)^2 blocks of 32x32 bits (LitBank: ORI_ML = 100, constant.py:227).
 * 128 < T <= 256 (ACE cased: ORI_ML = 231, constant.py:267): eight wavefronts per graph; the accumulators of a
 * 32-column tile go to an fp32 tile in LDS and the neighbour sums run over per-row edge lists made from the
 * row masks (exact fp32 sums).
 * The gate-diversity regulariser (models/bert_amir5.py:638) can ride along instead of taking
 * ggcn_gate_overlap's two launches: overlap_partial (NULL or float[B * ceil(F/64)]) receives, per graph
 * and 64-column group, sum_f pool_a[g,f]*pool_b[g,f] of THIS launch (layer 1: x1.y1); overlap_in /
 * overlap_out (both or neither) make this launch first reduce the partials an EARLIER launch on the
 * same stream wrote (same B, F) to *overlap_out = mean_b sum_f, in a fixed order (deterministic). */
int ggcn_layer_fused(const float *X, int64_t ldx, const void *wpack,
                     const uint32_t *rowmask, const void *graph_ops,
                     const float *bias, int B, int T, int K, int F,
                     const float *store_gate, const float *pool_gate_a, const float *pool_gate_b,
                     float *out, int64_t ldo, float *pool_a, float *pool_b,
                     float *overlap_partial, const float *overlap_in, float *overlap_out,
                     int precision, ggcn_stream_t stream);

/* The one-launch layer for graphs of 33..256 nodes with a bias added BEFORE the aggregation:
 *   y = D.A.(X.W + 1.bias_pre^T) + bias  =  D.A.X.W + rowsum(D.A).bias_pre + bias
 * -- the second half of the folded two-layer block when its input rows are already aggregated once: with Z = D.A.X
 * (ggcn_aggregate on the features), gc2(gc1(X)) = D.A.(Z.W12 + 1.bias_mid^T) + b2 (models/bert_amir5.py:626,639;
 * W12 = W1.W2, bias_mid = W2^T.b1), so an evaluation that needs only `out` (train.py:227) never multiplies by W1
 * (gated_block.py: the eval form for LitBank / ACE-cased lengths, constant.py:227,267).  Other arguments as in
 * ggcn_layer_fused (row masks required: T > 32; no regulariser partials). */
int ggcn_layer_fused_prebias(const float *X, int64_t ldx, const void *wpack, const uint32_t *rowmask,
                             const float *bias, const float *bias_pre, int B, int T, int K, int F,
                             const float *store_gate, const float *pool_gate_a, const float *pool_gate_b,
                             float *out, int64_t ldo, float *pool_a, float *pool_b, int precision, ggcn_stream_t stream);

/* The one-launch layer for a REAL-valued adjacency (models/gcn.py:33-41 take any `adj`: denom = rowsum(adj) + 1,
 * adj.hidden / denom; the reference's own graphs are 0/1, graph.py:66-74), graphs of <= 32 nodes:
 * ggcn_graph_operands_weighted turns the batched CSR with its weights (vals; NULL = all ones) into one operand block per
 * graph, M = D.A_w * 2^10 as hi / lo parts in the launch's plane type (`plane` as in ggcn_graph_operands2, same size:
 * ggcn_graph_operands2_bytes(B)); *flag (optional, device memory, zeroed by the caller) gets bit 0 when an entry does not
 * fit the plane type (|w / (rowsum + 1)| >= ~58 with fp16 planes, or a non-finite value: mixed-sign weights can do that) --
 * such an adjacency stays with ggcn_linear + ggcn_aggregate.  ggcn_layer_fused_weighted is ggcn_layer_fused on those blocks:
 * one split of `hidden` and 6 MFMAs per tile (hi.hi, hi.lo, lo.hi; the lo.lo term is 2^-22 of the result) where the 0/1
 * form needs 4, sums within 2^-21 of ggcn_aggregate's fp32 sums.  zero_mid: [F] zeros, 16-byte aligned (the kernel's
 * `mid` row, unused here).  Inference only (no gate dropout); other arguments as in ggcn_layer_fused. */
int ggcn_graph_operands_weighted(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, int plane,
                                 void *graph_opsw, int32_t *flag, ggcn_stream_t stream);
int ggcn_layer_fused_weighted(const float *X, int64_t ldx, const void *wpack, const void *graph_opsw, const float *bias,
                              const float *zero_mid, int B, int T, int K, int F, const float *store_gate,
                              const float *pool_gate_a, const float *pool_gate_b, float *out, int64_t ldo, float *pool_a,
                              float *pool_b, float *overlap_partial, const float *overlap_in, float *overlap_out, int precision,
                              ggcn_stream_t stream);

/* The same for graphs of 33..128 nodes (LitBank: ORI_ML = 100, constant.py:227 -- a learned or soft adjacency at the lengths
 * the reference trains on), float32 features.
 * ggcn_graph_operands_weighted_wide turns the batched CSR with its weights (vals; NULL = all ones) into W x W blocks per
 * graph, W = ceil(T/32): block (io, ii) -- rows 32 io .. 32 io + 31, columns 32 ii .. 32 ii + 31 of M = D.A_w,
 * D = diag(1 / (rowsum(A_w) + 1)) (gcn.py:35) -- lies at ((g * W + io) * W + ii) * GGCN_GRAPH_OPSW_BLOCK_BYTES and holds
 *     [0, 1024) hi = bf16(M), k-step 0;  [1024, 2048) hi, k-step 1;  [2048, 3072) lo = bf16(M - hi), k-step 0;  [3072, 4096) lo, k-step 1
 * each as 64 lanes x 16 bytes in the A-operand order of v_mfma_f32_32x32x16_bf16 (lane l: row l & 31, h = l >> 5; element j of
 * k-step s = column 16 s + 8 (j >> 2) + 4 h + (j & 3) of the block).  Rows and columns >= T are zero.  The planes are bf16 for
 * both precisions: the 33..128-node kernel holds `hidden` as bf16 planes whatever its main loop is.
 * D IS FOLDED INTO THE OPERAND, without a power-of-two scale: bf16 has fp32's exponent range, so D.A_w needs none (the <= 32
 * form scales by 2^10 for its fp16 planes), the kernel then applies no row factor at all -- the 16 registers and 16 cross-lane
 * moves per block row the 0/1 form spends on 1 / (deg + 1) carry operand fragments instead -- and no second array travels
 * beside the blocks.  A row's weights are summed in CSR order, as ggcn_aggregate and ggcn_inv_denominators sum them: D is the
 * same number on both paths (the products w * (1 / (rowsum + 1)) round once more than ggcn_aggregate's (sum w.h) * inv).
 * Size: ggcn_graph_operands_weighted_wide_bytes(B, T) = B * W * W * 4096 (0 for T outside 33..128 or B <= 0); 16-byte aligned.
 * *flag (optional, device memory, zeroed by the caller) gets bit 0 when an entry is not finite (rowsum + 1 == 0: mixed-sign
 * weights can do that) -- such an adjacency stays with ggcn_linear + ggcn_aggregate.
 * Refusals: T <= 32 -> GGCN_EUNSUPPORTED (ggcn_graph_operands_weighted is the one-block form); T > 128 -> GGCN_EUNSUPPORTED;
 * null rowptr / colidx / blocks, B <= 0 -> GGCN_EINVAL.
 * ggcn_layer_fused_weighted_wide is ggcn_layer_fused on those blocks: per 32 x 32 output tile 3 x W x 2 bf16 MFMAs
 * (Mlo.Hhi, Mhi.Hlo, Mhi.Hhi, small terms first; the lo.lo term is 2^-18 of a term) where the 0/1 form needs 2 x SB x 2, then
 * the 0/1 form's own epilogue (bias, store gate, both pools).  precision GGCN_PREC_BF16X3 or GGCN_PREC_F16MX8; 33 <= T <= 128
 * (else GGCN_EUNSUPPORTED); ldx >= K, ldo >= F, 16-byte aligned weight image and blocks, at least one output (else
 * GGCN_EINVAL).  Inference form (no gate dropout, no regulariser partials); other arguments as in ggcn_layer_fused. */
#define GGCN_GRAPH_OPSW_BLOCK_BYTES 4096
size_t ggcn_graph_operands_weighted_wide_bytes(int B, int T);
int ggcn_graph_operands_weighted_wide(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T,
                                      void *graph_opsww, int32_t *flag, ggcn_stream_t stream);
int ggcn_layer_fused_weighted_wide(const float *X, int64_t ldx, const void *wpack, const void *graph_opsww, const float *bias,
                                   int B, int T, int K, int F, const float *store_gate, const float *pool_gate_a,
                                   const float *pool_gate_b, float *out, int64_t ldo, float *pool_a, float *pool_b, int precision,
                                   ggcn_stream_t stream);

/* ---- gate dropout inside the launches on a REAL-valued adjacency (training a soft or learned graph) ----
 * The three entries above that serve a real-valued adjacency, with the gates' training-mode keep factors of ggcn_layer_fused_drop
 * (models/bert_amir5.py:621-625; csrc/dropout_hash.h: element ((b T + t) F + f) as uint32, streams 0 / 1 / 2 per gate slot):
 *   out = y * store_gate * k_store,   pool_x = max_t (y * pool_gate_x * k_x)        (every element has its own factor: the
 *   pools maximise the gated, kept values themselves, no max / min shortcut)
 * ggcn_layer_fused_weighted_drop: ggcn_layer_fused_weighted's operands (ggcn_graph_operands_weighted blocks, the zero `mid` row,
 *   GGCN_PREC_BF16X3 or GGCN_PREC_F16MX8) without the overlap arguments, graphs of <= 32 nodes; every shape that launch takes.
 * ggcn_layer_fused_weighted_wide_drop: the same on ggcn_graph_operands_weighted_wide blocks, graphs of 33..128 nodes.
 * ggcn_gate_pool_backward_weighted_drop: ggcn_gate_pool_backward_weighted with the forward's keep factors drawn again:
 *   y = k_store != 0 ? out / store_gate / k_store : 0;  the pools' candidates are y*ga*ka and y*gb*kb (ties to the smaller row);
 *   d_sg = sum_t d_out*y*k_store;   dY = d_out*sg*k_store + [t = ia] d_pa*ga*ka + [t = ib] d_pb*gb*kb  -- the dY that is stored
 *   for ggcn_adjacency_grad and multiplied by A_w^T . D.  A dropped store gate zeroes what y is read back from: exact where
 *   every pool in use shares the store gate's stream (ggcn_gate_pool_backward_drop).  No atomics, a fixed summation order:
 *   bit-identical from run to run.
 * p = 0 launches the kernels WITHOUT dropout: results are bit-identical to the three entries above.
 * Refusals, all before any launch: p outside [0, 1) or a stream outside 0..2 -> GGCN_EINVAL; B*T*F >= 2^32 ->
 * GGCN_EUNSUPPORTED (32-bit element index); forward: T > 32 (wide: outside 33..128) or GGCN_PREC_F16MX6 -> GGCN_EUNSUPPORTED,
 * null blocks or null zero row -> GGCN_EINVAL; every other refusal is the entry's without dropout.  float32 features only. */
int ggcn_layer_fused_weighted_drop(const float *X, int64_t ldx, const void *wpack, const void *graph_opsw, const float *bias,
                                   const float *zero_mid, int B, int T, int K, int F, const float *store_gate,
                                   const float *pool_gate_a, const float *pool_gate_b, float *out, int64_t ldo, float *pool_a,
                                   float *pool_b, int precision, float p, uint64_t seed, int stream_store, int stream_a,
                                   int stream_b, ggcn_stream_t stream);
int ggcn_layer_fused_weighted_wide_drop(const float *X, int64_t ldx, const void *wpack, const void *graph_opsww, const float *bias,
                                        int B, int T, int K, int F, const float *store_gate, const float *pool_gate_a,
                                        const float *pool_gate_b, float *out, int64_t ldo, float *pool_a, float *pool_b,
                                        int precision, float p, uint64_t seed, int stream_store, int stream_a, int stream_b,
                                        ggcn_stream_t stream);
int ggcn_gate_pool_backward_weighted_drop(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                                          const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa,
                                          const float *d_pb, const void *graph_ops_wt, const float *inv, int B, int T, int F,
                                          float *dH, int64_t ldh, float *dY, int64_t ldy, float *d_sg, float *d_ga, float *d_gb,
                                          float *d_bsum, float p, uint64_t seed, int stream_store, int stream_a, int stream_b,
                                          ggcn_stream_t stream);

/* ---- the whole gated block in one launch (graphs of <= 32 nodes, binary adjacency, inference) ----
 * Replaces models/bert_amir5.py:626-640 -- gc1, both gates, both max-pools, gc2, its gate and pool -- with
 * ONE launch that reads X once and never writes gcn1 unless asked to.  The reference feeds gc2 with the
 * UNGATED gcn1 and applies no non-linearity between the layers (models/gcn.py:19 declares a Tanh that
 * forward never calls; models/bert_amir5.py:626,639), so with D = diag(1/(rowsum(A)+1)):
 *     gcn1 = D.A.X.W1 + b1
 *     gcn2 = D.A.gcn1.W2 + b2 = D.A.( D.A.(X.W12) + bias_mid ) + b2,   W12 = W1.W2,  bias_mid = W2^T.b1
 * wpack1 / wpack12: ggcn_weight_pack images of W1 [K,F] and W12 [K,F] for `precision`; the caller makes
 * W12 and bias_mid once per weight update (ggcn_linear with GGCN_PREC_FP32: an exact fp32 product;
 * bias_mid is a vector of F zeros when gc1 has no bias).  bias1 / bias2 may be NULL.
 * Outputs: x1 = max_t gcn1*gate1, y1 = max_t gcn1*gate2 ([B,F], required), x_out = gate2*gcn2 [N, ld2]
 * (or NULL), pool_out = max_t x ([B,F] or NULL), gcn1 [N, ld1] only when non-NULL (nothing downstream
 * of the block reads it), overlap_partial (NULL or float[B*ceil(F/64)]) as in ggcn_layer_fused -- finish
 * it with ggcn_overlap_reduce.  Same flop count as two ggcn_layer_fused launches; X is read once and the
 * 4.N.F-byte write + read of gcn1 disappears.  Training keeps the two-launch path (autograd needs gcn1).
 * graph_ops: ggcn_graph_operands blocks (layer 1's aggregation); graph_ops2: ggcn_graph_operands2 blocks in the plane type
 * of `precision` (layer 2: both aggregations as one application of (D.A)^2, the `mid` bias times rowsum(D.A)). */
int ggcn_block_fused(const float *X, int64_t ldx, const void *wpack1, const void *wpack12,
                     const void *graph_ops, const void *graph_ops2, const float *bias1, const float *bias_mid, const float *bias2,
                     int B, int T, int K, int F, const float *gate1, const float *gate2,
                     float *gcn1, int64_t ld1, float *x_out, int64_t ld2,
                     float *x1, float *y1, float *pool_out, float *overlap_partial,
                     int precision, ggcn_stream_t stream);
/* ---- the gated block in one launch on a REAL-valued adjacency (graphs of <= 32 nodes, float32 features, inference) ----
 * The fold above holds for any `adj` (gcn.py:33-41): with M = D.A_w, D = diag(1 / (rowsum(A_w) + 1)),
 *     gc2(gc1(X)) = M^2.(X.W12) + rowsum(M).bias_mid^T + 1.b2^T
 * ggcn_graph_operands2_weighted turns the batched CSR with its weights (vals; NULL = all ones) into the blocks of
 * ggcn_graph_operands2 (GGCN_GRAPH_OPS2_BYTES per graph, size ggcn_graph_operands2_bytes(B), 16-byte aligned):
 *     [0, 4096)    M2 = M^2 * 2^10 as hi / lo fragments of the plane type (`plane` 0 = bf16 pairs, 1 = fp16 pairs), two k-steps
 *                  each, in the A-operand order documented at ggcn_graph_operands_weighted_wide; rows and columns >= T are zero
 *     [4096, 4224) rowsum(M) per row in accumulator order (float [h][16], entry r = row (r & 3) + 8 (r >> 2) + 4 h): the factor
 *                  of the `mid` bias; unlike deg / (deg + 1) it is real-valued and may be negative
 * A row's weights are summed in CSR order (as ggcn_aggregate, ggcn_inv_denominators and ggcn_graph_operands_weighted sum them),
 * M[r][j] = w * inv_r in fp32, M2[r][c] = sum_j M[r][j] * M[j][c] in fp32 with j ascending over 0..T-1, rowsum(M)[r] likewise: a
 * fixed order, no atomics, bit-identical from run to run.  One wavefront per graph.
 * *flag (optional, device memory, zeroed by the caller) gets bit 0 when an entry of M2 * 2^10 does not fit the plane type
 * (>= 60000 in fp16 planes, >= 3e38 in bf16 planes) or is not finite -- such an adjacency keeps one weighted launch per layer.
 * Refusals, all before any launch: T > 32 -> GGCN_EUNSUPPORTED; null rowptr / colidx / blocks, B <= 0, T <= 0, blocks not
 * 16-byte aligned, plane outside 0..1 -> GGCN_EINVAL.
 * ggcn_block_fused_weighted is ggcn_block_fused on those operands.  Its argument list is ggcn_block_fused's with graph_opsw
 * (ggcn_graph_operands_weighted blocks: layer 1) and graph_ops2w (the blocks above: layer 2) in place of graph_ops / graph_ops2,
 * and zero_mid after bias2: [F] zeros, 16-byte aligned, the `mid` row of the W1 tiles (as in ggcn_layer_fused_weighted).  Both
 * groups of column tiles end in the same epilogue: one split of `hidden`, 6 MFMAs (hi.hi, hi.lo, lo.hi), times 2^-10 -- the W1
 * tiles on M with the zero row, the W12 tiles on M2 with bias_mid.  Outputs and forms are ggcn_block_fused's: x1, y1, optional
 * gcn1, x_out, pool_out, overlap_partial; x1 = y1 = gcn1 = overlap_partial = NULL is the eval form (W12 tiles only; graph_opsw,
 * wpack1, gate1 and zero_mid may then be NULL).  precision GGCN_PREC_BF16X3 (plane 0 blocks) or GGCN_PREC_F16MX8 (plane 1 blocks,
 * the range flag of ggcn_range_flag as in ggcn_block_fused); GGCN_PREC_F16MX6 and T > 32 -> GGCN_EUNSUPPORTED.  Every other
 * refusal is ggcn_block_fused's, worded with this entry's name.  It never runs the eight-wavefront kernel of ggcn_block_fused. */
int ggcn_graph_operands2_weighted(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, int plane,
                                  void *graph_ops2w, int32_t *flag, ggcn_stream_t stream);
int ggcn_block_fused_weighted(const float *X, int64_t ldx, const void *wpack1, const void *wpack12,
                              const void *graph_opsw, const void *graph_ops2w, const float *bias1, const float *bias_mid,
                              const float *bias2, const float *zero_mid, int B, int T, int K, int F, const float *gate1,
                              const float *gate2, float *gcn1, int64_t ld1, float *x_out, int64_t ld2,
                              float *x1, float *y1, float *pool_out, float *overlap_partial,
                              int precision, ggcn_stream_t stream);

/* ---- training-mode dropout of the gates inside the one-launch layer (graphs of <= 256 nodes) ------------------
 * models/bert_amir5.py:621-625 repeats each gate to [B,T,H] and THEN applies F.dropout: one Bernoulli draw per (token,
 * feature) and gate.  Here the keep factors k[t,f] in {0, 1/(1-p)} come from a counter-based hash of (seed, element)
 * (csrc/dropout_hash.h) evaluated in the layer's epilogue -- nothing of size [B,T,H] is materialised -- and again in
 * the backward pass.  Two independent streams exist per seed (1, 2); a gate slot names the stream that drops it (0 =
 * not dropped).  The block uses stream 1 for gate1 and stream 2 for gate2 in BOTH layers (the reference drops gate2
 * once and uses it at :631 and :639):  layer 1: (store 0, pool a 1, pool b 2);  layer 2: (store 2, pool a 2, pool b 0).
 *   out = y * store_gate * k_store,   pool_x = max_t (y * pool_gate_x * k_x)
 * precision GGCN_PREC_BF16X3 or GGCN_PREC_F16MX8; B*T*F < 2^32; rowmask / graph_ops as in ggcn_layer_fused (T <= 32 reads
 * graph_ops, larger graphs the row masks).  ggcn_dropout_mask writes k (rows x F floats) of one stream: what a test or a
 * host-side oracle multiplies the repeated gate by. */
int ggcn_layer_fused_drop(const float *X, int64_t ldx, const void *wpack, const uint32_t *rowmask, const void *graph_ops,
                          const float *bias, int B, int T, int K, int F,
                          const float *store_gate, const float *pool_gate_a, const float *pool_gate_b,
                          float *out, int64_t ldo, float *pool_a, float *pool_b, int precision,
                          float p, uint64_t seed, int stream_store, int stream_a, int stream_b, ggcn_stream_t stream);
int ggcn_dropout_mask(int64_t rows, int F, float p, uint64_t seed, int stream_id, float *mask, ggcn_stream_t stream);

/* models/bert_amir5.py:638 from the partials a ggcn_block_fused / ggcn_layer_fused launch left:
 * *xy = mean_b sum_f x1*y1, fixed summation order (deterministic), one small launch. */
int ggcn_overlap_reduce(const float *partials, int B, int F, float *xy, ggcn_stream_t stream);

/* ---- dense head on the block's pooled output (+ the regulariser's final sum) in one launch -----------
 * Replaces the share of models/bert_amir5.py:643 `logits = self.dense(cat[.., out])` that reads the block's output -- and,
 * when asked, models/bert_amir5.py:638's final sum, which otherwise is ggcn_overlap_reduce's own launch:
 *   logits[b,c] = (bias ? bias[c] : 0) + sum_k pooled[b,k] * Wt[k,c]      pooled [B, ldp], Wt [H, ldw] (nn.Linear's weight
 *   slice, transposed: ggcn_transpose), C <= 64, logits [B, ldl]; plain fp32 FMA chains in a fixed order per row, so a row's
 *   logits do not depend on the batch (or shard) it sits in -- what every rank all-gathers per step when the batch is sharded;
 *   overlap_partials / xy (both or neither): the float[B * ceil(F_block/64)] partials of a ggcn_block_fused /
 *   ggcn_layer_fused launch with B graphs and F_block columns -> *xy = mean_b sum (fixed order; equal to
 *   ggcn_overlap_reduce's result up to the order of additions). */
int ggcn_dense_head(const float *pooled, int64_t ldp, const float *Wt, int64_t ldw, const float *bias, int B, int H, int C,
                    float *logits, int64_t ldl, const float *overlap_partials, int F_block, float *xy, ggcn_stream_t stream);

/* The same launch, counting itself done in memory: signal = two zero-initialised uint32 words in device memory; signal[1]
 * becomes n once the n-th launch on these words has written (and fenced, system scope) all of its logits and xy -- another stream
 * gated by hipStreamWaitValue32(signal + 1, >= n) may then read them, with no event record on the launching stream (the sharded
 * step hands its logits to the collective's stream this way: ed-gated-gcn_amd/shard.py, bench.py --gather-mode flag).
 * signal[0] is the launch's own arrival counter (zero between launches).  One launch at a time per pair of words. */
int ggcn_dense_head_signal(const float *pooled, int64_t ldp, const float *Wt, int64_t ldw, const float *bias, int B, int H, int C,
                           float *logits, int64_t ldl, const float *overlap_partials, int F_block, float *xy, uint32_t *signal,
                           ggcn_stream_t stream);

/* ---- gate-diversity regulariser --------------------------------------------
 * Replaces models/bert_amir5.py:638: *xy = mean_b sum_f x1[b,f]*y1[b,f].
 * x1,y1 [B,F] contiguous, xy one device float.  Deterministic (fixed-order
 * tree reduction).  workspace: ggcn_overlap_workspace_bytes(B) bytes. */
size_t ggcn_overlap_workspace_bytes(int B);
int ggcn_gate_overlap(const float *x1, const float *y1, int B, int F, float *xy,
                      void *workspace, ggcn_stream_t stream);

/* ---- the gate MLPs in one launch ------------------------------------------
 * Replaces models/bert_amir5.py:562-571,621-622: gate_k = Sigmoid(Linear2(Sigmoid(Linear1(Sigmoid(aspect))))) for
 * both gates at once; aspect [B,H] (lda in elements) -> gate_a, gate_b [B,H] contiguous (the reference's
 * .repeat(1,T).view() to [B,T,H] is never made: the layer kernels take [B,H] gates).  w*t are the nn.Linear
 * weights TRANSPOSED to [in,out] contiguous (ggcn_transpose, once per weight update); biases [H] or NULL.
 * The second gate (w1t_b .. gate_b) may be all NULL.  Plain fp32 FMA chains. */
int ggcn_transpose(const float *W, int rows, int cols, int64_t ldw, float *Wt, ggcn_stream_t stream);
int ggcn_gate_mlp(const float *aspect, int64_t lda, int B, int H,
                  const float *w1t_a, const float *b1_a, const float *w2t_a, const float *b2_a, float *gate_a,
                  const float *w1t_b, const float *b1_b, const float *w2t_b, const float *b2_b, float *gate_b,
                  ggcn_stream_t stream);

/* ---- the gate MLPs under autograd: saving forward, backward in one launch (training through models/bert_amir5.py:562-571) ----
 * ggcn_gate_mlp_save: ggcn_gate_mlp's launch and arguments, plus hid_a, hid_b [B,H] contiguous, which receive the hidden
 * activations h = Sigmoid(Linear1(Sigmoid(aspect))).  The gates are the bits ggcn_gate_mlp writes.  The refusals are
 * ggcn_gate_mlp's, plus a NULL hid_a (hid_b goes with the second gate: both NULL or neither).
 *
 * ggcn_gate_mlp_backward: per gate, with s = Sigmoid(aspect), the saved hid = h and gate = g, and d_gate = dG [B,H]:
 *     dz2 = dG * g(1-g)     dh = dz2.W2     dz1 = dh * h(1-h)     ds = dz1.W1
 *     d_aspect = (ds_A + ds_B) * s(1-s)     [B, ldda]; gate A first, then gate B; NULL: the W1 pass is skipped
 * w1_*, w2_* are the nn.Linear weights AS THEY LIE, [out][in] = [H,H] contiguous (no transposed copy); hid_*, gate_*, d_gate_*
 * are [B,H] contiguous.  g(1-g) and h(1-h) are taken from the stored float32 values.  A NULL d_gate_* means that gate
 * contributes nothing to d_aspect (its other pointers are not read); both NULL is refused.  w1_* is read only with d_aspect.
 * Z [B, ldz] (NULL: no weight or bias trains) receives what the weight products read, five column groups that each start at a
 * multiple of Hp = (H + 3) & ~3:   dz1_A | dz1_B | dz2_A | dz2_B | s   (ldz >= 5 Hp; the Hp - H columns behind each group are
 * written as zeros, the groups of a gate with a NULL d_gate as zeros).  From it, with the library's fixed-order products:
 *     dW1_A over dW1_B [2H,H] = ggcn_dweight(X = Z, K = 2 Hp, dH = Z + 4 Hp, F = H)    (Hp == H; else one call per gate, K = H)
 *     dW2_g [H,H]  = ggcn_dweight(X = Z + (2 + g) Hp, K = H, dH = hid_g, F = H)         both already in nn.Linear layout
 *     db1_A | db1_B | db2_A | db2_B = ggcn_colsum(Z, ldz, B, 4 Hp), each at its group's offset
 * One workgroup of 256 threads per 8 sentences, two 8 x H LDS buffers; exact fp32 FMA chains in a fixed order, no atomics: two
 * calls on the same inputs give the same bits.  No synchronisation.  GGCN_EUNSUPPORTED when 16 H floats exceed 64 KiB of
 * LDS (H > 1024), as ggcn_gate_mlp. */
int ggcn_gate_mlp_save(const float *aspect, int64_t lda, int B, int H,
                       const float *w1t_a, const float *b1_a, const float *w2t_a, const float *b2_a, float *gate_a,
                       const float *w1t_b, const float *b1_b, const float *w2t_b, const float *b2_b, float *gate_b,
                       float *hid_a, float *hid_b, ggcn_stream_t stream);
int ggcn_gate_mlp_backward(const float *aspect, int64_t lda, int B, int H,
                           const float *w1_a, const float *w2_a, const float *hid_a, const float *gate_a, const float *d_gate_a,
                           const float *w1_b, const float *w2_b, const float *hid_b, const float *gate_b, const float *d_gate_b,
                           float *d_aspect, int64_t ldda, float *Z, int64_t ldz, ggcn_stream_t stream);

/* ---- scores / kl head in one launch ----------------------------------------
 * Replaces models/bert_amir5.py:645-648:
 *     output_w = fc(cat[x, aspect repeated over t])       [B,T,C], fc.weight [C, 2H], fc.bias [C]
 *     scores   = sum_c logits[b,c] * output_w[b,t,c]      [B,T]
 *     kl       = mean_b sum_t softmax_t(scores) * softmax_t(dist)
 * without the [B,T,2H] concat or the [B,T,C] product: scores[b,t] = (Wx^T.logits_b).x_t + logits_b.(Wa.a_b + b).
 * X [B*T, ldx] is the block's gated layer-2 output; dist [B, ldd] float (the reference's dist_to_target.float());
 * kl_part [B] receives sum_t ... per sentence -- ggcn_overlap_reduce(kl_part, B, 1, kl) finishes the mean.
 * dist and kl_part may both be NULL (scores only). */
int ggcn_scores_head(const float *X, int64_t ldx, const float *aspect, int64_t lda,
                     const float *logits, int64_t ldl, const float *fc_weight, int64_t ldw, const float *fc_bias,
                     const float *dist, int64_t ldd, int B, int T, int H, int C,
                     float *scores, int64_t ld_scores, float *kl_part, ggcn_stream_t stream);

/* ---- backward of the scores / kl head in one launch (training through models/bert_amir5.py:645-648) ------------------
 * Inputs as ggcn_scores_head's, plus what its forward left: scores [B, ld_scores] and kl_part [B]; g_scores [B, ld_gs] is the
 * gradient of scores, g_kl ONE DEVICE float, the gradient of kl (read on the device: no host read-back).  Either may be
 * NULL (that term is zero); dist, scores and kl_part are read only with g_kl.  With v = Wx^T.logits_b, u = Wa.a_b + fc_bias:
 *     ds[b,t] = g_scores[b,t] + (g_kl / B) p_t (q_t - kl_part[b])      p = softmax_t(scores_b), q = softmax_t(dist_b)
 *     dX[b,t,:] = ds[b,t] v          [B*T, lddx]; NULL: not stored (x needs no gradient)
 *     dc0[b]    = sum_t g_scores[b,t]           (= sum_t ds[b,t]: the kl term's share is identically zero and is left out)
 *     d_logits[b] = Wx.dv_b + dc0[b] u          [B, lddl], dv_b = sum_t ds[b,t] x[b,t,:]
 *     d_aspect[b] = dc0[b] (Wa^T.logits_b)      [B, ldda]
 *     G[b] = [dv_b | dc0[b] a_b]                [B, ldg], ldg >= 2H: ggcn_scores_head_dweight's operand
 * d_aspect, d_logits and the pair (G, dc0) may be NULL.  One workgroup per sentence; X is read once and dX written once, in
 * 16-byte accesses when H % 4 == 0 and X / dX rows are 16-byte aligned, element by element otherwise.  Exact fp32 FMA chains,
 * every sum in a fixed order, no atomics: two calls on the same inputs give the same bits.  No synchronisation.
 * GGCN_EUNSUPPORTED when 6 H + C + T floats exceed 64 KiB of LDS.
 *
 * ggcn_scores_head_dweight: dW [C, lddw] = logits^T . G (the gradient of fc.weight [C, 2H]) and d_bias [C] = logits^T . dc0
 * (NULL: fc has no bias), summed over the sentences in a fixed order (slices of 128 sentences, then the slices ascending; two
 * launches).  workspace: ggcn_scores_head_dweight_workspace_bytes(B, H, C) bytes. */
int ggcn_scores_head_backward(const float *X, int64_t ldx, const float *aspect, int64_t lda,
                              const float *logits, int64_t ldl, const float *fc_weight, int64_t ldw, const float *fc_bias,
                              const float *dist, int64_t ldd, const float *scores, int64_t ld_scores, const float *kl_part,
                              const float *g_scores, int64_t ld_gs, const float *g_kl, int B, int T, int H, int C,
                              float *dX, int64_t lddx, float *d_aspect, int64_t ldda, float *d_logits, int64_t lddl,
                              float *G, int64_t ldg, float *dc0, ggcn_stream_t stream);
size_t ggcn_scores_head_dweight_workspace_bytes(int B, int H, int C);
int ggcn_scores_head_dweight(const float *logits, int64_t ldl, const float *G, int64_t ldg, const float *dc0,
                             int B, int H, int C, float *dW, int64_t lddw, float *d_bias, void *workspace,
                             ggcn_stream_t stream);

/* ---- the BiLSTM's recurrence in one launch (inference; models/bert_amir5.py:557,610) ----------------------------------
 * PyTorch's LSTM, gate order i, f, g, o, with h0 = c0 = 0, one layer, both directions.  G [B*T, ldg] is the input projection
 * X . [W_ih_f ; W_ih_r]^T (ggcn_linear: columns 0..4hd-1 belong to the forward direction, 4hd..8hd-1 to the reverse one).  For
 * direction d in {f, r} and sentence b, t running 0..T-1 for f and T-1..0 for r:
 *     a = G[b*T+t, d*4hd:(d+1)*4hd] + bias_d + h . Whh_d^T
 *     i, f, o = sigmoid(a[0:hd]), sigmoid(a[hd:2hd]), sigmoid(a[3hd:4hd])        g = tanh(a[2hd:3hd])
 *     c = f*c + i*g        h = o * tanh(c)        Y[b*T+t, d*hd:(d+1)*hd] = h
 * Whh_d is [4hd, hd] row-major as weight_hh_l0[_reverse] lies; bias_d [4hd] = b_ih + b_hh, NULL = zeros.  All T rows of every
 * sentence are run (a padded batch, no lengths).  One launch for all T steps and both directions: a workgroup of 512 threads
 * takes GGCN_BILSTM_TILE sentences of one direction, Whh_d stays in its registers, h and c never leave the chip.  Exact fp32
 * FMA chains in a fixed order, no atomics: two calls give the same bits, a sentence's result does not depend on B or on its
 * place in a tile, and the two directions run the same arithmetic.  sigmoid and tanh saturate to 0 / 1 / +-1 without a NaN for
 * every finite a.  No synchronisation.
 * Refusals, all before any launch: NULL G / Whh_f / Whh_r / Y, B or T <= 0, ldg < 8 hd, ldy < 2 hd, Whh_f or Whh_r off 16
 * bytes -> GGCN_EINVAL; hd != 128 (the reference's hidden_dim) and B*T >= 2^31 -> GGCN_EUNSUPPORTED. */
#define GGCN_BILSTM_TILE 16
int ggcn_bilstm_recurrence(const float *G, int64_t ldg, const float *Whh_f, const float *Whh_r,
                           const float *bias_f, const float *bias_r, float *Y, int64_t ldy, int B, int T, int hd,
                           ggcn_stream_t stream);

/* ---- the BiLSTM's recurrence under autograd: saving forward, backward in one launch (training through bert_amir5.py:610) ----
 * ggcn_bilstm_recurrence_save: ggcn_bilstm_recurrence's launch and arguments plus three outputs.  gates [B*T, ldg] receives the
 * activated i, f, g, o of every step and direction in the column layout of G; gates == G is allowed (each thread overwrites the
 * one element it has read: one [B*T, 8hd] buffer serves both).  C [B*T, 2hd] contiguous receives the cell state after each step,
 * Hprev [B*T, 2hd] contiguous the h each step read (zeros at a direction's first step: t = 0 forward, t = T-1 reverse), both in
 * the column layout of Y.  Y is the plain entry's bit for bit: one step body serves both kernels.  The refusals are
 * ggcn_bilstm_recurrence's, plus NULL gates / C / Hprev; the bias pointers stay optional.
 *
 * ggcn_bilstm_recurrence_backward: from dY [B*T, lddy] (the gradient of Y), the saved gates [B*T, ldg] and C, all T steps and both
 * directions in ONE launch, each direction's time walked backwards.  Per sentence and direction, with dh = dY[b,t,d] + dh_rec and
 * a carried dc (both zero at the start):
 *     tc = tanh(c_t)    do = dh*tc         dc += dh*o*(1-tc^2)
 *     di = dc*g         dg = dc*i          df = dc*c_{t-1}          dc <- dc*f
 *     da = [ di*i(1-i) | df*f(1-f) | dg*(1-g^2) | do*o(1-o) ]  -> dG[b*T+t, d*4hd:(d+1)*4hd]        dh_rec = da . Whh_d
 * c_{t-1} is read from C (zero at the direction's first step), i(1-i) and the like are taken from the stored float32 gates,
 * tanh(c) is recomputed.  dG [B*T, lddg] is the gradient of G + bias: from it, with the library's fixed-order products,
 *     d[W_ih_f ; W_ih_r] [8hd, I] = ggcn_dweight(X = dG, K = 8hd, dH = x, F = I)           already in nn.LSTM layout
 *     dW_hh_d [4hd, hd] = ggcn_dweight(X = dG + d*4hd, K = 4hd, dH = Hprev + d*hd, F = hd)
 *     d bias_f | d bias_r = ggcn_colsum(dG, lddg, B*T, 8hd)        (b_ih and b_hh both receive it)
 *     dX = dG . [W_ih_f ; W_ih_r] = ggcn_linear on the ggcn_weight_pack(transposed = 0) image of the [8hd, I] stack
 * Grid and workgroup as the forward's; a thread keeps a 128-long COLUMN piece of Whh_d in registers, da sits in LDS, the four
 * quarter sums of dh_rec are added in a fixed order, dc and dh_rec never leave the chip.  Exact fp32 FMA chains, no atomics: two
 * calls give the same bits, a sentence's result does not depend on B or on its place in a tile, and the two directions run the
 * same arithmetic.  No synchronisation.  Refusals, all before any launch: NULL dY / gates / C / Whh_f / Whh_r / dG, B or T <= 0,
 * lddy < 2 hd, ldg or lddg < 8 hd, Whh_f or Whh_r off 16 bytes, dG overlapping gates (dG is a buffer of its own, so that a second
 * backward can read the gates again) -> GGCN_EINVAL; hd != 128 and B*T >= 2^31 -> GGCN_EUNSUPPORTED. */
int ggcn_bilstm_recurrence_save(const float *G, int64_t ldg, const float *Whh_f, const float *Whh_r,
                                const float *bias_f, const float *bias_r, float *Y, int64_t ldy, int B, int T, int hd,
                                float *gates, float *C, float *Hprev, ggcn_stream_t stream);
int ggcn_bilstm_recurrence_backward(const float *dY, int64_t lddy, const float *gates, int64_t ldg, const float *C,
                                    const float *Whh_f, const float *Whh_r, float *dG, int64_t lddg, int B, int T, int hd,
                                    ggcn_stream_t stream);

/* ---- range check for GGCN_PREC_F16MX8 (on demand, not on the forward path) ----------------
 * out[0] = max |x| over the finite entries of X [M,K] (fp32, or IEEE half when is_half != 0; ld in
 * elements), out[1] = 1.0f when some entry is NaN or infinite.  f16mx8 needs |x|, |w| < 65504 and keeps
 * its full accuracy for |x| <= 448; the caller reads the two floats back when it wants the verdict. */
int ggcn_absmax(const void *X, int is_half, int64_t ld, int64_t M, int K, float *out, ggcn_stream_t stream);

/* ---- sticky range flag of GGCN_PREC_F16MX8 (what makes it safe as a default) ----------------------
 * models/gcn.py:34 multiplies in fp32 and has no range limit; f16mx8 meets the 1e-4 parity gate only inside a window, and
 * says so when the data leaves it.  Every f16mx8 main loop (ggcn_linear, ggcn_layer_fused, ggcn_block_fused) keeps the
 * running maximum of the |x| it splits (one v_max3 per two values: < 1 % of the block) and ORs these bits into a sticky
 * per-device flag:
 *   GGCN_RANGE_OVERFLOW  a value reached fp16's largest finite value 65504 (inf included; a NaN input shows as NaN in the
 *                        output instead); ggcn_weight_pack sets it for such a weight.  Results are saturated.
 *   GGCN_RANGE_WINDOW    a value left |x| <= 448, the range in which the fp8 correction terms are unsaturated: from there
 *                        on the product has plain fp16 accuracy (2^-12 relative), outside the parity gate.
 *   GGCN_RANGE_HIDDEN    the one-launch layer / block of graphs of <= 32 nodes (fp16 aggregation planes) could not rule
 *                        out |hidden| >= 65504: max|x| * max_f sum_k |w[k,f]| (+ max |mid bias|) reached it (a sufficient
 *                        bound from the weight image's trailer, not a detection: NaN is possible).
 * Any bit means "re-run with GGCN_PREC_BF16X3" (full fp32 range).  This call ORs the flag into *flag (device memory,
 * 4 bytes, zeroed by the caller) in stream order and, with clear != 0, resets it; the caller copies the word to the host
 * whenever it likes.  (The experimental f16mx6 form sets OVERFLOW and HIDDEN; its block scales have no window.) */
enum ggcn_range_bits { GGCN_RANGE_OVERFLOW = 1, GGCN_RANGE_WINDOW = 2, GGCN_RANGE_HIDDEN = 4 };
int ggcn_range_flag(uint32_t *flag, int clear, ggcn_stream_t stream);

/* ---- test hook: known garbage in every CU's LDS ---------------------------------------------------
 * Fills the whole LDS (160 KiB) of every CU with the 32-bit `pattern`, in stream order: the next kernel on the stream
 * starts on LDS whose stale contents are known.  The hardware never clears LDS between kernels, so a kernel that reads
 * a location it did not write itself returns whatever an EARLIER kernel left there -- a result that depends on the
 * process's history (models/gcn.py:41 and bert_amir5.py:635-640 have no such state).  The parity tests run every
 * LDS-resident path behind several patterns (+inf, -inf, NaN / id 0xFFFF) and demand bit-identical outputs. */
int ggcn_debug_poison_lds(uint32_t pattern, ggcn_stream_t stream);

/* ---- box calibration (diagnostics for bench.py's `box` block; never on the product path) ---------
 * The block kernel runs at the board's power cap, so its time follows the clock a given device holds under an MFMA-dense
 * load (devices differ by > 10 %).  Two probes make a figure taken on one box readable on another:
 * ggcn_debug_mfma_calibrate launches n_wg workgroups (256 threads, two per CU) that issue, per wavefront and stage, the
 * matrix-pipe work of the f16mx8 main loop -- 16 v_mfma_f32_32x32x16_f16 + 8 v_mfma_scale_f32_32x32x64_f8f6f4 on random
 * register operands -- and nothing else (no memory or LDS traffic, no barrier).  n_wg = 6144, stages = 24 is exactly the
 * main-loop MFMA work of ggcn_block_fused at BASELINE config 2.  stamps (NULL or uint64[2 * n_wg]) receives per workgroup
 * {d(s_memtime) in shader cycles, d(s_memrealtime) in 10 ns ticks} around its loop: clock under load = cycles / ticks x 100 MHz.
 * ggcn_debug_block_fused_stamped is ggcn_block_fused through a diagnostic instantiation of the same kernel that takes the
 * same two stamps around ITS main loop (f16mx8, T = 32, B % 4 == 0, K % 32 == 0, 16-byte aligned rows only; stamps
 * uint64[2 * workgroups], workgroups = ceil(B/16) * ceil(F/256) * 8): same results, a few percent slower; no product launch
 * executes a stamp. */
int ggcn_debug_mfma_calibrate(int n_wg, int stages, uint64_t *stamps, float *sink, ggcn_stream_t stream);
/* Which kernel ggcn_block_fused takes for the whole block (all outputs, GGCN_PREC_F16MX8, 16-byte aligned operands) at this shape:
 * 8 = one eight-wavefront workgroup per (row block, 256-column slice) that stages the row block's X planes once for its W1 and its
 * W12 tiles (fused_block8.hip) -- batches that make >= 6 rounds of one workgroup per CU, or >= 3 whole rounds; 2-4 % less time in
 * steady state at the board's power cap, the same bits -- else 4 = two four-wavefront workgroups per CU (fused_layer.hip).
 * GGCN_BLOCK_FORM=4 in the environment (read per call) keeps the four-wavefront kernel. */
int ggcn_block_fused_form(int B, int T, int K, int F);

/* Which kernel form a dense linear entry takes for these operands: a host-only query that launches nothing and looks at the
 * pointer VALUES for their alignment only (nothing is dereferenced; W is looked at for GGCN_PREC_FP32 alone, `precision` by the
 * entries that have one).  The launchers dispatch on the very function that answers here.  Returns a set of
 * ggcn_linear_form_bits, or -ggcn_status where the entry would refuse the call (the weight image, which the query does not see,
 * taken as valid):
 *   split kernels (ggcn_linear bf16x3 / f16mx8, ggcn_linear_h bf16x3 / f16mx8, ggcn_linear_bf16, ggcn_linear_out_bf16),
 *   tile 128 rows x 256 columns, 32 k per stage:
 *     XVEC              16-byte X loads: K and ldx multiples of 16 / sizeof(x), X 16-byte aligned, and
 *                       ldx * sizeof(x) * 257 < 2^31 (a tile's rows are addressed by 32-bit byte offsets from its first row)
 *     XVEC|KFULL        and K % 32 == 0: no k guard in the main loop
 *     XVEC|KFULL|VST    and float32 Y with F, ldy multiples of 4, Y 16-byte aligned: 16-byte row stores through LDS
 *     0                 element loads, guarded stores
 *     ggcn_linear_scaled takes XVEC|KFULL|VST or refuses.
 *   fp16 kernel (ggcn_linear_h, GGCN_PREC_F16), 64 k per stage: XVEC (K, ldx % 8 == 0, aligned), XVEC|KFULL (K % 64 == 0), 0.
 *   fp32 kernel (ggcn_linear, GGCN_PREC_FP32), tile 128 x 128, 16 k per stage: XVEC (K, ldx % 4 == 0, X aligned) and WVEC
 *   (F, ldw % 4 == 0, W aligned) independently; beyond 65535 row tiles the launcher walks the rows in slices of 65535 tiles. */
enum ggcn_linear_entry {
    GGCN_ENTRY_LINEAR = 0,          /* ggcn_linear */
    GGCN_ENTRY_LINEAR_H = 1,        /* ggcn_linear_h */
    GGCN_ENTRY_LINEAR_BF16 = 2,     /* ggcn_linear_bf16 */
    GGCN_ENTRY_LINEAR_OUT_BF16 = 3, /* ggcn_linear_out_bf16 */
    GGCN_ENTRY_LINEAR_SCALED = 4    /* ggcn_linear_scaled */
};
enum ggcn_linear_form_bits {
    GGCN_FORM_XVEC = 1,   /* 16-byte X loads */
    GGCN_FORM_KFULL = 2,  /* whole k stages */
    GGCN_FORM_VST = 4,    /* 16-byte row stores through LDS */
    GGCN_FORM_WVEC = 8    /* 16-byte W loads (the fp32 kernel) */
};
int ggcn_linear_form(int entry, const void *X, int64_t ldx, const void *W, int64_t ldw, const void *Y, int64_t ldy, int64_t M,
                     int K, int F, int precision);

/* The eight-wavefront kernel of the block called directly (fused_block8.hip): the kernel ggcn_block_fused itself runs for large
 * batches (the rule of ggcn_block_fused_form above: every output, GGCN_PREC_F16MX8, T <= 32, K % 32 == 0, F a multiple of 256,
 * 16-byte aligned operands, >= 6 rounds of one workgroup per CU or >= 3 whole rounds).  Workgroups of EIGHT wavefronts share a row
 * block's X planes between the W1 and the W12 column tiles of a 256-column slice (no gcn1).  Bit-identical to the four-wavefront
 * kernel; the same argument checks and messages.  Here for tools/block8_timing.py and the tests; the XCD mapping and staging
 * switches of the experiment are read from the environment (GGCN_LAB_BLOCK8_*; _PRIO: the W12 group of every workgroup at
 * s_setprio 1, which ggcn_block_fused always sets). */
int ggcn_lab_block_fused8(const float *X, int64_t ldx, const void *wpack1, const void *wpack12, const void *graph_ops,
                          const void *graph_ops2, const float *bias1, const float *bias_mid, const float *bias2,
                          int B, int T, int K, int F, const float *gate1, const float *gate2, float *x_out, int64_t ld2,
                          float *x1, float *y1, float *pool_out, float *overlap_partial, uint64_t *stamps, ggcn_stream_t stream);
/* (stamps: NULL, or uint64[workgroups * 2 groups * 4]: s_memrealtime at workgroup start / main loop start / main loop end / end) */
int ggcn_debug_block_fused_stamped(const float *X, int64_t ldx, const void *wpack1, const void *wpack12,
                                   const void *graph_ops, const void *graph_ops2, const float *bias1, const float *bias_mid,
                                   const float *bias2, int B, int T, int K, int F, const float *gate1, const float *gate2,
                                   float *gcn1, int64_t ld1, float *x_out, int64_t ld2, float *x1, float *y1, float *pool_out,
                                   float *overlap_partial, int precision, uint64_t *stamps, ggcn_stream_t stream);

/* ---- sub-word -> word pooling (the step before the path) ---------------
 * Replaces models/bert_amir5.py:600 `x = torch.bmm(transform, x)`:
 *   Y[b,r,:] = sum_c A[b,r,c] * X[b,c,:]
 * A [B,R,C] float32 with ELEMENT strides (the reference passes the non-contiguous slice
 * inputs['transform'][:, :T, :L]; data_utils.py:749-766 puts 1/l on the l sub-word positions of
 * word r), C <= 2048.  X [B,C,D] and Y [B,R,D] float32: row c of batch b starts at
 * X + b*x_batch + c*ldx (elements), likewise Y.  Only the non-zeros of A are multiplied, in
 * ascending c.  The backward dX = A^T . dY is the same call with sa_r / sa_c and R / C swapped. */
int ggcn_subword_pool(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c,
                      const float *X, int64_t x_batch, int64_t ldx,
                      float *Y, int64_t y_batch, int64_t ldy,
                      int B, int R, int C, int D, ggcn_stream_t stream);
/* The same with X and Y in bfloat16 (x from BERT under torch.autocast(dtype=torch.bfloat16)): fp32 sums, Y rounded to
 * nearest even once -- torch.bmm's result under autocast.  A stays float32. */
int ggcn_subword_pool_bf16(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c,
                           const void *X, int64_t x_batch, int64_t ldx,
                           void *Y, int64_t y_batch, int64_t ldy,
                           int B, int R, int C, int D, ggcn_stream_t stream);
/* The same straight from BERT's layer list (bert_amir5.py:596 concatenates the 12 layer outputs only to pool them at :600):
 *   Y[b, r, l*Dl + f] = sum_c A[b,r,c] * X_l[b,c,f],  l = 0..n_layers-1, ONE launch, no concatenated copy of x.
 * layers: a HOST array of n_layers device pointers (read during the call, passed to the kernel by value in its argument
 * block: capture-safe); every layer is [B,C,Dl] with the SAME x_batch and ldx (elements), float32 or, with is_bf16 != 0,
 * bfloat16 (then Y is bfloat16 too: fp32 sums, one RNE in the store).  A, its element strides, C <= 2048, "non-zeros only,
 * ascending c": as ggcn_subword_pool.  Layer l's columns of Y are bit for bit what ggcn_subword_pool / _bf16 write for
 * that layer alone (D = Dl, Y + l*Dl).  Y row r of batch b starts at Y + b*y_batch + r*ldy, ldy >= n_layers*Dl.
 * The vector form is taken when Dl, ldx, ldy, x_batch and y_batch are multiples of 4 and Y and every layer pointer are
 * aligned to 16 bytes (8 for bfloat16); otherwise the whole launch takes the scalar form (same bits).
 * GGCN_EINVAL: a NULL A, layers, Y or layers[l]; n_layers < 1; B, R, C or Dl <= 0; ldx < Dl; ldy < n_layers*Dl; a pointer
 * not aligned to its element.  GGCN_EUNSUPPORTED: n_layers > GGCN_POOL_MAX_LAYERS (split the layers into groups, each into
 * its own columns of Y); C > 2048; B*R > INT32_MAX; a grid dimension past 65535.  All before any launch. */
#define GGCN_POOL_MAX_LAYERS 16
int ggcn_subword_pool_layers(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c,
                             const void *const *layers, int n_layers, int is_bf16, int64_t x_batch, int64_t ldx,
                             void *Y, int64_t y_batch, int64_t ldy, int B, int R, int C, int Dl, ggcn_stream_t stream);
/* host-only: 1 = vector form, 0 = scalar form, -ggcn_status where the entry would refuse (ggcn_last_error names
 * ggcn_subword_pool_layers); launches nothing and dereferences nothing on the device.  The launcher dispatches on the
 * function that answers here. */
int ggcn_subword_pool_layers_form(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c,
                                  const void *const *layers, int n_layers, int is_bf16, int64_t x_batch, int64_t ldx,
                                  const void *Y, int64_t y_batch, int64_t ldy, int B, int R, int C, int Dl);
/* The step of the baselines bert_ed / bertdm (models/bert_ed.py:46-62, models/bertdm.py:164-198) in ONE launch, from BERT's
 * layer list to what the final linear reads.  With v[b, r, l*Dl + f] = sum_c A[b,r,c] * X_l[b,c,f] exactly as
 * ggcn_subword_pool_layers forms it (float32 FMAs in ascending c from 0; bfloat16 layers: one RNE to bfloat16),
 * a = clamp(anchor[b], 0, R-1) and n = clamp(length[b], 0, R), for j = 0..n_layers*Dl-1:
 *   Z[b, j]               = v[b, a, j]                                                  (the anchor word's row)
 *   Z[b, z_section + j]   = max(m0, max_{r <= a}    (v[b,r,j] + 1.0f)) - 1.0f,  m0 = 1.0f if a < R-1, else -inf
 *   Z[b, 2*z_section + j] = max(1.0f, max_{a < r < n} (v[b,r,j] + 1.0f)) - 1.0f
 * the last two only with sides != 0.  This is bertdm.py:176-185 bit for bit: it multiplies by a 0/1 mask, adds ones, takes the
 * max and subtracts ones, so a masked word contributes exactly 1.0f and every value goes through the rounding of v + 1.  A
 * NaN in a row that is pooled propagates, as torch.max's.  Masked rows are never read: the one divergence is a masked row
 * that is not finite, which the reference turns into NaN (inf * 0) and this entry ignores.  [B, R, n_layers*Dl] is never
 * formed; the rows are walked in ascending r without atomics, so a sentence gives the same bits alone as in a batch.
 * anchor, length: int64 [B] on the device, read by the kernel (no host read: capture-safe) and clamped there; length may be
 * NULL with sides == 0 and is then never touched.  Z: float32 always (a bfloat16 value is exact in it), row b at Z + b*ldz;
 * z_section (elements) is the distance between the three parts, so that a group of GGCN_POOL_MAX_LAYERS layers can write
 * into its own columns of a wider Z.  A, layers, x_batch, ldx, C <= 2048: as ggcn_subword_pool_layers.  The vector form is
 * taken when Dl, ldx, x_batch, ldz and (with sides) z_section are multiples of 4, Z is aligned to 16 bytes and every layer
 * pointer to 16 (8 for bfloat16); otherwise the whole launch takes the scalar form (same bits).
 * GGCN_EINVAL: a NULL A, layers, layers[l], anchor or Z; a NULL length with sides; n_layers < 1; B, R, C or Dl <= 0; with
 * sides z_section < n_layers*Dl; ldx < Dl; ldz < n_layers*Dl + (sides ? 2*z_section : 0); a pointer not aligned to its
 * element.  GGCN_EUNSUPPORTED: n_layers > GGCN_POOL_MAX_LAYERS; C > 2048; B*R > INT32_MAX; more than 65535 workgroups a
 * sentence.  All before any launch. */
int ggcn_anchor_pool_layers(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c,
                            const void *const *layers, int n_layers, int is_bf16, int64_t x_batch, int64_t ldx,
                            const int64_t *anchor, const int64_t *length, int sides,
                            float *Z, int64_t ldz, int64_t z_section,
                            int B, int R, int C, int Dl, ggcn_stream_t stream);
/* host-only: 1 = vector form, 0 = scalar form, -ggcn_status where the entry would refuse (ggcn_last_error names
 * ggcn_anchor_pool_layers); launches nothing and dereferences nothing on the device. */
int ggcn_anchor_pool_layers_form(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c,
                                 const void *const *layers, int n_layers, int is_bf16, int64_t x_batch, int64_t ldx,
                                 const int64_t *anchor, const int64_t *length, int sides,
                                 const float *Z, int64_t ldz, int64_t z_section,
                                 int B, int R, int C, int Dl);
/* The bf16x3 linear on pooled layers: the BiLSTM's input projection (bert_amir5.py:610) read straight from BERT's layer list,
 *   Y[b*R + r, f] = sum_l sum_k ( sum_c A[b,r,c] * X_l[b,c,k] ) * W[l*Dl + k, f],   ONE launch,
 * so that neither the concatenation [B,C,n_layers*Dl] nor the pooled words [B,R,n_layers*Dl] exist.  A, its three element
 * strides, layers (a HOST array of float32 device pointers, read during the call and passed by value: capture-safe), x_batch,
 * ldx, C <= 2048: as ggcn_subword_pool_layers.  wpack: the ggcn_weight_pack(GGCN_PREC_BF16X3) image of the
 * [K = n_layers*Dl, F] matrix W.  Y: float32, row b*R + r at Y + (b*R + r)*ldy; no bias.
 * Arithmetic: a pooled value is formed as ggcn_subword_pool_layers forms it (from 0.0f, one float32 FMA per non-zero of the
 * row of A in ascending c; an absent entry is skipped, so a NaN in a row of X that no row of A selects does not arrive), then
 * split and multiplied as ggcn_linear(GGCN_PREC_BF16X3) does: Y is bit for bit that entry on the output of
 * ggcn_subword_pool_layers.  A row of A with any number of non-zeros is taken (rows beyond the loader's fast capacity are
 * slower, not different).
 * GGCN_EINVAL: a NULL A, layers, layers[l], wpack or Y; n_layers < 1; B, R, C, Dl or F <= 0; ldx < Dl; ldy < F; a pointer not
 * aligned to its element; wpack off 16 bytes.  GGCN_EUNSUPPORTED: n_layers > GGCN_POOL_MAX_LAYERS; C > 2048;
 * B*R > INT32_MAX; more k-steps than ggcn_weight_pack takes (n_layers*Dl > 1048560); and the layouts the kernel has no form
 * for -- Dl % 32 != 0; ldx, x_batch, F or ldy not a multiple of 4; a layer or Y off 16 bytes -- for which the caller takes
 * ggcn_subword_pool_layers and ggcn_linear.  All before any launch. */
int ggcn_linear_pooled_layers(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c,
                              const void *const *layers, int n_layers, int64_t x_batch, int64_t ldx,
                              const void *wpack, float *Y, int64_t ldy,
                              int B, int R, int C, int Dl, int F, ggcn_stream_t stream);
/* host-only: 1 = the launch is taken, -ggcn_status where the entry would refuse (ggcn_last_error names
 * ggcn_linear_pooled_layers); launches nothing and dereferences nothing on the device. */
int ggcn_linear_pooled_layers_form(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c,
                                   const void *const *layers, int n_layers, int64_t x_batch, int64_t ldx,
                                   const void *wpack, const float *Y, int64_t ldy,
                                   int B, int R, int C, int Dl, int F);

/* ---- bfloat16 features (training and inference under torch.autocast(dtype=torch.bfloat16)) ----------------------
 * X (the layer's input) in bfloat16; weights, bias, gates, `out`, pools and dW stay float32, dX is bfloat16 -- the
 * dtypes of the reference layer under bf16 autocast (models/gcn.py:34-43: the `/ denom` promotes to float32).  A bf16
 * value is exact in the MFMA's operand type, so every product is TWO bf16 MFMAs on the GGCN_PREC_BF16X3 image of W
 * (hi.Whi + hi.Wlo; ggcn_weight_pack(..., GGCN_PREC_BF16X3)): the accuracy class of GGCN_PREC_BF16X3, the fp32 range.
 *   ggcn_linear_bf16      Y [M,F] float32 = X [M,K] bf16 (row stride ldx) . W            (then ggcn_aggregate)
 *   ggcn_linear_out_bf16  Y [M,F] bf16 (RNE in the store) = X [M,K] float32 . W          (dX = dH.W^T on the W^T image)
 *   ggcn_layer_fused_bf16 ggcn_layer_fused on bf16 X for graphs of <= 32 nodes (graph_ops of ggcn_graph_operands),
 *                         same gates, pools, overlap partials / reduction and bias (or NULL); no precision argument
 *   ggcn_layer_fused_bf16_drop  the same launch with the gates' training-mode dropout drawn in its epilogue: p, seed and the
 *                         three stream selectors of ggcn_layer_fused_drop (same hash, same ggcn_dropout_mask, same backward)
 *   ggcn_layer_fused_bf16_wide  graphs of 33..256 nodes in one launch: row masks (ggcn_rowmask_from_dense / ggcn_csr_rowmask),
 *                         edge_lists = NULL or the ggcn_graph_edge_lists blocks (read for T > 128 only), overlap partials /
 *                         reduction as ggcn_layer_fused; p = 0: no dropout, else as ggcn_layer_fused_bf16_drop
 *                         A T outside an entry's range returns GGCN_EUNSUPPORTED and names the entry to use; dropout needs
 *                         B*T*F < 2^32; overlap_in and overlap_out go together.
 *   ggcn_block_fused_bf16 ggcn_block_fused on bf16 X (graphs of <= 32 nodes): its argument list without `precision` -- always
 *                         the GGCN_PREC_BF16X3 images of W1 and W12 and the plane-0 blocks of ggcn_graph_operands2.  Same
 *                         contract: layer 1's outputs (gate1, x1, y1; gcn1 and overlap_partial optional) all together or none
 *                         (none = the eval form: only the W12 tiles are launched, graph_ops may be NULL), bias_mid required
 *                         (zeros when gc1 has no bias), all outputs float32.  T > 32: GGCN_EUNSUPPORTED (one
 *                         ggcn_layer_fused_bf16_wide per layer)
 *   ggcn_aggregate_bf16   Z [B*T,K] float32 (row stride ldz) = D.A.X for bf16 X (row stride ldx): ggcn_aggregate's sums over a
 *                         node's neighbours in CSR order, fp32 accumulation, divided by rowsum + 1; no bias, gates or pools.
 *                         Z equals ggcn_aggregate on the float32 copy of X bit for bit.  vals = NULL: 0/1 adjacency.  The
 *                         input of ggcn_layer_fused_prebias for the folded evaluation of graphs of 33..256 nodes
 *   ggcn_dweight_bf16     dW [K,F] float32 = X^T . dH with bf16 X, float32 dH: X is transposed in bf16 and dH packed,
 *                         then the split-K form of ggcn_dweight(GGCN_PREC_BF16X3); deterministic; workspace of
 *                         ggcn_dweight_bf16_workspace_bytes(n_rows, K, F) bytes, 16-byte aligned
 * Null pointers, ldx < K, ldy / ldo < F, misaligned elements and images or blocks off 16 bytes return GGCN_EINVAL without a launch. */
int ggcn_linear_bf16(const void *X, int64_t ldx, const void *wpack, float *Y, int64_t ldy,
                     int64_t M, int K, int F, ggcn_stream_t stream);
int ggcn_linear_out_bf16(const float *X, int64_t ldx, const void *wpack, void *Y, int64_t ldy,
                         int64_t M, int K, int F, ggcn_stream_t stream);
int ggcn_layer_fused_bf16(const void *X, int64_t ldx, const void *wpack, const void *graph_ops,
                          const float *bias, int B, int T, int K, int F,
                          const float *store_gate, const float *pool_gate_a, const float *pool_gate_b,
                          float *out, int64_t ldo, float *pool_a, float *pool_b,
                          float *overlap_partial, const float *overlap_in, float *overlap_out,
                          ggcn_stream_t stream);
int ggcn_layer_fused_bf16_drop(const void *X, int64_t ldx, const void *wpack, const void *graph_ops,
                               const float *bias, int B, int T, int K, int F,
                               const float *store_gate, const float *pool_gate_a, const float *pool_gate_b,
                               float *out, int64_t ldo, float *pool_a, float *pool_b,
                               float *overlap_partial, const float *overlap_in, float *overlap_out,
                               float p, uint64_t seed, int stream_store, int stream_a, int stream_b, ggcn_stream_t stream);
int ggcn_layer_fused_bf16_wide(const void *X, int64_t ldx, const void *wpack, const uint32_t *rowmask, const void *edge_lists,
                               const float *bias, int B, int T, int K, int F,
                               const float *store_gate, const float *pool_gate_a, const float *pool_gate_b,
                               float *out, int64_t ldo, float *pool_a, float *pool_b,
                               float *overlap_partial, const float *overlap_in, float *overlap_out,
                               float p, uint64_t seed, int stream_store, int stream_a, int stream_b, ggcn_stream_t stream);
int ggcn_block_fused_bf16(const void *X, int64_t ldx, const void *wpack1, const void *wpack12,
                          const void *graph_ops, const void *graph_ops2,
                          const float *bias1, const float *bias_mid, const float *bias2,
                          int B, int T, int K, int F, const float *gate1, const float *gate2,
                          float *gcn1, int64_t ld1, float *x_out, int64_t ld2,
                          float *x1, float *y1, float *pool_out, float *overlap_partial,
                          ggcn_stream_t stream);
int ggcn_aggregate_bf16(const void *X, int64_t ldx, const int32_t *rowptr, const int32_t *colidx,
                        const float *vals, int B, int T, int K, float *Z, int64_t ldz,
                        ggcn_stream_t stream);
size_t ggcn_dweight_bf16_workspace_bytes(int64_t n_rows, int K, int F);
int ggcn_dweight_bf16(const void *X, int64_t ldx, const float *dH, int64_t ldg, int64_t n_rows, int K, int F,
                      float *dW, int64_t lddw, void *workspace, ggcn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GGCN_H */
