// Shared host-side helpers for libggcn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/ggcn.h"

namespace ggcn {

struct DropSpec;
constexpr int kWave = 64;  // CDNA wavefront

// Thread-local message behind ggcn_last_error().
char *error_buffer();
int fail(int code, const char *fmt, ...);

inline hipStream_t as_stream(ggcn_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Every launch goes through this: a refused launch becomes GGCN_ELAUNCH, never a silent no-op.
inline int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GGCN_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return GGCN_OK;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- per-kernel launchers (one per .hip file) --------------------------------
int csr_from_dense(const void *adj, int adj_dtype, int B, int T, int64_t sb, int64_t sr, int64_t sc,
                   int32_t *rowptr, int32_t *colidx, float *vals, int64_t capacity, uint32_t *rowmask,
                   int32_t *flags, void *workspace, hipStream_t st);
size_t csr_workspace_bytes(int64_t n_rows);
int csr_transpose(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, int32_t *rowptr_t,
                  int32_t *colidx_t, float *vals_t, void *workspace, hipStream_t st);
int rowmask_from_dense(const void *adj, int adj_dtype, int B, int T, int64_t sb, int64_t sr, int64_t sc,
                       uint32_t *rowmask, int32_t *flags, hipStream_t st);

int linear_fp32(const float *X, int64_t ldx, const float *W, int64_t ldw, float *Y, int64_t ldy,
                int64_t M, int K, int F, hipStream_t st);

// Which kernel form a linear launcher takes, as ggcn_linear_form_bits (ggcn_linear_form answers with these, and the launchers
// themselves dispatch on them: one rule).  A bit is only set where the form that needs it is taken: KFULL implies XVEC, VST both.
// x_bytes: sizeof of X's element; y_f32: Y is float32 (the staged row stores exist for it alone).
int linear_split_form(int x_bytes, bool y_f32, const void *X, int64_t ldx, const void *Y, int64_t ldy, int K, int F);   // linear_split.hip: launch_linear
int linear_f16_form(const void *X, int64_t ldx, int K);                                                                // linear_split.hip: launch_linear_f16
int linear_fp32_form(const void *X, int64_t ldx, const void *W, int64_t ldw, int K, int F);                            // linear_fp32.hip
int64_t linear_split_grid(int64_t M, int F);   // workgroups of the split / fp16 kernels (refused beyond INT32_MAX)

size_t weight_pack_bytes(int K, int F, int precision);
int weight_pack(const float *W, int64_t ldw, int K, int F, int precision, bool transposed, void *wpack, hipStream_t st);
int linear_packed(const float *X, int64_t ldx, const void *wpack, float *Y, int64_t ldy,
                  int64_t M, int K, int F, int precision, hipStream_t st);

bool linear_scaled_takes(const float *X, int64_t ldx, const float *Y, int64_t ldy, int K, int F);
int linear_scaled(const float *X, int64_t ldx, const void *wpack, float *Y, int64_t ldy, int64_t M, int K, int F, const float *amax,
                  hipStream_t st);
int linear_packed_h(const void *X, int64_t ldx, const void *wpack, void *Y, int64_t ldy, int64_t M, int K,
                    int F, int precision, hipStream_t st);
// bf16 features (linear_split.hip): bf16 X -> fp32 Y, and fp32 X -> bf16 Y (dX of the backward), both on the bf16x3 image
int linear_bf16(const void *X, int64_t ldx, const void *wpack, float *Y, int64_t ldy, int64_t M, int K, int F, hipStream_t st);
int linear_out_bf16(const float *X, int64_t ldx, const void *wpack, void *Y, int64_t ldy, int64_t M, int K, int F, hipStream_t st);
int aggregate_t(const float *G, int64_t ldg, const int32_t *rowptr_t, const int32_t *colidx_t,
                const float *vals_t, const float *src_scale, int B, int T, int F, float *out, int64_t ldo,
                hipStream_t st);
int inv_denominators(const int32_t *rowptr, const float *vals, int64_t n, float *inv, hipStream_t st);
int adjacency_grad(const float *dY, int64_t ldy, const float *hidden, int64_t ldh, const float *inv, const int32_t *rowptr,
                   const int32_t *colidx, const float *vals, int B, int T, int F, float *d_adj, hipStream_t st);   // adjacency_grad.hip
int aggregate_h(const void *Hd, int64_t ldh, const int32_t *rowptr, const int32_t *colidx, const float *vals,
                const float *bias, int B, int T, int F, const float *store_gate, const float *pool_gate_a,
                const float *pool_gate_b, void *out, int64_t ldo, float *pool_a, float *pool_b, hipStream_t st);

int layer_fused_h(const void *X, int64_t ldx, const void *wpack, const int32_t *rowptr, const int32_t *colidx,
                  const float *vals, const float *bias, int B, int T, int K, int F, const float *store_gate,
                  const float *pool_gate_a, const float *pool_gate_b, void *out, int64_t ldo, float *pool_a,
                  float *pool_b, hipStream_t st);

int aggregate(const float *Hd, int64_t ldh, const int32_t *rowptr, const int32_t *colidx,
              const float *vals, const float *bias, int B, int T, int F, const float *store_gate,
              const float *pool_gate_a, const float *pool_gate_b, float *out, int64_t ldo,
              float *pool_a, float *pool_b, hipStream_t st);

// Z = D.A.X on bf16 features (aggregate.hip): ggcn_aggregate's sums, bit for bit, without the float32 copy of X
int aggregate_bf16(const void *X, int64_t ldx, const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, int K,
                   float *Z, int64_t ldz, hipStream_t st);

int subword_pool(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const float *X, int64_t x_batch,
                 int64_t ldx, float *Y, int64_t y_batch, int64_t ldy, int B, int R, int C, int D, hipStream_t st);
int subword_pool_bf16(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *X, int64_t x_batch,
                      int64_t ldx, void *Y, int64_t y_batch, int64_t ldy, int B, int R, int C, int D, hipStream_t st);
// every layer of `layers` (a host array) into its own Dl columns of Y, one launch; ..._form: 1 vector / 0 scalar / -status, host only
int subword_pool_layers(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *const *layers, int n_layers,
                        int is_bf16, int64_t x_batch, int64_t ldx, void *Y, int64_t y_batch, int64_t ldy, int B, int R, int C,
                        int Dl, hipStream_t st);
int subword_pool_layers_form(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *const *layers, int n_layers,
                             int is_bf16, int64_t x_batch, int64_t ldx, const void *Y, int64_t y_batch, int64_t ldy, int B, int R,
                             int C, int Dl);
// the anchor's pooled row and, with sides, the two masked max-pools of bertdm.py:176-185 per sentence, one launch; ..._form as above
int anchor_pool_layers(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *const *layers, int n_layers,
                       int is_bf16, int64_t x_batch, int64_t ldx, const int64_t *anchor, const int64_t *length, int sides, float *Z,
                       int64_t ldz, int64_t z_section, int B, int R, int C, int Dl, hipStream_t st);
int anchor_pool_layers_form(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *const *layers, int n_layers,
                            int is_bf16, int64_t x_batch, int64_t ldx, const int64_t *anchor, const int64_t *length, int sides,
                            const float *Z, int64_t ldz, int64_t z_section, int B, int R, int C, int Dl);
// the bf16x3 linear on the pooled layers, the pooled words never stored (linear_pooled.hip); ..._form: 1 taken / -status, host only
int linear_pooled_layers(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *const *layers, int n_layers,
                         int64_t x_batch, int64_t ldx, const void *wpack, float *Y, int64_t ldy, int B, int R, int C, int Dl, int F,
                         hipStream_t st);
int linear_pooled_layers_form(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *const *layers, int n_layers,
                              int64_t x_batch, int64_t ldx, const void *wpack, const float *Y, int64_t ldy, int B, int R, int C,
                              int Dl, int F);
int csr_rowmask(const int32_t *rowptr, const int32_t *colidx, int B, int T, uint32_t *rowmask, hipStream_t st);
int graph_operands(const uint32_t *rowmask, int B, int T, void *ops, hipStream_t st);
int graph_edge_lists(const uint32_t *rowmask, int B, int T, void *lists, hipStream_t st);   // fused_wide8.hip
int graph_operands2(const uint32_t *rowmask, int B, int T, int plane, void *ops2, hipStream_t st);
int graph_operands_weighted(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, int plane, void *ops,
                            int *flag, hipStream_t st);
size_t graph_operands_weighted_wide_bytes(int B, int T);   // fused_wide.hip
int graph_operands_weighted_wide(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, void *ops, int *flag,
                                 hipStream_t st);
int graph_operands2_weighted(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, int plane, void *ops2,
                             int *flag, hipStream_t st);   // fused_weighted_drop.hip
int dropout_mask(int64_t rows, int F, float p, uint64_t seed, int sel, float *out, hipStream_t st);
int mfma_calibrate(int n_wg, int stages, unsigned long long *stamps, float *sink, hipStream_t st);   // calib.hip (diagnostics)
int overlap_reduce(const float *partials, int B, int F, float *xy, hipStream_t st);

int gate_pool_backward(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                       const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa,
                       const float *d_pb, int B, int T, int F, float *dY, int64_t ldy, float *d_sg,
                       float *d_ga, float *d_gb, float *d_bsum, hipStream_t st, const struct DropSpec *drop = nullptr);
int gate_pool_backward_agg(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                           const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa,
                           const float *d_pb, const uint32_t *rowmask, int B, int T, int F, float *dH, int64_t ldh,
                           float *d_sg, float *d_ga, float *d_gb, float *d_bsum, hipStream_t st, const struct DropSpec *drop = nullptr,
                           float *dh_amax = nullptr);
int rowmask_transpose(const uint32_t *rowmask, int B, int T, uint32_t *rowmask_t, hipStream_t st);   // gate_pool_backward_mma.hip
int gate_pool_backward_mma(const float *out, int64_t ldo, const float *store_gate, const float *gate_a, const float *gate_b,
                           const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb, const void *graph_ops,
                           const void *graph_ops_t, int B, int T, int F, float *dH, int64_t ldh, float *d_sg, float *d_ga,
                           float *d_gb, float *d_bsum, float *dh_amax, hipStream_t st);
size_t graph_operands_weighted_t_bytes(int B);   // gate_pool_backward_weighted.hip
int graph_operands_weighted_t(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, void *ops, int *flag,
                              hipStream_t st);
int gate_pool_backward_weighted(const float *out, int64_t ldo, const float *store_gate, const float *gate_a, const float *gate_b,
                                const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb, const void *graph_ops_wt,
                                const float *inv, int B, int T, int F, float *dH, int64_t ldh, float *dY, int64_t ldy, float *d_sg,
                                float *d_ga, float *d_gb, float *d_bsum, hipStream_t st, const struct DropSpec *drop = nullptr);
int rowmask_transpose_wide(const uint32_t *rowmask, int B, int T, uint32_t *rowmask_t, hipStream_t st);   // gate_pool_backward_wide.hip
int gate_pool_backward_wide(const float *out, int64_t ldo, const float *store_gate, const float *gate_a, const float *gate_b,
                            const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb, const uint32_t *rowmask_t,
                            const float *inv, int B, int T, int F, float *dH, int64_t ldh, float *d_sg, float *d_ga, float *d_gb,
                            float *d_bsum, hipStream_t st);
size_t graph_operands_weighted_wide_t_bytes(int B, int T);   // gate_pool_backward_weighted_wide.hip
int graph_operands_weighted_wide_t(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, void *ops, int *flag,
                                   hipStream_t st);
int gate_pool_backward_weighted_wide(const float *out, int64_t ldo, const float *store_gate, const float *gate_a, const float *gate_b,
                                     const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb, const void *graph_ops_wwt,
                                     const float *inv, int B, int T, int F, float *dH, int64_t ldh, float *dY, int64_t ldy, float *d_sg,
                                     float *d_ga, float *d_gb, float *d_bsum, hipStream_t st);
size_t colsum_workspace_bytes(int F);
int colsum(const float *X, int64_t ld, int64_t M, int F, float *out, void *workspace, hipStream_t st);

size_t dweight_workspace_bytes(int64_t N, int K, int F);
size_t dweight_bx3_workspace_bytes(int64_t N, int K, int F);
bool dweight_tn_takes(const float *X, int64_t ldx, const float *G, int64_t ldg, int64_t N, int K, int F);   // dweight_tn.hip
size_t dweight_tn_workspace_bytes(int64_t N, int K, int F);
int dweight_tn(const float *X, int64_t ldx, const float *G, int64_t ldg, int64_t N, int K, int F, float *dW, int64_t lddw,
               void *workspace, hipStream_t st);
int dweight_bx3(const float *X, int64_t ldx, const float *G, int64_t ldg, int64_t N, int K, int F, float *dW,
                int64_t lddw, void *workspace, hipStream_t st);
size_t dweight_bf16_workspace_bytes(int64_t N, int K, int F);
int dweight_bf16(const void *X, int64_t ldx, const float *G, int64_t ldg, int64_t N, int K, int F, float *dW,
                 int64_t lddw, void *workspace, hipStream_t st);
int weight_pack_rows(const float *W, int64_t ldw, int64_t K_valid, int F, int k_steps_total, void *pack, hipStream_t st);
int dweight(const float *X, int64_t ldx, const float *G, int64_t ldg, int64_t N, int K, int F, float *dW,
            int64_t lddw, void *workspace, hipStream_t st);

int absmax(const void *X, int is_half, int64_t ld, int64_t M, int K, float *out, hipStream_t st);
int poison_lds(uint32_t pattern, hipStream_t st);                       // range_check.hip (test hook)
int range_flag_linear(unsigned int *dst, int clear, hipStream_t st);   // linear_split.hip
int range_flag_fused(unsigned int *dst, int clear, hipStream_t st);    // fused_layer.hip
int range_flag_wide(unsigned int *dst, int clear, hipStream_t st);     // fused_wide.hip
int range_flag_wide8(unsigned int *dst, int clear, hipStream_t st);    // fused_wide8.hip
int range_flag_block8(unsigned int *dst, int clear, hipStream_t st);   // fused_block8.hip
int range_flag_weighted_drop(unsigned int *dst, int clear, hipStream_t st);   // fused_weighted_drop.hip
int range_flag_fused6(unsigned int *dst, int clear, hipStream_t st);   // fused6.hip (GGCN_WITH_F16MX6)

int transpose_f32(const float *W, int rows, int cols, int64_t ldw, float *Wt, hipStream_t st);
int gate_mlp(const float *aspect, int64_t lda, int B, int H, const float *w1t_a, const float *b1_a, const float *w2t_a,
             const float *b2_a, float *gate_a, const float *w1t_b, const float *b1_b, const float *w2t_b,
             const float *b2_b, float *gate_b, hipStream_t st);
int gate_mlp_save(const float *aspect, int64_t lda, int B, int H, const float *w1t_a, const float *b1_a, const float *w2t_a,
                  const float *b2_a, float *gate_a, const float *w1t_b, const float *b1_b, const float *w2t_b,
                  const float *b2_b, float *gate_b, float *hid_a, float *hid_b, hipStream_t st);
int gate_mlp_backward(const float *aspect, int64_t lda, int B, int H, const float *w1_a, const float *w2_a, const float *hid_a,
                      const float *gate_a, const float *d_gate_a, const float *w1_b, const float *w2_b, const float *hid_b,
                      const float *gate_b, const float *d_gate_b, float *d_aspect, int64_t ldda, float *Z, int64_t ldz, hipStream_t st);
int scores_head(const float *X, int64_t ldx, const float *aspect, int64_t lda, const float *logits, int64_t ldl,
                const float *fcw, int64_t ldw, const float *fcb, const float *dist, int64_t ldd, int B, int T, int H,
                int C, float *scores, int64_t lds_, float *kl_part, hipStream_t st);
int scores_head_backward(const float *X, int64_t ldx, const float *aspect, int64_t lda, const float *logits, int64_t ldl,
                         const float *fcw, int64_t ldw, const float *fcb, const float *dist, int64_t ldd, const float *scores,
                         int64_t lds_, const float *kl_part, const float *g_scores, int64_t ldgs, const float *g_kl, int B, int T,
                         int H, int C, float *dX, int64_t lddx, float *d_aspect, int64_t ldda, float *d_logits, int64_t lddl, float *G,
                         int64_t ldg, float *dc0, hipStream_t st);
size_t scores_head_dweight_workspace_bytes(int B, int H, int C);
int scores_head_dweight(const float *logits, int64_t ldl, const float *G, int64_t ldg, const float *dc0, int B, int H, int C, float *dW,
                        int64_t lddw, float *d_bias, void *workspace, hipStream_t st);

int dense_head(const float *pooled, int64_t ldp, const float *Wt, int64_t ldw, const float *bias, int B, int H, int C,
               float *logits, int64_t ldl, const float *partials, int F_block, float *xy, hipStream_t st, unsigned *signal = nullptr);

size_t overlap_workspace_bytes(int B);
int gate_overlap(const float *x1, const float *y1, int B, int F, float *xy, void *workspace,
                 hipStream_t st);

}  // namespace ggcn
