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

// The f16mx8 range flag has one copy per translation unit; GGCN_RANGE_FLAG_TU (f16mx8_core.h) hands each copy's reader to the
// registry behind ggcn_range_flag (capi.hip) when the library is loaded.
typedef int (*RangeFlagReader)(unsigned int *dst, int clear, hipStream_t st);
int register_range_flag_reader(RangeFlagReader reader);

// ---- what more than one translation unit uses ---------------------------------
// An entry of ggcn.h whose C function is its launcher is defined extern "C" in the launcher's .hip file and needs nothing here.
// Declared below: the launchers of the entries that capi.hip defines (those with checks, a dispatch or a description of their
// own), the form rules those entries share with their launchers, and the internals of the weight gradient.
int linear_fp32(const float *X, int64_t ldx, const float *W, int64_t ldw, float *Y, int64_t ldy,
                int64_t M, int K, int F, hipStream_t st);

// Which kernel form a linear launcher takes, as ggcn_linear_form_bits (ggcn_linear_form answers with these, and the launchers
// themselves dispatch on them: one rule).  A bit is only set where the form that needs it is taken: KFULL implies XVEC, VST both.
// x_bytes: sizeof of X's element; y_f32: Y is float32 (the staged row stores exist for it alone).
int linear_split_form(int x_bytes, bool y_f32, const void *X, int64_t ldx, const void *Y, int64_t ldy, int K, int F);   // linear_split.hip: launch_linear
int linear_f16_form(const void *X, int64_t ldx, int K);                                                                // linear_split.hip: launch_linear_f16
int linear_fp32_form(const void *X, int64_t ldx, const void *W, int64_t ldw, int K, int F);                            // linear_fp32.hip
int64_t linear_split_grid(int64_t M, int F);   // workgroups of the split / fp16 kernels (refused beyond INT32_MAX)

int linear_packed(const float *X, int64_t ldx, const void *wpack, float *Y, int64_t ldy,
                  int64_t M, int K, int F, int precision, hipStream_t st);

bool linear_scaled_takes(const float *X, int64_t ldx, const float *Y, int64_t ldy, int K, int F);   // the shapes ggcn_linear_scaled takes
int linear_packed_h(const void *X, int64_t ldx, const void *wpack, void *Y, int64_t ldy, int64_t M, int K,
                    int F, int precision, hipStream_t st);
// bf16 features (linear_split.hip): bf16 X -> fp32 Y, and fp32 X -> bf16 Y (dX of the backward), both on the bf16x3 image
int linear_bf16(const void *X, int64_t ldx, const void *wpack, float *Y, int64_t ldy, int64_t M, int K, int F, hipStream_t st);
int linear_out_bf16(const float *X, int64_t ldx, const void *wpack, void *Y, int64_t ldy, int64_t M, int K, int F, hipStream_t st);

int gate_pool_backward(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                       const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa,
                       const float *d_pb, int B, int T, int F, float *dY, int64_t ldy, float *d_sg,
                       float *d_ga, float *d_gb, float *d_bsum, hipStream_t st, const struct DropSpec *drop = nullptr);
int gate_pool_backward_agg(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                           const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa,
                           const float *d_pb, const uint32_t *rowmask, int B, int T, int F, float *dH, int64_t ldh,
                           float *d_sg, float *d_ga, float *d_gb, float *d_bsum, hipStream_t st, const struct DropSpec *drop = nullptr,
                           float *dh_amax = nullptr);
int gate_pool_backward_weighted(const float *out, int64_t ldo, const float *store_gate, const float *gate_a, const float *gate_b,
                                const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb, const void *graph_ops_wt,
                                const float *inv, int B, int T, int F, float *dH, int64_t ldh, float *dY, int64_t ldy, float *d_sg,
                                float *d_ga, float *d_gb, float *d_bsum, hipStream_t st, const struct DropSpec *drop = nullptr);   // gate_pool_backward_weighted.hip

// the weight gradient: ggcn_dweight picks dweight (fp32) or dweight_bx3, which hands 16-byte aligned rows to dweight_tn and packs dH
// with weight_pack_rows (linear_split.hip)
size_t dweight_workspace_bytes(int64_t N, int K, int F);
size_t dweight_bx3_workspace_bytes(int64_t N, int K, int F);
bool dweight_tn_takes(const float *X, int64_t ldx, const float *G, int64_t ldg, int64_t N, int K, int F);   // dweight_tn.hip
size_t dweight_tn_workspace_bytes(int64_t N, int K, int F);
int dweight_tn(const float *X, int64_t ldx, const float *G, int64_t ldg, int64_t N, int K, int F, float *dW, int64_t lddw,
               void *workspace, hipStream_t st);
int dweight_bx3(const float *X, int64_t ldx, const float *G, int64_t ldg, int64_t N, int K, int F, float *dW,
                int64_t lddw, void *workspace, hipStream_t st);
int weight_pack_rows(const float *W, int64_t ldw, int64_t K_valid, int F, int k_steps_total, void *pack, hipStream_t st);
int dweight(const float *X, int64_t ldx, const float *G, int64_t ldg, int64_t N, int K, int F, float *dW,
            int64_t lddw, void *workspace, hipStream_t st);

int dense_head(const float *pooled, int64_t ldp, const float *Wt, int64_t ldw, const float *bias, int B, int H, int C,
               float *logits, int64_t ldl, const float *partials, int F_block, float *xy, hipStream_t st, unsigned *signal = nullptr);   // heads.hip

}  // namespace ggcn
