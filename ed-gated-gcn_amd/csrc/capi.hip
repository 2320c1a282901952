// extern "C" surface of libggcn_hip.so -- see include/ggcn.h for the contract.
// Argument checking lives here and in the per-kernel launchers; nothing in this
// library allocates, frees, copies to the host or synchronises.
// Defined here: the entries that have checks, a dispatch between launchers or a description (FusedArgs, DropSpec) of their own --
// the one-launch layers and blocks, the ggcn_linear* family and ggcn_linear_form, ggcn_dweight, the gate / pool backward entries that
// share a launcher, ggcn_dense_head[_signal], the *_bytes computed inline, ggcn_block_fused_form and ggcn_range_flag with its registry
// -- and the library's own (ggcn_abi_version, ggcn_has_f16mx6, ggcn_last_error).  Every other entry IS its launcher: it is defined
// extern "C" beside its kernels, at the end of that .hip file.
// The one-launch entries (ggcn_layer_fused*, ggcn_block_fused*, ggcn_lab_block_fused8, ggcn_debug_block_fused_stamped) check here
// only what is their own -- the graph sizes they take, the operands only they have, what must be looked at before it narrows into a
// field -- and write their arguments into a FusedArgs (fused_args.h) by name.  Everything else is checked once, on that description:
// launch_fused / fused_part_checks for a layer, launch_block for the three blocks, block_fused8 for the eight-wavefront kernel.
#include "fused_args.h"
#include <cstdlib>

#include <cstring>

namespace ggcn {

char *error_buffer()
{
    static thread_local char buf[512] = "";
    return buf;
}

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

namespace {
// The readers of the f16mx8 range flag, one per translation unit that holds a copy (GGCN_RANGE_FLAG_TU, f16mx8_core.h).  They
// register while the library loads, in no order this file may rely on: hence a function-local static, and no allocation.
constexpr int kMaxRangeFlagReaders = 16;
struct RangeFlagReaders {
    RangeFlagReader reader[kMaxRangeFlagReaders];
    int count;
    bool overflow;   // a registration found the array full: every ggcn_range_flag call says so
};
RangeFlagReaders &registered_readers()
{
    static RangeFlagReaders r = {};
    return r;
}
}  // namespace

int register_range_flag_reader(RangeFlagReader reader)
{
    RangeFlagReaders &r = registered_readers();
    if (r.count < kMaxRangeFlagReaders) r.reader[r.count++] = reader;
    else r.overflow = true;
    return r.count;
}

}  // namespace ggcn

using namespace ggcn;

namespace {
// what every entry with gate dropout checks of p and the gates' keep streams
int drop_entry_checks(const char *who, float p, int sel_store, int sel_a, int sel_b)
{
    if (!(p >= 0.0f && p < 1.0f) || sel_store < 0 || sel_store > 2 || sel_a < 0 || sel_a > 2 || sel_b < 0 || sel_b > 2)
        return fail(GGCN_EINVAL, "%s: p=%g streams %d %d %d", who, (double)p, sel_store, sel_a, sel_b);
    return GGCN_OK;
}

// the same for the one-launch entries, which hand the kernels' DropSpec on (p = 0: thr = 0, nothing is dropped)
int entry_drop_spec(const char *who, float p, uint64_t seed, int sel_store, int sel_a, int sel_b, DropSpec &d)
{
    if (int rc = drop_entry_checks(who, p, sel_store, sel_a, sel_b)) return rc;
    d = make_drop_spec(p, seed, sel_store, sel_a, sel_b);
    return GGCN_OK;
}

// what the one-launch layer entries check before their arguments narrow into a LayerPart (its ldo is an int)
int layer_entry_checks(const char *who, const float *out, int64_t ldo, const float *overlap_in, const float *overlap_out)
{
    if ((overlap_in == nullptr) != (overlap_out == nullptr)) return fail(GGCN_EINVAL, "%s: overlap_in and overlap_out go together", who);
    if (out && ldo > (int64_t)INT32_MAX) return fail(GGCN_EUNSUPPORTED, "%s: ldo too large", who);
    return GGCN_OK;
}

// the same for the three blocks' two outputs
int block_entry_checks(const char *who, const float *gcn1, int64_t ld1, const float *x_out, int64_t ld2)
{
    if ((gcn1 && ld1 > (int64_t)INT32_MAX) || (x_out && ld2 > (int64_t)INT32_MAX))
        return fail(GGCN_EUNSUPPORTED, "%s: leading dimension too large", who);
    return GGCN_OK;
}

const char *bytes(const void *p) { return static_cast<const char *>(p); }

// the preamble of the four ggcn_linear* entries (`null_operand`: one of the pointers that entry needs is NULL)
int linear_entry_checks(const char *who, bool null_operand, int64_t M, int K, int F, int64_t ldx, int64_t ldy)
{
    if (null_operand) return fail(GGCN_EINVAL, "%s: null pointer", who);
    if (M <= 0 || K <= 0 || F <= 0) return fail(GGCN_EINVAL, "%s: M=%lld K=%d F=%d must be positive", who, (long long)M, K, F);
    if (ldx < K || ldy < F) return fail(GGCN_EINVAL, "%s: leading dimension too small", who);
    return GGCN_OK;
}
}  // namespace

extern "C" {

int ggcn_abi_version(void) { return GGCN_ABI_VERSION; }

int ggcn_has_f16mx6(void)
{
#ifdef GGCN_WITH_F16MX6
    return 1;
#else
    return 0;
#endif
}

const char *ggcn_last_error(void) { return error_buffer(); }

size_t ggcn_graph_operands_bytes(int B) { return B > 0 ? (size_t)B * GGCN_GRAPH_OPS_BYTES : 0; }
size_t ggcn_graph_operands2_bytes(int B) { return B > 0 ? (size_t)B * GGCN_GRAPH_OPS2_BYTES : 0; }
size_t ggcn_graph_edge_lists_bytes(int B) { return B > 0 ? (size_t)B * GGCN_EDGE_LISTS_BYTES : 0; }

int ggcn_layer_fused(const float *X, int64_t ldx, const void *wpack, const uint32_t *rowmask, const void *graph_ops,
                     const float *bias, int B, int T, int K, int F, const float *store_gate,
                     const float *pool_gate_a, const float *pool_gate_b, float *out, int64_t ldo,
                     float *pool_a, float *pool_b, float *overlap_partial, const float *overlap_in,
                     float *overlap_out, int precision, ggcn_stream_t stream)
{
    const char *who = "ggcn_layer_fused";
    if (int rc = layer_entry_checks(who, out, ldo, overlap_in, overlap_out)) return rc;
    FusedArgs a = {};
    a.X = X; a.ldx = ldx; a.rowmask = rowmask; a.graph_ops = bytes(graph_ops);
    a.ov_in = overlap_in; a.ov_out = overlap_out;
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 1;
    LayerPart &l = a.part[0];
    l.wpack = bytes(wpack); l.bias = bias; l.store_gate = store_gate; l.pool_gate_a = pool_gate_a; l.pool_gate_b = pool_gate_b;
    l.out = out; l.ldo = (int)ldo; l.pool_a = pool_a; l.pool_b = pool_b; l.ov_partial = overlap_partial;
    return launch_fused(who, a, precision, as_stream(stream));
}

int ggcn_layer_fused_prebias(const float *X, int64_t ldx, const void *wpack, const uint32_t *rowmask, const float *bias,
                             const float *bias_pre, int B, int T, int K, int F, const float *store_gate,
                             const float *pool_gate_a, const float *pool_gate_b, float *out, int64_t ldo,
                             float *pool_a, float *pool_b, int precision, ggcn_stream_t stream)
{
    if (!bias_pre) return fail(GGCN_EINVAL, "ggcn_layer_fused_prebias: null bias_pre (ggcn_layer_fused is the plain form)");
    const char *who = "ggcn_layer_fused";   // (what this entry's shared refusals have always been reported as)
    if (int rc = layer_entry_checks(who, out, ldo, nullptr, nullptr)) return rc;
    if (T <= 32)
        return fail(GGCN_EUNSUPPORTED, "ggcn_layer_fused_prebias: graphs of <= 32 nodes fold both layers in ggcn_block_fused (its eval form); bias_pre is for 33..256 nodes");
    FusedArgs a = {};
    a.X = X; a.ldx = ldx; a.rowmask = rowmask;
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 1;
    LayerPart &l = a.part[0];
    l.wpack = bytes(wpack); l.bias = bias; l.pre = bias_pre; l.store_gate = store_gate; l.pool_gate_a = pool_gate_a; l.pool_gate_b = pool_gate_b;
    l.out = out; l.ldo = (int)ldo; l.pool_a = pool_a; l.pool_b = pool_b;
    return launch_fused(who, a, precision, as_stream(stream));
}

int ggcn_layer_fused_weighted(const float *X, int64_t ldx, const void *wpack, const void *graph_opsw, const float *bias,
                              const float *zero_mid, int B, int T, int K, int F, const float *store_gate,
                              const float *pool_gate_a, const float *pool_gate_b, float *out, int64_t ldo, float *pool_a,
                              float *pool_b, float *overlap_partial, const float *overlap_in, float *overlap_out, int precision,
                              ggcn_stream_t stream)
{
    // gcn.py:30-45 with a real-valued adjacency for graphs of <= 32 nodes in ONE launch: the W12 column tiles' form of the block
    // (MID epilogue: one split of `hidden`, 6 MFMAs with the hi / lo operand) on ggcn_graph_operands_weighted blocks; zero_mid is the
    // all-zero `mid` row that form reads ([F] floats)
    const char *who = "ggcn_layer_fused_weighted";
    if (!graph_opsw || !zero_mid) return fail(GGCN_EINVAL, "%s: the weighted operand blocks and the zero row are required", who);
    if (T > 32) return fail(GGCN_EUNSUPPORTED, "%s: T=%d > 32 (use ggcn_linear + ggcn_aggregate)", who, T);
    if (precision == GGCN_PREC_F16MX6) return fail(GGCN_EUNSUPPORTED, "%s: bf16x3 or f16mx8", who);
    if (int rc = layer_entry_checks(who, out, ldo, overlap_in, overlap_out)) return rc;
    FusedArgs a = {};
    a.X = X; a.ldx = ldx; a.graph_ops = bytes(graph_opsw); a.graph_ops2 = a.graph_ops;
    a.ov_in = overlap_in; a.ov_out = overlap_out;
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 1;
    LayerPart &l = a.part[0];
    l.wpack = bytes(wpack); l.bias = bias; l.mid = zero_mid; l.store_gate = store_gate; l.pool_gate_a = pool_gate_a; l.pool_gate_b = pool_gate_b;
    l.out = out; l.ldo = (int)ldo; l.pool_a = pool_a; l.pool_b = pool_b; l.ov_partial = overlap_partial;
    return launch_fused(who, a, precision, as_stream(stream));
}

int ggcn_layer_fused_weighted_wide(const float *X, int64_t ldx, const void *wpack, const void *graph_opsww, const float *bias,
                                   int B, int T, int K, int F, const float *store_gate, const float *pool_gate_a,
                                   const float *pool_gate_b, float *out, int64_t ldo, float *pool_a, float *pool_b, int precision,
                                   ggcn_stream_t stream)
{
    const char *who = "ggcn_layer_fused_weighted_wide";
    FusedArgs a = {};
    // (LayerPart's ldo is an int)
    if (out && ldo > (int64_t)INT32_MAX) return fail(GGCN_EUNSUPPORTED, "%s: T*ldo does not fit 32-bit offsets", who);
    a.X = X; a.ldx = ldx; a.graph_ops = bytes(graph_opsww);
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 1;
    LayerPart &l = a.part[0];
    l.wpack = bytes(wpack); l.bias = bias; l.store_gate = store_gate; l.pool_gate_a = pool_gate_a; l.pool_gate_b = pool_gate_b;
    l.out = out; l.ldo = (int)ldo; l.pool_a = pool_a; l.pool_b = pool_b;
    return launch_fused_weighted_wide(who, a, precision, as_stream(stream));
}

int ggcn_layer_fused_weighted_drop(const float *X, int64_t ldx, const void *wpack, const void *graph_opsw, const float *bias,
                                   const float *zero_mid, int B, int T, int K, int F, const float *store_gate,
                                   const float *pool_gate_a, const float *pool_gate_b, float *out, int64_t ldo, float *pool_a,
                                   float *pool_b, int precision, float p, uint64_t seed, int sel_store, int sel_a, int sel_b,
                                   ggcn_stream_t stream)
{
    // ggcn_layer_fused_weighted under the gates' training-mode dropout: layer_fused_weighted_drop_kernel on the same blocks; thr = 0
    // (p = 0) launches layer_fused_kernel's MID form -- ggcn_layer_fused_weighted's launch, bit for bit
    const char *who = "ggcn_layer_fused_weighted_drop";
    FusedArgs a = {};
    if (int rc = entry_drop_spec(who, p, seed, sel_store, sel_a, sel_b, a.drop)) return rc;
    if (!graph_opsw || !zero_mid) return fail(GGCN_EINVAL, "%s: the weighted operand blocks and the zero row are required", who);
    if (T > 32) return fail(GGCN_EUNSUPPORTED, "%s: T=%d > 32 (33..128 nodes: ggcn_layer_fused_weighted_wide_drop)", who, T);
    if (precision == GGCN_PREC_F16MX6) return fail(GGCN_EUNSUPPORTED, "%s: bf16x3 or f16mx8", who);
    if ((int64_t)B * T * F >= ((int64_t)1 << 32))   // (whatever p is)
        return fail(GGCN_EUNSUPPORTED, "%s: gate dropout indexes elements with 32 bits (B*T*F = %lld)", who, (long long)B * T * F);
    if (int rc = layer_entry_checks(who, out, ldo, nullptr, nullptr)) return rc;
    a.X = X; a.ldx = ldx; a.graph_ops = bytes(graph_opsw); a.graph_ops2 = a.graph_ops;
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 1;
    LayerPart &l = a.part[0];
    l.wpack = bytes(wpack); l.bias = bias; l.mid = zero_mid; l.store_gate = store_gate; l.pool_gate_a = pool_gate_a; l.pool_gate_b = pool_gate_b;
    l.out = out; l.ldo = (int)ldo; l.pool_a = pool_a; l.pool_b = pool_b;
    return launch_fused(who, a, precision, as_stream(stream));
}

int ggcn_layer_fused_weighted_wide_drop(const float *X, int64_t ldx, const void *wpack, const void *graph_opsww, const float *bias,
                                        int B, int T, int K, int F, const float *store_gate, const float *pool_gate_a,
                                        const float *pool_gate_b, float *out, int64_t ldo, float *pool_a, float *pool_b, int precision,
                                        float p, uint64_t seed, int sel_store, int sel_a, int sel_b, ggcn_stream_t stream)
{
    const char *who = "ggcn_layer_fused_weighted_wide_drop";
    FusedArgs a = {};
    if (int rc = entry_drop_spec(who, p, seed, sel_store, sel_a, sel_b, a.drop)) return rc;
    if ((int64_t)B * T * F >= ((int64_t)1 << 32))   // (whatever p is)
        return fail(GGCN_EUNSUPPORTED, "%s: gate dropout indexes elements with 32 bits (B*T*F = %lld)", who, (long long)B * T * F);
    // (LayerPart's ldo is an int)
    if (out && ldo > (int64_t)INT32_MAX) return fail(GGCN_EUNSUPPORTED, "%s: T*ldo does not fit 32-bit offsets", who);
    a.X = X; a.ldx = ldx; a.graph_ops = bytes(graph_opsww);
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 1;
    LayerPart &l = a.part[0];
    l.wpack = bytes(wpack); l.bias = bias; l.store_gate = store_gate; l.pool_gate_a = pool_gate_a; l.pool_gate_b = pool_gate_b;
    l.out = out; l.ldo = (int)ldo; l.pool_a = pool_a; l.pool_b = pool_b;
    return launch_fused_weighted_wide(who, a, precision, as_stream(stream));
}

int ggcn_gate_pool_backward_weighted_drop(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                                          const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb,
                                          const void *graph_ops_wt, const float *inv, int B, int T, int F, float *dH, int64_t ldh,
                                          float *dY, int64_t ldy, float *d_sg, float *d_ga, float *d_gb, float *d_bsum, float p,
                                          uint64_t seed, int sel_store, int sel_a, int sel_b, ggcn_stream_t stream)
{
    if (int rc = drop_entry_checks("ggcn_gate_pool_backward_weighted_drop", p, sel_store, sel_a, sel_b)) return rc;
    const DropSpec d = make_drop_spec(p, seed, sel_store, sel_a, sel_b);   // p = 0: thr = 0, the kernel without dropout
    return gate_pool_backward_weighted(out, ldo, store_gate, gate_a, gate_b, d_out, ldd, d_pa, d_pb, graph_ops_wt, inv, B, T, F, dH, ldh,
                                       dY, ldy, d_sg, d_ga, d_gb, d_bsum, as_stream(stream), &d);
}

int ggcn_block_fused(const float *X, int64_t ldx, const void *wpack1, const void *wpack12, const void *graph_ops,
                     const void *graph_ops2, const float *bias1, const float *bias_mid, const float *bias2, int B, int T, int K, int F,
                     const float *gate1, const float *gate2, float *gcn1, int64_t ld1, float *x_out, int64_t ld2,
                     float *x1, float *y1, float *pool_out, float *overlap_partial, int precision,
                     ggcn_stream_t stream)
{
    const char *who = "ggcn_block_fused";
    if (int rc = block_entry_checks(who, gcn1, ld1, x_out, ld2)) return rc;
    FusedArgs a = {};
    a.X = X; a.ldx = ldx; a.graph_ops = bytes(graph_ops); a.graph_ops2 = bytes(graph_ops2);
    // bert_amir5.py:626-636: gcn1 (ungated; optional here), x1 = max_t gcn1*gate1, y1 = max_t gcn1*gate2 in part[0];
    // bert_amir5.py:639-640: x = gate2 * gc2(gcn1), out = max_t x in part[1] (the other block entries describe theirs alike)
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 2;
    LayerPart &l1 = a.part[0], &l2 = a.part[1];
    l1.wpack = bytes(wpack1); l1.bias = bias1; l1.pool_gate_a = gate1; l1.pool_gate_b = gate2;
    l1.out = gcn1; l1.ldo = (int)ld1; l1.pool_a = x1; l1.pool_b = y1; l1.ov_partial = overlap_partial;
    l2.wpack = bytes(wpack12); l2.bias = bias2; l2.mid = bias_mid; l2.store_gate = gate2; l2.pool_gate_a = gate2;
    l2.out = x_out; l2.ldo = (int)ld2; l2.pool_a = pool_out;
    return launch_block(who, a, kBlockBinary, precision, as_stream(stream));
}

int ggcn_block_fused_weighted(const float *X, int64_t ldx, const void *wpack1, const void *wpack12, const void *graph_opsw,
                              const void *graph_ops2w, const float *bias1, const float *bias_mid, const float *bias2,
                              const float *zero_mid, int B, int T, int K, int F, const float *gate1, const float *gate2, float *gcn1,
                              int64_t ld1, float *x_out, int64_t ld2, float *x1, float *y1, float *pool_out, float *overlap_partial,
                              int precision, ggcn_stream_t stream)
{
    // ggcn_block_fused on a REAL-valued adjacency: layer 1's tiles apply M = D.A_w (ggcn_graph_operands_weighted blocks) with the zero
    // `mid` row, layer 2's tiles M2 = (D.A_w)^2 (ggcn_graph_operands2_weighted blocks) with bias_mid, both through the MID epilogue
    // (block_fused_weighted_kernel, fused_weighted_drop.hip).  Never the eight-wavefront kernel: fused_block8.hip reads the 0/1 format.
    const char *who = "ggcn_block_fused_weighted";
    if (int rc = block_entry_checks(who, gcn1, ld1, x_out, ld2)) return rc;
    FusedArgs a = {};
    a.X = X; a.ldx = ldx; a.graph_ops = bytes(graph_opsw); a.graph_ops2 = bytes(graph_ops2w);
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 2;
    LayerPart &l1 = a.part[0], &l2 = a.part[1];
    l1.wpack = bytes(wpack1); l1.bias = bias1; l1.mid = zero_mid; l1.pool_gate_a = gate1; l1.pool_gate_b = gate2;
    l1.out = gcn1; l1.ldo = (int)ld1; l1.pool_a = x1; l1.pool_b = y1; l1.ov_partial = overlap_partial;
    l2.wpack = bytes(wpack12); l2.bias = bias2; l2.mid = bias_mid; l2.store_gate = gate2; l2.pool_gate_a = gate2;
    l2.out = x_out; l2.ldo = (int)ld2; l2.pool_a = pool_out;
    return launch_block(who, a, kBlockWeighted, precision, as_stream(stream));
}

int ggcn_linear(const float *X, int64_t ldx, const float *W, int64_t ldw, const void *wpack, float *Y,
                int64_t ldy, int64_t M, int K, int F, int precision, ggcn_stream_t stream)
{
    if (int rc = linear_entry_checks("ggcn_linear", !X || !Y, M, K, F, ldx, ldy)) return rc;
    switch (precision) {
        case GGCN_PREC_BF16X3:
        case GGCN_PREC_F16MX8:
            return linear_packed(X, ldx, wpack, Y, ldy, M, K, F, precision, as_stream(stream));
        case GGCN_PREC_FP32:
            if (!W) return fail(GGCN_EINVAL, "ggcn_linear(fp32): W is NULL");
            if (ldw < F) return fail(GGCN_EINVAL, "ggcn_linear(fp32): ldw < F");
            return linear_fp32(X, ldx, W, ldw, Y, ldy, M, K, F, as_stream(stream));
        default:
            return fail(GGCN_EINVAL, "ggcn_linear: unknown precision %d", precision);
    }
}

int ggcn_linear_bf16(const void *X, int64_t ldx, const void *wpack, float *Y, int64_t ldy, int64_t M, int K, int F,
                     ggcn_stream_t stream)
{
    if (int rc = linear_entry_checks("ggcn_linear_bf16", !X || !Y || !wpack, M, K, F, ldx, ldy)) return rc;
    if (reinterpret_cast<uintptr_t>(X) % 2 || reinterpret_cast<uintptr_t>(Y) % 4)
        return fail(GGCN_EINVAL, "ggcn_linear_bf16: X / Y not aligned to their element size");
    return linear_bf16(X, ldx, wpack, Y, ldy, M, K, F, as_stream(stream));
}

int ggcn_linear_out_bf16(const float *X, int64_t ldx, const void *wpack, void *Y, int64_t ldy, int64_t M, int K, int F,
                         ggcn_stream_t stream)
{
    if (int rc = linear_entry_checks("ggcn_linear_out_bf16", !X || !Y || !wpack, M, K, F, ldx, ldy)) return rc;
    if (reinterpret_cast<uintptr_t>(X) % 4 || reinterpret_cast<uintptr_t>(Y) % 2)
        return fail(GGCN_EINVAL, "ggcn_linear_out_bf16: X / Y not aligned to their element size");
    return linear_out_bf16(X, ldx, wpack, Y, ldy, M, K, F, as_stream(stream));
}

int ggcn_layer_fused_bf16(const void *X, int64_t ldx, const void *wpack, const void *graph_ops, const float *bias, int B, int T,
                          int K, int F, const float *store_gate, const float *pool_gate_a, const float *pool_gate_b, float *out,
                          int64_t ldo, float *pool_a, float *pool_b, float *overlap_partial, const float *overlap_in,
                          float *overlap_out, ggcn_stream_t stream)
{
    const char *who = "ggcn_layer_fused_bf16";
    if (X && reinterpret_cast<uintptr_t>(X) % 2) return fail(GGCN_EINVAL, "%s: X not 2-byte aligned", who);
    if (T > 32) return fail(GGCN_EUNSUPPORTED, "%s: T=%d > 32 (use ggcn_layer_fused_bf16_wide up to %d nodes, ggcn_linear_bf16 + ggcn_aggregate beyond)", who, T, GGCN_MASK_MAX_T);
    FusedArgs a = {};
    if (!X) return fail(GGCN_EINVAL, "%s: null input pointer", who);   // (launch_fused sees the weight image in a.X)
    if (int rc = layer_entry_checks(who, out, ldo, overlap_in, overlap_out)) return rc;
    // a.X stays the fallback READ address for an absent gate / bias (the epilogues load unconditionally and discard the
    // value): it must be valid memory, and the weight image always is (>= 4 KiB; its NULL case is refused before the launch)
    a.X = static_cast<const float *>(wpack);
    a.Xb = static_cast<const __bf16 *>(X); a.ldx = ldx; a.graph_ops = bytes(graph_ops);
    a.ov_in = overlap_in; a.ov_out = overlap_out;
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 1;
    LayerPart &l = a.part[0];
    l.wpack = bytes(wpack); l.bias = bias; l.store_gate = store_gate; l.pool_gate_a = pool_gate_a; l.pool_gate_b = pool_gate_b;
    l.out = out; l.ldo = (int)ldo; l.pool_a = pool_a; l.pool_b = pool_b; l.ov_partial = overlap_partial;
    return launch_fused(who, a, GGCN_PREC_BF16X3, as_stream(stream));
}

int ggcn_layer_fused_bf16_drop(const void *X, int64_t ldx, const void *wpack, const void *graph_ops, const float *bias, int B, int T,
                               int K, int F, const float *store_gate, const float *pool_gate_a, const float *pool_gate_b, float *out,
                               int64_t ldo, float *pool_a, float *pool_b, float *overlap_partial, const float *overlap_in,
                               float *overlap_out, float p, uint64_t seed, int sel_store, int sel_a, int sel_b, ggcn_stream_t stream)
{
    const char *who = "ggcn_layer_fused_bf16_drop";
    FusedArgs a = {};
    if (X && reinterpret_cast<uintptr_t>(X) % 2) return fail(GGCN_EINVAL, "%s: X not 2-byte aligned", who);
    if (int rc = entry_drop_spec(who, p, seed, sel_store, sel_a, sel_b, a.drop)) return rc;
    if (T > 32) return fail(GGCN_EUNSUPPORTED, "%s: T=%d > 32 (use ggcn_layer_fused_bf16_wide up to %d nodes)", who, T, GGCN_MASK_MAX_T);
    if (!X) return fail(GGCN_EINVAL, "%s: null input pointer", who);   // (launch_fused sees the weight image in a.X)
    if (int rc = layer_entry_checks(who, out, ldo, overlap_in, overlap_out)) return rc;
    a.X = static_cast<const float *>(wpack);   // (the fallback read address: ggcn_layer_fused_bf16)
    a.Xb = static_cast<const __bf16 *>(X); a.ldx = ldx; a.graph_ops = bytes(graph_ops);
    a.ov_in = overlap_in; a.ov_out = overlap_out;
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 1;
    LayerPart &l = a.part[0];
    l.wpack = bytes(wpack); l.bias = bias; l.store_gate = store_gate; l.pool_gate_a = pool_gate_a; l.pool_gate_b = pool_gate_b;
    l.out = out; l.ldo = (int)ldo; l.pool_a = pool_a; l.pool_b = pool_b; l.ov_partial = overlap_partial;
    return launch_fused(who, a, GGCN_PREC_BF16X3, as_stream(stream));
}

int ggcn_layer_fused_bf16_wide(const void *X, int64_t ldx, const void *wpack, const uint32_t *rowmask, const void *edge_lists,
                               const float *bias, int B, int T, int K, int F, const float *store_gate, const float *pool_gate_a,
                               const float *pool_gate_b, float *out, int64_t ldo, float *pool_a, float *pool_b, float *overlap_partial,
                               const float *overlap_in, float *overlap_out, float p, uint64_t seed, int sel_store, int sel_a, int sel_b,
                               ggcn_stream_t stream)
{
    const char *who = "ggcn_layer_fused_bf16_wide";
    FusedArgs a = {};
    if (X && reinterpret_cast<uintptr_t>(X) % 2) return fail(GGCN_EINVAL, "%s: X not 2-byte aligned", who);
    if (int rc = entry_drop_spec(who, p, seed, sel_store, sel_a, sel_b, a.drop)) return rc;
    if (T <= 32) return fail(GGCN_EUNSUPPORTED, "%s: T=%d <= 32 (use ggcn_layer_fused_bf16 / ggcn_layer_fused_bf16_drop)", who, T);
    if (T > GGCN_MASK_MAX_T) return fail(GGCN_EUNSUPPORTED, "%s: T=%d > %d (use ggcn_linear_bf16 + ggcn_aggregate)", who, T, GGCN_MASK_MAX_T);
    if (!X) return fail(GGCN_EINVAL, "%s: null input pointer", who);   // (launch_fused sees the weight image in a.X)
    if (int rc = layer_entry_checks(who, out, ldo, overlap_in, overlap_out)) return rc;
    a.X = static_cast<const float *>(wpack);   // (the fallback read address: ggcn_layer_fused_bf16)
    a.Xb = static_cast<const __bf16 *>(X); a.ldx = ldx; a.rowmask = rowmask; a.graph_ops = T > 128 ? bytes(edge_lists) : nullptr;
    a.ov_in = overlap_in; a.ov_out = overlap_out;
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 1;
    LayerPart &l = a.part[0];
    l.wpack = bytes(wpack); l.bias = bias; l.store_gate = store_gate; l.pool_gate_a = pool_gate_a; l.pool_gate_b = pool_gate_b;
    l.out = out; l.ldo = (int)ldo; l.pool_a = pool_a; l.pool_b = pool_b; l.ov_partial = overlap_partial;
    return launch_fused(who, a, GGCN_PREC_BF16X3, as_stream(stream));
}

int ggcn_block_fused_bf16(const void *X, int64_t ldx, const void *wpack1, const void *wpack12, const void *graph_ops,
                          const void *graph_ops2, const float *bias1, const float *bias_mid, const float *bias2, int B, int T, int K,
                          int F, const float *gate1, const float *gate2, float *gcn1, int64_t ld1, float *x_out, int64_t ld2,
                          float *x1, float *y1, float *pool_out, float *overlap_partial, ggcn_stream_t stream)
{
    // ggcn_block_fused on bf16 features: the bf16 pair main loop on the bf16x3 images of W1 and W12, bf16 planes of (D.A)^2
    // (ggcn_graph_operands2 plane 0)
    const char *who = "ggcn_block_fused_bf16";
    if (X && reinterpret_cast<uintptr_t>(X) % 2) return fail(GGCN_EINVAL, "%s: X not 2-byte aligned", who);
    if (!X) return fail(GGCN_EINVAL, "%s: null input pointer", who);   // (launch_fused sees the weight image in a.X)
    if (int rc = block_entry_checks(who, gcn1, ld1, x_out, ld2)) return rc;
    FusedArgs a = {};
    a.X = static_cast<const float *>(wpack12);   // (the fallback read address: ggcn_layer_fused_bf16)
    a.Xb = static_cast<const __bf16 *>(X); a.ldx = ldx; a.graph_ops = bytes(graph_ops); a.graph_ops2 = bytes(graph_ops2);
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 2;
    LayerPart &l1 = a.part[0], &l2 = a.part[1];
    l1.wpack = bytes(wpack1); l1.bias = bias1; l1.pool_gate_a = gate1; l1.pool_gate_b = gate2;
    l1.out = gcn1; l1.ldo = (int)ld1; l1.pool_a = x1; l1.pool_b = y1; l1.ov_partial = overlap_partial;
    l2.wpack = bytes(wpack12); l2.bias = bias2; l2.mid = bias_mid; l2.store_gate = gate2; l2.pool_gate_a = gate2;
    l2.out = x_out; l2.ldo = (int)ld2; l2.pool_a = pool_out;
    return launch_block(who, a, kBlockBf16, GGCN_PREC_BF16X3, as_stream(stream));
}

int ggcn_linear_h(const void *X, int64_t ldx, const void *wpack, void *Y, int64_t ldy, int64_t M, int K, int F,
                  int precision, ggcn_stream_t stream)
{
    if (precision != GGCN_PREC_BF16X3 && precision != GGCN_PREC_F16MX8 && precision != GGCN_PREC_F16)
        return fail(GGCN_EUNSUPPORTED, "ggcn_linear_h: precision %d (use bf16x3, f16mx8 or f16)", precision);
    if (int rc = linear_entry_checks("ggcn_linear_h", !X || !Y, M, K, F, ldx, ldy)) return rc;
    return linear_packed_h(X, ldx, wpack, Y, ldy, M, K, F, precision, as_stream(stream));
}

int ggcn_gate_pool_backward(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                            const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa,
                            const float *d_pb, int B, int T, int F, float *dY, int64_t ldy, float *d_sg,
                            float *d_ga, float *d_gb, float *d_bsum, ggcn_stream_t stream)
{
    return gate_pool_backward(out, ldo, store_gate, gate_a, gate_b, d_out, ldd, d_pa, d_pb, B, T, F, dY, ldy, d_sg,
                              d_ga, d_gb, d_bsum, as_stream(stream));
}

int ggcn_gate_pool_backward_drop(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                                 const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa,
                                 const float *d_pb, int B, int T, int F, float *dY, int64_t ldy, float *d_sg,
                                 float *d_ga, float *d_gb, float *d_bsum, float p, uint64_t seed, int sel_store,
                                 int sel_a, int sel_b, ggcn_stream_t stream)
{
    if (int rc = drop_entry_checks("ggcn_gate_pool_backward_drop", p, sel_store, sel_a, sel_b)) return rc;
    const DropSpec d = make_drop_spec(p, seed, sel_store, sel_a, sel_b);
    return gate_pool_backward(out, ldo, store_gate, gate_a, gate_b, d_out, ldd, d_pa, d_pb, B, T, F, dY, ldy, d_sg,
                              d_ga, d_gb, d_bsum, as_stream(stream), &d);
}

int ggcn_gate_pool_backward_agg(const float *out, int64_t ldo, const float *store_gate, const float *gate_a,
                                const float *gate_b, const float *d_out, int64_t ldd, const float *d_pa,
                                const float *d_pb, const uint32_t *rowmask, int B, int T, int F, float *dH, int64_t ldh,
                                float *d_sg, float *d_ga, float *d_gb, float *d_bsum, float p, uint64_t seed, int sel_store,
                                int sel_a, int sel_b, float *dh_amax, ggcn_stream_t stream)
{
    if (int rc = drop_entry_checks("ggcn_gate_pool_backward_agg", p, sel_store, sel_a, sel_b)) return rc;
    const DropSpec d = make_drop_spec(p, seed, sel_store, sel_a, sel_b);
    return gate_pool_backward_agg(out, ldo, store_gate, gate_a, gate_b, d_out, ldd, d_pa, d_pb, rowmask, B, T, F, dH, ldh, d_sg,
                                  d_ga, d_gb, d_bsum, as_stream(stream), p > 0.0f ? &d : nullptr, dh_amax);
}

int ggcn_block_fused_form(int B, int T, int K, int F)
{
    const char *form = getenv("GGCN_BLOCK_FORM");
    return (block8_shape(B, T, K, F) && !(form && form[0] == '4')) ? 8 : 4;
}

int ggcn_linear_form(int entry, const void *X, int64_t ldx, const void *W, int64_t ldw, const void *Y, int64_t ldy, int64_t M, int K,
                     int F, int precision)
{
    // the checks of the entry itself in the entry's order, then the launcher's own form function (common.h); no launch, no dereference
    const char *who = "ggcn_linear_form";
    const uintptr_t xa = reinterpret_cast<uintptr_t>(X), ya = reinterpret_cast<uintptr_t>(Y);
    auto split = [&](int x_bytes, bool y_f32) -> int {
        if (linear_split_grid(M, F) > (int64_t)INT32_MAX) return -fail(GGCN_EUNSUPPORTED, "%s: M too large", who);
        return linear_split_form(x_bytes, y_f32, X, ldx, Y, ldy, K, F);
    };
    switch (entry) {
        case GGCN_ENTRY_LINEAR:
            if (int rc = linear_entry_checks(who, !X || !Y, M, K, F, ldx, ldy)) return -rc;
            if (precision == GGCN_PREC_BF16X3 || precision == GGCN_PREC_F16MX8) return split(4, true);
            if (precision != GGCN_PREC_FP32) return -fail(GGCN_EINVAL, "%s: ggcn_linear has no precision %d", who, precision);
            if (!W) return -fail(GGCN_EINVAL, "%s: ggcn_linear(fp32): W is NULL", who);
            if (ldw < F) return -fail(GGCN_EINVAL, "%s: ggcn_linear(fp32): ldw < F", who);
            return linear_fp32_form(X, ldx, W, ldw, K, F);
        case GGCN_ENTRY_LINEAR_H:
            if (precision != GGCN_PREC_BF16X3 && precision != GGCN_PREC_F16MX8 && precision != GGCN_PREC_F16)
                return -fail(GGCN_EUNSUPPORTED, "%s: ggcn_linear_h has no precision %d", who, precision);
            if (int rc = linear_entry_checks(who, !X || !Y, M, K, F, ldx, ldy)) return -rc;
            if (precision != GGCN_PREC_F16) return split(2, false);
            if (linear_split_grid(M, F) > (int64_t)INT32_MAX) return -fail(GGCN_EUNSUPPORTED, "%s: M too large", who);
            return linear_f16_form(X, ldx, K);
        case GGCN_ENTRY_LINEAR_BF16:
        case GGCN_ENTRY_LINEAR_OUT_BF16: {
            const bool out = entry == GGCN_ENTRY_LINEAR_OUT_BF16;   // fp32 X -> bf16 Y; otherwise bf16 X -> fp32 Y
            if (int rc = linear_entry_checks(who, !X || !Y, M, K, F, ldx, ldy)) return -rc;
            if (xa % (out ? 4 : 2) || ya % (out ? 2 : 4)) return -fail(GGCN_EINVAL, "%s: X / Y not aligned to their element size", who);
            return split(out ? 4 : 2, !out);
        }
        case GGCN_ENTRY_LINEAR_SCALED:
            if (!X || !Y) return -fail(GGCN_EINVAL, "%s: null pointer", who);
            if (M <= 0 || K <= 0 || F <= 0 || ldx < K || ldy < F) return -fail(GGCN_EINVAL, "%s: M=%lld K=%d F=%d", who, (long long)M, K, F);
            if (!linear_scaled_takes(static_cast<const float *>(X), ldx, static_cast<const float *>(Y), ldy, K, F))
                return -fail(GGCN_EUNSUPPORTED, "%s: ggcn_linear_scaled needs K %% 32 == 0, F %% 4 == 0 and 16-byte aligned rows", who);
            return split(4, true);
        default:
            return -fail(GGCN_EINVAL, "%s: unknown entry %d", who, entry);
    }
}

int ggcn_lab_block_fused8(const float *X, int64_t ldx, const void *wpack1, const void *wpack12, const void *graph_ops,
                          const void *graph_ops2, const float *bias1, const float *bias_mid, const float *bias2, int B, int T, int K, int F,
                          const float *gate1, const float *gate2, float *x_out, int64_t ld2, float *x1, float *y1, float *pool_out,
                          float *overlap_partial, uint64_t *stamps, ggcn_stream_t stream)
{
    const int flags = (getenv("GGCN_LAB_BLOCK8_ROWMAJOR") ? kBlock8RowMajor : 0) | (getenv("GGCN_LAB_BLOCK8_NODMA") ? kBlock8NoDma : 0) |
                      (getenv("GGCN_LAB_BLOCK8_SAMESLOTS") ? kBlock8SameSlots : 0) |
                      (getenv("GGCN_LAB_BLOCK8_PRIO") ? kBlock8Prio : 0);   // (the experiment's switches, read per call)
    FusedArgs a = {};
    a.X = X; a.ldx = ldx; a.graph_ops = bytes(graph_ops); a.graph_ops2 = bytes(graph_ops2);
    a.stamps = reinterpret_cast<unsigned long long *>(stamps);
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 2;
    LayerPart &l1 = a.part[0], &l2 = a.part[1];
    l1.wpack = bytes(wpack1); l1.bias = bias1; l1.pool_gate_a = gate1; l1.pool_gate_b = gate2;
    l1.pool_a = x1; l1.pool_b = y1; l1.ov_partial = overlap_partial;
    l2.wpack = bytes(wpack12); l2.bias = bias2; l2.mid = bias_mid; l2.store_gate = gate2; l2.pool_gate_a = gate2;
    // (a leading dimension that does not fit LayerPart's int stays one that block_fused8 refuses: too small below 0, no row stores beyond)
    l2.out = x_out; l2.ldo = (int)(ld2 < 0 ? -1 : ld2 > (int64_t)INT32_MAX ? (int64_t)INT32_MAX : ld2); l2.pool_a = pool_out;
    return block_fused8("ggcn_lab_block_fused8", a, flags, as_stream(stream));
}

int ggcn_gate_pool_backward_weighted(const float *out, int64_t ldo, const float *store_gate, const float *gate_a, const float *gate_b,
                                     const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb, const void *graph_ops_wt,
                                     const float *inv, int B, int T, int F, float *dH, int64_t ldh, float *dY, int64_t ldy, float *d_sg,
                                     float *d_ga, float *d_gb, float *d_bsum, ggcn_stream_t stream)
{
    return gate_pool_backward_weighted(out, ldo, store_gate, gate_a, gate_b, d_out, ldd, d_pa, d_pb, graph_ops_wt, inv, B, T, F, dH, ldh,
                                       dY, ldy, d_sg, d_ga, d_gb, d_bsum, as_stream(stream));
}

int ggcn_layer_fused_drop(const float *X, int64_t ldx, const void *wpack, const uint32_t *rowmask, const void *graph_ops,
                          const float *bias, int B, int T, int K, int F, const float *store_gate,
                          const float *pool_gate_a, const float *pool_gate_b, float *out, int64_t ldo,
                          float *pool_a, float *pool_b, int precision, float p, uint64_t seed, int sel_store,
                          int sel_a, int sel_b, ggcn_stream_t stream)
{
    const char *who = "ggcn_layer_fused";   // (what this entry's shared refusals have always been reported as)
    FusedArgs a = {};
    if (int rc = entry_drop_spec("ggcn_layer_fused_drop", p, seed, sel_store, sel_a, sel_b, a.drop)) return rc;
    if (int rc = layer_entry_checks(who, out, ldo, nullptr, nullptr)) return rc;
    a.X = X; a.ldx = ldx; a.rowmask = rowmask; a.graph_ops = bytes(graph_ops);
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 1;
    LayerPart &l = a.part[0];
    l.wpack = bytes(wpack); l.bias = bias; l.store_gate = store_gate; l.pool_gate_a = pool_gate_a; l.pool_gate_b = pool_gate_b;
    l.out = out; l.ldo = (int)ldo; l.pool_a = pool_a; l.pool_b = pool_b;
    return launch_fused(who, a, precision, as_stream(stream));
}

size_t ggcn_dweight_workspace_bytes(int64_t n_rows, int K, int F, int precision)
{
    return precision == GGCN_PREC_FP32 ? dweight_workspace_bytes(n_rows, K, F) : dweight_bx3_workspace_bytes(n_rows, K, F);
}

int ggcn_dweight(const float *X, int64_t ldx, const float *dH, int64_t ldg, int64_t n_rows, int K, int F,
                 float *dW, int64_t lddw, int precision, void *workspace, ggcn_stream_t stream)
{
    if (precision == GGCN_PREC_FP32)
        return dweight(X, ldx, dH, ldg, n_rows, K, F, dW, lddw, workspace, as_stream(stream));
    if (precision != GGCN_PREC_BF16X3)
        return fail(GGCN_EUNSUPPORTED, "ggcn_dweight: precision %d (gradients need fp32 range: use bf16x3 or fp32)", precision);
    return dweight_bx3(X, ldx, dH, ldg, n_rows, K, F, dW, lddw, workspace, as_stream(stream));
}

int ggcn_debug_block_fused_stamped(const float *X, int64_t ldx, const void *wpack1, const void *wpack12, const void *graph_ops,
                                   const void *graph_ops2, const float *bias1, const float *bias_mid, const float *bias2, int B,
                                   int T, int K, int F, const float *gate1, const float *gate2, float *gcn1, int64_t ld1,
                                   float *x_out, int64_t ld2, float *x1, float *y1, float *pool_out, float *overlap_partial,
                                   int precision, uint64_t *stamps, ggcn_stream_t stream)
{
    if (!stamps) return fail(GGCN_EINVAL, "ggcn_debug_block_fused_stamped: null stamp buffer");
    const char *who = "ggcn_block_fused";   // (what this entry's shared refusals have always been reported as)
    if (int rc = block_entry_checks(who, gcn1, ld1, x_out, ld2)) return rc;
    FusedArgs a = {};
    a.X = X; a.ldx = ldx; a.graph_ops = bytes(graph_ops); a.graph_ops2 = bytes(graph_ops2);
    a.stamps = reinterpret_cast<unsigned long long *>(stamps);
    a.B = B; a.T = T; a.K = K; a.F = F; a.n_parts = 2;
    LayerPart &l1 = a.part[0], &l2 = a.part[1];
    l1.wpack = bytes(wpack1); l1.bias = bias1; l1.pool_gate_a = gate1; l1.pool_gate_b = gate2;
    l1.out = gcn1; l1.ldo = (int)ld1; l1.pool_a = x1; l1.pool_b = y1; l1.ov_partial = overlap_partial;
    l2.wpack = bytes(wpack12); l2.bias = bias2; l2.mid = bias_mid; l2.store_gate = gate2; l2.pool_gate_a = gate2;
    l2.out = x_out; l2.ldo = (int)ld2; l2.pool_a = pool_out;
    return launch_block(who, a, kBlockBinary, precision, as_stream(stream));
}

int ggcn_range_flag(uint32_t *flag, int clear, ggcn_stream_t stream)
{
    if (!flag) return fail(GGCN_EINVAL, "ggcn_range_flag: null flag pointer");
    const RangeFlagReaders &r = registered_readers();
    if (r.overflow)
        return fail(GGCN_EINVAL, "ggcn_range_flag: more than %d translation units registered a reader of the range flag (kMaxRangeFlagReaders)",
                    kMaxRangeFlagReaders);
    // one copy of the flag per translation unit that holds an f16mx8 main loop
    int rc = GGCN_OK;
    for (int i = 0; i < r.count && !rc; ++i) rc = r.reader[i](flag, clear, as_stream(stream));
    return rc;
}

int ggcn_dense_head(const float *pooled, int64_t ldp, const float *Wt, int64_t ldw, const float *bias, int B, int H, int C,
                    float *logits, int64_t ldl, const float *overlap_partials, int F_block, float *xy, ggcn_stream_t stream)
{
    return dense_head(pooled, ldp, Wt, ldw, bias, B, H, C, logits, ldl, overlap_partials, F_block, xy, as_stream(stream));
}

int ggcn_dense_head_signal(const float *pooled, int64_t ldp, const float *Wt, int64_t ldw, const float *bias, int B, int H, int C,
                           float *logits, int64_t ldl, const float *overlap_partials, int F_block, float *xy, uint32_t *signal,
                           ggcn_stream_t stream)
{
    if (!signal) return fail(GGCN_EINVAL, "ggcn_dense_head_signal: null signal words (ggcn_dense_head is the plain form)");
    return dense_head(pooled, ldp, Wt, ldw, bias, B, H, C, logits, ldl, overlap_partials, F_block, xy, as_stream(stream), signal);
}

}  // extern "C"
