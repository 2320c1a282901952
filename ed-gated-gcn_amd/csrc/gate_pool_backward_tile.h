// The tile of the one-launch gate / max-pool backward kernels (gate_pool_backward_{mma,weighted,wide,weighted_wide}.hip), written once:
//
//   dY[t] = d_out[t]*sg + [t = argmax_a] d_pa*ga + [t = argmax_b] d_pb*gb         models/bert_amir5.py:627-640 backwards
//   dH    = A^T . D . dY,   D = diag(1 / (rowsum(A) + 1))                           models/gcn.py:35,41 backwards (train.py:120)
//
// ONE workgroup per graph: its rows are one contiguous block of `out`, `d_out`, dH (and dY).  Lane (c, h) = (lane & 31, lane >> 5)
// holds, of column c of a 32-column tile and of every 32-row block, the 16 rows row_of(r, h) -- the accumulator's register -> row map
// of v_mfma_f32_32x32x16_bf16, which is also the k order of the operand blocks (element e of k-step s = register 8 s + e), so what
// a lane loads is what it multiplies.  In the order a kernel uses them:
//   kMaxT, kMaxNB, kStageLd     the wide forms' limits and their staging tile's row pitch
//   column_operands    the gates and pool gradients of the lane's column
//   GraphRows (graph_rows, lane_voff, row_soff)     `out` / `d_out` / dY behind buffer resources that END with the graph's last row
//   Winners, scan_rows, exchange_halves  both pools' winners (first maximum in ascending row order) and d_sg
//   wins_a / wins_b, dy_row     whether a row takes a pool's share; dY of one element, in float
//   rinv_of_block       (wide forms) a source block's 1 / (rowsum + 1) in register order, from the table in LDS
//   split3              D.dY -> three bf16 planes;  mma_01 / GGCN_MMA_PLANES6: the MFMA chains, smallest product first
//   store_column_grads  d_bsum, d_sg, d_ga, d_gb
//   stage64_put / stage64_store (64-column groups, <= 32 nodes), store_block36 (32 x 32 blocks, 33..128 nodes)     dH through LDS
// and on the host backward_entry_checks, the refusals of the four entries.
// A kernel supplies what really differs: how A^T's fragments arrive, its loop structure (one pass, or two over NB row blocks), and
// any element math of its own (gate dropout, a float64 dY, max |dH|).  A helper that would need a flag for one kernel's case does
// not belong here.
#pragma once
#include <initializer_list>

#include "bf16x3_core.h"
#include "common.h"

namespace ggcn {
namespace gpb {

using namespace bx3;

constexpr int kMaxT = 128, kMaxNB = kMaxT / 32;   // the wide forms: 2..4 row blocks
constexpr int kStageLd = 36;   // words per staged row of a 32 x 32 block: 16-byte aligned, and the two lane halves (4 rows apart) miss each other's banks

__device__ __forceinline__ int row_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// x -> three bf16 values, p0 + p1 + p2 = x to 2^-25
__device__ __forceinline__ void planes_of(float x, __bf16 &p0, __bf16 &p1, __bf16 &p2)
{
    p0 = (__bf16)x;
    const float r1 = x - (float)p0;
    p1 = (__bf16)r1;
    p2 = (__bf16)(r1 - (float)p1);
}

// v -> three bf16 planes as B-operand fragments of the two k-steps
__device__ __forceinline__ void split3(const float (&v)[16], bf16x8 (&f)[3][2])
{
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            __bf16 p0, p1, p2;
            planes_of(v[8 * s + e], p0, p1, p2);
            f[0][s][e] = p0;
            f[1][s][e] = p1;
            f[2][s][e] = p2;
        }
}

struct Column {
    bool cok;           // the lane's column exists
    int colc;           // (a lane past F works on column 0's data and stores nothing)
    int64_t gf;         // of the [B, F] operands
    float sg, inv_sg, ga, gb, dpa, dpb;
    bool has_pa, has_pb;
};

__device__ __forceinline__ Column column_operands(int b, int col, int F, const float *store_gate, const float *gate_a, const float *gate_b,
                                                  const float *d_pa, const float *d_pb)
{
    Column k;
    k.cok = col < F;
    k.colc = k.cok ? col : 0;
    k.gf = (int64_t)b * F + k.colc;
    k.sg = store_gate ? store_gate[k.gf] : 1.0f;
    k.inv_sg = store_gate ? (k.sg != 0.0f ? 1.0f / k.sg : 0.0f) : 1.0f;
    k.ga = gate_a ? gate_a[k.gf] : 1.0f, k.gb = gate_b ? gate_b[k.gf] : 1.0f;
    k.dpa = d_pa ? d_pa[k.gf] : 0.0f, k.dpb = d_pb ? d_pb[k.gf] : 0.0f;
    k.has_pa = d_pa != nullptr, k.has_pb = d_pb != nullptr;
    return k;
}

// The rows of graph b of p [B*T, ld] (F columns of them) behind a buffer resource that ENDS with the graph's last row: a lane's rows
// are one lane offset (its column, its half's 4-row shift) + SCALAR row offsets, and rows past T read zeros -- and are not stored
// -- by the hardware's range check: no 64-bit lane arithmetic (32 address pairs cost 64 registers), no select per value.
// p == NULL: an empty resource at `spare` -- every load reads zero.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t graph_rows(const float *p, int64_t ld, int b, int T, int F, const float *spare)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p ? p + (int64_t)b * T * ld : spare), 0,
                                             p ? (int)((((int64_t)T - 1) * ld + F) * 4) : 0, 0x00020000);
}

__device__ __forceinline__ int lane_voff(int h, int64_t ld, int colc) { return (int)((4 * h * ld + colc) * 4); }

__device__ __forceinline__ int row_soff(int blk, int r, int64_t ld) { return (int)((32 * blk + (r & 3) + 8 * (r >> 2)) * ld * 4); }   // (the lane's row is this one + 4 h)

// row 32 blk + row_of(r, h) of the lane's column
__device__ __forceinline__ float load_row(__amdgpu_buffer_rsrc_t rsrc, int voff, int64_t ld, int blk, int r)
{
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, row_soff(blk, r, ld), 0));
}

// The rows of a 32-row block that a lane holds: a graph's `out` and `d_out` behind their resources and lane offsets
struct GraphRows {
    __amdgpu_buffer_rsrc_t orsrc, drsrc;
    int ovoff, dvoff;
    int64_t ldo, ldd;

    __device__ __forceinline__ GraphRows(const float *out, int64_t ldo_, const float *d_out, int64_t ldd_, int b, int T, int F, int h, int colc)
        : orsrc(graph_rows(out, ldo_, b, T, F, out)), drsrc(graph_rows(d_out, ldd_, b, T, F, out)),   // (no d_out: zeros)
          ovoff(lane_voff(h, ldo_, colc)), dvoff(lane_voff(h, ldd_, colc)), ldo(ldo_), ldd(ldd_) {}

    __device__ __forceinline__ void load(int blk, float (&ov)[16], float (&dv)[16]) const
    {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            ov[r] = load_row(orsrc, ovoff, ldo, blk, r);
            dv[r] = load_row(drsrc, dvoff, ldd, blk, r);
        }
    }
    __device__ __forceinline__ void load_d(int blk, float (&dv)[16]) const
    {
#pragma unroll
        for (int r = 0; r < 16; ++r) dv[r] = load_row(drsrc, dvoff, ldd, blk, r);
    }
};

// The pools' winners of a column (bert_amir5.py:627-640): the first maximum in ascending row order -- strict > inside a lane, whose
// rows ascend with block and register; the smaller row wins between the two lane halves -- with the forward value y at the winner,
// and d_sg's sum over the lane's rows.
struct Winners {
    float best_a = -INFINITY, best_b = -INFINITY, ya = 0.0f, yb = 0.0f, acc_sg = 0.0f;
    int ia = 0, ib = 0;
};

__device__ __forceinline__ void scan_rows(Winners &w, const Column &k, const float (&ov)[16], const float (&dv)[16], int blk, int h, int T)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = 32 * blk + row_of(r, h);
        const bool valid = row < T;
        const float y = ov[r] * k.inv_sg;          // (rows past T: 0)
        const float va = y * k.ga, vb = y * k.gb;
        if (valid && va > w.best_a) { w.best_a = va; w.ia = row; w.ya = y; }
        if (valid && vb > w.best_b) { w.best_b = vb; w.ib = row; w.yb = y; }
        w.acc_sg = fmaf(dv[r], y, w.acc_sg);
    }
}

__device__ __forceinline__ void exchange_halves(Winners &w)
{   // the two lane halves hold different rows of the same column: the smaller row wins a tie
    const float oa = __shfl_xor(w.best_a, 32), oya = __shfl_xor(w.ya, 32);
    const int oia = __shfl_xor(w.ia, 32);
    const bool ta = oa > w.best_a || (oa == w.best_a && oia < w.ia);
    w.best_a = ta ? oa : w.best_a; w.ia = ta ? oia : w.ia; w.ya = ta ? oya : w.ya;
    const float ob = __shfl_xor(w.best_b, 32), oyb = __shfl_xor(w.yb, 32);
    const int oib = __shfl_xor(w.ib, 32);
    const bool tb = ob > w.best_b || (ob == w.best_b && oib < w.ib);
    w.best_b = tb ? ob : w.best_b; w.ib = tb ? oib : w.ib; w.yb = tb ? oyb : w.yb;
}

// row is the winner of pool a (b), and that pool's gradient is there: dY of the row takes the pool's share
__device__ __forceinline__ bool wins_a(const Column &k, const Winners &w, int row, int T) { return k.has_pa && row == w.ia && row < T; }
__device__ __forceinline__ bool wins_b(const Column &k, const Winners &w, int row, int T) { return k.has_pb && row == w.ib && row < T; }

// dY of one element in float.  pa_g = dpa * ga, pb_g = dpb * gb: a winner's share, formed by the caller right before its loop over
// the rows -- under -ffp-contract=fast the compiler decides per row whether d_out*sg + share becomes one fma, and it decides by
// what stands next to what; tools/backward_digest.py shows whether a build still computes what the one before it did
__device__ __forceinline__ float dy_row(const Column &k, const Winners &w, float dv, int row, int T, float pa_g, float pb_g)
{
    float g = dv * k.sg;
    if (wins_a(k, w, row, T)) g += pa_g;
    if (wins_b(k, w, row, T)) g += pb_g;
    return g;
}

// acc += A^T . (y0 + y1 + y2), A^T an exact 0/1 operand: three planes x two k-steps, smallest plane first
__device__ __forceinline__ f32x16 mma_01(const bf16x8 (&a)[2], const bf16x8 (&y)[3][2], f32x16 acc)
{
#pragma unroll
    for (int p = 2; p >= 0; --p)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], y[p][s], acc, 0, 0, 0);
    return acc;
}

// acc += (n0 + n1 + n2) . (y0 + y1 + y2): of the nine plane products the six whose weight is >= 2^-16 of the leading one, smallest
// first.  The dropped products are 2^-24 of the leading one.
// A macro, not a function: as a function that returns the accumulator the weighted wide kernel needs 6 more VGPRs.
#define GGCN_NY(ACC, N, Y, P, Q) \
    _Pragma("unroll") for (int ks_ = 0; ks_ < 2; ++ks_) ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(N[P][ks_], Y[Q][ks_], ACC, 0, 0, 0)
#define GGCN_MMA_PLANES6(ACC, N, Y)                                                        \
    do {                                                                                   \
        GGCN_NY(ACC, N, Y, 2, 0); GGCN_NY(ACC, N, Y, 1, 1); GGCN_NY(ACC, N, Y, 0, 2); /* 2^-16 */ \
        GGCN_NY(ACC, N, Y, 1, 0); GGCN_NY(ACC, N, Y, 0, 1);                           /* 2^-8 */  \
        GGCN_NY(ACC, N, Y, 0, 0);                                                          \
    } while (0)

// bsum and w.acc_sg: already summed over the two lane halves
__device__ __forceinline__ void store_column_grads(const Column &k, const Winners &w, int h, float bsum, float *d_bsum, float *d_sg,
                                                   float *d_ga, float *d_gb)
{
    if (h == 0 && k.cok) {
        if (d_bsum) d_bsum[k.gf] = bsum;
        if (d_sg) d_sg[k.gf] = w.acc_sg;
        if (d_ga) d_ga[k.gf] = k.dpa * w.ya;
        if (d_gb) d_gb[k.gf] = k.dpb * w.yb;
    }
}

// ---- dH through LDS, graphs of <= 32 nodes: a wavefront stages 32 rows x 64 columns (two tiles j), then stores 16-byte row pieces.
// The forward's scheme: rows with bit 2 set swap their 32-column halves.
__device__ __forceinline__ void stage64_put(float *stage, const f32x16 &y, int j, int c, int h)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) stage[row_of(r, h) * 64 + ((32 * j + c) ^ (32 * h))] = y[r];
}

__device__ __forceinline__ void stage64_store(const float *stage, float *dH, int64_t ldh, int b, int T, int F, int col0, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    {
        const int colq = (lane & 15) * 4;
        float *gbase = dH + (int64_t)b * T * ldh + col0 + colq;
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int row = 4 * it + (lane >> 4);
            const float4 v4 = *reinterpret_cast<const float4 *>(&stage[row * 64 + (colq ^ (32 * ((row >> 2) & 1)))]);
            if (row < T && col0 + colq < F) *reinterpret_cast<float4 *>(gbase + (int64_t)row * ldh) = v4;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (the next group's tiles overwrite the staging area)
    __builtin_amdgcn_wave_barrier();
}

// ---- dH through LDS, graphs of 33..128 nodes: row block s of a 32-column tile through a 32 x 32 staging tile per wavefront (rows
// padded to kStageLd words): 16-byte stores, eight lanes per 128-byte row segment (lane -> row lane >> 3 of eight, columns 4 (lane & 7)..)
__device__ __forceinline__ void store_block36(float *stage, const f32x16 &acc, int s, float *dH, int64_t ldh, int b, int T, int F, int col0,
                                              int lane)
{
    const int c = lane & 31, h = lane >> 5;
    const int colq = (lane & 7) * 4;
    float *gbase = dH + (int64_t)b * T * ldh + col0 + colq;
    float *mine = stage + 4 * h * kStageLd + c;   // (one lane address + constant row offsets: the writes pair up as ds_write2_b32)
#pragma unroll
    for (int r = 0; r < 16; ++r) mine[row_of(r, 0) * kStageLd] = acc[r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = 8 * it + (lane >> 3);
        const float4 v4 = *reinterpret_cast<const float4 *>(&stage[row * kStageLd + colq]);
        if (32 * s + row < T && col0 + colq < F) *reinterpret_cast<float4 *>(gbase + (int64_t)(32 * s + row) * ldh) = v4;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (the next block overwrites the staging tile)
    __builtin_amdgcn_wave_barrier();
}

// 1 / (rowsum + 1) of source block t in register order, from the workgroup's table in LDS (zero beyond T)
__device__ __forceinline__ void rinv_of_block(const float *sinv, int t, int h, float (&rinv)[16])
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v4 = *reinterpret_cast<const float4 *>(&sinv[32 * t + 8 * q + 4 * h]);
        rinv[4 * q] = v4.x; rinv[4 * q + 1] = v4.y; rinv[4 * q + 2] = v4.z; rinv[4 * q + 3] = v4.w;
    }
}

// ---- host: what the four entries refuse after their null checks, in this order.  GGCN_OK, or the refusal's code.
struct EntryRules {
    const char *who;
    bool empty_batch;         // B == 0 is a call with nothing to do (its caller returns after the checks)
    int t_min;                // T below it: "use <below>"
    const char *below;
    int t_max;                // T above it: the two calls
    const char *ld_names;     // what the leading-dimension refusal says after "leading dimension"
    bool whole_blocks;        // the 2 GiB rule counts T rounded up to 32-row blocks: the offsets of the rows past T, which the range
                              // check zeroes, must not wrap either
    const char *needs;        // the alignment refusal, after "needs "
};

// lds: the leading dimensions of the operands that are there (each >= F); lds_2gib: the ones that join the 2 GiB rule;
// aligned: F, the leading dimensions and the pointers meet the entry's 16-byte rule
inline int backward_entry_checks(const EntryRules &k, int B, int T, int F, std::initializer_list<int64_t> lds,
                                 std::initializer_list<int64_t> lds_2gib, bool aligned)
{
    if (k.empty_batch) {
        if (B < 0 || T < 1 || F < 1) return fail(GGCN_EINVAL, "%s: B=%d T=%d F=%d (B >= 0, T and F positive)", k.who, B, T, F);
    } else if (B <= 0 || T <= 0 || F <= 0) {
        return fail(GGCN_EINVAL, "%s: B=%d T=%d F=%d must be positive", k.who, B, T, F);
    }
    if (T < k.t_min) return fail(GGCN_EUNSUPPORTED, "%s: T=%d <= %d; use %s", k.who, T, k.t_min - 1, k.below);
    if (T > k.t_max) return fail(GGCN_EUNSUPPORTED, "%s: T=%d > %d; use ggcn_gate_pool_backward + ggcn_aggregate_t", k.who, T, k.t_max);
    for (int64_t ld : lds)
        if (ld < F) return fail(GGCN_EINVAL, "%s: leading dimension%s smaller than F=%d", k.who, k.ld_names, F);
    int64_t ldmax = 0;
    for (int64_t ld : lds_2gib) ldmax = ld > ldmax ? ld : ldmax;
    const int64_t rows = k.whole_blocks ? (int64_t)32 * ((T + 31) / 32) : T;
    if (rows * ldmax * 4 >= ((int64_t)1 << 31)) return fail(GGCN_EUNSUPPORTED, "%s: a graph's rows exceed 2 GiB", k.who);
    if (!aligned) return fail(GGCN_EUNSUPPORTED, "%s: needs %s", k.who, k.needs);
    return GGCN_OK;
}

}  // namespace gpb
}  // namespace ggcn
