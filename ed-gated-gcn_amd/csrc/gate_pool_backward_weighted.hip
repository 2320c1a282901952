// Backward of the gate / max-pool epilogue AND the transposed aggregation in one launch, on the matrix cores, for a REAL-valued
// adjacency (a soft or learned graph) of graphs of <= 32 nodes, without gate dropout or (DROP) under it:
//
//   dY[t] = d_out[t]*sg + [t = argmax_a] d_pa*ga + [t = argmax_b] d_pb*gb         models/bert_amir5.py:627-640 backwards
//   dH    = A_w^T . D . dY,   D = diag(1 / (rowsum(A_w) + 1))                       models/gcn.py:35,41 backwards (train.py:120)
//
// The tile is gate_pool_backward_tile.h, the loop gate_pool_backward_mma.hip's (the 0/1 form of this launch): one workgroup per
// graph, four wavefronts that walk the 64-column groups w, w + 4, ..., two 32-column tiles per group, one pass each.  This
// file's own:
//   * A^T is no 0/1 operand: N = A_w^T arrives as THREE bf16 planes (n0 + n1 + n2 = N to 2^-24 of an entry) in
//     ggcn_graph_operands_weighted_t blocks, built once per adjacency from the CSR (graph_operands_wt_kernel below: no transposed
//     CSR).  D.dY is split into three planes y0 + y1 + y2 as before, and the six plane products of GGCN_MMA_PLANES6 -- n0.y0, n0.y1,
//     n1.y0, n0.y2, n1.y1, n2.y0 -- are summed: 12 MFMAs per 32-column tile where the 0/1 form needs 6.
//   * 1 / (rowsum + 1) comes from `inv` (ggcn_inv_denominators: float[B*T]), not from a 0/1 operand block's table; nothing is
//     folded into N, so the blocks depend on the adjacency's entries alone.
//   * dY (optional): the UNSCALED dY, stored for ggcn_adjacency_grad, which reads it from memory.  NULL: nothing of size
//     [B*T,F] but dH is written.
//   * no max |dH|.
//   * DROP (ggcn_gate_pool_backward_weighted_drop; training, bert_amir5.py:621-625): the element math of
//     gate_pool_backward_agg_kernel<true> (gate_pool_backward.hip) in this kernel's register -> row map.  Element
//     ((b T + row) F + col) as uint32 gives the hash of dropout_hash.h and from it the keep factors ks, ka, kb of the three gates;
//     y = out * inv_sg / ks (0 where ks = 0), the pools' candidates are y*ga*ka and y*gb*kb (the winner keeps y*k),
//     d_sg sums d_out*y*ks and dY = d_out*sg*ks + [row = ia] d_pa*ga*ka + [row = ib] d_pb*gb*kb.  The hash is evaluated again in the
//     dY loop: 16 hashes (or 48 keep factors) held per lane across the winners' exchange would cost the third workgroup per CU.
// No atomics, a fixed summation order: bit-identical from run to run.
// Registers (`make resources`): with the three operand planes held in 24 VGPRs and dY stored through lane pointers the kernel
// wants 208 VGPRs and spills 92 bytes per lane under __launch_bounds__(256, 3).  So the planes wait in LDS (6 KiB per workgroup,
// read per tile right before the MFMAs) and dY leaves through a buffer resource (scalar row offsets, no address pairs):
// 153 VGPRs, no scratch, 38 KiB of LDS -- three workgroups per CU (at most 168 VGPRs), as the 0/1 form (149 VGPRs).
// DROP: under that bound the keep factors spill 84 bytes per lane, so the DROP instantiation alone is bound to TWO workgroups per
// CU: 189 VGPRs, no scratch.  The instantiation without dropout keeps the figures above.
#include "dropout_hash.h"
#include "gate_pool_backward_tile.h"

namespace ggcn {
namespace {

using namespace bx3;
using namespace gpb;

constexpr int kOpsBytesWT = GGCN_GRAPH_OPSWT_BYTES;   // plane p, k-step s at (2 p + s) * 1024: 64 lanes x 16 bytes

template <bool DROP>
__global__ __launch_bounds__(256, DROP ? 2 : 3) void gate_pool_backward_weighted_kernel(
    const float *__restrict__ out, int64_t ldo, const float *__restrict__ store_gate, const float *__restrict__ gate_a,
    const float *__restrict__ gate_b, const float *__restrict__ d_out, int64_t ldd, const float *__restrict__ d_pa,
    const float *__restrict__ d_pb, const char *__restrict__ ops_wt, const float *__restrict__ inv, int T, int F,
    float *__restrict__ dH, int64_t ldh, float *__restrict__ dY, int64_t ldy, float *__restrict__ d_sg, float *__restrict__ d_ga,
    float *__restrict__ d_gb, float *__restrict__ d_bsum, DropSpec drop)
{
    __shared__ __attribute__((aligned(16))) float stage_all[4][32 * 64];   // per wavefront: 32 rows x 64 columns on their way to 16-byte stores
    const int b = blockIdx.x;          // one workgroup per graph: its rows are ONE contiguous block of `out` / `d_out` / dH / dY
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    float *stage = stage_all[wave];

    // the graph's operands: the three planes of A_w^T (the aggregation MFMA's A fragments) wait in LDS, read per tile right before
    // the MFMAs -- 24 registers held across the loads of a tile cost the third workgroup per CU; 1/(rowsum + 1) in register order
    __shared__ __attribute__((aligned(16))) char nplanes[kOpsBytesWT];
    for (int i = threadIdx.x; i < kOpsBytesWT / 16; i += 256)
        reinterpret_cast<uint4 *>(nplanes)[i] = reinterpret_cast<const uint4 *>(ops_wt + (int64_t)b * kOpsBytesWT)[i];
    __syncthreads();
    float rinv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row_of(r, h);
        rinv[r] = row < T ? inv[(int64_t)b * T + row] : 0.0f;
    }

#pragma unroll 1
    for (int col0 = wave * 64; col0 < F; col0 += 256) {   // wavefront-uniform walk over this wavefront's 64-column groups
#pragma unroll 1   // (one tile at a time, as in the 0/1 form)
    for (int j = 0; j < 2; ++j) {
        if (col0 + 32 * j >= F) break;   // wavefront-uniform: the group's last tile
        const Column k = column_operands(b, col0 + 32 * j + c, F, store_gate, gate_a, gate_b, d_pa, d_pb);
        float ov[16], dv[16];
        GraphRows(out, ldo, d_out, ldd, b, T, F, h, k.colc).load(0, ov, dv);
        Winners w;
        // DROP: the element of this lane's row 4 h (rows add rs * F), as the forward launch and ggcn_dropout_mask count it
        const uint32_t e0 = DROP ? (uint32_t)(((int64_t)b * T + 4 * h) * F + k.colc) : 0u;
        if constexpr (DROP) {   // scan_rows under the keep factors
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row_of(r, h);
                const bool valid = row < T;
                const uint32_t hh = drop_hash(e0 + (uint32_t)(((r & 3) + 8 * (r >> 2)) * F), drop.seed_lo, drop.seed_hi);
                const float ks = drop_keep(hh, drop.sel[0], drop.thr, drop.scale);
                const float ka = drop_keep(hh, drop.sel[1], drop.thr, drop.scale);
                const float kb = drop_keep(hh, drop.sel[2], drop.thr, drop.scale);
                const float y = ks != 0.0f ? ov[r] * k.inv_sg / ks : 0.0f;   // (rows past T: 0)
                const float va = y * k.ga * ka, vb = y * k.gb * kb;
                if (valid && va > w.best_a) { w.best_a = va; w.ia = row; w.ya = y * ka; }
                if (valid && vb > w.best_b) { w.best_b = vb; w.ib = row; w.yb = y * kb; }
                w.acc_sg = fmaf(dv[r], y * ks, w.acc_sg);
            }
        } else {
            scan_rows(w, k, ov, dv, 0, h, T);
        }
        exchange_halves(w);
        // dY (stored unscaled where the adjacency gradient wants it, behind a resource like the loads') and D.dY in register order
        float gw[16], bsum = 0.0f;
        const float pa_g = k.dpa * k.ga, pb_g = k.dpb * k.gb;
        const __amdgpu_buffer_rsrc_t yrsrc = graph_rows(dY, ldy, b, T, F, out);
        const int yvoff = lane_voff(h, ldy, k.colc);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row_of(r, h);
            float g;
            if constexpr (DROP) {   // the keep factors once more (see the head of the file)
                const uint32_t hh = drop_hash(e0 + (uint32_t)(((r & 3) + 8 * (r >> 2)) * F), drop.seed_lo, drop.seed_hi);
                g = dv[r] * k.sg * drop_keep(hh, drop.sel[0], drop.thr, drop.scale);
                if (wins_a(k, w, row, T)) g = fmaf(k.dpa, k.ga * drop_keep(hh, drop.sel[1], drop.thr, drop.scale), g);
                if (wins_b(k, w, row, T)) g = fmaf(k.dpb, k.gb * drop_keep(hh, drop.sel[2], drop.thr, drop.scale), g);
            } else {
                g = dy_row(k, w, dv[r], row, T, pa_g, pb_g);
            }
            bsum += g;
            if (dY && k.cok && row < T) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(g), yrsrc, yvoff, row_soff(0, r, ldy), 0);
            gw[r] = g * rinv[r];                                   // gcn.py:35: the row's own 1 / (rowsum + 1)
        }
        bsum += __shfl_xor(bsum, 32);
        w.acc_sg += __shfl_xor(w.acc_sg, 32);
        // dH tile = N . (D.dY), N = n0 + n1 + n2, D.dY = y0 + y1 + y2
        bf16x8 pl[3][2];
        split3(gw, pl);
        bf16x8 nft[3][2];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                union { bf16x8 v; uint4 q; } u;
                u.q = *reinterpret_cast<const uint4 *>(nplanes + (2 * p + s) * 1024 + lane * 16);
                nft[p][s] = u.v;
            }
        f32x16 y;
#pragma unroll
        for (int r = 0; r < 16; ++r) y[r] = 0.0f;
        GGCN_MMA_PLANES6(y, nft, pl);
        stage64_put(stage, y, j, c, h);
        store_column_grads(k, w, h, bsum, d_bsum, d_sg, d_ga, d_gb);
    }
    stage64_store(stage, dH, ldh, b, T, F, col0, lane);
    }   // column groups
}

// ggcn_graph_operands_weighted_t: N = A_w^T of a graph of <= 32 nodes as three bf16 planes in A-operand order.  One wavefront
// per graph: the graph's A_w is laid out dense in LDS (lane t < T walks row t of the CSR; entries of one (t, s) add up), then
// lane (s, h) reads column s -- row s of N -- at the 16 k positions its fragments hold and splits each entry as split3 does.
// Rows and columns >= T stay zero.  flag (optional): bit 0 when an entry of A_w is not finite.
__global__ __launch_bounds__(256) void graph_operands_wt_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                                const float *__restrict__ vals, int B, int T, char *__restrict__ ops,
                                                                int *__restrict__ flag)
{
    __shared__ float dense_all[4][32 * 33];   // [t][s], rows padded to 33 words: the column reads below hit 32 banks
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * 4 + wave;
    if (g >= B) return;   // wavefront-uniform (no workgroup barrier below)
    float *dense = dense_all[wave];
    for (int i = lane; i < 32 * 33; i += 64) dense[i] = 0.0f;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int64_t node0 = g * T;
    bool bad = false;
    if (lane < T) {
        const int e1 = rowptr[node0 + lane + 1];
        for (int e = rowptr[node0 + lane]; e < e1; ++e) {
            const int s = colidx[e] - (int)node0;
            const float w = vals ? vals[e] : 1.0f;
            bad = bad || !(fabsf(w) < 3.0e38f);
            if ((unsigned)s < (unsigned)T) dense[lane * 33 + s] += w;   // (an id outside the graph is not followed)
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int s_row = lane & 31, h = lane >> 5;
    char *dst = ops + g * kOpsBytesWT;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        union { uint4 q; unsigned short u[8]; } pl[3];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);   // the column of N = the row of A_w
            const float x = dense[t * 33 + s_row];
            bad = bad || !(fabsf(x) < 3.0e38f);                      // (a sum of finite duplicates may overflow)
            __bf16 p0, p1, p2;
            planes_of(x, p0, p1, p2);
            pl[0].u[j] = __builtin_bit_cast(unsigned short, p0);
            pl[1].u[j] = __builtin_bit_cast(unsigned short, p1);
            pl[2].u[j] = __builtin_bit_cast(unsigned short, p2);
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4 *>(dst + (2 * p + s) * 1024 + lane * 16) = pl[p].q;
    }
    if (bad && flag) atomicOr(flag, 1);
}

}  // namespace

int gate_pool_backward_weighted(const float *out, int64_t ldo, const float *store_gate, const float *gate_a, const float *gate_b,
                                const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb, const void *graph_ops_wt,
                                const float *inv, int B, int T, int F, float *dH, int64_t ldh, float *dY, int64_t ldy, float *d_sg,
                                float *d_ga, float *d_gb, float *d_bsum, hipStream_t st, const DropSpec *drop)
{
    // drop: NULL, or the keep streams of ggcn_gate_pool_backward_weighted_drop (thr = 0: p = 0, the form without dropout)
    const char *who = drop ? "ggcn_gate_pool_backward_weighted_drop" : "ggcn_gate_pool_backward_weighted";
    if (!out) return fail(GGCN_EINVAL, "%s: out is null", who);
    if (!dH) return fail(GGCN_EINVAL, "%s: dH is null", who);
    if (!inv) return fail(GGCN_EINVAL, "%s: inv is null", who);
    if (!graph_ops_wt) return fail(GGCN_EINVAL, "%s: graph_ops_wt is null", who);
    const EntryRules rules = {who, true, 1, "", 32, " (ldo, ldd, ldh, ldy)", false,
                              "F % 4 == 0, ldo, ldd, ldh, ldy % 4 == 0 and 16-byte aligned dH / dY / graph_ops_wt; use "
                              "ggcn_gate_pool_backward + ggcn_aggregate_t"};
    const int64_t ldd_in = d_out ? ldd : F, ldy_in = dY ? ldy : F;   // (an operand that is not there: its leading dimension is not read)
    if (const int rc = backward_entry_checks(rules, B, T, F, {ldo, ldh, ldd_in, ldy_in}, {ldo, ldh, ldd_in, ldy_in},
                                             F % 4 == 0 && ldh % 4 == 0 && ldo % 4 == 0 && ldd_in % 4 == 0 && ldy_in % 4 == 0 && aligned16(dH) &&
                                                 (!dY || aligned16(dY)) && aligned16(graph_ops_wt)))
        return rc;
    if (drop && (int64_t)B * T * F >= ((int64_t)1 << 32))
        return fail(GGCN_EUNSUPPORTED, "%s: gate dropout indexes elements with 32 bits (B*T*F = %lld)", who, (long long)B * T * F);
    if (B == 0) return GGCN_OK;
    if (drop && drop->thr != 0)
        hipLaunchKernelGGL(gate_pool_backward_weighted_kernel<true>, dim3((unsigned)B), dim3(256), 0, st, out, ldo, store_gate, gate_a, gate_b,
                           d_out, d_out ? ldd : ldo, d_pa, d_pb, static_cast<const char *>(graph_ops_wt), inv, T, F, dH, ldh, dY, ldy, d_sg,
                           d_ga, d_gb, d_bsum, *drop);
    else
        hipLaunchKernelGGL(gate_pool_backward_weighted_kernel<false>, dim3((unsigned)B), dim3(256), 0, st, out, ldo, store_gate, gate_a, gate_b,
                           d_out, d_out ? ldd : ldo, d_pa, d_pb, static_cast<const char *>(graph_ops_wt), inv, T, F, dH, ldh, dY, ldy, d_sg,
                           d_ga, d_gb, d_bsum, DropSpec{});
    return check_launch(who);
}

}  // namespace ggcn

using namespace ggcn;

extern "C" {

size_t ggcn_graph_operands_weighted_t_bytes(int B) { return B > 0 ? (size_t)B * kOpsBytesWT : 0; }

int ggcn_graph_operands_weighted_t(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, void *ops,
                                   int32_t *flag, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const char *who = "ggcn_graph_operands_weighted_t";
    if (!rowptr) return fail(GGCN_EINVAL, "%s: rowptr is null", who);
    if (!colidx) return fail(GGCN_EINVAL, "%s: colidx is null", who);
    if (!ops) return fail(GGCN_EINVAL, "%s: graph_ops_wt is null", who);
    if (B < 0) return fail(GGCN_EINVAL, "%s: B=%d must not be negative", who, B);
    if (T < 1) return fail(GGCN_EINVAL, "%s: T=%d must be positive", who, T);
    if (T > 32) return fail(GGCN_EUNSUPPORTED, "%s: T=%d > 32 (one 32 x 32 block per graph)", who, T);
    if (!aligned16(ops)) return fail(GGCN_EINVAL, "%s: graph_ops_wt must be 16-byte aligned", who);
    if (B == 0) return GGCN_OK;
    const int64_t grid = ((int64_t)B + 3) / 4;
    hipLaunchKernelGGL(graph_operands_wt_kernel, dim3((unsigned)grid), dim3(256), 0, st, rowptr, colidx, vals, B, T, static_cast<char *>(ops), flag);
    return check_launch(who);
}

}  // extern "C"
