// Backward of the gate / max-pool epilogue AND the transposed aggregation in one launch, on the matrix cores, for a REAL-valued
// adjacency (a soft or learned graph) of graphs of 33..128 nodes, without gate dropout:
//
//   dY[t] = d_out[t]*sg + [t = argmax_a] d_pa*ga + [t = argmax_b] d_pb*gb         models/bert_amir5.py:627-640 backwards
//   dH    = A_w^T . D . dY,   D = diag(1 / (rowsum(A_w) + 1))                       models/gcn.py:35,41 backwards (train.py:120)
//
// The tile is gate_pool_backward_tile.h, the two-pass loop gate_pool_backward_wide.hip's (the 0/1 form of this launch): one
// workgroup per graph, four wavefronts that walk the 32-column tiles w, w + 4, ...; pass 1 walks the NB = ceil(T/32) row blocks
// of `out` and `d_out` for the winners and d_sg; pass 2 reloads d_out per SOURCE block t (L2-hot), forms dY and D.dY and splits
// the latter into three bf16 planes y0 + y1 + y2.  This file's own:
//   * A^T is no 0/1 operand: N = A_w^T arrives as THREE bf16 planes n0 + n1 + n2 per 32 x 32 block
//     (ggcn_graph_operands_weighted_wide_t, built once per adjacency from the CSR: no transposed CSR), the three-plane scheme of
//     gate_pool_backward_weighted.hip.  The six plane products of GGCN_MMA_PLANES6 are added into acc[s] for every DESTINATION block s
//     whose (s, t) block is not empty: 12 MFMAs (v_mfma_f32_32x32x16_bf16) per block where the 0/1 form needs 6.
//   * the A-operand fragments come straight from global memory / L2 in fragment order (6 x 1 KiB per block, one 16-byte load per
//     lane and fragment): 96 KiB per graph at NB = 4 does not fit in LDS beside a second workgroup.  They are requested one
//     non-empty block AHEAD of their MFMAs (two sets of 24 registers), so that a block's L2 latency lies under the block before
//     it or under the d_out loads and the dY arithmetic of its source block.  A graph's operand is read once
//     per column tile.
//   * the 16-bit block summary (bit 4 s + t: block (s, t) of A_w^T has a non-zero entry) is the builder's word behind the blocks,
//     not a ballot: a wavefront skips the loads and the MFMAs of an empty block, uniformly.
//   * nothing is folded into N: 1 / (rowsum + 1) comes from `inv` (ggcn_inv_denominators: float[B*T]) through LDS, zero beyond T,
//     the same float the two passes use.
//   * dY is rounded ONCE: d_out*sg + d_pa*ga + d_pb*gb is formed in float64, where the three products are exact, and converted.
//     A winner's pool term can cancel most of d_out*sg; float32 sums would then leave an error of several u of the RESULT, and
//     this launch's dY is held to 4 u |dY| elementwise.  Sixteen conversions and at most 48 float64 operations per block and lane.
//   * dY (optional): the UNSCALED dY, stored for ggcn_adjacency_grad, which reads it from memory, through a buffer resource that
//     ends with the graph's last row.  NULL: nothing of size [B*T,F] but dH is written.  dH is the same with and without it.
//   * no max |dH| and no form under gate dropout: ggcn_gate_pool_backward_drop + ggcn_aggregate_t keep that case.
// No atomics, a fixed summation order (source blocks in ascending t, products smallest first): bit-identical from run to run.
// Traffic per layer: out + d_out read, d_out read again (L2), dH written (+ dY): 3 (4) N F 4 bytes from memory; the operand
// blocks come from L2 after the first column tile.
// Registers (`make resources`): 214 VGPRs (four accumulators, two sets of six fragments, the loads of a block in flight), no
// scratch, 18944 bytes of LDS: two workgroups per CU (__launch_bounds__(256, 2)).  graph_operands_wwt_kernel: 63 VGPRs, no
// scratch, 65552 bytes of LDS (four strips of 32 x 128 floats), two workgroups per CU.
#include "gate_pool_backward_tile.h"

namespace ggcn {
namespace {

using namespace bx3;
using namespace gpb;

constexpr int kBlockBytes = 6 * 1024; // one 32 x 32 block of A_w^T: plane p, k-step k at (2 p + k) * 1024, 64 lanes x 16 bytes

__global__ __launch_bounds__(256, 2) void gate_pool_backward_weighted_wide_kernel(
    const float *__restrict__ out, int64_t ldo, const float *__restrict__ store_gate, const float *__restrict__ gate_a,
    const float *__restrict__ gate_b, const float *__restrict__ d_out, int64_t ldd, const float *__restrict__ d_pa,
    const float *__restrict__ d_pb, const char *__restrict__ ops, const uint32_t *__restrict__ summary, const float *__restrict__ inv,
    int T, int F, float *__restrict__ dH, int64_t ldh, float *__restrict__ dY, int64_t ldy, float *__restrict__ d_sg,
    float *__restrict__ d_ga, float *__restrict__ d_gb, float *__restrict__ d_bsum)
{
    __shared__ __attribute__((aligned(16))) float stage_all[4][32 * kStageLd];   // per wavefront: one 32 x 32 block of dH on its way to 16-byte stores
    __shared__ __attribute__((aligned(16))) float sinv[kMaxT];                   // 1 / (rowsum + 1); zero beyond T
    const int b = blockIdx.x;          // one workgroup per graph: its rows are ONE contiguous block of `out` / `d_out` / dH / dY
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int nb = (T + 31) >> 5;      // 2..4 (the entry refuses anything else)
    float *stage = stage_all[wave];

    if (threadIdx.x < kMaxT) sinv[threadIdx.x] = (int)threadIdx.x < T ? inv[(int64_t)b * T + threadIdx.x] : 0.0f;
    __syncthreads();
    // bit 4 s + t: block (s, t) of A_w^T is not empty (bits of blocks the graph does not have are not followed)
    const uint32_t have = ((1u << nb) - 1u) * 0x1111u & ((1u << (4 * nb)) - 1u);
    const uint32_t live = __builtin_amdgcn_readfirstlane(summary[b]) & have;
    uint32_t live_t = 0u;              // the same bits in the order the blocks are used: bit 4 t + s
#pragma unroll
    for (int q = 0; q < 16; ++q) live_t |= ((live >> (4 * (q & 3) + (q >> 2))) & 1u) << q;
    const char *nlane = ops + (int64_t)b * nb * nb * kBlockBytes + lane * 16;   // this lane's 16 bytes of every fragment of the graph
    // the six fragments of block q = 4 t + s.  A block's fragments are requested one block AHEAD of their MFMAs: while the block
    // before it is multiplied, or -- the first block of a source block t -- before d_out of t is loaded and dY formed; the
    // request after a tile's last block is for the next tile's first.  (The last request of a workgroup is not used.)
    auto load6 = [&](bf16x8 (&f)[3][2], int q) {
        const char *blk = nlane + ((q & 3) * nb + (q >> 2)) * kBlockBytes;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                union { bf16x8 v; uint4 q; } u;
                u.q = *reinterpret_cast<const uint4 *>(blk + (2 * p + k) * 1024);
                f[p][k] = u.v;
            }
    };
    bf16x8 cur[3][2] = {};
    if (live_t) load6(cur, __builtin_ctz(live_t));   // wavefront-uniform

#pragma unroll 1
    for (int col0 = wave * 32; col0 < F; col0 += 128) {   // wavefront-uniform walk over this wavefront's 32-column tiles
        const Column k = column_operands(b, col0 + c, F, store_gate, gate_a, gate_b, d_pa, d_pb);
        // (this kernel's own text, not GraphRows: through the struct the kernel keeps 12 more scalars in VGPR lanes)
        const int colc = k.colc;
        const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(out + (int64_t)b * T * ldo), 0,
                                                                              (int)((((int64_t)T - 1) * ldo + F) * 4), 0x00020000);
        const __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>((d_out ? d_out : out) + (int64_t)b * T * (d_out ? ldd : ldo)), 0,
                                                                              d_out ? (int)((((int64_t)T - 1) * ldd + F) * 4) : 0, 0x00020000);
        const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(dY ? dY + (int64_t)b * T * ldy : const_cast<float *>(out), 0,
                                                                              dY ? (int)((((int64_t)T - 1) * ldy + F) * 4) : 0, 0x00020000);
        const int ovoff = (int)((4 * h * ldo + colc) * 4), dvoff = (int)((4 * h * ldd + colc) * 4), yvoff = (int)((4 * h * ldy + colc) * 4);

        // ---- pass 1: the pools' winners over every row block, d_sg
        Winners w;
#pragma unroll 1
        for (int blk = 0; blk < nb; ++blk) {
            float ov[16], dv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                ov[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(orsrc, ovoff, row_soff(blk, r, ldo), 0));
                dv[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(drsrc, dvoff, row_soff(blk, r, ldd), 0));   // (no d_out: zeros)
            }
            scan_rows(w, k, ov, dv, blk, h, T);
        }
        exchange_halves(w);

        // ---- pass 2: per source block t, dY (stored unscaled where the adjacency gradient wants it) and D.dY in register order,
        //      then dH[s] += N(s, t) . (D.dY)(t) for every live s
        f32x16 acc[kMaxNB];
#pragma unroll
        for (int s = 0; s < kMaxNB; ++s)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[s][r] = 0.0f;
        float bsum = 0.0f;
        const double sg64 = k.sg, pa_g64 = (double)k.dpa * k.ga, pb_g64 = (double)k.dpb * k.gb;
#pragma unroll 1
        for (int t = 0; t < nb; ++t) {
            float dv[16], rinv[16], gw[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) dv[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(drsrc, dvoff, row_soff(t, r, ldd), 0));
            rinv_of_block(sinv, t, h, rinv);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * t + row_of(r, h);
                // one rounding: the products are exact in float64, so a pool term that cancels d_out * sg costs no relative accuracy
                double g64 = (double)dv[r] * sg64;
                if (wins_a(k, w, row, T)) g64 += pa_g64;
                if (wins_b(k, w, row, T)) g64 += pb_g64;
                const float g = (float)g64;
                bsum += g;
                if (dY && k.cok && row < T) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(g), yrsrc, yvoff, row_soff(t, r, ldy), 0);
                {   // gcn.py:35: the row's own 1 / (rowsum + 1).  Under -ffp-contract=fast the compiler may fuse this product into
                    // split3's x - p0 (an fma of the unrounded product).  In the builds of this library it does so in the 0/1 kernels
                    // (all 16 rows) and in part of the weighted one, and never did here; each kernel's bits are pinned by
                    // tools/backward_digest.py against the build before it.  Here the compiler began to fuse 4 of the 16 rows once the
                    // split moved into the shared header, so the rounding this kernel always had is written down:
#pragma clang fp contract(off)
                    gw[r] = g * rinv[r];
                }
            }
            bf16x8 pl[3][2];
            split3(gw, pl);
#pragma unroll
            for (int s = 0; s < kMaxNB; ++s) {
                const int q = 4 * t + s;
                if (!((live_t >> q) & 1u)) continue;   // wavefront-uniform: block (s, t) is empty (or s >= nb)
                const uint32_t rest = live_t >> (q + 1);
                bf16x8 nxt[3][2];
                load6(nxt, rest ? q + 1 + __builtin_ctz(rest) : __builtin_ctz(live_t));
                GGCN_MMA_PLANES6(acc[s], cur, pl);
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) cur[p][kk] = nxt[p][kk];
            }
        }
        bsum += __shfl_xor(bsum, 32);
        w.acc_sg += __shfl_xor(w.acc_sg, 32);
        store_column_grads(k, w, h, bsum, d_bsum, d_sg, d_ga, d_gb);
        // ---- dH, one 32-row block at a time: store_block36's text in place (through the call the kernel needs 2 more VGPRs)
        const int colq = (lane & 7) * 4;
        float *gbase = dH + (int64_t)b * T * ldh + col0 + colq;
#pragma unroll
        for (int s = 0; s < kMaxNB; ++s) {
            if (s >= nb) break;   // wavefront-uniform
#pragma unroll
            for (int r = 0; r < 16; ++r) stage[row_of(r, h) * kStageLd + c] = acc[s][r];
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
    }   // column tiles
}

// ggcn_graph_operands_weighted_wide_t: N = A_w^T of a graph of 33..128 nodes as W x W blocks (W = ceil(T/32)) of three bf16 planes
// in A-operand order, and the graph's block summary.  One workgroup per graph, wavefront tb per 32-row block tb of A_w: the
// block's rows are laid out dense in LDS (lane r < 32 walks row 32 tb + r of the CSR in CSR order; entries of one (t, s) add up;
// word (s + r) & 127 of row r, so that the lanes of a dense row miss each other's banks), then for every s the lane (s_row, h)
// reads column 32 s + s_row -- row s_row of block (s, tb) of N -- at the 16 k positions its fragments hold and splits each entry
// as split3 does.  Rows and columns >= T stay zero.  The summary word (bit 4 s + t: block (s, t) has a non-zero entry) is put
// together in LDS and written once; -0.0 counts as zero there (x != 0.0f), so a block of nothing but signed zeros is skipped.
// flag (optional): bit 0 when an entry of A_w, or a sum of duplicates, is not finite or not below 3.0e38 in magnitude (its first
// bf16 plane would round to infinity).
__global__ __launch_bounds__(256) void graph_operands_wwt_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                                 const float *__restrict__ vals, int T, char *__restrict__ ops,
                                                                 uint32_t *__restrict__ summary, int *__restrict__ flag)
{
    __shared__ float dense_all[kMaxNB][32 * kMaxT];
    __shared__ uint32_t live_part[kMaxNB];
    const int lane = threadIdx.x & 63;
    const int tb = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W = (T + 31) >> 5;
    const int64_t g = blockIdx.x;
    const int64_t node0 = g * T;
    float *dense = dense_all[tb];
    bool bad = false;
    uint32_t bits = 0u;
    if (tb < W) {   // wavefront-uniform
        for (int i = lane; i < 32 * kMaxT; i += 64) dense[i] = 0.0f;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int trow = 32 * tb + lane;
        if (lane < 32 && trow < T) {
            auto take = [&](int col, float w) {
                const int s = col - (int)node0;
                bad = bad || !(fabsf(w) < 3.0e38f);
                if ((unsigned)s < (unsigned)T) dense[lane * kMaxT + ((s + lane) & (kMaxT - 1))] += w;   // (an id outside the graph is not followed)
            };
            const int e1 = rowptr[node0 + trow + 1];
            int e = rowptr[node0 + trow];
            for (; e + 4 <= e1; e += 4) {   // four edges per trip, their loads in flight together; CSR order kept
                int cj[4];
                float wj[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) { cj[q] = colidx[e + q]; wj[q] = vals ? vals[e + q] : 1.0f; }
#pragma unroll
                for (int q = 0; q < 4; ++q) take(cj[q], wj[q]);
            }
            for (; e < e1; ++e) take(colidx[e], vals ? vals[e] : 1.0f);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int s_row = lane & 31, h = lane >> 5;
        for (int s = 0; s < W; ++s) {
            char *dst = ops + ((g * W + s) * W + tb) * kBlockBytes;
            bool any = false;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                union { uint4 q; unsigned short u[8]; } pl[3];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int t = 16 * k + 8 * (j >> 2) + 4 * h + (j & 3);   // the column of N = the row of A_w inside block tb
                    const float x = dense[t * kMaxT + ((32 * s + s_row + t) & (kMaxT - 1))];
                    bad = bad || !(fabsf(x) < 3.0e38f);                      // (a sum of finite duplicates may overflow)
                    any = any || x != 0.0f;
                    __bf16 p0, p1, p2;
                    planes_of(x, p0, p1, p2);
                    pl[0].u[j] = __builtin_bit_cast(unsigned short, p0);
                    pl[1].u[j] = __builtin_bit_cast(unsigned short, p1);
                    pl[2].u[j] = __builtin_bit_cast(unsigned short, p2);
                }
#pragma unroll
                for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4 *>(dst + (2 * p + k) * 1024 + lane * 16) = pl[p].q;
            }
            if (__builtin_amdgcn_ballot_w64(any) != 0) bits |= 1u << (4 * s + tb);
        }
    }
    if (lane == 0) live_part[tb] = bits;
    __syncthreads();
    if (threadIdx.x == 0) summary[g] = live_part[0] | live_part[1] | live_part[2] | live_part[3];
    if (bad && flag) atomicOr(flag, 1);
}

}  // namespace
}  // namespace ggcn

using namespace ggcn;

extern "C" {

size_t ggcn_graph_operands_weighted_wide_t_bytes(int B, int T)
{
    if (B <= 0 || T <= 32 || T > kMaxT) return 0;
    const size_t W = (size_t)(T + 31) / 32;
    return (size_t)B * (W * W * kBlockBytes + 4);   // the blocks, then one summary word per graph
}

int ggcn_graph_operands_weighted_wide_t(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, void *ops,
                                        int32_t *flag, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const char *who = "ggcn_graph_operands_weighted_wide_t";
    if (!rowptr || !colidx || !ops) return fail(GGCN_EINVAL, "%s: null pointer", who);
    if (B <= 0 || T <= 0) return fail(GGCN_EINVAL, "%s: B=%d T=%d must be positive", who, B, T);
    if (T <= 32) return fail(GGCN_EUNSUPPORTED, "%s: T=%d <= 32; use ggcn_graph_operands_weighted_t", who, T);
    if (T > kMaxT) return fail(GGCN_EUNSUPPORTED, "%s: T=%d > 128 (four blocks per row of blocks)", who, T);
    if (!aligned16(ops)) return fail(GGCN_EINVAL, "%s: the blocks must be 16-byte aligned", who);
    if ((int64_t)B * T >= (int64_t)INT32_MAX) return fail(GGCN_EUNSUPPORTED, "%s: B*T does not fit int32 node ids", who);
    const int W = (T + 31) >> 5;
    char *blocks = static_cast<char *>(ops);
    hipLaunchKernelGGL(graph_operands_wwt_kernel, dim3((unsigned)B), dim3(256), 0, st, rowptr, colidx, vals, T, blocks,
                       reinterpret_cast<uint32_t *>(blocks + (size_t)B * W * W * kBlockBytes), flag);
    return check_launch(who);
}

int ggcn_gate_pool_backward_weighted_wide(const float *out, int64_t ldo, const float *store_gate, const float *gate_a, const float *gate_b,
                                          const float *d_out, int64_t ldd, const float *d_pa, const float *d_pb, const void *graph_ops_wwt,
                                          const float *inv, int B, int T, int F, float *dH, int64_t ldh, float *dY, int64_t ldy, float *d_sg,
                                          float *d_ga, float *d_gb, float *d_bsum, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const char *who = "ggcn_gate_pool_backward_weighted_wide";
    if (!out || !dH || !graph_ops_wwt || !inv) return fail(GGCN_EINVAL, "%s: null pointer", who);
    const EntryRules rules = {who, false, 33, "ggcn_gate_pool_backward_weighted", kMaxT, "", true,
                              "F % 4 == 0, ldh % 4 == 0 and 16-byte aligned dH / graph_ops_wwt; use ggcn_gate_pool_backward + ggcn_aggregate_t"};
    const int64_t ldd_in = d_out ? ldd : F, ldy_in = dY ? ldy : F;   // (an operand that is not there: its leading dimension is not read)
    if (const int rc = backward_entry_checks(rules, B, T, F, {ldo, ldh, ldd_in, ldy_in}, {ldo, ldh, ldd_in, ldy_in},
                                             F % 4 == 0 && ldh % 4 == 0 && aligned16(dH) && aligned16(graph_ops_wwt)))
        return rc;
    const int W = (T + 31) >> 5;
    const char *blocks = static_cast<const char *>(graph_ops_wwt);
    hipLaunchKernelGGL(gate_pool_backward_weighted_wide_kernel, dim3((unsigned)B), dim3(256), 0, st, out, ldo, store_gate, gate_a, gate_b,
                       d_out, d_out ? ldd : ldo, d_pa, d_pb, blocks, reinterpret_cast<const uint32_t *>(blocks + (size_t)B * W * W * kBlockBytes),
                       inv, T, F, dH, ldh, dY, dY ? ldy : ldo, d_sg, d_ga, d_gb, d_bsum);
    return check_launch(who);
}

}  // extern "C"
