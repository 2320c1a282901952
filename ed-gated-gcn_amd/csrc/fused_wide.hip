// One launch per gated layer for graphs of 33..128 nodes (LitBank: ORI_ML = 100, constant.py:227): see fused_layer.hip for
// the scheme (models/gcn.py:34-45 + bert_amir5.py:627-640 in one kernel, `hidden` never leaving the CU).
#include "fused_common.h"

namespace ggcn {
namespace {

// ---- graphs of 33..128 nodes (LitBank: ORI_ML = 100, constant.py:227) in the same one launch per layer; graphs of 129..256
// nodes (ACE cased: ORI_ML = 231, constant.py:267) take layer_fused_wide8_kernel (fused_wide8.hip) ----
// A graph occupies SB = 2 or 4 consecutive 32-row blocks of a wavefront's 128-row tile (64- or 128-row slot;
// T in 65..96 takes the 128-row slot), its adjacency is SB x SB blocks of 32 x 32 bits (row masks of
// ceil(T/32) words), and the neighbour sum of output block io is
//     agg[io] = sum_ii ADJ[io][ii] . hidden[ii]          (SB x 4 MFMAs per 32 x 32 output tile)
// with every hidden[ii] taken from the accumulator tiles as in the 32-node kernel.  All accumulators are first
// split into their two bf16 planes IN PLACE (same register count), then each output block is produced,
// normalised, gated, pooled and stored.  One part only (the two-layer block form stays with T <= 32).
// DROP (training, bert_amir5.py:621-625): the three gates are dropped per (token, feature) -- keep factors from the
// counter-based hash of dropout_hash.h, the same ones ggcn_gate_pool_backward_drop and ggcn_dropout_mask draw -- and the
// pools maximise the gated, kept values themselves (every element has its own factor: no max / min shortcut).
// XT: element type of the features -- float, or __bf16 (a.Xb; bf16x3 image, two MFMAs per product: bf16x3_core.h); the epilogue
// works on the float32 accumulators and is the same for both.
// WEIGHTED (ggcn_layer_fused_weighted_wide): a REAL-valued adjacency (gcn.py:33-41 take any `adj`).  No row masks are read: the
// A operands are the hi / lo bf16 fragments of M = D.A_w that ggcn_graph_operands_weighted_wide left in a.graph_ops (layout:
// kWOpsBlock in fused_common.h), D already inside, and an output block is
//     y[io] = sum_ii  Mlo[io][ii].Hhi[ii] + Mhi[io][ii].Hlo[ii] + Mhi[io][ii].Hhi[ii]      (3 x W x 2 MFMAs, small terms first;
// the lo.lo term is 2^-18 of a term) over the W = ceil(T/32) real blocks only.  Everything after y -- bias, gates, row stores,
// pools, ov_partial -- is the code of the 0/1 form with the row factor 1.  The fragments of block row io (W x 4 KiB) come from
// global memory into the registers the 0/1 form spends on masks, expanded fragments and rinv; a load waits 1-2 us in an
// epilogue (fused_common.h), so the lo fragments of the NEXT block row (the next graph's first one after the last) are
// requested as soon as the last column tile's lo products have issued and the hi fragments after its hi products: the
// element-wise work and stores of that tile and the next row's first products run under them.
// WEIGHTED && DROP (ggcn_layer_fused_weighted_wide_drop): both of the above -- the keep factors only touch what follows y.
// wide_one_wave: the one instantiation compiled WITHOUT the two-wavefronts-per-SIMD bound.  WEIGHTED && DROP with the general f16mx8 main loop at
// SB = 4 spills 8 bytes per lane under it -- 64 registers of fragments, 128 of planes and the pools' running maxima leave nothing
// for the hash; an opaque lane id after the main loop and a 32-bit element index left one register spilled.  Unbound it takes
// 253 VGPRs + 128 AGPRs and no scratch: ONE wavefront per SIMD, for the slow-shape form (K % 32 != 0 or rows off 16 bytes) of
// 65..128-node graphs under dropout in f16mx8 alone.  The fast shapes and every bf16x3 form keep two.  Its speed is not measured.
constexpr bool wide_one_wave(int sch, bool avec, int sb, bool drop, bool weighted) { return weighted && drop && sch == 1 && sb == 4 && !avec; }
template <int SCH, bool AVEC, bool KFULL, bool VST, int SB, bool DROP = false, typename XT = float, bool WEIGHTED = false>
__global__ __launch_bounds__(kThreads, wide_one_wave(SCH, AVEC, SB, DROP, WEIGHTED) ? 1 : kWavesPerSimd) void layer_fused_wide_kernel(const FusedArgs a)
{
    static_assert(SB == 2 || SB == 4, "a graph slot is 64 or 128 rows");
    static_assert(!WEIGHTED || std::is_same<XT, float>::value, "real-valued adjacency: float32 features");
    static_assert(std::is_same<XT, float>::value || SCH == 0, "bf16 features: the bf16x3 main loop");
    __shared__ __attribute__((aligned(16))) char lds[kLdsBytes];
    const int B = a.B, T = a.T, K = a.K, F = a.F;
    if (a.ov_in && blockIdx.x == 0) reduce_partials(a.ov_in, B * ((F + 63) / 64), B, a.ov_out, reinterpret_cast<float *>(lds));
    int g_tile, n_wgi;
    if (!tile_of_block(blockIdx.x, a.g_tiles, a.n_wg, g_tile, n_wgi)) return;
    const LayerPart &lp = a.part[0];
    const float *__restrict__ bias = lp.bias, *__restrict__ store_gate = lp.store_gate;
    const float *__restrict__ pool_gate_a = lp.pool_gate_a, *__restrict__ pool_gate_b = lp.pool_gate_b;
    float *__restrict__ out = lp.out, *__restrict__ pool_a = lp.pool_a, *__restrict__ pool_b = lp.pool_b;
    float *__restrict__ ov_partial = lp.ov_partial;
    const int ldo = lp.ldo;
    constexpr int S = 32 * SB;                     // rows per graph slot
    constexpr int GPT = 4 / SB;                    // graphs per workgroup

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    static_assert(WM == 1, "the wide-graph kernel is written for one wavefront row per workgroup");
    const int g0 = g_tile * GPT;
    const int n_tiles_total = (F + NT - 1) / NT;
    const int nt0 = n_wgi * (BN / NT) + wn * RN;
    const int W = (T + 31) >> 5;

    constexpr int NP = Geom<XT>::NP;
    // every accumulator tile -> its two bf16 planes (B-operand fragments of the aggregation MFMAs), in place
    bf16x8 hf[4][RN][2][2];
    // hidden = X . W, then split.  The ONE-TRIP loop is deliberate: this body once ran per 128-row half of a 256-row slot, and as a
    // plain block the compiler orders the code around the main loop differently -- every instantiation moves by a few instructions.
    // Kept so that the device code stays byte-identical; whoever next changes this kernel's code may make it a block.
#pragma unroll
    for (int once = 0; once < 1; ++once) {
        const XT *arow[NP];
        bool avalid[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int row = stage_row<XT>(i);
            const int g = g0 + row / S, r = row % S;
            avalid[i] = (g < B) && (r < T);
            const int64_t node = avalid[i] ? (int64_t)g * T + r : 0;
            arow[i] = fused_x<XT>(a) + node * a.ldx;
        }
        f32x16 acc[4][RN];
        if constexpr (SCH == 0)
            bx3::mainloop<XT, AVEC, KFULL, true>(arow, avalid, lp.wpack, K, a.k_steps, wm, nt0, n_tiles_total, lds, acc);
        else {
            constexpr bool BUF = AVEC && KFULL;   // buffer loads (f16mx8_core.h): offsets from the workgroup's first graph
            mx8::BufX<float> bx;
            if constexpr (BUF) {
                int rel[NP];
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const int row = stage_row<float>(i);
                    rel[i] = avalid[i] ? (row / S) * T + row % S : -1;
                }
                bx = mx8::make_bufx<float>(a.X, a.ldx, (int64_t)g0 * T, (int64_t)B * T, rel, tid);
            }
            mx8::mainloop<float, AVEC, KFULL, true, false, BUF>(arow, avalid, lp.wpack, K, a.k_steps / 2, wm, nt0, n_tiles_total, lds, acc, 0, 4,
                                                                 nullptr, &bx);
        }
        // `pre` (ggcn_layer_fused_prebias): y = D.A.(hidden + 1.pre^T) + bias -- the folded second layer of the eval form, whose
        // input rows are already aggregated once (gated_block.py).  Workgroup-uniform; padding rows are nobody's neighbours.
        // (float32 features only: the bf16 launches refuse `pre`, and without this branch their accumulators are never live twice)
        if (!WEIGHTED && std::is_same<XT, float>::value && lp.pre) {   // (the weighted entry takes no `pre`)
#pragma unroll
            for (int j = 0; j < RN; ++j) {
                const int gn = (nt0 + j) * NT + (lane & 31);
                const float pv = lp.pre[gn < F ? gn : 0];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] += pv;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < RN; ++j) split2(acc[i][j], hf[i][j]);
    }

    const int c = lane & 31, h = lane >> 5;
    float vb[RN], vsg[GPT][RN], vga[GPT][RN], vgb[GPT][RN];
    bool col_ok[RN];
    {
        const float *dummy = a.X;
        const float *pb = bias ? bias : dummy, *psg = store_gate ? store_gate : dummy;
        const float *pga = pool_gate_a ? pool_gate_a : dummy, *pgb = pool_gate_b ? pool_gate_b : dummy;
#pragma unroll
        for (int j = 0; j < RN; ++j) {
            const int gn = (nt0 + j) * NT + c;
            col_ok[j] = gn < F;
            const int gnc = col_ok[j] ? gn : 0;
            vb[j] = pb[bias ? gnc : 0];
#pragma unroll
            for (int s = 0; s < GPT; ++s) {
                const int64_t at = (int64_t)(g0 + s < B ? g0 + s : 0) * F + gnc;
                vsg[s][j] = psg[store_gate ? at : 0];
                vga[s][j] = pga[pool_gate_a ? at : 0];
                vgb[s][j] = pgb[pool_gate_b ? at : 0];
            }
        }
    }
    float *stage_lds = reinterpret_cast<float *>(lds) + wave * (32 * 64);
    const int perm_base = 16 * h;
    const int lane_off = 4 * h * ldo + c;
    // WEIGHTED: the A fragments of one block row, wf[plane][ii][ks] (plane 0 = hi, 1 = lo): 16 bytes per lane and fragment
    constexpr int WSB = WEIGHTED ? SB : 1;
    bf16x8 wf[2][WSB][2];
    // (no branch around a load: a conditional load makes the compiler copy the fragments where the paths meet, and wait for them there)
    auto fetch_w = [&](int g, int io, int plane) {
        const char *src = a.graph_ops + ((int64_t)g * W * W + (int64_t)io * W) * kWOpsBlock + plane * 2048 + lane * 16;
#pragma unroll
        for (int ii = 0; ii < WSB; ++ii) {
            const int ic = ii < W ? ii : 0;   // workgroup-uniform: the 128-row slot of a 65..96-node graph has three blocks (the fourth: block 0 again, unused)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) wf[plane][ii][ks] = *reinterpret_cast<const bf16x8 *>(src + ic * kWOpsBlock + ks * 1024);
        }
    };
    // the block row after (graph slot s, block row io) of this workgroup, requested while the current one is finished; after the
    // last one the current row once more (unused)
    auto fetch_next_w = [&](int s, int io, int plane) {
        const int g = g0 + s;
        const bool row = 32 * (io + 1) < T, graph = s + 1 < GPT && g + 1 < B;
        fetch_w(row ? g : graph ? g + 1 : g, row ? io + 1 : graph ? 0 : io, plane);
    };
    auto graphs = [&](auto has_out) {
        constexpr bool vst = VST && decltype(has_out)::value;
        constexpr bool direct_store = !VST && decltype(has_out)::value;
#pragma unroll
        for (int s = 0; s < GPT; ++s) {
            const int g = g0 + s;
            if (g >= B) break;  // workgroup-uniform
            // this lane's adjacency rows: node 32*io + (lane & 31), word ii, for the whole graph (one latency)
            uint32_t mw[SB][SB];
            auto load_masks = [&](int io, uint32_t (&m)[SB]) {
                const int node = 32 * io + c;
                const bool ok = node < T;
#pragma unroll
                for (int ii = 0; ii < SB; ++ii) {
                    const bool okw = ok && ii < W;
                    const uint32_t v = a.rowmask[okw ? ((int64_t)g * T + node) * W + ii : 0];
                    m[ii] = okw ? v : 0u;
                }
            };
            if constexpr (WEIGHTED) {
                if (s == 0) fetch_w(g, 0, 0), fetch_w(g, 0, 1);   // (later graphs: requested under the previous graph's last block row)
            } else {
#pragma unroll
                for (int io = 0; io < SB; ++io) load_masks(io, mw[io]);
            }
            float vmax[RN], vmin[RN], pmax_a[RN], pmax_b[RN];
#pragma unroll
            for (int j = 0; j < RN; ++j) { vmax[j] = -INFINITY; vmin[j] = INFINITY; pmax_a[j] = -INFINITY; pmax_b[j] = -INFINITY; }
#pragma unroll
            for (int io = 0; io < SB; ++io) {
                const int node0 = 32 * io;
                if (node0 >= T) break;  // workgroup-uniform: block of padding rows
                bf16x8 af[WEIGHTED ? 1 : SB][2];
                float rinv[16];
                if constexpr (WEIGHTED) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) rinv[r] = 1.0f;   // D is inside the operand
                } else {
                    int deg = 0;
#pragma unroll
                    for (int ii = 0; ii < SB; ++ii) {
                        deg += __popc(mw[io][ii]);
                        expand_mask(mw[io][ii] >> (4 * h), af[ii]);
                    }
                    const float inv = 1.0f / (float)(deg + 1);                  // gcn.py:35
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row0 = (r & 3) + 8 * (r >> 2);
                        rinv[r] = __int_as_float(__builtin_amdgcn_ds_bpermute(perm_base + 4 * row0, __float_as_int(inv)));
                    }
                }
#pragma unroll
                for (int j = 0; j < RN; ++j) {
                    // wavefront-uniform: column tile past F (WEIGHTED: a live wavefront computes it unstored -- the requests for the next
                    // block row ride in the last tile's products, and a branch around them would stall them: fetch_w)
                    if (!WEIGHTED && nt0 + j >= n_tiles_total) break;
                    f32x16 y;
#pragma unroll
                    for (int r = 0; r < 16; ++r) y[r] = 0.0f;
                    if constexpr (WEIGHTED) {
                        const bool last_tile = j == RN - 1;   // its products free the fragments for the next block row's
#pragma unroll
                        for (int t = 0; t < 3; ++t) {   // Mlo.Hhi, Mhi.Hlo, Mhi.Hhi: small terms first
                            const int pm = t == 0 ? 1 : 0, ph = t == 1 ? 1 : 0;
#pragma unroll
                            for (int ii = 0; ii < SB; ++ii) {
                                if (ii >= W) break;   // workgroup-uniform
#pragma unroll
                                for (int ks = 0; ks < 2; ++ks)
                                    y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[pm][ii][ks], hf[s * SB + ii][j][ph][ks], y, 0, 0, 0);   // gcn.py:41
                            }
                            if (last_tile && t == 0) fetch_next_w(s, io, 1);
                            if (last_tile && t == 2) fetch_next_w(s, io, 0);
                        }
                    } else {
#pragma unroll
                        for (int p = 1; p >= 0; --p)  // small plane first
#pragma unroll
                            for (int ii = 0; ii < SB; ++ii)
#pragma unroll
                                for (int ks = 0; ks < 2; ++ks)
                                    y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ii][ks], hf[s * SB + ii][j][p][ks], y, 0, 0, 0);   // gcn.py:41
                    }
                    float *tile = decltype(has_out)::value ? out + ((int64_t)g * T + node0) * ldo + (nt0 + j) * NT : nullptr;
                    const float sg = store_gate ? vsg[s][j] : 1.0f;
                    const float bj = bias ? vb[j] : 0.0f;
                    const float gaj = pool_gate_a ? vga[s][j] : 1.0f, gbj = pool_gate_b ? vgb[s][j] : 1.0f;
                    const uint32_t didx0 = DROP ? (uint32_t)(((int64_t)g * T + node0 + 4 * h) * F + (nt0 + j) * NT + c) : 0u;   // element of row 4h of the block
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row0 = (r & 3) + 8 * (r >> 2);  // this lane's row is row0 + 4h
                        const float v = y[r] * rinv[r] + bj;      // gcn.py:41,43
                        float vs = v * sg;
                        if constexpr (DROP) {
                            const uint32_t hh = drop_hash(didx0 + (uint32_t)(row0 * F), a.drop.seed_lo, a.drop.seed_hi);
                            vs *= drop_keep(hh, a.drop.sel[0], a.drop.thr, a.drop.scale);
                            if (node0 + row0 + 4 * h < T) {
                                pmax_a[j] = fmaxf(pmax_a[j], v * gaj * drop_keep(hh, a.drop.sel[1], a.drop.thr, a.drop.scale));
                                pmax_b[j] = fmaxf(pmax_b[j], v * gbj * drop_keep(hh, a.drop.sel[2], a.drop.thr, a.drop.scale));
                            }
                        }
                        if (vst) stage_lds[(row0 + 4 * h) * 64 + ((32 * j + c) ^ (32 * h))] = vs;
                        if (node0 + row0 + 4 * h < T) {
                            if (direct_store && col_ok[j]) tile[lane_off + row0 * ldo] = vs;
                            if constexpr (!DROP) {
                                vmax[j] = fmaxf(vmax[j], v);
                                vmin[j] = fminf(vmin[j], v);
                            }
                        }
                    }
                }
                if (vst) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    const int colq = (lane & 15) * 4;
                    const int gcol = nt0 * NT + colq;
                    float *gbase = out + ((int64_t)g * T + node0) * ldo + gcol;
#pragma unroll
                    for (int it = 0; it < 8; ++it) {
                        const int row = 4 * it + (lane >> 4);
                        const float4 v4 = *reinterpret_cast<const float4 *>(&stage_lds[row * 64 + (colq ^ (32 * ((row >> 2) & 1)))]);
                        if (node0 + row < T && gcol < F) store_out4(gbase + row * ldo, v4);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
            // pools of graph g: max over ALL its rows (bert_amir5.py:635-640), both gates from max and min of y
            float dot = 0.0f;
#pragma unroll
            for (int j = 0; j < RN; ++j) {
                if (nt0 + j >= n_tiles_total) break;
                float pa, pb;
                if constexpr (DROP) {
                    pa = fmaxf(pmax_a[j], upper_half_to_lower(pmax_a[j]));
                    pb = fmaxf(pmax_b[j], upper_half_to_lower(pmax_b[j]));
                } else {
                    const float mx = fmaxf(vmax[j], upper_half_to_lower(vmax[j]));
                    const float mn = fminf(vmin[j], upper_half_to_lower(vmin[j]));
                    const float ga = pool_gate_a ? vga[s][j] : 1.0f, gb = pool_gate_b ? vgb[s][j] : 1.0f;
                    pa = ga * (ga >= 0.0f ? mx : mn);
                    pb = gb * (gb >= 0.0f ? mx : mn);
                }
                if (h == 0 && col_ok[j]) {
                    const int gn = (nt0 + j) * NT + c;
                    if (pool_a) pool_a[(int64_t)g * F + gn] = pa;
                    if (pool_b) pool_b[(int64_t)g * F + gn] = pb;
                    dot = fmaf(pa, pb, dot);
                }
            }
            if (ov_partial && nt0 < n_tiles_total) {
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) dot += __shfl_xor(dot, d);
                if (lane == 0) ov_partial[(int64_t)g * ((F + 63) / 64) + (nt0 >> 1)] = dot;
            }
        }
    };
    if (WEIGHTED && nt0 >= n_tiles_total) return;   // wavefront-uniform: both column tiles past F (no barrier follows the main loop)
    if (out) graphs(std::true_type{});
    else graphs(std::false_type{});
}


// ggcn_graph_operands_weighted_wide: a REAL-valued adjacency of graphs of 33..128 nodes as the WEIGHTED kernel's A operands.
// M = D.A_w with D = diag(1 / (rowsum(A_w) + 1)) (gcn.py:35) folded in; bf16 keeps fp32's exponent, so no power-of-two scale
// rides along (the <= 32-node form scales by 2^10 for its fp16 planes).  One wavefront per 32 x 32 block (graph, io, ii):
// lane (r, h) walks row 32 io + r of the CSR -- the whole row, in CSR order, so that its rowsum is the number ggcn_aggregate
// and ggcn_inv_denominators compute -- and keeps the 16 columns of block column ii its fragments hold.  Rows >= T and columns
// >= T stay zero.  flag (optional): bit 0 when an entry is not finite (rowsum + 1 == 0 makes every entry of the row inf or NaN).
__global__ __launch_bounds__(256) void graph_operands_ww_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                                const float *__restrict__ vals, int B, int T, int W, char *__restrict__ ops,
                                                                int *__restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int WW = W * W;
    if (blk >= (int64_t)B * WW) return;   // wavefront-uniform
    const int g = (int)(blk / WW), io = (int)(blk % WW) / W, ii = (int)(blk % WW) % W;
    const int r = lane & 31, h = lane >> 5;
    const int64_t node0 = (int64_t)g * T;
    const int row = 32 * io + r;
    float a[16], wsum = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = 0.0f;
    if (row < T) {
        auto take = [&](int col, float w) {
            const int c = col - (int)node0 - 32 * ii;
            wsum += w;
            // column c of the block sits in k-step c >> 4 as element 4 ((c >> 3) & 1) + (c & 3) of the lane half (c >> 2) & 1
            const int idx = ((unsigned)c < 32u && ((c >> 2) & 1) == h) ? (c >> 4) * 8 + ((c >> 3) & 1) * 4 + (c & 3) : -1;
#pragma unroll
            for (int q = 0; q < 16; ++q) a[q] += idx == q ? w : 0.0f;
        };
        const int e1 = rowptr[node0 + row + 1];
        int e = rowptr[node0 + row];
        for (; e + 4 <= e1; e += 4) {   // four edges per trip, their loads in flight together (a dense row is 128 dependent trips otherwise); CSR order kept
            int cj[4];
            float wj[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { cj[q] = colidx[e + q]; wj[q] = vals ? vals[e + q] : 1.0f; }
#pragma unroll
            for (int q = 0; q < 4; ++q) take(cj[q], wj[q]);
        }
        for (; e < e1; ++e) take(colidx[e], vals ? vals[e] : 1.0f);
    }
    const float inv = 1.0f / (wsum + 1.0f);   // gcn.py:35
    char *dst = ops + blk * kWOpsBlock;
    bool bad = false;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        union { uint4 q; unsigned short u[8]; } hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = a[8 * s + e] * inv;
            bad = bad || !(fabsf(v) < 3.0e38f);
            const __bf16 vh = (__bf16)v, vl = (__bf16)(v - (float)vh);
            hi.u[e] = __builtin_bit_cast(unsigned short, vh);
            lo.u[e] = __builtin_bit_cast(unsigned short, vl);
        }
        *reinterpret_cast<uint4 *>(dst + s * 1024 + lane * 16) = hi.q;
        *reinterpret_cast<uint4 *>(dst + 2048 + s * 1024 + lane * 16) = lo.q;
    }
    if (bad && flag) atomicOr(flag, 1);
}

}  // namespace

int launch_fused_wide(const char *who, const FusedArgs &a, int precision, int sb, bool fast, bool vst, int64_t gridw, hipStream_t st)
{
#define GGCN_LAUNCHW(SC, AV, KF, VS, SBV, DR) \
    hipLaunchKernelGGL((layer_fused_wide_kernel<SC, AV, KF, VS, SBV, DR>), dim3((unsigned)gridw), dim3(kThreads), 0, st, a)
#define GGCN_PICKWD(SC, SBV, DR)                                             \
    do {                                                                     \
        if (fast && vst) GGCN_LAUNCHW(SC, true, true, true, SBV, DR);        \
        else if (fast) GGCN_LAUNCHW(SC, true, true, false, SBV, DR);         \
        else GGCN_LAUNCHW(SC, false, false, false, SBV, DR);                 \
    } while (0)
#define GGCN_PICKW(SC, SBV)                                                  \
    do {                                                                     \
        if (a.drop.thr != 0) GGCN_PICKWD(SC, SBV, true);                     \
        else GGCN_PICKWD(SC, SBV, false);                                    \
    } while (0)
    if (a.Xb) {   // bf16 features (bf16x3 image): the fast shape or the general form per slot size and DROP
        if (sb != 2 && sb != 4) return fail(GGCN_EUNSUPPORTED, "%s: no %d-row graph slot for bf16 features in this build", who, 32 * sb);
#define GGCN_LAUNCHWB(AV, KF, VS, SBV, DR) \
    hipLaunchKernelGGL((layer_fused_wide_kernel<0, AV, KF, VS, SBV, DR, __bf16>), dim3((unsigned)gridw), dim3(kThreads), 0, st, a)
#define GGCN_PICKWB(SBV, DR)                                                 \
    do {                                                                     \
        if (fast && vst) GGCN_LAUNCHWB(true, true, true, SBV, DR);           \
        else GGCN_LAUNCHWB(false, false, false, SBV, DR);                    \
    } while (0)
        if (a.drop.thr != 0) { if (sb == 2) GGCN_PICKWB(2, true); else GGCN_PICKWB(4, true); }
        else { if (sb == 2) GGCN_PICKWB(2, false); else GGCN_PICKWB(4, false); }
#undef GGCN_PICKWB
#undef GGCN_LAUNCHWB
        return check_launch(who);
    }
    if (sb != 2 && sb != 4) return fail(GGCN_EUNSUPPORTED, "%s: no %d-row graph slot in this build", who, 32 * sb);
    if (precision == GGCN_PREC_F16MX8) { if (sb == 2) GGCN_PICKW(1, 2); else GGCN_PICKW(1, 4); }
    else { if (sb == 2) GGCN_PICKW(0, 2); else GGCN_PICKW(0, 4); }
#undef GGCN_PICKW
#undef GGCN_PICKWD
#undef GGCN_LAUNCHW
    return check_launch(who);
}

// gcn.py:30-45 with a real-valued adjacency for graphs of 33..128 nodes in ONE launch: layer_fused_wide_kernel<.., WEIGHTED> on
// ggcn_graph_operands_weighted_wide blocks (a.graph_ops; no row masks).  The shape and the part are checked by fused_part_checks
// (fused_layer.hip), as launch_fused's are.  a.drop: the gates' keep streams (thr = 0: the launch without dropout)
int launch_fused_weighted_wide(const char *who, FusedArgs &a, int precision, hipStream_t st)
{
    if (precision != GGCN_PREC_BF16X3 && precision != GGCN_PREC_F16MX8)
        return fail(GGCN_EUNSUPPORTED, "%s: precision %d (bf16x3 or f16mx8)", who, precision);
    if (!a.X) return fail(GGCN_EINVAL, "%s: null input pointer", who);
    if (!a.graph_ops) return fail(GGCN_EINVAL, "%s: the weighted operand blocks are required", who);
    if (!aligned16(a.graph_ops)) return fail(GGCN_EINVAL, "%s: the operand blocks must be 16-byte aligned", who);
    bool vst;
    if (int rc = fused_part_checks(who, a, vst)) return rc;
    if (a.T <= 32) return fail(GGCN_EUNSUPPORTED, "%s: T=%d <= 32 (ggcn_layer_fused_weighted)", who, a.T);
    if (a.T > 128) return fail(GGCN_EUNSUPPORTED, "%s: T=%d > 128 (use ggcn_linear + ggcn_aggregate)", who, a.T);
    const bool fast = (a.K % 4 == 0) && (a.ldx % 4 == 0) && aligned16(a.X) && (int64_t)a.ldx * 4 * 257 < ((int64_t)1 << 31) && (a.K % BK == 0);
    a.k_steps = round_up(a.K, BK) / KSTEP;
    a.n_wg = (a.F + BN - 1) / BN;
    const int sb = a.T <= 64 ? 2 : 4;
    const int64_t gt = sb == 2 ? ((int64_t)a.B + 1) / 2 : a.B;   // two graphs per workgroup in the 64-row slot
    const int64_t gridw = grid_for(gt, a.n_wg);
    if (gridw > (int64_t)INT32_MAX) return fail(GGCN_EUNSUPPORTED, "%s: batch too large", who);
    a.g_tiles = (int)gt;
#define GGCN_LAUNCHWW(SC, AV, KF, VS, SBV, DR) \
    hipLaunchKernelGGL((layer_fused_wide_kernel<SC, AV, KF, VS, SBV, DR, float, true>), dim3((unsigned)gridw), dim3(kThreads), 0, st, a)
#define GGCN_PICKWWD(SC, SBV, DR)                                            \
    do {                                                                     \
        if (fast && vst) GGCN_LAUNCHWW(SC, true, true, true, SBV, DR);       \
        else if (fast) GGCN_LAUNCHWW(SC, true, true, false, SBV, DR);        \
        else GGCN_LAUNCHWW(SC, false, false, false, SBV, DR);                \
    } while (0)
#define GGCN_PICKWW(SC, SBV)                                                 \
    do {                                                                     \
        if (a.drop.thr != 0) GGCN_PICKWWD(SC, SBV, true);                    \
        else GGCN_PICKWWD(SC, SBV, false);                                   \
    } while (0)
    if (precision == GGCN_PREC_F16MX8) { if (sb == 2) GGCN_PICKWW(1, 2); else GGCN_PICKWW(1, 4); }
    else { if (sb == 2) GGCN_PICKWW(0, 2); else GGCN_PICKWW(0, 4); }
#undef GGCN_PICKWW
#undef GGCN_PICKWWD
#undef GGCN_LAUNCHWW
    return check_launch(who);
}

GGCN_RANGE_FLAG_TU(range_flag_wide)

}  // namespace ggcn

using namespace ggcn;

extern "C" {

size_t ggcn_graph_operands_weighted_wide_bytes(int B, int T)
{
    if (B <= 0 || T <= 32 || T > 128) return 0;
    const size_t W = (size_t)(T + 31) / 32;
    return (size_t)B * W * W * kWOpsBlock;
}

int ggcn_graph_operands_weighted_wide(const int32_t *rowptr, const int32_t *colidx, const float *vals, int B, int T, void *ops,
                                      int32_t *flag, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const char *who = "ggcn_graph_operands_weighted_wide";
    if (!rowptr || !colidx || !ops) return fail(GGCN_EINVAL, "%s: null pointer", who);
    if (B <= 0 || T <= 0) return fail(GGCN_EINVAL, "%s: B=%d T=%d must be positive", who, B, T);
    if (T <= 32) return fail(GGCN_EUNSUPPORTED, "%s: T=%d <= 32 (one block per graph: ggcn_graph_operands_weighted)", who, T);
    if (T > 128) return fail(GGCN_EUNSUPPORTED, "%s: T=%d > 128 (weighted graphs of more nodes: ggcn_linear + ggcn_aggregate)", who, T);
    if (!aligned16(ops)) return fail(GGCN_EINVAL, "%s: the blocks must be 16-byte aligned", who);
    if ((int64_t)B * T >= (int64_t)INT32_MAX) return fail(GGCN_EUNSUPPORTED, "%s: B*T does not fit int32 node ids", who);
    const int W = (T + 31) >> 5;
    const int64_t grid = ((int64_t)B * W * W + 3) / 4;
    if (grid > (int64_t)INT32_MAX) return fail(GGCN_EUNSUPPORTED, "%s: batch too large", who);
    hipLaunchKernelGGL(graph_operands_ww_kernel, dim3((unsigned)grid), dim3(256), 0, st, rowptr, colidx, vals, B, T, W, static_cast<char *>(ops), flag);
    return check_launch(who);
}

}  // extern "C"
