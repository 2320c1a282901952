// What ggcn_block_fused runs for large batches (the headline's kernel; ggcn_lab_block_fused8 reaches it directly): the two-layer
// block with ONE workgroup of EIGHT wavefronts per (row block, 256-column slice) that shares a row block's X planes between its W1
// and its W12 column tiles.  Dispatch rule (block8_shape / block8_takes below, ggcn_block_fused_form): every output of the block
// (no gcn1), f16mx8, T <= 32, K % 32 == 0, F a multiple of 256, 16-byte aligned operands, and a batch that makes >= 6 rounds of
// one workgroup per CU or >= 3 whole rounds (2048 x 768 and up; 1024 x 768); GGCN_BLOCK_FORM=4 keeps the four-wavefront kernel.
// Wavefronts 0-3 (group 0) own the slice's W1 tiles, wavefronts 4-7 (group 1) its W12 tiles; every thread stages 2
// of the stage's 4 passes (mx8::mainloop<..., XP = 2>), so X is loaded, split and written to LDS once for both layers -- half the
// X-side work per output (48 + 24 us of the elimination ladder) and one fetch of X per slice instead of one per part.
// What it gives up is what DESIGN.md 5b says it gives up: 8 x 235 registers fill the CU, so ONE workgroup is resident and both
// groups' epilogues run under nothing.  Block ids that share an XCD take a contiguous run of (slice-major) work items, so an XCD
// holds at most two column slices of both weight images (2.5 MB of its 4 MiB L2) -- the price: a row block's three slices sit on
// three XCDs.  Same tiles, same arithmetic, same order as the four-wavefront kernel: results are bit-identical (tests).
#include "fused_common.h"

#include <cstdlib>

namespace ggcn {
namespace {

constexpr int kB8Threads = 512;
constexpr int kB8Lds = kLdsBytes + 2 * kEpiLdsBytes;   // one set of stage buffers, two sets of epilogue operands: 94.5 KiB

__device__ __forceinline__ bool getenv_slot_same(const FusedArgs &a) { return (a.k_steps & 0x20000000) != 0; }   // (lab: both groups stage behind slots 0, 1)

// max |mid bias| of the slice from the W12 group's staged operands (LDS-DMA: the raw row, reduced per wavefront; else the
// per-wavefront maxima stage_epilogue_operands left) -- what dma_range_verdict / fused_range_verdict read
template <int BASE>
__device__ __forceinline__ float staged_mid_max(const char *lds, bool dma, int lane)
{
    if (dma) {
        const float4 m4 = *reinterpret_cast<const float4 *>(lds + EpiLds<BASE>::kBias + BN * 4 + lane * 16);
        float mm = fmaxf(fmaxf(fabsf(m4.x), fabsf(m4.y)), fmaxf(fabsf(m4.z), fabsf(m4.w)));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mm = fmaxf(mm, __shfl_xor(mm, d));
        return mm;
    }
    const float4 mm = *reinterpret_cast<const float4 *>(lds + EpiLds<BASE>::kMidMax);
    return fmaxf(fmaxf(mm.x, mm.y), fmaxf(mm.z, mm.w));
}

template <bool FULLT, bool VST>
__global__ __launch_bounds__(kB8Threads, 1) void block_fused8_kernel(const FusedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int B = a.B, T = a.T, K = a.K, F = a.F;
    // work item w = n_wgi * g_tiles + g_tile (slice-major); XCD x (= id & 7: observed dispatch, speed only) takes a contiguous run
    int n_wgi, g_tile;
    if (a.n_parts == 2) {
        const int xcd = blockIdx.x & 7, qb = blockIdx.x >> 3;
        const int total = a.g_tiles * a.n_wg, per_xcd = (total + 7) >> 3;
        const int w = xcd * per_xcd + qb;
        if (qb >= per_xcd || w >= total) return;   // whole workgroup, before any barrier
        n_wgi = w / a.g_tiles;
        g_tile = w - n_wgi * a.g_tiles;
    } else {   // (GGCN_LAB_BLOCK8_ROWMAJOR=1: a row block's slices on ONE XCD -- X fetched once, both weight images in every L2)
        if (!tile_of_block(blockIdx.x, a.g_tiles, a.n_wg, g_tile, n_wgi)) return;
    }

    const int tid8 = threadIdx.x;
    const unsigned long long t_start = a.stamps ? __builtin_amdgcn_s_memrealtime() : 0;   // (lab: phase stamps in 10 ns ticks, per group)
    const int group = __builtin_amdgcn_readfirstlane(tid8 >> 8);   // 0: the W1 tiles, 1: the W12 tiles (wavefront-uniform)
    const int tid = tid8 & 255;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const LayerPart &lp = a.part[group];
    const int gt0 = g_tile * 4, g0 = gt0;
    const int n_tiles_total = (F + NT - 1) / NT;
    const int nt0 = n_wgi * (BN / NT) + wave * RN;

    // this thread's two staging passes: passes 2 group, 2 group + 1 of the tile (pass p = rows 32 p .. 32 p + 31 = graph gt0 + p)
    constexpr int NP = Geom<float>::NP;
    const float *arow[NP];
    bool avalid[NP];
    int rel[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int row = stage_row<float>(i < 2 ? i + 2 * group : 0);
        const int g = gt0 + (row >> 5), r = row & 31;
        avalid[i] = i < 2 && (g < B) && (FULLT || r < T);
        arow[i] = a.X;   // (buffer path only)
        rel[i] = avalid[i] ? (row >> 5) * T + (row & 31) : -1;
    }
    // whole tiles take the LDS-DMA staging (workgroup-uniform; a.k_steps & 1 carries the launcher's alignment verdict)
    const bool dma = (a.n_wg * BN == F) && (gt0 + 4 <= B) && a.ov_in == nullptr && a.ov_out == nullptr && (a.k_steps & 0x40000000) != 0;
    const int k_steps = a.k_steps & 0x0fffffff;
    if (dma) {
        if (group == 0) stage_epilogue_operands_dma<kLdsBytes>(a, lp, g0, n_wgi, lds, tid);
        else stage_epilogue_operands_dma<kLdsBytes + kEpiLdsBytes>(a, lp, g0, n_wgi, lds, tid);
    } else {
        if (group == 0) stage_epilogue_operands<kLdsBytes>(a, lp, g0, n_wgi, lds, tid);
        else stage_epilogue_operands<kLdsBytes + kEpiLdsBytes>(a, lp, g0, n_wgi, lds, tid);
    }

    f32x16 acc[4][RN];
    float amax;
    const int64_t pack_bytes = (int64_t)n_tiles_total * (k_steps / 2) * mx8::STAGE_PACK_BYTES;
    // both weight images' hidden-value factors (their trailers), asked for before the main loop: no load waits behind it
    const float bw1 = *reinterpret_cast<const float *>(a.part[0].wpack + pack_bytes);
    const float bw12 = *reinterpret_cast<const float *>(a.part[1].wpack + pack_bytes);
    const unsigned long long t_loop0 = a.stamps ? __builtin_amdgcn_s_memrealtime() : 0;
    mx8::BufX<float> bx = mx8::make_bufx<float>(a.X, a.ldx, (int64_t)gt0 * T, (int64_t)B * T, rel, tid);
    // kBlock8Prio: the second-dispatched half of the workgroup -- the W12 group, whose epilogue is the longer one -- above its SIMD
    // partner in the issue arbitration, once and for the whole launch (the two groups' epilogues then end together: DESIGN.md 5b)
    if (group == 1 && (a.k_steps & 0x10000000) != 0) __builtin_amdgcn_s_setprio(1);
    // (two instantiations that meet at the same barriers: group 1's staging passes sit behind the stage's LAST two row blocks)
    if (group == 0 || getenv_slot_same(a))
        mx8::mainloop<float, true, true, !FULLT, false, true, 4, false, 2, 0>(arow, avalid, lp.wpack, K, k_steps / 2, 0, nt0, n_tiles_total, lds, acc, 0, 4,
                                                                               &amax, &bx, 1.0f, 2 * group);
    else
        mx8::mainloop<float, true, true, !FULLT, false, true, 4, false, 2, 2>(arow, avalid, lp.wpack, K, k_steps / 2, 0, nt0, n_tiles_total, lds, acc, 0, 4,
                                                                               &amax, &bx, 1.0f, 2 * group);
    unsigned long long t_loop1 = 0;
    if (a.stamps) { asm volatile("" :: "v"(acc[3][RN - 1][15])); t_loop1 = __builtin_amdgcn_s_memrealtime(); }
    // Each row of the tile is split by ONE group (group 0: graphs gt0, gt0 + 1; group 1: gt0 + 2, gt0 + 3), so each group judges
    // its amax against BOTH weight images' hidden-value bounds -- W1's, and W12's plus max |mid| from group 1's staged mid row
    // (written before the main loop; its barriers make it visible to all eight wavefronts, and no epilogue writes it)
    mx8::range_verdict(amax, bw12, staged_mid_max<kLdsBytes + kEpiLdsBytes>(lds, dma, tid & 63), true);
    mx8::range_verdict(amax, bw1, 0.0f, false);
    if (group == 0) {
        epilogue<1, FULLT, VST, false, false, kLdsBytes>(a, lp, acc, g0, nt0, n_tiles_total, lds, tid);
    } else {
        if (lp.out) epilogue<1, FULLT, VST, true, true, kLdsBytes + kEpiLdsBytes>(a, lp, acc, g0, nt0, n_tiles_total, lds, tid);
        else epilogue<1, FULLT, VST, true, false, kLdsBytes + kEpiLdsBytes>(a, lp, acc, g0, nt0, n_tiles_total, lds, tid);
    }
    if (a.stamps && tid == 0) {
        unsigned long long *o = a.stamps + ((size_t)blockIdx.x * 2 + group) * 4;
        o[0] = t_start; o[1] = t_loop0; o[2] = t_loop1; o[3] = __builtin_amdgcn_s_memrealtime();
    }
}

}  // namespace

// What ggcn_block_fused hands to this kernel (fused_layer.hip): the whole block with all of its outputs, f16mx8, on batches that
// make 6 and more rounds of one eight-wavefront workgroup per CU (or 3 and more whole rounds).  There, with the board at its power
// cap, the X planes staged once for a W1 and a W12 column slice are worth 2 % of the launch IN STEADY STATE (each form alone for
// 1.5 s: 603-604 vs 615-618 us at 4096 graphs on two boxes, 639 vs 653 on a slower one, 304-309 vs 313 at 2048; 512 graphs: 85 vs
// 80 us, so shards keep the four-wavefront kernel) -- while five-launch interleaved timings had shown it 3-6 % SLOWER:
// the power controller averages over milliseconds, and the benchmark's timed region is a steady state.
// One eight-wavefront workgroup per CU: a partial last round costs a whole one (1536 graphs = 4.5 rounds: 243 vs 237 us), so the
// kernel is taken from 6 rounds up (2048 graphs x 768 columns) or for 3 and more WHOLE rounds (1024 graphs: 149.5 vs 152-153 us).
int device_cu_count()
{
    static int cus = 0;   // (one device kind per process: MI355X, 256)
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus = n;
    }
    return cus;
}
// the shape's share of the rule (ggcn_block_fused_form: what bench.py labels its roofline line with, what the tests ask)
bool block8_shape(int B, int T, int K, int F)
{
    if (B <= 0 || T > 32 || T <= 0 || F <= 0 || K <= 0 || F % BN != 0 || K % BK != 0) return false;
    const int64_t total = (int64_t)((B + 3) / 4) * (F / BN), cus = device_cu_count();
    return total >= 6 * cus || (total >= 3 * cus && total % cus == 0);
}
// the fast shape of X (buffer loads: a tile's rows at 32-bit byte offsets from its first row) and, for the LDS-DMA staging of the
// epilogue's operands (the form that was measured), every gate / bias row and operand block this launch reads 16-byte aligned
static bool block8_fast_x(const FusedArgs &a)
{
    return (a.K % BK == 0) && (a.ldx % 4 == 0) && aligned16(a.X) && (int64_t)a.ldx * 4 * 257 < ((int64_t)1 << 31);
}
static bool block8_dma_aligned(const FusedArgs &a)
{
    const LayerPart &l1 = a.part[0], &l2 = a.part[1];
    return aligned16(l1.pool_gate_a) && aligned16(l2.store_gate) && aligned16(l1.bias) && aligned16(l2.bias) && aligned16(l2.mid) &&
           aligned16(a.graph_ops) && aligned16(a.graph_ops2);
}
// a: the block as launch_block (fused_layer.hip) holds it, layer 1 in part[0] and layer 2 in part[1]
bool block8_takes(const FusedArgs &a)
{
    const LayerPart &l1 = a.part[0], &l2 = a.part[1];
    if (!block8_shape(a.B, a.T, a.K, a.F)) return false;
    // what launch_fused would refuse goes there, so that both forms answer a bad call with the same code and message
    if (!a.X || !l1.wpack || !l2.wpack || a.ldx < a.K || !aligned16(l1.wpack) || !aligned16(l2.wpack) || (l2.out && l2.ldo < a.F)) return false;
    if (!block8_fast_x(a)) return false;
    if (!a.graph_ops || !a.graph_ops2 || !l1.pool_gate_a || !l2.store_gate || !l2.mid) return false;
    if (!block8_dma_aligned(a)) return false;
    if (l2.out && !vector_row_stores(a, l2)) return false;
    return true;
}

// hipFuncSetAttribute once per instantiation and device (the call takes a lock of the runtime's and a few microseconds)
template <typename KERN>
static bool block8_reserve_lds(KERN kern)
{
    static bool done[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    if (dev >= 0 && dev < 64 && done[dev]) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kB8Lds) != hipSuccess) return false;
    if (dev >= 0 && dev < 64) done[dev] = true;
    return true;
}

// who: the entry (ggcn_block_fused through launch_block, or ggcn_lab_block_fused8); a: the block, layer 1 in part[0] and layer 2 in part[1].
// flags (fused_args.h kBlock8*): ROWMAJOR = a row block's three column slices on one XCD (the product's map: ggcn_block_fused takes
// this kernel for large batches), else column slices pinned to XCDs; NODMA / SAMESLOTS: lab switches of ggcn_lab_block_fused8; PRIO: the W12
// group of every workgroup at s_setprio 1 (the product sets it; the lab entry on GGCN_LAB_BLOCK8_PRIO, so one process times both)
int block_fused8(const char *who, FusedArgs &a, int flags, hipStream_t st)
{
    LayerPart &l1 = a.part[0], &l2 = a.part[1];
    if (!a.X || !l1.wpack || !l2.wpack || !a.graph_ops || !a.graph_ops2 || !l1.pool_gate_a || !l2.store_gate || !l1.pool_a || !l1.pool_b || !l2.mid)
        return fail(GGCN_EINVAL, "%s: null pointer", who);
    if (a.B <= 0 || a.T <= 0 || a.T > 32 || a.K <= 0 || a.F <= 0)
        return fail(GGCN_EUNSUPPORTED, "%s: B=%d T=%d K=%d F=%d (graphs of <= 32 nodes)", who, a.B, a.T, a.K, a.F);
    if (!l2.out && !l2.pool_a) return fail(GGCN_EINVAL, "%s: neither x nor its pool requested", who);
    // x leaves as 16-byte row stores or not at all (a leading dimension below F is fused_part_checks' to name)
    if (l2.out && l2.ldo >= a.F && !vector_row_stores(a, l2)) return fail(GGCN_EUNSUPPORTED, "%s: x needs F %% 4 == 0 and 16-byte aligned rows", who);
    l1.out = nullptr; l1.ldo = 0;   // (this kernel stores no gcn1)
    bool vst;
    if (int rc = fused_part_checks(who, a, vst)) return rc;
    if (!block8_fast_x(a)) return fail(GGCN_EUNSUPPORTED, "%s: fast shapes only (K %% 32 == 0, 16-byte aligned rows)", who);
    const bool rowmajor = (flags & kBlock8RowMajor) != 0;
    a.n_parts = rowmajor ? 3 : 2;
    a.k_steps = round_up(a.K, BK) / KSTEP;
    // (bit 30 of k_steps: every gate / bias row this launch reads starts 16-byte aligned -- the LDS-DMA staging may be used)
    if ((a.F % 4 == 0) && block8_dma_aligned(a) && !(flags & kBlock8NoDma)) a.k_steps |= 0x40000000;
    if (flags & kBlock8SameSlots) a.k_steps |= 0x20000000;
    if (flags & kBlock8Prio) a.k_steps |= 0x10000000;
    a.n_wg = (a.F + BN - 1) / BN;
    const bool fullt = (a.T == 32) && (a.B % 4 == 0);
    const int64_t g_tiles = ((int64_t)a.B + 3) / 4, total = g_tiles * a.n_wg;   // (in 64 bits: B + 3 may not fit an int)
    const int64_t grid = rowmajor ? grid_for(g_tiles, a.n_wg) : 8 * ((total + 7) / 8);
    if (grid > (int64_t)INT32_MAX) return fail(GGCN_EUNSUPPORTED, "%s: batch too large", who);
    a.g_tiles = (int)g_tiles;
#define GGCN_L8(FT, VS)                                                                                                           \
    do {                                                                                                                          \
        auto kern = block_fused8_kernel<FT, VS>;                                                                                  \
        if (!block8_reserve_lds(kern)) return fail(GGCN_ELAUNCH, "%s: cannot reserve %d bytes of LDS", who, kB8Lds);              \
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kB8Threads), kB8Lds, st, a);                                          \
    } while (0)
    if (fullt && vst) GGCN_L8(true, true);
    else if (fullt) GGCN_L8(true, false);
    else if (vst) GGCN_L8(false, true);
    else GGCN_L8(false, false);
#undef GGCN_L8
    return check_launch(who);
}

GGCN_RANGE_FLAG_TU(range_flag_block8)

}  // namespace ggcn
