// Sub-word -> word pooling: Y[b, r, :] = sum_c A[b, r, c] * X[b, c, :]
// (models/bert_amir5.py:600 `torch.bmm(transform, x)`, the step right before the BiLSTM; the
// transform of data_utils.py:749-766 holds 1/l over the l sub-word positions of word r and zeros
// elsewhere, while x is 12 x 768 = 9216 features wide).  The dense product multiplies ~97 % zeros
// and reads every X row R times; here one workgroup per (b, r, 1024-feature slab) scans the dense
// row of A once, keeps its non-zeros (ascending c: a fixed summation order) in LDS and streams only
// the selected rows of X: HBM-bound, X is read once per word it belongs to.
// A is addressed with element strides, so the reference's non-contiguous slice
// `inputs['transform'][:, :T, :L]` is taken as it is, and the transposed product of the backward
// pass (dX = A^T . dY) is the same launch with the two strides swapped.
// XT = __bf16 (ggcn_subword_pool_bf16, x from BERT under bf16 autocast): X and Y in bf16, the sums in fp32, Y rounded to
// nearest even once -- what torch.bmm gives under autocast.
// ggcn_subword_pool_layers reads x where BERT left it: the 12 layer outputs of bert_amir5.py:596, before their `torch.cat`, each
// pooled into its own 768 columns of Y by ONE launch -- the same compaction and the same two loop bodies, so a layer's columns
// are bit for bit those of ggcn_subword_pool on that layer alone, and the 9216-wide copy is never made.
// ggcn_anchor_pool_layers serves the baselines bert_ed / bertdm, which keep of all pooled rows only the anchor's and two masked
// max-pools: one launch from the layer list to [B, 3*n*Dl], the pooled rows held in registers and never stored.
#include "common.h"

namespace ggcn {
namespace {

constexpr int kMaxCols = 2048;  // columns of A per row held in LDS as (index, value) pairs
constexpr int kSlab = 1024;     // features per workgroup: 256 threads x 4

typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 load4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 load4(const __bf16 *p)
{
    const bf16x4_t v = *reinterpret_cast<const bf16x4_t *>(p);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
__device__ __forceinline__ void store4(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ void store4(__bf16 *p, const float4 &v)
{
    *reinterpret_cast<bf16x4_t *>(p) = bf16x4_t{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
}

// What a workgroup keeps of its row of A: the non-zeros as (column, value) pairs, ascending column.
struct alignas(16) RowLds {   // (16-byte aligned: the loops read four pairs with one ds_read_b128 each)
    alignas(16) int idx[kMaxCols];
    alignas(16) float val[kMaxCols];
    int wave[4];
    int total;
};

// Compact the non-zeros of the row `arow` (C columns, sa_c elements apart) into `s`, ascending column, 256 columns per round.
// Called by all 256 threads; returns the number kept (the same in every thread, `s` is complete on return).
__device__ __forceinline__ int compact_row(RowLds &s, const float *__restrict__ arow, int64_t sa_c, int C)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s.total = 0;
    __syncthreads();
    for (int c0 = 0; c0 < C; c0 += 256) {
        const int c = c0 + tid;
        const float v = c < C ? arow[c * sa_c] : 0.0f;
        const bool nz = v != 0.0f;
        const unsigned long long m = __ballot(nz);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s.wave[wave] = __popcll(m);
        __syncthreads();
        int off = s.total;
        for (int w = 0; w < wave; ++w) off += s.wave[w];
        if (nz) {
            s.idx[off + before] = c;
            s.val[off + before] = v;
        }
        __syncthreads();
        if (tid == 0) s.total += s.wave[0] + s.wave[1] + s.wave[2] + s.wave[3];
        __syncthreads();
    }
    return s.total;
}

// The two loop bodies: one thread, four adjacent features (vector form) or one (scalar form) of the n kept rows of xb,
// from 0, one fmaf per kept entry in ascending column.
template <typename XT>
__device__ __forceinline__ float4 pooled4(const RowLds &s, int n, const XT *__restrict__ xb, int64_t ldx, int f)
{
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int e = 0;
    for (; e + 1 < n; e += 2) {  // two rows in flight
        const float4 x0 = load4(xb + (int64_t)s.idx[e] * ldx + f);
        const float4 x1 = load4(xb + (int64_t)s.idx[e + 1] * ldx + f);
        const float v0 = s.val[e], v1 = s.val[e + 1];
        acc.x = fmaf(v0, x0.x, acc.x); acc.y = fmaf(v0, x0.y, acc.y);
        acc.z = fmaf(v0, x0.z, acc.z); acc.w = fmaf(v0, x0.w, acc.w);
        acc.x = fmaf(v1, x1.x, acc.x); acc.y = fmaf(v1, x1.y, acc.y);
        acc.z = fmaf(v1, x1.z, acc.z); acc.w = fmaf(v1, x1.w, acc.w);
    }
    if (e < n) {
        const float4 x0 = load4(xb + (int64_t)s.idx[e] * ldx + f);
        const float v0 = s.val[e];
        acc.x = fmaf(v0, x0.x, acc.x); acc.y = fmaf(v0, x0.y, acc.y);
        acc.z = fmaf(v0, x0.z, acc.z); acc.w = fmaf(v0, x0.w, acc.w);
    }
    return acc;
}

template <typename XT>
__device__ __forceinline__ float pooled1(const RowLds &s, int n, const XT *__restrict__ xb, int64_t ldx, int f)
{
    float acc = 0.0f;
    for (int e = 0; e < n; ++e) acc = fmaf(s.val[e], (float)xb[(int64_t)s.idx[e] * ldx + f], acc);
    return acc;
}

template <bool VEC, typename XT = float>
__global__ __launch_bounds__(256) void subword_pool_kernel(const float *__restrict__ A, int64_t sa_b, int64_t sa_r,
                                                          int64_t sa_c, const XT *__restrict__ X,
                                                          int64_t x_batch, int64_t ldx, XT *__restrict__ Y,
                                                          int64_t y_batch, int64_t ldy, int R, int C, int D)
{
    __shared__ RowLds s;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / R, r = blockIdx.x % R;
    const int n = compact_row(s, A + b * sa_b + r * sa_r, sa_c, C);
    const XT *xb = X + b * x_batch;
    XT *yrow = Y + b * y_batch + (int64_t)r * ldy;
    if (VEC) {
        const int f = blockIdx.y * kSlab + tid * 4;
        if (f >= D) return;
        store4(yrow + f, pooled4(s, n, xb, ldx, f));
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int fq = blockIdx.y * kSlab + q * 256 + tid;  // coalesced scalar form
            if (fq >= D) continue;
            yrow[fq] = (XT)pooled1(s, n, xb, ldx, fq);
        }
    }
}

// All layers of BERT in one launch (ggcn_subword_pool_layers): Y[b, r, l*Dl + f] = sum_c A[b,r,c] * X_l[b,c,f].  The layers'
// base pointers travel in the kernel's argument block; nothing is written to device memory for them.
struct LayerPtrs {
    const void *p[GGCN_POOL_MAX_LAYERS];
};

constexpr int kUnit = 256;  // features per wavefront: 64 lanes x 4

// One workgroup per (b, r, four units); a unit is 256 adjacent features of ONE layer, so a wavefront's layer is uniform and
// at Dl = 768 (three units a layer) every lane of every wavefront has work.  units = ceil(Dl / 256), per layer.
template <bool VEC, typename XT>
__global__ __launch_bounds__(256) void subword_pool_layers_kernel(const float *__restrict__ A, int64_t sa_b, int64_t sa_r,
                                                                 int64_t sa_c, const LayerPtrs layers, int n_layers,
                                                                 int64_t x_batch, int64_t ldx, XT *__restrict__ Y,
                                                                 int64_t y_batch, int64_t ldy, int R, int C, int Dl, int units)
{
    __shared__ RowLds s;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x / R, r = blockIdx.x % R;
    const int n = compact_row(s, A + b * sa_b + r * sa_r, sa_c, C);
    const int u = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * 4 + (threadIdx.x >> 6)));   // this wavefront's unit
    const int l = u / units;
    if (l >= n_layers) return;
    const int f0 = (u - l * units) * kUnit;
    const XT *xb = static_cast<const XT *>(layers.p[l]) + b * x_batch;
    XT *yrow = Y + b * y_batch + (int64_t)r * ldy + (int64_t)l * Dl;
    if (VEC) {
        const int f = f0 + lane * 4;
        if (f >= Dl) return;
        store4(yrow + f, pooled4(s, n, xb, ldx, f));
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int fq = f0 + q * 64 + lane;  // coalesced scalar form
            if (fq >= Dl) continue;
            yrow[fq] = (XT)pooled1(s, n, xb, ldx, fq);
        }
    }
}

// The baselines' step (ggcn_anchor_pool_layers; models/bert_ed.py:46-62, models/bertdm.py:164-198): of the pooled rows
// v[b, r, :] above only the anchor's row and, with `sides`, the two masked max-pools of bertdm.py:176-185 leave the launch.
// One workgroup per (sentence, four units) walks the sentence's rows in ascending r: the compaction and the pooled values of
// subword_pool_layers_kernel row by row, a select into the anchor registers, an update of one of the two running maxima; it
// stores 3 x (its features) floats once, after the loop.  No atomics, one fixed order: [B, R, n*Dl] never exists.
__device__ __forceinline__ float nan_max(float m, float t) { return (t > m || t != t) ? t : m; }   // torch.max: a NaN stays

template <bool VEC, typename XT>
__global__ __launch_bounds__(256) void anchor_pool_layers_kernel(const float *__restrict__ A, int64_t sa_b, int64_t sa_r,
                                                                int64_t sa_c, const LayerPtrs layers, int n_layers,
                                                                int64_t x_batch, int64_t ldx, const int64_t *__restrict__ anchor,
                                                                const int64_t *__restrict__ length, int sides,
                                                                float *__restrict__ Z, int64_t ldz, int64_t z_section, int R, int C,
                                                                int Dl, int units)
{
    __shared__ RowLds s;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x;
    // read once, clamped (an index outside its range never reaches A or a layer) and uniform: the loop below holds barriers
    const int64_t a64 = anchor[b];
    const int a = __builtin_amdgcn_readfirstlane((int)(a64 < 0 ? 0 : (a64 > R - 1 ? R - 1 : a64)));
    int n = 0;
    if (sides) {                                                    // (sides == 0: `length` is never touched)
        const int64_t n64 = length[b];
        n = __builtin_amdgcn_readfirstlane((int)(n64 < 0 ? 0 : (n64 > R ? R : n64)));
    }
    const int r_first = sides ? 0 : a, r_last = (sides && n - 1 > a) ? n - 1 : a;
    const int u = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * 4 + (threadIdx.x >> 6)));   // this wavefront's unit
    const int l = u / units;
    const bool wave_live = l < n_layers;     // a wavefront past the last unit stays for the barriers of every compaction
    const int f0 = wave_live ? (u - l * units) * kUnit : 0;
    const XT *xb = static_cast<const XT *>(layers.p[wave_live ? l : 0]) + b * x_batch;
    int f[4];
    bool live[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f[q] = VEC ? f0 + lane * 4 + q : f0 + q * 64 + lane;        // (scalar form: coalesced, as subword_pool_layers_kernel)
        live[q] = wave_live && f[q] < Dl;
    }
    const float left0 = a < R - 1 ? 1.0f : -INFINITY;               // a masked word right of the anchor contributes 0 + 1
    float anc[4], left[4], right[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) anc[q] = 0.0f, left[q] = left0, right[q] = 1.0f;
    for (int r = r_first; r <= r_last; ++r) {
        const int cnt = compact_row(s, A + b * sa_b + r * sa_r, sa_c, C);
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (VEC) {
            if (live[0]) {                                          // (Dl % 4 == 0: four features live or none)
                const float4 p = pooled4(s, cnt, xb, ldx, f[0]);
                v[0] = p.x, v[1] = p.y, v[2] = p.z, v[3] = p.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (live[q]) v[q] = pooled1(s, cnt, xb, ldx, f[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float w = (float)(XT)v[q];                        // bf16 layers: the one rounding of the pooled value
            const float t = w + 1.0f;
            if (r == a) anc[q] = w;
            if (r <= a) left[q] = nan_max(left[q], t);
            else right[q] = nan_max(right[q], t);                   // a < r < n by the loop's bounds
        }
        __syncthreads();   // compact_row's result is read after its last barrier; the next call clears it first
    }
    float *zrow = Z + b * ldz + (int64_t)l * Dl;
    if (VEC) {
        if (!live[0]) return;
        store4(zrow + f[0], make_float4(anc[0], anc[1], anc[2], anc[3]));
        if (sides) {
            store4(zrow + z_section + f[0], make_float4(left[0] - 1.0f, left[1] - 1.0f, left[2] - 1.0f, left[3] - 1.0f));
            store4(zrow + 2 * z_section + f[0], make_float4(right[0] - 1.0f, right[1] - 1.0f, right[2] - 1.0f, right[3] - 1.0f));
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!live[q]) continue;
            zrow[f[q]] = anc[q];
            if (sides) {
                zrow[z_section + f[q]] = left[q] - 1.0f;
                zrow[2 * z_section + f[q]] = right[q] - 1.0f;
            }
        }
    }
}

template <typename XT>
void launch_layers(bool vec, const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const LayerPtrs &ptrs, int n_layers,
                   int64_t x_batch, int64_t ldx, void *Y, int64_t y_batch, int64_t ldy, int B, int R, int C, int Dl, hipStream_t st)
{
    const int units = (Dl + kUnit - 1) / kUnit;
    const dim3 grid((unsigned)(B * R), (unsigned)((n_layers * units + 3) / 4));
    if (vec)
        hipLaunchKernelGGL((subword_pool_layers_kernel<true, XT>), grid, dim3(256), 0, st, A, sa_b, sa_r, sa_c, ptrs, n_layers,
                           x_batch, ldx, static_cast<XT *>(Y), y_batch, ldy, R, C, Dl, units);
    else
        hipLaunchKernelGGL((subword_pool_layers_kernel<false, XT>), grid, dim3(256), 0, st, A, sa_b, sa_r, sa_c, ptrs, n_layers,
                           x_batch, ldx, static_cast<XT *>(Y), y_batch, ldy, R, C, Dl, units);
}

template <typename XT>
void launch_anchor(bool vec, const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const LayerPtrs &ptrs, int n_layers,
                   int64_t x_batch, int64_t ldx, const int64_t *anchor, const int64_t *length, int sides, float *Z, int64_t ldz,
                   int64_t z_section, int B, int R, int C, int Dl, hipStream_t st)
{
    const int units = (Dl + kUnit - 1) / kUnit;
    const dim3 grid((unsigned)B, (unsigned)((n_layers * units + 3) / 4));
    if (vec)
        hipLaunchKernelGGL((anchor_pool_layers_kernel<true, XT>), grid, dim3(256), 0, st, A, sa_b, sa_r, sa_c, ptrs, n_layers,
                           x_batch, ldx, anchor, length, sides, Z, ldz, z_section, R, C, Dl, units);
    else
        hipLaunchKernelGGL((anchor_pool_layers_kernel<false, XT>), grid, dim3(256), 0, st, A, sa_b, sa_r, sa_c, ptrs, n_layers,
                           x_batch, ldx, anchor, length, sides, Z, ldz, z_section, R, C, Dl, units);
}

}  // namespace
}  // namespace ggcn

using namespace ggcn;

extern "C" {

int ggcn_subword_pool(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const float *X, int64_t x_batch,
                      int64_t ldx, float *Y, int64_t y_batch, int64_t ldy, int B, int R, int C, int D, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    if (!A || !X || !Y) return fail(GGCN_EINVAL, "ggcn_subword_pool: null pointer");
    if (B <= 0 || R <= 0 || C <= 0 || D <= 0)
        return fail(GGCN_EINVAL, "ggcn_subword_pool: B=%d R=%d C=%d D=%d must be positive", B, R, C, D);
    if (C > kMaxCols) return fail(GGCN_EUNSUPPORTED, "ggcn_subword_pool: C=%d > %d columns", C, kMaxCols);
    if (ldx < D || ldy < D) return fail(GGCN_EINVAL, "ggcn_subword_pool: leading dimension too small");
    if ((int64_t)B * R > (int64_t)INT32_MAX) return fail(GGCN_EUNSUPPORTED, "ggcn_subword_pool: too many rows");
    const bool vec = (D % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && (x_batch % 4 == 0) && (y_batch % 4 == 0) &&
                     aligned16(X) && aligned16(Y);
    const dim3 grid((unsigned)(B * R), (unsigned)((D + kSlab - 1) / kSlab));
    if (vec)
        hipLaunchKernelGGL(subword_pool_kernel<true>, grid, dim3(256), 0, st, A, sa_b, sa_r, sa_c, X, x_batch, ldx, Y,
                           y_batch, ldy, R, C, D);
    else
        hipLaunchKernelGGL(subword_pool_kernel<false>, grid, dim3(256), 0, st, A, sa_b, sa_r, sa_c, X, x_batch, ldx, Y,
                           y_batch, ldy, R, C, D);
    return check_launch("ggcn_subword_pool");
}

int ggcn_subword_pool_bf16(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *Xv, int64_t x_batch,
                           int64_t ldx, void *Yv, int64_t y_batch, int64_t ldy, int B, int R, int C, int D, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const __bf16 *X = static_cast<const __bf16 *>(Xv);
    __bf16 *Y = static_cast<__bf16 *>(Yv);
    if (!A || !X || !Y) return fail(GGCN_EINVAL, "ggcn_subword_pool_bf16: null pointer");
    if (B <= 0 || R <= 0 || C <= 0 || D <= 0)
        return fail(GGCN_EINVAL, "ggcn_subword_pool_bf16: B=%d R=%d C=%d D=%d must be positive", B, R, C, D);
    if (C > kMaxCols) return fail(GGCN_EUNSUPPORTED, "ggcn_subword_pool_bf16: C=%d > %d columns", C, kMaxCols);
    if (ldx < D || ldy < D) return fail(GGCN_EINVAL, "ggcn_subword_pool_bf16: leading dimension too small");
    if ((int64_t)B * R > (int64_t)INT32_MAX) return fail(GGCN_EUNSUPPORTED, "ggcn_subword_pool_bf16: too many rows");
    // (8-byte loads and stores of four bf16)
    const bool vec = (D % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && (x_batch % 4 == 0) && (y_batch % 4 == 0) &&
                     (reinterpret_cast<uintptr_t>(X) % 8 == 0) && (reinterpret_cast<uintptr_t>(Y) % 8 == 0);
    const dim3 grid((unsigned)(B * R), (unsigned)((D + kSlab - 1) / kSlab));
    if (vec)
        hipLaunchKernelGGL((subword_pool_kernel<true, __bf16>), grid, dim3(256), 0, st, A, sa_b, sa_r, sa_c, X, x_batch, ldx, Y,
                           y_batch, ldy, R, C, D);
    else
        hipLaunchKernelGGL((subword_pool_kernel<false, __bf16>), grid, dim3(256), 0, st, A, sa_b, sa_r, sa_c, X, x_batch, ldx, Y,
                           y_batch, ldy, R, C, D);
    return check_launch("ggcn_subword_pool_bf16");
}

// 1 = vector form, 0 = scalar form, -ggcn_status (message set) where ggcn_subword_pool_layers refuses.  Host only: reads the
// n_layers entries of `layers` and nothing behind any device pointer.  The launcher dispatches on this answer.
int ggcn_subword_pool_layers_form(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *const *layers, int n_layers,
                                  int is_bf16, int64_t x_batch, int64_t ldx, const void *Y, int64_t y_batch, int64_t ldy, int B, int R,
                                  int C, int Dl)
{
    const char *who = "ggcn_subword_pool_layers";
    (void)sa_b; (void)sa_r; (void)sa_c;
    if (!A || !layers || !Y) return -fail(GGCN_EINVAL, "%s: null pointer", who);
    if (n_layers < 1) return -fail(GGCN_EINVAL, "%s: n_layers=%d must be positive", who, n_layers);
    if (n_layers > GGCN_POOL_MAX_LAYERS)
        return -fail(GGCN_EUNSUPPORTED, "%s: n_layers=%d > %d layers a launch (split the layers into groups of %d, each into its own columns of Y)",
                     who, n_layers, GGCN_POOL_MAX_LAYERS, GGCN_POOL_MAX_LAYERS);
    for (int l = 0; l < n_layers; ++l)
        if (!layers[l]) return -fail(GGCN_EINVAL, "%s: layers[%d] is a null pointer", who, l);
    if (B <= 0 || R <= 0 || C <= 0 || Dl <= 0)
        return -fail(GGCN_EINVAL, "%s: B=%d R=%d C=%d Dl=%d must be positive", who, B, R, C, Dl);
    if (C > kMaxCols) return -fail(GGCN_EUNSUPPORTED, "%s: C=%d > %d columns", who, C, kMaxCols);
    if (ldx < Dl || ldy < (int64_t)n_layers * Dl) return -fail(GGCN_EINVAL, "%s: leading dimension too small", who);
    if ((int64_t)B * R > (int64_t)INT32_MAX) return -fail(GGCN_EUNSUPPORTED, "%s: too many rows", who);
    const uintptr_t elem = is_bf16 ? 2 : 4, wide = is_bf16 ? 8 : 16;   // (8-byte loads and stores of four bf16)
    if (reinterpret_cast<uintptr_t>(A) % 4 || reinterpret_cast<uintptr_t>(Y) % elem)
        return -fail(GGCN_EINVAL, "%s: A or Y not aligned to its element", who);
    bool vec = (Dl % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && (x_batch % 4 == 0) && (y_batch % 4 == 0) &&
               (reinterpret_cast<uintptr_t>(Y) % wide == 0);
    for (int l = 0; l < n_layers; ++l) {
        if (reinterpret_cast<uintptr_t>(layers[l]) % elem)
            return -fail(GGCN_EINVAL, "%s: layers[%d] not aligned to its element", who, l);
        vec = vec && (reinterpret_cast<uintptr_t>(layers[l]) % wide == 0);
    }
    const int64_t units = ((int64_t)Dl + kUnit - 1) / kUnit;
    if ((n_layers * units + 3) / 4 > 65535)
        return -fail(GGCN_EUNSUPPORTED, "%s: n_layers=%d Dl=%d needs more than 65535 workgroups a row", who, n_layers, Dl);
    return vec ? 1 : 0;
}

int ggcn_subword_pool_layers(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *const *layers, int n_layers,
                             int is_bf16, int64_t x_batch, int64_t ldx, void *Y, int64_t y_batch, int64_t ldy, int B, int R, int C,
                             int Dl, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const int form = ggcn_subword_pool_layers_form(A, sa_b, sa_r, sa_c, layers, n_layers, is_bf16, x_batch, ldx, Y, y_batch, ldy, B,
                                                   R, C, Dl);
    if (form < 0) return -form;
    LayerPtrs ptrs = {};
    for (int l = 0; l < n_layers; ++l) ptrs.p[l] = layers[l];
    if (is_bf16)
        launch_layers<__bf16>(form == 1, A, sa_b, sa_r, sa_c, ptrs, n_layers, x_batch, ldx, Y, y_batch, ldy, B, R, C, Dl, st);
    else
        launch_layers<float>(form == 1, A, sa_b, sa_r, sa_c, ptrs, n_layers, x_batch, ldx, Y, y_batch, ldy, B, R, C, Dl, st);
    return check_launch("ggcn_subword_pool_layers");
}

// 1 = vector form, 0 = scalar form, -ggcn_status (message set) where ggcn_anchor_pool_layers refuses.  Host only, as
// ggcn_subword_pool_layers_form; its vector / scalar rule with Z, ldz and (with sides) z_section in the place of Y, y_batch and ldy.
int ggcn_anchor_pool_layers_form(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *const *layers, int n_layers,
                                 int is_bf16, int64_t x_batch, int64_t ldx, const int64_t *anchor, const int64_t *length, int sides,
                                 const float *Z, int64_t ldz, int64_t z_section, int B, int R, int C, int Dl)
{
    const char *who = "ggcn_anchor_pool_layers";
    (void)sa_b; (void)sa_r; (void)sa_c;
    if (!A || !layers || !anchor || !Z) return -fail(GGCN_EINVAL, "%s: null pointer", who);
    if (sides && !length) return -fail(GGCN_EINVAL, "%s: length is a null pointer with sides", who);
    if (n_layers < 1) return -fail(GGCN_EINVAL, "%s: n_layers=%d must be positive", who, n_layers);
    if (n_layers > GGCN_POOL_MAX_LAYERS)
        return -fail(GGCN_EUNSUPPORTED, "%s: n_layers=%d > %d layers a launch (split the layers into groups of %d, each into its own columns of Z)",
                     who, n_layers, GGCN_POOL_MAX_LAYERS, GGCN_POOL_MAX_LAYERS);
    for (int l = 0; l < n_layers; ++l)
        if (!layers[l]) return -fail(GGCN_EINVAL, "%s: layers[%d] is a null pointer", who, l);
    if (B <= 0 || R <= 0 || C <= 0 || Dl <= 0)
        return -fail(GGCN_EINVAL, "%s: B=%d R=%d C=%d Dl=%d must be positive", who, B, R, C, Dl);
    if (C > kMaxCols) return -fail(GGCN_EUNSUPPORTED, "%s: C=%d > %d columns", who, C, kMaxCols);
    const int64_t width = (int64_t)n_layers * Dl;
    if (sides && z_section < width)
        return -fail(GGCN_EINVAL, "%s: z_section=%lld < n_layers*Dl=%lld", who, (long long)z_section, (long long)width);
    if (ldx < Dl || ldz < width || (sides && (ldz - width) / 2 < z_section))
        return -fail(GGCN_EINVAL, "%s: leading dimension too small", who);
    // (this grid is (B, units) and would take more; kept so that whatever this entry accepts the composed path,
    // ggcn_subword_pool_layers on the same A, accepts too)
    if ((int64_t)B * R > (int64_t)INT32_MAX) return -fail(GGCN_EUNSUPPORTED, "%s: too many rows", who);
    const uintptr_t elem = is_bf16 ? 2 : 4, wide = is_bf16 ? 8 : 16;   // (8-byte loads of four bf16; Z is float32)
    if (reinterpret_cast<uintptr_t>(A) % 4 || reinterpret_cast<uintptr_t>(Z) % 4 || reinterpret_cast<uintptr_t>(anchor) % 8 ||
        (sides && reinterpret_cast<uintptr_t>(length) % 8))
        return -fail(GGCN_EINVAL, "%s: A, Z, anchor or length not aligned to its element", who);
    bool vec = (Dl % 4 == 0) && (ldx % 4 == 0) && (x_batch % 4 == 0) && (ldz % 4 == 0) && (!sides || z_section % 4 == 0) && aligned16(Z);
    for (int l = 0; l < n_layers; ++l) {
        if (reinterpret_cast<uintptr_t>(layers[l]) % elem)
            return -fail(GGCN_EINVAL, "%s: layers[%d] not aligned to its element", who, l);
        vec = vec && (reinterpret_cast<uintptr_t>(layers[l]) % wide == 0);
    }
    const int64_t units = ((int64_t)Dl + kUnit - 1) / kUnit;
    if ((n_layers * units + 3) / 4 > 65535)
        return -fail(GGCN_EUNSUPPORTED, "%s: n_layers=%d Dl=%d needs more than 65535 workgroups a sentence", who, n_layers, Dl);
    return vec ? 1 : 0;
}

int ggcn_anchor_pool_layers(const float *A, int64_t sa_b, int64_t sa_r, int64_t sa_c, const void *const *layers, int n_layers,
                            int is_bf16, int64_t x_batch, int64_t ldx, const int64_t *anchor, const int64_t *length, int sides,
                            float *Z, int64_t ldz, int64_t z_section, int B, int R, int C, int Dl, ggcn_stream_t stream)
{
    const hipStream_t st = as_stream(stream);
    const int form = ggcn_anchor_pool_layers_form(A, sa_b, sa_r, sa_c, layers, n_layers, is_bf16, x_batch, ldx, anchor, length, sides,
                                                  Z, ldz, z_section, B, R, C, Dl);
    if (form < 0) return -form;
    LayerPtrs ptrs = {};
    for (int l = 0; l < n_layers; ++l) ptrs.p[l] = layers[l];
    const int on = sides != 0;
    if (is_bf16)
        launch_anchor<__bf16>(form == 1, A, sa_b, sa_r, sa_c, ptrs, n_layers, x_batch, ldx, anchor, length, on, Z, ldz, z_section,
                              B, R, C, Dl, st);
    else
        launch_anchor<float>(form == 1, A, sa_b, sa_r, sa_c, ptrs, n_layers, x_batch, ldx, anchor, length, on, Z, ldz, z_section,
                             B, R, C, Dl, st);
    return check_launch("ggcn_anchor_pool_layers");
}

}  // extern "C"
