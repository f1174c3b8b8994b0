// Adaptive density control of vanilla 3DGS on the device, over the flat per-Gaussian layout of the fused optimizer
// (frosting_amd.parallel.flat_layout: means3D, scales, rotations, opacities, shs, ...; RAW scales (log) and RAW opacities
// (logit), the parameterisation the reference's GaussianModel densifies).
//
// Reference: gaussian_splatting/train.py:114-124 and gaussian_splatting/scene/gaussian_model.py
//   add_densification_stats :405-407   accum += ||viewspace_grad[:, :2]||, denom += 1 on the visible rows (+ train.py:116: max_radii2D)
//   densify_and_prune       :389-403   grads = accum / denom (NaN -> 0); clone :374-387; split :349-372; prune :396-401
//   reset_opacity           :210-213   raw <- logit(min(sigmoid(raw), 0.01)), both moments zeroed (:258-271)
// Four steps here:
//   densify_accumulate  one launch per training step, 4 B per Gaussian + 24 B per visible one
//   densify_plan        classify every row (20 B per Gaussian), scan the four output sections, leave per source row its
//                       destination row in each section and the section sizes in a 32-byte device record
//   densify_apply       one launch: parameters and both Adam moments of every group move to freshly allocated buffers
//   reset_opacity       one launch over the opacity segment
//
// Output row order = the reference's: [surviving originals | clones | first children of the split rows | second
// children], each in source-index order, each minus its pruned rows.  The reference reaches it by two concatenations and
// two boolean-indexed rebuilds of every tensor of the model and of the optimizer state.
//
// The decisions use the reference's float32 arithmetic and comparison directions.  Its final prune reads max_radii2D AFTER
// densification_postfix has zeroed it (:345-347), so the screen-size term (:398) is false on every row: max_screen_size
// only switches the world-size term (:399) on.  Reproduced, not repaired.
//
// Compiled with -ffp-contract=off: every product and sum below is rounded as the reference's elementwise torch ops round it.
#include "kernels.h"

namespace frg {

namespace {

typedef float nt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld_stream4(const float* p)
{
    const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_stream4(float* p, float4 v) { __builtin_nontemporal_store(nt_f4{v.x, v.y, v.z, v.w}, reinterpret_cast<nt_f4*>(p)); }
__device__ __forceinline__ float ld_stream1(const float* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st_stream1(float* p, float v) { __builtin_nontemporal_store(v, p); }

// lanes of this wave below the caller's lane that have the bit set (wave64: v_mbcnt_lo / v_mbcnt_hi)
__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The two computed quantities of a split (:358-364) and the opacity reset keep the reference's form and its float32
// intermediates, with exp and log themselves correctly rounded (evaluated in double, rounded once): the device library's
// expf / logf are good to one ulp, a one-ulp logf alone is 9.5e-7 on a log-scale of magnitude 8 -- twice what the host
// library the reference ran on leaves.  Only split rows and the reset pay for it.
__device__ __forceinline__ float exp_rounded(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float log_rounded(float x) { return (float)log((double)x); }
// raw scale of a split row's children: log(exp(raw) / (0.8 N)), N = 2, from e = exp(raw)
__device__ __forceinline__ float child_raw_scale(float e) { return log_rounded(e / 1.6f); }

// what the classification leaves per row between its two passes (in the plan's first column)
enum : int { ROW_KEEP = 1, ROW_CLONE = 2, ROW_CHILDREN = 4 };

constexpr int PLAN_BLOCK = 256;     // rows per workgroup of the classify / place passes
constexpr int SCAN_BLOCK = 1024;    // threads of the single workgroup that scans the workgroup totals

}  // namespace

// ---- a. statistics ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
densify_accumulate_kernel(int P, const int* __restrict__ radii, const float* __restrict__ dL_dmean2D,
                          const unsigned char* __restrict__ row_live, float* __restrict__ accum, float* __restrict__ denom,
                          float* __restrict__ max_radii2D)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int r = radii[i];
    if (r <= 0) return;
    // an unmarked row was never written: a zero gradient, not read
    float gx = 0.0f, gy = 0.0f;
    if (!row_live || row_live[i]) { gx = dL_dmean2D[3 * (size_t)i]; gy = dL_dmean2D[3 * (size_t)i + 1]; }
    accum[i] = accum[i] + sqrtf(gx * gx + gy * gy);
    denom[i] = denom[i] + 1.0f;
    max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
}

// ---- b. plan ------------------------------------------------------------------------------------------------------------
// Pass 1: the row's class, and per workgroup how many rows it adds to the sections (the two child sections are equal).
__global__ void __launch_bounds__(PLAN_BLOCK)
densify_classify_kernel(int P, const float* __restrict__ raw_scale, const float* __restrict__ raw_opacity,
                        const float* __restrict__ accum, const float* __restrict__ denom, DensifyThresholds t,
                        int* __restrict__ plan, uint32_t* __restrict__ block_tot)
{
    __shared__ uint32_t wave_tot[PLAN_BLOCK / 64][3];
    const int i = blockIdx.x * PLAN_BLOCK + threadIdx.x;
    int cls = 0;
    if (i < P) {
        float grad = accum[i] / denom[i];                               // :390
        if (grad != grad) grad = 0.0f;                                  // :391
        const float e0 = expf(raw_scale[3 * (size_t)i]), e1 = expf(raw_scale[3 * (size_t)i + 1]), e2 = expf(raw_scale[3 * (size_t)i + 2]);
        const float smax = fmaxf(fmaxf(e0, e1), e2);
        const bool selected = grad >= t.max_grad;                       // :354, :376 (the norm of a one-element row; grad >= 0)
        const bool big = smax > t.dense_scale;                          // :356 / :378 (<=)
        const bool faint = raw_sigmoid(raw_opacity[i]) < t.min_opacity; // :396
        const bool split = selected && big, clone = selected && !big;
        // :399 on the row's NEW scale: an original's and a clone's own, a child's the parent's / 1.6 through log and exp
        const bool prune_self = faint || (t.prune_world && smax > t.world_scale);
        bool prune_child = faint;
        if (split && t.prune_world) {
            // (the scale frg_densify_apply will write, activated again)
            const float c0 = expf(child_raw_scale(exp_rounded(raw_scale[3 * (size_t)i]))), c1 = expf(child_raw_scale(exp_rounded(raw_scale[3 * (size_t)i + 1]))),
                        c2 = expf(child_raw_scale(exp_rounded(raw_scale[3 * (size_t)i + 2])));
            prune_child = faint || fmaxf(fmaxf(c0, c1), c2) > t.world_scale;
        }
        if (!split && !prune_self) cls |= ROW_KEEP;
        if (clone && !prune_self) cls |= ROW_CLONE;
        if (split && !prune_child) cls |= ROW_CHILDREN;
        plan[i] = cls;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t nk = __popcll(__ballot(cls & ROW_KEEP)), nc = __popcll(__ballot(cls & ROW_CLONE)), ns = __popcll(__ballot(cls & ROW_CHILDREN));
    if (lane == 0) { wave_tot[wave][0] = nk; wave_tot[wave][1] = nc; wave_tot[wave][2] = ns; }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < PLAN_BLOCK / 64; w++) s += wave_tot[w][threadIdx.x];
        block_tot[3 * (size_t)blockIdx.x + threadIdx.x] = s;
    }
}

// inclusive prefix sum inside a wave (DPP row shifts / permutes under __shfl_up)
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// Pass 2, one workgroup: the workgroup totals become exclusive offsets in place; the section sizes go to the record.
__global__ void __launch_bounds__(SCAN_BLOCK)
densify_scan_kernel(int n_blocks, int P, uint32_t* __restrict__ block_tot, int* __restrict__ record)
{
    __shared__ uint32_t wave_sum[SCAN_BLOCK / 64][3];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int per = (n_blocks + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const int lo = min(tid * per, n_blocks), hi = min(lo + per, n_blocks);
    uint32_t mine[3] = {0, 0, 0};
    for (int b = lo; b < hi; b++)
#pragma unroll
        for (int k = 0; k < 3; k++) mine[k] += block_tot[3 * (size_t)b + k];
    uint32_t incl[3];
#pragma unroll
    for (int k = 0; k < 3; k++) incl[k] = wave_inclusive_sum(mine[k], lane);
    if (lane == 63)
#pragma unroll
        for (int k = 0; k < 3; k++) wave_sum[wave][k] = incl[k];
    __syncthreads();
    uint32_t run[3], total[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < SCAN_BLOCK / 64; w++) {
            const uint32_t s = wave_sum[w][k];
            if (w < wave) before += s;
            all += s;
        }
        run[k] = before + incl[k] - mine[k];
        total[k] = all;
    }
    for (int b = lo; b < hi; b++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t c = block_tot[3 * (size_t)b + k];
            block_tot[3 * (size_t)b + k] = run[k];
            run[k] += c;
        }
    if (tid == 0) {
        record[0] = (int)total[0]; record[1] = (int)total[1]; record[2] = (int)total[2]; record[3] = (int)total[2];
        record[4] = (int)(total[0] + total[1] + 2u * total[2]);
        record[5] = P; record[6] = 0; record[7] = 0;
    }
}

// Pass 3: every row's destination in each section (rows of the output), -1 where it has none.
__global__ void __launch_bounds__(PLAN_BLOCK)
densify_place_kernel(int P, const uint32_t* __restrict__ block_off, const int* __restrict__ record, int* __restrict__ plan)
{
    __shared__ uint32_t wave_tot[PLAN_BLOCK / 64][3];
    const int i = blockIdx.x * PLAN_BLOCK + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int cls = i < P ? plan[i] : 0;
    const unsigned long long mk = __ballot(cls & ROW_KEEP), mc = __ballot(cls & ROW_CLONE), ms = __ballot(cls & ROW_CHILDREN);
    if (lane == 0) { wave_tot[wave][0] = __popcll(mk); wave_tot[wave][1] = __popcll(mc); wave_tot[wave][2] = __popcll(ms); }
    __syncthreads();
    if (i >= P) return;
    uint32_t before[3] = {0, 0, 0};
#pragma unroll
    for (int w = 0; w < PLAN_BLOCK / 64; w++)
        if (w < wave)
#pragma unroll
            for (int k = 0; k < 3; k++) before[k] += wave_tot[w][k];
    const uint32_t nA = (uint32_t)record[0], nB = (uint32_t)record[1], nC = (uint32_t)record[2];
    const uint32_t a = block_off[3 * (size_t)blockIdx.x] + before[0] + lanes_below(mk);
    const uint32_t b = block_off[3 * (size_t)blockIdx.x + 1] + before[1] + lanes_below(mc);
    const uint32_t c = block_off[3 * (size_t)blockIdx.x + 2] + before[2] + lanes_below(ms);
    plan[i] = (cls & ROW_KEEP) ? (int)a : -1;
    plan[(size_t)P + i] = (cls & ROW_CLONE) ? (int)(nA + b) : -1;
    plan[2 * (size_t)P + i] = (cls & ROW_CHILDREN) ? (int)(nA + nB + c) : -1;
    plan[3 * (size_t)P + i] = (cls & ROW_CHILDREN) ? (int)(nA + nB + nC + c) : -1;
}

// ---- c. apply -----------------------------------------------------------------------------------------------------------
// A wave takes 64 consecutive source rows and, group by group, moves them: the source span of a group is contiguous
// (64 rows), read once with the widest access the row length allows, and every destination section is ascending in the
// source index, so the lanes' stores land on consecutive rows wherever consecutive sources go to the same section.
// Survivors carry their moments; clones and children get the parameter row and zero moments (:315-316).
struct Dest { int a, b, c, d; };

// rows of 4 k floats: 16-byte pieces
__device__ __forceinline__ void move_rows_vec(int rows, int w4, const Dest& dst, bool children, const float* __restrict__ src,
                                              const float* __restrict__ src_m, const float* __restrict__ src_v,
                                              float* __restrict__ out, float* __restrict__ out_m, float* __restrict__ out_v, int lane)
{
    const int pieces = rows * w4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    // (the trip count is the wave's, not the lane's: every lane takes part in the shuffles of the last, partial trip)
    for (int e0 = 0; e0 < pieces; e0 += 64) {
        const int e = e0 + lane;
        const bool valid = e < pieces;
        const int r = valid ? e / w4 : 0, q = e - r * w4;
        const int da = __shfl(dst.a, r, 64), db = __shfl(dst.b, r, 64), dc = __shfl(dst.c, r, 64), dd = __shfl(dst.d, r, 64);
        if (!valid || (da < 0 && db < 0 && (!children || (dc < 0 && dd < 0)))) continue;      // a pruned row: nothing of it is read
        const float4 p = ld_stream4(src + 4 * (size_t)e);
        if (da >= 0) {
            const size_t o = ((size_t)da * w4 + q) * 4;
            st_stream4(out + o, p);
            st_stream4(out_m + o, ld_stream4(src_m + 4 * (size_t)e));
            st_stream4(out_v + o, ld_stream4(src_v + 4 * (size_t)e));
        }
        if (db >= 0) {
            const size_t o = ((size_t)db * w4 + q) * 4;
            st_stream4(out + o, p); st_stream4(out_m + o, zero); st_stream4(out_v + o, zero);
        }
        if (children && dc >= 0) {
            const size_t o = ((size_t)dc * w4 + q) * 4;
            st_stream4(out + o, p); st_stream4(out_m + o, zero); st_stream4(out_v + o, zero);
        }
        if (children && dd >= 0) {
            const size_t o = ((size_t)dd * w4 + q) * 4;
            st_stream4(out + o, p); st_stream4(out_m + o, zero); st_stream4(out_v + o, zero);
        }
    }
}

// rows of any length, element by element (means3D, scales: 12 bytes; opacities: 4)
__device__ __forceinline__ void move_rows_scalar(int rows, int w, const Dest& dst, bool children, const float* __restrict__ src,
                                                 const float* __restrict__ src_m, const float* __restrict__ src_v,
                                                 float* __restrict__ out, float* __restrict__ out_m, float* __restrict__ out_v, int lane)
{
    const int elems = rows * w;
    for (int e0 = 0; e0 < elems; e0 += 64) {
        const int e = e0 + lane;
        const bool valid = e < elems;
        const int r = valid ? e / w : 0, q = e - r * w;
        const int da = __shfl(dst.a, r, 64), db = __shfl(dst.b, r, 64), dc = __shfl(dst.c, r, 64), dd = __shfl(dst.d, r, 64);
        if (!valid || (da < 0 && db < 0 && (!children || (dc < 0 && dd < 0)))) continue;
        const float p = ld_stream1(src + e);
        if (da >= 0) {
            const size_t o = (size_t)da * w + q;
            st_stream1(out + o, p); st_stream1(out_m + o, ld_stream1(src_m + e)); st_stream1(out_v + o, ld_stream1(src_v + e));
        }
        if (db >= 0) {
            const size_t o = (size_t)db * w + q;
            st_stream1(out + o, p); st_stream1(out_m + o, 0.0f); st_stream1(out_v + o, 0.0f);
        }
        if (children && dc >= 0) {
            const size_t o = (size_t)dc * w + q;
            st_stream1(out + o, p); st_stream1(out_m + o, 0.0f); st_stream1(out_v + o, 0.0f);
        }
        if (children && dd >= 0) {
            const size_t o = (size_t)dd * w + q;
            st_stream1(out + o, p); st_stream1(out_m + o, 0.0f); st_stream1(out_v + o, 0.0f);
        }
    }
}

__global__ void __launch_bounds__(256)
densify_apply_kernel(int P, int P_out, const int* __restrict__ plan, DensifyGroups g, const float* __restrict__ noise,
                     const float* __restrict__ src, const float* __restrict__ src_m, const float* __restrict__ src_v,
                     float* __restrict__ out, float* __restrict__ out_m, float* __restrict__ out_v)
{
    const int lane = threadIdx.x & 63;
    const int first = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    // the pad elements behind every segment of the new layout stay zero (flat_layout's rule; the optimizer steps them)
    if (blockIdx.x == 0 && threadIdx.x < FRG_DENSIFY_MAX_GROUPS) {
        const int k = threadIdx.x;
        if (k < g.count) {
            const long long end = k + 1 < g.count ? g.dst_offset[k + 1] : g.dst_total;
            for (long long e = g.dst_offset[k] + (long long)P_out * g.width[k]; e < end; e++) { out[e] = 0.0f; out_m[e] = 0.0f; out_v[e] = 0.0f; }
        }
    }
    if (first >= P) return;
    const int rows = min(64, P - first);
    const int i = first + lane;
    Dest dst{-1, -1, -1, -1};
    if (lane < rows) {
        dst.a = plan[i]; dst.b = plan[(size_t)P + i]; dst.c = plan[2 * (size_t)P + i]; dst.d = plan[3 * (size_t)P + i];
        // a plan that does not belong to these buffers must not write outside them
        if (dst.a >= P_out) dst.a = -1;
        if (dst.b >= P_out) dst.b = -1;
        if (dst.c >= P_out) dst.c = -1;
        if (dst.d >= P_out) dst.d = -1;
    }
    // the split rows' children (:358-364): lane = row; means3D and scales are computed, everything else is a copy below
    if (dst.c >= 0 || dst.d >= 0) {
        const float* xyz = src + g.src_offset[0] + 3 * (size_t)i;
        const float* rs = src + g.src_offset[1] + 3 * (size_t)i;
        const float* rq = src + g.src_offset[2] + 4 * (size_t)i;
        const float s0 = exp_rounded(rs[0]), s1 = exp_rounded(rs[1]), s2 = exp_rounded(rs[2]);
        // build_rotation (general_utils.py:78-99) on the stored quaternion
        const float q0 = rq[0], q1 = rq[1], q2 = rq[2], q3 = rq[3];
        const float norm = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
        const float r = q0 / norm, x = q1 / norm, y = q2 / norm, z = q3 / norm;
        const float R00 = 1.0f - 2.0f * (y * y + z * z), R01 = 2.0f * (x * y - r * z), R02 = 2.0f * (x * z + r * y);
        const float R10 = 2.0f * (x * y + r * z), R11 = 1.0f - 2.0f * (x * x + z * z), R12 = 2.0f * (y * z - r * x);
        const float R20 = 2.0f * (x * z - r * y), R21 = 2.0f * (y * z + r * x), R22 = 1.0f - 2.0f * (x * x + y * y);
        const float n0 = child_raw_scale(s0), n1 = child_raw_scale(s1), n2 = child_raw_scale(s2);
        const float px = xyz[0], py = xyz[1], pz = xyz[2];
#pragma unroll
        for (int child = 0; child < 2; child++) {
            const int d = child ? dst.d : dst.c;
            if (d < 0) continue;
            // (no samples given: the children sit on the parent's centre)
            const float* zn = noise + (2 * (size_t)i + child) * 3;
            const float z0 = noise ? zn[0] : 0.0f, z1 = noise ? zn[1] : 0.0f, z2 = noise ? zn[2] : 0.0f;
            const float a0 = s0 * z0, a1 = s1 * z1, a2 = s2 * z2;                          // normal(0, std) = std * z
            float* o = out + g.dst_offset[0] + 3 * (size_t)d;
            o[0] = (R00 * a0 + R01 * a1 + R02 * a2) + px;
            o[1] = (R10 * a0 + R11 * a1 + R12 * a2) + py;
            o[2] = (R20 * a0 + R21 * a1 + R22 * a2) + pz;
            float* os = out + g.dst_offset[1] + 3 * (size_t)d;
            os[0] = n0; os[1] = n1; os[2] = n2;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                out_m[g.dst_offset[0] + 3 * (size_t)d + c] = 0.0f; out_v[g.dst_offset[0] + 3 * (size_t)d + c] = 0.0f;
                out_m[g.dst_offset[1] + 3 * (size_t)d + c] = 0.0f; out_v[g.dst_offset[1] + 3 * (size_t)d + c] = 0.0f;
            }
        }
    }
#pragma unroll 1
    for (int k = 0; k < g.count; k++) {
        const int w = g.width[k];
        const bool children = k >= 2;        // groups 0 and 1 (means3D, scales) of a child were written above
        const size_t so = (size_t)g.src_offset[k] + (size_t)first * w, dof = (size_t)g.dst_offset[k];
        if ((w & 3) == 0)
            move_rows_vec(rows, w >> 2, dst, children, src + so, src_m + so, src_v + so, out + dof, out_m + dof, out_v + dof, lane);
        else
            move_rows_scalar(rows, w, dst, children, src + so, src_m + so, src_v + so, out + dof, out_m + dof, out_v + dof, lane);
    }
}

// ---- d. opacity reset -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
reset_opacity_kernel(int P, float* __restrict__ raw_opacity, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float x = fminf(1.0f / (1.0f + exp_rounded(-raw_opacity[i])), 0.01f);      // :211
    raw_opacity[i] = log_rounded(x / (1.0f - x));                                    // inverse_sigmoid, general_utils.py:18-19
    exp_avg[i] = 0.0f;
    exp_avg_sq[i] = 0.0f;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
hipError_t launch_densify_accumulate(int P, const int* radii, const float* dL_dmean2D, const unsigned char* row_live,
                                     float* accum, float* denom, float* max_radii2D, hipStream_t s)
{
    hipLaunchKernelGGL(densify_accumulate_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, radii, dL_dmean2D, row_live, accum,
                       denom, max_radii2D);
    return hipGetLastError();
}

size_t densify_workspace_bytes(int P) { return (size_t)((P + PLAN_BLOCK - 1) / PLAN_BLOCK) * 3 * sizeof(uint32_t); }

hipError_t launch_densify_plan(int P, const float* raw_scale, const float* raw_opacity, const float* accum, const float* denom,
                               const DensifyThresholds& t, int* plan, int* record, char* workspace, hipStream_t s)
{
    const int n_blocks = (P + PLAN_BLOCK - 1) / PLAN_BLOCK;
    uint32_t* block_tot = reinterpret_cast<uint32_t*>(workspace);
    hipLaunchKernelGGL(densify_classify_kernel, dim3(n_blocks), dim3(PLAN_BLOCK), 0, s, P, raw_scale, raw_opacity, accum, denom, t,
                       plan, block_tot);
    hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(SCAN_BLOCK), 0, s, n_blocks, P, block_tot, record);
    hipLaunchKernelGGL(densify_place_kernel, dim3(n_blocks), dim3(PLAN_BLOCK), 0, s, P, block_tot, record, plan);
    return hipGetLastError();
}

hipError_t launch_densify_apply(int P, int P_out, const int* plan, const DensifyGroups& g, const float* noise, const float* src,
                                const float* src_m, const float* src_v, float* out, float* out_m, float* out_v, hipStream_t s)
{
    const int waves = (P + 63) / 64;
    hipLaunchKernelGGL(densify_apply_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, P, P_out, plan, g, noise, src, src_m, src_v,
                       out, out_m, out_v);
    return hipGetLastError();
}

hipError_t launch_reset_opacity(int P, float* raw_opacity, float* exp_avg, float* exp_avg_sq, hipStream_t s)
{
    hipLaunchKernelGGL(reset_opacity_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, raw_opacity, exp_avg, exp_avg_sq);
    return hipGetLastError();
}

}  // namespace frg
