// Level-set crossings of the density field of K neighbour Gaussians along rays, forward only
// (frosting_scene/frosting_model.py: compute_level_points_along_normals :2016-2208,
// compute_level_surface_points_and_range_from_camera :1747-2013; both run under torch.no_grad()).
//
// Per ray r (origin o, direction d as given, t_scale, t_offset, K neighbour indices) and per call n sample parameters lin[j]:
//     t_j = lin[j] * t_scale + t_offset,   x_j = o + t_j * d          (every product and sum rounded on its own)
//     dens_j = sum_k density_factor * strength_k * exp(-0.5 * clamp(|A_k^T (x_j - mu_k)|^2, 0, 1e8)),  >= 1 -> d / (d + 1e-12)
// and per level the reference's search: first_above = the first j with dens_j > level (0 if none, and 0 if it is sample 0:
// index 0 doubles as "none"), last_above = the last such j (n - 1 if none) or, in the SECOND_CROSSING mode, the first j with
// dens_j > level and dens_{j+1} < level (a hit at 0 and no hit both give n - 1); a density equal to the level is neither above
// nor under.  The crossings are the reference's linear interpolations between the two samples, or the range's end when unbound.
// The normal is -normalize(sum_k o_k A_k (A_k^T shift)) at o + t_outer d, zeros where first_above == 0.
//
// Mapping: one lane per ray.  The K records (field.hip's 64-byte format, packed by its field_pack_kernel) are the outer loop,
// so each is gathered once per ray; the n running densities and the n sample parameters stay in registers (every index into
// them is a compile-time constant: the search captures the two samples around a crossing while it scans, it never indexes by
// the found position).  NS = 21 is the fast path of both callers (no per-sample guards); any other n <= 32 runs the capped
// form with the loops guarded by j < n.  The normal is a second walk over the ray's K records per level.
#include <cmath>

#include "frosting_rasterizer.h"
#include "kernels.h"
#include "field_record.h"

namespace frg {

namespace {

// One float32 operation, rounded on its own.  HIP's __fmul_rn / __fadd_rn are plain `*` / `+` and fuse into an fma under
// this file's default contraction; an operation written under `fp contract(off)` does not.
__device__ __forceinline__ float mul_r(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_r(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_r(float a, float b)
{
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float div_r(float a, float b)
{
#pragma clang fp contract(off)
    return a / b;
}

// (level - va) / (vb - va) * (tb - ta) + ta, every operation rounded on its own as a float32 tensor expression is
__device__ __forceinline__ float levelset_cross(float level, float va, float vb, float ta, float tb)
{
    return add_r(mul_r(div_r(sub_r(level, va), sub_r(vb, va)), sub_r(tb, ta)), ta);
}

// w = A^T (x - mu), m = clamp(w.w, 0, 1e8): field.hip's expressions
__device__ __forceinline__ float levelset_warp(const FieldGauss<float>& g, float x0, float x1, float x2, float* w)
{
    const float d0 = x0 - g.mu[0], d1 = x1 - g.mu[1], d2 = x2 - g.mu[2];
#pragma unroll
    for (int b = 0; b < 3; b++) w[b] = (g.A[b] * d0 + g.A[3 + b] * d1) + g.A[6 + b] * d2;
    const float m = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    return fminf(fmaxf(m, 0.0f), 1e8f);
}

__device__ __forceinline__ long long levelset_index(const LevelsetLaunch& p, size_t at)
{
    return p.idx64 ? static_cast<const long long*>(p.idx)[at] : (long long)static_cast<const int*>(p.idx)[at];
}

}  // namespace

template <int NS, bool FIXED>
__global__ void __launch_bounds__(256)
levelset_kernel(LevelsetLaunch p)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (size_t)p.R) return;
    const int n = FIXED ? NS : p.n;
    const size_t R = (size_t)p.R;
    const float o0 = p.origins[3 * r], o1 = p.origins[3 * r + 1], o2 = p.origins[3 * r + 2];
    const float d0 = p.directions[3 * r], d1 = p.directions[3 * r + 1], d2 = p.directions[3 * r + 2];
    const float ts = p.t_scale[r], to = p.t_offset[r];

    float t[NS], dens[NS];
#pragma unroll
    for (int j = 0; j < NS; j++) {
        t[j] = (FIXED || j < n) ? add_r(mul_r(p.lin[j], ts), to) : 0.0f;
        dens[j] = 0.0f;
    }

    bool bad = false;
    for (int k = 0; k < p.K; k++) {
        const long long gi = levelset_index(p, r * (size_t)p.K + (size_t)k);
        if (gi < 0 || gi >= (long long)p.P) { bad = true; continue; }        // never dereferenced, contributes nothing
        const FieldGauss<float> g = field_load_record(p.rec, (size_t)gi);
        const float sf = p.density_factor * g.strength;
#pragma unroll
        for (int j = 0; j < NS; j++) {
            if (FIXED || j < n) {
                float w[3];
                const float m = levelset_warp(g, add_r(o0, mul_r(t[j], d0)), add_r(o1, mul_r(t[j], d1)),
                                              add_r(o2, mul_r(t[j], d2)), w);
                dens[j] += sf * expf(-0.5f * m);
            }
        }
    }
    if (bad) *p.bad_index = 1;                             // every writer stores the same word

    float t_end = t[NS - 1];                               // t of sample n - 1
#pragma unroll
    for (int j = 0; j < NS; j++) {
        if (dens[j] >= 1.0f) dens[j] = dens[j] / (dens[j] + 1e-12f);
        if (!FIXED && j == n - 1) t_end = t[j];
        if (p.densities && (FIXED || j < n)) p.densities[r * (size_t)n + j] = dens[j];
    }

    for (int l = 0; l < p.L; l++) {
        const float level = p.levels[l];
        int first = 0, last = p.inner_mode == FRG_LEVELSET_INNER_LAST ? n - 1 : 0;
        bool found = false, found2 = false;
        float fa = 0.f, fb = 0.f, fta = 0.f, ftb = 0.f;    // the samples before and at first_above
        float la = 0.f, lb = 0.f, lta = 0.f, ltb = 0.f;    // the samples at and behind last_above
#pragma unroll
        for (int j = 0; j < NS; j++) {
            if (FIXED || j < n) {
                const bool above = dens[j] > level;
                if (above && !found) {
                    found = true;
                    first = j;
                    if (j > 0) { fa = dens[j - 1]; fb = dens[j]; fta = t[j - 1]; ftb = t[j]; }
                }
                if (j + 1 < NS && (FIXED || j + 1 < n)) {
                    if (p.inner_mode == FRG_LEVELSET_INNER_LAST) {
                        if (above) { last = j; la = dens[j]; lb = dens[j + 1]; lta = t[j]; ltb = t[j + 1]; }
                    } else if (above && dens[j + 1] < level && !found2) {
                        found2 = true;
                        last = j; la = dens[j]; lb = dens[j + 1]; lta = t[j]; ltb = t[j + 1];
                    }
                } else if (p.inner_mode == FRG_LEVELSET_INNER_LAST && above) {
                    last = j;                              // sample n - 1: unbound
                }
            }
        }
        if (p.inner_mode != FRG_LEVELSET_INNER_LAST && last == 0) last = n - 1;      // "no second crossing", and a crossing at 0
        const float t_outer = first > 0 ? levelset_cross(level, fa, fb, fta, ftb) : t[0];
        const float t_inner = last < n - 1 ? levelset_cross(level, la, lb, lta, ltb) : t_end;
        const size_t at = (size_t)l * R + r;
        if (p.t_outer) p.t_outer[at] = t_outer;
        if (p.t_inner) p.t_inner[at] = t_inner;
        if (p.first_above) p.first_above[at] = first;
        if (p.last_above) p.last_above[at] = last;
        if (p.under_first) p.under_first[at] = dens[0] < level ? 1 : 0;
        if (p.normals) {
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
            if (first > 0) {
                const float x0 = add_r(o0, mul_r(t_outer, d0)), x1 = add_r(o1, mul_r(t_outer, d1)),
                            x2 = add_r(o2, mul_r(t_outer, d2));
                for (int k = 0; k < p.K; k++) {
                    const long long gi = levelset_index(p, r * (size_t)p.K + (size_t)k);
                    if (gi < 0 || gi >= (long long)p.P) continue;
                    const FieldGauss<float> g = field_load_record(p.rec, (size_t)gi);
                    float w[3];
                    const float m = levelset_warp(g, x0, x1, x2, w);
                    const float ok = (p.density_factor * g.strength) * expf(-0.5f * m);
                    g0 += ok * ((g.A[0] * w[0] + g.A[1] * w[1]) + g.A[2] * w[2]);
                    g1 += ok * ((g.A[3] * w[0] + g.A[4] * w[1]) + g.A[5] * w[2]);
                    g2 += ok * ((g.A[6] * w[0] + g.A[7] * w[1]) + g.A[8] * w[2]);
                }
                const float len = fmaxf(sqrtf((g0 * g0 + g1 * g1) + g2 * g2), 1e-12f);      // F.normalize's eps
                g0 = -(g0 / len); g1 = -(g1 / len); g2 = -(g2 / len);
            }
            p.normals[3 * at] = g0; p.normals[3 * at + 1] = g1; p.normals[3 * at + 2] = g2;
        }
    }
}

size_t levelset_workspace_bytes(int P) { return align_up((size_t)(P > 0 ? P : 1) * 64, 256); }

hipError_t launch_levelset(LevelsetLaunch p, const float* points, const float* scaling, const float* quaternions,
                           const float* strengths, char* workspace, hipStream_t s)
{
    float4* rec = reinterpret_cast<float4*>(workspace);
    hipError_t e = launch_field_pack(p.P, points, scaling, quaternions, strengths, rec, s);
    if (e != hipSuccess) return e;
    p.rec = rec;
    const dim3 grid((unsigned)(((size_t)p.R + 255) / 256)), block(256);
    if (p.n == 21) hipLaunchKernelGGL((levelset_kernel<21, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((levelset_kernel<32, false>), grid, block, 0, s, p);
    return hipGetLastError();
}

}  // namespace frg
