// The per-Gaussian record of the density field and its builder, shared by field.hip (density / SDF field) and levelset.hip
// (level crossings along rays): A = R(q) diag(1 / max(s, 1e-8)), centre, strength, smallest scale.  field_pack_kernel
// (field.hip, launch_field_pack) writes one 64-byte record per Gaussian; field_load_record reads it back.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace frg {

// T = float in the forward, double in the backward (see the head of the file)
template <typename T>
struct FieldGauss {
    T A[9];                    // A[a * 3 + b] = R[a][b] / max(s_b, 1e-8)
    T mu[3];
    T strength, smin;
};

// pytorch3d.transforms.quaternion_to_matrix, row-major
template <typename T>
__device__ __forceinline__ void field_rotation(const float* q, T* R, T& two_s)
{
    const T r = q[0], i = q[1], j = q[2], k = q[3];
    two_s = T(2) / (((r * r + i * i) + j * j) + k * k);
    R[0] = T(1) - two_s * (j * j + k * k); R[1] = two_s * (i * j - k * r); R[2] = two_s * (i * k + j * r);
    R[3] = two_s * (i * j + k * r); R[4] = T(1) - two_s * (i * i + k * k); R[5] = two_s * (j * k - i * r);
    R[6] = two_s * (i * k - j * r); R[7] = two_s * (j * k + i * r); R[8] = T(1) - two_s * (i * i + j * j);
}

template <typename T>
__device__ __forceinline__ FieldGauss<T> field_make_gauss(const FieldLaunch& p, size_t j)
{
    FieldGauss<T> g;
    float q[4];
    T R[9], two_s;
    const float4 qv = *reinterpret_cast<const float4*>(p.quaternions + 4 * j);      // a [P,4] float32 tensor: rows are 16-byte aligned
    q[0] = qv.x; q[1] = qv.y; q[2] = qv.z; q[3] = qv.w;
    field_rotation<T>(q, R, two_s);
    const float s0 = p.scaling[3 * j], s1 = p.scaling[3 * j + 1], s2 = p.scaling[3 * j + 2];
    const T inv[3] = {T(1) / fmax(T(s0), T(1e-8)), T(1) / fmax(T(s1), T(1e-8)), T(1) / fmax(T(s2), T(1e-8))};
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) g.A[a * 3 + b] = R[a * 3 + b] * inv[b];
#pragma unroll
    for (int c = 0; c < 3; c++) g.mu[c] = p.points[3 * j + c];
    g.strength = p.strengths[j];
    g.smin = fminf(s0, fminf(s1, s2));
    return g;
}

__device__ __forceinline__ FieldGauss<float> field_load_record(const float4* rec, size_t j)
{
    const float4 a = rec[4 * j], b = rec[4 * j + 1], c = rec[4 * j + 2], d = rec[4 * j + 3];
    FieldGauss<float> g;
    g.A[0] = a.x; g.A[1] = a.y; g.A[2] = a.z; g.A[3] = a.w;
    g.A[4] = b.x; g.A[5] = b.y; g.A[6] = b.z; g.A[7] = b.w;
    g.A[8] = c.x; g.mu[0] = c.y; g.mu[1] = c.z; g.mu[2] = c.w;
    g.strength = d.x; g.smin = d.y;
    return g;
}

}  // namespace frg
