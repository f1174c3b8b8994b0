// Density / SDF field of SuGaR over the K neighbour Gaussians of every sample, forward and backward
// (frosting_scene/sugar_model.py: get_field_values, get_beta, compute_density).
//
// Per pair (sample s, its k-th neighbour j = idx[s][k]), with A_j = R(q_j) diag(1 / max(s_j, 1e-8)) and R pytorch3d's
// quaternion_to_matrix (real part first, two_s = 2 / |q|^2, the quaternion as given):
//     w = A_j^T (x_s - mu_j),   o = density_factor * strength_j * exp(-0.5 * clamp(w.w, 0, 1e8))
// and per sample density = sum_k o, beta ('average': mean_k min(s_j); 'weighted_average': sum_k min(s_j) o / max(sum o,
// opacity_min_clamp), a caller's constant where sum o == 0) and sdf = beta (sqrt(-2 log max(d_n, clamp)) - c0), d_n being
// the density after the reference's normalisation (rows >= 1 become d / (d.detach() + 1e-12)).
//
// Forward: pairs map to lanes.  A sample owns G = the power of two >= K consecutive lanes (64 / G samples per wave), so the
// idx rows are read coalesced, one gather per lane is in flight, and the K-wide sums are xor butterflies inside the group
// (every lane of a group ends with the same bits).  A pre-pass packs {A (9), mu (3), strength, min scale} into one 64-byte
// record per Gaussian: a pair's gather is one line instead of four arrays (FRG_FIELD_RECOMPUTE reads the four arrays and
// rebuilds A per pair instead; tools/field_bench.py times both).
//
// Backward, without atomics and in a fixed order, in DOUBLE from the float32 inputs to the one rounding of every stored value.
// exp(-m / 2) turns an absolute error of m into a relative one of o, so a float32 recomputation of a pair at m ~ 10 is off by
// several ulp before any gradient is formed; the kernels are bound by their gathers, CDNA runs double at half the float32 rate,
// and the records (float32) are not used here: the four arrays are read and R, 1 / max(s, 1e-8) rebuilt per pair.
//   1. the pair kernel again (BWD): recomputes the forward, forms per sample the two scalars (a, b) every pair's
//      dL/do = a + b * min(s_j) + dL/dopacities[s][k] and dL/dmin(s_j) = b * o (or b) follow from, reduces dL/dx over the
//      group and stores it, and writes the pair's sort key j (P for an index outside [0, P): such a pair contributes
//      nothing anywhere and raises *bad_index);
//   2. one stable rocPRIM radix sort of (j, pair id) with the pair ids from a counting iterator: the inverse neighbour
//      lists, each in ascending pair id; a boundary kernel records every list's [begin, end);
//   3. 16 lanes per Gaussian walk its list (element e by lane e % 16), recompute w and o from x_s and accumulate, in the
//      Gaussian's frame p = R^T (x - mu), the eleven sums  sum h p p^T (6), sum h p (3), sum dL/do * do/dstrength,
//      sum dL/dmin(s)  with h = -dL/do * o: the gradients of mu, s, q and strength are linear in them.
//      A fixed butterfly combines the 16 partial sums and lane 0 stores the Gaussian's rows once (zeros for an empty list);
//   4. lists longer than FIELD_HUB go to a second kernel, one workgroup of 256 per list (element e by thread e % 256,
//      butterfly per wave, the four waves added in order through LDS), found without a list of lists: the workgroup of
//      sorted chunk c owns the list that contains position c * FIELD_HUB if that is the first multiple at or behind the
//      list's begin.
// Which kernel takes a Gaussian, and which lane an element, depends only on the list's length and the element's place in
// it: the result does not change with what other Gaussians' lists hold.
#include <cmath>
#include <cstring>
#include <type_traits>

#include <rocprim/rocprim.hpp>

#include "frosting_rasterizer.h"
#include "kernels.h"
#include "field_record.h"

namespace frg {

#define FIELD_HUB 1024u        // a longer list gets a workgroup of its own; also the chunk the hub kernel's workgroups look at
#define FIELD_LANES 16         // lanes per Gaussian in the list walk

namespace {

template <int G, typename T>
__device__ __forceinline__ T group_sum(T v)
{
#pragma unroll
    for (int d = G / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

}  // namespace

__global__ void __launch_bounds__(256)
field_pack_kernel(FieldLaunch p)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= (size_t)p.P) return;
    const FieldGauss<float> g = field_make_gauss<float>(p, j);
    p.rec[4 * j] = make_float4(g.A[0], g.A[1], g.A[2], g.A[3]);
    p.rec[4 * j + 1] = make_float4(g.A[4], g.A[5], g.A[6], g.A[7]);
    p.rec[4 * j + 2] = make_float4(g.A[8], g.mu[0], g.mu[1], g.mu[2]);
    p.rec[4 * j + 3] = make_float4(g.strength, g.smin, 0.0f, 0.0f);
}

// lane = pair: sample gid / G, neighbour gid % G (lanes with neighbour >= K and samples >= N idle but take part in the shuffles)
template <int G, bool BWD>
__global__ void __launch_bounds__(256)
field_pair_kernel(FieldLaunch p)
{
    using T = typename std::conditional<BWD, double, float>::type;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t s = gid / G;
    const int k = (int)(gid % G);
    const bool row = s < (size_t)p.N;
    const bool live = row && k < p.K;
    const size_t pair = s * (size_t)p.K + (size_t)k;
    const T density_factor = (T)p.density_factor, min_clamp = (T)p.opacity_min_clamp, sdf_offset = (T)p.sdf_offset;

    long long j = -1;
    if (live) j = p.idx64 ? static_cast<const long long*>(p.idx)[pair] : (long long)static_cast<const int*>(p.idx)[pair];
    const bool ok = live && j >= 0 && j < (long long)p.P;
    if (live && !ok) *p.bad_index = 1;                     // every writer stores the same word

    FieldGauss<T> g;
    T w[3] = {0, 0, 0}, m = 0, E = 0, o = 0, smin = 0;
    if (ok) {
        if constexpr (BWD) g = field_make_gauss<T>(p, (size_t)j);
        else g = p.recompute ? field_make_gauss<T>(p, (size_t)j) : field_load_record(p.rec, (size_t)j);
        const T d0 = T(p.x[3 * s]) - g.mu[0], d1 = T(p.x[3 * s + 1]) - g.mu[1], d2 = T(p.x[3 * s + 2]) - g.mu[2];
#pragma unroll
        for (int b = 0; b < 3; b++) w[b] = (g.A[b] * d0 + g.A[3 + b] * d1) + g.A[6 + b] * d2;
        m = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
        E = exp(T(-0.5) * fmin(fmax(m, T(0)), T(1e8)));
        o = (density_factor * g.strength) * E;
        smin = g.smin;
    }

    // the sample's sums: every lane of the group ends with the same bits
    const T D = group_sum<G>(o);
    const T Sc = fmax(D, min_clamp);
    T beta_raw = 0, beta = 0;
    if (p.beta_mode == FRG_FIELD_BETA_AVERAGE) {
        beta_raw = beta = group_sum<G>(smin) / (T)p.K;
    } else if (p.beta_mode == FRG_FIELD_BETA_WEIGHTED) {
        beta_raw = group_sum<G>(smin * (o / Sc));
        beta = D == T(0) ? (T)*p.beta_fallback : beta_raw;
    }
    const bool unit = D >= T(1);                           // the reference's normalisation: d / (d.detach() + 1e-12)
    const T dn = unit ? D / (D + T(1e-12)) : D;
    const T c = fmax(dn, min_clamp);
    const T t = sqrt(T(-2) * log(c));

    if constexpr (!BWD) {
        if (live && p.opacities) p.opacities[pair] = o;
        if (row && k == 0) {
            if (p.density) p.density[s] = D;
            if (p.beta) p.beta[s] = beta;
            if (p.sdf) p.sdf[s] = beta * (t - sdf_offset);
        }
    } else {
        // dL/do of a pair = a + b * min(s_j) + dL/dopacities ('weighted_average'; b = 0 without a beta) or a + dL/dopacities
        // ('average'); dL/dmin(s_j) = b * o or b
        const T g_den = (row && p.g_density) ? p.g_density[s] : 0.f;
        const T g_beta = (row && p.g_beta) ? p.g_beta[s] : 0.f;
        const T g_sdf = (row && p.g_sdf) ? p.g_sdf[s] : 0.f;
        T a = g_den, b = 0;
        if (p.beta_mode != FRG_FIELD_BETA_NONE) {
            T Gb = g_beta;
            if (p.g_sdf) {
                Gb += g_sdf * (t - sdf_offset);
                // through sqrt, log, the clamp and the normalisation.  On a row >= 1 the reference's float32 sqrt is taken at
                // exactly 0 and its derivative is not finite: the density term of the sdf is given no gradient there
                T Gc = (!unit && t > T(0)) ? g_sdf * (-beta / (t * c)) : T(0);
                if (!(dn >= min_clamp)) Gc = 0;
                a += Gc;
            }
            if (p.beta_mode == FRG_FIELD_BETA_AVERAGE) {
                b = Gb / (T)p.K;
            } else {
                b = Gb / Sc;
                if (D >= min_clamp) a -= b * beta_raw;
            }
        }
        T Go = a + ((live && p.g_opacities) ? (T)p.g_opacities[pair] : T(0));
        if (p.beta_mode == FRG_FIELD_BETA_WEIGHTED) Go += b * smin;
        // dL/dx = sum_k A (h w), h = 2 dL/dm = -dL/do * o inside the clamp
        T gx[3] = {0, 0, 0};
        if (ok) {
            const T h = (m >= T(0) && m <= T(1e8)) ? -Go * o : T(0);
#pragma unroll
            for (int r = 0; r < 3; r++) gx[r] = h * ((g.A[3 * r] * w[0] + g.A[3 * r + 1] * w[1]) + g.A[3 * r + 2] * w[2]);
        }
#pragma unroll
        for (int r = 0; r < 3; r++) gx[r] = group_sum<G>(gx[r]);
        if (live) p.keys[pair] = ok ? (uint32_t)j : (uint32_t)p.P;
        if (row && k == 0) {
            p.dL_dx[3 * s] = (float)gx[0]; p.dL_dx[3 * s + 1] = (float)gx[1]; p.dL_dx[3 * s + 2] = (float)gx[2];
            p.ab[s] = make_double2(a, b);
        }
    }
}

// [begin, end) of every key's run in the sorted keys; seg_begin / seg_end were zeroed (a Gaussian no pair names: 0, 0)
__global__ void __launch_bounds__(256)
field_segment_kernel(uint32_t n, uint32_t P, const uint32_t* __restrict__ keys_s, uint32_t* __restrict__ seg_begin,
                     uint32_t* __restrict__ seg_end)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = keys_s[i];
    if (key >= P) return;                                  // the pairs with an index outside [0, P)
    if (i == 0 || keys_s[i - 1] != key) seg_begin[key] = (uint32_t)i;
    if (i + 1 == n || keys_s[i + 1] != key) seg_end[key] = (uint32_t)i + 1u;
}

namespace {

// a Gaussian as the list walk needs it
struct FieldOwn {
    double R[9], inv[3], two_s;
    float s[3], q[4], mu[3];
    float strength, smin;
};

__device__ __forceinline__ FieldOwn field_own(const FieldLaunch& p, size_t j)
{
    FieldOwn g;
    const float4 qv = *reinterpret_cast<const float4*>(p.quaternions + 4 * j);
    g.q[0] = qv.x; g.q[1] = qv.y; g.q[2] = qv.z; g.q[3] = qv.w;
    field_rotation<double>(g.q, g.R, g.two_s);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        g.s[c] = p.scaling[3 * j + c];
        g.inv[c] = 1.0 / fmax((double)g.s[c], 1e-8);
        g.mu[c] = p.points[3 * j + c];
    }
    g.strength = p.strengths[j];
    g.smin = fminf(g.s[0], fminf(g.s[1], g.s[2]));
    return g;
}

// v: Q00 Q01 Q02 Q11 Q12 Q22 | P0 P1 P2 | dL/dstrength | dL/dmin(s)
__device__ __forceinline__ void field_accumulate(const FieldLaunch& p, const FieldOwn& g, uint32_t pair, double* v)
{
    const uint32_t s = pair / (uint32_t)p.K;
    const double d0 = (double)p.x[3 * (size_t)s] - (double)g.mu[0], d1 = (double)p.x[3 * (size_t)s + 1] - (double)g.mu[1],
                 d2 = (double)p.x[3 * (size_t)s + 2] - (double)g.mu[2];
    const double2 ab = p.ab[s];
    double pf[3], w[3];
#pragma unroll
    for (int b = 0; b < 3; b++) {
        pf[b] = (g.R[b] * d0 + g.R[3 + b] * d1) + g.R[6 + b] * d2;
        w[b] = g.inv[b] * pf[b];
    }
    const double m = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double E = exp(-0.5 * fmin(fmax(m, 0.0), 1e8));
    const double o = (p.density_factor * (double)g.strength) * E;
    double Go = ab.x + (p.g_opacities ? (double)p.g_opacities[pair] : 0.0);
    double Gs = ab.y;
    if (p.beta_mode == FRG_FIELD_BETA_WEIGHTED) { Go += ab.y * (double)g.smin; Gs = ab.y * o; }
    const double h = (m >= 0.0 && m <= 1e8) ? -Go * o : 0.0;
    v[0] += h * pf[0] * pf[0]; v[1] += h * pf[0] * pf[1]; v[2] += h * pf[0] * pf[2];
    v[3] += h * pf[1] * pf[1]; v[4] += h * pf[1] * pf[2]; v[5] += h * pf[2] * pf[2];
    v[6] += h * pf[0]; v[7] += h * pf[1]; v[8] += h * pf[2];
    v[9] += Go * (p.density_factor * E);
    v[10] += Gs;
}

// the Gaussian's eleven gradient values from its eleven sums, rounded to float32 and stored once
__device__ __forceinline__ void field_store_rows(const FieldLaunch& p, const FieldOwn& g, size_t j, const double* v, bool empty)
{
    double out[11];
    if (empty) {
#pragma unroll
        for (int c = 0; c < 11; c++) out[c] = 0.0;
    } else {
        const double i2[3] = {g.inv[0] * g.inv[0], g.inv[1] * g.inv[1], g.inv[2] * g.inv[2]};
        const double Q[9] = {v[0], v[1], v[2], v[1], v[3], v[4], v[2], v[4], v[5]};
        // dL/dmu = -R (inv^2 * P)
#pragma unroll
        for (int a = 0; a < 3; a++)
            out[a] = -((g.R[3 * a] * (i2[0] * v[6]) + g.R[3 * a + 1] * (i2[1] * v[7])) + g.R[3 * a + 2] * (i2[2] * v[8]));
        // dL/ds_b = -inv_b^3 Q_bb inside the 1e-8 clamp; the min-scale sum goes to the first smallest component
        const int amin = (g.s[0] <= g.s[1] && g.s[0] <= g.s[2]) ? 0 : (g.s[1] <= g.s[2] ? 1 : 2);
#pragma unroll
        for (int b = 0; b < 3; b++)
            out[3 + b] = (g.s[b] >= 1e-8f ? -(g.inv[b] * Q[4 * b]) * i2[b] : 0.0) + (b == amin ? v[10] : 0.0);
        // dL/dR[a][b] = inv_b^2 sum_c R[a][c] Q[c][b], then through quaternion_to_matrix (B = (R - I) / two_s)
        double GR[9];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++)
                GR[3 * a + b] = i2[b] * ((g.R[3 * a] * Q[b] + g.R[3 * a + 1] * Q[3 + b]) + g.R[3 * a + 2] * Q[6 + b]);
        const double r = g.q[0], i = g.q[1], jj = g.q[2], k = g.q[3];
        const double B[9] = {-(jj * jj + k * k), i * jj - k * r, i * k + jj * r,
                             i * jj + k * r, -(i * i + k * k), jj * k - i * r,
                             i * k - jj * r, jj * k + i * r, -(i * i + jj * jj)};
        double GB = 0.0;
#pragma unroll
        for (int c = 0; c < 9; c++) GB += GR[c] * B[c];
        const double q[4] = {r, i, jj, k};
        const double gq[4] = {
            k * (GR[3] - GR[1]) + jj * (GR[2] - GR[6]) + i * (GR[7] - GR[5]),
            jj * (GR[1] + GR[3]) + k * (GR[2] + GR[6]) + r * (GR[7] - GR[5]) - 2.0 * i * (GR[4] + GR[8]),
            i * (GR[1] + GR[3]) + r * (GR[2] - GR[6]) + k * (GR[5] + GR[7]) - 2.0 * jj * (GR[0] + GR[8]),
            r * (GR[3] - GR[1]) + i * (GR[2] + GR[6]) + jj * (GR[5] + GR[7]) - 2.0 * k * (GR[0] + GR[4])};
        const double GBn = GB * g.two_s;                   // 2 GB / |q|^2
#pragma unroll
        for (int c = 0; c < 4; c++) out[6 + c] = g.two_s * (gq[c] - q[c] * GBn);
        out[10] = v[9];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) { p.dL_dpoints[3 * j + c] = (float)out[c]; p.dL_dscaling[3 * j + c] = (float)out[3 + c]; }
    *reinterpret_cast<float4*>(p.dL_dquaternions + 4 * j) = make_float4((float)out[6], (float)out[7], (float)out[8], (float)out[9]);
    p.dL_dstrengths[j] = (float)out[10];
}

}  // namespace

// FIELD_LANES lanes per Gaussian; lists longer than FIELD_HUB are left to field_hub_kernel
__global__ void __launch_bounds__(256)
field_gauss_kernel(FieldLaunch p)
{
    const size_t j = (size_t)blockIdx.x * (256 / FIELD_LANES) + threadIdx.x / FIELD_LANES;
    const uint32_t t = threadIdx.x % FIELD_LANES;
    const bool have = j < (size_t)p.P;
    const uint32_t begin = have ? p.seg_begin[j] : 0u, end = have ? p.seg_end[j] : 0u;
    const uint32_t len = end - begin;
    const bool mine = have && len <= FIELD_HUB;
    FieldOwn g;
    if (mine) g = field_own(p, j);
    double v[11];
#pragma unroll
    for (int c = 0; c < 11; c++) v[c] = 0.0;
    if (mine)
        for (uint32_t e = begin + t; e < end; e += FIELD_LANES) field_accumulate(p, g, p.vals_s[e], v);
#pragma unroll
    for (int c = 0; c < 11; c++) v[c] = group_sum<FIELD_LANES>(v[c]);
    if (mine && t == 0) field_store_rows(p, g, j, v, len == 0u);
}

// workgroup c looks at sorted position c * FIELD_HUB: the list that holds it is this workgroup's if it is longer than
// FIELD_HUB and that position is the first multiple of FIELD_HUB at or behind the list's begin
__global__ void __launch_bounds__(256)
field_hub_kernel(FieldLaunch p, uint32_t n)
{
    __shared__ double s_part[4][11];
    const uint32_t pos = blockIdx.x * FIELD_HUB;
    if (pos >= n) return;
    const uint32_t key = p.keys_s[pos];
    if (key >= (uint32_t)p.P) return;
    const uint32_t begin = p.seg_begin[key], end = p.seg_end[key];
    if (end - begin <= FIELD_HUB || pos < begin || pos - begin >= FIELD_HUB) return;      // workgroup-uniform
    const FieldOwn g = field_own(p, key);
    double v[11];
#pragma unroll
    for (int c = 0; c < 11; c++) v[c] = 0.0;
    for (uint32_t e = begin + threadIdx.x; e < end; e += 256u) field_accumulate(p, g, p.vals_s[e], v);
#pragma unroll
    for (int c = 0; c < 11; c++) v[c] = group_sum<64>(v[c]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int c = 0; c < 11; c++) s_part[threadIdx.x >> 6][c] = v[c];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 11; c++) v[c] = ((s_part[0][c] + s_part[1][c]) + s_part[2][c]) + s_part[3][c];
        field_store_rows(p, g, key, v, false);
    }
}

namespace {

struct FieldWs {
    float4* rec;
    double2* ab;
    uint32_t *keys, *keys_s, *vals_s, *seg_begin, *seg_end;
    void* sort_tmp;
    size_t sort_bytes, bytes;
};

int field_key_bits(int P) { int b = 1; while (b < 32 && (1ll << b) <= (long long)P) b++; return b; }       // keys 0 ... P

hipError_t field_sort(void* tmp, size_t& tmp_bytes, const uint32_t* keys, uint32_t* keys_s, uint32_t* vals_s, size_t n, int P,
                      hipStream_t s)
{
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, keys_s, rocprim::counting_iterator<uint32_t>(0u), vals_s, n, 0,
                                     field_key_bits(P), s);
}

// ws == nullptr only sizes
FieldWs field_carve(int P, int N, int K, bool backward, char* ws)
{
    FieldWs f{};
    size_t o = 0;
    auto take = [&](size_t bytes) { char* q = ws ? ws + o : nullptr; o += align_up(bytes, 256); return q; };
    const size_t Pp = (size_t)(P > 0 ? P : 1), Np = (size_t)(N > 0 ? N : 1), n = Np * (size_t)(K > 0 ? K : 1);
    if (!backward) {
        f.rec = (float4*)take(Pp * 64);
    } else {
        f.ab = (double2*)take(Np * 16);
        f.keys = (uint32_t*)take(n * 4);
        f.keys_s = (uint32_t*)take(n * 4);
        f.vals_s = (uint32_t*)take(n * 4);
        f.seg_begin = (uint32_t*)take(Pp * 4);
        f.seg_end = (uint32_t*)take(Pp * 4);
        (void)field_sort(nullptr, f.sort_bytes, nullptr, nullptr, nullptr, n, P, (hipStream_t)0);
        f.sort_tmp = take(f.sort_bytes);
    }
    f.bytes = o;
    return f;
}

template <bool BWD>
void launch_pair(const FieldLaunch& p, hipStream_t s)
{
    const int G = p.K <= 1 ? 1 : p.K <= 2 ? 2 : p.K <= 4 ? 4 : p.K <= 8 ? 8 : p.K <= 16 ? 16 : 32;
    const dim3 grid((unsigned)(((size_t)p.N * G + 255) / 256)), block(256);
    switch (G) {
    case 1: hipLaunchKernelGGL((field_pair_kernel<1, BWD>), grid, block, 0, s, p); break;
    case 2: hipLaunchKernelGGL((field_pair_kernel<2, BWD>), grid, block, 0, s, p); break;
    case 4: hipLaunchKernelGGL((field_pair_kernel<4, BWD>), grid, block, 0, s, p); break;
    case 8: hipLaunchKernelGGL((field_pair_kernel<8, BWD>), grid, block, 0, s, p); break;
    case 16: hipLaunchKernelGGL((field_pair_kernel<16, BWD>), grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL((field_pair_kernel<32, BWD>), grid, block, 0, s, p); break;
    }
}

}  // namespace

size_t field_workspace_bytes(int P, int N, int K, bool backward) { return field_carve(P, N, K, backward, nullptr).bytes; }

hipError_t launch_field_pack(int P, const float* points, const float* scaling, const float* quaternions, const float* strengths,
                             float4* rec, hipStream_t s)
{
    FieldLaunch p{};
    p.P = P; p.points = points; p.scaling = scaling; p.quaternions = quaternions; p.strengths = strengths; p.rec = rec;
    hipLaunchKernelGGL(field_pack_kernel, dim3((P + 255) / 256), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_field(FieldLaunch p, bool backward, char* ws, hipStream_t s)
{
    const FieldWs f = field_carve(p.P, p.N, p.K, backward, ws);
    hipError_t e;
    p.rec = f.rec;
    if (!backward && !p.recompute) {
        hipLaunchKernelGGL(field_pack_kernel, dim3((p.P + 255) / 256), dim3(256), 0, s, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (!backward) {
        launch_pair<false>(p, s);
        return hipGetLastError();
    }
    const size_t n = (size_t)p.N * (size_t)p.K;
    p.ab = f.ab; p.keys = f.keys; p.keys_s = f.keys_s; p.vals_s = f.vals_s; p.seg_begin = f.seg_begin; p.seg_end = f.seg_end;
    launch_pair<true>(p, s);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t sort_bytes = f.sort_bytes;
    if ((e = field_sort(f.sort_tmp, sort_bytes, f.keys, f.keys_s, f.vals_s, n, p.P, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(f.seg_begin, 0, (size_t)p.P * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(f.seg_end, 0, (size_t)p.P * 4, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(field_segment_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (uint32_t)n, (uint32_t)p.P, f.keys_s,
                       f.seg_begin, f.seg_end);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int per_block = 256 / FIELD_LANES;
    hipLaunchKernelGGL(field_gauss_kernel, dim3((p.P + per_block - 1) / per_block), dim3(256), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (n > FIELD_HUB) {
        hipLaunchKernelGGL(field_hub_kernel, dim3((unsigned)((n + FIELD_HUB - 1) / FIELD_HUB)), dim3(256), 0, s, p, (uint32_t)n);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace frg
