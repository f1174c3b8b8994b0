// Mean squared distance to the three nearest neighbours of every point.
//
// Replaces simple-knn's distCUDA2 (gaussian_splatting/submodules/simple-knn/simple_knn.cu:64-222,
// spatial.cu:15-26), which initialises the Gaussians' scales (gaussian_model.py:134,
// frosting_model.py:530).  The value is fully specified -- for point p the three smallest
// |p - q|^2 over q != p, summed smallest first and divided by 3 -- so any exact search gives the
// reference's numbers; this one is organised for a wave64 machine:
//   1. bounding box by order-preserving integer atomics, 30-bit Morton codes, one rocPRIM radix sort
//      of (code, index) pairs (the only global sort in this library), points gathered into Morton order;
//   2. leaf boxes of KNN_LEAF consecutive sorted points with their bounds;
//   3. one query per lane, 256 queries per workgroup over the same stretch of the curve: the leaf table
//      is streamed through LDS in slabs, a leaf is opened when ANY lane's current third-best distance
//      reaches it (ballot), its points are staged in LDS once for the workgroup and scanned by the lanes
//      that need it.  The own and the neighbouring leaves go first, so the bound is tight before the sweep.
// Squared distances are evaluated as (dx*dx + dy*dy) + dz*dz without contraction (the order of
// simple_knn.cu:150-151), the result as (b0 + b1 + b2) / 3.0f (:197).
//
// The second half of the file is the general search over the same structure: the K nearest points of a set p2
// for every point of a set p1, with their indices (pytorch3d.ops.knn_points; see knn_points_kernel).
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "kernels.h"

#pragma clang fp contract(off)

namespace frg {

#define KNN_LEAF 256
#define KNN_SLAB 1024          // leaf descriptors staged per sweep step (24 KB)

__device__ __forceinline__ uint32_t f2ord(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// bbox[0..2] = min (ordered ints), bbox[3..5] = max; initialised to 0xFFFFFFFF / 0 by the host memsets
__global__ void __launch_bounds__(256)
knn_bbox_kernel(int P, const float* __restrict__ pts, uint32_t* __restrict__ bbox)
{
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256)
#pragma unroll
        for (int c = 0; c < 3; c++) { const float v = pts[3 * i + c]; lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v); }
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo[c] = fminf(lo[c], __shfl_xor(lo[c], d, 64));
            hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], d, 64));
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(&bbox[c], f2ord(lo[c])); atomicMax(&bbox[3 + c], f2ord(hi[c])); }
    }
}

__device__ __forceinline__ uint32_t spread10(uint32_t x)
{
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__global__ void __launch_bounds__(256)
knn_morton_kernel(int P, const float* __restrict__ pts, const uint32_t* __restrict__ bbox, uint32_t* __restrict__ codes,
                  uint32_t* __restrict__ idx)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    uint32_t q[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float lo = ord2f(bbox[c]), hi = ord2f(bbox[3 + c]);
        const float ext = hi - lo;
        const float t = ext > 0.f ? (pts[3 * i + c] - lo) / ext : 0.f;
        q[c] = (uint32_t)fminf(fmaxf(t * 1023.0f, 0.f), 1023.f);
    }
    codes[i] = spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2);
    idx[i] = (uint32_t)i;
}

// points in Morton order (float4: x, y, z, original index bits) and the bounds of every leaf
__global__ void __launch_bounds__(KNN_LEAF)
knn_leaf_kernel(int P, const float* __restrict__ pts, const uint32_t* __restrict__ order, float4* __restrict__ sorted,
                float* __restrict__ leaf_lo, float* __restrict__ leaf_hi)
{
    const int i = blockIdx.x * KNN_LEAF + threadIdx.x;
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    if (i < P) {
        const uint32_t o = order[i];
        const float x = pts[3 * o], y = pts[3 * o + 1], z = pts[3 * o + 2];
        sorted[i] = make_float4(x, y, z, __uint_as_float(o));
        lo[0] = hi[0] = x; lo[1] = hi[1] = y; lo[2] = hi[2] = z;
    }
    __shared__ float red[6][KNN_LEAF / 64];
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo[c] = fminf(lo[c], __shfl_xor(lo[c], d, 64));
            hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], d, 64));
        }
        if ((threadIdx.x & 63) == 0) { red[c][threadIdx.x >> 6] = lo[c]; red[3 + c][threadIdx.x >> 6] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float a = red[threadIdx.x][0], b = red[3 + threadIdx.x][0];
        for (int w = 1; w < KNN_LEAF / 64; w++) { a = fminf(a, red[threadIdx.x][w]); b = fmaxf(b, red[3 + threadIdx.x][w]); }
        leaf_lo[3 * blockIdx.x + threadIdx.x] = a;
        leaf_hi[3 * blockIdx.x + threadIdx.x] = b;
    }
}

__device__ __forceinline__ void keep3(float d, float* best)
{
    // simple_knn.cu:147-160: insertion into the ascending triple
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (best[j] > d) { const float t = best[j]; best[j] = d; d = t; }
}

__device__ __forceinline__ float box_dist2(const float* lo, const float* hi, float x, float y, float z)
{
    const float dx = fmaxf(fmaxf(lo[0] - x, x - hi[0]), 0.f);
    const float dy = fmaxf(fmaxf(lo[1] - y, y - hi[1]), 0.f);
    const float dz = fmaxf(fmaxf(lo[2] - z, z - hi[2]), 0.f);
    return (dx * dx + dy * dy) + dz * dz;
}

// workgroup = KNN_LEAF threads = the queries of one leaf
__global__ void __launch_bounds__(KNN_LEAF)
knn_search_kernel(int P, int nleaf, const float4* __restrict__ sorted, const float* __restrict__ leaf_lo,
                  const float* __restrict__ leaf_hi, float* __restrict__ out)
{
    __shared__ float4 s_pts[KNN_LEAF];
    __shared__ float s_lo[KNN_SLAB * 3], s_hi[KNN_SLAB * 3];
    __shared__ uint32_t s_open[KNN_SLAB / 32];      // bitmap: leaves of the slab some query must still open
    const int me = blockIdx.x * KNN_LEAF + threadIdx.x;
    const bool live = me < P;
    const float4 q = live ? sorted[me] : make_float4(0.f, 0.f, 0.f, 0.f);
    float best[3] = {3.402823466e38f, 3.402823466e38f, 3.402823466e38f};   // FLT_MAX (:169)

    auto scan_leaf = [&](int leaf, bool need) {          // all threads call; `need` selects who scans
        __syncthreads();
        const int j = leaf * KNN_LEAF + threadIdx.x;
        s_pts[threadIdx.x] = j < P ? sorted[j] : make_float4(3.0e18f, 3.0e18f, 3.0e18f, 0.f);
        __syncthreads();
        if (need) {
            const int cnt = min(KNN_LEAF, P - leaf * KNN_LEAF);
            for (int k = 0; k < cnt; k++) {
                if (leaf * KNN_LEAF + k == me) continue;
                const float4 p = s_pts[k];
                const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
                keep3((dx * dx + dy * dy) + dz * dz, best);
            }
        }
    };
    // own leaf and its two neighbours on the curve first: a tight bound before the sweep
    const int own = blockIdx.x;
    scan_leaf(own, live);
    if (own > 0) scan_leaf(own - 1, live);
    if (own + 1 < nleaf) scan_leaf(own + 1, live);

    for (int base = 0; base < nleaf; base += KNN_SLAB) {
        const int cnt = min(KNN_SLAB, nleaf - base);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt * 3; i += KNN_LEAF) { s_lo[i] = leaf_lo[base * 3 + i]; s_hi[i] = leaf_hi[base * 3 + i]; }
        if (threadIdx.x < KNN_SLAB / 32) s_open[threadIdx.x] = 0u;
        __syncthreads();
        // which leaves of this slab does ANY query of the workgroup still have to open?
        for (int l = 0; l < cnt; l++) {
            const int leaf = base + l;
            if (leaf >= own - 1 && leaf <= own + 1) continue;
            const bool need = live && !(box_dist2(s_lo + 3 * l, s_hi + 3 * l, q.x, q.y, q.z) > best[2]);
            if (__ballot(need) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&s_open[l >> 5], 1u << (l & 31));
        }
        __syncthreads();
        // open them in ascending order (workgroup-uniform walk over the bitmap); the bound is re-tested
        // per query with its current third-best distance
        for (int w = 0; w < (cnt + 31) / 32; w++) {
            uint32_t bits = s_open[w];
            while (bits) {
                const int l = w * 32 + __builtin_ctz(bits);
                bits &= bits - 1u;
                const bool need = live && !(box_dist2(s_lo + 3 * l, s_hi + 3 * l, q.x, q.y, q.z) > best[2]);
                scan_leaf(base + l, need);
            }
        }
    }
    if (live) out[__float_as_uint(q.w)] = (best[0] + best[1] + best[2]) / 3.0f;
}

// ---- K nearest neighbours between two point sets (pytorch3d.ops.knn_points) -----------------------------------
// The same structure over the searched set p2; the queries p1 get Morton codes in p2's bounding box (clamped: a
// query may lie far outside it) and are sorted too, so the 256 lanes of a workgroup hold neighbouring queries (a
// self-query reuses p2's order).  Every lane finds the leaf whose code range contains its query by binary search
// over the leaves' first codes and scans that leaf and its two neighbours on the curve first; then the leaf table
// is swept in slabs through LDS as in knn_search_kernel.  A leaf is opened when !(box_dist2 > worst kept) holds
// for any lane: equality must open, because an equal-distance point with a smaller index displaces a kept one.
// Every lane keeps the KC best (distance, index in p2) pairs, ascending in that lexicographic order, in registers
// (KC = capacity, a template parameter >= K; every loop over the list is unrolled, so no slot is addressed at run
// time).  A leaf is scanned at most once per lane, so no pair can enter a list twice.

#define KNN_NONE 0xFFFFFFFFu   // index of an empty slot: (inf, KNN_NONE) is above every real pair

template <int KC>
__device__ __forceinline__ void keepk(float d, uint32_t i, float* bd, uint32_t* bi)
{
#pragma unroll
    for (int j = 0; j < KC; j++) {
        const bool lt = d < bd[j] || (d == bd[j] && i < bi[j]);
        const float td = bd[j];
        const uint32_t ti = bi[j];
        bd[j] = lt ? d : td; bi[j] = lt ? i : ti;
        d = lt ? td : d; i = lt ? ti : i;
    }
}

// queries in Morton order (float4: x, y, z, original row bits)
__global__ void __launch_bounds__(256)
knn_query_gather_kernel(int P, const float* __restrict__ pts, const uint32_t* __restrict__ order, float4* __restrict__ sorted)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const uint32_t o = order[i];
    sorted[i] = make_float4(pts[3 * o], pts[3 * o + 1], pts[3 * o + 2], __uint_as_float(o));
}

// workgroup = KNN_LEAF consecutive queries of the sorted order; qcodes == nullptr: a self-query, the queries are
// `sorted` itself and the own leaf is the workgroup's
template <int KC>
__global__ void __launch_bounds__(KNN_LEAF)
knn_points_kernel(int P1, int P2, int nleaf, int K, const float4* __restrict__ queries, const uint32_t* __restrict__ qcodes,
                  const float4* __restrict__ sorted, const uint32_t* __restrict__ codes, const float* __restrict__ leaf_lo,
                  const float* __restrict__ leaf_hi, float* __restrict__ dists, long long* __restrict__ idx)
{
    __shared__ float4 s_pts[KNN_LEAF];
    __shared__ float s_lo[KNN_SLAB * 3], s_hi[KNN_SLAB * 3];
    __shared__ uint32_t s_open[KNN_SLAB / 32];
    __shared__ int s_range[2];
    const int me = blockIdx.x * KNN_LEAF + threadIdx.x;
    const bool live = me < P1;
    const float4 q = live ? queries[me] : make_float4(0.f, 0.f, 0.f, 0.f);
    float bd[KC];
    uint32_t bi[KC];
#pragma unroll
    for (int j = 0; j < KC; j++) { bd[j] = __builtin_inff(); bi[j] = KNN_NONE; }

    // the leaf whose code range contains the query: the last leaf whose first code is not above the query's
    int own = blockIdx.x;
    if (qcodes) {
        const uint32_t c = live ? qcodes[me] : 0u;
        int lo = 0, hi = nleaf;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (codes[(size_t)mid * KNN_LEAF] <= c) lo = mid; else hi = mid;
        }
        own = lo;
    }
    // the queries are sorted by code, so the workgroup's leaves run from the first lane's to the last live lane's
    if (threadIdx.x == 0) s_range[0] = own;
    if (threadIdx.x == min(KNN_LEAF, P1 - (int)blockIdx.x * KNN_LEAF) - 1) s_range[1] = own;
    __syncthreads();
    const int first = max(s_range[0] - 1, 0), last = min(s_range[1] + 1, nleaf - 1);

    auto scan_leaf = [&](int leaf, bool need) {          // all threads call; `need` selects who scans
        __syncthreads();
        const int j = leaf * KNN_LEAF + threadIdx.x;
        s_pts[threadIdx.x] = j < P2 ? sorted[j] : make_float4(3.0e18f, 3.0e18f, 3.0e18f, 0.f);
        __syncthreads();
        if (need) {
            const int cnt = min(KNN_LEAF, P2 - leaf * KNN_LEAF);
            for (int k = 0; k < cnt; k++) {
                const float4 p = s_pts[k];
                const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
                const float d = (dx * dx + dy * dy) + dz * dz;
                if (!(d > bd[KC - 1])) keepk<KC>(d, __float_as_uint(p.w), bd, bi);
            }
        }
    };
    // own leaf and its two neighbours on the curve first: a tight bound before the sweep.  Between two sets the
    // workgroup's queries may straddle many leaves; one no lane is next to is not staged.
    for (int leaf = first; leaf <= last; leaf++) {
        const bool need = live && leaf >= own - 1 && leaf <= own + 1;
        if (last - first > 2 && !__syncthreads_or(need)) continue;
        scan_leaf(leaf, need);
    }

    for (int base = 0; base < nleaf; base += KNN_SLAB) {
        const int cnt = min(KNN_SLAB, nleaf - base);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt * 3; i += KNN_LEAF) { s_lo[i] = leaf_lo[base * 3 + i]; s_hi[i] = leaf_hi[base * 3 + i]; }
        if (threadIdx.x < KNN_SLAB / 32) s_open[threadIdx.x] = 0u;
        __syncthreads();
        for (int l = 0; l < cnt; l++) {
            const int leaf = base + l;
            const bool need = live && (leaf < own - 1 || leaf > own + 1) &&
                              !(box_dist2(s_lo + 3 * l, s_hi + 3 * l, q.x, q.y, q.z) > bd[KC - 1]);
            if (__ballot(need) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&s_open[l >> 5], 1u << (l & 31));
        }
        __syncthreads();
        for (int w = 0; w < (cnt + 31) / 32; w++) {
            uint32_t bits = s_open[w];
            while (bits) {
                const int l = w * 32 + __builtin_ctz(bits);
                bits &= bits - 1u;
                const int leaf = base + l;
                const bool need = live && (leaf < own - 1 || leaf > own + 1) &&
                                  !(box_dist2(s_lo + 3 * l, s_hi + 3 * l, q.x, q.y, q.z) > bd[KC - 1]);
                scan_leaf(leaf, need);
            }
        }
    }
    if (live) {
        const size_t row = (size_t)__float_as_uint(q.w) * (size_t)K;
#pragma unroll
        for (int j = 0; j < KC; j++)
            if (j < K) {                                 // empty slots (K > P2): pytorch3d's padding
                const bool none = bi[j] == KNN_NONE;
                dists[row + j] = none ? 0.f : bd[j];
                idx[row + j] = none ? 0ll : (long long)bi[j];
            }
    }
}

namespace {

// the search structure of one point set, carved from a workspace
struct KnnSet {
    uint32_t *bbox, *codes, *codes_s, *idx, *idx_s;
    float4* sorted;
    float *leaf_lo, *leaf_hi;
    void* sort_tmp;
    size_t bytes;
};

size_t knn_sort_bytes(size_t n)
{
    size_t sort_tmp = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                    (uint32_t*)nullptr, n, 0, 30, (hipStream_t)0);
    return sort_tmp;
}

// ws == nullptr only sizes the structure
KnnSet knn_carve(int P, char* ws)
{
    const size_t Pp = (size_t)(P > 0 ? P : 1), nleaf = (Pp + KNN_LEAF - 1) / KNN_LEAF;
    KnnSet k;
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = ws ? ws + o : nullptr; o += bytes; return p; };
    k.bbox = (uint32_t*)take(256);
    k.codes = (uint32_t*)take(align_up(Pp * 4, 256));
    k.codes_s = (uint32_t*)take(align_up(Pp * 4, 256));
    k.idx = (uint32_t*)take(align_up(Pp * 4, 256));
    k.idx_s = (uint32_t*)take(align_up(Pp * 4, 256));
    k.sorted = (float4*)take(align_up(Pp * 16, 256));
    k.leaf_lo = (float*)take(align_up(nleaf * 12, 256));
    k.leaf_hi = (float*)take(align_up(nleaf * 12, 256));
    k.sort_tmp = take(align_up(knn_sort_bytes(Pp), 256));
    k.bytes = o;
    return k;
}

// bounding box, Morton codes, sort, points in Morton order, leaf bounds
hipError_t knn_build(int P, const float* pts, const KnnSet& k, hipStream_t s)
{
    const size_t Pp = (size_t)P;
    const int nleaf = (P + KNN_LEAF - 1) / KNN_LEAF;
    size_t sort_bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, k.codes, k.codes_s, k.idx, k.idx_s, Pp, 0, 30, s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(k.bbox, 0xFF, 12, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(k.bbox + 3, 0x00, 12, s)) != hipSuccess) return e;
    const int rb = min(1024, (P + 255) / 256);
    hipLaunchKernelGGL(knn_bbox_kernel, dim3(rb), dim3(256), 0, s, P, pts, k.bbox);
    hipLaunchKernelGGL(knn_morton_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, pts, k.bbox, k.codes, k.idx);
    if ((e = rocprim::radix_sort_pairs(k.sort_tmp, sort_bytes, k.codes, k.codes_s, k.idx, k.idx_s, Pp, 0, 30, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(knn_leaf_kernel, dim3(nleaf), dim3(KNN_LEAF), 0, s, P, pts, k.idx_s, k.sorted, k.leaf_lo, k.leaf_hi);
    return hipGetLastError();
}

// the sorted queries of a two-set search, behind the set's structure
struct KnnQueries {
    uint32_t *codes, *codes_s, *idx, *idx_s;
    float4* sorted;
    void* sort_tmp;
    size_t bytes;
};

KnnQueries knn_carve_queries(int P1, char* ws)
{
    KnnQueries k;
    std::memset(&k, 0, sizeof(k));
    if (P1 <= 0) return k;
    const size_t Pp = (size_t)P1;
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = ws ? ws + o : nullptr; o += bytes; return p; };
    k.codes = (uint32_t*)take(align_up(Pp * 4, 256));
    k.codes_s = (uint32_t*)take(align_up(Pp * 4, 256));
    k.idx = (uint32_t*)take(align_up(Pp * 4, 256));
    k.idx_s = (uint32_t*)take(align_up(Pp * 4, 256));
    k.sorted = (float4*)take(align_up(Pp * 16, 256));
    k.sort_tmp = take(align_up(knn_sort_bytes(Pp), 256));
    k.bytes = o;
    return k;
}

}  // namespace

size_t knn_workspace_bytes(int P) { return knn_carve(P, nullptr).bytes; }

hipError_t launch_knn(int P, const float* pts, float* out, char* ws, hipStream_t s)
{
    const int nleaf = (P + KNN_LEAF - 1) / KNN_LEAF;
    const KnnSet k = knn_carve(P, ws);
    hipError_t e = knn_build(P, pts, k, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(knn_search_kernel, dim3(nleaf), dim3(KNN_LEAF), 0, s, P, nleaf, k.sorted, k.leaf_lo, k.leaf_hi, out);
    return hipGetLastError();
}

int knn_points_capacity(int K) { return K <= 1 ? 1 : K <= 4 ? 4 : K <= 8 ? 8 : K <= 16 ? 16 : 32; }

// P1 = 0 sizes a self-query (the queries are the set's own sorted points)
size_t knn_points_workspace_bytes(int P1, int P2, int K)
{
    (void)K;                                             // the lists live in registers
    return knn_carve(P2, nullptr).bytes + knn_carve_queries(P1, nullptr).bytes;
}

template <int KC>
static void launch_points_kernel(int P1, int P2, int K, const float4* queries, const uint32_t* qcodes, const KnnSet& k,
                                 float* dists, long long* idx, hipStream_t s)
{
    const int nleaf = (P2 + KNN_LEAF - 1) / KNN_LEAF;
    hipLaunchKernelGGL(knn_points_kernel<KC>, dim3((P1 + KNN_LEAF - 1) / KNN_LEAF), dim3(KNN_LEAF), 0, s, P1, P2, nleaf, K,
                       queries, qcodes, k.sorted, k.codes_s, k.leaf_lo, k.leaf_hi, dists, idx);
}

hipError_t launch_knn_points(int P1, const float* p1, int P2, const float* p2, int K, bool self, float* dists, long long* idx,
                             char* ws, hipStream_t s)
{
    const KnnSet k = knn_carve(P2, ws);
    hipError_t e = knn_build(P2, p2, k, s);
    if (e != hipSuccess) return e;
    const float4* queries = k.sorted;
    const uint32_t* qcodes = nullptr;
    if (!self) {
        const KnnQueries qs = knn_carve_queries(P1, ws + k.bytes);
        const size_t Pp = (size_t)P1;
        size_t sort_bytes = 0;
        if ((e = rocprim::radix_sort_pairs(nullptr, sort_bytes, qs.codes, qs.codes_s, qs.idx, qs.idx_s, Pp, 0, 30, s)) != hipSuccess) return e;
        // codes in p2's bounding box: knn_morton_kernel clamps the cell coordinates
        hipLaunchKernelGGL(knn_morton_kernel, dim3((P1 + 255) / 256), dim3(256), 0, s, P1, p1, k.bbox, qs.codes, qs.idx);
        if ((e = rocprim::radix_sort_pairs(qs.sort_tmp, sort_bytes, qs.codes, qs.codes_s, qs.idx, qs.idx_s, Pp, 0, 30, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(knn_query_gather_kernel, dim3((P1 + 255) / 256), dim3(256), 0, s, P1, p1, qs.idx_s, qs.sorted);
        queries = qs.sorted;
        qcodes = qs.codes_s;
    }
    switch (knn_points_capacity(K)) {
    case 1: launch_points_kernel<1>(P1, P2, K, queries, qcodes, k, dists, idx, s); break;
    case 4: launch_points_kernel<4>(P1, P2, K, queries, qcodes, k, dists, idx, s); break;
    case 8: launch_points_kernel<8>(P1, P2, K, queries, qcodes, k, dists, idx, s); break;
    case 16: launch_points_kernel<16>(P1, P2, K, queries, qcodes, k, dists, idx, s); break;
    default: launch_points_kernel<32>(P1, P2, K, queries, qcodes, k, dists, idx, s); break;
    }
    return hipGetLastError();
}

}  // namespace frg
