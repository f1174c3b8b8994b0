// Slot-sum exchange of the view-parallel step (no counterpart in the single-GPU reference).
//
// After phase 1 of the backward (blend backward + slot reduction) everything one view contributes to the gradient of a
// Gaussian is determined by TWELVE floats -- the clamp-masked colour gradient, the six pixel moments of G dL/dalpha
// (preprocess_bwd.hip, "sums") and the three view-direction terms d(colour)/d(direction) . dRGB (what phase 2 forms from the
// forward's sh_dir) -- together with data every rank already holds: the parameters and the view's camera.
// And only the Gaussians some pixel reached before its tile saturated have sums at all (one in eight at C3).  So the
// ranks exchange those sums instead of finished gradients:
//
//   pack     the rows {dRGB[3], moments[6], dd[3]} (48 bytes) of the Gaussians with a gradient, IN INDEX ORDER, behind a bit mask
//            (one bit per Gaussian) and one row offset per block of 64 Gaussians: Gaussian g finds its row in view v as
//            base[v][g / 64] + popcount(mask[v][g / 64] below g).  Fixed capacity: no host wait for a count.
//   gather   one all-gather of the packets (host side: frosting_amd/parallel.py).
//   combine  ONE pass over the Gaussians: for every view that has a row, in VIEW ORDER, the per-Gaussian backward chain of
//            preprocess_bwd.hip (sections 2-5: cov2D, projection, SH, cov3D -> scale / quaternion) with that view's camera,
//            the 59 gradient floats accumulated in registers and every row written once -- the single-process accumulation
//            of the per-view gradients, bit for bit (same expressions, no contraction, same order of additions), without
//            the dense zero fills, per-view scatters and SH rebuild of the round-5 plans.
//
// What a view's geometry record held for phase 2 -- conic and opacity -- is recomputed here from the parameters with the
// forward's own functions (gauss_math.h), bit-identically.  The view-direction terms travel in the rows because forming them
// needs the 192-byte SH row of the Gaussian: read once per (Gaussian, view) pair by every rank, those rows were the larger
// part of the combine pass's memory traffic (0.84 GB fetched for eight C3 views; 12 more bytes per row on the wire instead).
#include "gauss_math.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace frg {

// ---- packet layout (uint32 words) -------------------------------------------------------------------------------------------
//   [0] rows packed  [1] rows wanted (> capacity: overflow)  [2] Gaussians of the packet  [3] capacity  [4] first Gaussian
//   [5] magic  [8..23] viewmatrix  [24..39] projmatrix  [40..42] camera centre  [43] tan_fovx  [44] tan_fovy
//   [45] width  [46] height  [47] scale_modifier  [48] active SH degree  [49] focal_x  [50] focal_y (api.hip make_view's)
//   masks   uint64[nblk]  at word 64                 (nblk = blocks of 64 Gaussians)
//   bases   uint32[nblk]  behind them, 16-byte aligned
//   rows    float[capacity][12] behind them, 16-byte aligned
//   visible uint64[nblk]  behind the rows, 16-byte aligned -- OPTIONAL (frg_pack_sum_rows_ex with radii): bit g % 64 of word g / 64 =
//           radii[first + g] > 0; header word [6] = the section's word offset, 0 = the packet has none
__host__ __device__ inline size_t sum_packet_blocks(size_t n) { return (n + 63) / 64; }
__host__ __device__ inline size_t sum_packet_bases_word(size_t n) { return FRG_SUM_HDR_WORDS + 2 * sum_packet_blocks(n); }
__host__ __device__ inline size_t sum_packet_rows_word(size_t n) { return (sum_packet_bases_word(n) + sum_packet_blocks(n) + 3) / 4 * 4; }
size_t sum_packet_bytes(size_t n, size_t capacity) { return ((sum_packet_rows_word(n) + FRG_SUM_ROW_FLOATS * capacity + 3) / 4 * 4) * 4; }
__host__ __device__ inline size_t sum_packet_visible_word(size_t n, size_t capacity) { return (sum_packet_rows_word(n) + FRG_SUM_ROW_FLOATS * capacity + 3) / 4 * 4; }
size_t sum_packet_bytes_visible(size_t n, size_t capacity) { return ((sum_packet_visible_word(n, capacity) + 2 * sum_packet_blocks(n) + 3) / 4 * 4) * 4; }

// Pack, two launches over the packet's blocks of 64 Gaussians:
//   sum_rows_local_kernel   one thread per block, 256 blocks per workgroup: the mask word (copied from the phase-1 workspace),
//                           its popcount, the exclusive prefix WITHIN the group of 256 blocks -> bases[], the group's total ->
//                           group_tot[] (scratch behind the masks in the workspace);
//   sum_rows_pack_kernel    one wave per block: the prefix of the groups before its own (a few hundred totals: three loads
//                           per lane and a wave scan) makes bases[] global; the rows of the marked Gaussians, in index order;
//                           the first wave writes the header (rows wanted = the sum of all totals, the camera).
// (Round 6's first forms scanned all blocks in ONE workgroup: 70, 30 and again 70 us per packet of 47 000 blocks -- one CU's
// load path.)
// VIS (frg_pack_sum_rows_ex with radii): the wave that packs a block of 64 Gaussians also ballots radii > 0 over it -- the
// packet's visibility section, what the densification statistics of the view need beside its rows (densify_views_kernel).
#define SUM_GROUP 256
__global__ void __launch_bounds__(SUM_GROUP)
sum_rows_local_kernel(int first, int n, const unsigned long long* __restrict__ live_masks, uint32_t* __restrict__ packet,
                      uint32_t* __restrict__ group_tot)
{
    __shared__ uint32_t wave_tot[SUM_GROUP / 64];
    const int nblk = (int)sum_packet_blocks((size_t)n), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x * SUM_GROUP + tid;
    const unsigned long long m = b < nblk ? (live_masks + first / 64)[b] : 0ull;
    const uint32_t c = (uint32_t)__popcll(m), incl = wave_incl_scan_dpp(c);
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SUM_GROUP / 64; w++) { const uint32_t t = wave_tot[w]; if (w < wave) before += t; total += t; }
    if (b < nblk) {
        reinterpret_cast<unsigned long long*>(packet + FRG_SUM_HDR_WORDS)[b] = m;
        (packet + sum_packet_bases_word((size_t)n))[b] = before + incl - c;
    }
    if (tid == 0) group_tot[blockIdx.x] = total;
}

template <bool VIS>
__global__ void __launch_bounds__(256)
sum_rows_pack_kernel(int first, int n, uint32_t capacity, const float* __restrict__ sums, const float* __restrict__ view_dir_terms,
                     const float* __restrict__ drgb_masked, uint32_t* __restrict__ packet, const uint32_t* __restrict__ group_tot, SumCamera cam,
                     const float* __restrict__ viewmatrix, const float* __restrict__ projmatrix, const float* __restrict__ campos,
                     const int* __restrict__ radii)
{
    const int lane = threadIdx.x & 63, blk = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nblk = (int)sum_packet_blocks((size_t)n);
    if (blk >= nblk) return;
    if (VIS) {
        const int gl = blk * 64 + lane;
        const unsigned long long seen = __builtin_amdgcn_ballot_w64(gl < n && radii[(size_t)first + gl] > 0);
        if (lane == 0) reinterpret_cast<unsigned long long*>(packet + sum_packet_visible_word((size_t)n, (size_t)capacity))[blk] = seen;
    }
    const int ngroups = (nblk + SUM_GROUP - 1) / SUM_GROUP, grp = blk / SUM_GROUP;
    // rows before this block's group (and, for the header, of all groups)
    uint32_t before = 0, all = 0;
    for (int j = lane; j < ngroups; j += 64) { const uint32_t t = group_tot[j]; all += t; if (j < grp) before += t; }
    before = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_dpp(before), 63);
    uint32_t* bases = packet + sum_packet_bases_word((size_t)n);
    const uint32_t base = before + bases[blk];
    if (blk == 0) {
        all = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_dpp(all), 63);
        float* f = reinterpret_cast<float*>(packet);
        if (lane < 16) { f[8 + lane] = viewmatrix[lane]; f[24 + lane] = projmatrix[lane]; }
        if (lane < 3) f[40 + lane] = campos[lane];
        if (lane >= 51 && lane < FRG_SUM_HDR_WORDS) packet[lane] = 0u;
        if (lane == 0) {
            packet[0] = all < capacity ? all : capacity;
            packet[1] = all;
            packet[2] = (uint32_t)n; packet[3] = capacity; packet[4] = (uint32_t)first; packet[5] = FRG_SUM_MAGIC;
            packet[6] = VIS ? (uint32_t)sum_packet_visible_word((size_t)n, (size_t)capacity) : 0u; packet[7] = 0u;
            f[43] = cam.tan_fovx; f[44] = cam.tan_fovy;
            packet[45] = (uint32_t)cam.width; packet[46] = (uint32_t)cam.height;
            f[47] = cam.scale_modifier; packet[48] = (uint32_t)cam.D;
            f[49] = cam.width / (2.0f * cam.tan_fovx);        // rasterizer_impl.cu:222-223, as api.hip make_view forms them
            f[50] = cam.height / (2.0f * cam.tan_fovy);
        }
    }
    const unsigned long long m = reinterpret_cast<const unsigned long long*>(packet + FRG_SUM_HDR_WORDS)[blk];
    if (lane == 0) bases[blk] = base;                   // (this wave alone reads and writes the block's entry)
    if (!((m >> lane) & 1ull)) return;
    const uint32_t row = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (row >= capacity) return;                 // (over capacity: the header says so; the host packs again into a larger packet)
    const size_t g = (size_t)first + (size_t)blk * 64 + lane;
    float4* dst = reinterpret_cast<float4*>(reinterpret_cast<float*>(packet) + sum_packet_rows_word((size_t)n) + (size_t)row * FRG_SUM_ROW_FLOATS);
    const float* sp = sums + g * FRG_SLOT_FLOATS;
    const float* dd = view_dir_terms + 3 * g;
    dst[0] = make_float4(drgb_masked[3 * g], drgb_masked[3 * g + 1], drgb_masked[3 * g + 2], sp[3]);
    dst[1] = make_float4(sp[4], sp[5], sp[6], sp[7]);
    dst[2] = make_float4(sp[8], dd[0], dd[1], dd[2]);
}

hipError_t launch_pack_sum_rows(int first, int n, uint32_t capacity, const unsigned long long* live_masks, const float* sums,
                                const float* view_dir_terms, const float* drgb_masked, const SumCamera& cam, const float* viewmatrix, const float* projmatrix,
                                const float* campos, void* packet, uint32_t* group_tot, hipStream_t s, const int* radii)
{
    uint32_t* pk = reinterpret_cast<uint32_t*>(packet);
    const int nblk = (int)sum_packet_blocks((size_t)n);
    hipLaunchKernelGGL(sum_rows_local_kernel, dim3((nblk + SUM_GROUP - 1) / SUM_GROUP), dim3(SUM_GROUP), 0, s, first, n, live_masks, pk, group_tot);
    if (radii)
        hipLaunchKernelGGL(sum_rows_pack_kernel<true>, dim3((nblk + 3) / 4), dim3(256), 0, s, first, n, capacity, sums, view_dir_terms, drgb_masked, pk, group_tot,
                           cam, viewmatrix, projmatrix, campos, radii);
    else
        hipLaunchKernelGGL(sum_rows_pack_kernel<false>, dim3((nblk + 3) / 4), dim3(256), 0, s, first, n, capacity, sums, view_dir_terms, drgb_masked, pk, group_tot,
                           cam, viewmatrix, projmatrix, campos, radii);
    return hipGetLastError();
}

// ---- combine ------------------------------------------------------------------------------------------------------------------
#define CMB_MAX_VIEWS 16
#define CMB_ACC 11

// A view's camera = words 8 .. 50 of its packet header, copied to LDS once per workgroup (CAM_WORDS floats per view at an odd
// stride: lanes that look at different views hit different banks).  Offsets inside a view's camera:
#define CAM_WORDS 43
#define CAM_STRIDE 45
#define CAM_VIEW 0
#define CAM_PROJ 16
#define CAM_POS 32
#define CAM_TANX 35
#define CAM_TANY 36
#define CAM_W 37
#define CAM_H 38
#define CAM_SCALE 39
#define CAM_D 40
#define CAM_FX 41
#define CAM_FY 42

// sections 2, 3 and 5 of preprocess_bwd_kernel, and the view-direction term of section 4, for ONE (Gaussian, view): `part` = the
// view's nine slot sums of the Gaussian (the colour part clamp-masked), dd = its three view-direction terms.  Writes the view's
// eleven terms to out[11].  Expression for expression the chain of preprocess_bwd.hip (has_grad branch); tests pin the two bit
// for bit.  Raw-parameter mode (raw_params.h): the activations' Jacobians are applied per view, as phase 2 applies them.
// cam: the view's camera in LDS (per lane: the lanes of a wave work on different views).
// (cam_at(): the camera's LDS offset made opaque anew in front of every section, so that its ~45 values are read where they are
// used instead of being loaded -- and held in 45 vector registers -- ahead of the whole chain)
__device__ __forceinline__ const float* cam_at(const float* __restrict__ cams, int off) { asm volatile("" : "+v"(off)); return cams + off; }
__device__ __forceinline__ void combine_one_view(const float* __restrict__ cams, const int cam_off, const float3 mean, const float3 sc, const float4 q, const float o,
                                                 const bool raw_opacity, const bool raw_scale, const bool raw_rot, const float4 q_raw,
                                                 float (&part)[FRG_SLOT_FLOATS], const float dd0, const float dd1, const float dd2,
                                                 float* __restrict__ out /* [11]: mean3D 3, scale 3, rot 4, opacity */)
{
    const float* cam = cam_at(cams, cam_off);
    const float* vmat = cam + CAM_VIEW;
    const float scale_modifier = cam[CAM_SCALE], focal_x = cam[CAM_FX], focal_y = cam[CAM_FY];
    const float half_w = 0.5f * (float)__float_as_int(cam[CAM_W]), half_h = 0.5f * (float)__float_as_int(cam[CAM_H]);
    // the forward's conic (preprocess.hip preprocess_one): cov3D -> EWA cov2D -> + 0.3 -> inverse
    float cov[6];
    cov3d_from_scale_rot(sc, scale_modifier, q, cov);
    const Ewa e = ewa_setup(mean, focal_x, focal_y, cam[CAM_TANX], cam[CAM_TANY], vmat);
    float a, b, c;
    ewa_cov2d(e, cov, a, b, c);
    a += 0.3f; c += 0.3f;
    const float denom = a * c - b * b;
    const float det_inv = 1.f / denom;
    const float4 kc = make_float4(c * det_inv, -b * det_inv, a * det_inv, o);
    // pixel moments -> the reference's terms (backward.cu:536-554), once per Gaussian
    {
        const float m3 = part[3], m4 = part[4];
        part[3] = -o * (kc.x * m3 + kc.y * m4) * half_w;
        part[4] = -o * (kc.z * m4 + kc.y * m3) * half_h;
        part[5] = -0.5f * o * part[5];
        part[6] = -0.5f * o * part[6];
        part[7] = -0.5f * o * part[7];
    }
    float dmean[3], dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // ---- computeCov2DCUDA (backward.cu:144-274) ----
    {
        const float dLc0 = part[5], dLc1 = part[6], dLc3 = part[7];
        float dL_da = 0, dL_db = 0, dL_dc = 0;
        const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
#define T_(cc, rr) e.T[cc][rr]
        if (denom2inv != 0) {
            dL_da = denom2inv * (-c * c * dLc0 + 2 * b * c * dLc1 + (denom - a * c) * dLc3);
            dL_dc = denom2inv * (-a * a * dLc3 + 2 * a * b * dLc1 + (denom - a * c) * dLc0);
            dL_db = denom2inv * 2 * (b * c * dLc0 - (denom + 2 * b * b) * dLc1 + a * b * dLc3);
            dcov[0] = (T_(0, 0) * T_(0, 0) * dL_da + T_(0, 0) * T_(1, 0) * dL_db + T_(1, 0) * T_(1, 0) * dL_dc);
            dcov[3] = (T_(0, 1) * T_(0, 1) * dL_da + T_(0, 1) * T_(1, 1) * dL_db + T_(1, 1) * T_(1, 1) * dL_dc);
            dcov[5] = (T_(0, 2) * T_(0, 2) * dL_da + T_(0, 2) * T_(1, 2) * dL_db + T_(1, 2) * T_(1, 2) * dL_dc);
            dcov[1] = 2 * T_(0, 0) * T_(0, 1) * dL_da + (T_(0, 0) * T_(1, 1) + T_(0, 1) * T_(1, 0)) * dL_db + 2 * T_(1, 0) * T_(1, 1) * dL_dc;
            dcov[2] = 2 * T_(0, 0) * T_(0, 2) * dL_da + (T_(0, 0) * T_(1, 2) + T_(0, 2) * T_(1, 0)) * dL_db + 2 * T_(1, 0) * T_(1, 2) * dL_dc;
            dcov[4] = 2 * T_(0, 2) * T_(0, 1) * dL_da + (T_(0, 1) * T_(1, 2) + T_(0, 2) * T_(1, 1)) * dL_db + 2 * T_(1, 1) * T_(1, 2) * dL_dc;
        }
        const float V[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}};
#define TV_(rw, k) (T_(rw, 0) * V[k][0] + T_(rw, 1) * V[k][1] + T_(rw, 2) * V[k][2])
        const float dL_dT00 = 2 * TV_(0, 0) * dL_da + TV_(1, 0) * dL_db;
        const float dL_dT01 = 2 * TV_(0, 1) * dL_da + TV_(1, 1) * dL_db;
        const float dL_dT02 = 2 * TV_(0, 2) * dL_da + TV_(1, 2) * dL_db;
        const float dL_dT10 = 2 * TV_(1, 0) * dL_dc + TV_(0, 0) * dL_db;
        const float dL_dT11 = 2 * TV_(1, 1) * dL_dc + TV_(0, 1) * dL_db;
        const float dL_dT12 = 2 * TV_(1, 2) * dL_dc + TV_(0, 2) * dL_db;
#undef TV_
#undef T_
        const float* vmat2 = cam_at(cams, cam_off) + CAM_VIEW;
#define W_(k, rr) vmat2[4 * (rr) + (k)]
        const float dL_dJ00 = W_(0, 0) * dL_dT00 + W_(0, 1) * dL_dT01 + W_(0, 2) * dL_dT02;
        const float dL_dJ02 = W_(2, 0) * dL_dT00 + W_(2, 1) * dL_dT01 + W_(2, 2) * dL_dT02;
        const float dL_dJ11 = W_(1, 0) * dL_dT10 + W_(1, 1) * dL_dT11 + W_(1, 2) * dL_dT12;
        const float dL_dJ12 = W_(2, 0) * dL_dT10 + W_(2, 1) * dL_dT11 + W_(2, 2) * dL_dT12;
#undef W_
        const float h_x = focal_x, h_y = focal_y;
        const float tz = 1.f / e.t[2], tz2 = tz * tz, tz3 = tz2 * tz;
        const float dL_dtx = e.xmul * -h_x * tz2 * dL_dJ02;
        const float dL_dty = e.ymul * -h_y * tz2 * dL_dJ12;
        const float dL_dtz = -h_x * tz2 * dL_dJ00 - h_y * tz2 * dL_dJ11 + (2 * h_x * e.t[0]) * tz3 * dL_dJ02 + (2 * h_y * e.t[1]) * tz3 * dL_dJ12;
        const float* vm = cam_at(cams, cam_off) + CAM_VIEW;
        dmean[0] = vm[0] * dL_dtx + vm[1] * dL_dty + vm[2] * dL_dtz;
        dmean[1] = vm[4] * dL_dtx + vm[5] * dL_dty + vm[6] * dL_dtz;
        dmean[2] = vm[8] * dL_dtx + vm[9] * dL_dty + vm[10] * dL_dtz;
    }
    // ---- projection path (backward.cu:367-387) ----
    {
        const float* proj = cam_at(cams, cam_off) + CAM_PROJ;
        const float4 m_hom = xform44(mean, proj);
        const float m_w = 1.0f / (m_hom.w + 0.0000001f);
        const float mul1 = (proj[0] * mean.x + proj[4] * mean.y + proj[8] * mean.z + proj[12]) * m_w * m_w;
        const float mul2 = (proj[1] * mean.x + proj[5] * mean.y + proj[9] * mean.z + proj[13]) * m_w * m_w;
        const float g2x = part[3], g2y = part[4];
        dmean[0] += (proj[0] * m_w - proj[3] * mul1) * g2x + (proj[1] * m_w - proj[3] * mul2) * g2y;
        dmean[1] += (proj[4] * m_w - proj[7] * mul1) * g2x + (proj[5] * m_w - proj[7] * mul2) * g2y;
        dmean[2] += (proj[8] * m_w - proj[11] * mul1) * g2x + (proj[9] * m_w - proj[11] * mul2) * g2y;
    }
    // ---- view-direction term of the SH path (backward.cu:130-138; auxiliary.h:107-117 dnormvdv) ----
    {
        const float* cp = cam_at(cams, cam_off) + CAM_POS;
        const float dox = mean.x - cp[0], doy = mean.y - cp[1], doz = mean.z - cp[2];
        const float sum2 = dox * dox + doy * doy + doz * doz;
        const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
        dmean[0] += ((+sum2 - dox * dox) * dd0 - doy * dox * dd1 - doz * dox * dd2) * invsum32;
        dmean[1] += (-dox * doy * dd0 + (sum2 - doy * doy) * dd1 - doz * doy * dd2) * invsum32;
        dmean[2] += (-dox * doz * dd0 - doy * doz * dd1 + (sum2 - doz * doz) * dd2) * invsum32;
    }
    out[0] = dmean[0]; out[1] = dmean[1]; out[2] = dmean[2];
    out[10] = raw_opacity ? part[8] * ((1.0f - o) * o) : part[8];
    // ---- cov3D -> scale, quaternion (backward.cu:278-341) ----
    {
        const float r = q.x, qx = q.y, qy = q.z, qz = q.w;
        const Rot3 R = quat_to_rot(q);
        const float scale_mod2 = cam_at(cams, cam_off)[CAM_SCALE];
        const float s[3] = {scale_mod2 * sc.x, scale_mod2 * sc.y, scale_mod2 * sc.z};
        float Mm[3][3];
#pragma unroll
        for (int cc = 0; cc < 3; cc++)
#pragma unroll
            for (int rr = 0; rr < 3; rr++) Mm[cc][rr] = s[rr] * R.c[cc][rr];
        const float dS[3][3] = {{dcov[0], 0.5f * dcov[1], 0.5f * dcov[2]},
                                {0.5f * dcov[1], dcov[3], 0.5f * dcov[4]},
                                {0.5f * dcov[2], 0.5f * dcov[4], dcov[5]}};
        float dMt[3][3];
#pragma unroll
        for (int cc = 0; cc < 3; cc++)
#pragma unroll
            for (int rr = 0; rr < 3; rr++)
                dMt[rr][cc] = (Mm[0][rr] * 2.0f) * dS[cc][0] + (Mm[1][rr] * 2.0f) * dS[cc][1] + (Mm[2][rr] * 2.0f) * dS[cc][2];
        float ds[3], dq[4];
#pragma unroll
        for (int cc = 0; cc < 3; cc++) ds[cc] = R.c[0][cc] * dMt[cc][0] + R.c[1][cc] * dMt[cc][1] + R.c[2][cc] * dMt[cc][2];
#pragma unroll
        for (int cc = 0; cc < 3; cc++)
#pragma unroll
            for (int rr = 0; rr < 3; rr++) dMt[cc][rr] *= s[cc];
        dq[0] = 2 * qz * (dMt[0][1] - dMt[1][0]) + 2 * qy * (dMt[2][0] - dMt[0][2]) + 2 * qx * (dMt[1][2] - dMt[2][1]);
        dq[1] = 2 * qy * (dMt[1][0] + dMt[0][1]) + 2 * qz * (dMt[2][0] + dMt[0][2]) + 2 * r * (dMt[1][2] - dMt[2][1]) - 4 * qx * (dMt[2][2] + dMt[1][1]);
        dq[2] = 2 * qx * (dMt[1][0] + dMt[0][1]) + 2 * r * (dMt[2][0] - dMt[0][2]) + 2 * qz * (dMt[1][2] + dMt[2][1]) - 4 * qy * (dMt[2][2] + dMt[0][0]);
        dq[3] = 2 * r * (dMt[0][1] - dMt[1][0]) + 2 * qx * (dMt[2][0] + dMt[0][2]) + 2 * qy * (dMt[1][2] + dMt[2][1]) - 4 * qz * (dMt[1][1] + dMt[0][0]);
        if (raw_scale) { ds[0] *= sc.x; ds[1] *= sc.y; ds[2] *= sc.z; }          // d exp = exp
        if (raw_rot) {            // y = x / max(|x|, eps): dx = (g - y (y . g)) / max(|x|, eps)
            const float4 xr = q_raw;
            const float nrm = sqrtf(xr.x * xr.x + xr.y * xr.y + xr.z * xr.z + xr.w * xr.w);
            const float inv = 1.0f / fmaxf(nrm, 1e-12f);
            const float4 yn = make_float4(xr.x * inv, xr.y * inv, xr.z * inv, xr.w * inv);
            const float d = nrm > 1e-12f ? (yn.x * dq[0] + yn.y * dq[1] + yn.z * dq[2] + yn.w * dq[3]) : 0.0f;
            dq[0] = (dq[0] - yn.x * d) * inv; dq[1] = (dq[1] - yn.y * d) * inv;
            dq[2] = (dq[2] - yn.z * d) * inv; dq[3] = (dq[3] - yn.w * d) * inv;
        }
        out[3] = ds[0]; out[4] = ds[1]; out[5] = ds[2];
        out[6] = dq[0]; out[7] = dq[1]; out[8] = dq[2]; out[9] = dq[3];
    }
}

// The exchange's verdict for the host (pinned memory, polled): word 0 = any packet overflowed / does not describe this range,
// words 1 .. n_views = the rows each view wanted -- every one a 64-bit (sequence number << 32 | value) stored at once, so the
// host knows a word is this pass's by its tag and no fence is needed (a system-scope release here writes the L2's dirty
// lines back first: a one-thread kernel doing that took 60 - 160 us behind a backward).  Posted by the first wave of the
// combine pass's first workgroup as it starts: the host learns the verdict while the pass runs.
__device__ __forceinline__ void post_verdict(unsigned long long* __restrict__ status, uint32_t seq, const uint32_t* __restrict__ packets,
                                             size_t packet_stride_words, int n_views, int first, int n, int lane)
{
    const int v = lane;
    uint32_t bad = 0;
    if (v < n_views) {
        const uint32_t* h = packets + (size_t)v * packet_stride_words;
        const uint32_t want = h[1];
        bad = (want > h[3] || h[5] != FRG_SUM_MAGIC || h[2] != (uint32_t)n || h[4] != (uint32_t)first) ? 1u : 0u;
        __hip_atomic_store(&status[1 + v], ((unsigned long long)seq << 32) | want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const unsigned long long any = __builtin_amdgcn_ballot_w64(bad != 0u);
    if (v == 0) __hip_atomic_store(&status[0], ((unsigned long long)seq << 32) | (any ? 1ull : 0ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ONE launch: a workgroup of 256 threads takes a TILE of B blocks of 64 Gaussians.  B is chosen by the host from the number of
// views so that a tile holds a few hundred (Gaussian, view) PAIRS at C3's density (one Gaussian in eight has a row per view):
// B = 3 for eight views (192 +- 21 pairs: one balanced pass of the four waves), 24 for a single view.
//   set-up    the views' cameras, mask words and row offsets of the tile's blocks -> LDS; per Gaussian the views it has a row in
//             (one bit each) and an exclusive prefix of the pair counts over the tile: the pairs are ordered by (Gaussian, view);
//   pairs     in passes of at most 256, dealt evenly to as few of the four waves as hold them, ONE LANE PER PAIR: its packed
//             row (48 bytes), the Gaussian's parameters, the view's camera read from LDS by the lane; the per-Gaussian chain of
//             phase 2 (combine_one_view) and the sixteen SH basis weights of the view's direction -> 30 floats per pair in LDS;
//   sums      dense part: one thread per Gaussian adds the eleven terms of its pairs IN VIEW ORDER; SH part in the OUTPUT's
//             mapping: thread t < 252 owns float4 t % 12 of the SH rows of Gaussians t / 12 + 21 k = four consecutive
//             (coefficient, channel) products, and adds, for each pair of that Gaussian in view order, weight x dRGB read
//             from the staged pair (a wave covers 5.3 Gaussians: the view loop runs to THEIR longest list, ~2.5 steps, not
//             to the wave's eight; which operands a thread reads of a pair is fixed by t % 12 for the whole tile);
//   stores    every row once, in the pass that holds its Gaussian's last pair (the first pass for a Gaussian without pairs:
//             zeros -- or, row_live, nothing but the byte): the SH rows as contiguous non-temporal float4 streams straight from
//             the accumulators (no LDS transpose: the mapping is the output's), the dense rows by their Gaussian's thread.
//             Only a Gaussian whose pairs straddle two passes (at most one per pass boundary) leaves a partial sum in its
//             output row and reads it back in the next pass (the same threads; L2) -- so no accumulator lives across the pair
//             phase: 128 vector registers, four waves per SIMD.  No staging through HBM, no row -> Gaussian index pass.
// Forms of round 6 that were measured and replaced (eight C3 views, 3 M Gaussians, 3 M pairs): one lane per Gaussian walking
// its views with 59 accumulators -- 27 % busy lanes: 0.76 ms; tiles of 1024 / 512 Gaussians with the views in an outer loop and
// the sums in LDS -- a chain of barriers with one or two waves at work: 0.41 / 0.44 ms; four launches (row -> Gaussian index
// 0.037, one lane per packed row with the camera in scalar registers and the terms staged in HBM 0.146, ordered sum 0.089, SH
// rows with one lane per Gaussian and a wave-uniform view loop at one busy lane in eight 0.191): 0.476 ms.  This form: 0.256.
#define CT_PC 256
#define CT_STRIDE 31                  // 11 chain terms, 16 basis weights, 3 dRGB; odd: lane-consecutive pairs hit different banks
#define CT_SH_THREADS 252             // 21 Gaussians x 12 float4 of their SH rows per step of the SH sums
#define CT_W 11                       // first basis weight in a staged pair
#define CT_RGB 27                     // first dRGB component
// RAW: some parameter arrives in its raw form (the activations and their Jacobians cost 50 vector registers: the plain
// instantiation keeps four waves per SIMD)
template <int B, bool RAW>
__global__ void __launch_bounds__(256)
combine_tile_kernel(int first, int n, int n_views, const uint32_t* __restrict__ packets, size_t packet_stride_words, uint32_t capacity,
                    const float* __restrict__ means3D, const float* __restrict__ scales, const float* __restrict__ rotations,
                    const float* __restrict__ opacities, RawInputs raw_in, float* __restrict__ dL_dmean3D, float* __restrict__ dL_dscale,
                    float* __restrict__ dL_drot, float* __restrict__ dL_dopacity, float* __restrict__ dL_dsh,
                    unsigned char* __restrict__ row_live, unsigned long long* __restrict__ status, uint32_t seq)
{
    constexpr int G = 64 * B, GI = (G + 255) / 256;        // Gaussians of a tile; per thread
    static_assert(G <= 2048, "a pair is (Gaussian of the tile: 11 bits, view: 4 bits)");
    __shared__ float s_stage[CT_PC * CT_STRIDE];
    __shared__ float s_cam[CMB_MAX_VIEWS * CAM_STRIDE];
    __shared__ unsigned long long s_mask[CMB_MAX_VIEWS * B];
    __shared__ uint32_t s_base[CMB_MAX_VIEWS * B];
    __shared__ uint32_t s_start[G + 1];                    // exclusive prefix of the pair counts
    __shared__ uint16_t s_views[G];                        // the views a Gaussian has a row in
    __shared__ uint16_t s_pair[CT_PC];
    __shared__ uint32_t s_wtot[4];
    const RawInputs raw = RAW ? raw_in : RawInputs{};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = (int)sum_packet_blocks((size_t)n), blk0 = blockIdx.x * B, g0 = blk0 * 64;
    const size_t bases_w = sum_packet_bases_word((size_t)n), rows_w = sum_packet_rows_word((size_t)n);
    if (status && blockIdx.x == 0 && wave == 0) post_verdict(status, seq, packets, packet_stride_words, n_views, first, n, lane);
    // ---- set-up ----
    for (int v = wave; v < n_views; v += 4)
        if (lane < CAM_WORDS) s_cam[v * CAM_STRIDE + lane] = __uint_as_float(packets[(size_t)v * packet_stride_words + 8 + lane]);
    for (int i = tid; i < n_views * B; i += 256) {
        const int v = i / B, b = i - v * B, blk = blk0 + b;
        const uint32_t* pk = packets + (size_t)v * packet_stride_words;
        s_mask[i] = blk < nblk ? reinterpret_cast<const unsigned long long*>(pk + FRG_SUM_HDR_WORDS)[blk] : 0ull;
        s_base[i] = blk < nblk ? (pk + bases_w)[blk] : 0u;
    }
    __syncthreads();
    uint32_t T = 0;
#pragma unroll
    for (int it = 0; it < GI; it++) {
        const int g = it * 256 + tid;
        uint32_t views_of = 0;
        if (g < G && g0 + g < n)
            for (int v = 0; v < n_views; v++) views_of |= (uint32_t)((s_mask[v * B + (g >> 6)] >> lane) & 1ull) << v;
        const uint32_t cnt = (uint32_t)__popc(views_of), incl = wave_incl_scan_dpp(cnt);
        if (lane == 63) s_wtot[wave] = incl;
        __syncthreads();
        uint32_t before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) { const uint32_t t = s_wtot[w]; if (w < wave) before += t; tot += t; }
        if (g < G) { s_start[g] = T + before + incl - cnt; s_views[g] = (uint16_t)views_of; }
        T += tot;
        if (it + 1 < GI) __syncthreads();
    }
    if (tid == 0) s_start[G] = T;
    __syncthreads();

    typedef float nt_f4 __attribute__((ext_vector_type(4)));
    float4* const sh_dst = reinterpret_cast<float4*>(dL_dsh) + ((size_t)first + g0) * 12;
    const int gmax = min(G, n - g0);                       // Gaussians of this tile
    if (T == 0) {                                          // no view has a row in this tile: zeros (or, row_live, nothing but the bytes)
        if (!row_live)
            for (int f = tid; f < gmax * 12; f += 256) __builtin_nontemporal_store(nt_f4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<nt_f4*>(sh_dst + f));
        for (int g = tid; g < gmax; g += 256) {
            const size_t gi = (size_t)first + g0 + g;
            if (row_live) { row_live[gi] = 0; continue; }
            dL_dmean3D[3 * gi] = 0.f; dL_dmean3D[3 * gi + 1] = 0.f; dL_dmean3D[3 * gi + 2] = 0.f;
            dL_dscale[3 * gi] = 0.f; dL_dscale[3 * gi + 1] = 0.f; dL_dscale[3 * gi + 2] = 0.f;
            *reinterpret_cast<float4*>(dL_drot + 4 * gi) = make_float4(0.f, 0.f, 0.f, 0.f);
            dL_dopacity[gi] = 0.f;
        }
        return;
    }

#pragma unroll 1
    for (uint32_t p0 = 0; p0 < T; p0 += CT_PC) {
        const uint32_t npass = min(T - p0, (uint32_t)CT_PC), p1 = p0 + npass;
        const bool first_pass = p0 == 0;
        // ---- the pass's pairs, ordered by (Gaussian, view) ----
        for (int g = tid; g < gmax; g += 256) {
            const uint32_t s0 = s_start[g];
            uint32_t vs = s_views[g];
            if (!vs || s0 >= p1 || s_start[g + 1] <= p0) continue;
            uint32_t s = s0 - p0;                            // (unsigned: pairs before the pass compare as huge)
            while (vs) {
                const int v = __ffs((int)vs) - 1;
                vs &= vs - 1;
                if (s < (uint32_t)CT_PC) s_pair[s] = (uint16_t)(g | (v << 11));
                s++;
            }
        }
        __syncthreads();
        // ---- one lane per pair ----
        {
            const uint32_t nw = (npass + 63) >> 6, q = (npass + nw - 1) / nw, sl = wave * q + lane;     // the fewest waves, evenly filled
            if ((uint32_t)wave < nw && (uint32_t)lane < q && sl < npass) {
                const uint32_t info = s_pair[sl];
                const int gl = (int)(info & 2047u), v = (int)(info >> 11), b = gl >> 6, gln = gl & 63;
                const unsigned long long m = s_mask[v * B + b];
                const uint32_t row = s_base[v * B + b] + (uint32_t)__popcll(m & ((1ull << gln) - 1ull));
                float* st = s_stage + sl * CT_STRIDE;
                if (row < capacity) {
                    const uint32_t* pk = packets + (size_t)v * packet_stride_words;
                    const float4* r = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(pk) + rows_w + (size_t)row * FRG_SUM_ROW_FLOATS);
                    const float4 r0 = r[0], r1 = r[1], r2 = r[2];
                    const int idx = first + g0 + gl;
                    const float3 mean = param_mean(means3D, raw, idx);
                    const float3 sc = param_scale(scales, raw, idx);
                    const float4 qt = param_rot(rotations, raw, idx);
                    const float o = param_opacity(opacities, raw, idx);
                    float4 q_raw = qt;
                    if (RAW && raw.raw_rot) q_raw = make_float4(raw.raw_rot[4 * idx], raw.raw_rot[4 * idx + 1], raw.raw_rot[4 * idx + 2], raw.raw_rot[4 * idx + 3]);
                    const float* cam = cam_at(s_cam, v * CAM_STRIDE);
                    st[CT_RGB] = r0.x; st[CT_RGB + 1] = r0.y; st[CT_RGB + 2] = r0.z;
                    {   // the SH basis of the view's direction (forward.cu:20-71 in weight form; view_exchange.hip's expressions)
                        const int D = __float_as_int(cam[CAM_D]);
                        const float dox = mean.x - cam[CAM_POS], doy = mean.y - cam[CAM_POS + 1], doz = mean.z - cam[CAM_POS + 2];
                        const float len = sqrtf(dox * dox + doy * doy + doz * doz);
                        const float x = dox / len, y = doy / len, z = doz / len;
                        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                        float wgt[16];
#pragma unroll
                        for (int i = 0; i < 16; i++) wgt[i] = 0.0f;
                        wgt[0] = kSH0;
                        if (D > 0) { wgt[1] = -kSH1 * y; wgt[2] = kSH1 * z; wgt[3] = -kSH1 * x; }
                        if (D > 1) {
                            wgt[4] = kSH2[0] * xy; wgt[5] = kSH2[1] * yz; wgt[6] = kSH2[2] * (2.f * zz - xx - yy);
                            wgt[7] = kSH2[3] * xz; wgt[8] = kSH2[4] * (xx - yy);
                        }
                        if (D > 2) {
                            wgt[9] = kSH3[0] * y * (3.f * xx - yy); wgt[10] = kSH3[1] * xy * z;
                            wgt[11] = kSH3[2] * y * (4.f * zz - xx - yy); wgt[12] = kSH3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy);
                            wgt[13] = kSH3[4] * x * (4.f * zz - xx - yy); wgt[14] = kSH3[5] * z * (xx - yy);
                            wgt[15] = kSH3[6] * x * (xx - 3.f * yy);
                        }
#pragma unroll
                        for (int i = 0; i < 16; i++) st[CT_W + i] = wgt[i];
                    }
                    float part[FRG_SLOT_FLOATS] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x};
                    float out[CMB_ACC];
                    combine_one_view(s_cam, v * CAM_STRIDE, mean, sc, qt, o, RAW && raw.raw_opacity != nullptr, RAW && raw.raw_scale != nullptr,
                                     RAW && raw.raw_rot != nullptr, q_raw,
                                     part, r2.y, r2.z, r2.w, out);
#pragma unroll
                    for (int k = 0; k < CMB_ACC; k++) st[k] = out[k];
                } else {                                   // beyond the packet's capacity (the verdict says so): contributes nothing
#pragma unroll
                    for (int k = 0; k < CT_STRIDE - 1; k++) st[k] = 0.0f;
                }
            }
        }
        __syncthreads();
        // ---- ordered sums; a row leaves in the pass that holds its Gaussian's last pair ----
        for (int g = tid; g < gmax; g += 256) {
            const uint32_t s0 = s_start[g], s1 = s_start[g + 1];
            const size_t gi = (size_t)first + g0 + g;
            if (first_pass && row_live) row_live[gi] = s1 > s0 ? 1 : 0;
            const uint32_t lo = max(s0, p0), hi = min(s1, p1);
            if (s0 == s1 ? !(first_pass && !row_live) : lo >= hi) continue;
            float acc[CMB_ACC];
#pragma unroll
            for (int k = 0; k < CMB_ACC; k++) acc[k] = 0.0f;
            if (s0 < p0 && s0 != s1) {                     // pairs in an earlier pass: the partial sums are in the row
                acc[0] = dL_dmean3D[3 * gi]; acc[1] = dL_dmean3D[3 * gi + 1]; acc[2] = dL_dmean3D[3 * gi + 2];
                acc[3] = dL_dscale[3 * gi]; acc[4] = dL_dscale[3 * gi + 1]; acc[5] = dL_dscale[3 * gi + 2];
                const float4 rq = *reinterpret_cast<const float4*>(dL_drot + 4 * gi);
                acc[6] = rq.x; acc[7] = rq.y; acc[8] = rq.z; acc[9] = rq.w;
                acc[10] = dL_dopacity[gi];
            }
            for (uint32_t s = lo; s < hi; s++) {
                const float* st = s_stage + (s - p0) * CT_STRIDE;
#pragma unroll
                for (int k = 0; k < CMB_ACC; k++) acc[k] += st[k];
            }
            dL_dmean3D[3 * gi] = acc[0]; dL_dmean3D[3 * gi + 1] = acc[1]; dL_dmean3D[3 * gi + 2] = acc[2];
            dL_dscale[3 * gi] = acc[3]; dL_dscale[3 * gi + 1] = acc[4]; dL_dscale[3 * gi + 2] = acc[5];
            *reinterpret_cast<float4*>(dL_drot + 4 * gi) = make_float4(acc[6], acc[7], acc[8], acc[9]);
            dL_dopacity[gi] = acc[10];
        }
        if (tid < CT_SH_THREADS) {
            // thread t: float4 j = t % 12 of the rows of Gaussians t / 12 + 21 k -- elements i = 4 j + e (e < 4): coefficient i / 3,
            // channel i % 3; the staged pair's offsets of the four (weight, dRGB) operands are the thread's own for the whole tile
            int tc = tid;
            asm volatile("" : "+v"(tc));                   // (opaque: formed per pass, not held across the pair phase)
            const int tg = tc / 12, j = tc - 12 * tg, c0 = (4 * j) / 3, r = j - 3 * (j / 3);
            int wo[4], co[4];
#pragma unroll
            for (int e = 0; e < 4; e++) { const int t = r + e; wo[e] = CT_W + c0 + (t >= 3 ? 1 : 0); co[e] = CT_RGB + (t >= 3 ? t - 3 : t); }
#pragma unroll 1
            for (int gl = tg; gl < gmax; gl += CT_SH_THREADS / 12) {
                const uint32_t s0 = s_start[gl], s1 = s_start[gl + 1];
                const uint32_t lo = max(s0, p0), hi = min(s1, p1);
                if (s0 == s1 ? !(first_pass && !row_live) : lo >= hi) continue;      // not this pass's / nothing to write
                const int f = gl * 12 + j;
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                if (s0 < p0 && s0 != s1) acc = sh_dst[f];
                for (uint32_t s = lo; s < hi; s++) {
                    const float* st = s_stage + (s - p0) * CT_STRIDE;
                    acc.x += st[wo[0]] * st[co[0]];
                    acc.y += st[wo[1]] * st[co[1]];
                    acc.z += st[wo[2]] * st[co[2]];
                    acc.w += st[wo[3]] * st[co[3]];
                }
                if (s1 <= p1) __builtin_nontemporal_store(nt_f4{acc.x, acc.y, acc.z, acc.w}, reinterpret_cast<nt_f4*>(sh_dst + f));
                else sh_dst[f] = acc;
            }
        }
        if (p1 < T) __syncthreads();
    }
}

size_t combine_workspace_bytes(int n_views, size_t capacity)
{
    (void)n_views; (void)capacity;
    return 256;                 // the pass stages nothing in HBM any more; the argument stays in the ABI
}


template <bool RAW>
static void launch_tile(int B, int nblk, hipStream_t s, int first, int n, int n_views, const uint32_t* pk, size_t stride_w, uint32_t capacity,
                        const FwdInputs& in, const BwdOutputs& out, unsigned char* row_live, unsigned long long* status, uint32_t seq)
{
#define FRG_TILE_LAUNCH(BB) hipLaunchKernelGGL((combine_tile_kernel<BB, RAW>), dim3((nblk + BB - 1) / BB), dim3(256), 0, s, first, n, n_views, pk, stride_w, \
        capacity, in.means3D, in.scales, in.rotations, in.opacities, in.raw, out.dL_dmean3D, out.dL_dscale, out.dL_drot, out.dL_dopacity, out.dL_dsh,       \
        row_live, status, seq)
    if (B >= 24) FRG_TILE_LAUNCH(24); else if (B >= 12) FRG_TILE_LAUNCH(12); else if (B >= 6) FRG_TILE_LAUNCH(6); else if (B >= 3) FRG_TILE_LAUNCH(3); else FRG_TILE_LAUNCH(2);
#undef FRG_TILE_LAUNCH
}

hipError_t launch_backward_combine(int first, int n, int n_views, const void* packets, size_t packet_stride_bytes, uint32_t capacity,
                                   const FwdInputs& in, const BwdOutputs& out, unsigned long long* status, uint32_t seq, unsigned char* row_live,
                                   char* workspace, hipStream_t s)
{
    (void)workspace;
    const uint32_t* pk = reinterpret_cast<const uint32_t*>(packets);
    const size_t stride_w = packet_stride_bytes / 4;
    const int nblk = (int)sum_packet_blocks((size_t)n);
    // a tile of a few hundred pairs where one Gaussian in eight has a row per view (C3); any density is handled (more passes)
    const int asked = g_combine_blocks.load(std::memory_order_relaxed);
    const int B = asked > 0 ? asked : n_views >= 6 ? 3 : n_views >= 3 ? 6 : n_views == 2 ? 12 : 24;
    const bool raw = in.raw.raw_opacity || in.raw.raw_scale || in.raw.raw_rot;
    if (raw) launch_tile<true>(B, nblk, s, first, n, n_views, pk, stride_w, capacity, in, out, row_live, status, seq);
    else launch_tile<false>(B, nblk, s, first, n, n_views, pk, stride_w, capacity, in, out, row_live, status, seq);
    return hipGetLastError();
}

// ---- densification statistics of every view, from the packets ---------------------------------------------------------------
// What frg_densify_accumulate (densify.hip) adds for ONE view from that view's radii and dL_dmean2D, added here for EVERY view of
// the step, in view order, from the gathered packets: a packet with a visibility section says which Gaussians the view saw
// (denom += 1, max_radii2D = max(., radius)) and carries, for those with a row, the two pixel moments dL_dmean2D is formed from
// (combine_one_view's expressions: accum += |dL_dmean2D.xy|); conic, opacity and the radius are recomputed from the replicated
// parameters with the forward's own functions (preprocess.hip preprocess_one), bit-identically.  A visible Gaussian without a
// row has a zero viewspace gradient: it adds sqrtf(0), as the one-view kernel does.
// One wave per block of 64 Gaussians, one lane per Gaussian: a view's visibility word, mask word, row offset and camera are
// wave-uniform (scalar loads); the three statistics are read once and written once, by the lanes some view saw.
// EVERY wave first looks at all the views' headers (a few cache lines): one packet without the section, of another range or
// capacity, or overflowed -- and the whole launch writes nothing but the status word.
__global__ void __launch_bounds__(256)
densify_views_kernel(int first, int n, int n_views, const uint32_t* __restrict__ packets, size_t packet_stride_words, uint32_t capacity,
                     const float* __restrict__ means3D, const float* __restrict__ scales, const float* __restrict__ rotations,
                     const float* __restrict__ opacities, RawInputs raw, float* __restrict__ accum, float* __restrict__ denom,
                     float* __restrict__ max_radii2D, unsigned long long* __restrict__ status, uint32_t seq)
{
    const int lane = threadIdx.x & 63;
    const int blk = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int nblk = (int)sum_packet_blocks((size_t)n);
    const size_t bases_w = sum_packet_bases_word((size_t)n), rows_w = sum_packet_rows_word((size_t)n);
    const size_t vis_w = sum_packet_visible_word((size_t)n, (size_t)capacity);
    bool bad = false;
    if (lane < n_views) {
        const uint32_t* h = packets + (size_t)lane * packet_stride_words;
        bad = h[1] > h[3] || h[5] != FRG_SUM_MAGIC || h[2] != (uint32_t)n || h[4] != (uint32_t)first || h[3] != capacity || h[6] != (uint32_t)vis_w;
    }
    const bool refused = __builtin_amdgcn_ballot_w64(bad) != 0ull;
    if (status && blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(status, ((unsigned long long)seq << 32) | (refused ? 1ull : 0ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (refused || blk >= nblk) return;
    unsigned long long seen_any = 0ull;
    for (int v = 0; v < n_views; v++)
        seen_any |= reinterpret_cast<const unsigned long long*>(packets + (size_t)v * packet_stride_words + vis_w)[blk];
    const int gl = blk * 64 + lane;
    if (!((seen_any >> lane) & 1ull) || gl >= n) return;
    const int idx = first + gl;
    const float3 mean = param_mean(means3D, raw, idx);
    const float3 sc = param_scale(scales, raw, idx);
    const float4 q = param_rot(rotations, raw, idx);
    const float o = param_opacity(opacities, raw, idx);
    float acc = accum[idx], den = denom[idx], rad = max_radii2D[idx];
    for (int v = 0; v < n_views; v++) {
        const uint32_t* pk = packets + (size_t)v * packet_stride_words;
        const unsigned long long seen = reinterpret_cast<const unsigned long long*>(pk + vis_w)[blk];
        if (!((seen >> lane) & 1ull)) continue;
        const float* cam = reinterpret_cast<const float*>(pk) + 8;
        // the forward's covariance, radius and conic (preprocess.hip preprocess_one; combine_one_view above)
        float cov[6];
        cov3d_from_scale_rot(sc, cam[CAM_SCALE], q, cov);
        const Ewa e = ewa_setup(mean, cam[CAM_FX], cam[CAM_FY], cam[CAM_TANX], cam[CAM_TANY], cam + CAM_VIEW);
        float a, b, c;
        ewa_cov2d(e, cov, a, b, c);
        a += 0.3f; c += 0.3f;
        const float det = a * c - b * b;
        const float mid = 0.5f * (a + c);
        const float lambda1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
        const float lambda2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
        const float my_radius = ceilf(3.f * sqrtf(fmaxf(lambda1, lambda2)));
        rad = fmaxf(rad, (float)f2i(my_radius));
        den = den + 1.0f;
        float gx = 0.0f, gy = 0.0f;
        const unsigned long long m = reinterpret_cast<const unsigned long long*>(pk + FRG_SUM_HDR_WORDS)[blk];
        if ((m >> lane) & 1ull) {
            const uint32_t row = (pk + bases_w)[blk] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (row < capacity) {
                const float* r = reinterpret_cast<const float*>(pk) + rows_w + (size_t)row * FRG_SUM_ROW_FLOATS;
                const float m3 = r[3], m4 = r[4];
                const float half_w = 0.5f * (float)__float_as_int(cam[CAM_W]), half_h = 0.5f * (float)__float_as_int(cam[CAM_H]);
                const float det_inv = 1.f / det;
                const float4 kc = make_float4(c * det_inv, -b * det_inv, a * det_inv, o);
                gx = -o * (kc.x * m3 + kc.y * m4) * half_w;
                gy = -o * (kc.z * m4 + kc.y * m3) * half_h;
            }
        }
        acc = acc + sqrtf(gx * gx + gy * gy);
    }
    accum[idx] = acc; denom[idx] = den; max_radii2D[idx] = rad;
}

hipError_t launch_densify_views(int first, int n, int n_views, const void* packets, size_t packet_stride_bytes, uint32_t capacity,
                                const FwdInputs& in, float* accum, float* denom, float* max_radii2D, unsigned long long* status, uint32_t seq,
                                hipStream_t s)
{
    const int nblk = (int)sum_packet_blocks((size_t)n);
    hipLaunchKernelGGL(densify_views_kernel, dim3((nblk + 3) / 4), dim3(256), 0, s, first, n, n_views, reinterpret_cast<const uint32_t*>(packets),
                       packet_stride_bytes / 4, capacity, in.means3D, in.scales, in.rotations, in.opacities, in.raw, accum, denom, max_radii2D, status, seq);
    return hipGetLastError();
}

}  // namespace frg
