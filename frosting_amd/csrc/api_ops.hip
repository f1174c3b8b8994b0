// C ABI of libfrosting_rasterizer.so, everything beside the rasterizer (api.hip): the two gradient-exchange plans' pack,
// scatter and combine calls, the fused Adam step, the photometric loss, the parameter activations, kNN, the shell
// parameterisation and adaptive density control.  Each entry point validates its arguments and enqueues its kernels on
// the caller's HIP stream; none keeps state between calls (the two that take a forward's buffers ask api.hip's notes whether
// that forward rotated its SH directions, and refuse).
#include "host_common.h"

#include <cmath>

using frg::fail;

extern "C" {

int frg_sh_color_grad(int P, const char* geom_buffer, const int* radii, const float* dL_dcolors,
                      float* out_drgb, void* hip_stream)
{
    if (P < 0) return fail(FRG_EINVAL, "P < 0");
    if (P == 0) return FRG_OK;
    if (!geom_buffer || !radii || !dL_dcolors || !out_drgb) return fail(FRG_EINVAL, "null pointer");
    if (frg::forward_was_rotated(geom_buffer)) return fail(FRG_EINVAL, "frg_sh_color_grad: %s", frg::kRotatedSingleView);
    const frg::GeomState g = frg::GeomState::carve(const_cast<char*>(geom_buffer), P);
    FRG_HIP(frg::launch_sh_color_grad(P, g, radii, dL_dcolors, out_drgb, (hipStream_t)hip_stream));
    return FRG_OK;
}

int frg_sh_grad_from_views(int P, int D, int M, int n_views, const float* means3D,
                           const float* campos, long long campos_stride,
                           const float* drgb, long long view_stride, float* dL_dsh, void* hip_stream)
{
    if (P < 0 || n_views < 0 || D < 0 || D > 3) return fail(FRG_EINVAL, "bad sizes P=%d views=%d D=%d", P, n_views, D);
    if (M < (D + 1) * (D + 1)) return fail(FRG_EINVAL, "degree %d needs %d coefficients, got M=%d", D, (D + 1) * (D + 1), M);
    if (P == 0) return FRG_OK;
    if (!means3D || !dL_dsh || (n_views > 0 && (!campos || !drgb))) return fail(FRG_EINVAL, "null pointer");
    FRG_HIP(frg::launch_sh_grad_from_views(P, D, M, n_views, means3D, campos, campos_stride, drgb, view_stride, dL_dsh,
                                           (hipStream_t)hip_stream));
    return FRG_OK;
}

int frg_pack_grad_rows(int P, const float* dL_dmeans3D, const float* dL_dscales, const float* dL_drotations, const float* dL_dopacity,
                       const float* drgb, float* rows, long long capacity_rows, unsigned int* count, void* hip_stream)
{
    if (P < 0 || capacity_rows < 0 || capacity_rows > 0xffffffffLL) return fail(FRG_EINVAL, "bad sizes P=%d capacity=%lld", P, capacity_rows);
    if (!count) return fail(FRG_EINVAL, "null pointer");
    if (P == 0) { FRG_HIP(hipMemsetAsync(count, 0, sizeof(unsigned int), (hipStream_t)hip_stream)); return FRG_OK; }
    if (!dL_dmeans3D || !dL_dscales || !dL_drotations || !dL_dopacity || !drgb || (!rows && capacity_rows > 0)) return fail(FRG_EINVAL, "null pointer");
    if (reinterpret_cast<uintptr_t>(rows) % 16 != 0) return fail(FRG_EINVAL, "rows must be 16-byte aligned");
    FRG_HIP(frg::launch_pack_grad_rows(P, dL_dmeans3D, dL_dscales, dL_drotations, dL_dopacity, drgb, rows, (unsigned int)capacity_rows, count,
                                       (hipStream_t)hip_stream));
    return FRG_OK;
}

int frg_scatter_grad_rows(long long n_rows, int P, const float* rows, float* dL_dmeans3D, float* dL_dscales, float* dL_drotations,
                          float* dL_dopacity, float* drgb_dense, void* hip_stream)
{
    if (P < 0 || n_rows < 0 || n_rows > 0xffffffffLL) return fail(FRG_EINVAL, "bad sizes P=%d rows=%lld", P, n_rows);
    if (n_rows == 0 || P == 0) return FRG_OK;
    if (!rows || !dL_dmeans3D || !dL_dscales || !dL_drotations || !dL_dopacity) return fail(FRG_EINVAL, "null pointer");
    if (reinterpret_cast<uintptr_t>(rows) % 16 != 0) return fail(FRG_EINVAL, "rows must be 16-byte aligned");
    FRG_HIP(frg::launch_scatter_grad_rows((unsigned int)n_rows, P, rows, dL_dmeans3D, dL_dscales, dL_drotations, dL_dopacity, drgb_dense,
                                          (hipStream_t)hip_stream));
    return FRG_OK;
}

size_t frg_sum_packet_bytes(int n_gaussians, long long capacity_rows)
{
    if (n_gaussians < 0 || capacity_rows < 0) return 0;
    return frg::sum_packet_bytes((size_t)n_gaussians, (size_t)capacity_rows);
}

size_t frg_sum_packet_bytes_ex(int n_gaussians, long long capacity_rows, int with_visibility)
{
    if (n_gaussians < 0 || capacity_rows < 0) return 0;
    return with_visibility ? frg::sum_packet_bytes_visible((size_t)n_gaussians, (size_t)capacity_rows)
                           : frg::sum_packet_bytes((size_t)n_gaussians, (size_t)capacity_rows);
}

int frg_pack_sum_rows_ex(const frg_pack_sum_args* a)
{
    if (!a || a->struct_size != sizeof(frg_pack_sum_args))
        return fail(FRG_EINVAL, "frg_pack_sum_args: struct_size %zu, this library expects %zu", a ? a->struct_size : (size_t)0, sizeof(frg_pack_sum_args));
    if (a->P < 0 || a->R < 0 || a->first < 0 || a->count < 0 || (long long)a->first + a->count > a->P || a->first % 64 != 0)
        return fail(FRG_EINVAL, "bad range: P=%d first=%d (a multiple of 64) count=%d", a->P, a->first, a->count);
    if (a->capacity_rows < 0 || a->capacity_rows > 0x7fffffffLL) return fail(FRG_EINVAL, "capacity_rows %lld", a->capacity_rows);
    if (!a->workspace || a->workspace_bytes < frg_backward_workspace_bytes(a->P, a->R)) return fail(FRG_EALLOC, "not the workspace of a backward with P=%d R=%d", a->P, a->R);
    if (frg::phase1_was_rotated(a->workspace)) return fail(FRG_EINVAL, "frg_pack_sum_rows: %s", frg::kRotatedSingleView);
    const size_t need = frg_sum_packet_bytes_ex(a->count, a->capacity_rows, a->radii != nullptr);
    if (!a->packet || a->packet_bytes < need || reinterpret_cast<uintptr_t>(a->packet) % 16 != 0)
        return fail(FRG_EALLOC, "packet: need %zu bytes, 16-byte aligned", need);
    if (!a->drgb_masked || !a->viewmatrix || !a->projmatrix || !a->campos) return fail(FRG_EINVAL, "null pointer");
    if (a->width <= 0 || a->height <= 0 || a->D < 0 || a->D > 3) return fail(FRG_EINVAL, "bad view: %dx%d degree %d", a->width, a->height, a->D);
    const frg::BwdWorkspace ws = frg::BwdWorkspace::carve(a->workspace, a->P, a->R);      // what phase 1 of that backward left
    const frg::SumCamera cam{a->tan_fovx, a->tan_fovy, a->scale_modifier, a->width, a->height, a->D};
    FRG_HIP(frg::launch_pack_sum_rows(a->first, a->count, (uint32_t)a->capacity_rows, ws.live_masks, ws.sums, ws.dir_terms, a->drgb_masked, cam, a->viewmatrix,
                                      a->projmatrix, a->campos, a->packet, ws.group_tot, (hipStream_t)a->hip_stream, a->radii));
    return FRG_OK;
}

int frg_pack_sum_rows(int P, int R, int first, int count, char* workspace, size_t workspace_bytes, const float* drgb_masked,
                      const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                      int width, int height, float scale_modifier, int D, void* packet, size_t packet_bytes, long long capacity_rows,
                      void* hip_stream)
{
    frg_pack_sum_args a{};
    a.struct_size = sizeof(a);
    a.P = P; a.R = R; a.first = first; a.count = count;
    a.workspace = workspace; a.workspace_bytes = workspace_bytes;
    a.drgb_masked = drgb_masked; a.viewmatrix = viewmatrix; a.projmatrix = projmatrix; a.campos = campos;
    a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy; a.width = width; a.height = height; a.scale_modifier = scale_modifier; a.D = D;
    a.packet = packet; a.packet_bytes = packet_bytes; a.capacity_rows = capacity_rows;
    a.radii = nullptr; a.hip_stream = hip_stream;
    return frg_pack_sum_rows_ex(&a);
}

size_t frg_combine_workspace_bytes(int n_views, long long capacity_rows)
{
    if (n_views < 0 || capacity_rows < 0) return 0;
    return frg::combine_workspace_bytes(n_views, (size_t)capacity_rows);
}

int frg_backward_combine(const frg_combine_args* a)
{
    if (!a || a->struct_size != sizeof(frg_combine_args))
        return fail(FRG_EINVAL, "frg_combine_args: struct_size %zu, this library expects %zu", a ? a->struct_size : (size_t)0, sizeof(frg_combine_args));
    if (a->P < 0 || a->first < 0 || a->count < 0 || (long long)a->first + a->count > a->P || a->first % 64 != 0)
        return fail(FRG_EINVAL, "bad range: P=%d first=%d (a multiple of 64) count=%d", a->P, a->first, a->count);
    if (a->n_views < 1 || a->n_views > 16) return fail(FRG_EINVAL, "1..16 views expected, got %d", a->n_views);
    if (a->M != 16) return fail(FRG_EINVAL, "the combine pass takes SH rows of 16 coefficients (M = %d)", a->M);
    if (a->capacity_rows >= 65535LL * 256) return fail(FRG_EINVAL, "capacity_rows %lld: a packet holds fewer than 2^24 rows (cut the Gaussians into more ranges)", a->capacity_rows);
    if (a->count == 0) return FRG_OK;
    if (!a->packets || a->packet_stride_bytes % 16 != 0 || a->packet_stride_bytes < frg_sum_packet_bytes(a->count, a->capacity_rows))
        return fail(FRG_EINVAL, "packets: stride %zu, a packet of %d Gaussians and %lld rows has %zu bytes", a->packet_stride_bytes, a->count,
                    a->capacity_rows, frg_sum_packet_bytes(a->count, a->capacity_rows));
    if ((a->means3D == nullptr) || !a->shs) return fail(FRG_EINVAL, "means3D and shs are required (shell-bound centres are not offered here)");
    if (!a->workspace || a->workspace_bytes < frg_combine_workspace_bytes(a->n_views, a->capacity_rows) || reinterpret_cast<uintptr_t>(a->workspace) % 16 != 0)
        return fail(FRG_EALLOC, "workspace: need %zu bytes, 16-byte aligned", frg_combine_workspace_bytes(a->n_views, a->capacity_rows));
    if ((a->opacities == nullptr) == (a->raw_opacities == nullptr)) return fail(FRG_EINVAL, "provide exactly one of opacities / raw_opacities");
    const bool raw_sr = a->raw_scales && a->raw_rotations;
    if (raw_sr == (a->scales && a->rotations) || (a->raw_scales == nullptr) != (a->raw_rotations == nullptr) || (a->scales == nullptr) != (a->rotations == nullptr))
        return fail(FRG_EINVAL, "provide (scales, rotations) or (raw_scales, raw_rotations)");
    if (!a->dL_dmean3D || !a->dL_dscale || !a->dL_drot || !a->dL_dopacity || !a->dL_dsh) return fail(FRG_EINVAL, "null gradient output");
    if ((reinterpret_cast<uintptr_t>(a->shs) | reinterpret_cast<uintptr_t>(a->dL_dsh) | reinterpret_cast<uintptr_t>(a->dL_drot) |
         reinterpret_cast<uintptr_t>(a->rotations) | reinterpret_cast<uintptr_t>(a->packets)) % 16 != 0)
        return fail(FRG_EINVAL, "shs, rotations, dL_dsh, dL_drot and the packets must be 16-byte aligned");
    frg::FwdInputs in{a->means3D, a->scales, a->rotations, a->opacities, a->shs, nullptr, nullptr, nullptr, nullptr, nullptr};
    in.raw.raw_opacity = a->raw_opacities; in.raw.raw_scale = a->raw_scales; in.raw.raw_rot = a->raw_rotations;
    frg::BwdOutputs out{nullptr, nullptr, a->dL_dopacity, nullptr, a->dL_dmean3D, nullptr, a->dL_dsh, a->dL_dscale, a->dL_drot};
    FRG_HIP(frg::launch_backward_combine(a->first, a->count, a->n_views, a->packets, a->packet_stride_bytes, (uint32_t)a->capacity_rows, in, out,
                                         a->status, a->status_seq, a->row_live, a->workspace, (hipStream_t)a->hip_stream));
    return FRG_OK;
}

}  // extern "C"

namespace {

// One Adam step as its three entry points state it: the arrays (pointing at the first of n elements), the segment
// tables, the hyper-parameters, and what only some of them offer.
struct AdamCall {
    long long n;
    float* params; const float* grads; float* exp_avg; float* exp_avg_sq;
    const long long* segment_ends; const float* segment_lrs; const int* segment_period; const int* segment_head; const float* segment_head_lrs;
    int n_segments;
    double beta1, beta2, eps;
    int step;
    float grad_scale;
    void* hip_stream;
    const frg::AdamRows* rows = nullptr;      // frg_adam_step_rows: the gradient rows of unmarked Gaussians are zero and not read
    bool shifted_ends = false;                // frg_adam_step_shard: segment ends before the first element (negative) are expected
};

int adam_step_impl(const AdamCall& c)
{
    const long long n = c.n;
    const int n_segments = c.n_segments;
    if (n < 0 || c.step < 1) return fail(FRG_EINVAL, "bad sizes n=%lld step=%d", n, c.step);
    if (n_segments < 1 || n_segments > FRG_ADAM_MAX_SEGMENTS || !c.segment_ends || !c.segment_lrs)
        return fail(FRG_EINVAL, "1..%d segments expected, got %d", FRG_ADAM_MAX_SEGMENTS, n_segments);
    for (int k = 1; k < n_segments; k++)
        if (c.segment_ends[k] < c.segment_ends[k - 1]) return fail(FRG_EINVAL, "segment ends must not decrease");
    if ((c.segment_ends[0] < 0 && !c.shifted_ends) || c.segment_ends[n_segments - 1] != n) return fail(FRG_EINVAL, "the last segment must end at n");
    if (n == 0) return FRG_OK;
    if (!c.params || !c.grads || !c.exp_avg || !c.exp_avg_sq) return fail(FRG_EINVAL, "null pointer");
    if ((reinterpret_cast<uintptr_t>(c.params) | reinterpret_cast<uintptr_t>(c.grads) | reinterpret_cast<uintptr_t>(c.exp_avg) |
         reinterpret_cast<uintptr_t>(c.exp_avg_sq)) % 16 != 0)
        return fail(FRG_EINVAL, "the four arrays must be 16-byte aligned");
    if ((n + 3) / 4 / 256 + 1 > 0x7fffffffLL) return fail(FRG_EINVAL, "n too large for one launch");
    // Python-float arithmetic of torch/optim/adam.py: doubles, rounded to float where a tensor op takes them
    const double bc1 = 1.0 - std::pow(c.beta1, (double)c.step);
    const double bc2 = 1.0 - std::pow(c.beta2, (double)c.step);
    frg::AdamSegments seg;
    seg.count = n_segments;
    for (int k = 0; k < FRG_ADAM_MAX_SEGMENTS; k++) {
        seg.end[k] = k < n_segments ? c.segment_ends[k] : n;
        seg.step_size[k] = k < n_segments ? (float)((double)c.segment_lrs[k] / bc1) : 0.0f;
        const bool sub = k < n_segments && c.segment_period && c.segment_head && c.segment_head_lrs && c.segment_period[k] > 0;
        if (sub && (c.segment_head[k] < 0 || c.segment_head[k] > c.segment_period[k]))
            return fail(FRG_EINVAL, "segment %d: head %d outside its period %d", k, c.segment_head[k], c.segment_period[k]);
        seg.period[k] = sub ? c.segment_period[k] : 0;
        seg.head[k] = sub ? c.segment_head[k] : 0;
        seg.head_step_size[k] = sub ? (float)((double)c.segment_head_lrs[k] / bc1) : 0.0f;
    }
    const float w1 = (float)(1.0 - c.beta1);      // betas arrive as doubles: 1 - beta is formed before rounding to float,
    const float omb2 = (float)(1.0 - c.beta2);    // as the Python floats of torch/optim/adam.py are
    const float inv_bc2_sqrt = 1.0f / (float)std::sqrt(bc2);   // ATen divides by a scalar as a multiplication by its float reciprocal
    FRG_HIP(frg::launch_adam_step(n, c.params, c.grads, c.exp_avg, c.exp_avg_sq, seg, w1, (float)c.beta2, omb2, inv_bc2_sqrt, (float)c.eps, c.grad_scale,
                                  (hipStream_t)c.hip_stream, c.rows));
    return FRG_OK;
}

}  // namespace

extern "C" {

int frg_adam_step(long long n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                  const long long* segment_ends, const float* segment_lrs, const int* segment_period,
                  const int* segment_head, const float* segment_head_lrs, int n_segments,
                  double beta1, double beta2, double eps, int step, float grad_scale, void* hip_stream)
{
    return adam_step_impl(AdamCall{n, params, grads, exp_avg, exp_avg_sq, segment_ends, segment_lrs, segment_period, segment_head, segment_head_lrs,
                                   n_segments, beta1, beta2, eps, step, grad_scale, hip_stream});
}

int frg_adam_step_shard(long long n, long long first, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                        const long long* segment_ends, const float* segment_lrs, const int* segment_period,
                        const int* segment_head, const float* segment_head_lrs, int n_segments,
                        double beta1, double beta2, double eps, int step, float grad_scale, void* hip_stream)
{
    // elements [first, first + n) of the flat layout, the four arrays pointing at element `first`: the segment table is
    // shifted by `first` behind a zero-length segment that ends at -first -- the kernel takes an element's segment as the last
    // one whose predecessor ends at or before it and its offset from that end, so negative ends give every element of the
    // shard its true segment and its true phase inside it (the DC / rest split of the SH rows)
    if (n < 0 || first < 0 || first % 4 != 0) return fail(FRG_EINVAL, "bad shard: n=%lld first=%lld (a multiple of 4 elements)", n, first);
    if (n_segments < 1 || n_segments + 1 > FRG_ADAM_MAX_SEGMENTS || !segment_ends || !segment_lrs)
        return fail(FRG_EINVAL, "a sharded step takes 1..%d segments, got %d", FRG_ADAM_MAX_SEGMENTS - 1, n_segments);
    if (first + n > segment_ends[n_segments - 1]) return fail(FRG_EINVAL, "the shard ends behind the last segment");
    long long ends[FRG_ADAM_MAX_SEGMENTS];
    float lrs[FRG_ADAM_MAX_SEGMENTS], hlrs[FRG_ADAM_MAX_SEGMENTS];
    int per[FRG_ADAM_MAX_SEGMENTS], head[FRG_ADAM_MAX_SEGMENTS];
    ends[0] = -first; lrs[0] = 0.0f; hlrs[0] = 0.0f; per[0] = 0; head[0] = 0;
    for (int k = 0; k < n_segments; k++) {
        ends[k + 1] = segment_ends[k] - first;
        lrs[k + 1] = segment_lrs[k];
        per[k + 1] = segment_period ? segment_period[k] : 0;
        head[k + 1] = segment_head ? segment_head[k] : 0;
        hlrs[k + 1] = segment_head_lrs ? segment_head_lrs[k] : 0.0f;
    }
    ends[n_segments] = n;       // the shard ends inside (or at the end of) the last segment it reaches; later ones are cut off
    for (int k = 1; k <= n_segments; k++) if (ends[k] > n) ends[k] = n;
    AdamCall c{n, params, grads, exp_avg, exp_avg_sq, ends, lrs, per, head, hlrs, n_segments + 1, beta1, beta2, eps, step, grad_scale, hip_stream};
    c.shifted_ends = true;
    return adam_step_impl(c);
}

int frg_adam_step_rows(long long n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                       const long long* segment_ends, const float* segment_lrs, const int* segment_period,
                       const int* segment_head, const float* segment_head_lrs, int n_segments,
                       double beta1, double beta2, double eps, int step, float grad_scale,
                       const unsigned char* row_live, int P, const int* segment_width, void* hip_stream)
{
    AdamCall c{n, params, grads, exp_avg, exp_avg_sq, segment_ends, segment_lrs, segment_period, segment_head, segment_head_lrs,
               n_segments, beta1, beta2, eps, step, grad_scale, hip_stream};
    if (!row_live) return adam_step_impl(c);
    if (P < 0 || !segment_width) return fail(FRG_EINVAL, "row_live needs P >= 0 and segment_width");
    if (n_segments < 1 || n_segments > FRG_ADAM_MAX_SEGMENTS) return fail(FRG_EINVAL, "1..%d segments expected, got %d", FRG_ADAM_MAX_SEGMENTS, n_segments);
    for (int k = 0; k < n_segments; k++) {
        const long long begin = k ? segment_ends[k - 1] : 0;
        if (segment_width[k] < 0 || (long long)segment_width[k] * P > segment_ends[k] - begin)
            return fail(FRG_EINVAL, "segment %d: %d elements per Gaussian x %d Gaussians exceed its %lld elements", k, segment_width[k], P, segment_ends[k] - begin);
        if (segment_width[k] > 0 && segment_ends[k] - begin > 0xffffffffLL)
            return fail(FRG_EINVAL, "segment %d: a per-Gaussian segment of a masked step holds at most 2^32 elements", k);
        // the kernel takes four consecutive elements per thread and lets ONE mask look-up stand for all four when the rows of
        // their segment are a multiple of four elements long: true only if the segment starts on a multiple of four elements
        if (segment_width[k] > 0 && segment_width[k] % 4 == 0 && begin % 4 != 0)
            return fail(FRG_EINVAL, "segment %d: rows of %d elements must begin on a multiple of 4 elements (begins at %lld)", k, segment_width[k], begin);
    }
    frg::AdamRows rows;
    rows.live = row_live; rows.P = P;
    for (int k = 0; k < FRG_ADAM_MAX_SEGMENTS; k++) {
        rows.width[k] = k < n_segments ? segment_width[k] : 0;
        rows.magic[k] = rows.width[k] > 1 ? (unsigned int)(0x100000000ull / (unsigned long long)rows.width[k]) : 0u;
    }
    c.rows = &rows;
    return adam_step_impl(c);
}

size_t frg_photometric_workspace_bytes(int channels, int width, int height)
{
    if (channels <= 0 || width <= 0 || height <= 0) return 0;
    return frg::photometric_workspace_bytes(channels, width, height);
}

int frg_photometric_loss(int channels, int width, int height, const float* image, const float* target,
                         const float* window11, float lambda_dssim, float* loss, float* dL_dimage,
                         char* workspace, size_t workspace_bytes, void* hip_stream)
{
    if (channels <= 0 || width <= 0 || height <= 0) return fail(FRG_EINVAL, "bad sizes C=%d W=%d H=%d", channels, width, height);
    if (!image || !target || !window11 || !loss) return fail(FRG_EINVAL, "null pointer");
    if (!workspace || workspace_bytes < frg_photometric_workspace_bytes(channels, width, height))
        return fail(FRG_EALLOC, "workspace too small: need %zu bytes", frg_photometric_workspace_bytes(channels, width, height));
    if ((long long)channels * ((width + 15) / 16) * ((height + 15) / 16) > 0x7fffffffLL) return fail(FRG_EINVAL, "image too large");
    FRG_HIP(frg::launch_photometric(channels, width, height, image, target, window11, lambda_dssim, loss, dL_dimage, workspace,
                                    (hipStream_t)hip_stream));
    return FRG_OK;
}

int frg_activate(int P, const float* raw_opacity, const float* raw_scale, const float* raw_rot,
                 float* opacity, float* scale, float* rot, void* hip_stream)
{
    if (P < 0) return fail(FRG_EINVAL, "P < 0");
    if (P == 0) return FRG_OK;
    if (!raw_opacity || !raw_scale || !raw_rot || !opacity || !scale || !rot) return fail(FRG_EINVAL, "null pointer");
    FRG_HIP(frg::launch_activate(P, raw_opacity, raw_scale, raw_rot, opacity, scale, rot, (hipStream_t)hip_stream));
    return FRG_OK;
}

int frg_activate_backward(int P, const float* opacity, const float* scale, const float* raw_rot,
                          float* g_opacity, float* g_scale, float* g_rot, void* hip_stream)
{
    if (P < 0) return fail(FRG_EINVAL, "P < 0");
    if (P == 0) return FRG_OK;
    if (!opacity || !scale || !raw_rot || !g_opacity || !g_scale || !g_rot) return fail(FRG_EINVAL, "null pointer");
    FRG_HIP(frg::launch_activate_bwd(P, opacity, scale, raw_rot, g_opacity, g_scale, g_rot, (hipStream_t)hip_stream));
    return FRG_OK;
}

size_t frg_knn_workspace_bytes(int P) { return P > 0 ? frg::knn_workspace_bytes(P) : 0; }

int frg_knn_mean_dist2(int P, const float* points, float* mean_dist2, char* workspace, size_t workspace_bytes, void* hip_stream)
{
    if (P < 0) return fail(FRG_EINVAL, "P < 0");
    if (P == 0) return FRG_OK;
    if (!points || !mean_dist2) return fail(FRG_EINVAL, "null pointer");
    if (!workspace || workspace_bytes < frg_knn_workspace_bytes(P))
        return fail(FRG_EALLOC, "workspace too small: need %zu bytes", frg_knn_workspace_bytes(P));
    if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return fail(FRG_EINVAL, "workspace must be 256-byte aligned");
    FRG_HIP(frg::launch_knn(P, points, mean_dist2, workspace, (hipStream_t)hip_stream));
    return FRG_OK;
}

size_t frg_knn_points_workspace_bytes(int P1, int P2, int K)
{
    return P2 > 0 && P1 >= 0 ? frg::knn_points_workspace_bytes(P1, P2, K) : 0;
}

int frg_knn_points(int P1, const float* p1, int P2, const float* p2, int K, float* dists, long long* idx, char* workspace,
                   size_t workspace_bytes, void* hip_stream)
{
    if (P1 < 0 || P2 < 0) return fail(FRG_EINVAL, "P1 = %d or P2 = %d < 0", P1, P2);
    if (K < 1 || K > FRG_KNN_MAX_K) return fail(FRG_EINVAL, "K = %d outside 1 ... %d", K, FRG_KNN_MAX_K);
    if (P1 == 0) return FRG_OK;
    if (!p1 || !dists || !idx) return fail(FRG_EINVAL, "null pointer");
    if (P2 == 0) {                                       // nothing to find: every slot is padding
        FRG_HIP(hipMemsetAsync(dists, 0, (size_t)P1 * K * sizeof(float), (hipStream_t)hip_stream));
        FRG_HIP(hipMemsetAsync(idx, 0, (size_t)P1 * K * sizeof(long long), (hipStream_t)hip_stream));
        return FRG_OK;
    }
    if (!p2) return fail(FRG_EINVAL, "null pointer");
    const bool self = p1 == p2 && P1 == P2;
    const size_t need = frg_knn_points_workspace_bytes(self ? 0 : P1, P2, K);
    if (!workspace || workspace_bytes < need) return fail(FRG_EALLOC, "workspace too small: need %zu bytes", need);
    if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return fail(FRG_EINVAL, "workspace must be 256-byte aligned");
    FRG_HIP(frg::launch_knn_points(P1, p1, P2, p2, K, self, dists, idx, workspace, (hipStream_t)hip_stream));
    return FRG_OK;
}

int frg_shell_points(int P, const float* bary_logits, const float* cell_verts, const long long* point_cell_indices,
                     float* points, void* hip_stream)
{
    if (P < 0) return fail(FRG_EINVAL, "P < 0");
    if (P == 0) return FRG_OK;
    if (!bary_logits || !cell_verts || !point_cell_indices || !points) return fail(FRG_EINVAL, "null pointer");
    FRG_HIP(frg::launch_shell_points(P, bary_logits, cell_verts, point_cell_indices, points, (hipStream_t)hip_stream));
    return FRG_OK;
}

int frg_shell_points_backward(int P, const float* bary_logits, const float* cell_verts, const long long* point_cell_indices,
                              const float* dL_dpoints, float* dL_dlogits, void* hip_stream)
{
    if (P < 0) return fail(FRG_EINVAL, "P < 0");
    if (P == 0) return FRG_OK;
    if (!bary_logits || !cell_verts || !point_cell_indices || !dL_dpoints || !dL_dlogits) return fail(FRG_EINVAL, "null pointer");
    FRG_HIP(frg::launch_shell_points_bwd(P, bary_logits, cell_verts, point_cell_indices, dL_dpoints, dL_dlogits,
                                         (hipStream_t)hip_stream));
    return FRG_OK;
}

// ---- adaptive density control (densify.hip) ----
int frg_densify_accumulate(int P, const int* radii, const float* dL_dmean2D, const unsigned char* row_live,
                           float* xyz_gradient_accum, float* denom, float* max_radii2D, void* hip_stream)
{
    if (P < 0) return fail(FRG_EINVAL, "P < 0");
    if (P == 0) return FRG_OK;
    if (!radii || !dL_dmean2D || !xyz_gradient_accum || !denom || !max_radii2D) return fail(FRG_EINVAL, "null pointer");
    FRG_HIP(frg::launch_densify_accumulate(P, radii, dL_dmean2D, row_live, xyz_gradient_accum, denom, max_radii2D,
                                           (hipStream_t)hip_stream));
    return FRG_OK;
}

int frg_densify_accumulate_views(const frg_densify_views_args* a)
{
    if (!a || a->struct_size != sizeof(frg_densify_views_args))
        return fail(FRG_EINVAL, "frg_densify_views_args: struct_size %zu, this library expects %zu", a ? a->struct_size : (size_t)0,
                    sizeof(frg_densify_views_args));
    if (a->P < 0 || a->first < 0 || a->count < 0 || (long long)a->first + a->count > a->P || a->first % 64 != 0)
        return fail(FRG_EINVAL, "bad range: P=%d first=%d (a multiple of 64) count=%d", a->P, a->first, a->count);
    if (a->n_views < 1 || a->n_views > 16) return fail(FRG_EINVAL, "1..16 views expected, got %d", a->n_views);
    if (a->capacity_rows < 0 || a->capacity_rows >= 65535LL * 256) return fail(FRG_EINVAL, "capacity_rows %lld: a packet holds fewer than 2^24 rows", a->capacity_rows);
    if (a->count == 0) return FRG_OK;
    const size_t need = frg_sum_packet_bytes_ex(a->count, a->capacity_rows, 1);
    if (!a->packets || a->packet_stride_bytes % 16 != 0 || a->packet_stride_bytes < need || reinterpret_cast<uintptr_t>(a->packets) % 16 != 0)
        return fail(FRG_EINVAL, "packets: stride %zu, a packet of %d Gaussians and %lld rows with its visibility section has %zu bytes (16-byte aligned)",
                    a->packet_stride_bytes, a->count, a->capacity_rows, need);
    if (!a->means3D) return fail(FRG_EINVAL, "means3D is required (shell-bound centres are not offered here)");
    if ((a->opacities == nullptr) == (a->raw_opacities == nullptr)) return fail(FRG_EINVAL, "provide exactly one of opacities / raw_opacities");
    const bool raw_sr = a->raw_scales && a->raw_rotations;
    if (raw_sr == (a->scales && a->rotations) || (a->raw_scales == nullptr) != (a->raw_rotations == nullptr) || (a->scales == nullptr) != (a->rotations == nullptr))
        return fail(FRG_EINVAL, "provide (scales, rotations) or (raw_scales, raw_rotations)");
    if (reinterpret_cast<uintptr_t>(a->rotations) % 16 != 0) return fail(FRG_EINVAL, "rotations must be 16-byte aligned");
    if (!a->xyz_gradient_accum || !a->denom || !a->max_radii2D) return fail(FRG_EINVAL, "null statistics pointer");
    frg::FwdInputs in{a->means3D, a->scales, a->rotations, a->opacities, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    in.raw.raw_opacity = a->raw_opacities; in.raw.raw_scale = a->raw_scales; in.raw.raw_rot = a->raw_rotations;
    FRG_HIP(frg::launch_densify_views(a->first, a->count, a->n_views, a->packets, a->packet_stride_bytes, (uint32_t)a->capacity_rows, in,
                                      a->xyz_gradient_accum, a->denom, a->max_radii2D, a->status, a->status_seq, (hipStream_t)a->hip_stream));
    return FRG_OK;
}

size_t frg_densify_workspace_bytes(int P) { return P > 0 ? frg::densify_workspace_bytes(P) : 0; }

int frg_densify_plan(int P, const float* raw_scales, const float* raw_opacities, const float* xyz_gradient_accum,
                     const float* denom, const frg_densify_params* params, int* plan, int* record,
                     char* workspace, size_t workspace_bytes, void* hip_stream)
{
    if (P <= 0) return fail(FRG_EINVAL, "P = %d: a model to densify has Gaussians", P);
    if (P > 0x7fffffff / 3) return fail(FRG_EINVAL, "P = %d: up to 3 P resulting rows must fit 31 bits", P);
    if (!params || params->struct_size < sizeof(frg_densify_params)) return fail(FRG_EINVAL, "frg_densify_params: struct_size");
    if (!raw_scales || !raw_opacities || !xyz_gradient_accum || !denom || !plan || !record) return fail(FRG_EINVAL, "null pointer");
    if (!workspace || workspace_bytes < frg_densify_workspace_bytes(P))
        return fail(FRG_EALLOC, "workspace too small: need %zu bytes", frg_densify_workspace_bytes(P));
    if (reinterpret_cast<uintptr_t>(workspace) % 4 != 0) return fail(FRG_EINVAL, "workspace must be 4-byte aligned");
    // the reference compares float32 tensors with Python floats: the products are formed in double and rounded once
    frg::DensifyThresholds t;
    t.max_grad = (float)params->max_grad;
    t.min_opacity = (float)params->min_opacity;
    t.dense_scale = (float)(params->percent_dense * params->extent);
    t.world_scale = (float)(0.1 * params->extent);
    t.prune_world = params->prune_big_points ? 1 : 0;
    FRG_HIP(frg::launch_densify_plan(P, raw_scales, raw_opacities, xyz_gradient_accum, denom, t, plan, record, workspace,
                                     (hipStream_t)hip_stream));
    return FRG_OK;
}

int frg_densify_apply(int P, int P_out, const int* plan, int n_groups, const int* group_width,
                      const long long* src_offsets, const long long* dst_offsets, long long out_numel, const float* noise,
                      const float* params, const float* exp_avg, const float* exp_avg_sq,
                      float* out_params, float* out_exp_avg, float* out_exp_avg_sq, void* hip_stream)
{
    if (P <= 0 || P_out < 0) return fail(FRG_EINVAL, "P = %d, P_out = %d", P, P_out);
    if (n_groups < 3 || n_groups > FRG_DENSIFY_MAX_GROUPS) return fail(FRG_EINVAL, "n_groups = %d: 3 .. %d", n_groups, FRG_DENSIFY_MAX_GROUPS);
    if (!plan || !group_width || !src_offsets || !dst_offsets || !params || !exp_avg || !exp_avg_sq) return fail(FRG_EINVAL, "null pointer");
    if (P_out > 0 && (!out_params || !out_exp_avg || !out_exp_avg_sq)) return fail(FRG_EINVAL, "null output buffer");
    if (group_width[0] != 3 || group_width[1] != 3 || group_width[2] != 4)
        return fail(FRG_EINVAL, "the first three groups must be means3D [P,3], scales [P,3], rotations [P,4]");
    frg::DensifyGroups g{};
    g.count = n_groups;
    g.dst_total = out_numel;
    for (int k = 0; k < n_groups; k++) {
        if (group_width[k] <= 0 || src_offsets[k] < 0 || dst_offsets[k] < 0 || (src_offsets[k] & 3) || (dst_offsets[k] & 3))
            return fail(FRG_EINVAL, "group %d: width %d, offsets %lld -> %lld (offsets are multiples of 4 elements)", k, group_width[k],
                        src_offsets[k], dst_offsets[k]);
        const long long end = k + 1 < n_groups ? dst_offsets[k + 1] : out_numel;
        if (dst_offsets[k] + (long long)P_out * group_width[k] > end || end - (dst_offsets[k] + (long long)P_out * group_width[k]) > 64)
            return fail(FRG_EINVAL, "group %d: %d rows of %d elements from %lld do not end at %lld", k, P_out, group_width[k], dst_offsets[k], end);
        if (k + 1 < n_groups && src_offsets[k] + (long long)P * group_width[k] > src_offsets[k + 1])
            return fail(FRG_EINVAL, "group %d overlaps the next in the old layout", k);
        g.width[k] = group_width[k];
        g.src_offset[k] = src_offsets[k];
        g.dst_offset[k] = dst_offsets[k];
    }
    if (P_out == 0) return FRG_OK;
    FRG_HIP(frg::launch_densify_apply(P, P_out, plan, g, noise, params, exp_avg, exp_avg_sq, out_params, out_exp_avg,
                                      out_exp_avg_sq, (hipStream_t)hip_stream));
    return FRG_OK;
}

int frg_reset_opacity(int P, float* raw_opacities, float* exp_avg, float* exp_avg_sq, void* hip_stream)
{
    if (P < 0) return fail(FRG_EINVAL, "P < 0");
    if (P == 0) return FRG_OK;
    if (!raw_opacities || !exp_avg || !exp_avg_sq) return fail(FRG_EINVAL, "null pointer");
    FRG_HIP(frg::launch_reset_opacity(P, raw_opacities, exp_avg, exp_avg_sq, (hipStream_t)hip_stream));
    return FRG_OK;
}

// ---- density / SDF field over K neighbour Gaussians (field.hip) ----
size_t frg_field_workspace_bytes(int P, int N, int K, int flags)
{
    if (P <= 0 || N <= 0 || K < 1 || K > FRG_KNN_MAX_K) return 0;
    return frg::field_workspace_bytes(P, N, K, (flags & FRG_FIELD_BACKWARD) != 0);
}

static int field_call(const frg_field_args* a, bool backward)
{
    const char* what = backward ? "frg_field_backward" : "frg_field_forward";
    if (!a || a->struct_size != sizeof(frg_field_args))
        return fail(FRG_EINVAL, "frg_field_args: struct_size %zu, this library expects %zu", a ? a->struct_size : (size_t)0, sizeof(frg_field_args));
    if (a->K < 1 || a->K > FRG_KNN_MAX_K) return fail(FRG_EINVAL, "%s: K = %d outside 1 ... %d", what, a->K, FRG_KNN_MAX_K);
    if (a->P < 0 || a->N < 0) return fail(FRG_EINVAL, "%s: P = %d or N = %d < 0", what, a->P, a->N);
    if ((long long)a->N * 32 > 0x7fffffffLL) return fail(FRG_EINVAL, "%s: N = %d: 32 N must stay below 2^31", what, a->N);
    if (a->beta_mode != FRG_FIELD_BETA_NONE && a->beta_mode != FRG_FIELD_BETA_AVERAGE && a->beta_mode != FRG_FIELD_BETA_WEIGHTED)
        return fail(FRG_EINVAL, "%s: unknown beta_mode %d", what, a->beta_mode);
    if (a->beta_mode == FRG_FIELD_BETA_NONE && (a->beta || a->sdf || a->dL_dbeta || a->dL_dsdf))
        return fail(FRG_EINVAL, "%s: beta and sdf need a beta_mode", what);
    if (a->N > 0 && a->P == 0) return fail(FRG_EINVAL, "%s: samples without Gaussians", what);
    if (a->N > 0 && (!a->idx || !a->x || !a->bad_index)) return fail(FRG_EINVAL, "%s: null pointer (idx, x, bad_index)", what);
    if (a->P > 0 && (!a->points || !a->scaling || !a->quaternions || !a->strengths)) return fail(FRG_EINVAL, "%s: null pointer (points, scaling, quaternions, strengths)", what);
    if (a->beta_mode == FRG_FIELD_BETA_WEIGHTED && !a->beta_fallback) return fail(FRG_EINVAL, "%s: null pointer (beta_fallback of the weighted average)", what);
    if (backward && ((a->N > 0 && !a->dL_dx) || (a->P > 0 && (!a->dL_dpoints || !a->dL_dscaling || !a->dL_dquaternions || !a->dL_dstrengths))))
        return fail(FRG_EINVAL, "%s: null gradient output", what);
    if ((reinterpret_cast<uintptr_t>(a->quaternions) | reinterpret_cast<uintptr_t>(a->dL_dquaternions)) % 16 != 0)
        return fail(FRG_EINVAL, "%s: quaternions and dL_dquaternions must be 16-byte aligned", what);
    hipStream_t s = (hipStream_t)a->hip_stream;
    if (a->N == 0) {                                       // no pair names anybody: every Gaussian's rows are zeros
        if (backward && a->P > 0) {
            FRG_HIP(hipMemsetAsync(a->dL_dpoints, 0, (size_t)a->P * 12, s));
            FRG_HIP(hipMemsetAsync(a->dL_dscaling, 0, (size_t)a->P * 12, s));
            FRG_HIP(hipMemsetAsync(a->dL_dquaternions, 0, (size_t)a->P * 16, s));
            FRG_HIP(hipMemsetAsync(a->dL_dstrengths, 0, (size_t)a->P * 4, s));
        }
        return FRG_OK;
    }
    const size_t need = frg::field_workspace_bytes(a->P, a->N, a->K, backward);
    if (!a->workspace || a->workspace_bytes < need) return fail(FRG_EINVAL, "%s: workspace too small: need %zu bytes", what, need);
    if (reinterpret_cast<uintptr_t>(a->workspace) % 256 != 0) return fail(FRG_EINVAL, "%s: workspace must be 256-byte aligned", what);
    frg::FieldLaunch p{};
    p.P = a->P; p.N = a->N; p.K = a->K; p.idx64 = a->idx_is_int64 ? 1 : 0; p.beta_mode = a->beta_mode;
    p.recompute = (a->flags & FRG_FIELD_RECOMPUTE) ? 1 : 0;
    p.idx = a->idx; p.x = a->x; p.points = a->points; p.scaling = a->scaling; p.quaternions = a->quaternions; p.strengths = a->strengths;
    // the reference's Python floats: formed in double, rounded once where a float32 tensor op takes them
    p.density_factor = a->density_factor;
    p.sdf_offset = std::sqrt(-2.0 * std::log(std::fmin(a->density_threshold, 1.0)));
    p.opacity_min_clamp = a->opacity_min_clamp;
    p.beta_fallback = a->beta_fallback;
    p.density = a->density; p.opacities = a->opacities; p.beta = a->beta; p.sdf = a->sdf;
    p.g_density = a->dL_ddensity; p.g_opacities = a->dL_dopacities; p.g_beta = a->dL_dbeta; p.g_sdf = a->dL_dsdf;
    p.dL_dx = a->dL_dx; p.dL_dpoints = a->dL_dpoints; p.dL_dscaling = a->dL_dscaling; p.dL_dquaternions = a->dL_dquaternions;
    p.dL_dstrengths = a->dL_dstrengths;
    p.bad_index = a->bad_index;
    FRG_HIP(frg::launch_field(p, backward, a->workspace, s));
    return FRG_OK;
}

int frg_field_forward(const frg_field_args* a) { return field_call(a, false); }
int frg_field_backward(const frg_field_args* a) { return field_call(a, true); }

// ---- level crossings of the density field along rays (levelset.hip) ----
size_t frg_levelset_workspace_bytes(int P, int R, int K, int flags)
{
    (void)flags;
    if (P <= 0 || R <= 0 || K < 1 || K > FRG_KNN_MAX_K) return 0;
    return frg::levelset_workspace_bytes(P);
}

int frg_levelset(const frg_levelset_args* a)
{
    const char* what = "frg_levelset";
    if (!a || a->struct_size != sizeof(frg_levelset_args))
        return fail(FRG_EINVAL, "frg_levelset_args: struct_size %zu, this library expects %zu", a ? a->struct_size : (size_t)0, sizeof(frg_levelset_args));
    if (a->K < 1 || a->K > FRG_KNN_MAX_K) return fail(FRG_EINVAL, "%s: K = %d outside 1 ... %d", what, a->K, FRG_KNN_MAX_K);
    if (a->n < 2 || a->n > FRG_LEVELSET_MAX_SAMPLES) return fail(FRG_EINVAL, "%s: n = %d samples outside 2 ... %d", what, a->n, FRG_LEVELSET_MAX_SAMPLES);
    if (a->L < 1 || a->L > FRG_LEVELSET_MAX_LEVELS) return fail(FRG_EINVAL, "%s: L = %d levels outside 1 ... %d", what, a->L, FRG_LEVELSET_MAX_LEVELS);
    if (a->inner_mode != FRG_LEVELSET_INNER_LAST && a->inner_mode != FRG_LEVELSET_INNER_SECOND_CROSSING)
        return fail(FRG_EINVAL, "%s: unknown inner_mode %d", what, a->inner_mode);
    if (a->P < 0 || a->R < 0) return fail(FRG_EINVAL, "%s: P = %d or R = %d < 0", what, a->P, a->R);
    if ((long long)a->R * (a->n > a->K ? a->n : a->K) > 0x7fffffffLL)
        return fail(FRG_EINVAL, "%s: R = %d: R * max(n, K) must stay below 2^31", what, a->R);
    if (a->R == 0) return FRG_OK;
    if (a->P == 0) return fail(FRG_EINVAL, "%s: rays without Gaussians", what);
    if (!a->idx || !a->origins || !a->directions || !a->t_scale || !a->t_offset || !a->lin || !a->bad_index)
        return fail(FRG_EINVAL, "%s: null pointer (idx, origins, directions, t_scale, t_offset, lin, bad_index)", what);
    if (!a->points || !a->scaling || !a->quaternions || !a->strengths) return fail(FRG_EINVAL, "%s: null pointer (points, scaling, quaternions, strengths)", what);
    if (reinterpret_cast<uintptr_t>(a->quaternions) % 16 != 0) return fail(FRG_EINVAL, "%s: quaternions must be 16-byte aligned", what);
    const size_t need = frg::levelset_workspace_bytes(a->P);
    if (!a->workspace || a->workspace_bytes < need) return fail(FRG_EINVAL, "%s: workspace too small: need %zu bytes", what, need);
    if (reinterpret_cast<uintptr_t>(a->workspace) % 256 != 0) return fail(FRG_EINVAL, "%s: workspace must be 256-byte aligned", what);
    frg::LevelsetLaunch p{};
    p.P = a->P; p.R = a->R; p.K = a->K; p.n = a->n; p.L = a->L; p.idx64 = a->idx_is_int64 ? 1 : 0; p.inner_mode = a->inner_mode;
    p.idx = a->idx; p.origins = a->origins; p.directions = a->directions; p.t_scale = a->t_scale; p.t_offset = a->t_offset; p.lin = a->lin;
    for (int l = 0; l < a->L; l++) p.levels[l] = (float)a->levels[l];
    p.density_factor = (float)a->density_factor;
    p.densities = a->densities; p.t_outer = a->t_outer; p.t_inner = a->t_inner; p.first_above = a->first_above;
    p.last_above = a->last_above; p.under_first = a->under_first; p.normals = a->normals; p.bad_index = a->bad_index;
    FRG_HIP(frg::launch_levelset(p, a->points, a->scaling, a->quaternions, a->strengths, a->workspace, (hipStream_t)a->hip_stream));
    return FRG_OK;
}

}  // extern "C"
