// PyTorch-ROCm extension module `diff_gaussian_rasterization._C`.
//
// Drop-in for the reference's pybind module (DGR = gaussian_splatting/submodules/
// diff-gaussian-rasterization): DGR/ext.cpp:15-18 exports rasterize_gaussians,
// rasterize_gaussians_backward and mark_visible with the signatures of
// DGR/rasterize_points.h:18-67; so does this file, positional argument for positional
// argument and tuple slot for tuple slot.  Underneath there is no CUDA-shaped code at all:
// the three functions marshal tensors into the C ABI of libfrosting_rasterizer.so
// (include/frosting_rasterizer.h -- frg_forward_ex / frg_backward / frg_mark_visible), on
// torch's CURRENT HIP stream under a device guard for means3D's device (the reference
// launches on the legacy default stream, e.g. forward.cu:389).
//
// Differences that a caller can observe, all permitted by the reference's contract:
//   * absent optional inputs are recognised by numel() == 0 (the reference tests
//     data_ptr() == nullptr, forward.cu:205,241);
//   * outputs are torch::empty, not zero-filled: every element is written by the kernels
//     (the reference must pre-zero ~300 B/Gaussian of gradients, rasterize_points.cu:151-159);
//   * scratch comes from torch's caching allocator through the C ABI's allocation callbacks
//     (replaces resizeFunctional, rasterize_points.cu:27-33): after the first view no
//     hipMalloc remains on the path, and -- unlike one shared arena -- several forwards may
//     be outstanding before their backwards run;
//   * one extra export, rasterize_gaussians_masked(..., keep_mask): Frosting's occlusion
//     culling as a per-Gaussian skip flag (frosting_scene/frosting_model.py:1564-1586).
#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <string>
#include <tuple>
#include <vector>

#include "frosting_rasterizer.h"

namespace {

// One growable byte tensor per scratch chunk; `grow` is the frg_alloc_fn the C ABI calls.
struct Chunk {
    torch::Tensor t;
    torch::Device device;
    explicit Chunk(torch::Device d) : t(torch::empty({0}, torch::TensorOptions(torch::kByte).device(d))), device(d) {}
    static char* grow(void* user, size_t bytes)
    {
        Chunk* c = static_cast<Chunk*>(user);
        c->t = torch::empty({static_cast<int64_t>(bytes ? bytes : 1)}, torch::TensorOptions(torch::kByte).device(c->device));
        return reinterpret_cast<char*>(c->t.data_ptr());
    }
};

// The C ABI hands every callback the same `user`; three chunks -> three trampolines over one struct.
struct Chunks {
    Chunk geom, binning, img;
    explicit Chunks(torch::Device d) : geom(d), binning(d), img(d) {}
    static char* grow_geom(void* u, size_t n) { return Chunk::grow(&static_cast<Chunks*>(u)->geom, n); }
    static char* grow_binning(void* u, size_t n) { return Chunk::grow(&static_cast<Chunks*>(u)->binning, n); }
    static char* grow_img(void* u, size_t n) { return Chunk::grow(&static_cast<Chunks*>(u)->img, n); }
};

// float32 device pointer of an optional input; NULL when the tensor is the reference's
// "absent" encoding (empty tensor, DGR/diff_gaussian_rasterization/__init__.py:197-207)
const float* opt_f32(const torch::Tensor& t, const torch::Device& dev, const char* name, torch::Tensor& keep_alive)
{
    if (!t.defined() || t.numel() == 0) return nullptr;
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be float32, got ", t.scalar_type());
    TORCH_CHECK(t.device() == dev, name, " is on ", t.device(), ", expected ", dev);
    keep_alive = t.contiguous();
    return keep_alive.data_ptr<float>();
}

// frg_forward_args / frg_backward_args::sh_rotations: [P,3,3] float32 on the Gaussians' device, made contiguous; an empty
// tensor means none
const float* opt_sh_rotations(const torch::Tensor& t, int P, const torch::Device& dev, torch::Tensor& keep_alive)
{
    if (!t.defined() || t.numel() == 0) return nullptr;
    TORCH_CHECK(t.dim() == 3 && t.size(0) == P && t.size(1) == 3 && t.size(2) == 3 && t.scalar_type() == torch::kFloat32 && t.device() == dev,
                "sh_rotations must be a float32 tensor of shape (num_points, 3, 3) on the Gaussians' device");
    keep_alive = t.contiguous();
    return keep_alive.data_ptr<float>();
}

void check_rc(int rc, const char* what)
{
    TORCH_CHECK(rc >= 0, what, " failed (", rc, "): ", frg_last_error());
}

std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
forward_common(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors,
               const torch::Tensor& opacity, const torch::Tensor& scales, const torch::Tensor& rotations,
               const float scale_modifier, const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
               const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy, const int image_height,
               const int image_width, const torch::Tensor& sh, const int degree, const torch::Tensor& campos,
               const bool prefiltered, const bool debug, const torch::Tensor* keep_mask, const bool forward_only = false,
               const int exact_blend = -1, const torch::Tensor* sh_rotations = nullptr)
{
    TORCH_CHECK(means3D.dim() == 2 && means3D.size(1) == 3, "means3D must have dimensions (num_points, 3)");  // rasterize_points.cu:57-59
    TORCH_CHECK(means3D.is_cuda(), "frosting_amd rasterizer: means3D must live on a ROCm device (no CPU path)");
    const torch::Device dev = means3D.device();
    const c10::hip::HIPGuard guard(dev.index());
    const int P = static_cast<int>(means3D.size(0));
    const int H = image_height, W = image_width;

    torch::Tensor out_color = torch::empty({3, H, W}, means3D.options().dtype(torch::kFloat32));
    torch::Tensor radii = torch::empty({P}, means3D.options().dtype(torch::kInt32));
    Chunks chunks(dev);

    torch::Tensor k[13];
    frg_forward_args a{};
    a.struct_size = sizeof(a);
    a.geometry_alloc = &Chunks::grow_geom;
    a.binning_alloc = &Chunks::grow_binning;
    a.image_alloc = &Chunks::grow_img;
    a.user = &chunks;
    a.P = P;
    a.D = degree;
    a.M = (sh.defined() && sh.numel() != 0) ? static_cast<int>(sh.size(1)) : 0;   // rasterize_points.cu:83-87
    a.background = opt_f32(background, dev, "background", k[0]);
    a.width = W;
    a.height = H;
    a.means3D = opt_f32(means3D, dev, "means3D", k[1]);
    a.shs = opt_f32(sh, dev, "sh", k[2]);
    a.colors_precomp = opt_f32(colors, dev, "colors", k[3]);
    a.opacities = opt_f32(opacity, dev, "opacity", k[4]);
    a.scales = opt_f32(scales, dev, "scales", k[5]);
    a.scale_modifier = scale_modifier;
    a.rotations = opt_f32(rotations, dev, "rotations", k[6]);
    a.cov3D_precomp = opt_f32(cov3D_precomp, dev, "cov3D_precomp", k[7]);
    a.viewmatrix = opt_f32(viewmatrix, dev, "viewmatrix", k[8]);
    a.projmatrix = opt_f32(projmatrix, dev, "projmatrix", k[9]);
    a.cam_pos = opt_f32(campos, dev, "campos", k[10]);
    a.tan_fovx = tan_fovx;
    a.tan_fovy = tan_fovy;
    a.prefiltered = prefiltered ? 1 : 0;
    a.out_color = out_color.data_ptr<float>();
    a.radii = P ? radii.data_ptr<int>() : nullptr;
    a.debug = debug ? 1 : 0;
    a.hip_stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
    a.instance_capacity = 0;
    a.keep_mask = nullptr;
    a.forward_only = forward_only ? 1 : 0;
    TORCH_CHECK(exact_blend >= -1 && exact_blend <= 1, "exact_blend must be -1 (the process option), 0 or 1");
    a.exact_blend = exact_blend + 1;      // frg_forward_args: 0 = the process-wide option, k + 1 = value k for this call
    if (keep_mask && keep_mask->defined() && P && keep_mask->numel() != 0) {   // (the forward-only / _ex exports take an empty tensor for "no mask")
        TORCH_CHECK(keep_mask->dim() == 1 && keep_mask->size(0) == P && keep_mask->device() == dev &&
                        (keep_mask->scalar_type() == torch::kBool || keep_mask->scalar_type() == torch::kUInt8),
                    "keep_mask must be a bool / uint8 tensor of shape (num_points,) on the Gaussians' device");
        k[11] = keep_mask->contiguous();
        a.keep_mask = static_cast<const unsigned char*>(k[11].data_ptr());
    }
    if (sh_rotations) a.sh_rotations = opt_sh_rotations(*sh_rotations, P, dev, k[12]);
    const int rendered = frg_forward_ex(&a);
    check_rc(rendered, "frg_forward");
    return std::make_tuple(rendered, out_color, radii, chunks.geom.t, chunks.binning.t, chunks.img.t);
}

}  // namespace

// DGR/rasterize_points.h:18-38
std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansHIP(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors,
                      const torch::Tensor& opacity, const torch::Tensor& scales, const torch::Tensor& rotations,
                      const float scale_modifier, const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                      const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy, const int image_height,
                      const int image_width, const torch::Tensor& sh, const int degree, const torch::Tensor& campos,
                      const bool prefiltered, const bool debug)
{
    return forward_common(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                          projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                          nullptr);
}

std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansMaskedHIP(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors,
                            const torch::Tensor& opacity, const torch::Tensor& scales, const torch::Tensor& rotations,
                            const float scale_modifier, const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                            const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                            const int image_height, const int image_width, const torch::Tensor& sh, const int degree,
                            const torch::Tensor& campos, const bool prefiltered, const bool debug,
                            const torch::Tensor& keep_mask)
{
    return forward_common(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                          projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                          &keep_mask);
}

// the forward of a call no backward will follow (frg_forward_args::forward_only): the 19 arguments + keep_mask (may be empty)
std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansForwardOnlyHIP(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors,
                                 const torch::Tensor& opacity, const torch::Tensor& scales, const torch::Tensor& rotations,
                                 const float scale_modifier, const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                                 const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                                 const int image_height, const int image_width, const torch::Tensor& sh, const int degree,
                                 const torch::Tensor& campos, const bool prefiltered, const bool debug,
                                 const torch::Tensor& keep_mask)
{
    return forward_common(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                          projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                          &keep_mask, true);
}

// exact_blend: -1 = the arithmetic of the forward that filled the buffers (what the library remembers of it, else what it
// stamped into imageBuffer), 0 | 1 = the caller carried the forward's mode itself (the autograd ctx of frosting_amd/rasterizer.py)
static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
backward_common(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii,
                const torch::Tensor& colors, const torch::Tensor& scales, const torch::Tensor& rotations,
                const float scale_modifier, const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                const torch::Tensor& dL_dout_color, const torch::Tensor& sh, const int degree,
                const torch::Tensor& campos, const torch::Tensor& geomBuffer, const int R,
                const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const bool debug, const int exact_blend,
                const torch::Tensor* sh_rotations = nullptr)
{
    TORCH_CHECK(exact_blend >= -1 && exact_blend <= 1, "exact_blend must be -1 (as the forward), 0 or 1");
    TORCH_CHECK(means3D.is_cuda(), "frosting_amd rasterizer: means3D must live on a ROCm device (no CPU path)");
    const torch::Device dev = means3D.device();
    const c10::hip::HIPGuard guard(dev.index());
    const int P = static_cast<int>(means3D.size(0));
    const int H = static_cast<int>(dL_dout_color.size(1)), W = static_cast<int>(dL_dout_color.size(2));  // rasterize_points.cu:142-143
    const bool has_sh = sh.defined() && sh.numel() != 0;
    const bool has_sr = scales.defined() && scales.numel() != 0;
    const int M = has_sh ? static_cast<int>(sh.size(1)) : 0;

    const auto f32 = means3D.options().dtype(torch::kFloat32);
    torch::Tensor dL_dmeans3D = torch::empty({P, 3}, f32), dL_dmeans2D = torch::empty({P, 3}, f32);
    torch::Tensor dL_dcolors = torch::empty({P, 3}, f32), dL_dopacity = torch::empty({P, 1}, f32);
    torch::Tensor dL_dcov3D = torch::empty({P, 6}, f32);
    // rows the kernels do not write (absent input) stay zero, as in the reference's zero-allocated outputs
    torch::Tensor dL_dsh = has_sh ? torch::empty({P, M, 3}, f32) : torch::zeros({P, M, 3}, f32);
    torch::Tensor dL_dscales = has_sr ? torch::empty({P, 3}, f32) : torch::zeros({P, 3}, f32);
    torch::Tensor dL_drotations = has_sr ? torch::empty({P, 4}, f32) : torch::zeros({P, 4}, f32);

    if (P != 0) {
        torch::Tensor k[12];
        const size_t ws_bytes = frg_backward_workspace_bytes(P, R);
        torch::Tensor workspace = torch::empty({static_cast<int64_t>(ws_bytes)}, torch::TensorOptions(torch::kByte).device(dev));
        torch::Tensor radii_c = radii.contiguous();
        TORCH_CHECK(radii_c.scalar_type() == torch::kInt32 && radii_c.device() == dev, "radii must be int32 on ", dev);
        TORCH_CHECK(geomBuffer.device() == dev && binningBuffer.device() == dev && imageBuffer.device() == dev,
                    "the forward's scratch buffers must be on ", dev);
        frg_backward_args a{};
        a.struct_size = sizeof(a);
        a.P = P; a.D = degree; a.M = M; a.R = R;
        a.background = opt_f32(background, dev, "background", k[0]);
        a.width = W; a.height = H;
        a.means3D = opt_f32(means3D, dev, "means3D", k[1]);
        a.shs = opt_f32(sh, dev, "sh", k[2]);
        a.colors_precomp = opt_f32(colors, dev, "colors", k[3]);
        a.scales = opt_f32(scales, dev, "scales", k[4]);
        a.scale_modifier = scale_modifier;
        a.rotations = opt_f32(rotations, dev, "rotations", k[5]);
        a.cov3D_precomp = opt_f32(cov3D_precomp, dev, "cov3D_precomp", k[6]);
        a.viewmatrix = opt_f32(viewmatrix, dev, "viewmatrix", k[7]);
        a.projmatrix = opt_f32(projmatrix, dev, "projmatrix", k[8]);
        a.campos = opt_f32(campos, dev, "campos", k[9]);
        a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy;
        a.radii = radii_c.data_ptr<int>();
        a.geom_buffer = reinterpret_cast<char*>(geomBuffer.data_ptr());
        a.binning_buffer = reinterpret_cast<char*>(binningBuffer.data_ptr());
        a.image_buffer = reinterpret_cast<char*>(imageBuffer.data_ptr());
        a.dL_dpix = opt_f32(dL_dout_color, dev, "dL_dout_color", k[10]);
        a.dL_dmean2D = dL_dmeans2D.data_ptr<float>();
        a.dL_dconic = nullptr;                      // never returned (rasterize_points.cu:195)
        a.dL_dopacity = dL_dopacity.data_ptr<float>();
        a.dL_dcolor = dL_dcolors.data_ptr<float>();
        a.dL_dmean3D = dL_dmeans3D.data_ptr<float>();
        a.dL_dcov3D = dL_dcov3D.data_ptr<float>();
        a.dL_dsh = has_sh ? dL_dsh.data_ptr<float>() : nullptr;
        a.dL_dscale = has_sr ? dL_dscales.data_ptr<float>() : nullptr;
        a.dL_drot = has_sr ? dL_drotations.data_ptr<float>() : nullptr;
        a.workspace = reinterpret_cast<char*>(workspace.data_ptr());
        a.workspace_bytes = ws_bytes;
        a.debug = debug ? 1 : 0;
        a.hip_stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
        a.exact_blend = exact_blend + 1;            // frg_backward_args: 0 = as the forward, k + 1 = value k
        if (sh_rotations) a.sh_rotations = opt_sh_rotations(*sh_rotations, P, dev, k[11]);
        const int rc = frg_backward_ex(&a);
        check_rc(rc, "frg_backward");
        // `workspace` returns to the caching allocator here; reuse is ordered on this same stream
    }
    return std::make_tuple(dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations);
}

// DGR/rasterize_points.h:40-62; returns the reference's eight gradients in its order (rasterize_points.cu:195)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansBackwardHIP(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii,
                              const torch::Tensor& colors, const torch::Tensor& scales, const torch::Tensor& rotations,
                              const float scale_modifier, const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                              const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                              const torch::Tensor& dL_dout_color, const torch::Tensor& sh, const int degree,
                              const torch::Tensor& campos, const torch::Tensor& geomBuffer, const int R,
                              const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const bool debug)
{
    return backward_common(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                           projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer,
                           imageBuffer, debug, -1);
}

// The same with the forward's blend arithmetic handed over by the caller (who carried it beside the buffers -- the autograd
// ctx): nothing about the forward has to be remembered by the library or read back from the buffers.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansBackwardExHIP(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii,
                                const torch::Tensor& colors, const torch::Tensor& scales, const torch::Tensor& rotations,
                                const float scale_modifier, const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                                const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                                const torch::Tensor& dL_dout_color, const torch::Tensor& sh, const int degree,
                                const torch::Tensor& campos, const torch::Tensor& geomBuffer, const int R,
                                const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const bool debug,
                                const int exact_blend)
{
    return backward_common(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                           projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer,
                           imageBuffer, debug, exact_blend);
}

// every forward option of the Python layer in one export: the 19 arguments, keep_mask (may be empty), exact_blend
// (-1 = the process option | 0 | 1, for THIS call), forward_only
std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansExHIP(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors,
                        const torch::Tensor& opacity, const torch::Tensor& scales, const torch::Tensor& rotations,
                        const float scale_modifier, const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                        const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                        const int image_height, const int image_width, const torch::Tensor& sh, const int degree,
                        const torch::Tensor& campos, const bool prefiltered, const bool debug,
                        const torch::Tensor& keep_mask, const int exact_blend, const bool forward_only)
{
    return forward_common(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                          projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                          &keep_mask, forward_only, exact_blend);
}

// rasterize_gaussians_ex + sh_rotations ([P,3,3], or empty for none): the SH colour of Gaussian i is evaluated at d @ R_i
std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansRotHIP(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors,
                         const torch::Tensor& opacity, const torch::Tensor& scales, const torch::Tensor& rotations,
                         const float scale_modifier, const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                         const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                         const int image_height, const int image_width, const torch::Tensor& sh, const int degree,
                         const torch::Tensor& campos, const bool prefiltered, const bool debug,
                         const torch::Tensor& keep_mask, const int exact_blend, const bool forward_only,
                         const torch::Tensor& sh_rotations)
{
    return forward_common(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                          projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                          &keep_mask, forward_only, exact_blend, &sh_rotations);
}

// rasterize_gaussians_backward_ex + the forward's sh_rotations (empty exactly when it had none)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansBackwardRotHIP(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii,
                                 const torch::Tensor& colors, const torch::Tensor& scales, const torch::Tensor& rotations,
                                 const float scale_modifier, const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                                 const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                                 const torch::Tensor& dL_dout_color, const torch::Tensor& sh, const int degree,
                                 const torch::Tensor& campos, const torch::Tensor& geomBuffer, const int R,
                                 const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const bool debug,
                                 const int exact_blend, const torch::Tensor& sh_rotations)
{
    return backward_common(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                           projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer,
                           imageBuffer, debug, exact_blend, &sh_rotations);
}

// DGR/rasterize_points.h:64-67, rasterize_points.cu:198-217
torch::Tensor markVisibleHIP(torch::Tensor& means3D, torch::Tensor& viewmatrix, torch::Tensor& projmatrix)
{
    TORCH_CHECK(means3D.is_cuda(), "frosting_amd rasterizer: means3D must live on a ROCm device (no CPU path)");
    const torch::Device dev = means3D.device();
    const c10::hip::HIPGuard guard(dev.index());
    const int P = static_cast<int>(means3D.size(0));
    torch::Tensor present = torch::zeros({P}, means3D.options().dtype(torch::kBool));
    if (P != 0) {
        torch::Tensor k[3];
        const int rc = frg_mark_visible(P, opt_f32(means3D, dev, "means3D", k[0]), opt_f32(viewmatrix, dev, "viewmatrix", k[1]),
                                        opt_f32(projmatrix, dev, "projmatrix", k[2]),
                                        static_cast<unsigned char*>(present.data_ptr()),
                                        c10::hip::getCurrentHIPStream(dev.index()).stream());
        check_rc(rc, "frg_mark_visible");
    }
    return present;
}

// ---- adaptive density control (frg_densify_*, frg_reset_opacity): what frosting_amd/densify.py calls through ctypes ----
namespace {

void check_on(const torch::Tensor& t, const torch::Device& dev, torch::ScalarType type, int64_t numel, const char* name)
{
    TORCH_CHECK(t.defined() && t.device() == dev && t.scalar_type() == type && t.is_contiguous() && (numel < 0 || t.numel() == numel),
                name, ": expected a contiguous ", type, " tensor", numel < 0 ? "" : " of the model's size", " on ", dev);
}

}  // namespace

void DensifyAccumulateHIP(const torch::Tensor& radii, const torch::Tensor& dL_dmean2D, const torch::Tensor& row_live,
                          torch::Tensor& xyz_gradient_accum, torch::Tensor& denom, torch::Tensor& max_radii2D)
{
    TORCH_CHECK(radii.is_cuda(), "frosting_amd densify: tensors must live on a ROCm device (no CPU path)");
    const torch::Device dev = radii.device();
    const c10::hip::HIPGuard guard(dev.index());
    const int64_t P = radii.numel();
    check_on(radii, dev, torch::kInt32, P, "radii");
    check_on(dL_dmean2D, dev, torch::kFloat32, 3 * P, "dL_dmean2D");
    check_on(xyz_gradient_accum, dev, torch::kFloat32, P, "xyz_gradient_accum");
    check_on(denom, dev, torch::kFloat32, P, "denom");
    check_on(max_radii2D, dev, torch::kFloat32, P, "max_radii2D");
    const bool masked = row_live.defined() && row_live.numel() != 0;
    if (masked) check_on(row_live, dev, torch::kUInt8, P, "row_live");
    check_rc(frg_densify_accumulate(static_cast<int>(P), radii.data_ptr<int>(), dL_dmean2D.data_ptr<float>(),
                                    masked ? row_live.data_ptr<unsigned char>() : nullptr, xyz_gradient_accum.data_ptr<float>(),
                                    denom.data_ptr<float>(), max_radii2D.data_ptr<float>(),
                                    c10::hip::getCurrentHIPStream(dev.index()).stream()),
             "frg_densify_accumulate");
}

// the statistics of every view of a view-parallel step from the gathered slot-sum packets (frg_densify_accumulate_views)
void DensifyAccumulateViewsHIP(const torch::Tensor& packets, const int64_t first, const int64_t count, const int64_t capacity_rows,
                               const torch::Tensor& means3D, const torch::Tensor& scales, const torch::Tensor& rotations,
                               const torch::Tensor& opacities, const bool raw_params, torch::Tensor& xyz_gradient_accum,
                               torch::Tensor& denom, torch::Tensor& max_radii2D, const torch::Tensor& status, const int64_t status_seq)
{
    TORCH_CHECK(packets.is_cuda(), "frosting_amd densify: tensors must live on a ROCm device (no CPU path)");
    const torch::Device dev = packets.device();
    const c10::hip::HIPGuard guard(dev.index());
    TORCH_CHECK(packets.dim() == 2, "packets must be [n_views, words]");
    check_on(packets, dev, torch::kInt32, -1, "packets");
    const int64_t P = max_radii2D.numel();
    check_on(means3D, dev, torch::kFloat32, 3 * P, "means3D");
    check_on(scales, dev, torch::kFloat32, 3 * P, "scales");
    check_on(rotations, dev, torch::kFloat32, 4 * P, "rotations");
    check_on(opacities, dev, torch::kFloat32, P, "opacities");
    check_on(xyz_gradient_accum, dev, torch::kFloat32, P, "xyz_gradient_accum");
    check_on(denom, dev, torch::kFloat32, P, "denom");
    check_on(max_radii2D, dev, torch::kFloat32, P, "max_radii2D");
    const bool posts = status.defined() && status.numel() != 0;
    if (posts)
        TORCH_CHECK(status.scalar_type() == torch::kInt64 && status.is_contiguous() && (status.is_pinned() || status.device() == dev),
                    "status: one int64 word in pinned host memory or on the device");
    frg_densify_views_args a{};
    a.struct_size = sizeof(a);
    a.P = static_cast<int>(P); a.first = static_cast<int>(first); a.count = static_cast<int>(count);
    a.n_views = static_cast<int>(packets.size(0));
    a.packets = packets.data_ptr();
    a.packet_stride_bytes = static_cast<size_t>(packets.size(1)) * 4;
    a.capacity_rows = capacity_rows;
    a.means3D = means3D.data_ptr<float>();
    (raw_params ? a.raw_scales : a.scales) = scales.data_ptr<float>();
    (raw_params ? a.raw_rotations : a.rotations) = rotations.data_ptr<float>();
    (raw_params ? a.raw_opacities : a.opacities) = opacities.data_ptr<float>();
    a.xyz_gradient_accum = xyz_gradient_accum.data_ptr<float>(); a.denom = denom.data_ptr<float>(); a.max_radii2D = max_radii2D.data_ptr<float>();
    a.status = posts ? reinterpret_cast<unsigned long long*>(status.data_ptr()) : nullptr;
    a.status_seq = static_cast<unsigned int>(status_seq);
    a.hip_stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
    check_rc(frg_densify_accumulate_views(&a), "frg_densify_accumulate_views");
}

// -> (plan [4,P] int32, record [8] int32 on the device)
std::tuple<torch::Tensor, torch::Tensor>
DensifyPlanHIP(const torch::Tensor& raw_scales, const torch::Tensor& raw_opacities, const torch::Tensor& xyz_gradient_accum,
               const torch::Tensor& denom, const double max_grad, const double min_opacity, const double extent,
               const double percent_dense, const bool prune_big_points)
{
    TORCH_CHECK(raw_scales.is_cuda(), "frosting_amd densify: tensors must live on a ROCm device (no CPU path)");
    const torch::Device dev = raw_scales.device();
    const c10::hip::HIPGuard guard(dev.index());
    const int64_t P = raw_opacities.numel();
    check_on(raw_scales, dev, torch::kFloat32, 3 * P, "raw_scales");
    check_on(raw_opacities, dev, torch::kFloat32, P, "raw_opacities");
    check_on(xyz_gradient_accum, dev, torch::kFloat32, P, "xyz_gradient_accum");
    check_on(denom, dev, torch::kFloat32, P, "denom");
    const auto i32 = torch::TensorOptions(torch::kInt32).device(dev);
    torch::Tensor plan = torch::empty({4, P}, i32), record = torch::empty({8}, i32);
    const size_t ws_bytes = frg_densify_workspace_bytes(static_cast<int>(P));
    torch::Tensor workspace = torch::empty({static_cast<int64_t>(ws_bytes ? ws_bytes : 1)}, torch::TensorOptions(torch::kByte).device(dev));
    frg_densify_params prm{};
    prm.struct_size = sizeof(prm);
    prm.max_grad = max_grad; prm.min_opacity = min_opacity; prm.extent = extent; prm.percent_dense = percent_dense;
    prm.prune_big_points = prune_big_points ? 1 : 0;
    check_rc(frg_densify_plan(static_cast<int>(P), raw_scales.data_ptr<float>(), raw_opacities.data_ptr<float>(),
                              xyz_gradient_accum.data_ptr<float>(), denom.data_ptr<float>(), &prm, plan.data_ptr<int>(),
                              record.data_ptr<int>(), reinterpret_cast<char*>(workspace.data_ptr()), ws_bytes,
                              c10::hip::getCurrentHIPStream(dev.index()).stream()),
             "frg_densify_plan");
    return std::make_tuple(plan, record);
}

// -> the new (params, exp_avg, exp_avg_sq) flat buffers of out_numel elements
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>
DensifyApplyHIP(const torch::Tensor& plan, const int64_t P_out, const std::vector<int64_t>& group_width,
                const std::vector<int64_t>& src_offsets, const std::vector<int64_t>& dst_offsets, const int64_t out_numel,
                const torch::Tensor& noise, const torch::Tensor& params, const torch::Tensor& exp_avg, const torch::Tensor& exp_avg_sq)
{
    TORCH_CHECK(params.is_cuda(), "frosting_amd densify: tensors must live on a ROCm device (no CPU path)");
    const torch::Device dev = params.device();
    const c10::hip::HIPGuard guard(dev.index());
    TORCH_CHECK(plan.dim() == 2 && plan.size(0) == 4, "plan must be [4, P]");
    const int64_t P = plan.size(1);
    check_on(plan, dev, torch::kInt32, 4 * P, "plan");
    check_on(params, dev, torch::kFloat32, -1, "params");
    check_on(exp_avg, dev, torch::kFloat32, params.numel(), "exp_avg");
    check_on(exp_avg_sq, dev, torch::kFloat32, params.numel(), "exp_avg_sq");
    const bool has_noise = noise.defined() && noise.numel() != 0;
    if (has_noise) check_on(noise, dev, torch::kFloat32, 6 * P, "noise");
    const size_t n = group_width.size();
    TORCH_CHECK(n >= 3 && n <= FRG_DENSIFY_MAX_GROUPS && src_offsets.size() == n && dst_offsets.size() == n, "3 .. 8 groups, one width and two offsets each");
    int widths[FRG_DENSIFY_MAX_GROUPS];
    long long so[FRG_DENSIFY_MAX_GROUPS], dof[FRG_DENSIFY_MAX_GROUPS];
    for (size_t k = 0; k < n; k++) {
        widths[k] = static_cast<int>(group_width[k]); so[k] = src_offsets[k]; dof[k] = dst_offsets[k];
        TORCH_CHECK(so[k] >= 0 && so[k] + P * group_width[k] <= params.numel(), "group ", k, " does not lie inside the old buffers");
    }
    TORCH_CHECK(out_numel >= 0 && P_out >= 0 && P_out <= 3 * P, "bad output size");
    const auto f32 = params.options();
    torch::Tensor out = torch::empty({out_numel}, f32), out_m = torch::empty({out_numel}, f32), out_v = torch::empty({out_numel}, f32);
    check_rc(frg_densify_apply(static_cast<int>(P), static_cast<int>(P_out), plan.data_ptr<int>(), static_cast<int>(n), widths, so, dof,
                               out_numel, has_noise ? noise.data_ptr<float>() : nullptr, params.data_ptr<float>(),
                               exp_avg.data_ptr<float>(), exp_avg_sq.data_ptr<float>(), out.data_ptr<float>(), out_m.data_ptr<float>(),
                               out_v.data_ptr<float>(), c10::hip::getCurrentHIPStream(dev.index()).stream()),
             "frg_densify_apply");
    return std::make_tuple(out, out_m, out_v);
}

void ResetOpacityHIP(torch::Tensor& raw_opacities, torch::Tensor& exp_avg, torch::Tensor& exp_avg_sq)
{
    TORCH_CHECK(raw_opacities.is_cuda(), "frosting_amd densify: tensors must live on a ROCm device (no CPU path)");
    const torch::Device dev = raw_opacities.device();
    const c10::hip::HIPGuard guard(dev.index());
    const int64_t P = raw_opacities.numel();
    check_on(raw_opacities, dev, torch::kFloat32, P, "raw_opacities");
    check_on(exp_avg, dev, torch::kFloat32, P, "exp_avg");
    check_on(exp_avg_sq, dev, torch::kFloat32, P, "exp_avg_sq");
    check_rc(frg_reset_opacity(static_cast<int>(P), raw_opacities.data_ptr<float>(), exp_avg.data_ptr<float>(),
                               exp_avg_sq.data_ptr<float>(), c10::hip::getCurrentHIPStream(dev.index()).stream()),
             "frg_reset_opacity");
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "MI355X-native Gaussian-splat rasterizer (hand-written gfx950 HIP behind include/frosting_rasterizer.h)";
    m.def("rasterize_gaussians", &RasterizeGaussiansHIP);
    m.def("rasterize_gaussians_backward", &RasterizeGaussiansBackwardHIP);
    m.def("mark_visible", &markVisibleHIP);
    m.def("rasterize_gaussians_masked", &RasterizeGaussiansMaskedHIP);
    m.def("rasterize_gaussians_forward_only", &RasterizeGaussiansForwardOnlyHIP);
    m.def("rasterize_gaussians_ex", &RasterizeGaussiansExHIP);
    m.def("rasterize_gaussians_backward_ex", &RasterizeGaussiansBackwardExHIP);
    m.def("rasterize_gaussians_rot", &RasterizeGaussiansRotHIP);
    m.def("rasterize_gaussians_backward_rot", &RasterizeGaussiansBackwardRotHIP);
    m.def("densify_accumulate", &DensifyAccumulateHIP);
    m.def("densify_accumulate_views", &DensifyAccumulateViewsHIP);
    m.def("densify_plan", &DensifyPlanHIP);
    m.def("densify_apply", &DensifyApplyHIP);
    m.def("reset_opacity", &ResetOpacityHIP);
    m.def("get_option", [](const std::string& name) { return frg_get_option(name.c_str()); });
    m.def("library_version", []() { return frg_version(); });
}
