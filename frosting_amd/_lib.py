"""ctypes binding of libfrosting_rasterizer.so (include/frosting_rasterizer.h).

There is no fallback: if the HIP library is missing or cannot be loaded the
import-time / first-use error is fatal by design (a silent CPU or eager path
would void every parity and performance claim).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# FROSTING_LIB: another build of the same library (A/B timing of kernel variants in one GPU session; tools/ab.py)
LIB_PATH = os.environ.get("FROSTING_LIB") or os.path.join(_PKG, "lib", "libfrosting_rasterizer.so")
CSRC = os.path.join(_PKG, "csrc")

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
ECAPACITY = -5

_lib = None


class ForwardArgs(C.Structure):
    """frg_forward_args (include/frosting_rasterizer.h)."""
    _fields_ = [("struct_size", C.c_size_t),
                ("geometry_alloc", ALLOC_FN), ("binning_alloc", ALLOC_FN), ("image_alloc", ALLOC_FN),
                ("user", C.c_void_p),
                ("P", C.c_int), ("D", C.c_int), ("M", C.c_int),
                ("background", C.c_void_p),
                ("width", C.c_int), ("height", C.c_int),
                ("means3D", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p),
                ("opacities", C.c_void_p), ("scales", C.c_void_p),
                ("scale_modifier", C.c_float),
                ("rotations", C.c_void_p), ("cov3D_precomp", C.c_void_p), ("viewmatrix", C.c_void_p),
                ("projmatrix", C.c_void_p), ("cam_pos", C.c_void_p),
                ("tan_fovx", C.c_float), ("tan_fovy", C.c_float),
                ("prefiltered", C.c_int),
                ("out_color", C.c_void_p), ("radii", C.c_void_p),
                ("debug", C.c_int),
                ("hip_stream", C.c_void_p),
                ("instance_capacity", C.c_int),
                ("keep_mask", C.c_void_p),
                # raw-parameter mode (activations and the shell gather inside the per-Gaussian kernels)
                ("raw_opacities", C.c_void_p), ("raw_scales", C.c_void_p), ("raw_rotations", C.c_void_p),
                ("shell_logits", C.c_void_p), ("shell_cell_verts", C.c_void_p), ("shell_cells", C.c_void_p),
                # per-call modes: 0 = the process-wide frg_set_option value, k + 1 = value k for this call
                ("exact_blend", C.c_int), ("tight_binning", C.c_int), ("async_sh", C.c_int),
                ("shell_bary_mode", C.c_int),
                # no backward will follow: nothing is kept for one
                ("forward_only", C.c_int),
                # optional [P,3,3] (with shs): the SH colour of Gaussian i is evaluated at d @ R_i
                ("sh_rotations", C.c_void_p)]


def mode_fields(modes) -> dict:
    """{'exact_blend': 0|1, 'tight_binning': 0|1, 'async_sh': 0..3} (any subset, or None) -> the per-call mode fields
    of frg_forward_args (0 = process default, k + 1 = value k)."""
    out = {"exact_blend": 0, "tight_binning": 0, "async_sh": 0}
    forward_only = 0
    for k, v in (modes or {}).items():
        if k == "forward_only":          # a plain 0 | 1 field, no process-wide form
            forward_only = int(bool(v))
            continue
        if k not in out:
            raise KeyError(f"unknown per-call mode '{k}'")
        out[k] = int(v) + 1
    out["forward_only"] = forward_only
    return out


class BackwardArgs(C.Structure):
    """frg_backward_args (include/frosting_rasterizer.h)."""
    _fields_ = [("struct_size", C.c_size_t),
                ("P", C.c_int), ("D", C.c_int), ("M", C.c_int), ("R", C.c_int),
                ("background", C.c_void_p),
                ("width", C.c_int), ("height", C.c_int),
                ("means3D", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p), ("scales", C.c_void_p),
                ("scale_modifier", C.c_float),
                ("rotations", C.c_void_p), ("cov3D_precomp", C.c_void_p), ("viewmatrix", C.c_void_p),
                ("projmatrix", C.c_void_p), ("campos", C.c_void_p),
                ("tan_fovx", C.c_float), ("tan_fovy", C.c_float),
                ("radii", C.c_void_p),
                ("geom_buffer", C.c_void_p), ("binning_buffer", C.c_void_p), ("image_buffer", C.c_void_p),
                ("dL_dpix", C.c_void_p),
                ("dL_dmean2D", C.c_void_p), ("dL_dconic", C.c_void_p), ("dL_dopacity", C.c_void_p), ("dL_dcolor", C.c_void_p),
                ("dL_dmean3D", C.c_void_p), ("dL_dcov3D", C.c_void_p), ("dL_dsh", C.c_void_p), ("dL_dscale", C.c_void_p),
                ("dL_drot", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("debug", C.c_int),
                ("hip_stream", C.c_void_p),
                ("raw_opacities", C.c_void_p), ("raw_scales", C.c_void_p), ("raw_rotations", C.c_void_p),
                ("shell_logits", C.c_void_p), ("shell_cell_verts", C.c_void_p), ("shell_cells", C.c_void_p),
                ("dL_dshell_logits", C.c_void_p), ("dL_dshell_cell_verts", C.c_void_p),
                ("exact_blend", C.c_int), ("shell_bary_mode", C.c_int),
                # the backward in two calls: 1 = blend + slot sums (dL_dcolor complete), 2 = the rest; 0 = one call
                ("phase", C.c_int),
                # optional [P] bytes: 1 = the Gaussian has a gradient; the rows of the others are then not written
                ("row_live", C.c_void_p),
                # phase 1 in pieces: Gaussians [range_first, + range_count) (range_count 0: the whole phase)
                ("range_first", C.c_int), ("range_count", C.c_int),
                # the forward's sh_rotations (NULL exactly when it had none)
                ("sh_rotations", C.c_void_p)]


class CombineArgs(C.Structure):
    """frg_combine_args (include/frosting_rasterizer.h)."""
    _fields_ = [("struct_size", C.c_size_t),
                ("P", C.c_int), ("first", C.c_int), ("count", C.c_int), ("n_views", C.c_int),
                ("packets", C.c_void_p),
                ("packet_stride_bytes", C.c_size_t),
                ("capacity_rows", C.c_longlong),
                ("M", C.c_int),
                ("means3D", C.c_void_p), ("shs", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p), ("opacities", C.c_void_p),
                ("raw_opacities", C.c_void_p), ("raw_scales", C.c_void_p), ("raw_rotations", C.c_void_p),
                ("dL_dmean3D", C.c_void_p), ("dL_dscale", C.c_void_p), ("dL_drot", C.c_void_p), ("dL_dopacity", C.c_void_p),
                ("dL_dsh", C.c_void_p),
                ("status", C.c_void_p),
                ("status_seq", C.c_uint),
                ("row_live", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("hip_stream", C.c_void_p)]


class PackSumArgs(C.Structure):
    """frg_pack_sum_args (include/frosting_rasterizer.h)."""
    _fields_ = [("struct_size", C.c_size_t),
                ("P", C.c_int), ("R", C.c_int), ("first", C.c_int), ("count", C.c_int),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("drgb_masked", C.c_void_p), ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p),
                ("tan_fovx", C.c_float), ("tan_fovy", C.c_float),
                ("width", C.c_int), ("height", C.c_int),
                ("scale_modifier", C.c_float),
                ("D", C.c_int),
                ("packet", C.c_void_p), ("packet_bytes", C.c_size_t),
                ("capacity_rows", C.c_longlong),
                ("radii", C.c_void_p),
                ("hip_stream", C.c_void_p)]


class DensifyViewsArgs(C.Structure):
    """frg_densify_views_args (include/frosting_rasterizer.h)."""
    _fields_ = [("struct_size", C.c_size_t),
                ("P", C.c_int), ("first", C.c_int), ("count", C.c_int), ("n_views", C.c_int),
                ("packets", C.c_void_p),
                ("packet_stride_bytes", C.c_size_t),
                ("capacity_rows", C.c_longlong),
                ("means3D", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p), ("opacities", C.c_void_p),
                ("raw_opacities", C.c_void_p), ("raw_scales", C.c_void_p), ("raw_rotations", C.c_void_p),
                ("xyz_gradient_accum", C.c_void_p), ("denom", C.c_void_p), ("max_radii2D", C.c_void_p),
                ("status", C.c_void_p),
                ("status_seq", C.c_uint),
                ("hip_stream", C.c_void_p)]


class DensifyParams(C.Structure):
    """frg_densify_params (include/frosting_rasterizer.h)."""
    _fields_ = [("struct_size", C.c_size_t),
                ("max_grad", C.c_double), ("min_opacity", C.c_double), ("extent", C.c_double), ("percent_dense", C.c_double),
                ("prune_big_points", C.c_int)]


class FieldArgs(C.Structure):
    """frg_field_args (include/frosting_rasterizer.h)."""
    _fields_ = [("struct_size", C.c_size_t),
                ("P", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("idx_is_int64", C.c_int),
                ("idx", C.c_void_p),
                ("x", C.c_void_p), ("points", C.c_void_p), ("scaling", C.c_void_p), ("quaternions", C.c_void_p), ("strengths", C.c_void_p),
                ("beta_mode", C.c_int),
                ("flags", C.c_int),
                ("density_threshold", C.c_double), ("density_factor", C.c_double), ("opacity_min_clamp", C.c_double),
                ("beta_fallback", C.c_void_p),
                ("density", C.c_void_p), ("opacities", C.c_void_p), ("beta", C.c_void_p), ("sdf", C.c_void_p),
                ("dL_ddensity", C.c_void_p), ("dL_dopacities", C.c_void_p), ("dL_dbeta", C.c_void_p), ("dL_dsdf", C.c_void_p),
                ("dL_dx", C.c_void_p), ("dL_dpoints", C.c_void_p), ("dL_dscaling", C.c_void_p), ("dL_dquaternions", C.c_void_p),
                ("dL_dstrengths", C.c_void_p),
                ("bad_index", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("hip_stream", C.c_void_p)]


class LevelsetArgs(C.Structure):
    """frg_levelset_args (include/frosting_rasterizer.h)."""
    _fields_ = [("struct_size", C.c_size_t),
                ("P", C.c_int), ("R", C.c_int), ("K", C.c_int), ("n", C.c_int), ("L", C.c_int),
                ("idx_is_int64", C.c_int),
                ("inner_mode", C.c_int),
                ("idx", C.c_void_p),
                ("origins", C.c_void_p), ("directions", C.c_void_p), ("t_scale", C.c_void_p), ("t_offset", C.c_void_p), ("lin", C.c_void_p),
                ("points", C.c_void_p), ("scaling", C.c_void_p), ("quaternions", C.c_void_p), ("strengths", C.c_void_p),
                ("levels", C.c_double * 8),
                ("density_factor", C.c_double),
                ("densities", C.c_void_p), ("t_outer", C.c_void_p), ("t_inner", C.c_void_p),
                ("first_above", C.c_void_p), ("last_above", C.c_void_p),
                ("under_first", C.c_void_p),
                ("normals", C.c_void_p),
                ("bad_index", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("hip_stream", C.c_void_p)]


# The parameters of the reference-shaped entry points are fields of the structs: their positional order, written once.
# (argtypes of the functions and the arguments of a call are both derived from it.)
FORWARD_POSITIONAL = [name for name, _ in ForwardArgs._fields_[1:ForwardArgs._fields_.index(("hip_stream", C.c_void_p)) + 1]]
# frg_forward_deferred: the same list, instance_capacity in the place of debug
FORWARD_DEFERRED_POSITIONAL = ["instance_capacity" if name == "debug" else name for name in FORWARD_POSITIONAL]
BACKWARD_POSITIONAL = [name for name, _ in BackwardArgs._fields_[1:BackwardArgs._fields_.index(("hip_stream", C.c_void_p)) + 1]]


_FIELD_NAMES = {cls: frozenset(name for name, _ in cls._fields_) for cls in (ForwardArgs, BackwardArgs)}


def _args(cls, fields):
    if "modes" in fields:
        fields.update(mode_fields(fields.pop("modes")))
    unknown = fields.keys() - _FIELD_NAMES[cls]
    if unknown:
        raise TypeError(f"{cls.__name__} has no field {sorted(unknown)}")
    tensors = []
    for name, value in fields.items():
        if isinstance(value, torch.Tensor):
            tensors.append(value)
            fields[name] = value.data_ptr() if value.numel() else None
    a = cls(struct_size=C.sizeof(cls), **fields)
    a.tensors = tensors        # what the pointers point into lives as long as the struct does
    return a


def forward_args(**fields) -> ForwardArgs:
    """A filled frg_forward_args.  Pointer fields take a tensor, None or the reference's 'absent' encoding (an empty
    tensor, DGR/diff_gaussian_rasterization/__init__.py:197-207); modes= takes what mode_fields takes.  The struct keeps
    every tensor it points into referenced (and, through its callback fields, the scratch chunks)."""
    return _args(ForwardArgs, fields)


def backward_args(**fields) -> BackwardArgs:
    """A filled frg_backward_args; pointer fields and lifetimes as in forward_args."""
    return _args(BackwardArgs, fields)


def positional(a, order) -> list:
    """The fields of a filled struct as the arguments of the reference-shaped function with that parameter order."""
    return [getattr(a, name) for name in order]


def ptr(t):
    """Device pointer of a tensor as a ctypes argument; NULL for None and for the reference's 'absent' encoding (an empty tensor)."""
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def check(rc: int, what: str) -> int:
    if rc < 0:
        raise RuntimeError(f"{what} failed ({rc}): {last_error()}")
    return rc


class Scratch:
    """A device buffer grown through the C ABI's allocation callbacks (.cb) or by ensure(): reallocated, `slack` times the
    size asked for, when it is too small.  slack 1.0: the per-call chunks of the reference binding
    (rasterize_points.cu:27-33,71-78); 1.25: a grow-only arena -- after the first view no allocator call remains on the
    per-step path (image size and P are constant per model, only R varies -- SURVEY Appendix A-18).
    The callback holds the tensor's holder, not this object: nothing here forms a cycle, the memory goes with the last reference."""

    def __init__(self, device, slack: float = 1.0):
        self._held = held = [torch.empty(0, dtype=torch.uint8, device=device)]

        def alloc(_user, nbytes):
            if held[0].numel() < max(nbytes, 1):
                held[0] = torch.empty(int(nbytes * slack) + 256, dtype=torch.uint8, device=device)
            return held[0].data_ptr()

        self._alloc = alloc
        self.cb = ALLOC_FN(alloc)

    @property
    def buf(self):
        return self._held[0]

    @buf.setter
    def buf(self, tensor):
        self._held[0] = tensor

    def ensure(self, nbytes):
        self._alloc(None, nbytes)
        return self.buf


def build(verbose: bool = False) -> str:
    """Compile every HIP translation unit for gfx950 (hipcc cross-compiles on CPU-only hosts)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", CSRC, "-j8"], stdout=out)
    return LIB_PATH


class RasterizerLibraryError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RasterizerLibraryError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            f"or make -C {CSRC}).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    L.frg_version.restype = i
    L.frg_last_error.restype = C.c_char_p
    L.frg_set_option.argtypes = [C.c_char_p, i]
    L.frg_get_option.argtypes = [C.c_char_p]
    L.frg_geometry_bytes.restype = sz
    L.frg_geometry_bytes.argtypes = [i]
    L.frg_image_bytes.restype = sz
    L.frg_image_bytes.argtypes = [i, i]
    L.frg_binning_bytes.restype = sz
    L.frg_binning_bytes.argtypes = [i, i]
    L.frg_backward_workspace_bytes.restype = sz
    L.frg_backward_workspace_bytes.argtypes = [i, i]
    L.frg_geometry_layout.argtypes = [i, vp]
    if hasattr(L, "frg_geometry_layout_n"):        # (absent from a version-1 library loaded through FROSTING_LIB for an A/B)
        L.frg_geometry_layout_n.restype = i
        L.frg_geometry_layout_n.argtypes = [i, vp, i]
    L.frg_image_layout.argtypes = [i, i, vp]
    L.frg_binning_layout.argtypes = [i, i, vp]
    L.frg_mark_visible.restype = i
    L.frg_mark_visible.argtypes = [i, vp, vp, vp, vp, vp]
    L.frg_forward.restype = i
    L.frg_forward.argtypes = [dict(ForwardArgs._fields_)[name] for name in FORWARD_POSITIONAL]
    L.frg_forward_deferred.restype = i
    L.frg_forward_deferred.argtypes = [dict(ForwardArgs._fields_)[name] for name in FORWARD_DEFERRED_POSITIONAL]
    L.frg_knn_workspace_bytes.restype = sz
    L.frg_knn_workspace_bytes.argtypes = [i]
    L.frg_knn_mean_dist2.restype = i
    L.frg_knn_mean_dist2.argtypes = [i, vp, vp, vp, sz, vp]
    if hasattr(L, "frg_knn_points"):              # (absent from an older library loaded through FROSTING_LIB for an A/B)
        L.frg_knn_points_workspace_bytes.restype = sz
        L.frg_knn_points_workspace_bytes.argtypes = [i, i, i]
        L.frg_knn_points.restype = i
        L.frg_knn_points.argtypes = [i, vp, i, vp, i, vp, vp, vp, sz, vp]
    L.frg_shell_points.restype = i
    L.frg_shell_points.argtypes = [i, vp, vp, vp, vp, vp]
    L.frg_shell_points_backward.restype = i
    L.frg_shell_points_backward.argtypes = [i, vp, vp, vp, vp, vp, vp]
    L.frg_activate.restype = i
    L.frg_activate.argtypes = [i, vp, vp, vp, vp, vp, vp, vp]
    L.frg_activate_backward.restype = i
    L.frg_activate_backward.argtypes = [i, vp, vp, vp, vp, vp, vp, vp]
    L.frg_photometric_workspace_bytes.restype = sz
    L.frg_photometric_workspace_bytes.argtypes = [i, i, i]
    L.frg_photometric_loss.restype = i
    L.frg_photometric_loss.argtypes = [i, i, i, vp, vp, C.POINTER(C.c_float), f, vp, vp, vp, sz, vp]
    L.frg_adam_step.restype = i
    L.frg_adam_step.argtypes = [C.c_longlong, vp, vp, vp, vp, C.POINTER(C.c_longlong), C.POINTER(C.c_float),
                                C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), i,
                                C.c_double, C.c_double, C.c_double, i, f, vp]
    L.frg_forward_ex.restype = i
    L.frg_forward_ex.argtypes = [C.POINTER(ForwardArgs)]
    L.frg_backward_ex.restype = i
    L.frg_backward_ex.argtypes = [C.POINTER(BackwardArgs)]
    L.frg_forward_finish.restype = i
    L.frg_forward_finish.argtypes = [vp, i, C.POINTER(C.c_int)]
    L.frg_backward.restype = i
    L.frg_backward.argtypes = [dict(BackwardArgs._fields_)[name] for name in BACKWARD_POSITIONAL]
    L.frg_stage_times.restype = i
    L.frg_stage_times.argtypes = [vp, i]
    L.frg_mesh_raster_workspace_bytes.restype = sz
    L.frg_mesh_raster_workspace_bytes.argtypes = [i, i, i]
    L.frg_mesh_rasterize.restype = i
    L.frg_mesh_rasterize.argtypes = [i, i, vp, vp, i, i, vp, vp, sz, vp]
    L.frg_mesh_occlusion_workspace_bytes.restype = sz
    L.frg_mesh_occlusion_workspace_bytes.argtypes = [i, i, i, i]
    L.frg_mesh_occlusion_mask.restype = i
    L.frg_mesh_occlusion_mask.argtypes = [i, i, vp, vp, vp, i, i, i, vp, i, vp, vp, vp, sz, vp]
    if hasattr(L, "frg_mesh_visible_faces"):
        L.frg_mesh_visible_faces.restype = i
        L.frg_mesh_visible_faces.argtypes = [i, i, vp, vp, i, i, vp, vp, sz, vp]
    L.frg_sh_color_grad.restype = i
    L.frg_sh_color_grad.argtypes = [i, vp, vp, vp, vp, vp]
    L.frg_sh_grad_from_views.restype = i
    L.frg_sh_grad_from_views.argtypes = [i, i, i, i, vp, vp, C.c_longlong, vp, C.c_longlong, vp, vp]
    L.frg_adam_step_shard.restype = i
    L.frg_adam_step_shard.argtypes = [C.c_longlong, C.c_longlong, vp, vp, vp, vp, C.POINTER(C.c_longlong), C.POINTER(C.c_float),
                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), i,
                                      C.c_double, C.c_double, C.c_double, i, f, vp]
    L.frg_adam_step_rows.restype = i
    L.frg_adam_step_rows.argtypes = [C.c_longlong, vp, vp, vp, vp, C.POINTER(C.c_longlong), C.POINTER(C.c_float),
                                     C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), i,
                                     C.c_double, C.c_double, C.c_double, i, f, vp, i, C.POINTER(C.c_int), vp]
    L.frg_pack_grad_rows.restype = i
    L.frg_pack_grad_rows.argtypes = [i, vp, vp, vp, vp, vp, vp, C.c_longlong, vp, vp]
    L.frg_scatter_grad_rows.restype = i
    L.frg_scatter_grad_rows.argtypes = [C.c_longlong, i, vp, vp, vp, vp, vp, vp, vp]
    L.frg_sum_packet_bytes.restype = sz
    L.frg_sum_packet_bytes.argtypes = [i, C.c_longlong]
    L.frg_pack_sum_rows.restype = i
    L.frg_pack_sum_rows.argtypes = [i, i, i, i, vp, sz, vp, vp, vp, vp, f, f, i, i, f, i, vp, sz, C.c_longlong, vp]
    L.frg_combine_workspace_bytes.restype = sz
    L.frg_combine_workspace_bytes.argtypes = [i, C.c_longlong]
    L.frg_backward_combine.restype = i
    L.frg_backward_combine.argtypes = [C.POINTER(CombineArgs)]
    if hasattr(L, "frg_densify_plan"):            # (absent from an older library loaded through FROSTING_LIB for an A/B)
        L.frg_densify_accumulate.restype = i
        L.frg_densify_accumulate.argtypes = [i, vp, vp, vp, vp, vp, vp, vp]
        L.frg_densify_workspace_bytes.restype = sz
        L.frg_densify_workspace_bytes.argtypes = [i]
        L.frg_densify_plan.restype = i
        L.frg_densify_plan.argtypes = [i, vp, vp, vp, vp, C.POINTER(DensifyParams), vp, vp, vp, sz, vp]
        L.frg_densify_apply.restype = i
        L.frg_densify_apply.argtypes = [i, i, vp, i, C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                        C.c_longlong, vp, vp, vp, vp, vp, vp, vp, vp]
        L.frg_reset_opacity.restype = i
        L.frg_reset_opacity.argtypes = [i, vp, vp, vp, vp]
    if hasattr(L, "frg_densify_accumulate_views"):
        L.frg_sum_packet_bytes_ex.restype = sz
        L.frg_sum_packet_bytes_ex.argtypes = [i, C.c_longlong, i]
        L.frg_pack_sum_rows_ex.restype = i
        L.frg_pack_sum_rows_ex.argtypes = [C.POINTER(PackSumArgs)]
        L.frg_densify_accumulate_views.restype = i
        L.frg_densify_accumulate_views.argtypes = [C.POINTER(DensifyViewsArgs)]
    if hasattr(L, "frg_field_forward"):           # (absent from an older library loaded through FROSTING_LIB for an A/B)
        L.frg_field_workspace_bytes.restype = sz
        L.frg_field_workspace_bytes.argtypes = [i, i, i, i]
        L.frg_field_forward.restype = i
        L.frg_field_forward.argtypes = [C.POINTER(FieldArgs)]
        L.frg_field_backward.restype = i
        L.frg_field_backward.argtypes = [C.POINTER(FieldArgs)]
    if hasattr(L, "frg_levelset"):
        L.frg_levelset_workspace_bytes.restype = sz
        L.frg_levelset_workspace_bytes.argtypes = [i, i, i, i]
        L.frg_levelset.restype = i
        L.frg_levelset.argtypes = [C.POINTER(LevelsetArgs)]
    _lib = L
    return L


def build_fingerprint() -> dict:
    """What identifies the kernels a measurement was taken with: sha256 over the kernel sources (csrc/*.hip, *.h, the
    Makefile and the public header, sorted by name -- the same wherever the tree is checked out) and over the loaded
    library file.  tools/collect_traffic.py stores it beside the PMC figures; bench.py only quotes figures whose
    source hash is that of the running tree."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")) or f == "Makefile")
    for f in files:
        h.update(f.encode())
        h.update(open(os.path.join(CSRC, f), "rb").read())
    h.update(open(os.path.join(os.path.dirname(_PKG), "include", "frosting_rasterizer.h"), "rb").read())
    lib_sha = hashlib.sha256(open(LIB_PATH, "rb").read()).hexdigest() if os.path.exists(LIB_PATH) else None
    return {"kernel_sources_sha256": h.hexdigest(), "library_sha256": lib_sha}


def last_error() -> str:
    return lib().frg_last_error().decode("utf-8", "replace")


def set_option(name: str, value: int) -> int:
    return lib().frg_set_option(name.encode(), int(value))


def get_option(name: str) -> int:
    return lib().frg_get_option(name.encode())


STAGE_NAMES = ["preprocess", "scan", "scatter", "sort", "blend_fwd", "blend_bwd", "preprocess_bwd", "sh_color"]


def stage_times() -> dict:
    """Milliseconds per stage of the last forward/backward (needs set_option('profile', 1))."""
    buf = (C.c_float * 16)()
    n = lib().frg_stage_times(buf, 16)
    return {STAGE_NAMES[k]: float(buf[k]) for k in range(min(n, len(STAGE_NAMES)))}


EXPORTED_SYMBOLS = [
    "frg_version", "frg_last_error", "frg_mark_visible", "frg_forward", "frg_backward_workspace_bytes",
    "frg_backward", "frg_set_option", "frg_get_option", "frg_stage_times", "frg_geometry_bytes", "frg_image_bytes",
    "frg_binning_bytes", "frg_geometry_layout", "frg_geometry_layout_n", "frg_image_layout", "frg_binning_layout",
    "frg_mesh_raster_workspace_bytes", "frg_mesh_rasterize", "frg_mesh_visible_faces", "frg_mesh_occlusion_workspace_bytes", "frg_mesh_occlusion_mask", "frg_sh_color_grad", "frg_sh_grad_from_views",
    "frg_pack_grad_rows", "frg_scatter_grad_rows", "frg_adam_step_rows", "frg_adam_step_shard",
    "frg_sum_packet_bytes", "frg_pack_sum_rows", "frg_combine_workspace_bytes", "frg_backward_combine",
    "frg_forward_deferred", "frg_forward_finish", "frg_forward_ex", "frg_backward_ex", "frg_adam_step",
    "frg_photometric_workspace_bytes", "frg_photometric_loss", "frg_activate", "frg_activate_backward",
    "frg_knn_workspace_bytes", "frg_knn_mean_dist2", "frg_shell_points", "frg_shell_points_backward",
    "frg_densify_accumulate", "frg_densify_workspace_bytes", "frg_densify_plan", "frg_densify_apply", "frg_reset_opacity",
    "frg_sum_packet_bytes_ex", "frg_pack_sum_rows_ex", "frg_densify_accumulate_views",
    "frg_knn_points_workspace_bytes", "frg_knn_points",
    "frg_field_workspace_bytes", "frg_field_forward", "frg_field_backward",
    "frg_levelset_workspace_bytes", "frg_levelset",
]
