"""Forward timings of rotated SH view directions (sh_rotations) on the C4 shape: 2 M shell Gaussians, 1600 x 1056, the
occlusion path's keep_mask, random rotations, forward_only.  One process, the variants interleaved round after round:
  a  the reference's route as a user takes it without the feature: sh.points_rgb with the rotation in torch on the device,
     then the colors_precomp forward (frosting_model.py:1478-1485)
  b  the fused call: shs + sh_rotations
  c  the unrotated SH forward (the call this library had before; run the same tool on the parent commit's library through
     FROSTING_LIB for the other half of the comparison -- the variants that need sh_rotations are then left out)
usage: python tools/time_sh_rotations.py [--points N] [--rounds 9] [--reps 20]"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from frosting_amd import _lib, mesh as M, scenes, sh

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=0)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
dev = torch.device("cuda:0")
shell, cam, bg = scenes.config_shell_scene("c4", 0, P=a.points or None)
shell, cam, bg = shell.to(dev), cam.to(dev), bg.to(dev)
sc = shell.scene
P, H, W = sc.P, cam.image_height, cam.image_width
keep = M.occlusion_keep_mask(shell.verts, shell.faces, cam.projmatrix, H, W, shell.cell)
g = torch.Generator().manual_seed(scenes.SEED_BASE + 40)
q = torch.nn.functional.normalize(torch.randn(P, 4, generator=g, dtype=torch.float64), dim=-1)
r, x, y, z = q.unbind(-1)
rot = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                   2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(P, 3, 3).float().to(dev)
e = torch.Tensor([])
fwd_only = {"forward_only": 1}
# Does the loaded library (FROSTING_LIB may name another build) know the fifth generation of frg_forward_args?  An empty struct
# of that size is refused either way, by one that does not know it for its struct_size.
_probe = _lib.ForwardArgs(struct_size=C.sizeof(_lib.ForwardArgs))
_lib.lib().frg_forward_ex(C.byref(_probe))
has_rot = "struct_size" not in _lib.last_error()
GENERATION_SIZE = C.sizeof(_lib.ForwardArgs) if has_rot else _lib.ForwardArgs.sh_rotations.offset     # fifth | fourth generation


color = torch.empty((3, H, W), device=dev)
radii = torch.empty((P,), dtype=torch.int32, device=dev)
chunks = [_lib.Scratch(dev, 1.25) for _ in range(3)]


def call(shs, colors, sh_rotations=None):
    """frg_forward_ex, the struct stated at the size of the generation the loaded library knows -> (R, image)"""
    args = _lib.forward_args(geometry_alloc=chunks[0].cb, binning_alloc=chunks[1].cb, image_alloc=chunks[2].cb, P=P, D=3, M=16, background=bg,
                             width=W, height=H, means3D=sc.means3D, shs=shs, colors_precomp=colors, opacities=sc.opacities, scales=sc.scales,
                             scale_modifier=1.0, rotations=sc.rotations, viewmatrix=cam.viewmatrix, projmatrix=cam.projmatrix, cam_pos=cam.campos,
                             tan_fovx=cam.tanfovx, tan_fovy=cam.tanfovy, out_color=color, radii=radii,
                             hip_stream=torch.cuda.current_stream(dev).cuda_stream, keep_mask=keep.contiguous(), modes=fwd_only,
                             sh_rotations=sh_rotations)
    args.struct_size = GENERATION_SIZE
    return _lib.check(_lib.lib().frg_forward_ex(C.byref(args)), "frg_forward_ex"), color


def route_a():
    with torch.no_grad():
        return call(e, sh.points_rgb(sc.means3D, sc.shs, cam.campos, 3, sh_rotations=rot))


variants = {"c unrotated shs": lambda: call(sc.shs, e)}
if has_rot:
    variants = {"a torch colours + colors_precomp": route_a, "b fused shs + sh_rotations": lambda: call(sc.shs, e, sh_rotations=rot), **variants}
print(f"C4 shape: P {P}, {W} x {H}, kept by the occlusion mask {int(keep.sum())}, library {_lib.LIB_PATH}", flush=True)
if has_rot:
    ia, ib = route_a()[1].clone(), variants["b fused shs + sh_rotations"]()[1].clone()
    print(f"image a against b: max abs difference {float((ia - ib).abs().max()):.3e}", flush=True)
for f in variants.values():
    for _ in range(10): f()
times = {k: [] for k in variants}
for _ in range(a.rounds):
    for k, f in variants.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.reps): f()
        torch.cuda.synchronize(); times[k].append(1e3 * (time.perf_counter() - t0) / a.reps)
for k, t in times.items():
    print(f"[{k:34s}] median {np.median(t):.4f} ms  min {min(t):.4f}  max {max(t):.4f}  over {a.rounds} rounds of {a.reps}", flush=True)
