"""What one looks at after a run, on the HIP path: turntable spins of a mesh (reference src/vis/mesh_turntable.py:27-68), the per-vertex
Chamfer heat maps of src/eval/eval_3d.py:171-189 and OBJ export in the layout of trimesh's export_obj (eval_3d.py:204-217,
src/train/trainer.py:260-296).

A spin is ONE kind of render call.  Upstream rotates the mesh about world z by theta and renders it with a fixed camera (R0, T0):
X = verts @ Rz(theta), then X @ R0 + T0 -- 250 single-image calls per spin.  FootRenderer's only light, PointLights((0, 0, 100)), lies ON the
rotation axis, so the rotated mesh under the fixed camera is exactly the still mesh under the cameras R_i = Rz(theta_i) @ R0, T_i = T0:
  diffuse   (n Rz) . (L - v Rz) = n . (L Rz^T - v) = n . (L - v)          (L Rz^T = L for L on the z axis)
  specular  the camera centre -T0 R0^T becomes -T0 R0^T Rz^T: the view vector turns with the mesh.
turntable_views makes those cameras and turntable hands them to the renderer `views_per_call` at a time; each chunk's float images become
bytes on the device (functional.frames_u8) before the next is rendered, so a spin never holds more than one chunk of float frames."""
import math
import os
import warnings

import numpy as np
import torch

from . import functional as FN
from .renderer import FootRenderer
from .structures import TexturesVertex

MAX_COL = 30e-6   # eval_3d.py:180 (its comment says 50 um; the number is what the heat maps are drawn with)
PIL_FORMATS = ('.gif', '.png', '.webp')


def turntable_views(renderer, nframes=250, azim=-90, dist=0.3):
	"""The cameras of a spin: R (nframes,3,3), T (nframes,3) with p @ R_i + T_i == (p @ Rz(theta_i)) @ R0 + T0, where (R0, T0) =
	renderer.linspace_views(nviews=1, dist=dist, azim_min=azim, azim_max=azim), theta = torch.linspace(0, 2 pi, nframes) in float32 (both
	ends included, as upstream: the first and the last frame show the same pose) and Rz(theta) = euler_angles_to_matrix([0, 0, theta],
	'XYZ') in the row-vector convention of the registration.  The product is formed in float64 and rounded once."""
	R0, T0 = renderer.linspace_views(nviews=1, dist=dist, azim_min=azim, azim_max=azim)
	theta = torch.linspace(0, 2 * math.pi, nframes, dtype=torch.float32).double()
	c, s = torch.cos(theta), torch.sin(theta)
	Rz = torch.zeros(nframes, 3, 3, dtype=torch.float64)
	Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = c, -s, s, c, 1.0
	R = (Rz @ R0[0].double()).float()
	return R, T0.float().expand(nframes, 3).contiguous()


def _writer(out_loc, fps):
	"""The function that writes uint8 frames (n,H,W,3) (a numpy array) to out_loc, chosen by its extension; raises for one that cannot be
	written here -- before anything is rendered."""
	ext = os.path.splitext(out_loc)[1].lower()
	if ext == '.npy':
		return lambda frames: np.save(out_loc, frames)
	if ext in PIL_FORMATS:
		def write(frames):
			from PIL import Image
			imgs = [Image.fromarray(f) for f in frames]
			imgs[0].save(out_loc, save_all=True, append_images=imgs[1:], duration=1000 / fps, loop=0)
		return write
	if ext == '.mp4':
		try:
			import imageio
			return lambda frames: imageio.mimwrite(out_loc, list(frames), fps=fps)
		except ImportError:
			pass
	raise RuntimeError(f'find_amd.vis.turntable: cannot write {out_loc!r}' + (' (.mp4 needs imageio, which is not installed)' if ext == '.mp4' else '')
					   + f'; formats that work here: .npy, {", ".join(PIL_FORMATS)}' + ('' if ext == '.mp4' else ', .mp4 with imageio'))


def turntable(mesh, out_loc=None, image_size=256, nframes=250, fps=25, silent=False, azim=-90, dist=0.3, views_per_call=50, device=None):
	"""One full turn of `mesh` about world z, as reference mesh_turntable.turntable renders it: torch.uint8 frames (nframes, H, W, 3) on the
	device, each cv2.rotate(ROTATE_180) of (255 * image).astype(uint8); written to out_loc when given (.npy the array; .gif, .png (APNG)
	and .webp through PIL with duration = 1000 / fps; .mp4 through imageio where it is installed).  TexturesVertex and TexturesUV meshes both
	work; only the first mesh of a batch is rendered (a warning says so, as upstream's print).  The views go to the renderer
	`views_per_call` at a time (at most 256, the rasteriser's limit); the frames do not depend on that choice, the default is a measured
	one (250 frames at 512^2 take 3.3 ms in calls of 50 and 2.8 ms in one call, which holds 4.7 GB more).  A CPU mesh raises:
	there is no CPU fallback.
	azim = -90 is upstream's default and is kept, but it is no useful one: with FIND's "up = world x" the camera of azim = -90, elev = 0 looks
	along the up vector, the look-at frame is degenerate and nothing is drawn (by rotated vertices or rotated views alike).  eval_3d passes
	azim=70, dist=0.35."""
	write = None if out_loc is None else _writer(out_loc, fps)
	if mesh.device.type != 'cuda':
		raise RuntimeError('find_amd.vis.turntable: the HIP path needs a mesh on a ROCm device (got a CPU mesh); there is no CPU fallback')
	if device is not None and torch.device(device).type != 'cuda':
		raise RuntimeError(f'find_amd.vis.turntable: device {device!r} is no ROCm device; there is no CPU fallback')
	if nframes < 1 or not 1 <= views_per_call <= 256:
		raise ValueError(f'find_amd.vis.turntable: nframes >= 1 and 1 <= views_per_call <= 256 expected, got {nframes} / {views_per_call}')
	if len(mesh) > 1:
		warnings.warn('More than 1 mesh given to turntable - only rendering first mesh...')
		mesh = mesh[0]
	if device is not None:
		mesh = mesh.to(device)
	dev = mesh.device
	renderer = FootRenderer(image_size=image_size, device=dev)
	R, T = turntable_views(renderer, nframes=nframes, azim=azim, dist=dist)
	R, T = R.to(dev), T.to(dev)
	frames = None
	with torch.no_grad():
		for a in range(0, nframes, views_per_call):
			image = renderer(mesh, R[a:a + views_per_call], T[a:a + views_per_call])['image'][0]
			if frames is None:
				frames = torch.empty((nframes,) + tuple(image.shape[1:]), dtype=torch.uint8, device=dev)
			FN.frames_u8(image, rot180=True, out=frames[a:a + image.shape[0]])
	if write is not None:
		write(frames.cpu().numpy())
		if not silent:
			print(f'Video written to {out_loc}')
	return frames


def vertex_errors(pred_verts, gt_verts, pred_samples, gt_lengths=None):
	"""Per-vertex squared distances behind the Chamfer heat maps (eval_3d.py:171-178): (pred_err (N,V), gt_err (N,Vg_max)).
	pred_err: every predicted vertex to its nearest GT vertex; gt_err: every GT vertex to its nearest predicted SAMPLE (pred_samples
	(N,S,3): upstream takes the surface samples on purpose, for models of few vertices).  gt_verts (N,Vg_max,3) is padded, gt_lengths (N)
	its vertex counts (None: all Vg_max); padded rows are not read as targets, and their gt_err entries are 0."""
	lens = None if gt_lengths is None else torch.as_tensor(gt_lengths, device=gt_verts.device).to(torch.int32)
	with torch.no_grad():
		pred_err, _ = FN.knn1(pred_verts.detach(), gt_verts.detach(), None, lens)
		gt_err, _ = FN.knn1(gt_verts.detach(), pred_samples.detach(), lens, None)
	return pred_err, gt_err


def surface_errors(pred_meshes, gt_meshes):
	"""Per-vertex squared distances to the other SURFACE (losses.point_mesh_distance), the exact counterpart of vertex_errors:
	(pred_err (N,V), gt_err (N,Vg_max)); padded rows are 0."""
	from .losses import point_mesh_distance
	with torch.no_grad():
		pred_err, _, _ = point_mesh_distance(pred_meshes.verts_padded().detach(), gt_meshes, pred_meshes.num_verts_per_mesh())
		gt_err, _, _ = point_mesh_distance(gt_meshes.verts_padded().detach(), pred_meshes, gt_meshes.num_verts_per_mesh())
	return pred_err, gt_err


def error_colours(err, max_col=MAX_COL):
	"""(..., 3) heat-map colours of squared distances: red = clamp(err / max_col, 0, 1), green = blue = 0 (eval_3d.py:180-187).  An error of
	max_col or more is exactly 1 (torch divides by a Python number as a product with its reciprocal, which may fall one ulp short)."""
	top = torch.full((), max_col, dtype=err.dtype, device=err.device)
	col = torch.zeros(tuple(err.shape) + (3,), dtype=err.dtype, device=err.device)
	col[..., 0] = torch.where(err >= top, torch.ones_like(err), torch.clamp(err / top, min=0, max=1))
	return col


def export_obj(mesh, loc, idx=0, include_colour=True):
	"""Mesh `idx` of `mesh` as a Wavefront OBJ in the layout of trimesh's export_obj: `v x y z r g b` lines for a vertex-coloured mesh
	(`v x y z` for a UV-textured or untextured one, or with include_colour=False), then `f a b c`, 1-based.  Every float is written with
	%.9g, so float32 values read back bit for bit (read_obj_colours)."""
	n = mesh._num_verts[idx]
	verts = mesh.verts_padded()[idx, :n].detach().cpu().numpy().astype(np.float32)
	faces = mesh.faces_list()[idx].detach().cpu().numpy().astype(np.int64) + 1
	cols = None
	if include_colour and isinstance(mesh.textures, TexturesVertex):
		cols = mesh.textures.verts_features_padded()[idx, :n, :3].detach().cpu().numpy().astype(np.float32)
	rows = verts if cols is None else np.concatenate([verts, cols], axis=1)
	lines = ['v ' + ' '.join('%.9g' % x for x in row) for row in rows.tolist()]
	lines += ['f %d %d %d' % tuple(f) for f in faces.tolist()]
	with open(loc, 'w') as fh:
		fh.write('\n'.join(lines) + '\n')
	return loc


def read_obj_colours(loc):
	"""(verts (V,3) float32, colours (V,3) float32 or None, faces (F,3) int64, 0-based) of an OBJ as export_obj writes it (`v` lines of
	3 or 6 numbers, triangular `f` lines; a `/` suffix on a face index is ignored)."""
	verts, faces = [], []
	with open(loc) as fh:
		for line in fh:
			p = line.split()
			if not p:
				continue
			if p[0] == 'v':
				verts.append([float(x) for x in p[1:]])
			elif p[0] == 'f':
				faces.append([int(x.split('/')[0]) - 1 for x in p[1:4]])
	widths = {len(v) for v in verts}
	if widths - {3, 6} or len(widths) > 1:
		raise ValueError(f'find_amd.vis.read_obj_colours: {loc}: `v` lines of 3 or of 6 numbers expected, got {sorted(widths)}')
	v = torch.tensor(verts, dtype=torch.float64).reshape(len(verts), -1).float()
	f = torch.tensor(faces, dtype=torch.int64).reshape(len(faces), 3)
	return v[:, :3].contiguous(), (v[:, 3:].contiguous() if v.shape[1] == 6 else None), f
