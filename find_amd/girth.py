"""Tape girths on the HIP path (find_section_hull_*, csrc/girth.hip); not in the reference.  A tape drawn round a foot does not follow the
section of the mesh by its plane into the arch or between the toes: it spans them.  Its number is the perimeter of the section's CONVEX HULL,
which is what section_hulls returns -- by the section rule of find_amd.measure (the same crossing points, bit for bit), the hull taken in
the plane's own 2-D coordinates with strict corners (include/find_hip.h has the rule).  Differentiable in the vertices and in all four
components of the planes, so a plane derived from landmarks on the mesh (plane_through) moves with the mesh.  One workgroup per (mesh,
plane); no atomics either way: two runs agree bit for bit and a mesh's row does not depend on the rest of the batch.  GPU only."""
import torch

from . import _lib
from ._lib import check, current_stream, ptr
from .functional import _c, _faces_i32, _require_gpu

MAX_PLANES = 64


class _SectionHulls(torch.autograd.Function):
	@staticmethod
	def forward(ctx, verts, planes, faces, max_points, max_hull):
		L = _lib.lib()
		verts, planes = _c(verts), _c(planes)
		N, V, _ = verts.shape
		fb, F = (1, faces.shape[0]) if faces.dim() == 2 else faces.shape[:2]
		pb, P = (1, planes.shape[0]) if planes.dim() == 2 else planes.shape[:2]
		nbytes = L.find_section_hull_ws_bytes(N, F, P, max_points, 0)
		if nbytes < 0:
			check(-1, 'find_section_hull_ws_bytes')
		dev = verts.device
		ws = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)   # per (mesh, plane): max_points faces, 2 max_points points (x, y)
		girth = torch.empty(N, P, device=dev, dtype=torch.float32)
		count = torch.empty(N, P, device=dev, dtype=torch.int32)
		n_hull = torch.empty(N, P, device=dev, dtype=torch.int32)
		status = torch.empty(N, P, device=dev, dtype=torch.int32)
		hull_ids = torch.empty(N, P, 2 * max_points, device=dev, dtype=torch.int32)   # the corners in order (2 face + edge): the backward's list
		hull_points = torch.empty(N, P, max_hull, 3, device=dev, dtype=torch.float32) if max_hull > 0 else None
		check(L.find_section_hull_fwd(ptr(verts), ptr(faces), fb, ptr(planes), pb, N, V, F, P, max_points, max_hull, ptr(girth), ptr(count), ptr(n_hull),
									  ptr(status), ptr(hull_ids), ptr(hull_points), ptr(ws), ws.numel() * 8, current_stream(dev)), 'find_section_hull_fwd')
		ctx.dims = (N, V, F, P, fb, pb, max_points)
		ctx.save_for_backward(verts, planes, faces, n_hull, hull_ids)
		if hull_points is None:
			hull_points = girth.new_zeros(N, P, 0, 3)
		ctx.mark_non_differentiable(count, n_hull, status, hull_points)
		return girth, count, n_hull, status, hull_points

	@staticmethod
	def backward(ctx, g, _gc, _gn, _gs, _gp):
		verts, planes, faces, n_hull, hull_ids = ctx.saved_tensors
		N, V, F, P, fb, pb, max_points = ctx.dims
		L = _lib.lib()
		nbytes = L.find_section_hull_ws_bytes(N, F, P, max_points, 1)
		ws = torch.empty(nbytes // 8, device=verts.device, dtype=torch.float64)   # four doubles per (mesh, plane)
		d_verts = torch.empty_like(verts)
		d_planes = torch.empty_like(planes) if ctx.needs_input_grad[1] else None
		check(L.find_section_hull_bwd(ptr(verts), ptr(faces), fb, ptr(planes), pb, N, V, F, P, max_points, ptr(_c(g)), ptr(n_hull), ptr(hull_ids),
									  ptr(d_verts), ptr(d_planes), ptr(ws), ws.numel() * 8, current_stream(verts.device)), 'find_section_hull_bwd')
		return d_verts, d_planes, None, None, None


def section_hulls(verts, faces, planes, return_hull=False, max_points=None, max_hull=256):
	"""Girth (N, P) fp32: the perimeter of the convex hull of the section of mesh n by plane p -- what a tape round the foot in that plane
	reads.  verts (N, V, 3); faces (F, 3) shared or (N, F, 3) per mesh, any integer dtype -- a row with a -1, an index outside [0, V) or a
	repeated vertex contributes nothing; planes (P, 4) shared or (N, P, 4), rows (nx, ny, nz, d) of the plane n . v = d with the normal taken
	as given (normalise it), 1 <= P <= 64.  Differentiable in the vertices and in ALL FOUR components of the planes (the normal is not
	renormalised inside: its gradient is with respect to the components as given).  A section of several loops (the toes, two feet) is
	wrapped as one; two distinct points give twice their distance, one or none 0, a plane that misses 0.

	max_points: the crossing faces a section may have (default: F, which cannot overflow; the workspace is N P max_points 28 bytes, so a
	caller with 200k-face scans may lower it).  A section with more gets status bit 1, girth 0 and a zero gradient.

	With return_hull: (girth, n_hull, count, status, hull_points) -- n_hull (N, P) int32 the hull's corners, count (N, P) int32 the crossing
	faces (plane_sections' count), status (N, P) int32 (0; bit 1: more than max_points crossing faces; bit 2: the walk did not close), and
	hull_points (N, P, max_hull, 3) the corners in order, counter-clockwise about the normal, zeros past n_hull -- for drawing a section.  A
	hull of more than max_hull corners is truncated there; the girth is unaffected."""
	if verts.dim() != 3 or verts.shape[-1] != 3 or verts.shape[0] < 1 or verts.shape[1] < 1:
		raise ValueError(f'find_amd.girth.section_hulls: verts (N, V, 3) expected, got {tuple(verts.shape)}')
	N, V, _ = verts.shape
	if faces.dim() not in (2, 3) or faces.shape[-1] != 3 or faces.is_floating_point() or faces.shape[-2] < 1:
		raise ValueError(f'find_amd.girth.section_hulls: integer faces (F, 3) or (N, F, 3) expected, got {tuple(faces.shape)} {faces.dtype}')
	if faces.dim() == 3 and faces.shape[0] not in (1, N):
		raise ValueError(f'find_amd.girth.section_hulls: {faces.shape[0]} face lists for {N} meshes')
	if planes.dim() not in (2, 3) or planes.shape[-1] != 4 or not 1 <= planes.shape[-2] <= MAX_PLANES:
		raise ValueError(f'find_amd.girth.section_hulls: planes (P, 4) or (N, P, 4), 1 <= P <= {MAX_PLANES}, expected, got {tuple(planes.shape)}')
	if planes.dim() == 3 and planes.shape[0] not in (1, N):
		raise ValueError(f'find_amd.girth.section_hulls: {planes.shape[0]} plane lists for {N} meshes')
	F = faces.shape[-2]
	max_points = F if max_points is None else int(max_points)
	if not 1 <= max_points <= F:
		raise ValueError(f'find_amd.girth.section_hulls: max_points must lie in 1 .. F = {F}, got {max_points}')
	max_hull = min(int(max_hull), 2 * max_points) if return_hull else 0
	if return_hull and max_hull < 1:
		raise ValueError(f'find_amd.girth.section_hulls: max_hull must be at least 1, got {max_hull}')
	_require_gpu(verts, faces, planes)
	f32 = _faces_i32(faces)
	girth, count, n_hull, status, hull_points = _SectionHulls.apply(verts, planes, f32, max_points, max_hull)
	return (girth, n_hull, count, status, hull_points) if return_hull else girth


def plane_through(a, b, up=(0., 0., 1.)):
	"""The plane (..., 4) = (n, d) that contains the points a and b (..., 3) and the direction `up`: n = normalize((b - a) x up), d = n . a.
	Pure torch, differentiable in a and b (and in `up` if it is a tensor).  With a and b the two metatarsal-head landmarks of a mesh, say
	verts[:, i1] and verts[:, i5], section_hulls(verts, faces, plane_through(verts[:, i1], verts[:, i5])[:, None]) is the ISO-style ball
	girth: the tape round the foot through both heads, in the tilted plane they define, which moves with the mesh.  WHICH vertices of a
	template are the landmarks is the caller's knowledge: nothing here chooses them."""
	up = torch.as_tensor(up, dtype=a.dtype, device=a.device)
	n = torch.linalg.cross(b - a, up.expand_as(a))
	n = n / n.norm(dim=-1, keepdim=True)
	return torch.cat([n, (n * a).sum(-1, keepdim=True)], dim=-1)
