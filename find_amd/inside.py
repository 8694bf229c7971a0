"""Inside and outside on the HIP path: generalised winding numbers (find_winding_fwd, csrc/winding.hip; Jacobson et al. 2013) and what
follows from them -- a signed point-to-surface distance, occupancy grids, the volume of an open scan and the volumetric IoU of two meshes.
Not in the reference.  w(p) is the sum over the faces of the solid angle they subtend at p, over 4 pi: 1 inside an outward-oriented closed
mesh, 0 outside, -1 inside an inward-oriented one; on a mesh with a hole (scans and the template are open at the ankle) it varies smoothly,
and w > 0.5 closes the hole about flat.  There is no CPU or eager fallback: CPU tensors raise (mesh_volume(res=None), which is pure torch,
apart).  The workspace comes from functional._ws and w is torch.empty, which the kernels write in full (tests/test_gpu_inside.py runs the
module over poisoned memory)."""
import torch

from . import _lib
from . import functional as FN
from ._lib import check, current_stream, ptr

_CHUNK_POINTS = 1 << 19   # grid cells of all meshes together that are generated and consumed at a time


def _check(who, points, verts, faces, need_gpu=True):
	"""Shapes first (they can be told on any device), then the device.  Returns (N, P, V, F, faces_batch)."""
	if points.dim() != 3 or verts.dim() != 3 or points.shape[-1] != 3 or verts.shape[-1] != 3 or verts.shape[0] != points.shape[0]:
		raise RuntimeError(f'find_amd.inside.{who}: points (N, P, 3) and verts (N, V, 3) expected, got {tuple(points.shape)} / {tuple(verts.shape)}')
	N = points.shape[0]
	if faces.dim() not in (2, 3) or faces.shape[-1] != 3 or (faces.dim() == 3 and faces.shape[0] not in (1, N)) or faces.is_floating_point():
		raise RuntimeError(f'find_amd.inside.{who}: integer faces (F, 3) or ({N}, F, 3) expected, got {tuple(faces.shape)} {faces.dtype}')
	if need_gpu:
		for t in (points, verts, faces):
			if not t.is_cuda:
				raise RuntimeError(f'find_amd.inside.{who}: the HIP path needs tensors on a ROCm device (got a CPU tensor); there is no CPU fallback')
		for t in (points, verts):
			if t.dtype != torch.float32:
				raise RuntimeError(f'find_amd.inside.{who}: fp32 tensors required, got {t.dtype}')
	return N, points.shape[1], verts.shape[1], faces.shape[-2], 1 if faces.dim() == 2 else faces.shape[0]


def _winding(who, points, verts, faces, p_len):
	N, P, V, F, fb = _check(who, points, verts, faces)
	L = _lib.lib()
	points, verts = points.detach().contiguous(), verts.detach().contiguous()
	faces = FN._faces_i32(faces)
	dev = points.device
	pl = None if p_len is None else torch.as_tensor(p_len).to(device=dev, dtype=torch.int32).contiguous()
	if pl is not None and pl.shape != (N,):
		raise RuntimeError(f'find_amd.inside.{who}: p_len ({N},) expected, got {tuple(pl.shape)}')
	w = torch.empty(N, P, device=dev, dtype=torch.float32)
	ws = FN._ws(L.find_winding_ws_bytes(N, P, F), dev)
	check(L.find_winding_fwd(ptr(points), ptr(pl), ptr(verts), ptr(faces), fb, N, P, V, F, ptr(w), ptr(ws), ws.numel(), current_stream(dev)), 'find_winding_fwd')
	return w


def winding_number(points, verts, faces, p_len=None):
	"""The generalised winding number of every point about its mesh.  points (N, P, 3), verts (N, V, 3), faces (F, 3) shared or (N, Fmax, 3)
	with -1 rows as padding, p_len (N) point counts or None: the conventions of functional.point_face_distance.  Returns w (N, P) float32.
	A -1 row, a face with an index outside [0, V), a face with a corner at the point and a face whose plane holds the point (det == 0
	exactly) contribute 0; rows at or past p_len and a mesh without a face give 0.  Summed in double in a fixed order: two calls agree bit for
	bit, and a row does not depend on the rest of the batch.  Not differentiable (inputs are detached)."""
	return _winding('winding_number', points, verts, faces, p_len)


class _SignedRoot(torch.autograd.Function):
	"""sign * sqrt(dist2) with the gradient sign / (2 sqrt(dist2)), and 0 -- not inf or NaN -- where dist2 == 0 (a point on the surface has
	no direction to leave it by)."""

	@staticmethod
	def forward(ctx, dist2, sign):
		root = dist2.sqrt()
		ctx.save_for_backward(root, sign)
		return sign * root

	@staticmethod
	def backward(ctx, g):
		root, sign = ctx.saved_tensors
		return torch.where(root > 0, g * sign * 0.5 / root.clamp(min=1e-38), torch.zeros_like(g)), None


def signed_distance(points, verts, faces, p_len=None, level=0.5):
	"""The signed distance to the surface: (sdf (N, P), idx (N, P) int32, bary (N, P, 3), w (N, P)) with |sdf| = sqrt(dist2) of
	functional.point_face_distance, whose idx and bary these are, and sdf < 0 where the winding number w > level (inside).  Differentiable in
	points and verts through find_point_face_bwd; the sign is a constant, and the gradient is 0 where dist2 == 0.  Rows at or past p_len: 0."""
	_check('signed_distance', points, verts, faces)
	dist2, idx, bary = FN.point_face_distance(points, verts, faces, p_len)
	w = _winding('signed_distance', points, verts, faces, p_len)
	sign = torch.where(w > level, -torch.ones_like(w), torch.ones_like(w))
	return _SignedRoot.apply(dist2, sign), idx, bary, w


# ---------------------------------------------------------------------------------------------- grids
def grid_points(origin, spacing, res, start, stop):
	"""The centres of the cells start .. stop - 1 of a res^3 grid, cell (i, j, k) -- flat index (i res + j) res + k, i along x -- at
	origin + (i + 0.5, j + 0.5, k + 0.5) * spacing.  origin, spacing (N, 3) -> (N, stop - start, 3).  Pure torch, on the tensors' device."""
	flat = torch.arange(start, stop, device=origin.device)
	ijk = torch.stack([flat // (res * res), (flat // res) % res, flat % res], -1).to(origin.dtype) + 0.5
	return origin[:, None, :] + ijk[None] * spacing[:, None, :]


def _box(who, verts_list, bounds, pad):
	"""(origin (N, 3), spacing * res (N, 3)) of the grid: `bounds` = (lo, hi), each (3,) or (N, 3), taken as given; None: the box of all
	vertices of mesh n over verts_list, grown by pad on every side."""
	N, dev = verts_list[0].shape[0], verts_list[0].device
	if bounds is None:
		lo = torch.stack([v.detach().amin(1) for v in verts_list]).amin(0) - pad
		hi = torch.stack([v.detach().amax(1) for v in verts_list]).amax(0) + pad
	else:
		lo, hi = (torch.as_tensor(b, dtype=torch.float32, device=dev).expand(N, 3) for b in bounds)
	if not bool((hi > lo).all()):
		raise RuntimeError(f'find_amd.inside.{who}: an empty box: lo {lo.tolist()}, hi {hi.tolist()}')
	return lo.contiguous(), (hi - lo).contiguous()


def _res(who, res):
	if not isinstance(res, int) or isinstance(res, bool) or not 1 <= res <= 1024:
		raise RuntimeError(f'find_amd.inside.{who}: res must be an int in [1, 1024], got {res!r}')
	return res


def _for_each_chunk(who, meshes, origin, spacing, res, level, visit):
	"""Calls visit(start, stop, [inside (N, stop - start) bool per mesh]) over the grid, a chunk of cells at a time."""
	N = origin.shape[0]
	chunk = max(1 << 10, _CHUNK_POINTS // N)
	for start in range(0, res ** 3, chunk):
		stop = min(start + chunk, res ** 3)
		pts = grid_points(origin, spacing, res, start, stop)
		visit(start, stop, [_winding(who, pts, v, f, None) > level for v, f in meshes])


def _mesh_args(who, verts, faces):
	_check(who, verts, verts, faces)   # (verts stands in for the points: the grid's are made here)
	return verts, faces


def occupancy_grid(verts, faces, res=64, bounds=None, pad=0.005, level=0.5):
	"""Which cells of a res^3 grid lie inside each mesh (winding number at the cell's centre > level).  verts (N, V, 3), faces as in
	winding_number; bounds None: each mesh's own box grown by pad (metres) on every side, else (lo, hi), each (3,) or (N, 3), as given.
	Returns (occ (N, res, res, res) bool, indexed [n, i, j, k] with i along x; origin (N, 3); spacing (N, 3)): cell (i, j, k) is centred at
	origin + (i + 0.5, j + 0.5, k + 0.5) * spacing (grid_points).  The points are generated and consumed a chunk at a time."""
	who = 'occupancy_grid'
	verts, faces = _mesh_args(who, verts, faces)
	res = _res(who, res)
	origin, extent = _box(who, [verts], bounds, pad)
	spacing = extent / res
	occ = torch.empty(verts.shape[0], res ** 3, dtype=torch.bool, device=verts.device)

	def visit(start, stop, inside):
		occ[:, start:stop] = inside[0]
	_for_each_chunk(who, [(verts, faces)], origin, spacing, res, level, visit)
	return occ.view(-1, res, res, res), origin, spacing


def _signed_volume(verts, faces):
	"""sum a . (b x c) / 6 over the faces that count (no -1 row, every index in [0, V)), float64."""
	V = verts.shape[1]
	f = (faces if faces.dim() == 3 else faces[None]).long()
	ok = ((f >= 0) & (f < V)).all(-1)
	f = f.clamp(0, max(V - 1, 0)).expand(verts.shape[0], -1, -1)
	v = verts.double()
	a, b, c = (torch.gather(v, 1, f[..., k:k + 1].expand(-1, -1, 3)) for k in range(3))
	six = (a * torch.linalg.cross(b, c)).sum(-1)
	return torch.where(ok.expand_as(six), six, torch.zeros_like(six)).sum(1) / 6.


def mesh_volume(verts, faces, res=None, level=0.5):
	"""The volume each mesh encloses, (N) float64, m^3.  res None: the exact signed volume sum a . (b x c) / 6 in float64 -- pure torch, on any
	device, differentiable in verts, positive for outward-oriented faces; it means something for CLOSED meshes only.  res an int: the cells of
	occupancy_grid(verts, faces, res, level=level) counted inside, times the cell volume: the one for open scans (no gradient)."""
	who = 'mesh_volume'
	if res is None:
		_check(who, verts, verts, faces, need_gpu=False)
		return _signed_volume(verts, faces)
	verts, faces = _mesh_args(who, verts, faces)
	res = _res(who, res)
	origin, extent = _box(who, [verts], None, 0.005)
	spacing = extent / res
	count = torch.zeros(verts.shape[0], dtype=torch.int64, device=verts.device)

	def visit(start, stop, inside):
		count.add_(inside[0].sum(1))
	_for_each_chunk(who, [(verts, faces)], origin, spacing, res, level, visit)
	return count.double() * spacing.double().prod(-1)


def volume_iou(verts_a, faces_a, verts_b, faces_b, res=64, level=0.5, bounds=None, pad=0.005):
	"""The volumetric intersection over union of mesh n of a with mesh n of b, on ONE res^3 grid over both (bounds None: the box of both
	meshes' vertices grown by pad; else as occupancy_grid).  Returns (iou (N), vol_a (N), vol_b (N)), float64: cells inside both over cells
	inside either (0 where there is none), and the two grid volumes in m^3.  The meshes may differ in V and F; no gradient."""
	who = 'volume_iou'
	for v, f in ((verts_a, faces_a), (verts_b, faces_b)):   # (both meshes' shapes before either's device)
		_check(who, v, v, f, need_gpu=False)
	verts_a, faces_a = _mesh_args(who, verts_a, faces_a)
	verts_b, faces_b = _mesh_args(who, verts_b, faces_b)
	if verts_a.shape[0] != verts_b.shape[0]:
		raise RuntimeError(f'find_amd.inside.{who}: {verts_a.shape[0]} meshes against {verts_b.shape[0]}')
	res = _res(who, res)
	origin, extent = _box(who, [verts_a, verts_b], bounds, pad)
	spacing = extent / res
	counts = torch.zeros(4, verts_a.shape[0], dtype=torch.int64, device=verts_a.device)   # a, b, both, either

	def visit(start, stop, inside):
		a, b = inside
		counts[0].add_(a.sum(1)); counts[1].add_(b.sum(1)); counts[2].add_((a & b).sum(1)); counts[3].add_((a | b).sum(1))
	_for_each_chunk(who, [(verts_a, faces_a), (verts_b, faces_b)], origin, spacing, res, level, visit)
	cell = spacing.double().prod(-1)
	iou = torch.where(counts[3] > 0, counts[2].double() / counts[3].clamp(min=1).double(), torch.zeros_like(cell))
	return iou, counts[0].double() * cell, counts[1].double() * cell
