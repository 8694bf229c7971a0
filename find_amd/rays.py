"""Rays on the HIP path: the closest hit of a ray on a triangle mesh, or whether anything is hit at all (find_ray_fwd / find_ray_bwd,
csrc/raycast.hip: the watertight pair test of Woop, Benthin & Wald 2013, every ray against every face), and what follows from them --
which vertices a camera sees, and ambient occlusion at points and at vertices.  Not in the reference.  d need not be normalised: t is in
units of |d|, and o + t[..., None] * d is the hit point.  A ray through a shared edge or a vertex of a closed mesh hits (a zero of an edge
function counts as inside); a face with a corner exactly at the origin is never hit, which is what lets rays start AT vertices.  accel= gives the same bits through a bounding-volume hierarchy over the
faces (MeshBVH, build_bvh; find_ray_bvh_fwd, csrc/bvh.hip) instead of against every face.  There is no
CPU or eager fallback: CPU tensors raise.  The workspace comes from functional._ws and the outputs are torch.empty, which the kernels write
in full (tests/test_gpu_rays.py runs the module over poisoned memory)."""
import functools
import math
import threading

import torch

from . import _lib
from . import functional as FN
from ._lib import check, current_stream, ptr

_CHUNK_RAYS = 1 << 20   # rays of all meshes together that vertex_visibility generates and consumes at a time
BVH_LEAF, BVH_ARITY = 4, 4   # faces per leaf and children per node of a MeshBVH (FIND_BVH_LEAF, FIND_BVH_ARITY of include/find_hip.h)


def _check(who, origins, dirs, verts, faces):
	"""Shapes first (they can be told on any device), then the device.  Returns (N, R, V, F, faces_batch)."""
	if (origins.dim() != 3 or origins.shape[-1] != 3 or dirs.shape != origins.shape or verts.dim() != 3 or verts.shape[-1] != 3
			or verts.shape[0] != origins.shape[0]):
		raise RuntimeError(f'find_amd.rays.{who}: origins, dirs (N, R, 3) and verts (N, V, 3) expected, got {tuple(origins.shape)} / {tuple(dirs.shape)} / '
						   f'{tuple(verts.shape)}')
	N = origins.shape[0]
	if faces.dim() not in (2, 3) or faces.shape[-1] != 3 or (faces.dim() == 3 and faces.shape[0] not in (1, N)) or faces.is_floating_point():
		raise RuntimeError(f'find_amd.rays.{who}: integer faces (F, 3) or ({N}, F, 3) expected, got {tuple(faces.shape)} {faces.dtype}')
	for t in (origins, dirs, verts, faces):
		if not t.is_cuda:
			raise RuntimeError(f'find_amd.rays.{who}: the HIP path needs tensors on a ROCm device (got a CPU tensor); there is no CPU fallback')
	for t in (origins, dirs, verts):
		if t.dtype != torch.float32:
			raise RuntimeError(f'find_amd.rays.{who}: fp32 tensors required, got {t.dtype}')
	return N, origins.shape[1], verts.shape[1], faces.shape[-2], 1 if faces.dim() == 2 else faces.shape[0]


def _interval(who, t_min, t_max):
	t_min, t_max = float(t_min), float(t_max)
	if not t_min >= 0 or math.isnan(t_max):
		raise RuntimeError(f'find_amd.rays.{who}: t_min >= 0 and a t_max that is not NaN expected, got {t_min} / {t_max}')
	return t_min, t_max


def _per_ray(who, name, x, N, R, dev):
	"""r_len (N) / skip (N, R) as int32 on the device, or None."""
	if x is None:
		return None
	x = torch.as_tensor(x).to(device=dev, dtype=torch.int32).contiguous()
	want = (N,) if name == 'r_len' else (N, R)
	if x.shape != want:
		raise RuntimeError(f'find_amd.rays.{who}: {name} {want} expected, got {tuple(x.shape)}')
	return x


class MeshBVH:
	"""A bounding-volume hierarchy over the faces of a batch of meshes (find_bvh_keys / find_bvh_build / find_bvh_refit, csrc/bvh.hip): what
	accel= of this module's functions takes.  Opaque: `data` is the library's buffer (find_bvh_bytes).  It remembers N, V, F and faces_batch
	and refuses tensors of other shapes; the faces it was built on are taken to be the faces of every later call.  After the vertices
	change, call refit(verts) -- boxes again from the new vertices in the stored order, no sort; exact however far they moved, only the
	speed depends on the order -- or the answers are wrong (never a fault: every index in the structure is computed or range-checked)."""

	def __init__(self, N, V, F, faces_batch, faces, data):
		self.N, self.V, self.F, self.faces_batch, self.faces, self.data = N, V, F, faces_batch, faces, data

	@property
	def nbytes(self):
		return self.data.numel()

	def _fits(self, who, N, V, F, fb, dev):
		if (N, V, F, fb) != (self.N, self.V, self.F, self.faces_batch) or dev != self.data.device:
			raise RuntimeError(f'find_amd.rays.{who}: this MeshBVH was built for N, V, F, faces_batch = {(self.N, self.V, self.F, self.faces_batch)} on '
							   f'{self.data.device}, got {(N, V, F, fb)} on {dev}')

	def refit(self, verts):
		"""The boxes again from `verts` (N, V, 3), with the faces of the build (self.faces, int32).  Returns self."""
		N, V, F, fb = _check_mesh('MeshBVH.refit', verts, self.faces)
		self._fits('MeshBVH.refit', N, V, F, fb, verts.device)
		verts = verts.detach().contiguous()
		check(_lib.lib().find_bvh_refit(ptr(verts), ptr(self.faces), fb, N, V, F, ptr(self.data), self.data.numel(), current_stream(verts.device)),
			  'find_bvh_refit')
		return self


def _check_mesh(who, verts, faces):
	"""(N, V, F, faces_batch) of verts (N, V, 3) and faces, as _check sees them."""
	if verts.dim() != 3 or verts.shape[-1] != 3:
		raise RuntimeError(f'find_amd.rays.{who}: verts (N, V, 3) expected, got {tuple(verts.shape)}')
	N, _, V, F, fb = _check(who, verts, verts, verts, faces)   # (verts stands in for the rays)
	return N, V, F, fb


def build_bvh(verts, faces):
	"""A MeshBVH of verts (N, V, 3) and faces (F, 3) shared or (N, Fmax, 3) with -1 rows: Morton keys of the faces' centroids (find_bvh_keys),
	torch.sort of every row (the keys are below 2^63, so the signed sort is the unsigned one), the boxes bottom-up (find_bvh_build).  No
	gradient, no CPU fallback."""
	who = 'build_bvh'
	N, V, F, fb = _check_mesh(who, verts, faces)
	verts, faces = verts.detach().contiguous(), FN._faces_i32(faces)
	L = _lib.lib()
	dev = verts.device
	data = torch.empty(L.find_bvh_bytes(N, F), device=dev, dtype=torch.uint8)
	keys = torch.empty(N, F, device=dev, dtype=torch.int64)
	s = current_stream(dev)
	check(L.find_bvh_keys(ptr(verts), ptr(faces), fb, N, V, F, ptr(keys), ptr(data), data.numel(), s), 'find_bvh_keys')
	keys = torch.sort(keys, dim=1)[0].contiguous()
	check(L.find_bvh_build(ptr(verts), ptr(faces), fb, N, V, F, ptr(keys), ptr(data), data.numel(), s), 'find_bvh_build')
	return MeshBVH(N, V, F, fb, faces, data)


_STATE = threading.local()   # .accel: what the accel= keyword of the call in progress on this thread asked for ('bvh' until the first cast builds it)


def _accel_keyword(fn):
	"""Gives a public function the keyword accel=None | 'bvh' | MeshBVH.  The function's own parameters stay the ones it has without the
	keyword (tests/test_rays_host.py pins those lists, and inspect.signature reports them: accel is this wrapper's, documented in each
	docstring).  The request travels to _cast in _STATE for the time of the call, so the functions that cast in chunks, or through one
	another, share one structure; with accel=None the function is called as it always was."""
	@functools.wraps(fn)
	def call(*args, accel=None, **kw):
		if accel is None:
			return fn(*args, **kw)
		if not (isinstance(accel, MeshBVH) or (isinstance(accel, str) and accel == 'bvh')):
			raise RuntimeError(f"find_amd.rays.{fn.__name__}: accel None, 'bvh' or a MeshBVH expected, got {accel!r}")
		before = getattr(_STATE, 'accel', None)
		_STATE.accel = accel
		try:
			return fn(*args, **kw)
		finally:
			_STATE.accel = before
	return call


def _cast(who, origins, dirs, verts, faces, r_len, skip, t_min, t_max, any_hit):
	"""One find_ray_fwd call -- find_ray_bvh_fwd under accel= (_STATE) --: (t, idx, bary), or hit (N, R) bool, and the contiguous inputs it was made on."""
	N, R, V, F, fb = _check(who, origins, dirs, verts, faces)
	origins, dirs, verts, faces = origins.detach().contiguous(), dirs.detach().contiguous(), verts.detach().contiguous(), FN._faces_i32(faces)
	t_min, t_max = _interval(who, t_min, t_max)
	L = _lib.lib()
	dev = origins.device
	accel = getattr(_STATE, 'accel', None)
	if isinstance(accel, str):   # 'bvh': built at the call's first cast, then shared by the rest of the call
		accel = _STATE.accel = build_bvh(verts, faces)
	if accel is not None:
		accel._fits(who, N, V, F, fb, dev)
	rl, sk = _per_ray(who, 'r_len', r_len, N, R, dev), _per_ray(who, 'skip', skip, N, R, dev)
	ws = FN._ws(L.find_ray_ws_bytes(N, R, F), dev)
	if any_hit:
		hit = torch.empty(N, R, device=dev, dtype=torch.uint8)
		out = (None, None, None, hit)
	else:
		out = (torch.empty(N, R, device=dev, dtype=torch.float32), torch.empty(N, R, device=dev, dtype=torch.int32),
			   torch.empty(N, R, 3, device=dev, dtype=torch.float32), None)
	if accel is None:
		check(L.find_ray_fwd(ptr(origins), ptr(dirs), ptr(rl), ptr(sk), ptr(verts), ptr(faces), fb, N, R, V, F, t_min, t_max, 1 if any_hit else 0, ptr(out[0]),
							 ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(ws), ws.numel(), current_stream(dev)), 'find_ray_fwd')
	else:
		check(L.find_ray_bvh_fwd(ptr(origins), ptr(dirs), ptr(rl), ptr(sk), ptr(verts), ptr(faces), fb, N, R, V, F, t_min, t_max, 1 if any_hit else 0, ptr(out[0]),
								 ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(accel.data), accel.data.numel(), ptr(ws), ws.numel(), current_stream(dev)),
			  'find_ray_bvh_fwd')
	return (out[3].bool() if any_hit else out[:3]), (origins, dirs, verts, faces)


class _Intersect(torch.autograd.Function):
	"""The closest hit (find_ray_fwd / find_ray_bwd): t, and idx and bary as non-differentiable outputs."""

	@staticmethod
	def forward(ctx, origins, dirs, verts, faces, r_len, skip, t_min, t_max):
		(t, idx, bary), (origins, dirs, verts, faces) = _cast('ray_mesh_intersect', origins, dirs, verts, faces, r_len, skip, t_min, t_max, False)
		ctx.save_for_backward(origins, dirs, verts, faces, idx, bary, t)
		ctx.mark_non_differentiable(idx, bary)
		ctx.set_materialize_grads(False)
		return t, idx, bary

	@staticmethod
	def backward(ctx, g, _g_idx=None, _g_bary=None):
		origins, dirs, verts, faces, idx, bary, t = ctx.saved_tensors
		need_o, need_d, need_v = ctx.needs_input_grad[:3]
		if g is None or not (need_o or need_d or need_v):
			return (None,) * 8
		N, R, V = origins.shape[0], origins.shape[1], verts.shape[1]
		fb, F = (1, faces.shape[0]) if faces.dim() == 2 else faces.shape[:2]
		d_o = torch.empty_like(origins) if need_o else None
		d_d = torch.empty_like(dirs) if need_d else None
		d_v = torch.zeros_like(verts) if need_v else None   # (find_ray_bwd adds to it)
		check(_lib.lib().find_ray_bwd(ptr(origins), ptr(dirs), ptr(verts), ptr(faces), fb, ptr(idx), ptr(bary), ptr(t), ptr(g.contiguous()), N, R, V, F, ptr(d_o),
									  ptr(d_d), ptr(d_v), current_stream(origins.device)), 'find_ray_bwd')
		return d_o, d_d, d_v, None, None, None, None, None


@_accel_keyword
def ray_mesh_intersect(origins, dirs, verts, faces, r_len=None, skip=None, t_min=0.0, t_max=math.inf):
	"""The closest hit of every ray on its mesh.  origins, dirs (N, R, 3), verts (N, V, 3), faces (F, 3) shared or (N, Fmax, 3) with -1 rows as
	padding, r_len (N) ray counts or None, skip (N, R) a face per ray that it never hits (the face its origin lies on; -1: none) or None.
	Returns (t (N, R): the distance in units of |d| with t_min < t <= t_max, +inf for a miss; idx (N, R) int32: the face, -1 for a miss;
	bary (N, R, 3): the hit point's barycentrics, 0 for a miss).  Rows at or past r_len are misses.  Never hit: a -1 row, a face with an
	index outside [0, V), a face with a corner exactly at the origin, the skip face; a ray with a non-finite component or d == 0 hits
	nothing.  Among equal t the smallest face wins.  Two calls agree bit for bit, and a row does not depend on the rest of the batch.
	Differentiable in origins, dirs and verts through t (the face and the barycentrics are constants: dt/do = -n / g, dt/dd = -t n / g,
	dt/dv_i = w_i n / g with n the face's normal and g = n . d); idx and bary carry no gradient.
	Keyword accel (added by _accel_keyword): None -- every ray against every face --, 'bvh' -- a MeshBVH built for this call -- or a
	MeshBVH of these meshes (build_bvh; refit after the vertices moved).  The results are the same bits and the gradients come from the same backward, with one difference: under
	accel a face with a non-finite corner is never hit (without it that is left to the pair test, in practice a miss)."""
	return _Intersect.apply(origins, dirs, verts, faces, r_len, skip, t_min, t_max)


@_accel_keyword
def ray_occluded(origins, dirs, verts, faces, r_len=None, skip=None, t_min=0.0, t_max=math.inf):
	"""Whether each ray hits anything in (t_min, t_max]: bool (N, R), bit for bit isfinite(t) of ray_mesh_intersect with the same arguments.
	The kernel stops walking the faces of a block of rays once all of them have hit; with accel (as in ray_mesh_intersect) a ray
	stops at its first accepted pair.  No gradient."""
	return _cast('ray_occluded', origins, dirs, verts, faces, r_len, skip, t_min, t_max, True)[0]


# ---------------------------------------------------------------------------------------------- visibility
def camera_centres(R, T):
	"""C = -T @ R^T of cameras in the library's convention p_view = p_world @ R + T.  R (..., 3, 3), T (..., 3) -> (..., 3).  Pure torch."""
	return -(T[..., None, :] @ R.transpose(-1, -2))[..., 0, :]


@_accel_keyword
def vertex_visibility(verts, faces, R, T):
	"""Which vertices each camera sees: bool (N, M, V).  verts (N, V, 3), faces as in ray_mesh_intersect, cameras R (M, 3, 3) / T (M, 3) shared
	by the meshes or (N, M, 3, 3) / (N, M, 3), in the convention p_view = p_world @ R + T, so the centre is C = -T @ R^T.  One ray per
	(camera, vertex) goes from C with d = v - C; the vertex is visible iff the ray hits nothing or the face it hits contains that vertex.
	There is no tolerance: the faces at the vertex share its projected bits, so the ray hits one of them at t about 1 unless something
	nearer is in the way.  The rays are generated and consumed a chunk of cameras at a time; accel as in ray_mesh_intersect, the
	structure built once for all chunks.  No gradient."""
	who = 'vertex_visibility'
	if verts.dim() != 3 or verts.shape[-1] != 3 or R.shape[-2:] != (3, 3) or T.shape != R.shape[:-1] or R.dim() not in (3, 4) or (R.dim() == 4 and R.shape[0] != verts.shape[0]):
		raise RuntimeError(f'find_amd.rays.{who}: verts (N, V, 3), R (M, 3, 3) or (N, M, 3, 3) and T (M, 3) or (N, M, 3) expected, got {tuple(verts.shape)} / '
						   f'{tuple(R.shape)} / {tuple(T.shape)}')
	N, V = verts.shape[:2]
	_check(who, verts, verts, verts, faces)   # (verts stands in for the rays: they are made here)
	if not (R.is_cuda and T.is_cuda):
		raise RuntimeError(f'find_amd.rays.{who}: the HIP path needs tensors on a ROCm device (got a CPU tensor); there is no CPU fallback')
	verts = verts.detach().contiguous()
	f32 = FN._faces_i32(faces)
	C = camera_centres(R.detach().float(), T.detach().float())
	C = C.expand(N, -1, -1) if C.dim() == 3 else C[None].expand(N, -1, -1)   # (N, M, 3)
	M = C.shape[1]
	fl = (f32 if f32.dim() == 3 else f32[None]).long()   # (1 | N, F, 3)
	own = torch.arange(V, device=verts.device)
	vis = torch.empty(N, M, V, dtype=torch.bool, device=verts.device)
	step = max(1, _CHUNK_RAYS // max(N * V, 1))
	for m0 in range(0, M, step):
		c = C[:, m0:m0 + step]   # (N, m, 3)
		m = c.shape[1]
		o = c[:, :, None, :].expand(N, m, V, 3)
		d = verts[:, None] - o
		(_, idx, _), _ = _cast(who, o.reshape(N, m * V, 3), d.reshape(N, m * V, 3), verts, f32, None, None, 0., math.inf, False)
		idx = idx.view(N, m, V).long()
		hit_face = torch.gather(fl.expand(N, -1, -1), 1, idx.clamp(min=0).reshape(N, m * V, 1).expand(-1, -1, 3)).view(N, m, V, 3) if fl.shape[1] else None
		seen = idx < 0
		if hit_face is not None:
			seen = seen | (hit_face == own[None, None, :, None]).any(-1)
		vis[:, m0:m0 + m] = seen
	return vis


# ---------------------------------------------------------------------------------------------- ambient occlusion
def hemisphere_directions(n_dirs, device=None):
	"""The fixed, cosine-distributed direction set, (n_dirs, 3) float32 unit vectors about +z: for i = 0 .. n_dirs - 1, in float64,
	u = (i + 0.5) / n_dirs, phi = 2 pi frac(i (sqrt(5) - 1) / 2) (the golden-ratio spiral), r = sqrt(u):
	(r cos phi, r sin phi, sqrt(1 - u)), rounded to float32 (Malley's method: a uniform disc lifted to the hemisphere)."""
	i = torch.arange(n_dirs, dtype=torch.float64)
	u = (i + 0.5) / n_dirs
	phi = 2 * math.pi * torch.frac(i * ((math.sqrt(5.) - 1) / 2))
	r = u.sqrt()
	return torch.stack([r * phi.cos(), r * phi.sin(), (1 - u).sqrt()], -1).float().to(device)


def normal_frames(normals):
	"""The per-point frame (t1, t2, n), each (..., 3): n = normal / max(|normal|, 1e-12); a = the coordinate axis along which |n| is smallest
	(the first of equals); t1 = a x n normalised; t2 = n x t1.  Pure torch."""
	n = normals / normals.norm(dim=-1, keepdim=True).clamp(min=1e-12)
	a = torch.nn.functional.one_hot(n.abs().argmin(-1), 3).to(n.dtype)
	t1 = torch.linalg.cross(a, n)
	t1 = t1 / t1.norm(dim=-1, keepdim=True).clamp(min=1e-12)
	return t1, torch.linalg.cross(n, t1), n


@_accel_keyword
def ambient_occlusion(points, normals, verts, faces, n_dirs=64, max_dist=None, skip=None, rays_per_call=1 << 20):
	"""The share of n_dirs hemisphere directions about each normal that escape: (N, P) float32 in [0, 1], 1 = open sky.  points, normals
	(N, P, 3), verts, faces as in ray_mesh_intersect; skip (N, P) the face each point lies on (never hit by its rays) or None -- a point AT a
	vertex needs none, the faces with a corner at the origin are never hit.  max_dist: how far, in the mesh's units, a hit still occludes
	(None: no limit).  The direction set is hemisphere_directions(n_dirs) -- fixed, cosine-distributed, so the plain share is the
	cosine-weighted visibility -- and direction i at a point is x t1 + y t2 + z n in the frame of normal_frames(normals): the same for every
	call.  Rays are cast by ray_occluded, at most about rays_per_call at a time; accel as in ray_mesh_intersect, the structure
	built once for all chunks.  No gradient."""
	who = 'ambient_occlusion'
	if normals.shape != points.shape:
		raise RuntimeError(f'find_amd.rays.{who}: points and normals (N, P, 3) expected, got {tuple(points.shape)} / {tuple(normals.shape)}')
	N, P, _, _, _ = _check(who, points, normals, verts, faces)
	if not isinstance(n_dirs, int) or isinstance(n_dirs, bool) or n_dirs < 1 or rays_per_call < 1:
		raise RuntimeError(f'find_amd.rays.{who}: n_dirs >= 1 (an int) and rays_per_call >= 1 expected, got {n_dirs!r} / {rays_per_call!r}')
	t_max = math.inf if max_dist is None else float(max_dist)
	if not t_max > 0:
		raise RuntimeError(f'find_amd.rays.{who}: max_dist > 0 or None expected, got {max_dist!r}')
	dev = points.device
	points, verts = points.detach().contiguous(), verts.detach().contiguous()
	f32 = FN._faces_i32(faces)
	sk = _per_ray(who, 'skip', skip, N, P, dev)
	t1, t2, n = normal_frames(normals.detach())
	local = hemisphere_directions(n_dirs, dev)
	ao = torch.empty(N, P, device=dev, dtype=torch.float32)
	step = max(1, int(rays_per_call) // max(N * n_dirs, 1))
	for p0 in range(0, P, step):
		s = slice(p0, p0 + step)
		d = local[:, 0, None] * t1[:, s, None] + local[:, 1, None] * t2[:, s, None] + local[:, 2, None] * n[:, s, None]   # (N, p, n_dirs, 3)
		p = d.shape[1]
		o = points[:, s, None].expand(-1, -1, n_dirs, -1)
		k = None if sk is None else sk[:, s, None].expand(-1, -1, n_dirs).reshape(N, p * n_dirs)
		hit, _ = _cast(who, o.reshape(N, p * n_dirs, 3), d.reshape(N, p * n_dirs, 3), verts, f32, None, k, 0., t_max, True)
		ao[:, s] = (~hit).view(N, p, n_dirs).sum(-1).float() / n_dirs
	return ao


@_accel_keyword
def vertex_ambient_occlusion(verts, faces, n_dirs=64, max_dist=None, rays_per_call=1 << 20):
	"""ambient_occlusion at the vertices themselves, about functional.vertex_normals: (N, V).  The faces at a vertex have a corner at its rays'
	origin and are never hit, so no skip is needed.  A vertex no face touches has no normal: its rays have d = 0, hit nothing, and it gets 1."""
	who = 'vertex_ambient_occlusion'
	_check(who, verts, verts, verts, faces)
	normals = FN.vertex_normals(verts.detach(), faces)
	return ambient_occlusion(verts, normals, verts, faces, n_dirs=n_dirs, max_dist=max_dist, rays_per_call=rays_per_call)
