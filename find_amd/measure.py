"""Foot measurements on the HIP path (find_plane_sections_*, find_extents_*, csrc/measure.hip); not in the reference.  Length and width are
extents of the registered vertices along two axes of the dataset's frame (x towards the toes, y across the foot, z up); a girth is the
perimeter of the polyline in which a plane normal to the length axis cuts the mesh.  The section rule (include/find_hip.h): a vertex is above
a plane iff s = n . v - d >= 0, a face whose vertices are not all on one side crosses, and adds the distance between the two points where its
edges meet the plane -- closed meshes give closed loops, an edge lying in the plane counts once.  One pass over the faces serves every plane;
no float atomics either way: two runs agree bit for bit and a mesh's row does not depend on the rest of the batch.  GPU only."""
import dataclasses
import functools
import weakref

import torch

from . import _lib
from ._lib import check, current_stream, ptr
from .functional import _c, _corner_tables, _faces_i32, _require_gpu

MAX_PLANES = 64
MAX_DIRS = 8


class _PlaneSections(torch.autograd.Function):
	@staticmethod
	def forward(ctx, verts, planes, faces, vf_off, vf_items):
		L = _lib.lib()
		verts, planes = _c(verts), _c(planes)
		N, V, _ = verts.shape
		fb, F = (1, faces.shape[0]) if faces.dim() == 2 else faces.shape[:2]
		pb, P = (1, planes.shape[0]) if planes.dim() == 2 else planes.shape[:2]
		nbytes = L.find_plane_sections_ws_bytes(N, F, P, 0)
		if nbytes < 0:
			check(-1, 'find_plane_sections_ws_bytes')
		ws = torch.empty(nbytes // 8, device=verts.device, dtype=torch.float64)   # a double and a count per workgroup and plane
		perimeter = torch.empty(N, P, device=verts.device, dtype=torch.float32)
		count = torch.empty(N, P, device=verts.device, dtype=torch.int32)
		check(L.find_plane_sections_fwd(ptr(verts), ptr(faces), fb, ptr(planes), pb, N, V, F, P, ptr(perimeter), ptr(count), ptr(ws), ws.numel() * 8,
										current_stream(verts.device)), 'find_plane_sections_fwd')
		ctx.dims = (N, V, F, P, fb, pb)
		ctx.save_for_backward(verts, planes, faces, vf_off, vf_items)
		ctx.mark_non_differentiable(count)
		return perimeter, count

	@staticmethod
	def backward(ctx, g, _gc):
		verts, planes, faces, vf_off, vf_items = ctx.saved_tensors
		N, V, F, P, fb, pb = ctx.dims
		if vf_off is None:
			raise RuntimeError('find_amd.measure: the forward ran without the corner tables (no input required a gradient)')
		L = _lib.lib()
		nbytes = L.find_plane_sections_ws_bytes(N, F, P, 1)
		ws = torch.empty(nbytes // 8, device=verts.device, dtype=torch.float64)   # nine floats per face, a double per workgroup and plane
		d_verts = torch.empty_like(verts)
		d_offset = torch.empty(pb, P, device=verts.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
		check(L.find_plane_sections_bwd(ptr(verts), ptr(faces), fb, ptr(vf_off), ptr(vf_items), ptr(planes), pb, N, V, F, P, ptr(_c(g)), ptr(d_verts),
										ptr(d_offset), ptr(ws), ws.numel() * 8, current_stream(verts.device)), 'find_plane_sections_bwd')
		d_planes = None
		if d_offset is not None:   # the normals are taken as given: no gradient
			d_planes = torch.zeros_like(planes)
			d_planes[..., 3] = d_offset.reshape(planes.shape[:-1])
		return d_verts, d_planes, None, None, None


class _Extents(torch.autograd.Function):
	@staticmethod
	def forward(ctx, verts, dirs, v_len):
		verts = _c(verts)
		N, V, _ = verts.shape
		D = dirs.shape[0]
		lo = torch.empty(N, D, device=verts.device, dtype=torch.float32)
		hi = torch.empty(N, D, device=verts.device, dtype=torch.float32)
		arg_lo = torch.empty(N, D, device=verts.device, dtype=torch.int32)
		arg_hi = torch.empty(N, D, device=verts.device, dtype=torch.int32)
		check(_lib.lib().find_extents_fwd(ptr(verts), ptr(v_len), ptr(dirs), N, V, D, ptr(lo), ptr(hi), ptr(arg_lo), ptr(arg_hi), current_stream(verts.device)),
			  'find_extents_fwd')
		ctx.dims = (N, V, D)
		ctx.save_for_backward(dirs, arg_lo, arg_hi)
		ctx.mark_non_differentiable(arg_lo, arg_hi)
		return lo, hi, arg_lo, arg_hi

	@staticmethod
	def backward(ctx, g_lo, g_hi, _a, _b):
		dirs, arg_lo, arg_hi = ctx.saved_tensors
		N, V, D = ctx.dims
		d_verts = torch.zeros(N, V, 3, device=dirs.device, dtype=torch.float32)   # added into
		check(_lib.lib().find_extents_bwd(ptr(_c(g_lo)), ptr(_c(g_hi)), ptr(arg_lo), ptr(arg_hi), ptr(dirs), N, V, D, ptr(d_verts), current_stream(dirs.device)),
			  'find_extents_bwd')
		return d_verts, None, None


# vertex -> corner tables of a SHARED faces tensor, built once per tensor object (as functional.MeshTopology.get keeps its own), by the
# device sort of functional._corner_tables: rows of -1 and indices outside [0, V) are allowed
_tables = {}


def _shared_tables(faces, f32, n_verts):
	key = (id(faces), int(n_verts))
	ent = _tables.get(key)
	if ent is not None and ent[0]() is faces and ent[1] == int(faces._version):
		return ent[2]
	if len(_tables) > 16:
		_tables.clear()
	off, items = _corner_tables(f32[None], n_verts)
	_tables[key] = (weakref.ref(faces), int(faces._version), (off, items))
	return off, items


def plane_sections(verts, faces, planes, return_count=False):
	"""Perimeter (N, P) fp32 of the polyline in which plane p cuts mesh n.  verts (N, V, 3); faces (F, 3) shared or (N, F, 3) per mesh, any
	integer dtype -- a row with a -1, an index outside [0, V) or a repeated vertex contributes nothing; planes (P, 4) shared or (N, P, 4), rows
	(nx, ny, nz, d) of the plane n . v = d with the normal taken as given (normalise it), 1 <= P <= 64.  With return_count also the (N, P)
	int32 number of faces that cross.  Differentiable in the vertices and in the offsets planes[..., 3]; the normals receive no gradient
	(zeros).  A plane that misses gives 0; one that touches the mesh at a vertex gives 0 with a zero gradient."""
	if verts.dim() != 3 or verts.shape[-1] != 3 or verts.shape[0] < 1 or verts.shape[1] < 1:
		raise ValueError(f'find_amd.measure.plane_sections: verts (N, V, 3) expected, got {tuple(verts.shape)}')
	N, V, _ = verts.shape
	if faces.dim() not in (2, 3) or faces.shape[-1] != 3 or faces.is_floating_point() or faces.shape[-2] < 1:
		raise ValueError(f'find_amd.measure.plane_sections: integer faces (F, 3) or (N, F, 3) expected, got {tuple(faces.shape)} {faces.dtype}')
	if faces.dim() == 3 and faces.shape[0] not in (1, N):
		raise ValueError(f'find_amd.measure.plane_sections: {faces.shape[0]} face lists for {N} meshes')
	if planes.dim() not in (2, 3) or planes.shape[-1] != 4 or not 1 <= planes.shape[-2] <= MAX_PLANES:
		raise ValueError(f'find_amd.measure.plane_sections: planes (P, 4) or (N, P, 4), 1 <= P <= {MAX_PLANES}, expected, got {tuple(planes.shape)}')
	if planes.dim() == 3 and planes.shape[0] not in (1, N):
		raise ValueError(f'find_amd.measure.plane_sections: {planes.shape[0]} plane lists for {N} meshes')
	_require_gpu(verts, faces, planes)
	f32 = _faces_i32(faces)
	off = items = None
	if torch.is_grad_enabled() and (verts.requires_grad or planes.requires_grad):   # the backward gathers through them
		off, items = _shared_tables(faces, f32, V) if faces.dim() == 2 else _corner_tables(f32, V)
	perimeter, count = _PlaneSections.apply(verts, planes, f32, off, items)
	return (perimeter, count) if return_count else perimeter


def extents(verts, dirs, v_len=None, return_index=False):
	"""(lo, hi), each (N, D) fp32: the minimum and maximum of dir_d . v over the first v_len[n] vertices (all V without v_len) of verts
	(N, V, 3); dirs (D, 3), 1 <= D <= 8, taken as given.  With return_index also (arg_lo, arg_hi) (N, D) int32, the vertices where they are
	taken: among equal values the smallest index.  A mesh with v_len 0 gets 0, 0, -1, -1; rows at or past v_len are never read.
	Differentiable in the vertices: the gradient lands on the arg vertices."""
	if verts.dim() != 3 or verts.shape[-1] != 3 or verts.shape[0] < 1 or verts.shape[1] < 1:
		raise ValueError(f'find_amd.measure.extents: verts (N, V, 3) expected, got {tuple(verts.shape)}')
	dirs = torch.as_tensor(dirs, dtype=torch.float32, device=verts.device)
	if dirs.dim() != 2 or dirs.shape[-1] != 3 or not 1 <= dirs.shape[0] <= MAX_DIRS:
		raise ValueError(f'find_amd.measure.extents: dirs (D, 3), 1 <= D <= {MAX_DIRS}, expected, got {tuple(dirs.shape)}')
	if v_len is not None and (v_len.dim() != 1 or v_len.shape[0] != verts.shape[0] or v_len.is_floating_point()):
		raise ValueError(f'find_amd.measure.extents: v_len ({verts.shape[0]}) integers expected, got {tuple(v_len.shape)} {v_len.dtype}')
	_require_gpu(verts)
	if v_len is not None:
		v_len = v_len.to(device=verts.device, dtype=torch.int32).contiguous()
	lo, hi, arg_lo, arg_hi = _Extents.apply(verts, dirs.detach().contiguous(), v_len)
	return (lo, hi, arg_lo, arg_hi) if return_index else (lo, hi)


def _unit(axis, what):
	a = tuple(float(x) for x in axis)
	n = sum(x * x for x in a) ** 0.5
	if len(a) != 3 or not n > 0:
		raise ValueError(f'FootSpec: {what} must be a non-zero 3-vector, got {axis!r}')
	return tuple(x / n for x in a)


@dataclasses.dataclass(frozen=True)
class FootSpec:
	"""What foot_measurements measures.  length_axis, width_axis: directions in the frame of the vertices (the dataset's: x towards the toes,
	y across the foot), normalised here.  Length and width are the extents of the vertices along them.  girths: (name, fraction) pairs; a girth
	is the perimeter of the section by the plane normal to the length axis at that fraction of the foot's OWN length from the heel,
	d = lo + fraction * (hi - lo) along the length axis.  The defaults -- ball at 0.68, instep at 0.50 of the length -- are this project's
	convention, not a standard: they are configurable.  girth_kind: 'section' (the default) measures that perimeter, plane_sections';
	'tape' measures the perimeter of the section's convex hull, girth.section_hulls' -- what a tape reads: a section perimeter is at least the
	tape's number, and larger wherever the sole is concave or the plane cuts the toes into separate loops.  Not claimed by either: the ISO
	ball-girth plane through the two metatarsal heads (a tilted plane from landmarks); girth.plane_through builds that plane for a caller
	who knows the landmark vertices."""
	length_axis: tuple = (1., 0., 0.)
	width_axis: tuple = (0., 1., 0.)
	girths: tuple = (('ball', 0.68), ('instep', 0.50))
	girth_kind: str = 'section'

	def __post_init__(self):
		object.__setattr__(self, 'length_axis', _unit(self.length_axis, 'length_axis'))
		object.__setattr__(self, 'width_axis', _unit(self.width_axis, 'width_axis'))
		girths = tuple((str(n), float(f)) for n, f in self.girths)
		if len(girths) > MAX_PLANES or not all(0. <= f <= 1. for _, f in girths) or len({n for n, _ in girths}) != len(girths):
			raise ValueError(f'FootSpec: at most {MAX_PLANES} girths (name, fraction in [0, 1]) of distinct names, got {self.girths!r}')
		object.__setattr__(self, 'girths', girths)
		if self.girth_kind not in ('section', 'tape'):
			raise ValueError(f"FootSpec: girth_kind must be 'section' or 'tape', got {self.girth_kind!r}")

	@property
	def names(self):
		return ('length', 'width') + tuple(f'{n}_girth' for n, _ in self.girths)


@functools.lru_cache(maxsize=32)
def _spec_tensors(spec, device):
	"""The spec's two axes (2, 3) and girth fractions (G) on `device`, uploaded once: a call in a fitting loop copies nothing from the host."""
	return (torch.tensor([spec.length_axis, spec.width_axis], device=device, dtype=torch.float32),
			torch.tensor([f for _, f in spec.girths], device=device, dtype=torch.float32))


def foot_measurements(verts, faces, spec=FootSpec(), v_len=None):
	"""(values (N, M) fp32 in metres, names): with the default spec ('length', 'width', 'ball_girth', 'instep_girth').  verts (N, V, 3) registered
	vertices, faces (F, 3) or (N, F, 3) (-1 padded), v_len (N) the vertex counts of a padded batch.  One extents call and one plane_sections
	call (girth_kind 'tape': one girth.section_hulls call); the gradient reaches the vertices directly and, for the girths, through the offsets
	of their planes (the heel and toe vertices)."""
	if not isinstance(spec, FootSpec):
		raise ValueError(f'find_amd.measure.foot_measurements: spec must be a FootSpec, got {type(spec).__name__}')
	dirs, frac = _spec_tensors(spec, verts.device)
	lo, hi = extents(verts, dirs, v_len)
	size = hi - lo
	cols = [size]
	if spec.girths:
		N, G = verts.shape[0], len(spec.girths)
		d = lo[:, :1] + frac[None] * size[:, :1]
		planes = torch.cat([dirs[0].expand(N, G, 3), d[..., None]], dim=-1)
		if spec.girth_kind == 'tape':
			from .girth import section_hulls   # (a module of its own: it allocates)
			cols.append(section_hulls(verts, faces, planes))
		else:
			cols.append(plane_sections(verts, faces, planes))
	return torch.cat(cols, dim=1), spec.names


def of_meshes(meshes, spec=None):
	"""foot_measurements of a Meshes (shared or ragged, -1 padded faces), its vertex counts as v_len."""
	faces = meshes.faces_shared()
	if faces is None:
		faces = meshes.faces_padded()
	return foot_measurements(meshes.verts_padded(), faces, FootSpec() if spec is None else spec, meshes.num_verts_per_mesh())
