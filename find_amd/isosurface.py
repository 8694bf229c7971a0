"""From a field on a grid back to a mesh, on the HIP path: iso-surface extraction by surface nets (find_surface_nets_count / _emit / _bwd,
csrc/surface_nets.hip; Gibson 1998, "naive dual contouring") and what follows from it and find_amd.inside -- the watertight remesh of a scan
or a prediction that is open at the ankle, and offset surfaces ("the foot grown by 3 mm").  Not in the reference.  One vertex per grid cell
the level set passes through, one quad (two triangles) per lattice edge whose ends lie on different sides; include/find_hip.h writes the
definition out.  The result is closed wherever the surface stays off the grid boundary (every edge in an even number of triangles) and
2-manifold wherever no lattice face has four sign changes -- two inside samples diagonal on a face give an edge with four triangles; smooth
shapes at a sensible resolution do not do that.  There is no CPU or eager fallback: CPU tensors raise.  Outputs are torch.empty, which the
kernels write in full, and the workspace comes from functional._ws (tests/test_gpu_isosurface.py runs the module over poisoned memory)."""
import torch

from . import _lib
from . import functional as FN
from . import inside
from ._lib import check, current_stream, ptr

BLOCK_CELLS = 256   # FIND_SURFACE_NETS_BLOCK: the cells (and samples) one workgroup counts and ranks
BOUNDARY, VERTS_OVERFLOW, FACES_OVERFLOW, NON_FINITE = 1, 2, 4, 8   # the bits of `status`
_CHUNK_POINTS = 1 << 19   # grid samples of all meshes together whose distance is taken at a time


def _check_values(who, values):
	if values.dim() != 4 or any(not 2 <= s <= 1024 for s in values.shape[1:]):
		raise RuntimeError(f'find_amd.isosurface.{who}: values (N, nx, ny, nz) with 2 .. 1024 samples per axis expected, got {tuple(values.shape)}')
	if not values.is_cuda:
		raise RuntimeError(f'find_amd.isosurface.{who}: the HIP path needs tensors on a ROCm device (got a CPU tensor); there is no CPU fallback')
	if values.dtype != torch.float32:
		raise RuntimeError(f'find_amd.isosurface.{who}: fp32 values required, got {values.dtype}')


def _capacity(who, name, cap, limit):
	if cap is None:
		return None
	if not isinstance(cap, int) or isinstance(cap, bool) or not 0 <= cap < limit:
		raise RuntimeError(f'find_amd.isosurface.{who}: {name} must be an int in [0, {limit}), got {cap!r}')
	return cap


class _SurfaceNets(torch.autograd.Function):
	"""(g, faces, v_len, f_len, status) of find_surface_nets_count + _emit; backward: find_surface_nets_bwd, d L / d values and -- `iso` a
	tensor -- d L / d iso summed over the meshes.  The faces, the lengths and the status are constants."""

	@staticmethod
	def forward(ctx, values, iso_tensor, iso, max_verts, max_faces):
		L = _lib.lib()
		values = values.detach().contiguous()
		N, nx, ny, nz = values.shape
		dev = values.device
		st = current_stream(dev)
		ws = FN._ws(L.find_surface_nets_ws_bytes(N, nx, ny, nz), dev)
		v_len = torch.empty(N, dtype=torch.int64, device=dev)
		f_len = torch.empty(N, dtype=torch.int64, device=dev)
		status = torch.empty(N, dtype=torch.int32, device=dev)
		check(L.find_surface_nets_count(ptr(values), iso, N, nx, ny, nz, ptr(v_len), ptr(f_len), ptr(status), ptr(ws), ws.numel(), st), 'find_surface_nets_count')
		if max_verts is None or max_faces is None:
			counts = torch.stack([v_len, f_len]).cpu()   # (the one read-back)
			need_v, need_f = (int(counts[0].max()), int(counts[1].max())) if N else (0, 0)
			max_verts = need_v if max_verts is None else max_verts
			max_faces = need_f if max_faces is None else max_faces
		g = torch.empty(N, max_verts, 3, dtype=torch.float32, device=dev)
		faces = torch.empty(N, max_faces, 3, dtype=torch.int32, device=dev)
		check(L.find_surface_nets_emit(ptr(values), iso, N, nx, ny, nz, ptr(v_len), ptr(f_len), max_verts, max_faces, ptr(g) if g.numel() else None,
									   ptr(faces) if faces.numel() else None, ptr(status), ptr(ws), ws.numel(), st), 'find_surface_nets_emit')
		ctx.save_for_backward(values, ws)
		ctx.iso, ctx.iso_is_tensor = iso, iso_tensor is not None
		ctx.mark_non_differentiable(faces, v_len, f_len, status)
		return g, faces, v_len, f_len, status

	@staticmethod
	def backward(ctx, grad_g, *unused):
		L = _lib.lib()
		values, ws = ctx.saved_tensors   # (the cell -> vertex map is the head of the emit call's workspace)
		N, nx, ny, nz = values.shape
		dev = values.device
		grad_g = grad_g.contiguous().float()
		grad_values = torch.empty_like(values)
		grad_iso = torch.empty(N, dtype=torch.float32, device=dev)
		bws = FN._ws(L.find_surface_nets_bwd_ws_bytes(N, nx, ny, nz), dev)
		check(L.find_surface_nets_bwd(ptr(values), ctx.iso, N, nx, ny, nz, ptr(ws), ptr(grad_g) if grad_g.numel() else None, grad_g.shape[1], ptr(grad_values),
									  ptr(grad_iso), ptr(bws), bws.numel(), current_stream(dev)), 'find_surface_nets_bwd')
		return grad_values, (grad_iso.sum() if ctx.iso_is_tensor else None), None, None, None


def extract_surface(values, origin, spacing, iso=0.0, max_verts=None, max_faces=None):
	"""The level set values == iso as an indexed triangle mesh (surface nets).  values (N, nx, ny, nz) float32, indexed [n, i, j, k] with i along
	x, 2 .. 1024 samples per axis; sample (i, j, k) sits at origin + (i + 0.5, j + 0.5, k + 0.5) * spacing, the convention of inside.grid_points
	(origin, spacing: (N, 3) or (3,)).  A sample is inside iff value < iso (exactly; value == iso and non-finite values are outside).
	Returns (verts (N, Vmax, 3) float32, faces (N, Fmax, 3) int32 with -1 rows past f_len, v_len (N) int64, f_len (N) int64, status (N) int32).
	Vertices come in flat cell order, faces in flat sample order and +x, +y, +z per sample, normals from inside to outside; rows of verts past
	v_len are origin + 0.5 spacing.  status bits: 1 (BOUNDARY) the surface leaves the grid and the mesh is open there; 2 / 4 (VERTS_OVERFLOW /
	FACES_OVERFLOW) a capacity was too small: v_len and f_len are still the true counts, that mesh's rows are unspecified; 8 (NON_FINITE).

	With max_verts or max_faces None the counts are READ BACK once between the count and the emit call (one host synchronisation), and Vmax /
	Fmax are the batch maxima.  With both given nothing is read back and an overflow shows in status.  `iso` is a float, or a 0-dim tensor
	(read back once) that then receives a gradient.  Differentiable in values and iso through find_surface_nets_bwd and in origin and spacing
	through torch; the topology is a constant.  Two calls agree bit for bit; a mesh does not depend on the rest of the batch."""
	who = 'extract_surface'
	_check_values(who, values)
	N = values.shape[0]
	max_verts = _capacity(who, 'max_verts', max_verts, 1 << 30)
	max_faces = _capacity(who, 'max_faces', max_faces, 1 << 33)
	dev = values.device
	origin, spacing = (torch.as_tensor(t, dtype=torch.float32, device=dev) if not torch.is_tensor(t) else t for t in (origin, spacing))
	for name, t in (('origin', origin), ('spacing', spacing)):
		if t.shape not in ((3,), (N, 3)) or not t.is_cuda or t.dtype != torch.float32:
			raise RuntimeError(f'find_amd.isosurface.{who}: {name} (3,) or ({N}, 3) float32 on the device expected, got {tuple(t.shape)} {t.dtype} on {t.device}')
	iso_tensor = iso if torch.is_tensor(iso) else None
	if iso_tensor is not None and iso_tensor.numel() != 1:
		raise RuntimeError(f'find_amd.isosurface.{who}: one iso per call, got {tuple(iso_tensor.shape)}')
	g, faces, v_len, f_len, status = _SurfaceNets.apply(values, iso_tensor, float(iso if iso_tensor is None else iso_tensor.detach()), max_verts, max_faces)
	verts = origin.expand(N, 3)[:, None, :] + (g + 0.5) * spacing.expand(N, 3)[:, None, :]
	return verts, faces, v_len, f_len, status


def field_grid(verts, faces, res=64, offset=0.0, pad=0.005, level=0.5):
	"""inside.signed_distance of each mesh on a res^3 grid that holds the level set sdf == offset with a layer to spare.  verts (N, V, 3), faces
	as in inside.winding_number.  The vertices' box is grown by max(offset, 0) + pad to (lo, hi); spacing = (hi - lo) / (res - 3) and
	origin = lo - 1.5 spacing, so samples 1 .. res - 2 run from lo to hi and the outermost layer lies a full spacing beyond: certainly outside
	the level, so the extracted surface is closed.  (A grid made like occupancy_grid's has its first sample half a cell INSIDE the padded box.)
	res >= 4.  Returns (sdf (N, res, res, res) float32, origin (N, 3), spacing (N, 3)); no gradient; the samples are generated and consumed a
	chunk at a time."""
	who = 'field_grid'
	try:
		inside._check(who, verts, verts, faces)
	except RuntimeError as e:
		raise RuntimeError(str(e).replace('find_amd.inside.', 'find_amd.isosurface.')) from None
	if not isinstance(res, int) or isinstance(res, bool) or not 4 <= res <= 1024:
		raise RuntimeError(f'find_amd.isosurface.{who}: res must be an int in [4, 1024], got {res!r}')
	with torch.no_grad():
		lo, extent = inside._box(who, [verts], None, max(float(offset), 0.) + pad)
		spacing = extent / (res - 3)
		origin = lo - 1.5 * spacing
		N = verts.shape[0]
		sdf = torch.empty(N, res ** 3, dtype=torch.float32, device=verts.device)
		chunk = max(1 << 10, _CHUNK_POINTS // N)
		for start in range(0, res ** 3, chunk):
			stop = min(start + chunk, res ** 3)
			sdf[:, start:stop] = inside.signed_distance(inside.grid_points(origin, spacing, res, start, stop), verts, faces, level=level)[0]
	return sdf.view(N, res, res, res), origin, spacing


def remesh(verts, faces, res=64, offset=0.0, pad=0.005, level=0.5, as_meshes=False):
	"""field_grid followed by extract_surface(iso=offset): with offset 0 the watertight remesh of a scan or a prediction, open ones included
	(the winding number closes the hole about flat); with offset d the surface at distance d outside (d < 0: inside) a CLOSED mesh -- across
	the virtual cap of an open one the sign flips while the distance does not vanish, a jump in the field, and the offset surface there is not
	manifold.  Returns extract_surface's tuple, or -- as_meshes -- a structures.Meshes.  No gradient reaches verts (the field is sampled
	without one)."""
	sdf, origin, spacing = field_grid(verts, faces, res, offset, pad, level)
	out = extract_surface(sdf, origin, spacing, iso=float(offset))
	if not as_meshes:
		return out
	from .structures import Meshes
	v, f, v_len, f_len, _ = out
	return Meshes(v, f.long(), _num_verts=v_len.tolist(), _num_faces=f_len.tolist())
