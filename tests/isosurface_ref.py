"""A vectorised numpy restatement of surface nets as include/find_hip.h defines them (find_surface_nets_count / _emit), a torch float64 version
of the vertices with the topology held fixed (for gradients by autograd), the fields the tests extract, and mesh helpers.  A helper of
test_isosurface_host.py and test_gpu_isosurface.py, not a test.

A sample is inside iff value < iso (float32, exactly) and finite.  Cell (i, j, k) has corners c = 4 di + 2 dj + dk; its 12 edges (a, b), a < b,
differ in one bit and are taken in lexicographic order; on a crossing edge t = (iso - v_a) / (v_b - v_a) (0.5 if not finite) and
p = corner_a + t (corner_b - corner_a); g = (i, j, k) + (sum of p in edge order) / n.  The per-vertex arithmetic runs in `dtype`; sides, and with
them the order of vertices (flat cell order) and faces (flat sample order, +x +y +z per sample), never depend on it."""
import numpy as np
import torch

EDGES = [(a, b) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count('1') == 1]   # lexicographic
AXIS = {4: 0, 2: 1, 1: 2}   # b - a -> the edge's axis
QUAD = ((-1, -1), (0, -1), (0, 0), (-1, 0))
BOUNDARY, VERTS_OVERFLOW, FACES_OVERFLOW, NON_FINITE = 1, 2, 4, 8


def sides(values, iso):
	v = np.asarray(values, np.float32)
	with np.errstate(invalid='ignore'):
		return np.isfinite(v) & (v < np.float32(iso))


def _corner(arr, c):
	nx, ny, nz = arr.shape
	di, dj, dk = (c >> 2) & 1, (c >> 1) & 1, c & 1
	return arr[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk]


class Result:
	"""g (V, 3) in `dtype`, grid coordinates; faces (F, 3) int64; cellmap (nx-1, ny-1, nz-1) int64 (-1: no vertex); status (bits 1 and 8);
	ambiguous: the number of lattice faces with four sign changes (where the result is not 2-manifold)."""


def extract(values, iso=0.0, dtype=np.float64):
	values = np.asarray(values, np.float32)
	assert values.ndim == 3 and min(values.shape) >= 2
	dtype = np.dtype(dtype).type
	nx, ny, nz = values.shape
	iso32 = np.float32(iso)
	ins = sides(values, iso32)
	cin = [_corner(ins, c) for c in range(8)]
	cnt = sum(c.astype(np.int64) for c in cin)
	active = (cnt > 0) & (cnt < 8)
	r = Result()
	r.cellmap = np.full(active.shape, -1, np.int64)
	r.cellmap[active] = np.arange(int(active.sum()))   # (C order: flat cell order)
	idx = np.argwhere(active)
	V = len(idx)
	cv = [_corner(values, c)[active].astype(dtype) for c in range(8)]
	ci = [c[active] for c in cin]
	s, n = np.zeros((V, 3), dtype), np.zeros(V, np.int64)
	for a, b in EDGES:
		cross = ci[a] != ci[b]
		with np.errstate(all='ignore'):
			t = (dtype(iso32) - cv[a]) / (cv[b] - cv[a])
		t = np.where(np.isfinite(t), t, dtype(0.5))
		p = np.empty((V, 3), dtype)
		p[:] = [(a >> 2) & 1, (a >> 1) & 1, a & 1]
		p[:, AXIS[b - a]] = t
		s = s + np.where(cross[:, None], p, dtype(0))
		n += cross
	r.g = (idx.astype(dtype) + s / n[:, None].astype(dtype)).astype(dtype)
	assert r.g.dtype == dtype
	keys, quads = [], []
	shape = values.shape
	for ax in range(3):
		u, w = (ax + 1) % 3, (ax + 2) % 3
		lo, hi = [None] * 3, [None] * 3
		lo[ax], hi[ax] = slice(0, shape[ax] - 1), slice(1, shape[ax])
		lo[u] = hi[u] = slice(1, shape[u] - 1)
		lo[w] = hi[w] = slice(1, shape[w] - 1)
		a_in, b_in = ins[tuple(lo)], ins[tuple(hi)]
		cross = a_in != b_in
		smp = np.argwhere(cross)
		if len(smp) == 0:
			continue
		smp[:, u] += 1
		smp[:, w] += 1
		q = []
		for du, dw in QUAD:
			c = smp.copy()
			c[:, u] += du
			c[:, w] += dw
			q.append(r.cellmap[c[:, 0], c[:, 1], c[:, 2]])
		q = np.stack(q, -1)
		assert (q >= 0).all()
		q = np.where(a_in[cross][:, None], q, q[:, ::-1])
		keys.append(((smp[:, 0] * ny + smp[:, 1]) * nz + smp[:, 2]) * 3 + ax)
		quads.append(q)
	if quads:
		q = np.concatenate(quads)[np.argsort(np.concatenate(keys), kind='stable')]
		r.faces = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3)
	else:
		r.faces = np.zeros((0, 3), np.int64)
	edge = np.zeros(active.shape, bool)
	for axis in range(3):
		sl = [slice(None)] * 3
		for at in (0, -1):
			sl[axis] = at
			edge[tuple(sl)] = True
	r.status = (BOUNDARY if (active & edge).any() else 0) | (0 if np.isfinite(values).all() else NON_FINITE)
	r.ambiguous = 0
	for axis in range(3):
		u, w = (axis + 1) % 3, (axis + 2) % 3

		def at(du, dw):
			sl = [slice(None)] * 3
			sl[u] = slice(du, shape[u] - 1 + du)
			sl[w] = slice(dw, shape[w] - 1 + dw)
			return ins[tuple(sl)]
		r.ambiguous += int(((at(0, 0) == at(1, 1)) & (at(0, 1) == at(1, 0)) & (at(0, 0) != at(0, 1))).sum())
	return r


def g_torch(values, iso):
	"""g (V, 3) as a torch function of values (nx, ny, nz) and iso (0-dim), both float64 (holding float32 numbers) or float32: the sides, the
	active cells and the crossing edges are decided once on the float32 numbers and held fixed, so autograd gives d g / d values and
	d g / d iso of the definition."""
	v32 = values.detach().float().cpu().numpy()
	ins = torch.from_numpy(sides(v32, np.float32(float(iso.detach()))))
	cin = [_corner(ins, c) for c in range(8)]
	cnt = sum(c.long() for c in cin)
	active = (cnt > 0) & (cnt < 8)
	idx = active.nonzero().to(values.dtype)
	cv = [_corner(values, c)[active] for c in range(8)]
	ci = [c[active] for c in cin]
	s, n = torch.zeros(len(idx), 3, dtype=values.dtype), torch.zeros(len(idx), dtype=values.dtype)
	for a, b in EDGES:
		cross = ci[a] != ci[b]
		d = torch.where(cross, cv[b] - cv[a], torch.ones_like(cv[a]))
		t = (iso - cv[a]) / d
		assert torch.isfinite(t[cross]).all(), 'the gradient cases have no degenerate edge'
		p = torch.tensor([(a >> 2) & 1, (a >> 1) & 1, a & 1], dtype=values.dtype).repeat(len(idx), 1)
		p = torch.where(torch.arange(3) == AXIS[b - a], t[:, None], p)
		s = s + torch.where(cross[:, None], p, torch.zeros_like(p))
		n = n + cross.to(values.dtype)
	return idx + s / n[:, None]


# ------------------------------------------------------------------ mesh helpers
def _valid(faces):
	faces = np.asarray(faces).reshape(-1, 3)
	return faces[(faces >= 0).all(1)].astype(np.int64)


def directed_edge_counts(faces):
	f = _valid(faces)
	e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
	return np.unique(e, axis=0, return_counts=True)[1] if len(e) else np.zeros(0, np.int64)


def undirected_edge_counts(faces):
	f = _valid(faces)
	e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
	return np.unique(e, axis=0, return_counts=True)[1] if len(e) else np.zeros(0, np.int64)


def watertight(faces):
	"""Every undirected edge in exactly two triangles, once in each direction."""
	u, d = undirected_edge_counts(faces), directed_edge_counts(faces)
	return len(u) > 0 and bool((u == 2).all()) and bool((d == 1).all())


def closed(faces):
	"""Every undirected edge in an even number of triangles."""
	return bool((undirected_edge_counts(faces) % 2 == 0).all())


def euler(faces):
	f = _valid(faces)
	return len(np.unique(f)) - len(undirected_edge_counts(f)) + len(f)


def exact_volume(verts, faces):
	v, f = np.asarray(verts, np.float64), _valid(faces)
	return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.)


# ------------------------------------------------------------------ the fields, from formulas
def sample_points(shape, half):
	"""(nx, ny, nz, 3) float64: sample (i, j, k) of a grid over the box +-half at origin + (i + 0.5, j + 0.5, k + 0.5) spacing; and origin, spacing."""
	half = np.broadcast_to(np.asarray(half, np.float64), (3,))
	spacing = 2 * half / np.asarray(shape)
	ijk = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing='ij'), -1)
	return -half + (ijk + 0.5) * spacing, -half, spacing


def _sphere(n, r=0.04, half=0.06):
	p, _, _ = sample_points((n, n, n), half)
	return np.sqrt((p ** 2).sum(-1)) - r


def _ellipsoid(shape=(9, 17, 33), axes=(0.02, 0.04, 0.1)):
	p, _, _ = sample_points(shape, np.asarray(axes) + 0.02)
	return np.sqrt(((p / np.asarray(axes)) ** 2).sum(-1)) - 1.


def _torus():
	p, _, _ = sample_points((32, 32, 16), (0.06, 0.06, 0.03))
	return np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - 0.035) ** 2 + p[..., 2] ** 2) - 0.012


def _two_spheres():
	p, _, _ = sample_points((24, 24, 24), 0.06)
	return np.minimum(*[np.sqrt(((p - [x, 0, 0]) ** 2).sum(-1)) - 0.02 for x in (-0.03, 0.03)])


def _one_sample():
	v = np.ones((3, 3, 3))
	v[1, 1, 1] = -1.
	return v


def _one_cell():
	v = np.ones((2, 2, 2))
	v[0, 0, 0] = -0.5
	return v


def _plane(shape=(6, 5, 7)):
	i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
	return i + 0.25 * j - 0.125 * k - 2.3


def _checkerboard():
	v = np.ones((4, 4, 4))
	v[1, 1, 1] = v[1, 2, 2] = -1.
	return v


_MAKERS = {'sphere8': lambda: _sphere(8), 'sphere16': lambda: _sphere(16), 'sphere32': lambda: _sphere(32), 'ellipsoid': _ellipsoid, 'torus': _torus,
		   'two_spheres': _two_spheres, 'one_sample': _one_sample, 'one_cell': _one_cell, 'plane': _plane, 'checkerboard': _checkerboard}
CASES = tuple(_MAKERS)
SMOOTH = {'sphere8': 2, 'sphere16': 2, 'sphere32': 2, 'ellipsoid': 2, 'torus': 0, 'two_spheres': 4}   # case -> Euler characteristic
_FIELDS, _RESULTS = {}, {}


def field(name):
	"""The case's samples, float32 (nx, ny, nz), made once; iso is 0."""
	if name not in _FIELDS:
		_FIELDS[name] = np.ascontiguousarray(_MAKERS[name](), np.float32)
	return _FIELDS[name]


def result(name, dtype=np.float64):
	"""extract(field(name)) in `dtype`, computed once."""
	key = (name, np.dtype(dtype).name)
	if key not in _RESULTS:
		_RESULTS[key] = extract(field(name), 0.0, dtype)
	return _RESULTS[key]
