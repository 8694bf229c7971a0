"""Winding numbers on the MI355X: find_winding_fwd through find_amd.inside against the numpy restatement of the definition (tests/inside_ref.py)
in float64 on the same fp32 inputs, and what is built on it: the signed distance, occupancy grids, grid volumes, the volumetric IoU,
losses.PenetrationLoss and eval_3d_metrics(volume=).

Margins: none is a constant of the code under test.  Every float comparison follows _held of tests/test_gpu_arap.py: the restatement is also
evaluated in float32 on the CPU; with e32 its worst error against float64 over the case's tensor, the HIP result must lie within
max(4 e32, 2 ulp of the largest value) of the float64 one.  Each case prints its figures (DESIGN 7.14 records the worst).  A case's queries
are box-uniform points (the mesh's box grown by 2 cm), every vertex of the mesh (a zero length on every incident face) and face centroids
(in the face's plane up to the centroid's own rounding: det is 0 or a rounding error of either sign, and w jumps by 1 across the face -- there
e32 is of order 1, which is why the box points and the vertices are ALSO held on their own).

Shapes, the smallest that cross each boundary: F = 1 (the octant), 4 (a tetrahedron), 128 and 2000 (ellipsoids (4, 16), (25, 40)), 13 776
(template(6890), P = 5000, N = 2, the second mesh open and its faces -1 padded); the kernel stages tiles of 512 faces, a wave sums 128 and a
chunk is 1024: F = 127 .. 129, 511 .. 513, 1023 .. 1025, 2047 .. 2049 (faces taken off the end of the template's list); a block owns 128
queries: P = 1, 127, 128, 129, 257; N = 1 and 3.  The chunks go to blocks of their own when ceil(P / 128) N < 2048 and F > 1024: every case
with more faces runs both ways (find_render_switches bit 8192 holds the split off) and must agree bit for bit.  Every case runs twice and must
repeat bit for bit.

One literal of the issue cannot hold in float32 and is replaced by what it stands for: |sdf|^2 == dist2 bit for bit (the square of a rounded
root is not the radicand).  Asserted instead: |sdf| is bit for bit sqrt(dist2) of point_face_distance, idx and bary are its outputs bit for
bit, and sdf^2 is within 2 ulp of dist2 (one rounding of the root, doubled by squaring, and one of the square)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import inside_ref as ref   # noqa: E402
import poison   # noqa: E402
import surface_ref as SR   # noqa: E402

WORST = {}   # quantity -> the worst e_hip / max(e32, ulp) seen (printed by the last test of the file)
_MESHES, _REFS = {}, {}


def _ulp(x):
	return float(np.spacing(np.float32(abs(float(x)))))


def _held(name, hip, ref64, ref32, kind=None):
	hip, ref64, ref32 = (torch.as_tensor(np.asarray(t)).detach().double().cpu() if not torch.is_tensor(t) else t.detach().double().cpu() for t in (hip, ref64, ref32))
	assert hip.shape == ref64.shape, (name, hip.shape, ref64.shape)
	e_hip = (hip - ref64).abs().max().item()
	e32 = (ref32 - ref64).abs().max().item()
	ulp = _ulp(ref64.abs().max().item())
	ratio = e_hip / max(e32, ulp)
	print(f'{name}: e_hip {e_hip:.3e}  e32 {e32:.3e}  ulp {ulp:.3e}  scale {ref64.abs().max().item():.3e}  e_hip / max(e32, ulp) {ratio:.2f}')
	if kind:
		WORST[kind] = max(WORST.get(kind, 0.), ratio)
	assert np.isfinite(e_hip) and e_hip <= max(4 * e32, 2 * ulp), (name, e_hip, e32, ulp)


# ------------------------------------------------------------------ inputs, the reference (computed once per case), the HIP run
def _mesh(key):
	"""'octant', 'tet', (rings, segs), 'template', ('open',): the template without the top 15 % of its faces; (n,): the template's first n faces."""
	if key not in _MESHES:
		from find_amd import synthetic
		if key == 'octant':
			v, f = (x.copy() for x in ref.OCTANT)
			v = v * 0.05
		elif key == 'tet':
			v = np.array([[0.03, 0.03, 0.03], [0.03, -0.03, -0.03], [-0.03, 0.03, -0.03], [-0.03, -0.03, 0.03]])
			f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
		elif key == 'template':
			v, f = (x.numpy() for x in synthetic.template(6890))
		elif key == ('open',):
			v, f = _mesh('template')
			f = ref.without_top(v, f, 0.15)
		elif len(key) == 1:
			v, f = _mesh('template')
			f = f[:key[0]]
		else:
			v, f = (x.numpy() for x in synthetic.ellipsoid_mesh(*key))
		_MESHES[key] = (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int64))
	return _MESHES[key]


def _queries(key, n_box, seed=0, n_verts=None, n_cent=None):
	"""(points (P, 3) float32, the slices of the box points, the vertices and the centroids)."""
	v, f = _mesh(key)
	verts = v[np.unique(f)][:n_verts]
	cent = ((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / np.float32(3)
	cent = cent[::max(1, len(cent) // n_cent)] if n_cent else cent
	pts = np.concatenate([ref.box_points(v[np.unique(f)], n_box, 0.02, seed), verts, cent]).astype(np.float32)
	return pts, slice(0, n_box), slice(n_box, n_box + len(verts)), slice(n_box + len(verts), len(pts))


def _refs(tag, points, verts, faces):
	"""(w64, w32) of the restatement, computed once per tag."""
	if tag not in _REFS:
		_REFS[tag] = tuple(ref.winding(points, verts, faces, dt) for dt in (np.float64, np.float32))
	return _REFS[tag]


def _t(x, dtype=torch.float32):
	return torch.as_tensor(np.asarray(x)).to(dtype).cuda()


def _hip(points, verts, faces, p_len=None, unsplit=False):
	"""w (N, P) of the HIP path as numpy, from two calls that must agree bit for bit.  points, verts: (N, ., 3) arrays; faces (F, 3) or (N, F, 3)."""
	from find_amd import _lib, inside
	p, v, f = _t(points), _t(verts), _t(faces, torch.int64)
	_lib.set_tuning('raster_ablate', 8192 if unsplit else 0)
	try:
		a = inside.winding_number(p, v, f, p_len)
		b = inside.winding_number(p, v, f, p_len)
		torch.cuda.synchronize()
	finally:
		_lib.set_tuning('raster_ablate', 0)
	assert a.shape == p.shape[:2] and a.dtype == torch.float32 and not a.requires_grad
	assert torch.equal(a, b), 'two runs differ'
	assert torch.isfinite(a).all()
	return a.cpu().numpy()


def _both_ways(points, verts, faces, p_len=None):
	"""The split decided by size and the unsplit path: the same bits."""
	a, b = _hip(points, verts, faces, p_len), _hip(points, verts, faces, p_len, unsplit=True)
	assert np.array_equal(a, b), 'the split and the unsplit path differ'
	return a


def _check_values(tag, key, n_box, **kw):
	v, f = _mesh(key)
	pts, box, at_verts, at_cent = _queries(key, n_box, **kw)
	w64, w32 = _refs(tag, pts, v, f)
	w = _both_ways(pts[None], v[None], f)[0]
	_held(f'{tag} box points', w[box], w64[box], w32[box], 'w')
	if at_verts.stop > at_verts.start:
		_held(f'{tag} at vertices', w[at_verts], w64[at_verts], w32[at_verts], 'w at vertices')
	_held(f'{tag} all queries', w, w64, w32)
	return pts, w, w64


# ------------------------------------------------------------------ values
@pytest.mark.parametrize('key', ['octant', 'tet', (4, 16), (25, 40)], ids=str)
def test_shapes(key):
	pts, w, w64 = _check_values(f'shape {key}', key, 300)
	if key == 'octant':   # from the origin the triangle subtends an octant; from its own corners nothing
		v, f = _mesh(key)
		o = _hip(np.concatenate([np.zeros((1, 3), np.float32), v])[None], v[None], f)[0]
		assert abs(abs(o[0]) - 0.125) <= 2 * _ulp(0.125) and (o[1:] == 0).all()
	if key in ('tet', (4, 16), (25, 40)):   # closed: 0 or 1 away from the surface, as the float64 restatement has it
		assert np.abs(w64[:300] - (w64[:300] > 0.5)).max() <= 1e-12


@pytest.mark.parametrize('F', [127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049])
def test_face_counts_on_each_side_of_a_wave_a_tile_and_a_chunk(F):
	_check_values(f'F = {F}', (F,), 200, n_verts=40, n_cent=40)


@pytest.mark.parametrize('P', [1, 127, 128, 129, 257])
def test_query_counts_on_each_side_of_a_block(P):
	key = (25, 40)
	v, f = _mesh(key)
	pts = np.stack([ref.box_points(v, 257, 0.02, seed)[:P] for seed in (11, 12, 13)])
	w = _both_ways(pts, np.stack([v, v, v]), f)
	big64, big32 = _refs('P cases', np.concatenate([ref.box_points(v, 257, 0.02, seed) for seed in (11, 12, 13)]), v, f)
	w64, w32 = (np.stack([b[257 * n:257 * n + P] for n in range(3)]) for b in (big64, big32))
	_held(f'P = {P}', w, w64, w32, 'w')
	# N = 1: the same rows
	assert np.array_equal(_hip(pts[:1], v[None], f)[0], w[0])


def _training_size():
	"""template(6890), P = 5000, N = 2: mesh 0 the closed template, mesh 1 the template without its top, its face list padded with -1 rows."""
	v, f = _mesh('template')
	_, fo = _mesh(('open',))
	faces = np.full((2, len(f), 3), -1, np.int64)
	faces[0], faces[1, :len(fo)] = f, fo
	pts = np.stack([ref.box_points(v, 5000, 0.02, 21), ref.box_points(v, 5000, 0.02, 22)])
	r = [_refs(f'training size {n}', pts[n], v, faces[n]) for n in range(2)]
	return v, faces, pts, np.stack([r[0][0], r[1][0]]), np.stack([r[0][1], r[1][1]])


def test_training_size_split_and_unsplit():
	v, faces, pts, w64, w32 = _training_size()
	w = _both_ways(pts, np.stack([v, v]), faces)
	_held('template(6890) closed', w[0], w64[0], w32[0], 'w')
	_held('template(6890) open', w[1], w64[1], w32[1], 'w')
	# the shared face list gives the closed mesh's row the same bits
	assert np.array_equal(_hip(pts[:1], v[None], faces[0])[0], w[0])


def test_ragged_points_padded_faces_and_a_mesh_without_faces():
	v, f = _mesh((25, 40))
	v2, f2 = _mesh((4, 16))
	V, F = len(v), len(f)
	verts = np.zeros((4, V, 3), np.float32)
	verts[0], verts[1, :len(v2)], verts[2], verts[3] = v, v2, v * np.float32(1.1), v
	faces = np.full((4, F + 3, 3), -1, np.int64)
	faces[0, :F] = f
	faces[0, F:] = [[0, 1, V], [5, -2, 7], [V + 3, 2, 1]]                       # out of range: do not count
	faces[1, 10:10 + len(f2)] = f2                                             # -1 rows before and after
	faces[2, :F] = f
	faces[3, :4] = [[-1, -1, -1], [0, 1, V], [-5, 2, 3], [1 << 30, 0, 1]]       # no face that counts
	P, p_len = 200, [200, 77, 0, 150]
	pts = np.stack([ref.box_points(v, P, 0.02, 30 + n) for n in range(4)])
	w = _both_ways(pts, verts, faces, torch.tensor(p_len))
	for n, (vn, fn) in enumerate(((v, f), (v2, f2), (v * np.float32(1.1), f), (v, f[:0]))):
		w64, w32 = _refs(f'ragged {n}', pts[n, :p_len[n]], vn, fn)
		assert (w[n, p_len[n]:] == 0).all(), n
		if p_len[n] and len(fn):
			_held(f'ragged mesh {n}', w[n, :p_len[n]], w64, w32, 'w')
			# ... the restatement skips the rows itself: handed the padded list, it says the same
			assert np.array_equal(ref.winding(pts[n, :p_len[n]], verts[n], faces[n]), w64)
	assert (w[3] == 0).all() and (w[2] == 0).all()
	# p_len as a list and on the device, F = 0, P = 0
	assert np.array_equal(_hip(pts, verts, faces, p_len), w) and np.array_equal(_hip(pts, verts, faces, torch.tensor(p_len).cuda()), w)
	assert (_hip(pts[:2], verts[:2], faces[:2, :0]) == 0).all() and _hip(pts[:2, :0], verts[:2], faces[:2]).shape == (2, 0)


# ------------------------------------------------------------------ independence
def test_a_row_does_not_depend_on_its_batch_its_position_or_the_split():
	key = (25, 40)   # F = 2000: two chunks, split at this size
	v, f = _mesh(key)
	pts = ref.box_points(v, 300, 0.02, 41)
	alone = _hip(pts[None], v[None], f)[0]
	others = np.stack([ref.box_points(v, 300, 0.02, 42), ref.box_points(v, 300, 0.02, 43), pts])
	batch = _hip(others, np.stack([v * np.float32(0.9), v * np.float32(1.2), v]), f)
	assert np.array_equal(batch[2], alone)
	longer = np.concatenate([ref.box_points(v, 100, 0.02, 44), pts])   # P padded by 100 points, the row's queries moved to the end
	assert np.array_equal(_hip(longer[None], v[None], f)[0, 100:], alone)
	assert np.array_equal(_hip(np.concatenate([pts, longer[:100]])[None], v[None], f)[0, :300], alone)
	assert np.array_equal(_hip(pts[None], v[None], f, unsplit=True)[0], alone)
	# 2048 blocks: unsplit by size; the same rows
	many = np.concatenate([pts] + [ref.box_points(v, 128 * 2048 - 300, 0.02, 45)])
	assert np.array_equal(_hip(many[None], v[None], f)[0, :300], alone)


# ------------------------------------------------------------------ sides
def _distance(points, verts, faces):
	"""The unsigned distance of the existing op (tests/test_gpu_surface.py holds it to float64): the filter of the side tests, not their subject."""
	from find_amd import functional as FN
	return FN.point_face_distance(_t(points)[None], _t(verts)[None], _t(faces, torch.int64))[0][0].sqrt().cpu().numpy()


@pytest.mark.parametrize('key', ['tet', (4, 16), (25, 40), 'template'], ids=str)
def test_sides_on_closed_meshes(key):
	v, f = _mesh(key)
	if key == 'template':
		_, faces, pts, w64, _ = _training_size()
		pts, w64 = pts[0], w64[0]
	else:
		pts = ref.box_points(v, 2000, 0.02, 51)
		w64, _ = _refs(f'sides {key}', pts, v, f)
	w = _hip(pts[None], v[None], f)[0]
	keep = _distance(pts, v, f) > 1e-4
	print(f'sides {key}: {100 * (1 - keep.mean()):.3f} % within 1e-4 m of the surface, {100 * (w64 > 0.5).mean():.1f} % inside')
	assert 1 - keep.mean() <= 0.01 and 0.02 < (w64 > 0.5).mean() < 0.98
	assert np.array_equal(w[keep] > 0.5, w64[keep] > 0.5)


def test_sides_on_the_open_template():
	v, faces, pts, w64, _ = _training_size()
	w = _hip(pts[1:], v[None], faces[1])[0]
	keep = np.abs(w64[1] - 0.5) >= 0.05
	print(f'open template: {100 * (1 - keep.mean()):.2f} % within 0.05 of the level, {100 * (w64[1] > 0.5).mean():.2f} % inside')
	assert 1 - keep.mean() <= 0.02 and 0.1 < (w64[1] > 0.5).mean() < 0.5
	assert np.array_equal(w[keep] > 0.5, w64[1][keep] > 0.5)


# ------------------------------------------------------------------ signed distance
def _sdf_case():
	v, f = _mesh((25, 40))
	g = torch.Generator().manual_seed(61)
	verts = torch.stack([torch.from_numpy(v), torch.from_numpy(v) * torch.tensor([1.1, 0.9, 1.05]) + 0.001 * torch.randn(v.shape, generator=g)])
	pts = torch.stack([torch.from_numpy(ref.box_points(vn.numpy(), 600, 0.02, 62 + n)) for n, vn in enumerate(verts)])
	pts[:, :20] = verts[:, 100:120]   # queries ON vertices: dist2 == 0
	return verts, torch.from_numpy(f), pts, torch.randn(2, 600, generator=g)


def test_signed_distance_sign_magnitude_and_gradients():
	from find_amd import functional as FN
	from find_amd import inside
	verts, f, pts, g = _sdf_case()
	r64 = [SR.point_face(pts[n].double(), verts[n].double(), f, far=1e-4) for n in range(2)]
	r32 = [SR.point_face(pts[n], verts[n], f) for n in range(2)]
	w64 = np.stack([_refs(f'sdf {n}', pts[n].numpy(), verts[n].numpy(), f.numpy())[0] for n in range(2)])
	off = torch.stack([r['dist2'].sqrt() > 1e-4 for r in r64])
	smooth = torch.stack([~(r['runner_up'] <= r['dist2'] * (1 + 1e-4) + 1e-12) for r in r64]) & off   # off the medial axis (test_gpu_surface.py)
	print(f'signed distance: {int((~off).sum())} queries within 1e-4 m of the surface, {int((~smooth).sum())} left out of the gradient check')
	assert (~off).sum() <= 60 and smooth.float().mean() > 0.9
	gm = torch.where(smooth, g, torch.zeros_like(g))
	gm[:, :20] = g[:, :20]   # the queries on vertices keep their weight: their gradient must come out 0, not NaN
	runs = []
	for _ in range(2):
		p, v = pts.cuda().requires_grad_(True), verts.cuda().requires_grad_(True)
		sdf, idx, bary, w = inside.signed_distance(p, v, f.cuda())
		assert sdf.requires_grad and not idx.requires_grad and not bary.requires_grad and not w.requires_grad
		dp, dv = torch.autograd.grad(sdf, (p, v), gm.cuda())
		runs.append(dict(sdf=sdf.detach(), idx=idx, bary=bary, w=w, dp=dp, dv=dv))
	for k in ('sdf', 'idx', 'bary', 'w', 'dp'):   # (dv is a float-atomic sum: find_point_face_bwd)
		assert torch.equal(runs[0][k], runs[1][k]), k
	a = runs[0]
	assert all(torch.isfinite(t).all() for k, t in a.items() if t.is_floating_point())
	dist2, idx, bary = FN.point_face_distance(pts.cuda(), verts.cuda(), f.cuda())
	assert torch.equal(a['sdf'].abs(), dist2.sqrt()) and torch.equal(a['idx'], idx) and torch.equal(a['bary'], bary)
	assert ((a['sdf'].double() ** 2 - dist2.double()).abs() <= 2 * torch.from_numpy(np.spacing(dist2.cpu().numpy())).cuda().double()).all()
	assert torch.equal(a['w'], inside.winding_number(pts.cuda(), verts.cuda(), f.cuda()))
	# the sign: negative inside, by the float64 restatement, wherever the query is off the surface
	inside64 = torch.from_numpy(w64 > 0.5)
	assert torch.equal((a['sdf'].cpu() < 0)[off], inside64[off]) and 0.05 < inside64.float().mean() < 0.95
	assert (a['sdf'][:, :20] == 0).all() and (a['dp'][:, :20] == 0).all()
	sign = torch.where(inside64, -1., 1.).double()
	on = ~off   # (a query within 1e-4 m of the surface has no side to be held to: its magnitude is)
	d64, d32 = torch.stack([r['dist2'] for r in r64]).sqrt(), torch.stack([r['dist2'] for r in r32]).double().sqrt()
	_held('sdf', torch.where(on.cuda(), a['sdf'].abs(), a['sdf']), torch.where(on, d64, sign * d64), torch.where(on, d32, sign * d32), 'sdf')
	# gradients: sign * d sqrt(dist2) = sign * g / (2 sqrt(dist2)) * d dist2, the restatement's (0 where dist2 == 0)
	dp64, dv64, dp32, dv32 = [], [], [], []
	for n in range(2):
		for dt, r, dps, dvs in ((torch.float64, r64[n], dp64, dv64), (torch.float32, r32[n], dp32, dv32)):
			root = r['dist2'].sqrt()
			gs = torch.where(root > 0, (sign[n] * gm[n].double()).to(dt) * 0.5 / root.clamp(min=1e-30), torch.zeros_like(root))
			gs[:20] = 0
			dp_, dv_ = SR.gradients(pts[n].to(dt), verts[n].to(dt), f, r['idx'], r['bary'], gs)
			dps.append(dp_), dvs.append(dv_)
	_held('sdf d points', a['dp'], torch.stack(dp64), torch.stack(dp32), 'sdf gradient')
	_held('sdf d verts', a['dv'], torch.stack(dv64), torch.stack(dv32), 'sdf gradient')
	assert a['dv'].abs().max().item() > 0 and a['dp'].abs().max().item() > 0


# ------------------------------------------------------------------ grids
def _cells64(verts, faces, origin, spacing, res, tag):
	"""The restatement's w at the centres of the grid the package names (its origin and spacing, its own grid_points on the CPU)."""
	from find_amd import inside
	pts = inside.grid_points(origin.cpu(), spacing.cpu(), res, 0, res ** 3).numpy()
	return np.stack([_refs(f'{tag} {n}', pts[n], verts[n], faces)[0] for n in range(len(verts))])


@pytest.mark.parametrize('key,res,N', [((25, 40), 16, 2), ((4, 16), 32, 1)], ids=str)
def test_occupancy_grid_cell_for_cell(key, res, N):
	from find_amd import inside
	v, f = _mesh(key)
	verts = np.stack([v * np.float32(1 + 0.1 * n) for n in range(N)])
	runs = [inside.occupancy_grid(_t(verts), _t(f, torch.int64), res) for _ in range(2)]
	occ, origin, spacing = runs[0]
	assert all(torch.equal(a, b) for a, b in zip(*runs))
	assert occ.shape == (N, res, res, res) and occ.dtype == torch.bool and origin.shape == spacing.shape == (N, 3)
	lo, hi = verts.min(1) - np.float32(0.005), verts.max(1) + np.float32(0.005)
	assert np.array_equal(origin.cpu().numpy(), lo) and np.allclose(spacing.cpu().numpy() * res, hi - lo, rtol=1e-6)
	w64 = _cells64(verts, f, origin, spacing, res, f'grid {key} {res}')
	assert (np.abs(w64 - 0.5) < 1e-4).sum() == 0   # a closed mesh: no cell to except
	assert np.array_equal(occ.cpu().numpy().reshape(N, -1), w64 > 0.5)
	assert 0.2 < occ.float().mean().item() < 0.6
	# the grid volume is the count times the cell, and close to the exact volume of a closed mesh
	vol = inside.mesh_volume(_t(verts), _t(f, torch.int64), res=res)
	want = occ.reshape(N, -1).sum(1).double() * spacing.double().prod(-1)
	assert vol.dtype == torch.float64 and torch.equal(vol, want)
	exact = inside.mesh_volume(_t(verts), _t(f, torch.int64))
	print(f'grid {key} {res}^3: grid volume / exact volume {(vol / exact).tolist()}')
	assert ((vol / exact - 1).abs() < 0.1).all()
	# explicit bounds, taken as given; and the cells consumed 1500 / N at a time (chunk boundaries off every power of two) instead of at once
	occ2, o2, s2 = inside.occupancy_grid(_t(verts), _t(f, torch.int64), res, bounds=(torch.from_numpy(lo), torch.from_numpy(hi)))
	assert np.array_equal(o2.cpu().numpy(), lo) and torch.equal(occ2, occ)
	whole = inside._CHUNK_POINTS
	inside._CHUNK_POINTS = 1500
	try:
		assert max(1 << 10, inside._CHUNK_POINTS // N) < res ** 3 / 2
		occ3, _, _ = inside.occupancy_grid(_t(verts), _t(f, torch.int64), res)
		assert torch.equal(occ3, occ) and torch.equal(inside.mesh_volume(_t(verts), _t(f, torch.int64), res=res), vol)
	finally:
		inside._CHUNK_POINTS = whole


def test_volume_iou():
	from find_amd import inside
	va, fa = _mesh((25, 40))
	vb, fb = _mesh((4, 16))
	res = 16
	A, FA = _t(va)[None], _t(fa, torch.int64)
	one = inside.volume_iou(A, FA, A, FA, res)
	assert all(t.dtype == torch.float64 and t.shape == (1,) for t in one)
	assert one[0].item() == 1.0 and torch.equal(one[1], one[2]) and torch.equal(one[1], inside.mesh_volume(A, FA, res=res))
	# a copy shifted by a fifth of its length, a smaller ellipsoid (V_a != V_b, F_a != F_b) and a disjoint copy: one batch of three
	shift = np.array([0.2 * (va[:, 0].max() - va[:, 0].min()), 0, 0], np.float32)
	Vb = np.zeros((3, len(va), 3), np.float32)
	Vb[0], Vb[1, :len(vb)], Vb[2] = va + shift, vb * np.float32(0.8), va + np.float32(6) * shift
	Vb[1, len(vb):] = Vb[1, 0]   # (rows no face names: inside the box)
	Fb = np.full((3, len(fa), 3), -1, np.int64)
	Fb[0], Fb[1, :len(fb)], Fb[2] = fa, fb, fa
	Va = np.stack([va, va, va])
	runs = [inside.volume_iou(_t(Va), FA, _t(Vb), _t(Fb, torch.int64), res) for _ in range(2)]
	assert all(torch.equal(a, b) for a, b in zip(*runs))
	iou, vol_a, vol_b = (t.cpu().numpy() for t in runs[0])
	# the restatement on the same grid: the box of both meshes grown by 5 mm, in float32 as the package forms it
	lo = torch.minimum(torch.from_numpy(Va).amin(1), torch.from_numpy(Vb).amin(1)) - 0.005
	hi = torch.maximum(torch.from_numpy(Va).amax(1), torch.from_numpy(Vb).amax(1)) + 0.005
	spacing = (hi - lo) / res
	wa = _cells64(Va, fa, lo, spacing, res, 'iou a')
	wb = np.stack([_cells64(Vb[n:n + 1], Fb[n], lo[n:n + 1], spacing[n:n + 1], res, f'iou b{n}')[0] for n in range(3)])
	assert (np.abs(wa - 0.5) < 1e-4).sum() == 0 and (np.abs(wb - 0.5) < 1e-4).sum() == 0
	ia, ib = wa > 0.5, wb > 0.5
	cell = spacing.double().prod(-1).numpy()
	print('volume_iou:', iou.tolist(), 'inside a / b / both:', ia.sum(1).tolist(), ib.sum(1).tolist(), (ia & ib).sum(1).tolist())
	assert np.array_equal(vol_a, ia.sum(1) * cell) and np.array_equal(vol_b, ib.sum(1) * cell)
	assert np.array_equal(iou, (ia & ib).sum(1) / np.maximum((ia | ib).sum(1), 1))
	assert 0.3 < iou[0] < 0.9 and 0.2 < iou[1] < 0.9 and iou[2] == 0 and vol_b[2] > 0
	# nothing inside either mesh: 0, not NaN
	none = inside.volume_iou(A, FA[:0], A, FA[:0], res)
	assert none[0].item() == 0 and none[1].item() == 0


# ------------------------------------------------------------------ the loss and the metric
def test_penetration_loss():
	from find_amd import functional as FN
	from find_amd.losses import PenetrationLoss
	from find_amd.structures import Meshes
	v, f = _mesh((25, 40))
	verts = np.stack([v, v * np.float32(1.1)])
	pts = np.stack([ref.box_points(verts[n], 500, 0.02, 71 + n) for n in range(2)])
	for n in range(2):   # a condition on the inputs: a query within 1e-3 m of the surface is moved to the centre, where its side is beyond doubt
		pts[n][_distance(pts[n], verts[n], f) < 1e-3] = 0
	w64 = np.stack([_refs(f'penetration {n}', pts[n], verts[n], f)[0] for n in range(2)])
	inside64 = torch.from_numpy(w64 > 0.5).cuda()
	assert 20 < inside64.sum().item() < 900
	p, vv = _t(pts).requires_grad_(True), _t(verts).requires_grad_(True)
	meshes = Meshes(vv, _t(f, torch.int64))
	loss = PenetrationLoss()(p, meshes)
	dist2 = FN.point_face_distance(p.detach(), vv.detach(), _t(f, torch.int64))[0]
	assert (dist2.sqrt()[inside64] > 1e-4).all()   # (no inside query so near the surface that float32 could name its side otherwise)
	want = torch.where(inside64, dist2, torch.zeros_like(dist2)).sum() / 1000
	assert loss.item() > 0 and torch.equal(loss.detach(), want)
	dp, dv = torch.autograd.grad(loss, (p, vv))
	assert torch.isfinite(dp).all() and torch.isfinite(dv).all()
	assert (dp[~inside64] == 0).all() and (dp[inside64].abs().sum(-1) > 0).all() and dv.abs().max().item() > 0
	# points outside cost nothing; padded rows do not count
	outside = torch.where(inside64[..., None], torch.full_like(p.detach(), 0.5), p.detach())
	assert PenetrationLoss()(outside, meshes).item() == 0
	lengths = torch.tensor([300, 0])
	part = PenetrationLoss()(p.detach(), meshes, lengths)
	counts = inside64 & (torch.arange(500, device='cuda')[None] < lengths.cuda()[:, None])
	# (the same sum, term for term, and a division by the count as a tensor: by a Python number torch multiplies with the rounded reciprocal)
	assert torch.equal(part.detach(), torch.where(counts, dist2, torch.zeros_like(dist2)).sum() / lengths.sum().cuda()) and part.item() > 0
	assert abs(part.item() / (torch.where(counts, dist2, torch.zeros_like(dist2)).double().sum().item() / 300) - 1) <= 1e-6


def test_eval_3d_metrics_volume():
	from find_amd import inside, synthetic
	from find_amd.eval_metrics import eval_3d_metrics
	from find_amd.structures import Meshes
	N, S = 2, 400
	v, f = synthetic.template(1002)
	g = torch.Generator().manual_seed(81)
	pv = torch.stack([v * (1 + 0.1 * torch.randn(3, generator=g)) for _ in range(N)])
	scans = [synthetic.ellipsoid_mesh(10, 14), synthetic.ellipsoid_mesh(12, 16)]   # two sizes: a ragged batch
	pred = Meshes(pv.cuda(), f.cuda())
	gt = Meshes([sv.cuda() for sv, _ in scans], [sf.cuda() for _, sf in scans])
	draws_p = synthetic.surface_draws(N, S, f.shape[0], seed=1, device='cuda')
	draws_g = (torch.stack([torch.randint(0, sf.shape[0], (S,), generator=g) for _, sf in scans]).to(torch.int32).cuda(), torch.rand(N, S, 2, generator=g).cuda())
	kw = dict(samples=S, draws_gt=draws_g, draws_pred=draws_p)
	plain = eval_3d_metrics(pred, gt, **kw)
	state = torch.cuda.get_rng_state()
	out, per_foot = eval_3d_metrics(pred, gt, volume=16, return_per_foot=True, **kw)
	assert torch.equal(torch.cuda.get_rng_state(), state)   # no random number is drawn
	assert list(out) == list(plain) + ['Vol IoU (%)', 'Volume err (ml)'] and all(torch.equal(out[k], plain[k]) for k in plain)
	assert list(per_foot) == ['vol_iou', 'volume_pred_ml', 'volume_gt_ml'] and all(t.shape == (N,) for t in per_foot.values())
	assert torch.equal(out['Vol IoU (%)'], per_foot['vol_iou'].mean() * 100) and 30 < out['Vol IoU (%)'].item() < 100
	assert torch.allclose(out['Volume err (ml)'], (per_foot['volume_pred_ml'] - per_foot['volume_gt_ml']).abs().mean(), rtol=1e-12, atol=0)
	# the grid volumes are near the exact ones (closed meshes; 16^3 over both boxes is coarse: 15 %)
	for n in range(N):
		exact_p = inside.mesh_volume(pv[n:n + 1], f).item() * 1e6
		exact_g = inside.mesh_volume(scans[n][0][None], scans[n][1]).item() * 1e6
		print(f'foot {n}: predicted {per_foot["volume_pred_ml"][n].item():.1f} ml (exact {exact_p:.1f}), scan {per_foot["volume_gt_ml"][n].item():.1f} ml (exact {exact_g:.1f})')
		assert abs(per_foot['volume_pred_ml'][n].item() / exact_p - 1) < 0.15 and abs(per_foot['volume_gt_ml'][n].item() / exact_g - 1) < 0.15
	assert list(eval_3d_metrics(pred, gt, volume=None, **kw)) == list(plain)


# ------------------------------------------------------------------ poison
def test_poisoned_allocations():
	"""w, the workspace and the grid of find_amd.inside are torch.empty: whatever they hold before the call, the results are the same bits.  The
	workspace comes from functional._ws, which tests/poison.py covers; the module itself is given the harness's proxy for its module-level
	`torch` here, as tests/test_gpu_arap.py does for its module."""
	from find_amd import inside as module
	v, f = _mesh((25, 40))
	v2, f2 = _mesh((4, 16))
	verts = np.zeros((2, len(v), 3), np.float32)
	verts[0], verts[1, :len(v2)] = v, v2
	faces = np.full((2, len(f), 3), -1, np.int64)
	faces[0], faces[1, 5:5 + len(f2)] = f, f2
	pts = np.stack([ref.box_points(v, 300, 0.02, 91), ref.box_points(v, 300, 0.02, 92)])
	P, V, F, PL = _t(pts), _t(verts), _t(faces, torch.int64), torch.tensor([300, 131])
	sv, sf, sp, sg = _sdf_case()

	def run():
		from find_amd import _lib
		out = dict(w_split=module.winding_number(P, V, F, PL))
		_lib.set_tuning('raster_ablate', 8192)
		try:
			out['w_unsplit'] = module.winding_number(P, V, F, PL)
		finally:
			_lib.set_tuning('raster_ablate', 0)
		out['w_no_faces'] = module.winding_number(P, V, F[:, :0])
		p, vv = sp.cuda().requires_grad_(True), sv.cuda().requires_grad_(True)
		sdf, idx, bary, w = module.signed_distance(p, vv, sf.cuda())
		(dp,) = torch.autograd.grad(sdf, p, sg.cuda())
		out.update(sdf=sdf.detach(), idx=idx, bary=bary, w=w, dp=dp)
		occ, origin, spacing = module.occupancy_grid(V[:1], F[0], 20)
		out.update(occ=occ.to(torch.uint8), origin=origin, spacing=spacing, volume=module.mesh_volume(V[:1], F[0], res=12))
		out.update(zip(('iou', 'vol_a', 'vol_b'), module.volume_iou(V[:1], F[0], V[:1] * 0.9, F[0], 12)))
		torch.cuda.synchronize()
		return out

	run()
	clean = run()
	runs = []
	for byte in poison.PATTERNS:
		with poison.poisoned(byte) as proxy:
			assert module.torch is torch
			module.torch = proxy
			try:
				runs.append(run())
			finally:
				module.torch = torch
		assert proxy.calls >= 20, proxy.calls   # w and its workspace per winding call, the point-face op's buffers, the grid
	assert np.array_equal(clean['w_split'].cpu().numpy(), clean['w_unsplit'].cpu().numpy()) and (clean['w_split'][1, 131:] == 0).all()
	bad = poison.compare('inside', clean, runs[0], runs[1])
	assert not bad, '\n'.join(bad)


def test_zz_worst_ratios():
	"""Prints the worst e_hip / max(e32, ulp) per quantity over the file's cases."""
	for k, v in sorted(WORST.items()):
		print(f'worst {k}: {v:.3f}')
	assert all(v <= 4. for v in WORST.values())
