"""Ray casting on the MI355X: find_ray_fwd / find_ray_bwd through find_amd.rays against the numpy restatement of the pair test
(tests/rays_ref.py) in float64 on the same fp32 inputs, and what is built on it: vertex visibility, ambient occlusion and the baked AO map.

Margins: none is a constant of the code under test.  Every float comparison follows _held of tests/test_gpu_inside.py: the restatement is also
evaluated in float32 on the CPU; with e32 its worst error against float64 over the case's tensor, the HIP result must lie within
max(4 e32, 2 ulp of the largest value) of the float64 one.  Each case prints its figures (DESIGN 7.16 records the worst).

Box rays: the origin is uniform in the mesh's box grown by 2 cm, aimed at a second such point (on the partial templates half of the rays
are aimed at a point of the surface instead: _box_rays).  A ray is SETTLED when the float32 and the
float64 restatement agree on (hit, idx).  On settled rays idx equals theirs and t and bary are held; unsettled rays may be at most 1 % of a
case (a condition on the inputs), and on them HIP must agree with one of the two restatements.  Every case runs twice and must repeat bit for
bit, and the any_hit call must equal isfinite(t) bit for bit.

Shapes, the smallest that cross each boundary: F = 1, 2 (one shared edge), 4 (a tetrahedron); the kernel stages tiles of 512 faces, a wave
scans 128, and a split piece holds at least 1024: F = 127 .. 129, 511 .. 513, 1023 .. 1025, 2047 .. 2049 (faces taken off the end of the
template's list); F = 13 776 with N = 2, the second mesh open and its faces -1 padded; a block owns 128 rays: R = 1, 127, 128, 129, 257; N = 1
and 3; ragged r_len, 0 included.  The face range is split over workgroups from F = 2048 on at these ray counts: every case with as many faces
runs both ways (find_render_switches bit 8192 holds the split off) and must agree bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import inside_ref   # noqa: E402
import poison   # noqa: E402
import rays_ref as ref   # noqa: E402

WORST = {}   # quantity -> the worst e_hip / max(e32, ulp) seen (printed by the last test of the file)
_MESHES, _REFS = {}, {}
SPLIT_FROM = 2048   # faces from which find_ray_fwd splits the range at a small ray count


def _ulp(x):
	return float(np.spacing(np.float32(abs(float(x)))))


def _held(name, hip, ref64, ref32, kind=None):
	hip, ref64, ref32 = (torch.as_tensor(np.asarray(t)).detach().double().cpu() if not torch.is_tensor(t) else t.detach().double().cpu() for t in (hip, ref64, ref32))
	assert hip.shape == ref64.shape, (name, hip.shape, ref64.shape)
	if hip.numel() == 0:
		return
	e_hip = (hip - ref64).abs().max().item()
	e32 = (ref32 - ref64).abs().max().item()
	ulp = _ulp(ref64.abs().max().item())
	ratio = e_hip / max(e32, ulp)
	print(f'{name}: e_hip {e_hip:.3e}  e32 {e32:.3e}  ulp {ulp:.3e}  scale {ref64.abs().max().item():.3e}  e_hip / max(e32, ulp) {ratio:.2f}')
	if kind:
		WORST[kind] = max(WORST.get(kind, 0.), ratio)
	assert np.isfinite(e_hip) and e_hip <= max(4 * e32, 2 * ulp), (name, e_hip, e32, ulp)


# ------------------------------------------------------------------ inputs, the reference (computed once per case), the HIP run
def _dented(rings, segs):
	"""An ellipsoid with a waist pressed in around x = 0: closed, outward oriented, concave."""
	from find_amd import synthetic
	v, f = (x.numpy() for x in synthetic.ellipsoid_mesh(rings, segs))
	v = v.astype(np.float64)
	v[:, 1:] *= (1 - 0.6 * np.exp(-(v[:, 0] / 0.03) ** 2))[:, None]
	return v, f


def _mesh(key):
	"""'one', 'two', 'tet', (rings, segs), 'template', ('open',): the template without the top 15 % of its faces; (n,): the template's first n
	faces; ('dent', rings, segs)."""
	if key not in _MESHES:
		from find_amd import synthetic
		if key == 'one':
			v, f = np.array([[0.05, 0, 0], [0, 0.05, 0], [0, 0, 0.05]]), np.array([[0, 1, 2]])
		elif key == 'two':   # two triangles with the edge (0, 1) in common, not coplanar
			v, f = np.array([[0.04, -0.03, 0.01], [-0.04, 0.03, 0.02], [0.03, 0.04, -0.02], [-0.03, -0.04, -0.01]]), np.array([[0, 1, 2], [1, 0, 3]])
		elif key == 'tet':
			v = np.array([[0.03, 0.03, 0.03], [0.03, -0.03, -0.03], [-0.03, 0.03, -0.03], [-0.03, -0.03, 0.03]])
			f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
		elif key == 'template':
			v, f = (x.numpy() for x in synthetic.template(6890))
		elif key == ('open',):
			v, f = _mesh('template')
			f = inside_ref.without_top(v, f, 0.15)
		elif key[0] == 'dent':
			v, f = _dented(*key[1:])
		elif len(key) == 1:
			v, f = _mesh('template')
			f = f[:key[0]]
		else:
			v, f = (x.numpy() for x in synthetic.ellipsoid_mesh(*key))
		_MESHES[key] = (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int64))
	return _MESHES[key]


def _box_rays(key, n, seed, on_surface=0):
	"""n box rays of the mesh; the last `on_surface` of them are aimed instead at a uniform point of a random face and go half as far again (a
	partial template is a thin band that box rays seldom meet)."""
	v, f = _mesh(key)
	o, d = ref.box_rays(v[np.unique(f)], n, 0.02, seed)
	if on_surface:
		rng = np.random.RandomState(seed + 1000)
		w = rng.dirichlet(np.ones(3), on_surface).astype(np.float32)
		target = (w[:, :, None] * v[f[rng.randint(0, len(f), on_surface)]]).sum(1)
		d[-on_surface:] = (target - o[-on_surface:]) * np.float32(1.5)
	return o, d


def _refs(tag, o, d, v, f, **kw):
	"""((t, idx, bary) in float64, the same in float32) of the restatement, computed once per tag."""
	if tag not in _REFS:
		_REFS[tag] = tuple(ref.cast(o, d, v, f, dt, **kw) for dt in (np.float64, np.float32))
	return _REFS[tag]


def _t(x, dtype=torch.float32):
	return torch.as_tensor(np.asarray(x)).to(dtype).cuda()


def _hip(o, d, v, f, r_len=None, skip=None, unsplit=False, **kw):
	"""(t, idx, bary) of the HIP path as numpy, from two calls that must agree bit for bit, with the any_hit call held to isfinite(t).
	o, d, v: (N, ., 3) arrays; f (F, 3) or (N, F, 3)."""
	from find_amd import _lib, rays
	O, D, V, F = _t(o), _t(d), _t(v), _t(f, torch.int64)
	_lib.set_tuning('raster_ablate', 8192 if unsplit else 0)
	try:
		a = rays.ray_mesh_intersect(O, D, V, F, r_len, skip, **kw)
		b = rays.ray_mesh_intersect(O, D, V, F, r_len, skip, **kw)
		h = rays.ray_occluded(O, D, V, F, r_len, skip, **kw)
		h2 = rays.ray_occluded(O, D, V, F, r_len, skip, **kw)
		torch.cuda.synchronize()
	finally:
		_lib.set_tuning('raster_ablate', 0)
	t, idx, bary = a
	assert t.shape == O.shape[:2] and t.dtype == torch.float32 and idx.shape == t.shape and idx.dtype == torch.int32 and bary.shape == O.shape
	assert not idx.requires_grad and not bary.requires_grad
	assert all(torch.equal(x, y) for x, y in zip(a, b)), 'two runs differ'
	assert h.dtype == torch.bool and torch.equal(h, torch.isfinite(t)) and torch.equal(h, h2), 'any_hit is not isfinite(t)'
	miss = ~torch.isfinite(t)
	assert not torch.isnan(t).any() and (t[miss] == float('inf')).all() and (idx[miss] == -1).all() and (bary[miss] == 0).all() and (idx[~miss] >= 0).all()
	return t.cpu().numpy(), idx.cpu().numpy().astype(np.int64), bary.cpu().numpy()


def _both_ways(o, d, v, f, **kw):
	"""The split decided by size and the unsplit path: the same bits."""
	a = _hip(o, d, v, f, **kw)
	if np.asarray(f).shape[-2] >= SPLIT_FROM:
		b = _hip(o, d, v, f, unsplit=True, **kw)
		assert all(np.array_equal(x, y) for x, y in zip(a, b)), 'the split and the unsplit path differ'
	return a


def _compare(tag, hip, r64, r32, kind='t', min_hits=1):
	"""One mesh's rays: hip, r64, r32 are (t (R,), idx (R,), bary (R, 3))."""
	(t, idx, bary), (t64, i64, b64), (t32, i32, b32) = hip, r64, r32
	settled = i64 == i32   # (idx == -1 is a miss: (hit, idx) in one)
	n_un = int((~settled).sum())
	print(f'{tag}: {len(t)} rays, {int((i64 >= 0).sum())} hit, {n_un} unsettled')
	assert n_un <= 0.01 * len(t), (tag, n_un)
	assert (i64 >= 0).sum() >= min_hits, tag
	assert np.array_equal(idx[settled], i64[settled]), (tag, np.nonzero(settled & (idx != i64))[0][:10])
	both = settled & (i64 >= 0)
	_held(f'{tag} t', t[both], t64[both], t32[both], kind)
	_held(f'{tag} bary', bary[both], b64[both], b32[both], 'bary')
	for r in np.nonzero(~settled)[0]:
		assert idx[r] in (i64[r], i32[r]), (tag, r, idx[r], i64[r], i32[r])


def _check_case(tag, key, n_rays, seed=0, min_hits=1, on_surface=0):
	v, f = _mesh(key)
	o, d = _box_rays(key, n_rays, seed, on_surface)
	r64, r32 = _refs(tag, o, d, v, f)
	hip = _both_ways(o[None], d[None], v[None], f)
	_compare(tag, tuple(x[0] for x in hip), r64, r32, min_hits=min_hits)
	return o, d, hip


# ------------------------------------------------------------------ values
@pytest.mark.parametrize('key', ['one', 'two', 'tet', (4, 16), (25, 40)], ids=str)
def test_shapes(key):
	_check_case(f'shape {key}', key, 600, min_hits=20)


@pytest.mark.parametrize('F', [127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049])
def test_face_counts_on_each_side_of_a_wave_a_tile_and_a_split_piece(F):
	_check_case(f'F = {F}', (F,), 400, seed=F, min_hits=150, on_surface=200)


@pytest.mark.parametrize('R', [1, 127, 128, 129, 257])
def test_ray_counts_on_each_side_of_a_block(R):
	key = (25, 40)
	v, f = _mesh(key)
	rays_ = [_box_rays(key, 257, seed) for seed in (11, 12, 13)]
	o, d = np.stack([r[0][:R] for r in rays_]), np.stack([r[1][:R] for r in rays_])
	hip = _hip(o, d, np.stack([v, v, v]), f)
	for n in range(3):
		r64, r32 = _refs(f'R cases {n}', rays_[n][0], rays_[n][1], v, f)
		_compare(f'R = {R}, mesh {n}', tuple(x[n] for x in hip), tuple(x[:R] for x in r64), tuple(x[:R] for x in r32), min_hits=0)
	# N = 1: the same rows
	assert all(np.array_equal(a[0], b[0]) for a, b in zip(_hip(o[:1], d[:1], v[None], f), hip))


def _training_size():
	"""template(6890), R = 2000, N = 2: mesh 0 the closed template, mesh 1 the template without its top, its face list padded with -1 rows."""
	v, f = _mesh('template')
	_, fo = _mesh(('open',))
	faces = np.full((2, len(f), 3), -1, np.int64)
	faces[0], faces[1, :len(fo)] = f, fo
	rays_ = [_box_rays('template', 2000, seed) for seed in (21, 22)]
	refs = [_refs(f'training size {n}', rays_[n][0], rays_[n][1], v, faces[n]) for n in range(2)]
	return v, faces, np.stack([r[0] for r in rays_]), np.stack([r[1] for r in rays_]), refs


def test_training_size_split_and_unsplit():
	v, faces, o, d, refs = _training_size()
	hip = _both_ways(o, d, np.stack([v, v]), faces)
	for n, name in enumerate(('closed', 'open')):
		_compare(f'template(6890) {name}', tuple(x[n] for x in hip), *refs[n], min_hits=500)
	# the open mesh lets rays through that the closed one stops
	assert np.isfinite(hip[0][1]).sum() < np.isfinite(_hip(o[1:], d[1:], v[None], faces[0])[0]).sum()
	# the shared face list gives the closed mesh's row the same bits
	assert all(np.array_equal(a[0], b[0]) for a, b in zip(_hip(o[:1], d[:1], v[None], faces[0]), hip))


def test_ragged_rays_padded_faces_skip_and_a_mesh_without_faces():
	v, f = _mesh((25, 40))
	v2, f2 = _mesh((4, 16))
	V, F = len(v), len(f)
	verts = np.zeros((4, V, 3), np.float32)
	verts[0], verts[1, :len(v2)], verts[2], verts[3] = v, v2, v * np.float32(1.1), v
	faces = np.full((4, F + 3, 3), -1, np.int64)
	faces[0, :F] = f
	faces[0, F:] = [[0, 1, V], [5, -2, 7], [V + 3, 2, 1]]                       # out of range: never hit
	faces[1, 10:10 + len(f2)] = f2                                             # -1 rows before and after
	faces[2, :F] = f
	faces[3, :4] = [[-1, -1, -1], [0, 1, V], [-5, 2, 3], [1 << 30, 0, 1]]       # no face that can be hit
	R, r_len = 200, [200, 77, 0, 150]
	rays_ = [ref.box_rays(v, R, 0.02, 30 + n) for n in range(4)]
	o, d = np.stack([r[0] for r in rays_]), np.stack([r[1] for r in rays_])
	d[0, 5], d[0, 6, 1], o[0, 7, 2] = 0, np.nan, np.inf   # dead rays
	hip = _hip(o, d, verts, faces, torch.tensor(r_len))
	for n, (vn, fn) in enumerate(((v, f), (v2, f2), (v * np.float32(1.1), f), (v, f[:0]))):
		assert (hip[1][n, r_len[n]:] == -1).all() and np.isinf(hip[0][n, r_len[n]:]).all() and (hip[2][n, r_len[n]:] == 0).all(), n
		if r_len[n] and len(fn):
			r64, r32 = _refs(f'ragged {n}', o[n, :r_len[n]], d[n, :r_len[n]], vn, fn)
			shift = 10 if n == 1 else 0   # (mesh 1's faces sit behind ten -1 rows)
			r64, r32 = ((r[0], np.where(r[1] >= 0, r[1] + shift, -1), r[2]) for r in (r64, r32))
			_compare(f'ragged mesh {n}', tuple(x[n, :r_len[n]] for x in hip), r64, r32, min_hits=10)
			# ... the restatement skips the rows itself: handed the padded list, it says the same
			assert all(np.array_equal(a, b) for a, b in zip(ref.cast(o[n, :r_len[n]], d[n, :r_len[n]], verts[n], faces[n]), r64))
	assert (hip[1][3] == -1).all() and (hip[1][2] == -1).all() and (hip[1][0, 5:8] == -1).all()
	# r_len as a list and on the device, F = 0, R = 0
	for rl in (r_len, torch.tensor(r_len).cuda()):
		assert all(np.array_equal(a, b) for a, b in zip(_hip(o, d, verts, faces, rl), hip))
	assert (_hip(o[:2], d[:2], verts[:2], faces[:2, :0])[1] == -1).all() and _hip(o[:2, :0], d[:2, :0], verts[:2], faces[:2])[0].shape == (2, 0)
	# skip: every ray that hit is cast again with the face it hit skipped, and takes what the restatement says is next
	first = hip[1][0]
	r64, r32 = _refs('skip', o[0], d[0], v, f, skip=first)
	again = _hip(o[:1], d[:1], verts[:1], faces[0], skip=torch.from_numpy(first)[None])
	_compare('skip the first hit', tuple(x[0] for x in again), r64, r32, min_hits=10)
	hit = first >= 0
	assert (again[1][0][hit] != first[hit]).all() and (again[0][0][hit] >= hip[0][0][hit]).all() and np.array_equal(again[1][0][~hit], first[~hit])
	# the interval: (t_first, inf) finds the same second hit or a face at the same t; (0, t_first] finds the first, (0, t_first / 2] nothing nearer
	tq = float(np.sort(hip[0][0][hit])[hit.sum() // 2])   # (a float32: the C call and both restatements see the same bound)
	near, far = _hip(o[:1], d[:1], verts[:1], faces[0], t_max=tq), _hip(o[:1], d[:1], verts[:1], faces[0], t_min=tq)
	assert np.array_equal(near[1][0], np.where(hip[0][0] <= np.float32(tq), first, -1)) and (far[0][0] > np.float32(tq)).all()
	r64, r32 = _refs('t_min', o[0], d[0], v, f, t_min=np.float32(tq))
	_compare('t_min', tuple(x[0] for x in far), r64, r32, min_hits=10)


# ------------------------------------------------------------------ independence
def test_a_row_does_not_depend_on_its_batch_its_position_or_the_split():
	key = (2049,)   # two pieces at this size
	v, f = _mesh(key)
	o, d = _box_rays(key, 300, 41)
	alone = _hip(o[None], d[None], v[None], f)
	o2, d2 = _box_rays(key, 300, 42)
	batch = _hip(np.stack([o2, o2 * np.float32(0.5), o]), np.stack([d2, d2, d]), np.stack([v * np.float32(0.9), v * np.float32(1.2), v]), f)
	assert all(np.array_equal(b[2], a[0]) for a, b in zip(alone, batch))
	longer = _hip(np.concatenate([o2[:100], o])[None], np.concatenate([d2[:100], d])[None], v[None], f)   # R padded by 100 rays, the row's rays moved to the end
	assert all(np.array_equal(b[0, 100:], a[0]) for a, b in zip(alone, longer))
	front = _hip(np.concatenate([o, o2[:100]])[None], np.concatenate([d, d2[:100]])[None], v[None], f)
	assert all(np.array_equal(b[0, :300], a[0]) for a, b in zip(alone, front))
	assert all(np.array_equal(b[0], a[0]) for a, b in zip(alone, _hip(o[None], d[None], v[None], f, unsplit=True)))
	# 1024 blocks: unsplit by size; the same rows
	rng = np.random.RandomState(45)
	many_o = np.concatenate([o, rng.uniform(-0.1, 0.1, (128 * 1024 - 300, 3)).astype(np.float32)])
	many_d = np.concatenate([d, rng.uniform(-0.1, 0.1, (128 * 1024 - 300, 3)).astype(np.float32)])
	many = _hip(many_o[None], many_d[None], v[None], f)
	assert all(np.array_equal(b[0, :300], a[0]) for a, b in zip(alone, many))


# ------------------------------------------------------------------ watertightness
def test_watertight_on_the_device():
	v, f = _mesh('template')
	o, d = ref.aimed_rays(v, f)
	assert len(o) == 9842
	r64, r32 = _refs('aimed', o, d, v, f)
	assert np.isfinite(r64[0]).all() and np.isfinite(r32[0]).all()
	t, idx, bary = (x[0] for x in _both_ways(o[None], d[None], v[None], f))
	print(f'aimed rays: {int((~np.isfinite(t)).sum())} of {len(t)} miss; idx differs from float64 on {100 * (idx != r64[1]).mean():.1f} %, float32 from float64 on {100 * (r32[1] != r64[1]).mean():.1f} %')
	assert np.isfinite(t).all() and (idx >= 0).all()
	_held('aimed rays t', t, r64[0], r32[0], 't aimed')
	assert (f[idx[:6890]] == np.arange(6890)[:, None]).any(1).all()   # the face that is hit holds the target vertex
	# through the shared edge of the F = 2 case, from four origins on either side
	v2, f2 = _mesh('two')
	s = np.linspace(0.05, 0.95, 500).astype(np.float32)[:, None]
	on_edge = v2[0] + s * (v2[1] - v2[0])
	for k, origin in enumerate(([0.01, 0.02, 0.2], [-0.05, 0.01, 0.15], [0.0, 0.0, -0.1], [0.02, -0.01, -0.3])):
		oo = np.broadcast_to(np.array(origin, np.float32), on_edge.shape).copy()
		dd = (on_edge - oo) * np.float32(0.7)
		e64, e32 = _refs(f'edge {k}', oo, dd, v2, f2)
		assert np.isfinite(e64[0]).all() and np.isfinite(e32[0]).all()
		te, ie, _ = (x[0] for x in _hip(oo[None], dd[None], v2[None], f2))
		assert np.isfinite(te).all(), f'{int((~np.isfinite(te)).sum())} rays pass through the shared edge'
		_held(f'shared edge, origin {k}: t', te, e64[0], e32[0], 't aimed')


# ------------------------------------------------------------------ gradients
def _torch_t(o, d, v, f, idx):
	"""t = n . (a - o) / (n . d) with the face fixed, in the tensors' dtype; 0 where idx < 0."""
	tri = v[f[idx.clamp(min=0)]]
	a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
	n = torch.linalg.cross(b - a, c - a)
	return torch.where(idx >= 0, (n * (a - o)).sum(-1) / (n * d).sum(-1), torch.zeros_like(o[:, 0]))


def test_gradients_against_autograd_of_the_restatement():
	from find_amd import rays
	key = (25, 40)
	v, f = _mesh(key)
	N, R = 2, 700
	verts = np.stack([v, v * np.float32(1.1)])
	rays_ = [ref.box_rays(verts[n], R, 0.02, 51 + n) for n in range(N)]
	o, d = np.stack([r[0] for r in rays_]), np.stack([r[1] for r in rays_])
	g = torch.Generator().manual_seed(53)
	w = torch.randn(N, R, generator=g)
	refs = [_refs(f'grad {n}', o[n], d[n], verts[n], f) for n in range(N)]
	settled = np.stack([r[0][1] == r[1][1] for r in refs])
	wm = torch.where(torch.from_numpy(settled), w, torch.zeros_like(w))
	runs = []
	for _ in range(2):
		O, D, V = _t(o).requires_grad_(True), _t(d).requires_grad_(True), _t(verts).requires_grad_(True)
		t, idx, bary = rays.ray_mesh_intersect(O, D, V, _t(f, torch.int64))
		assert t.requires_grad and not idx.requires_grad and not bary.requires_grad
		hit = torch.isfinite(t)
		(t[hit] * wm.cuda()[hit]).sum().backward()
		runs.append((O.grad.clone(), D.grad.clone(), V.grad.clone(), idx))
	assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])   # (the vertices' is a float-atomic sum: find_ray_bwd)
	d_o, d_d, d_v, idx = runs[0]
	assert all(torch.isfinite(x).all() for x in (d_o, d_d, d_v))
	miss = (idx < 0).cpu()
	assert miss.sum() > 50 and (d_o.cpu()[miss] == 0).all() and (d_d.cpu()[miss] == 0).all()
	want = {}
	for dt in (torch.float64, torch.float32):
		go, gd, gv = [], [], []
		for n in range(N):
			O, D, V = (torch.from_numpy(x).to(dt).requires_grad_(True) for x in (o[n], d[n], verts[n]))
			i64 = torch.from_numpy(np.where(settled[n], refs[n][0][1], -1))
			(_torch_t(O, D, V, torch.from_numpy(f), i64) * wm[n].to(dt)).sum().backward()
			go.append(O.grad), gd.append(D.grad), gv.append(V.grad)
		want[dt] = tuple(torch.stack(x) for x in (go, gd, gv))
	keep = torch.from_numpy(settled)
	assert np.array_equal(idx.cpu().numpy()[settled], np.stack([r[0][1] for r in refs])[settled])
	_held('d t / d origins', d_o.cpu()[keep], want[torch.float64][0][keep], want[torch.float32][0][keep], 'gradient')
	_held('d t / d dirs', d_d.cpu()[keep], want[torch.float64][1][keep], want[torch.float32][1][keep], 'gradient')
	_held('d t / d verts', d_v, want[torch.float64][2], want[torch.float32][2], 'gradient')
	assert d_v.abs().max().item() > 0 and (d_v.abs().sum(-1) > 0).sum().item() > 100
	# a vertex shared by the two hit faces receives the sum of what each ray alone gives it
	v2, f2 = _mesh('two')
	cents = v2[f2].mean(1)
	oo = np.array([[0.0, 0.0, 0.3], [0.01, -0.01, 0.25]], np.float32)
	dd = cents - oo
	parts = []
	for rows in ([0], [1], [0, 1]):
		O, D, V = _t(oo[rows])[None], _t(dd[rows])[None], _t(v2)[None].requires_grad_(True)
		t, idx, _ = rays.ray_mesh_intersect(O, D, V, _t(f2, torch.int64))
		assert idx[0].tolist() == rows
		t.sum().backward()
		parts.append(V.grad[0].clone())
	assert torch.equal(parts[2], parts[0] + parts[1]) and (parts[0][:2].abs().sum(-1) > 0).all() and (parts[1][:2].abs().sum(-1) > 0).all()
	assert (parts[0][3] == 0).all() and (parts[1][2] == 0).all()
	# o + t d is differentiable by torch
	O = _t(oo)[None].requires_grad_(True)
	t, _, bary = rays.ray_mesh_intersect(O, _t(dd)[None], _t(v2)[None], _t(f2, torch.int64))
	(O + t[..., None] * _t(dd)[None]).sum().backward()
	assert torch.isfinite(O.grad).all() and ((bary.sum(-1) - 1).abs() <= 1e-6).all()


# ------------------------------------------------------------------ visibility
def test_vertex_visibility_on_an_ellipsoid_and_on_the_template_from_below():
	from find_amd import rays
	from test_rays_host import ellipsoid_case
	centres = [(0.5, 0., 0.), (-0.3, 0.2, 0.4)]
	cases = [ellipsoid_case(centre=c) for c in centres]
	v, f = cases[0][0], cases[0][1]
	R = torch.eye(3)[None].expand(2, -1, -1).cuda()
	T = -torch.tensor(centres).cuda()   # R = I: C = -T
	runs = [rays.vertex_visibility(_t(np.stack([v, v])), _t(f, torch.int64), R, T) for _ in range(2)]
	assert runs[0].shape == (2, 2, len(v)) and runs[0].dtype == torch.bool and torch.equal(runs[0], runs[1]) and torch.equal(runs[0][0], runs[0][1])
	vis = runs[0][0].cpu().numpy()
	for m, (_, _, C, h, margin) in enumerate(cases):
		seen_side, far_side = h > margin, h < -margin
		print(f'camera {m}: {seen_side.sum()} vertices above their margin, {far_side.sum()} below, {vis[m].sum()} seen of {len(v)}')
		assert seen_side.sum() >= 0.2 * len(v) and far_side.sum() >= 0.3 * len(v)
		assert vis[m][seen_side].all() and not vis[m][far_side].any()
		v32, v64 = ref.visibility(v, f, C, np.float32), ref.visibility(v, f, C, np.float64)
		same = v32 == v64
		assert same.mean() >= 0.99 and np.array_equal(vis[m][same], v64[same])
	# a rotated camera: the same centre through C = -T @ R^T; per-mesh cameras (N, M, 3, 3); the rays consumed a camera at a time
	g = torch.Generator().manual_seed(5)
	Q = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
	Tq = -(torch.tensor(centres[1]) @ Q)
	assert (rays.camera_centres(Q, Tq) - torch.tensor(centres[1])).abs().max() <= 1e-6
	whole = rays._CHUNK_RAYS
	rays._CHUNK_RAYS = len(v)
	try:
		per_mesh = rays.vertex_visibility(_t(v)[None], _t(f, torch.int64), R[None], T[None])
	finally:
		rays._CHUNK_RAYS = whole
	assert torch.equal(per_mesh, runs[0][:1])
	# the template from below: the sole is seen, the instep is not
	tv, tf, C, h, margin = ellipsoid_case(84, 82, centre=(0., 0., -0.5))
	sole, instep = tv[:, 2] < -0.02, tv[:, 2] > 0.02
	assert (h[sole] > margin[sole]).all() and (h[instep] < -margin[instep]).all() and sole.sum() > 1000 and instep.sum() > 1000
	vis = rays.vertex_visibility(_t(tv)[None], _t(tf, torch.int64), torch.eye(3)[None].cuda(), torch.tensor([[0., 0., 0.5]]).cuda())[0, 0].cpu().numpy()
	print(f'template from below: {vis.sum()} of {len(tv)} vertices seen; sole {sole.sum()}, instep {instep.sum()}')
	assert vis[sole].all() and not vis[instep].any()


# ------------------------------------------------------------------ ambient occlusion
def _hull(v):
	"""The convex hull of the points as a mesh over the same vertex array, faces oriented outward."""
	from scipy.spatial import ConvexHull
	hull = ConvexHull(v.astype(np.float64))
	f = hull.simplices.astype(np.int64)
	n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
	flip = (n * (v[f].mean(1) - v.mean(0))).sum(1) < 0
	f[flip] = f[flip][:, ::-1]
	return f, np.unique(f)


def test_ambient_occlusion():
	from find_amd import rays
	from find_amd import functional as FN
	v, f = _mesh((25, 40))
	V, F = _t(v)[None], _t(f, torch.int64)
	axes = np.array([0.12, 0.045, 0.04])
	# a convex mesh sees the whole sky: from its vertices (the faces at a vertex have a corner at the origin) about the ellipsoid's own
	# outward normals, about the vertex normals, and from face centroids about the face normals with the face skipped -- exactly 1
	n_analytic = _t(v.astype(np.float64) / axes ** 2)[None]
	assert (rays.ambient_occlusion(V, n_analytic, V, F) == 1).all()
	ao = rays.vertex_ambient_occlusion(V, F, n_dirs=32)
	assert ao.shape == (1, len(v)) and ao.dtype == torch.float32 and (ao == 1).all()
	cents = V[0][F].mean(1)[None]
	nf = torch.linalg.cross(V[0][F][:, 1] - V[0][F][:, 0], V[0][F][:, 2] - V[0][F][:, 0])[None]
	skip = torch.arange(len(f))[None]
	assert (rays.ambient_occlusion(cents, nf, V, F, skip=skip) == 1).all()
	# ... turned inward every ray hits the far wall, whatever the skip
	assert (rays.ambient_occlusion(cents, -nf, V, F, skip=skip) == 0).all()
	# inside a closed cube nothing escapes: watertightness again
	cv, cf = _t(inside_ref.CUBE_VERTS * 0.1)[None], _t(inside_ref.CUBE_FACES, torch.int64)
	g = torch.Generator().manual_seed(7)
	pts = (0.005 + 0.09 * torch.rand(1, 500, 3, generator=g)).cuda()
	nrm = torch.randn(1, 500, 3, generator=g).cuda()
	a = rays.ambient_occlusion(pts, nrm, cv, cf, n_dirs=64)
	assert a.shape == (1, 500) and (a == 0).all()
	# max_dist: nothing within 1 mm of a point at least 5 mm from every wall; everything within the cube's diagonal
	assert (rays.ambient_occlusion(pts, nrm, cv, cf, max_dist=0.001) == 1).all() and (rays.ambient_occlusion(pts, nrm, cv, cf, max_dist=0.18) == 0).all()
	# the direction set and the frames are what the value is made of: the same rays through ray_occluded, and in chunks
	loc = rays.hemisphere_directions(16, 'cuda')
	dv, df = _mesh(('dent', 25, 40))
	DV, DF = _t(dv)[None], _t(df, torch.int64)
	P = (DV[:, ::7] * 1.0).contiguous()
	PN = FN.vertex_normals(DV, DF)[:, ::7].contiguous()
	t1, t2, n = rays.normal_frames(PN)
	dirs = (loc[:, 0, None] * t1[:, :, None] + loc[:, 1, None] * t2[:, :, None] + loc[:, 2, None] * n[:, :, None]).reshape(1, -1, 3)
	occ = rays.ray_occluded(P[:, :, None].expand(-1, -1, 16, -1).reshape(1, -1, 3), dirs, DV, DF)
	a16 = rays.ambient_occlusion(P, PN, DV, DF, n_dirs=16)
	assert torch.equal(a16, (~occ).view(1, -1, 16).sum(-1).float() / 16) and torch.equal(a16, rays.ambient_occlusion(P, PN, DV, DF, n_dirs=16, rays_per_call=100))
	assert 0 < (a16 < 1).float().mean().item() < 1
	# vertex AO on the template lies in [0, 1]; a concave mesh is darker on average than its convex hull
	tv, tf = _mesh('template')
	at = rays.vertex_ambient_occlusion(_t(tv)[None], _t(tf, torch.int64), n_dirs=16)
	assert at.shape == (1, 6890) and (at >= 0).all() and (at <= 1).all() and torch.equal(at, rays.vertex_ambient_occlusion(_t(tv)[None], _t(tf, torch.int64), n_dirs=16))
	hf, used = _hull(dv)
	concave = rays.vertex_ambient_occlusion(DV, DF)
	convex = rays.vertex_ambient_occlusion(DV, _t(hf, torch.int64))[:, torch.from_numpy(used).cuda()]
	print(f'vertex AO: dented ellipsoid mean {concave.mean().item():.4f} min {concave.min().item():.4f}; its hull ({len(used)} vertices) mean {convex.mean().item():.4f}')
	assert (concave >= 0).all() and (concave <= 1).all() and (convex == 1).all() and concave.mean().item() < convex.mean().item() and concave.min().item() < 0.9


def test_bake_ambient_occlusion():
	from find_amd import bake, rays, synthetic
	v, f = _mesh(('dent', 6, 16))
	vu, fu = synthetic.face_atlas(len(f))
	plan = bake.plan(vu.cuda(), fu.cuda(), 64, pad=2)
	verts = _t(np.stack([v, v * np.float32(1.2)]))
	F = _t(f, torch.int64)
	maps = bake.bake_ambient_occlusion(plan, verts, F, n_dirs=32, fill=0.5)
	assert maps.shape == (2, 64, 64, 1) and maps.dtype == torch.float32 and torch.equal(maps, bake.bake_ambient_occlusion(plan, verts, F, n_dirs=32, fill=0.5))
	T = plan.idx.numel()
	assert T > 500
	pts = plan.points(verts, F).contiguous()
	skip = plan.face.reshape(-1)[plan.idx][None].expand(2, -1)
	want = rays.ambient_occlusion(pts, bake.texel_normals(plan, verts, F).contiguous(), verts, F, n_dirs=32, skip=skip)
	flat = maps.reshape(2, -1)
	assert torch.equal(flat[:, plan.idx], want) and (want >= 0).all() and (want <= 1).all() and 0 < (want < 1).float().mean().item() < 1
	# the gutter: a texel within the pad copies its covered texel, the rest is fill
	table = torch.cat([want, want.new_full((2, 1), 0.5)], 1)
	assert torch.equal(flat, table[:, plan.lookup]) and (plan.lookup == T).any() and ((plan.lookup < T).sum() > T)
	# faces given as (1, F, 3), one mesh
	assert bake.bake_ambient_occlusion(plan, verts[:1], F[None], n_dirs=32).shape == (1, 64, 64, 1)


# ------------------------------------------------------------------ poison
def test_poisoned_allocations():
	"""t, idx, bary, hit, the key workspace and the gradients of find_amd.rays are torch.empty: whatever they hold before the call, the results
	are the same bits.  The workspace comes from functional._ws, which tests/poison.py covers; the module itself is given the harness's proxy
	for its module-level `torch` here, as tests/test_gpu_inside.py does for its module."""
	from find_amd import _lib, bake, synthetic
	from find_amd import rays as module
	v, f = _mesh((2049,))
	v2, f2 = _mesh((4, 16))
	verts = np.zeros((2, len(v), 3), np.float32)
	verts[0], verts[1, :len(v2)] = v, v2
	faces = np.full((2, len(f), 3), -1, np.int64)
	faces[0], faces[1, 5:5 + len(f2)] = f, f2
	o, d = (np.stack(x) for x in zip(_box_rays((2049,), 300, 91), ref.box_rays(v2, 300, 0.02, 92)))
	O, D, V, F, RL = _t(o), _t(d), _t(verts), _t(faces, torch.int64), torch.tensor([300, 131])
	g = torch.Generator().manual_seed(93)
	w = torch.randn(2, 300, generator=g).cuda()
	dv, df = _mesh(('dent', 6, 16))
	DV, DF = _t(dv)[None], _t(df, torch.int64)
	vu, fu = synthetic.face_atlas(len(df))
	plan = bake.plan(vu.cuda(), fu.cuda(), 32, pad=2)
	cam_R, cam_T = torch.eye(3)[None].cuda(), torch.tensor([[0., 0., 0.5]]).cuda()

	def run():
		out = {}
		for tag, bits in (('split', 0), ('unsplit', 8192)):
			_lib.set_tuning('raster_ablate', bits)
			try:
				out.update(zip((f't_{tag}', f'idx_{tag}', f'bary_{tag}'), module.ray_mesh_intersect(O, D, V, F, RL)))
				out[f'hit_{tag}'] = module.ray_occluded(O, D, V, F, RL).to(torch.uint8)
			finally:
				_lib.set_tuning('raster_ablate', 0)
		out.update(zip(('t_no_faces', 'idx_no_faces', 'bary_no_faces'), module.ray_mesh_intersect(O, D, V, F[:, :0])))
		out['hit_no_faces'] = module.ray_occluded(O, D, V, F[:, :0]).to(torch.uint8)
		first = out['idx_split']
		out.update(zip(('t_skip', 'idx_skip', 'bary_skip'), module.ray_mesh_intersect(O, D, V, F, RL, skip=first)))
		o_, d_ = O.clone().requires_grad_(True), D.clone().requires_grad_(True)
		t, _, _ = module.ray_mesh_intersect(o_, d_, V, F, RL)
		hit = torch.isfinite(t)
		out['d_o'], out['d_d'] = torch.autograd.grad((t[hit] * w[hit]).sum(), (o_, d_))
		out['vis'] = module.vertex_visibility(DV, DF, cam_R, cam_T).to(torch.uint8)
		out['ao'] = module.vertex_ambient_occlusion(DV, DF, n_dirs=8)
		out['ao_map'] = bake.bake_ambient_occlusion(plan, DV, DF, n_dirs=8)
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
		assert proxy.calls >= 30, proxy.calls   # the outputs and the key workspace per ray call, the two gradients, the chunks' buffers
	assert all(torch.equal(clean[f'{k}_split'], clean[f'{k}_unsplit']) for k in ('t', 'idx', 'bary', 'hit'))
	assert torch.isinf(clean['t_split'][1, 131:]).all() and (clean['idx_split'][1, 131:] == -1).all() and (clean['idx_no_faces'] == -1).all()
	assert 0 < clean['hit_split'].float().mean().item() < 1 and 0 < clean['vis'].float().mean().item() < 1 and (clean['ao'] < 1).any()
	bad = poison.compare('rays', clean, runs[0], runs[1])
	assert not bad, '\n'.join(bad)


def test_zz_worst_ratios():
	"""Prints the worst e_hip / max(e32, ulp) per quantity over the file's cases."""
	for k, v in sorted(WORST.items()):
		print(f'worst {k}: {v:.3f}')
	assert all(v <= 4. for v in WORST.values())
