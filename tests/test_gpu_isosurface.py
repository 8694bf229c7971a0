"""Surface nets on the MI355X: find_surface_nets_count / _emit / _bwd through find_amd.isosurface against the numpy restatement of the
definition (tests/isosurface_ref.py), and field_grid / remesh on top of find_amd.inside.

Topology is exact: faces, v_len, f_len and status equal the restatement's element for element -- the sides are exact float32 comparisons.
Positions and gradients follow _held of tests/test_gpu_inside.py: the restatement is also evaluated in float32 on the CPU; with e32 its worst
error against float64 over the case's tensor, the HIP result must lie within max(4 e32, 2 ulp of the largest value) of the float64 one.  No
constant of the code under test enters a margin.  Each case prints its figures (DESIGN 7.15 records the worst).

All fields are made on the CPU from formulas (isosurface_ref.field), so the extraction is tested without the other kernels, the remesh cases
apart.  Shapes, the smallest that cross each boundary: a workgroup owns 256 consecutive samples and 256 consecutive cells
(isosurface.BLOCK_CELLS): grids of 8 samples (one block), (5, 9, 17) (three blocks, every axis different: a transposed stride shows), thin
grids (2, 2, n) with 255, 256, 257 and 513 cells, the host file's cases up to 32^3 (128 blocks); N = 1 and 3.  Every case runs twice and
must repeat bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import inside_ref   # noqa: E402
import isosurface_ref as ref   # noqa: E402
import poison   # noqa: E402
import surface_ref as SR   # noqa: E402

WORST = {}   # quantity -> the worst e_hip / max(e32, ulp) seen (printed by the last test of the file)


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


def _t(x, dtype=torch.float32):
	return torch.as_tensor(np.asarray(x)).to(dtype).cuda()


def _nets(values, iso=0.0, max_verts=None, max_faces=None):
	"""(g, faces, v_len, f_len, status) of the op under find_amd.isosurface.extract_surface -- g in grid coordinates, before origin and spacing
	-- as numpy, from two runs that must agree bit for bit.  values (N, nx, ny, nz)."""
	from find_amd import isosurface
	v = _t(values)
	a = isosurface._SurfaceNets.apply(v, None, float(iso), max_verts, max_faces)
	b = isosurface._SurfaceNets.apply(v, None, float(iso), max_verts, max_faces)
	torch.cuda.synchronize()
	for x, y, dt in zip(a, b, (torch.float32, torch.int32, torch.int64, torch.int64, torch.int32)):
		assert x.dtype == dt and x.shape == y.shape and torch.equal(x, y), 'two runs differ'
	return tuple(x.cpu().numpy() for x in a)


def _same_mesh(tag, out, n, r64, r32, kind='g'):
	"""Mesh n of a HIP result against the restatement: topology exactly, padding, positions by _held."""
	g, faces, v_len, f_len, status = out
	V, F = len(r64.g), len(r64.faces)
	assert (v_len[n], f_len[n], status[n]) == (V, F, r64.status), (tag, v_len[n], f_len[n], status[n], V, F, r64.status)
	assert np.array_equal(faces[n, :F], r64.faces), f'{tag}: faces differ'
	assert (faces[n, F:] == -1).all() and (g[n, V:] == 0).all(), f'{tag}: padding'
	assert np.isfinite(g[n]).all()
	_held(f'{tag} g', g[n, :V], r64.g, r32.g, kind)


def _check_field(tag, values, iso=0.0):
	r64, r32 = ref.extract(values, iso, np.float64), ref.extract(values, iso, np.float32)
	out = _nets(values[None], iso)
	assert out[0].shape == (1, len(r64.g), 3) and out[1].shape == (1, len(r64.faces), 3)
	_same_mesh(tag, out, 0, r64, r32)
	return out, r64


def _random_field(shape, seed):
	return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


# ------------------------------------------------------------------ topology and positions
@pytest.mark.parametrize('name', ref.CASES)
def test_cases_of_the_host_file(name):
	out = _nets(ref.field(name)[None])
	_same_mesh(name, out, 0, ref.result(name), ref.result(name, np.float32))


@pytest.mark.parametrize('shape', [(2, 2, 2), (3, 3, 3), (2, 5, 9), (5, 9, 17), (17, 9, 5)], ids=str)
def test_grid_sizes(shape):
	"""Random samples (every corner mask, many lattice faces with four sign changes) and the ellipsoid: a transposed stride shows in either."""
	(g, faces, v_len, f_len, status), r = _check_field(f'random {shape}', _random_field(shape, 3))
	assert v_len[0] > 0 and (f_len[0] > 0) == (sorted(shape)[1] > 2)   # (a quad needs two axes with an interior sample)
	if min(shape) > 2:
		out, r = _check_field(f'ellipsoid {shape}', ref._ellipsoid(shape, np.array(shape) / 170.).astype(np.float32))
		assert ref.closed(out[1][0])


@pytest.mark.parametrize('cells', [255, 256, 257, 513])
def test_thin_grids_on_each_side_of_a_block(cells):
	from find_amd import isosurface
	assert isosurface.BLOCK_CELLS == 256
	for shape in ((2, 2, cells + 1), (cells + 1, 2, 2)):
		(g, faces, v_len, f_len, status), r = _check_field(f'thin {shape}', _random_field(shape, cells))
		assert v_len[0] > cells // 4 and f_len[0] == 0 and status[0] == ref.BOUNDARY
	# with faces: (3, 3, n) has n - 1 interior lattice edges along z and crosses the sample blocks as well
	(g, faces, v_len, f_len, status), r = _check_field(f'thin (3, 3, {cells})', _random_field((3, 3, cells), cells + 1))
	assert f_len[0] > 0


def test_batches():
	"""N = 3 with a sphere, an all-outside field and a plane: each mesh is bit-identical to its own N = 1 run, padded to the batch's maxima."""
	sphere = ref.field('sphere16')
	fields = np.stack([sphere, np.ones_like(sphere), ref._plane((16, 16, 16)).astype(np.float32)])
	batch = _nets(fields)
	assert batch[0].shape[1] == batch[2].max() and batch[1].shape[1] == batch[3].max() and batch[2][1] == 0 and batch[3][1] == 0 and batch[4][1] == 0
	for order in ((0, 1, 2), (2, 0, 1)):
		out = _nets(fields[list(order)])
		for at, n in enumerate(order):
			one = _nets(fields[n:n + 1])
			V, F = one[2][0], one[3][0]
			assert (out[2][at], out[3][at], out[4][at]) == (V, F, one[4][0])
			assert np.array_equal(out[0][at, :V], one[0][0]) and np.array_equal(out[1][at, :F], one[1][0]), 'a mesh depends on its batch'
			assert (out[0][at, V:] == 0).all() and (out[1][at, F:] == -1).all()
			_same_mesh(f'batch {order} mesh {n}', out, at, ref.extract(fields[n]), ref.extract(fields[n], 0., np.float32))


def test_iso_values_a_sample_at_iso_and_a_nan():
	v = ref.field('sphere16').copy()
	for iso in (0.005, -0.0125):
		_check_field(f'sphere16 iso {iso}', v, iso)
	iso = float(v[7, 7, 4])   # a sample (and its mirror images) exactly at iso: outside
	assert (v == np.float32(iso)).sum() >= 1
	(g, faces, v_len, f_len, status), r = _check_field('a sample at iso', v, iso)
	above = float(np.nextafter(np.float32(iso), np.float32(1)))
	out2, r2 = _check_field('a sample one ulp below iso', v, above)
	assert not np.array_equal(r.cellmap, r2.cellmap)
	for bad in (np.nan, np.inf, -np.inf):
		w = v.copy()
		w[8, 8, 8] = bad
		(g, faces, v_len, f_len, status), r = _check_field(f'a {bad} sample', w)
		assert status[0] == ref.NON_FINITE and np.isfinite(g).all() and ref.closed(faces[0])
	w = v.copy()
	w[0, 3, 3] = np.nan   # (outside anyway: only the status changes)
	(g, faces, v_len, f_len, status), r = _check_field('a NaN far outside', w)
	assert status[0] == ref.NON_FINITE and np.array_equal(faces[0], ref.result('sphere16').faces)


# ------------------------------------------------------------------ shape
@pytest.mark.parametrize('name', list(ref.SMOOTH))
def test_smooth_shapes_are_watertight(name):
	"""Every undirected edge in exactly two triangles, once in each direction; the Euler characteristic; bit 1.  On the restatement first."""
	r = ref.result(name)
	g, faces, v_len, f_len, status = _nets(ref.field(name)[None])
	for who, f, st in (('restatement', r.faces, r.status), ('HIP', faces[0, :f_len[0]], status[0])):
		assert ref.watertight(f), who
		assert ref.euler(f) == ref.SMOOTH[name], who
		assert st == (ref.BOUNDARY if name == 'sphere8' else 0), who   # (the 8^3 sphere's second sample layer is inside: the bit is conservative)
	assert ref.exact_volume(g[0], faces[0]) > 0
	plane = _nets(ref.field('plane')[None])
	assert plane[4][0] == ref.BOUNDARY == ref.result('plane').status and not ref.closed(plane[1][0])


# ------------------------------------------------------------------ capacities
def _raw(values, iso, vcap, fcap, canary=64):
	"""The C calls on buffers with `canary` rows behind the capacities: (g, faces, both with the canary rows, v_len, f_len, status)."""
	from find_amd import _lib
	from find_amd._lib import check, current_stream, ptr
	L = _lib.lib()
	v = _t(values)
	N, nx, ny, nz = v.shape
	assert N == 1
	ws = torch.full((L.find_surface_nets_ws_bytes(N, nx, ny, nz),), 0xA5, dtype=torch.uint8, device='cuda')
	v_len, f_len = torch.full((N,), -7, dtype=torch.int64, device='cuda'), torch.full((N,), -7, dtype=torch.int64, device='cuda')
	status = torch.full((N,), -7, dtype=torch.int32, device='cuda')
	g = torch.full((vcap + canary, 3), 12345.5, dtype=torch.float32, device='cuda')
	faces = torch.full((fcap + canary, 3), 424242, dtype=torch.int32, device='cuda')
	st = current_stream(v.device)
	check(L.find_surface_nets_count(ptr(v), iso, N, nx, ny, nz, ptr(v_len), ptr(f_len), ptr(status), ptr(ws), ws.numel(), st), 'count')
	check(L.find_surface_nets_emit(ptr(v), iso, N, nx, ny, nz, ptr(v_len), ptr(f_len), vcap, fcap, ptr(g), ptr(faces), ptr(status), ptr(ws), ws.numel(), st), 'emit')
	torch.cuda.synchronize()
	return g.cpu().numpy(), faces.cpu().numpy(), int(v_len[0]), int(f_len[0]), int(status[0])


@pytest.mark.parametrize('name', ['sphere16', 'plane'])
def test_capacities(name):
	values = ref.field(name)[None]
	r = ref.result(name)
	V, F = len(r.g), len(r.faces)
	read_back = _nets(values)
	exact = _nets(values, 0., V, F)
	for a, b in zip(read_back, exact):
		assert np.array_equal(a, b), 'exact capacities differ from the read-back path'
	roomy = _nets(values, 0., V + 37, F + 5)
	assert roomy[0].shape == (1, V + 37, 3) and roomy[1].shape == (1, F + 5, 3) and roomy[4][0] == r.status
	assert np.array_equal(roomy[0][0, :V], exact[0][0]) and (roomy[0][0, V:] == 0).all() and np.array_equal(roomy[1][0, :F], exact[1][0]) and (roomy[1][0, F:] == -1).all()
	for dv, df, bits in ((1, 0, ref.VERTS_OVERFLOW), (0, 1, ref.FACES_OVERFLOW), (1, 1, ref.VERTS_OVERFLOW | ref.FACES_OVERFLOW), (V, F, ref.VERTS_OVERFLOW | ref.FACES_OVERFLOW)):
		g, faces, v_len, f_len, status = _nets(values, 0., V - dv, F - df)
		assert (v_len[0], f_len[0], status[0]) == (V, F, r.status | bits) and g.shape == (1, V - dv, 3) and faces.shape == (1, F - df, 3)
		if dv == 0:
			assert np.array_equal(g, exact[0])
		if df == 0:
			assert np.array_equal(faces, exact[1])
	# nothing at or past the capacity is written: too small, exact and roomy
	for vcap, fcap in ((V - 1, F - 1), (V, F), (V + 3, F + 3), (0, 0), (V // 2, F // 2 + 1)):
		g, faces, v_len, f_len, status = _raw(values, 0., vcap, fcap)
		assert (v_len, f_len) == (V, F) and status == (r.status | (ref.VERTS_OVERFLOW if vcap < V else 0) | (ref.FACES_OVERFLOW if fcap < F else 0))
		assert (g[vcap:] == 12345.5).all() and (faces[fcap:] == 424242).all(), 'the canary behind the capacity was written'
		assert not (g[:vcap] == 12345.5).any() and not (faces[:fcap] == 424242).any(), 'a row below the capacity was left unwritten'


# ------------------------------------------------------------------ gradients
@pytest.mark.parametrize('name', ['sphere16', 'ellipsoid (5, 9, 17)'])
def test_gradients(name):
	"""d / d values and d / d iso of sum g . r, r fixed and random, against float64 autograd through the restatement with the topology held;
	origin and spacing through extract_surface."""
	from find_amd import isosurface
	values = ref.field(name) if name == 'sphere16' else ref._ellipsoid((5, 9, 17), np.array((5, 9, 17)) / 170.).astype(np.float32)
	iso = 0.0025 if name == 'sphere16' else 0.0
	r64 = ref.extract(values, iso)
	V = len(r64.g)
	rr = torch.from_numpy(np.random.RandomState(5).standard_normal((V, 3))).double()
	refs = {}
	for dt in (torch.float64, torch.float32):
		v = torch.from_numpy(values).to(dt).requires_grad_(True)
		i = torch.tensor(iso, dtype=torch.float32).to(dt).requires_grad_(True)
		g = ref.g_torch(v, i)
		refs[dt] = torch.autograd.grad((g * rr.to(dt)).sum(), (v, i)) + (g.detach(),)
	assert np.abs(refs[torch.float64][2].numpy() - r64.g).max() <= 1e-13

	def run():
		v = _t(values[None]).requires_grad_(True)
		i = torch.tensor(iso, dtype=torch.float32, device='cuda', requires_grad=True)
		g = isosurface._SurfaceNets.apply(v, i, float(i.detach()), None, None)[0]
		assert g.requires_grad and g.shape == (1, V, 3)
		return torch.autograd.grad((g * rr.float().cuda()).sum(), (v, i))
	(gv, gi), (gv2, gi2) = run(), run()
	assert torch.equal(gv, gv2) and torch.equal(gi, gi2), 'two runs differ'
	assert gv.shape == (1,) + values.shape and torch.isfinite(gv).all()
	_held(f'{name} grad_values', gv[0], refs[torch.float64][0], refs[torch.float32][0], 'grad_values')
	_held(f'{name} grad_iso', gi, refs[torch.float64][1], refs[torch.float32][1], 'grad_iso')
	# samples that touch no active cell have no gradient, exactly
	assert (gv[0].cpu()[refs[torch.float64][0] == 0] == 0).all()
	# origin, spacing: verts = origin + (g + 0.5) spacing, formed in torch
	origin = torch.tensor([[-0.06, -0.05, -0.04]], device='cuda', requires_grad=True)
	spacing = torch.tensor([[0.0075, 0.005, 0.0025]], device='cuda', requires_grad=True)
	v = _t(values[None]).requires_grad_(True)
	verts, faces, v_len, f_len, status = isosurface.extract_surface(v, origin, spacing, iso)
	assert not faces.requires_grad and verts.shape == (1, V, 3) and int(v_len[0]) == V
	go, gs, gv3 = torch.autograd.grad((verts[0] * rr.float().cuda()).sum(), (origin, spacing, v))
	want = {}
	for dt in (torch.float64, torch.float32):
		o, s = origin.detach().cpu().to(dt).requires_grad_(True), spacing.detach().cpu().to(dt).requires_grad_(True)
		vv = torch.from_numpy(values).to(dt).requires_grad_(True)
		w = o + (ref.g_torch(vv, torch.tensor(iso, dtype=torch.float32).to(dt)) + 0.5) * s
		want[dt] = torch.autograd.grad((w * rr.to(dt)).sum(), (o, s, vv)) + (w.detach(),)
	_held(f'{name} verts', verts[0], want[torch.float64][3], want[torch.float32][3], 'verts')
	_held(f'{name} grad_origin', go, want[torch.float64][0], want[torch.float32][0], 'grad_origin')
	_held(f'{name} grad_spacing', gs, want[torch.float64][1], want[torch.float32][1], 'grad_spacing')
	_held(f'{name} grad_values through spacing', gv3[0], want[torch.float64][2], want[torch.float32][2], 'grad_values')


# ------------------------------------------------------------------ remesh
_TEMPLATE = {}


def _template(opened):
	if opened not in _TEMPLATE:
		from find_amd import synthetic
		v, f = (x.numpy() for x in synthetic.template(1002))
		if opened:
			f = inside_ref.without_top(v, f, 0.15)
		_TEMPLATE[opened] = (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int64))
	return _TEMPLATE[opened]


def _remesh_case(opened, res, offset):
	from find_amd import inside, isosurface
	v, f = _template(opened)
	V, F = _t(v[None]), _t(f, torch.int64)
	sdf, origin, spacing = isosurface.field_grid(V, F, res, offset)
	assert sdf.shape == (1, res, res, res) and sdf.dtype == torch.float32 and not sdf.requires_grad
	# the grid: samples 1 .. res - 2 from lo to hi of the grown box, one layer a full spacing beyond
	lo, hi = v.min(0) - (max(offset, 0.) + 0.005), v.max(0) + (max(offset, 0.) + 0.005)
	assert np.allclose(spacing.cpu().numpy()[0], (hi - lo) / (res - 3), rtol=1e-6) and np.allclose((origin + 1.5 * spacing).cpu().numpy()[0], lo, atol=1e-7)
	direct = inside.signed_distance(inside.grid_points(origin, spacing, res, 0, res ** 3), V, F)[0]
	assert torch.equal(sdf.view(1, -1), direct), 'field_grid is not signed_distance at grid_points'
	out = isosurface.remesh(V, F, res, offset)
	again = isosurface.remesh(V, F, res, offset)
	assert all(torch.equal(a, b) for a, b in zip(out, again)), 'two runs differ'
	verts, faces, v_len, f_len, status = (x.cpu().numpy() for x in out)
	field = sdf[0].cpu().numpy()
	r64, r32 = ref.extract(field, offset), ref.extract(field, offset, np.float32)
	nv, nf = len(r64.g), len(r64.faces)
	assert (v_len[0], f_len[0], status[0]) == (nv, nf, r64.status) and np.array_equal(faces[0], r64.faces)
	o, s = origin[0].cpu().numpy(), spacing[0].cpu().numpy()
	w64 = o.astype(np.float64) + (r64.g + 0.5) * s.astype(np.float64)
	w32 = o + (r32.g + np.float32(0.5)) * s
	assert w32.dtype == np.float32
	_held(f'remesh opened {opened} res {res} offset {offset} verts', verts[0], w64, w32, 'remesh verts')
	for who, ff, st in (('restatement', r64.faces, r64.status), ('HIP', faces[0], status[0])):
		assert ref.watertight(ff) and ref.euler(ff) == 2 and st == 0, who
	return V, F, verts[0], w64, w32


@pytest.mark.parametrize('res', [16, 32])
@pytest.mark.parametrize('opened', [False, True], ids=['closed', 'opened'])
def test_remesh(opened, res):
	V, F, verts, w64, w32 = _remesh_case(opened, res, 0.0)
	v, f = _template(False)
	from find_amd import isosurface
	m = isosurface.remesh(V, F, res, as_meshes=True)
	assert m.verts_padded().shape == (1, len(verts), 3) and np.array_equal(m.verts_padded()[0].cpu().numpy(), verts)
	exact = inside_ref.exact_volume(v, f)
	got = ref.exact_volume(verts, m.faces_padded()[0].cpu().numpy())
	print(f'remesh opened {opened} res {res}: volume {got * 1e6:.2f} ml, the closed template {exact * 1e6:.2f} ml, {100 * (got / exact - 1):.2f} % off')
	assert got > 0


@pytest.mark.parametrize('res', [16, 32])
def test_offset_surface_of_the_closed_template(res):
	"""The distance of every output vertex to the input mesh against 0.003: within the restatement's own worst deviation on that grid, measured
	in float64, with a margin of 4 e32 (e32: the float32 restatement's vertices against the float64 ones; a distance is 1-Lipschitz)."""
	from find_amd import functional as FN
	offset = 0.003
	V, F, verts, w64, w32 = _remesh_case(False, res, offset)
	v, f = _template(False)
	d64 = SR.point_face(torch.from_numpy(w64), torch.from_numpy(v).double(), torch.from_numpy(f))['dist2'].sqrt().numpy()
	dev64 = np.abs(d64 - offset).max()
	e32 = np.sqrt(((w32.astype(np.float64) - w64) ** 2).sum(1)).max()
	d_hip = FN.point_face_distance(_t(verts[None]), V, F)[0][0].sqrt().cpu().numpy().astype(np.float64)
	dev_hip = np.abs(d_hip - offset).max()
	print(f'offset 0.003 at res {res}: the restatement deviates by {dev64:.3e}, HIP by {dev_hip:.3e}, e32 {e32:.3e}, (dev_hip - dev64) / e32 {(dev_hip - dev64) / e32:.2f}')
	assert dev_hip <= dev64 + 4 * e32
	assert (d_hip > 0).all()   # outside the mesh everywhere


# ------------------------------------------------------------------ poison
def test_poisoned_allocations():
	"""g, faces, the counts, the status, the workspaces, the gradients and the field of find_amd.isosurface are torch.empty: whatever they hold
	before the call, the results are the same bits.  The workspaces come from functional._ws, which tests/poison.py covers; the module itself is
	given the harness's proxy for its module-level `torch` here, as tests/test_gpu_inside.py does for its module."""
	from find_amd import isosurface as module
	sphere = ref.field('sphere16')
	fields = _t(np.stack([sphere, np.ones_like(sphere), ref._plane((16, 16, 16)).astype(np.float32)]))
	origin, spacing = torch.tensor([-0.06, -0.06, -0.06], device='cuda'), torch.tensor([0.0075, 0.0075, 0.0075], device='cuda')
	V = len(ref.result('sphere16').g)
	rr = _t(np.random.RandomState(6).standard_normal((3, 1, 3)))
	tv, tf = _template(True)
	TV, TF = _t(tv[None]), _t(tf, torch.int64)

	def run():
		out = dict(zip(('verts', 'faces', 'v_len', 'f_len', 'status'), module.extract_surface(fields, origin, spacing)))
		out.update(zip(('c_verts', 'c_faces', 'c_v_len', 'c_f_len', 'c_status'), module.extract_surface(fields, origin, spacing, 0.001, V // 2, 3 * V)))
		v = fields.clone().requires_grad_(True)
		i = torch.tensor(0.002, device='cuda', requires_grad=True)
		o, s = origin.clone().requires_grad_(True), spacing.clone().requires_grad_(True)
		verts = module.extract_surface(v, o, s, i)[0]
		out.update(zip(('d_values', 'd_iso', 'd_origin', 'd_spacing'), torch.autograd.grad((verts * rr).sum(), (v, i, o, s))))
		sdf, go, gs = module.field_grid(TV, TF, 12)
		out.update(sdf=sdf, grid_origin=go, grid_spacing=gs)
		out.update(zip(('r_verts', 'r_faces', 'r_v_len', 'r_f_len', 'r_status'), module.remesh(TV, TF, 12)))
		torch.cuda.synchronize()
		return {k: x.detach() for k, x in out.items()}

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
		assert proxy.calls >= 25, proxy.calls   # five outputs and a workspace per extraction, the gradients, the field, the distance's buffers
	assert clean['c_status'][0].item() == ref.VERTS_OVERFLOW and clean['c_status'][1].item() == 0 and clean['r_status'].tolist() == [0]
	bad = poison.compare('isosurface', clean, runs[0], runs[1])
	assert not bad, '\n'.join(bad)


def test_zz_worst_ratios():
	"""Prints the worst e_hip / max(e32, ulp) per quantity over the file's cases."""
	for k, v in sorted(WORST.items()):
		print(f'worst {k}: {v:.3f}')
	assert all(v <= 4. for v in WORST.values())
