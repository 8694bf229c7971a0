"""Foot measurements on the MI355X: find_plane_sections_* / find_extents_* through find_amd.measure against the float64 torch restatement of
the rule (tests/measure_ref.py) on the same fp32 inputs, and their place in losses, eval_metrics and evaluate.eval_3d.

Margins: none is a constant of the code under test.  Counts of crossing faces must be equal: every case is drawn so that, in float64, each
vertex lies at least 1e-5 of the mesh's extent away from each plane (the generator asserts it), far more than the 2e-7 or so by which the
fp32 fma chain can misplace a signed distance.  Every float comparison also evaluates the same reference in float32 on the CPU; with e32
its worst error against float64 over the case's tensor, the HIP result must lie within max(4 e32, 2 ulp of the largest value) of the
float64 one (the kernel sums in another order than torch, hence the factor).  Each case prints its figures (DESIGN 7.9 records the worst).

Shapes: a workgroup takes 256 faces.  Random triangle soup of F = 1, 255, 256, 257 faces (less than a wave, one short of a workgroup, one
workgroup, one more), the 80-face closed ellipsoid, and the 13 776-face template once; N = 1 and 3; P = 1, 5 and 64 planes.  A single face
cut by a single plane gives one number, whose float32 reference error is 0 by chance too often to size a bound from: F = 1 runs with 5
and 64 planes, so each (F, N, P) below holds at least five numbers."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import poison   # noqa: E402
from measure_ref import cube, ellipse_perimeter, extents_ref, octahedron, plane_sections_ref   # noqa: E402

WORST = {}   # name of a quantity -> the worst e_hip / max(e32, ulp) seen (printed by the last test of the file)


def _ulp(x):
	return float(np.spacing(np.float32(abs(float(x)))))


def _held(name, hip, ref64, ref32, kind=None):
	hip, ref64, ref32 = hip.detach().double().cpu(), ref64.detach().double(), ref32.detach().double()
	assert hip.shape == ref64.shape, (name, hip.shape, ref64.shape)
	e_hip = (hip - ref64).abs().max().item()
	e32 = (ref32 - ref64).abs().max().item()
	ulp = _ulp(ref64.abs().max().item())
	ratio = e_hip / max(e32, ulp)
	print(f'{name}: e_hip {e_hip:.3e}  e32 {e32:.3e}  ulp {ulp:.3e}  scale {ref64.abs().max().item():.3e}  e_hip / max(e32, ulp) {ratio:.2f}')
	if kind:
		WORST[kind] = max(WORST.get(kind, 0.), ratio)
	assert np.isfinite(e_hip) and e_hip <= max(4 * e32, 2 * ulp), (name, e_hip, e32, ulp)


# ------------------------------------------------------------------ inputs
def _soup(F, N, g):
	"""Random triangles over few enough vertices that they share them: verts (N, V, 3) in [-1, 1]^3, faces (F, 3)."""
	V = max(4, F // 2)
	verts = torch.rand(N, V, 3, generator=g) * 2 - 1
	faces = torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(F)])
	return verts, faces


def _planes(verts, P, per_mesh, g, miss=True):
	"""P planes (shared: (P, 4), per mesh: (N, P, 4)) with fp32 unit normals, offsets inside the range of n . v over the mesh(es) -- the last one
	beyond it when `miss` and P > 1 -- redrawn until, in float64, every vertex is at least 1e-5 of the extent away from every plane."""
	N = verts.shape[0]
	v64 = verts.double()
	extent = (v64.reshape(-1, 3).max(0).values - v64.reshape(-1, 3).min(0).values).max().item()
	out = torch.empty(N if per_mesh else 1, P, 4)
	for b in range(out.shape[0]):
		cloud = v64[b] if per_mesh else v64.reshape(-1, 3)
		for p in range(P):
			n = torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0)
			s = cloud @ n.double()
			for _ in range(1000):
				if miss and P > 1 and p == P - 1:
					d = (s.max() + 0.1 * extent * (1 + torch.rand((), generator=g).double())).float()
				else:
					u = 0.15 + 0.7 * torch.rand((), generator=g).double()
					d = (s.min() + u * (s.max() - s.min())).float()
				if (s - d.double()).abs().min().item() >= 1e-5 * extent:
					break
			out[b, p, :3], out[b, p, 3] = n, d
	full = out.double().expand(N, -1, -1)
	dist = (torch.einsum('nvk,npk->npv', v64, full[..., :3]) - full[..., 3:]).abs().min().item()
	assert dist >= 1e-5 * extent, (dist, extent)
	return out if per_mesh else out[0]


def _odd_faces(faces, V):
	"""faces plus a -1 row, a row with an index outside [0, V) and a row with a repeated vertex, in the middle of the list."""
	odd = torch.tensor([[-1, -1, -1], [0, V + 3, 1], [2, 2, min(3, V - 1)]], dtype=faces.dtype)
	h = faces.shape[0] // 2
	return torch.cat([faces[:h], odd, faces[h:]])


def _hip(verts, faces, planes, weight):
	from find_amd.measure import plane_sections
	vs, ps = verts.detach().cuda().requires_grad_(), planes.detach().cuda().requires_grad_()
	per, cnt = plane_sections(vs, faces.cuda(), ps, return_count=True)
	assert per.dtype == torch.float32 and cnt.dtype == torch.int32 and not cnt.requires_grad and per.shape == cnt.shape == weight.shape
	(per * weight.cuda()).sum().backward()
	torch.cuda.synchronize()
	assert (ps.grad[..., :3] == 0).all()   # the normals are taken as given
	return per.detach(), cnt, vs.grad, ps.grad[..., 3]


def _ref(dtype, verts, faces, planes, weight):
	vs = verts.detach().clone().to(dtype).requires_grad_()
	off = planes[..., 3].detach().clone().to(dtype).requires_grad_()
	per, cnt = plane_sections_ref(vs, faces, torch.cat([planes[..., :3].to(dtype), off[..., None]], -1))
	(per * weight.to(dtype)).sum().backward()
	return per.detach(), cnt, vs.grad, off.grad


def _against_float64(name, verts, faces, planes, seed=0):
	weight = torch.rand(verts.shape[0], planes.shape[-2], generator=torch.Generator().manual_seed(seed)) + 0.5
	got = _hip(verts, faces, planes, weight)
	r64, r32 = _ref(torch.float64, verts, faces, planes, weight), _ref(torch.float32, verts, faces, planes, weight)
	assert torch.equal(got[1].cpu().long(), r64[1]), (name, got[1].cpu().tolist(), r64[1].tolist())
	for what, k in (('perimeter', 0), ('d_verts', 2), ('d_offset', 3)):
		_held(f'{name} {what}', got[k], r64[k], r32[k], kind=what)
	return got, r64


# ------------------------------------------------------------------ exact cases
def test_exact_cases():
	"""Small-integer meshes, where every fp32 operation of the rule is exact up to the square root."""
	from find_amd.measure import plane_sections
	v, f = octahedron(torch.float32)
	planes = torch.tensor([[0., 0., 1., 0.], [0., 0., 1., 1.], [0., 0., 1., -1.], [0., 0., 1., 2.]])
	want_cnt, want = [4, 4, 0, 0], [4 * 2 ** 0.5, 0., 0., 0.]
	per, cnt = plane_sections(v[None].cuda(), f.cuda(), planes.cuda(), return_count=True)
	r64, c64 = plane_sections_ref(v[None].double(), f, planes.double())
	assert cnt.cpu().tolist() == [want_cnt] == c64.tolist()
	for p in range(4):
		assert abs(per[0, p].item() - want[p]) <= 2 * _ulp(want[p]) and abs(r64[0, p].item() - want[p]) < 1e-15, p
		alone, c1 = plane_sections(v[None].cuda(), f.cuda(), planes[p:p + 1].cuda(), return_count=True)
		assert torch.equal(alone[0, 0], per[0, p]) and c1.item() == want_cnt[p]
	v, f = cube(torch.float32)
	planes = torch.tensor([[0., 0., 1., 1.], [0., 0., 1., 0.5], [0., 0., 1., 0.], [1., 0., 0., 0.25]])
	per, cnt = plane_sections(v[None].cuda(), f.cuda(), planes.cuda(), return_count=True)
	assert cnt.cpu().tolist() == [[8, 8, 0, 8]] and per.cpu().tolist() == [[4., 4., 0., 4.]]


# ------------------------------------------------------------------ forward and backward against float64
CASES = [('soup', 1, 1, 5), ('soup', 1, 3, 64), ('soup', 255, 1, 1), ('soup', 255, 3, 5), ('soup', 256, 1, 5), ('soup', 256, 3, 1), ('soup', 257, 1, 64),
		 ('soup', 257, 3, 5), ('ellipsoid', 80, 1, 1), ('ellipsoid', 80, 3, 5), ('ellipsoid', 80, 3, 64), ('template', 13776, 3, 5)]


@pytest.mark.parametrize('kind,F,N,P', CASES, ids=lambda c: str(c))
def test_sections_against_float64(kind, F, N, P):
	from find_amd import synthetic
	g = torch.Generator().manual_seed(1000 * F + 10 * N + P)
	if kind == 'soup':
		verts, faces = _soup(F, N, g)
	else:
		v, faces = synthetic.ellipsoid_mesh(5, 8) if kind == 'ellipsoid' else synthetic.template(6890)
		verts = v[None] * (0.8 + 0.4 * torch.rand(N, 1, 3, generator=g)) + 0.002 * v.abs().max() * torch.randn(N, v.shape[0], 3, generator=g)
	assert faces.shape[0] == F
	V = verts.shape[1]
	for shared_planes in (True, False):
		planes = _planes(verts, P, not shared_planes, g)
		tag = f'{kind} F={F} N={N} P={P} {"shared" if shared_planes else "per-mesh"} planes'
		(per, cnt, d_v, d_o), _ = _against_float64(tag + ', shared faces', verts, faces, planes)
		assert d_v.shape == verts.shape and d_o.shape == planes.shape[:-1]
		if P > 1:
			assert (cnt[..., -1] == 0).all() and (per[..., -1] == 0).all()   # the plane that misses
		if F > 1 and V > 4:
			odd = _odd_faces(faces, V)
			got, _ = _against_float64(tag + ', shared faces with odd rows', verts, odd, planes)
			assert torch.equal(got[1], cnt)   # (they contribute nothing)
	if F > 1 and V > 4 and F < 1000:
		# per-mesh faces: each mesh keeps another part of the list, the rest padded with -1 rows; one odd row each
		ragged = torch.stack([torch.cat([_odd_faces(faces[:F - 7 * n], V), torch.full((7 * n, 3), -1, dtype=faces.dtype)]) for n in range(N)])
		planes = _planes(verts, P, True, g)
		_against_float64(f'{kind} F={F} N={N} P={P} per-mesh planes, per-mesh faces', verts, ragged.to(torch.int32), planes)


def test_shared_vertex_of_two_sections_and_tangent_plane():
	"""The top vertex of the octahedron belongs to faces that plane z = 0.5 cuts and to faces that plane x = 0.25 cuts: its gradient is the sum
	over both planes.  Plane z = 1 touches it: four crossing faces of length 0, a finite zero gradient."""
	from find_amd.measure import plane_sections
	v, f = octahedron(torch.float32)
	planes = torch.tensor([[0., 0., 1., 0.5], [1., 0., 0., 0.25], [0., 0., 1., 1.]])
	(per, cnt, d_v, d_o), (_, _, g64, _) = _against_float64('octahedron, two sections and a tangent plane', v[None], f, planes)
	assert cnt.cpu().tolist() == [[4, 4, 4]] and per[0, 2].item() == 0. and d_o[2].item() == 0.
	one = [_hip(v[None], f, planes[p:p + 1], torch.ones(1, 1))[2] for p in range(3)]
	assert one[0][0, 4].abs().max() > 0 and one[1][0, 4].abs().max() > 0      # the top vertex moves both sections
	assert torch.isfinite(one[2]).all() and (one[2] == 0).all()               # and the tangent plane moves nothing
	vs = v[None].cuda().requires_grad_()
	ps = planes[2:].cuda().requires_grad_()
	plane_sections(vs, f.cuda(), ps).sum().backward()
	assert (vs.grad == 0).all() and (ps.grad == 0).all()


def test_two_runs_agree_bit_for_bit_and_a_row_does_not_depend_on_the_batch():
	from find_amd import synthetic
	g = torch.Generator().manual_seed(77)
	v, faces = synthetic.ellipsoid_mesh(12, 23)   # 552 faces: three workgroups
	verts = v[None] * (0.8 + 0.4 * torch.rand(3, 1, 3, generator=g))
	weight = torch.rand(3, 5, generator=g) + 0.5
	for per_mesh in (False, True):
		planes = _planes(verts, 5, per_mesh, g)
		a, b = _hip(verts, faces, planes, weight), _hip(verts, faces, planes, weight)
		assert all(torch.equal(p, q) for p, q in zip(a, b))
		for n in range(3):
			alone = _hip(verts[n:n + 1], faces, planes[n:n + 1] if per_mesh else planes, weight[n:n + 1])
			assert torch.equal(alone[0][0], a[0][n]) and torch.equal(alone[1][0], a[1][n]) and torch.equal(alone[2][0], a[2][n]), (per_mesh, n)
			if per_mesh:
				assert torch.equal(alone[3][0], a[3][n])
	# no gradient asked for: the same values
	from find_amd.measure import plane_sections
	with torch.no_grad():
		assert torch.equal(plane_sections(verts.cuda().requires_grad_(), faces.cuda(), planes.cuda()), a[0])


# ------------------------------------------------------------------ extents
def test_extents():
	from find_amd.measure import extents
	g = torch.Generator().manual_seed(5)
	dirs = torch.nn.functional.normalize(torch.randn(8, 3, generator=g), dim=1)
	for V in (1, 63, 1024, 1025, 3000):
		verts = torch.rand(3, V, 3, generator=g) * 2 - 1
		for D in (1, 3, 8):
			lo, hi, alo, ahi = extents(verts.cuda(), dirs[:D].cuda(), return_index=True)
			r, r32 = extents_ref(verts.double(), dirs[:D].double()), extents_ref(verts, dirs[:D])
			_held(f'extents V={V} D={D} lo', lo, r[0], r32[0], kind='extents')
			_held(f'extents V={V} D={D} hi', hi, r[1], r32[1], kind='extents')
			# the vertex named is an extreme one (two vertices within fp32 rounding of each other may swap places against float64)
			s64 = torch.einsum('nvk,dk->ndv', verts.double(), dirs[:D].double())
			for arg, val in ((alo, r[0]), (ahi, r[1])):
				at = torch.gather(s64, 2, arg.cpu().long()[..., None])[..., 0]
				assert (arg >= 0).all() and (arg < V).all() and ((at - val).abs() <= 2 * _ulp(val.abs().max())).all(), (V, D)
			# along the axes the projection is the coordinate itself: the same vertex as in float64
			lo, hi, alo, ahi = extents(verts.cuda(), torch.eye(3)[:min(D, 3)].cuda(), return_index=True)
			r = extents_ref(verts.double(), torch.eye(3, dtype=torch.float64)[:min(D, 3)])
			assert torch.equal(alo.cpu().long(), r[2]) and torch.equal(ahi.cpu().long(), r[3]) and torch.equal(lo.cpu().double(), r[0]) and torch.equal(hi.cpu().double(), r[1])
	# ties go to the smallest index: a mesh whose vertices all appear twice more, far apart in the list (other threads, other waves)
	base = torch.rand(1, 700, 3, generator=g)
	verts = torch.cat([base, base, base], 1)
	lo, hi, alo, ahi = extents(verts.cuda(), torch.eye(3).cuda(), return_index=True)
	assert (alo < 700).all() and (ahi < 700).all()
	assert torch.equal(alo.cpu().long()[0], base[0].argmin(0)) and torch.equal(ahi.cpu().long()[0], base[0].argmax(0))
	assert torch.equal(lo.cpu()[0], base[0].min(0).values) and torch.equal(hi.cpu()[0], base[0].max(0).values)
	# v_len shorter than V, NaN in the padding rows
	verts = torch.rand(3, 1500, 3, generator=g)
	v_len = torch.tensor([1500, 1100, 7])
	padded = verts.clone()
	for n in range(3):
		padded[n, int(v_len[n]):] = float('nan')
	got = extents(padded.cuda(), torch.eye(3).cuda(), v_len.cuda(), return_index=True)
	for n in range(3):
		k = int(v_len[n])
		alone = extents(verts[n:n + 1, :k].contiguous().cuda(), torch.eye(3).cuda(), return_index=True)
		assert all(torch.equal(a[n], b[0]) for a, b in zip(got, alone)) and torch.isfinite(got[0][n]).all(), n
	# v_len = 0
	got = extents(padded.cuda(), torch.eye(3)[:2].cuda(), torch.tensor([0, 1500, 0]).cuda(), return_index=True)
	assert (got[0][[0, 2]] == 0).all() and (got[1][[0, 2]] == 0).all() and (got[2][[0, 2]] == -1).all() and (got[3][[0, 2]] == -1).all()
	assert (got[2][1] >= 0).all()


def test_extents_backward_is_exact():
	"""d_verts is +-dir at the arg vertices, added in the order lo_0, hi_0, lo_1, ...; vertex 0 is the maximum of two directions."""
	from find_amd.measure import extents
	g = torch.Generator().manual_seed(6)
	verts = torch.rand(2, 300, 3, generator=g) * 2 - 1
	verts[:, 0] = torch.tensor([5., 5., 0.])
	dirs = torch.tensor([[1., 0., 0.], [0., 1., 0.], [0.6, 0., 0.8], [0.3, 0.4, -0.5]])
	vs = verts.cuda().requires_grad_()
	lo, hi, alo, ahi = extents(vs, dirs.cuda(), return_index=True)
	assert (ahi[:, :2] == 0).all()
	w_lo, w_hi = torch.rand(2, 4, generator=g), torch.rand(2, 4, generator=g)
	((hi * w_hi.cuda()).sum() - (lo * w_lo.cuda()).sum()).backward()
	want = torch.zeros(2, 300, 3)
	for n in range(2):
		for d in range(4):
			want[n, int(alo[n, d])] += -w_lo[n, d] * dirs[d]
			want[n, int(ahi[n, d])] += w_hi[n, d] * dirs[d]
	assert torch.equal(vs.grad.cpu(), want) and (vs.grad[:, 0, :2] != 0).all()
	# v_len 0: nothing lands anywhere
	vs = verts.cuda().requires_grad_()
	lo, hi = extents(vs, dirs.cuda(), torch.tensor([0, 300]).cuda())
	(hi - lo).sum().backward()
	assert (vs.grad[0] == 0).all() and (vs.grad[1] != 0).any()


# ------------------------------------------------------------------ foot_measurements
def test_foot_measurements_against_closed_forms():
	"""synthetic.template(6890) is a latitude-longitude ellipsoid of 84 rings (polar angles k pi / 85) and 82 segments: its vertices reach
	+-a cos(pi / 170) along x (segments 0 and 41 on the rings next to the equator) and +-b cos(pi / 170) cos(pi / 82) along y -- the closed
	forms of ITS length and width, scaled per foot; no vertex lies on the ellipsoid's own poles (2a, 2b are 1.7e-4 and 9e-4 away).  A value is the
	difference of two fp32 coordinates, each rounded when the template is made and again when it is scaled, rounded once more: 4 ulp.
	The girths: sections at 0.68 and 0.50 of that length, against the perimeter of the ellipsoid's own section there, 5e-4 relative."""
	import math
	from find_amd import measure, synthetic
	v, f = synthetic.template(6890)
	scale = torch.tensor([[1., 1., 1.], [0.9, 1.1, 1.05], [1.1, 0.95, 0.9]])
	verts = (v[None] * scale[:, None]).cuda().requires_grad_()
	values, names = measure.foot_measurements(verts, f.cuda())
	assert names == ('length', 'width', 'ball_girth', 'instep_girth') and values.shape == (3, 4) and values.dtype == torch.float32
	a, b, c = 0.12, 0.045, 0.04
	k = math.cos(math.pi / 170)
	for n in range(3):
		sx, sy, sz = (float(s) for s in scale[n].double())
		length, width = 2 * a * sx * k, 2 * b * sy * k * math.cos(math.pi / 82)
		assert abs(values[n, 0].item() - length) <= 4 * _ulp(length) and abs(values[n, 1].item() - width) <= 4 * _ulp(width), n
		for col, frac in ((2, 0.68), (3, 0.50)):
			x0 = (2 * frac - 1) * a * sx * k
			r = math.sqrt(1 - (x0 / (a * sx)) ** 2)
			want = ellipse_perimeter(b * sy * r, c * sz * r)
			rel = abs(values[n, col].item() - want) / want
			print(f'foot {n} {names[col]}: {values[n, col].item():.6f} m, ellipse {want:.6f} m, relative difference {rel:.2e}')
			assert rel < 5e-4, (n, col, rel)
	# a girth moves with the heel-most vertex: it moves the plane
	_, _, alo, ahi = measure.extents(verts.detach(), [(1., 0., 0.)], return_index=True)
	values[:, 2].sum().backward()
	for n in range(3):
		assert verts.grad[n, int(alo[n, 0]), 0].item() != 0 and verts.grad[n, int(ahi[n, 0]), 0].item() != 0, n
	assert torch.isfinite(verts.grad).all()
	# a Meshes gives the same numbers
	from find_amd.structures import Meshes
	again, _ = measure.of_meshes(Meshes(verts.detach(), f.cuda()))
	assert torch.equal(again, values.detach())


# ------------------------------------------------------------------ loss and evaluation
def test_measurement_loss():
	from find_amd import measure, synthetic
	from find_amd.losses import MeasurementLoss
	n = 3
	model = synthetic.make_model(1002, train_size=n, val_size=1)
	lat = {k: t.clone().requires_grad_() for k, t in synthetic.latents(n, seed=2).items()}
	faces = model.template_faces.data[0]
	verts = model.get_meshes(**lat)['verts']
	own, names = measure.foot_measurements(verts.detach(), faces)
	assert own.shape == (n, 4) and (own > 0).all()
	target = own * torch.tensor([1.05, 0.97, 1.02, 0.99], device='cuda')
	for relative in (False, True):
		loss = MeasurementLoss(relative=relative)(verts, faces, target)
		d = (own - target) / (target if relative else 1.)
		assert loss.dim() == 0 and torch.allclose(loss.detach(), (d * d).mean(), rtol=1e-5, atol=0)
		grad, = torch.autograd.grad(loss, lat['shapevec'], retain_graph=True)
		assert torch.isfinite(grad).all() and grad.abs().max().item() > 0, relative
	# a NaN entry is "not measured": the mean runs over the others
	holes = target.clone()
	holes[0, 2] = holes[2, 0] = float('nan')
	keep = ~torch.isnan(holes)
	loss = MeasurementLoss()(verts, faces, holes)
	assert torch.allclose(loss.detach(), ((own - target)[keep] ** 2).mean(), rtol=1e-5, atol=0)
	grad, = torch.autograd.grad(loss, lat['shapevec'], retain_graph=True)
	assert torch.isfinite(grad).all() and grad.abs().max().item() > 0
	assert MeasurementLoss()(verts, faces, torch.full_like(target, float('nan'))).item() == 0.
	# zero at the mesh's own measurements
	assert MeasurementLoss()(verts, faces, own).item() == 0. and MeasurementLoss(relative=True)(verts, faces, own).item() == 0.
	# another spec: one girth
	spec = measure.FootSpec(girths=(('waist', 0.4),))
	vals, names = measure.foot_measurements(verts.detach(), faces, spec)
	assert names == ('length', 'width', 'waist_girth') and torch.equal(vals[:, :2], own[:, :2])
	assert MeasurementLoss(spec)(verts, faces, vals).item() == 0.


def test_measurement_errors_on_a_ragged_batch():
	"""Scans of two sizes as one Meshes: -1 padded faces, zero padding rows among the vertices, which lie inside both scans' extents and
	must not matter: each scan measures as it does alone."""
	from find_amd import eval_metrics, measure, synthetic
	from find_amd.structures import Meshes
	scans = [synthetic.ellipsoid_mesh(10, 14), synthetic.ellipsoid_mesh(12, 16)]
	scans = [(sv + torch.tensor([0.2, 0.1, 0.]), sf) for sv, sf in scans]   # (away from the origin: a padding row of zeros would be the heel)
	gt = Meshes([sv.cuda() for sv, _ in scans], [sf.cuda() for _, sf in scans])
	v, f = synthetic.template(1002)
	pred = Meshes((v[None] * torch.tensor([[[1.02, 1., 1.]], [[0.97, 1.05, 1.]]])).cuda() + torch.tensor([0.2, 0.1, 0.]).cuda(), f.cuda())
	out, p_mm, g_mm = eval_metrics.measurement_errors_mm(pred, gt, return_per_foot=True)
	assert list(out) == ['Length (mm)', 'Width (mm)', 'Ball girth (mm)', 'Instep girth (mm)'] and p_mm.shape == g_mm.shape == (2, 4)
	for n, (sv, sf) in enumerate(scans):
		alone, _ = measure.foot_measurements(sv[None].cuda(), sf.cuda())
		assert torch.equal(alone[0] * 1e3, g_mm[n]), n
	for j, key in enumerate(out):
		assert torch.equal(out[key], (p_mm[:, j] - g_mm[:, j]).abs().mean()) and out[key].item() > 0
	assert eval_metrics.measurement_errors_mm(pred, pred)['Ball girth (mm)'].item() == 0.


def test_eval_3d_reports_the_measurements(tmp_path):
	"""evaluate.eval_3d(measurements=True) on the four keypointed synthetic scans of tests/test_gpu_points.py: the four keys beside today's
	numbers, the per-foot tables, and exactly today's dict without the keyword."""
	from tests.test_gpu_eval2d import _model
	from tests.test_gpu_points import _foot3d_val_kp
	from find_amd import evaluate
	from find_amd.measure import FootSpec
	ds = _foot3d_val_kp(tmp_path)
	model = _model(len(ds))
	kp_idx = [3, 17, 40, 101]
	torch.manual_seed(31)
	plain = evaluate.eval_3d(model, ds, kp_idx, samples=500)
	torch.manual_seed(31)
	plain2, extra_plain = evaluate.eval_3d(model, ds, kp_idx, samples=500, return_per_foot=True)
	torch.manual_seed(31)
	res, extra = evaluate.eval_3d(model, ds, kp_idx, samples=500, return_per_foot=True, measurements=True)
	new = ['Length (mm)', 'Width (mm)', 'Ball girth (mm)', 'Instep girth (mm)']
	assert list(plain) == ['Keypoint (mm)', 'Chamf z-cutoff 0.07 (μm)', 'Chamf (μm)'] and plain2 == plain and list(extra_plain) == ['keypoint_mm']
	assert list(res) == list(plain) + new and all(res[k] == plain[k] for k in plain)   # no draw was added
	assert all(isinstance(res[k], float) and np.isfinite(res[k]) and res[k] > 0 for k in new)
	assert list(extra) == ['keypoint_mm', 'measure_pred_mm', 'measure_gt_mm'] and torch.equal(extra['keypoint_mm'], extra_plain['keypoint_mm'])
	p_mm, g_mm = extra['measure_pred_mm'], extra['measure_gt_mm']
	assert p_mm.shape == g_mm.shape == (4, 4) and torch.isfinite(p_mm).all() and torch.isfinite(g_mm).all()
	for j, k in enumerate(new):
		assert res[k] == pytest.approx(float((p_mm[:, j] - g_mm[:, j]).abs().mean()), rel=1e-6), k
	# scan k is a sheet of (7 + k)^2 vertices, 1 cm apart: its length and width are 6 + k cm
	side = torch.tensor([60., 70., 80., 90.])
	assert torch.allclose(g_mm[:, 0].cpu(), side, rtol=1e-5, atol=0) and torch.allclose(g_mm[:, 1].cpu(), side, rtol=1e-5, atol=0)
	assert (g_mm[:, 2:] >= g_mm[:, 1:2] * (1 - 1e-5)).all()   # a section of the sheet runs across its whole width, up and down its 2 mm steps
	torch.manual_seed(31)
	spec = evaluate.eval_3d(model, ds, kp_idx, samples=500, measurements=FootSpec(girths=(('waist', 0.4),)))
	assert list(spec) == list(plain) + ['Length (mm)', 'Width (mm)', 'Waist girth (mm)'] and spec['Length (mm)'] == res['Length (mm)']


# ------------------------------------------------------------------ poison
@contextlib.contextmanager
def poisoned_measure(byte):
	"""tests/poison.py's proxy on find_amd.measure: every torch.empty / torch.empty_like of the module comes back filled with `byte`."""
	from find_amd import measure as mod
	if byte not in poison.PATTERNS:
		raise ValueError(byte)
	assert mod.torch is torch
	proxy = poison._TorchProxy(byte)
	try:
		mod.torch = proxy
		yield proxy
	finally:
		mod.torch = torch


def test_no_op_reads_or_leaves_unwritten_memory():
	from test_poison_host import allocating_ops
	from find_amd import measure as mod
	from find_amd import synthetic
	g = torch.Generator().manual_seed(41)
	v, faces = synthetic.ellipsoid_mesh(12, 23)
	verts = v[None] * (0.8 + 0.4 * torch.rand(3, 1, 3, generator=g))
	V = verts.shape[1]
	ragged = torch.stack([torch.cat([_odd_faces(faces[:552 - 7 * n], V), torch.full((7 * n, 3), -1)]) for n in range(3)])
	shared, per_mesh = _planes(verts, 5, False, g), _planes(verts, 5, True, g)
	weight = torch.rand(3, 5, generator=g) + 0.5
	dirs = torch.nn.functional.normalize(torch.randn(3, 3, generator=g), dim=1)
	padded = torch.cat([verts, torch.full((3, 9, 3), float('nan'))], 1)
	v_len = torch.tensor([V, V - 40, 0])
	ran = set()

	def run():
		out = {}
		for tag, f, pl in (('shared', faces, shared), ('per mesh', ragged, per_mesh)):
			for what, t in zip(('perimeter', 'count', 'd_verts', 'd_offset'), _hip(verts, f, pl, weight)):
				out[f'{tag} {what}'] = t.clone()
		ran.add('_PlaneSections')
		vs = padded.cuda().requires_grad_()
		lo, hi, alo, ahi = mod.extents(vs, dirs.cuda(), v_len.cuda(), return_index=True)
		(hi - 0.5 * lo).sum().backward()
		out.update(lo=lo.detach().clone(), hi=hi.detach().clone(), arg_lo=alo.clone(), arg_hi=ahi.clone(), d_extents=vs.grad.clone())
		ran.add('_Extents')
		return out
	runs = []
	for byte in (None, 0xFF, 0x00):
		run()   # (what a forgotten region would hold: the right values of this call)
		with (poisoned_measure(byte) if byte is not None else contextlib.nullcontext()) as proxy:
			runs.append(run())
			assert byte is None or proxy.calls >= 2 * 6 + 4
	assert mod.torch is torch
	rules = dict(arg_lo=poison.Rule(irange=(0, V)), arg_hi=poison.Rule(irange=(0, V)))
	bad = poison.compare('measure', *runs, rules)
	assert not bad, '\n'.join(bad)
	assert torch.isfinite(runs[1]['d_extents']).all() and (runs[1]['d_extents'][2] == 0).all()
	ops = allocating_ops(os.path.join(os.path.dirname(HERE), 'find_amd', 'measure.py'))
	assert ops == ['_PlaneSections', '_Extents'] and set(ops) <= ran


def test_print_the_worst_ratios():
	"""Not a check of its own: the worst e_hip / max(e32, ulp) of the comparisons above, per quantity, for the test log."""
	print('worst e_hip / max(e32, 1 ulp) per quantity:', {k: round(v, 3) for k, v in WORST.items()})
