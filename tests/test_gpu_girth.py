"""Tape girths on the MI355X: find_section_hull_* through find_amd.girth against the float64 restatement of the rule (tests/girth_ref.py) on
the same fp32 inputs, and their place in measure.FootSpec, losses.MeasurementLoss and eval_metrics.

Margins: none is a constant of the code under test; the rule of tests/test_gpu_measure.py is taken over unchanged.  Counts of crossing faces
must be equal: every case is drawn so that, in float64, each vertex lies at least 1e-5 of the mesh's extent away from each plane.  The
number of corners is compared, for equality, only where the float64 and the float32 evaluation of the reference agree on it: the generator
redraws a case until they do and asserts it.  Every float comparison also evaluates the reference in float32 on the CPU; with e32 its worst
error against float64 over the case's tensor, the HIP result must lie within max(4 e32, 2 ulp of the largest value) of the float64 one.
Each case prints its figures (DESIGN 7.12 records the worst).

Shapes: a workgroup compacts 256 faces at a time and walks 256 points at a time.  Random triangle soup of F = 1, 255, 256, 257 faces, the
80-face ellipsoid, the arched templates of 2000 and 13 776 faces (sections of up to 420 crossing faces: two rounds of the walk's fold,
one or two rounds of 256 corners in the backward); N = 1 and 3; P = 1, 5 and 64 planes.  Smooth meshes are jittered as in
tests/test_gpu_measure.py: unjittered, a section has hundreds of corners turning by 1e-5 rad, where the two formats legitimately decide
differently and the gradient is conditioned like extent / segment length -- there only the value is compared."""
import contextlib
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import poison   # noqa: E402
from girth_ref import arched, ring_girth, ring_strip, section_hulls_ref, two_feet   # noqa: E402
from measure_ref import cube, octahedron, plane_sections_ref   # noqa: E402

WORST = {}   # name of a quantity -> the worst e_hip / max(e32, ulp) seen (printed by the last test of the file)
D_PLANE = ('d_nx', 'd_ny', 'd_nz', 'd_d')


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


def _jitter(v, N, g):
	return v[None] * (0.8 + 0.4 * torch.rand(N, 1, 3, generator=g)) + 0.002 * v.abs().max() * torch.randn(N, v.shape[0], 3, generator=g)


def _hip(verts, faces, planes, weight, **kw):
	"""(girth, count, n_hull, status, d_verts, d_planes) of the weighted sum of the girths."""
	from find_amd.girth import section_hulls
	vs, ps = verts.detach().cuda().requires_grad_(), planes.detach().cuda().requires_grad_()
	girth, n_hull, count, status, _ = section_hulls(vs, faces.cuda(), ps, return_hull=True, **kw)
	assert girth.dtype == torch.float32 and girth.requires_grad and girth.shape == weight.shape
	for t in (n_hull, count, status):
		assert t.dtype == torch.int32 and not t.requires_grad and t.shape == weight.shape
	(girth * weight.cuda()).sum().backward()
	torch.cuda.synchronize()
	assert vs.grad.shape == verts.shape and ps.grad.shape == planes.shape
	return girth.detach(), count, n_hull, status, vs.grad, ps.grad


def _ref(dtype, verts, faces, planes, weight):
	vs = verts.detach().clone().to(dtype).requires_grad_()
	ps = planes.detach().clone().to(dtype).requires_grad_()
	girth, n_hull, count = section_hulls_ref(vs, faces, ps)
	(girth * weight.to(dtype)).sum().backward()
	return girth.detach(), count, n_hull, vs.grad, ps.grad


def _drawn(name, draw, seed=0):
	"""draw() -> (verts, faces, planes): redrawn until the float64 and the float32 reference agree on every section's number of corners.
	Returns the case, its weight and both references."""
	for attempt in range(8):
		verts, faces, planes = draw()
		weight = torch.rand(verts.shape[0], planes.shape[-2], generator=torch.Generator().manual_seed(seed)) + 0.5
		r64, r32 = _ref(torch.float64, verts, faces, planes, weight), _ref(torch.float32, verts, faces, planes, weight)
		if torch.equal(r64[2], r32[2]):
			break
		print(f'{name}: draw {attempt}: the float32 reference finds other corners than the float64 one in {int((r64[2] != r32[2]).sum())} sections, redrawn')
	assert torch.equal(r64[2], r32[2]) and torch.equal(r64[1], r32[1]), name
	return verts, faces, planes, weight, r64, r32


def _against_float64(name, draw, seed=0, **kw):
	verts, faces, planes, weight, r64, r32 = _drawn(name, draw, seed)
	got = _hip(verts, faces, planes, weight, **kw)
	assert (got[3] == 0).all(), (name, got[3].cpu().tolist())
	assert torch.equal(got[1].cpu().long(), r64[1]), (name, got[1].cpu().tolist(), r64[1].tolist())
	assert torch.equal(got[2].cpu().long(), r64[2]), (name, got[2].cpu().tolist(), r64[2].tolist())
	_held(f'{name} girth', got[0], r64[0], r32[0], kind='girth')
	_held(f'{name} d_verts', got[4], r64[3], r32[3], kind='d_verts')
	for k, what in enumerate(D_PLANE):
		_held(f'{name} {what}', got[5][..., k], r64[4][..., k], r32[4][..., k], kind=what)
	return got, r64, (verts, faces, planes, weight)


# ------------------------------------------------------------------ exact cases
def test_exact_cases():
	"""Small-integer meshes, where every fp32 operation of the rule is exact up to the square root."""
	from find_amd.girth import section_hulls
	from find_amd.measure import plane_sections
	v, f = cube(torch.float32)
	planes = torch.tensor([[0., 0., 1., 0.5], [1., 0., 0., 0.25]])
	girth, n_hull, count, status, pts = section_hulls(v[None].cuda(), f.cuda(), planes.cuda(), return_hull=True)
	assert girth.cpu().tolist() == [[4., 4.]] and n_hull.cpu().tolist() == [[4, 4]] and count.cpu().tolist() == [[8, 8]] and status.cpu().tolist() == [[0, 0]]
	assert pts.shape == (1, 2, 24, 3) and (pts[0, 0, :4, 2] == 0.5).all() and (pts[0, 1, :4, 0] == 0.25).all() and (pts[:, :, 4:] == 0).all()
	assert sorted(map(tuple, pts[0, 0, :4, :2].cpu().tolist())) == [(0., 0.), (0., 1.), (1., 0.), (1., 1.)]   # (the diagonals' points are no corners)
	v, f = octahedron(torch.float32)
	planes = torch.tensor([[0., 0., 1., 0.], [0., 0., 1., 1.], [0., 0., 1., 2.]])
	vs, ps = v[None].cuda().requires_grad_(), planes.cuda().requires_grad_()
	girth, n_hull, count, status, pts = section_hulls(vs, f.cuda(), ps, return_hull=True)
	_, c_sec = plane_sections(v[None].cuda(), f.cuda(), planes.cuda(), return_count=True)
	want = 4 * 2 ** 0.5
	assert abs(girth[0, 0].item() - want) <= 2 * _ulp(want) and n_hull[0, 0].item() == 4
	assert girth[0, 1].item() == 0. and n_hull[0, 1].item() <= 1 and count[0, 1].item() == 4          # z = 1 touches the top vertex
	assert girth[0, 2].item() == 0. and n_hull[0, 2].item() == 0 and count[0, 2].item() == 0 and (pts[0, 2] == 0).all()   # z = 2 misses
	assert (status == 0).all() and torch.equal(count, c_sec)
	girth[0, 1:].sum().backward()
	assert torch.isfinite(vs.grad).all() and (vs.grad == 0).all() and torch.isfinite(ps.grad).all() and (ps.grad == 0).all()
	for p in range(3):   # a plane alone: the same bits as among others
		alone, nh1, c1, _, pts1 = section_hulls(v[None].cuda(), f.cuda(), planes[p:p + 1].cuda(), return_hull=True)
		assert torch.equal(alone[0, 0], girth[0, p].detach()) and nh1.item() == n_hull[0, p].item() and c1.item() == count[0, p].item() and torch.equal(pts1[0, 0], pts[0, p])


# ------------------------------------------------------------------ forward and backward against float64
CASES = [('soup', 1, 1, 5), ('soup', 1, 3, 64), ('soup', 255, 1, 1), ('soup', 255, 3, 5), ('soup', 256, 1, 5), ('soup', 256, 3, 1), ('soup', 257, 1, 64),
		 ('soup', 257, 3, 5), ('ellipsoid', 80, 1, 1), ('ellipsoid', 80, 3, 5), ('ellipsoid', 80, 3, 64), ('arched', 2000, 1, 1), ('arched', 2000, 3, 5),
		 ('arched', 2000, 1, 64), ('arched', 2000, 3, 64), ('arched', 13776, 1, 1), ('arched', 13776, 3, 5), ('arched', 13776, 1, 64), ('two feet', 160, 3, 5)]


@pytest.mark.parametrize('kind,F,N,P', CASES, ids=lambda c: str(c))
def test_hulls_against_float64(kind, F, N, P):
	from find_amd import synthetic
	g = torch.Generator().manual_seed(1000 * F + 10 * N + P)
	if kind == 'soup':
		base, faces = None, _soup(F, 1, g)[1]
	elif kind == 'ellipsoid':
		base, faces = synthetic.ellipsoid_mesh(5, 8)
	elif kind == 'two feet':
		base, faces = two_feet(*synthetic.ellipsoid_mesh(5, 8))
	else:
		base, faces = synthetic.template(1002 if F == 2000 else 6890)
		base = arched(base)
	assert faces.shape[0] == F
	V = max(4, F // 2) if base is None else base.shape[0]
	big = F > 10000   # (the float64 reference walks every section on the host: the large template runs each variant of the case once)

	def verts_of():
		return torch.rand(N, V, 3, generator=g) * 2 - 1 if base is None else _jitter(base, N, g)

	def draw_with(faces_of, per_mesh_planes):
		def draw():
			verts = verts_of()
			return verts, faces_of(verts), _planes(verts, P, per_mesh_planes, g)
		return draw
	plain, odd = (lambda verts: faces), (lambda verts: _odd_faces(faces, V))
	if big:
		runs = [(N > 1, 'shared faces with odd rows', odd)]   # shared planes for the batch, per-mesh ones for the single mesh
	else:
		runs = [(sp, what, fo) for sp in (True, False) for what, fo in (('shared faces', plain), ('shared faces with odd rows', odd)) if fo is plain or (F > 1 and V > 4)]
	for shared_planes, what, faces_of in runs:
		tag = f'{kind} F={F} N={N} P={P} {"shared" if shared_planes else "per-mesh"} planes, {what}'
		(girth, cnt, nh, _, d_v, d_p), _, (verts, _, planes, _) = _against_float64(tag, draw_with(faces_of, not shared_planes))
		assert d_v.shape == verts.shape and d_p.shape == planes.shape
		if P > 1:
			assert (cnt[..., -1] == 0).all() and (girth[..., -1] == 0).all() and (nh[..., -1] == 0).all()   # the plane that misses
	if F > 1 and V > 4 and not big:
		# per-mesh faces: each mesh keeps another part of the list, the rest padded with -1 rows; one odd row each
		def ragged(verts):
			return torch.stack([torch.cat([_odd_faces(faces[:F - 7 * n], V), torch.full((7 * n, 3), -1, dtype=faces.dtype)]) for n in range(N)]).to(torch.int32)
		_against_float64(f'{kind} F={F} N={N} P={P} per-mesh planes, per-mesh faces', draw_with(ragged, True))


# ------------------------------------------------------------------ tape against section
def test_tape_against_section():
	from find_amd import measure, synthetic
	from find_amd.girth import section_hulls
	v, f = synthetic.template(6890)
	x = v[:, 0].double()
	planes = torch.tensor([[1., 0., 0., float(x.min() + fr * (x.max() - x.min()))] for fr in (0.68, 0.50, 0.31)])
	# the convex template, unjittered: a section is its own hull -- both ops within their own allowances of the same float64 number
	sec64, cnt64 = plane_sections_ref(v[None].double(), f, planes.double())
	hull64, _, _ = section_hulls_ref(v[None].double(), f, planes.double())
	assert ((hull64 - sec64).abs() <= 1e-12 * sec64).all()
	sec32, _ = plane_sections_ref(v[None], f, planes)
	hull32, _, _ = section_hulls_ref(v[None], f, planes)
	girth, n_hull, count, status, _ = section_hulls(v[None].cuda(), f.cuda(), planes.cuda(), return_hull=True)
	sec, cnt = measure.plane_sections(v[None].cuda(), f.cuda(), planes.cuda(), return_count=True)
	assert torch.equal(count, cnt) and torch.equal(cnt.cpu().long(), cnt64) and (status == 0).all() and (n_hull > 100).all()
	_held('convex template, tape girth', girth, sec64, hull32, kind='girth')
	_held('convex template, section perimeter', sec, sec64, sec32)
	# the arched template through foot_measurements: the tape spans the arch
	va = arched(v)[None].cuda()
	tape = measure.FootSpec(girth_kind='tape')
	m_sec, names = measure.foot_measurements(va, f.cuda())
	m_tape, names_t = measure.foot_measurements(va, f.cuda(), tape)
	assert names == names_t == ('length', 'width', 'ball_girth', 'instep_girth') and m_tape.shape == m_sec.shape == (1, 4)
	assert torch.equal(m_sec[:, :2], m_tape[:, :2])   # length and width: bit-identical
	rel = ((m_sec[0, 2:] - m_tape[0, 2:]) / m_tape[0, 2:]).cpu().tolist()
	print(f'arched template(6890): section perimeter over tape girth - 1 at the ball and instep planes {rel} (float64: 1.39e-3, 2.41e-3)')
	assert all(r >= 1e-3 for r in rel), rel
	# two feet in one mesh: the tape wraps both
	v1, f1 = synthetic.ellipsoid_mesh(5, 8)
	v2, f2 = two_feet(v1, f1)
	pl = torch.tensor([[1., 0., 0., 0.013]]).cuda()
	both, nh, cnt2, _, _ = section_hulls(v2[None].cuda(), f2.cuda(), pl, return_hull=True)
	one, _, cnt1, _, _ = section_hulls(v1[None].cuda(), f1.cuda(), pl, return_hull=True)
	other = section_hulls(v2[None, v1.shape[0]:].contiguous().cuda(), f1.cuda(), pl)
	assert cnt2.item() == 2 * cnt1.item() and both.item() > one.item() + 0.26 and both.item() > other.item() + 0.26   # (there and back across 3 b = 0.135)


# ------------------------------------------------------------------ ring strip
LDS_POINTS = 2048   # girth.hip: the points (two per crossing face) a workgroup keeps on chip


@pytest.mark.parametrize('two_k', [6, 256, LDS_POINTS // 2 + 256])
def test_ring_strip(two_k):
	"""2K faces, all crossing z = 0, 4K points of which 2K are distinct.  girth.hip keeps LDS_POINTS = 2048 points -- those of 1024 crossing
	faces -- on chip: 2K = 1280 is one workgroup of 256 faces above that, and walks from the workspace.  2K = 6 is less than a wave, 2K = 256
	one round of the compaction."""
	plane = torch.tensor([[0., 0., 1., 0.]])
	ones = torch.ones(1, 1)
	v, f = ring_strip(two_k)
	got = _hip(v[None], f, plane, ones)
	r32 = _ref(torch.float32, v[None], f, plane, ones)
	assert got[1].item() == two_k and got[2].item() == two_k and got[3].item() == 0
	_held(f'ring strip 2K={two_k} girth against the closed form', got[0], torch.tensor([[ring_girth(two_k)]], dtype=torch.float64), r32[0], kind='girth')

	def pulled():
		vp, fp = ring_strip(two_k, pulled=True)
		return vp[None], fp, plane
	(girth, cnt, nh, st, d_v, d_p), r64, _ = _against_float64(f'ring strip 2K={two_k}, every third vertex at radius 0.7', pulled)
	assert cnt.item() == two_k and (two_k == 6 or nh.item() < two_k)
	# fewer points allowed than the section has: refused for that section, nothing NaN
	vp, fp = ring_strip(two_k, pulled=True)
	girth, cnt, nh, st, d_v, d_p = _hip(vp[None], fp, plane, ones, max_points=two_k - 1)
	assert st.item() & 1 and cnt.item() == two_k and nh.item() == 0 and girth.item() == 0.
	assert torch.isfinite(d_v).all() and (d_v == 0).all() and torch.isfinite(d_p).all() and (d_p == 0).all()
	got = _hip(vp[None], fp, plane, ones, max_points=two_k)
	assert got[3].item() == 0 and got[0].item() > 0


# ------------------------------------------------------------------ plane_through
def test_plane_through_moves_with_the_mesh():
	"""The plane through two vertices of the mesh: the gradient reaches the vertices through the section and through the plane, and is
	checked against the float64 reference composed the same way.  The two landmarks lie IN their plane, so s there is rounding noise of
	either sign: which of their faces count as crossing, and how many nearly identical points sit at a landmark, differs between the three
	evaluations and is printed, not compared.  The girth and the composed gradient do not depend on it beyond rounding: s at a landmark is
	0 identically, and what the points at a landmark send to the plane cancels what they send to the vertex."""
	from find_amd import synthetic
	from find_amd.girth import plane_through, section_hulls
	g = torch.Generator().manual_seed(9)
	base, faces = synthetic.template(1002)
	base = arched(base)
	i = int(((base[:, 0] - 0.030) ** 2 + (base[:, 1] - 0.03) ** 2 + 10 * (base[:, 2] > 0)).argmin())   # two vertices of the sole, either side
	j = int(((base[:, 0] - 0.045) ** 2 + (base[:, 1] + 0.03) ** 2 + 10 * (base[:, 2] > 0)).argmin())
	verts = _jitter(base, 2, g)
	out = {}
	for dtype in (torch.float64, torch.float32):
		vs = verts.detach().clone().to(dtype).requires_grad_()
		girth, nh, cnt = section_hulls_ref(vs, faces, plane_through(vs[:, i], vs[:, j])[:, None])
		girth.sum().backward()
		out[dtype] = (girth.detach(), nh, cnt, vs.grad)
	r64, r32 = out[torch.float64], out[torch.float32]
	vs = verts.cuda().requires_grad_()
	pl = plane_through(vs[:, i], vs[:, j])[:, None]
	assert pl.shape == (2, 1, 4)
	girth, nh, cnt, st, _ = section_hulls(vs, faces.cuda(), pl, return_hull=True)
	girth.sum().backward()
	print(f'landmarks {i}, {j}: corners / crossing faces  HIP {nh.cpu().tolist()} / {cnt.cpu().tolist()}  float64 {r64[1].tolist()} / {r64[2].tolist()}  float32 {r32[1].tolist()} / {r32[2].tolist()}')
	assert (st == 0).all() and (girth > 0.1).all() and torch.isfinite(vs.grad).all()
	assert (vs.grad[:, i] != 0).any(dim=1).all() and (vs.grad[:, j] != 0).any(dim=1).all()
	_held('plane_through girth', girth, r64[0], r32[0], kind='girth')
	_held('plane_through d_verts', vs.grad, r64[3], r32[3], kind='d_verts through the plane')
	# without the plane's share the landmarks get another gradient
	vs2 = verts.cuda().requires_grad_()
	section_hulls(vs2, faces.cuda(), pl.detach()).sum().backward()
	assert not torch.equal(vs2.grad[:, i], vs.grad[:, i]) and not torch.equal(vs2.grad[:, j], vs.grad[:, j])


# ------------------------------------------------------------------ determinism
def test_two_runs_agree_bit_for_bit_and_a_row_does_not_depend_on_the_batch():
	from find_amd import synthetic
	from find_amd.girth import section_hulls
	g = torch.Generator().manual_seed(77)
	v, faces = synthetic.ellipsoid_mesh(12, 23)   # 552 faces: three rounds of the compaction
	verts = _jitter(v, 3, g)
	weight = torch.rand(3, 5, generator=g) + 0.5
	for per_mesh in (False, True):
		planes = _planes(verts, 5, per_mesh, g)
		a, b = _hip(verts, faces, planes, weight), _hip(verts, faces, planes, weight)
		assert all(torch.equal(p, q) for p, q in zip(a, b))
		assert (a[0][:, :4] > 0).all() and (a[2][:, :4] >= 3).all() and (a[4] != 0).any() and (a[5][..., :4, :] != 0).any()
		for n in range(3):
			alone = _hip(verts[n:n + 1], faces, planes[n:n + 1] if per_mesh else planes, weight[n:n + 1])
			assert all(torch.equal(alone[k][0], a[k][n]) for k in range(5)), (per_mesh, n)
			if per_mesh:
				assert torch.equal(alone[5][0], a[5][n])
		if not per_mesh:   # shared planes: the meshes' shares, added in mesh order
			shares = [_hip(verts[n:n + 1], faces, planes, weight[n:n + 1])[5].double() for n in range(3)]
			assert torch.allclose(a[5].double(), shares[0] + shares[1] + shares[2], rtol=0, atol=1e-6 * max(float(t.abs().max()) for t in shares))
	with torch.no_grad():   # no gradient asked for: the same values
		assert torch.equal(section_hulls(verts.cuda().requires_grad_(), faces.cuda(), planes.cuda()), a[0])


# ------------------------------------------------------------------ return_hull
def test_return_hull():
	from find_amd import synthetic
	from find_amd.girth import section_hulls
	g = torch.Generator().manual_seed(12)
	base, faces = synthetic.template(1002)
	verts = _jitter(arched(base), 2, g)
	planes = _planes(verts, 5, True, g)
	girth, n_hull, count, status, pts = section_hulls(verts.cuda(), faces.cuda(), planes.cuda(), return_hull=True)
	assert pts.shape == (2, 5, 256, 3) and pts.dtype == torch.float32 and (status == 0).all() and (n_hull[:, :4] > 8).all() and (n_hull < 256).all()
	ref, nh64, _, ref_pts = section_hulls_ref(verts.double(), faces, planes.double(), return_points=True)
	for n in range(2):
		for p in range(5):
			k = n_hull[n, p].item()
			h = pts[n, p, :k].double().cpu()
			assert (pts[n, p, k:] == 0).all(), (n, p)
			if k == 0:
				assert girth[n, p].item() == 0.
				continue
			host = (h - h.roll(-1, 0)).float().double().norm(dim=1).float().double().sum().item()   # (each distance an fp32 number)
			assert abs(host - girth[n, p].item()) <= 2 * _ulp(girth[n, p].item()), (n, p, host, girth[n, p].item())
			# the corners lie in the plane and run counter-clockwise about its normal from the float64 reference's first corner
			nrm = planes[n, p, :3].double()
			assert ((h @ nrm) - planes[n, p, 3].double()).abs().max() < 1e-6
			area2 = (torch.linalg.cross(h, h.roll(-1, 0)).sum(0) @ nrm).item()
			assert area2 > 0, (n, p)
			if k == nh64[n, p].item():
				assert (h - ref_pts[n][p]).abs().max() < 1e-6, (n, p)
	few, nh_few, _, _, pts_few = section_hulls(verts.cuda(), faces.cuda(), planes.cuda(), return_hull=True, max_hull=7)
	assert torch.equal(few, girth) and torch.equal(nh_few, n_hull) and pts_few.shape == (2, 5, 7, 3) and torch.equal(pts_few[:, :4], pts[:, :4, :7])
	assert torch.equal(section_hulls(verts.cuda(), faces.cuda(), planes.cuda()), girth)


# ------------------------------------------------------------------ loss and evaluation
def test_measurement_loss_with_the_tape():
	from find_amd import measure, synthetic
	from find_amd.losses import MeasurementLoss
	n = 3
	tape = measure.FootSpec(girth_kind='tape')
	model = synthetic.make_model(1002, train_size=n, val_size=1)
	lat = {k: t.clone().requires_grad_() for k, t in synthetic.latents(n, seed=2).items()}
	faces = model.template_faces.data[0]
	verts = model.get_meshes(**lat)['verts']
	own, names = measure.foot_measurements(verts.detach(), faces, tape)
	assert own.shape == (n, 4) and (own > 0).all() and names == measure.FootSpec().names
	plain, _ = measure.foot_measurements(verts.detach(), faces)
	assert torch.equal(own[:, :2], plain[:, :2]) and (own[:, 2:] <= plain[:, 2:] * (1 + 1e-6)).all()
	assert MeasurementLoss(tape)(verts, faces, own).item() == 0. and MeasurementLoss(tape, relative=True)(verts, faces, own).item() == 0.
	target = own * torch.tensor([1.05, 0.97, 1.02, 0.99], device='cuda')
	for relative in (False, True):
		loss = MeasurementLoss(tape, relative=relative)(verts, faces, target)
		d = (own - target) / (target if relative else 1.)
		assert loss.dim() == 0 and torch.allclose(loss.detach(), (d * d).mean(), rtol=1e-5, atol=0)
		grad, = torch.autograd.grad(loss, lat['shapevec'], retain_graph=True)
		assert torch.isfinite(grad).all() and grad.abs().max().item() > 0, relative
	only_girths = target.clone()
	only_girths[:, :2] = float('nan')   # (not measured: the gradient then comes through the hulls alone)
	grad, = torch.autograd.grad(MeasurementLoss(tape)(verts, faces, only_girths), lat['shapevec'], retain_graph=True)
	assert torch.isfinite(grad).all() and grad.abs().max().item() > 0


def test_measurement_errors_with_the_tape_on_a_ragged_batch():
	"""The ragged two-scan batch of tests/test_gpu_measure.py: each scan measures as it measures alone."""
	from find_amd import eval_metrics, measure, synthetic
	from find_amd.structures import Meshes
	tape = measure.FootSpec(girth_kind='tape')
	scans = [synthetic.ellipsoid_mesh(10, 14), synthetic.ellipsoid_mesh(12, 16)]
	scans = [(sv + torch.tensor([0.2, 0.1, 0.]), sf) for sv, sf in scans]
	gt = Meshes([sv.cuda() for sv, _ in scans], [sf.cuda() for _, sf in scans])
	v, f = synthetic.template(1002)
	pred = Meshes((v[None] * torch.tensor([[[1.02, 1., 1.]], [[0.97, 1.05, 1.]]])).cuda() + torch.tensor([0.2, 0.1, 0.]).cuda(), f.cuda())
	out, p_mm, g_mm = eval_metrics.measurement_errors_mm(pred, gt, spec=tape, return_per_foot=True)
	assert list(out) == ['Length (mm)', 'Width (mm)', 'Ball girth (mm)', 'Instep girth (mm)'] and p_mm.shape == g_mm.shape == (2, 4)
	for n, (sv, sf) in enumerate(scans):
		alone, _ = measure.foot_measurements(sv[None].cuda(), sf.cuda(), tape)
		assert torch.equal(alone[0] * 1e3, g_mm[n]) and (alone[0, 2:] > 0).all(), n
	for j, key in enumerate(out):
		assert torch.equal(out[key], (p_mm[:, j] - g_mm[:, j]).abs().mean()) and out[key].item() > 0
	assert eval_metrics.measurement_errors_mm(pred, pred, spec=tape)['Ball girth (mm)'].item() == 0.


# ------------------------------------------------------------------ poison
@contextlib.contextmanager
def poisoned_girth(byte):
	"""tests/poison.py's proxy on find_amd.girth: every torch.empty / torch.empty_like of the module comes back filled with `byte`."""
	from find_amd import girth as mod
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
	from find_amd import girth as mod
	from find_amd import synthetic
	g = torch.Generator().manual_seed(41)
	v, faces = synthetic.ellipsoid_mesh(12, 23)
	verts = _jitter(v, 3, g)
	V = verts.shape[1]
	ragged = torch.stack([torch.cat([_odd_faces(faces[:552 - 7 * n], V), torch.full((7 * n, 3), -1)]) for n in range(3)])
	shared, per_mesh = _planes(verts, 5, False, g), _planes(verts, 5, True, g)
	weight = torch.rand(3, 5, generator=g) + 0.5
	ring_v, ring_f = ring_strip(LDS_POINTS // 2 + 256, pulled=True)   # (walks from the workspace)
	ran = set()

	def run():
		out = {}
		for tag, vv, f, pl, w, kw in (('shared', verts, faces, shared, weight, {}), ('per mesh', verts, ragged, per_mesh, weight, {}),
									  ('ring', ring_v[None], ring_f, torch.tensor([[0., 0., 1., 0.]]), torch.ones(1, 1), {}),
									  ('refused', verts, faces, shared, weight, dict(max_points=8))):
			vs, ps = vv.cuda().requires_grad_(), pl.cuda().requires_grad_()
			girth, n_hull, count, status, pts = mod.section_hulls(vs, f.cuda(), ps, return_hull=True, max_hull=40, **kw)
			(girth * w.cuda()).sum().backward()
			for what, t in zip(('girth', 'n_hull', 'count', 'status', 'hull_points', 'd_verts', 'd_planes'), (girth.detach(), n_hull, count, status, pts, vs.grad, ps.grad)):
				out[f'{tag} {what}'] = t.clone()
		ran.add('_SectionHulls')
		return out
	runs = []
	for byte in (None, 0xFF, 0x00):
		run()   # (what a forgotten region would hold: the right values of this call)
		with (poisoned_girth(byte) if byte is not None else contextlib.nullcontext()) as proxy:
			runs.append(run())
			assert byte is None or proxy.calls >= 4 * (7 + 3)
	assert mod.torch is torch
	bad = poison.compare('girth', *runs)
	assert not bad, '\n'.join(bad)
	clean = runs[0]
	assert (clean['refused status'][:, :4] == 1).all() and (clean['refused girth'] == 0).all() and (clean['refused d_verts'] == 0).all()
	assert (clean['shared status'] == 0).all() and (clean['ring status'] == 0).all() and (clean['shared girth'][:, :4] > 0).all()
	ops = allocating_ops(os.path.join(os.path.dirname(HERE), 'find_amd', 'girth.py'))
	assert ops == ['_SectionHulls'] and set(ops) <= ran


def test_print_the_worst_ratios():
	"""Not a check of its own: the worst e_hip / max(e32, ulp) of the comparisons above, per quantity, for the test log."""
	print('worst e_hip / max(e32, 1 ulp) per quantity:', {k: round(v, 3) for k, v in WORST.items()})
	assert math.isfinite(sum(WORST.values()))
