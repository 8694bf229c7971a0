"""Tape girths on the host: the float64 restatement of the rule (tests/girth_ref.py) against closed forms and against the section
perimeter, the C interface, plane_through, and what the wrappers say before any kernel runs."""
import dataclasses
import inspect
import math
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from girth_ref import arched, basis, ring_girth, ring_strip, section_hulls_ref, two_feet   # noqa: E402
from measure_ref import cube, octahedron, plane_sections_ref   # noqa: E402

SYMBOLS = ('find_section_hull_fwd', 'find_section_hull_bwd')


def _planes(*rows):
	return torch.tensor(rows, dtype=torch.float64)


# ------------------------------------------------------------------ the reference
def test_reference_on_the_cube_and_the_octahedron():
	"""The cube's sections are squares whose sides each carry the point of a face diagonal: collinear, no corner."""
	v, f = cube()
	g, nh, cnt = section_hulls_ref(v[None], f, _planes((0, 0, 1, .5), (1, 0, 0, .25)))
	assert g.tolist() == [[4., 4.]] and nh.tolist() == [[4, 4]] and cnt.tolist() == [[8, 8]]
	v, f = octahedron()
	vs = v[None].clone().requires_grad_()
	pl = _planes((0, 0, 1, 0), (0, 0, 1, 1), (0, 0, 1, 2)).requires_grad_()
	g, nh, cnt = section_hulls_ref(vs, f, pl)
	assert abs(g[0, 0].item() - 4 * math.sqrt(2)) < 1e-15 and g[0, 1:].tolist() == [0., 0.]
	assert nh.tolist() == [[4, 1, 0]] and cnt.tolist() == [[4, 4, 0]]
	g[0, 1:].sum().backward()
	assert (vs.grad == 0).all() and (pl.grad == 0).all()


def test_reference_basis():
	for n, k in (((1., 0., 0.), 1), ((0., 0., 1.), 0), ((0.6, 0., 0.8), 1), ((0.5, 0.5, 0.5 ** 0.5), 0), ((-0.8, 0.6, 0.), 2)):
		n = torch.tensor(n, dtype=torch.float64)
		e1, e2 = basis(n)
		assert int(torch.argmin(n.abs())) == k
		assert abs(e1.norm().item() - 1) < 1e-15 and abs(e1 @ n) < 1e-15 and abs(e2 @ n) < 1e-15 and abs(e1 @ e2) < 1e-15
		assert torch.allclose(torch.linalg.cross(e1, e2), n, atol=1e-15)   # counter-clockwise about n


def test_reference_hull_against_the_section():
	"""Convex template: every section is its own hull.  Arched template: the tape spans the arch, shorter by a relative 1e-3 and more at
	both default planes (0.68 and 0.50 of the length)."""
	from find_amd import synthetic
	for nv in (1002, 6890):
		v, f = synthetic.template(nv)
		x = v[:, 0].double()
		d = [float(x.min() + fr * (x.max() - x.min())) for fr in (0.68, 0.50)]
		pl = _planes((1, 0, 0, d[0]), (1, 0, 0, d[1]))
		hull, nh, cnt = section_hulls_ref(v[None].double(), f, pl)
		sec, cnt2 = plane_sections_ref(v[None].double(), f, pl)
		assert torch.equal(cnt, cnt2) and ((hull - sec).abs() <= 1e-12 * sec).all(), (nv, hull, sec)
		va = arched(v)
		assert torch.equal(va[:, 0], v[:, 0])
		hull, nh, cnt = section_hulls_ref(va[None].double(), f, pl)
		sec, cnt2 = plane_sections_ref(va[None].double(), f, pl)
		rel = (sec - hull) / hull
		print(f'arched template({nv}): section over hull - 1 at the ball and instep planes {rel[0].tolist()}, corners {nh[0].tolist()} of {cnt[0].tolist()} points')
		assert torch.equal(cnt, cnt2) and (rel >= 1e-3).all() and (rel < 5e-3).all(), (nv, rel)


def test_reference_on_two_feet_and_the_ring_strip():
	from find_amd import synthetic
	v, f = synthetic.ellipsoid_mesh(5, 8)
	v2, f2 = two_feet(v, f)
	pl = _planes((1, 0, 0, 0.013))
	one, nh1, c1 = section_hulls_ref(v[None].double(), f, pl)
	both, nh2, c2 = section_hulls_ref(v2[None].double(), f2, pl)
	assert c2.item() == 2 * c1.item() and both.item() > one.item() + 2 * 3 * 0.045 * 0.999   # there and back across the gap
	for two_k in (6, 256, 1280):
		v, f = ring_strip(two_k, dtype=torch.float64)
		g, nh, cnt = section_hulls_ref(v[None], f, _planes((0, 0, 1, 0)))
		assert nh.item() == cnt.item() == two_k and abs(g.item() - ring_girth(two_k)) < 1e-13 * two_k, two_k
		v, f = ring_strip(two_k, pulled=True, dtype=torch.float64)
		gp, nh, cnt = section_hulls_ref(v[None], f, _planes((0, 0, 1, 0)))
		assert cnt.item() == two_k and (nh.item() < two_k or two_k == 6) and gp.item() < g.item(), two_k   # (of six points all stay corners)


def test_reference_gradient_is_autograd():
	from find_amd import synthetic
	g = torch.Generator().manual_seed(0)
	v, f = synthetic.ellipsoid_mesh(3, 5, axes=(1.0, 0.7, 0.5))
	v = (v.double() + 0.01 * torch.randn(v.shape, generator=g, dtype=torch.float64))[None].requires_grad_()
	n = torch.nn.functional.normalize(torch.randn(2, 3, generator=g, dtype=torch.float64), dim=1)
	pl = torch.cat([n, torch.tensor([[0.05], [-0.21]], dtype=torch.float64)], 1).requires_grad_()
	fn = lambda vv, pp: section_hulls_ref(vv, f, pp)[0]   # noqa: E731
	assert (fn(v, pl) > 1).all()
	assert torch.autograd.gradcheck(fn, (v, pl), eps=1e-7, atol=1e-6)


# ------------------------------------------------------------------ interface
def test_header_and_bindings_declare_the_symbols():
	from find_amd import _lib
	root = os.path.dirname(HERE)
	hdr = open(os.path.join(root, 'include', 'find_hip.h')).read()
	L = _lib.lib()
	for name in SYMBOLS:
		assert re.search(r'\bint ' + name + r'\(', hdr), name
		assert name in _lib.PROTOTYPES and hasattr(L, name), name
	assert re.search(r'\bint64_t find_section_hull_ws_bytes\(', hdr) and 'find_section_hull_ws_bytes' in _lib.PROTOTYPES
	assert {n: len(_lib.PROTOTYPES[n][1]) for n in SYMBOLS} == dict(zip(SYMBOLS, (20, 18)))
	assert _lib.ABI_VERSION == 3 and L.find_abi_version() == 3 and '#define FIND_ABI_VERSION 3' in hdr
	assert os.path.exists(os.path.join(root, 'find_amd', 'csrc', 'girth.hip'))
	# one statement of the section rule: both files include it
	for src in ('measure.hip', 'girth.hip'):
		text = open(os.path.join(root, 'find_amd', 'csrc', src)).read()
		assert '#include "section.h"' in text and 'bool cut_of(' not in text and 'bool load_face(' not in text, src


def test_ws_bytes_and_refusals():
	from find_amd import _lib
	L = _lib.lib()
	# forward, per (mesh, plane): max_points int32 faces and 2 max_points (x, y) pairs, each array rounded up to 256 bytes; backward: 4 doubles
	assert L.find_section_hull_ws_bytes(1, 256, 1, 256, 0) == 256 * 4 + 256 * 16
	assert L.find_section_hull_ws_bytes(16, 13776, 2, 13776, 0) == 16 * 2 * 13776 * 20
	assert L.find_section_hull_ws_bytes(16, 13776, 2, 1024, 0) == 16 * 2 * 1024 * 20
	assert L.find_section_hull_ws_bytes(3, 80, 5, 80, 1) == 512 and L.find_section_hull_ws_bytes(16, 13776, 64, 13776, 1) == 16 * 64 * 32
	for bad in ((0, 10, 1, 10), (1, 0, 1, 1), (1, 10, 0, 10), (1, 10, 65, 10), (65536, 10, 1, 10), (1, 10, 1, 0), (1, 10, 1, 11)):
		L.find_image_mse_ws_bytes()
		assert L.find_section_hull_ws_bytes(*bad, 0) == -1 and b'bad sizes' in L.find_last_error() and b'find_section_hull_ws_bytes' in L.find_last_error(), bad
	one = torch.zeros(64)
	o = _lib.ptr(one)
	# refused before anything is launched (host pointers are never read)
	fwd = lambda verts=o, faces=o, fb=1, planes=o, pb=1, N=2, V=4, F=3, Pn=2, mp=3, mh=0, girth=o, cnt=o, nh=o, st=o, ids=o, pts=None, ws=o, nb=1 << 20: L.find_section_hull_fwd(   # noqa: E731
		verts, faces, fb, planes, pb, N, V, F, Pn, mp, mh, girth, cnt, nh, st, ids, pts, ws, nb, None)
	for kw in (dict(verts=None), dict(faces=None), dict(planes=None), dict(girth=None), dict(cnt=None), dict(nh=None), dict(st=None), dict(ids=None)):
		assert fwd(**kw) == -1 and b'NULL' in L.find_last_error(), kw
	for kw in (dict(Pn=0), dict(Pn=65), dict(fb=3), dict(fb=0), dict(pb=3), dict(N=0), dict(F=0), dict(V=0), dict(mp=0), dict(mp=4)):
		assert fwd(**kw) == -1 and b'bad sizes' in L.find_last_error(), kw
	for kw in (dict(mh=2), dict(mh=-1), dict(mh=7, pts=o)):
		assert fwd(**kw) == -1 and b'max_hull' in L.find_last_error(), kw
	assert fwd(ws=None) == -2 and fwd(nb=8) == -2 and b'workspace' in L.find_last_error()
	bwd = lambda verts=o, fb=1, pb=1, N=2, Pn=2, mp=3, g=o, nh=o, ids=o, dv=o, ws=o, nb=1 << 20: L.find_section_hull_bwd(   # noqa: E731
		verts, o, fb, o, pb, N, 4, 3, Pn, mp, g, nh, ids, dv, None, ws, nb, None)
	for kw in (dict(verts=None), dict(g=None), dict(nh=None), dict(ids=None), dict(dv=None)):
		assert bwd(**kw) == -1 and b'NULL' in L.find_last_error(), kw
	for kw in (dict(Pn=0), dict(Pn=65), dict(fb=3), dict(pb=5), dict(mp=0)):
		assert bwd(**kw) == -1 and b'bad sizes' in L.find_last_error(), kw
	assert bwd(nb=8) == -2 and b'workspace' in L.find_last_error()


def test_argument_checks_come_before_the_device_check():
	from find_amd import girth, measure
	from find_amd.losses import MeasurementLoss
	v, f = torch.rand(2, 6, 3), torch.tensor([[0, 1, 2], [3, 4, 5]])
	pl = torch.tensor([[1., 0., 0., 0.5]])
	tape = measure.FootSpec(girth_kind='tape')
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		girth.section_hulls(v, f, pl)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		girth.section_hulls(v, f, pl, return_hull=True, max_points=1, max_hull=2)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		measure.foot_measurements(v, f, tape)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		MeasurementLoss(tape)(v, f, torch.zeros(2, 4))
	with pytest.raises(ValueError, match='verts'):
		girth.section_hulls(v[0], f, pl)
	with pytest.raises(ValueError, match='faces'):
		girth.section_hulls(v, f.float(), pl)
	with pytest.raises(ValueError, match='face lists'):
		girth.section_hulls(v, f[None].expand(3, -1, -1), pl)
	with pytest.raises(ValueError, match='planes'):
		girth.section_hulls(v, f, pl[:, :3])
	with pytest.raises(ValueError, match='planes'):
		girth.section_hulls(v, f, pl.expand(65, -1))
	with pytest.raises(ValueError, match='planes'):
		girth.section_hulls(v, f, pl[:0])
	with pytest.raises(ValueError, match='plane lists'):
		girth.section_hulls(v, f, pl[None].expand(3, -1, -1))
	with pytest.raises(ValueError, match='max_points'):
		girth.section_hulls(v, f, pl, max_points=0)
	with pytest.raises(ValueError, match='max_points'):
		girth.section_hulls(v, f, pl, max_points=3)
	with pytest.raises(ValueError, match='max_hull'):
		girth.section_hulls(v, f, pl, return_hull=True, max_hull=0)
	with pytest.raises(ValueError, match='FootSpec'):
		measure.FootSpec(girth_kind='rope')
	with pytest.raises(ValueError, match='FootSpec'):
		measure.FootSpec(girth_kind=None)


def test_defaults_names_and_signatures():
	from find_amd import girth, measure
	spec = measure.FootSpec()
	assert spec.girth_kind == 'section' and spec == measure.FootSpec(girth_kind='section') and hash(spec) == hash(measure.FootSpec(girth_kind='section'))
	assert [fl.name for fl in dataclasses.fields(spec)] == ['length_axis', 'width_axis', 'girths', 'girth_kind']
	tape = measure.FootSpec(girth_kind='tape')
	assert tape != spec and tape.names == spec.names == ('length', 'width', 'ball_girth', 'instep_girth')
	assert (tape.length_axis, tape.width_axis, tape.girths) == (spec.length_axis, spec.width_axis, spec.girths)
	assert inspect.signature(measure.foot_measurements).parameters['spec'].default == spec
	doc = ' '.join(measure.FootSpec.__doc__.split())
	assert "'tape'" in doc and 'section_hulls' in doc and 'plane_through' in doc
	sig = inspect.signature(girth.section_hulls).parameters
	assert list(sig) == ['verts', 'faces', 'planes', 'return_hull', 'max_points', 'max_hull']
	assert (sig['return_hull'].default, sig['max_points'].default, sig['max_hull'].default) == (False, None, 256)
	sig = inspect.signature(girth.plane_through).parameters
	assert list(sig) == ['a', 'b', 'up'] and sig['up'].default == (0., 0., 1.)
	doc = ' '.join(girth.plane_through.__doc__.split())
	assert 'ISO' in doc and "caller's knowledge" in doc and 'metatarsal' in doc


def test_wrappers_live_in_a_module_of_their_own():
	from test_poison_host import allocating_ops
	root = os.path.join(os.path.dirname(HERE), 'find_amd')
	assert allocating_ops(os.path.join(root, 'girth.py')) == ['_SectionHulls']
	assert allocating_ops(os.path.join(root, 'measure.py')) == ['_PlaneSections', '_Extents']
	for mod in ('functional.py', 'functional_render.py', 'vis.py', 'optim.py', 'measure.py'):
		assert 'find_section_hull' not in open(os.path.join(root, mod)).read(), mod


# ------------------------------------------------------------------ plane_through
def test_plane_through_by_hand():
	"""a = (1, 0, 0), b = (1, 2, 0), up = z: (b - a) x up = (2, 0, 0), n = (1, 0, 0), d = 1.  Moving a along x by e tilts the plane:
	b - a = (-e, 2, 0), (b - a) x up = (2, e, 0): dn_y / da_x = 1 / 2 at e = 0, and d = n . a = (2 (1 + e)) / |.| : dd / da_x = 1."""
	from find_amd.girth import plane_through
	a = torch.tensor([1., 0., 0.], dtype=torch.float64, requires_grad=True)
	b = torch.tensor([1., 2., 0.], dtype=torch.float64, requires_grad=True)
	pl = plane_through(a, b)
	assert pl.shape == (4,) and pl.tolist() == [1., 0., 0., 1.]
	jac = torch.stack([torch.autograd.grad(pl[k], (a, b), retain_graph=True)[0] for k in range(4)])   # d plane_k / d a
	want = torch.tensor([[0., 0., 0.], [0.5, 0., 0.], [0., 0., 0.], [1., 0., 0.]], dtype=torch.float64)
	assert torch.allclose(jac, want, atol=1e-15), jac
	jac_b = torch.stack([torch.autograd.grad(pl[k], (a, b), retain_graph=True)[1] for k in range(4)])
	want_b = torch.tensor([[0., 0., 0.], [-0.5, 0., 0.], [0., 0., 0.], [0., 0., 0.]], dtype=torch.float64)
	assert torch.allclose(jac_b, want_b, atol=1e-15), jac_b
	# batched, another up: both points and the direction lie in the plane, the normal is a unit vector
	g = torch.Generator().manual_seed(3)
	a, b = torch.randn(5, 3, generator=g, dtype=torch.float64), torch.randn(5, 3, generator=g, dtype=torch.float64)
	up = torch.tensor([0.1, -0.2, 0.9], dtype=torch.float64)
	pl = plane_through(a, b, up)
	n, d = pl[:, :3], pl[:, 3]
	assert pl.shape == (5, 4) and torch.allclose(n.norm(dim=1), torch.ones(5, dtype=torch.float64), atol=1e-15)
	assert ((n * a).sum(1) - d).abs().max() < 1e-14 and ((n * b).sum(1) - d).abs().max() < 1e-14 and (n @ up).abs().max() < 1e-14
	assert plane_through(a.float(), b.float()).dtype == torch.float32
	assert torch.autograd.gradcheck(lambda x, y: plane_through(x, y, up), (a.clone().requires_grad_(), b.clone().requires_grad_()))
