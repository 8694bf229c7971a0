"""Foot measurements on the host: the torch restatement (tests/measure_ref.py) against closed forms, the C interface, and what the wrappers
say before any kernel runs."""
import inspect
import math
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from measure_ref import cube, ellipse_perimeter, extents_ref, foot_measurements_ref, octahedron, plane_sections_ref   # noqa: E402

SYMBOLS = ('find_plane_sections_fwd', 'find_plane_sections_bwd', 'find_extents_fwd', 'find_extents_bwd')
AXES = (0.12, 0.045, 0.04)   # synthetic.ellipsoid_mesh's default


def _plane(normal, d):
	return torch.tensor([list(normal) + [d]], dtype=torch.float64)


# ------------------------------------------------------------------ the reference against closed forms
def test_octahedron_cut_through_its_equator():
	"""Plane z = 0: the four equatorial vertices and edges lie in it.  They count as above, so the four upper faces do not cross and each
	lower face adds its equatorial edge, once."""
	v, f = octahedron()
	per, cnt = plane_sections_ref(v[None], f, _plane((0, 0, 1), 0.))
	assert cnt.tolist() == [[4]] and abs(per.item() - 4 * math.sqrt(2)) < 1e-15


def test_octahedron_tangent_missed_and_below():
	v, f = octahedron()
	vs = v[None].clone().requires_grad_()
	off = torch.tensor([1.0], dtype=torch.float64, requires_grad=True)
	planes = torch.cat([torch.tensor([[0., 0., 1.]], dtype=torch.float64), off[:, None]], 1)
	per, cnt = plane_sections_ref(vs, f, planes)          # z = 1 touches the top vertex: four crossing faces of length 0
	assert cnt.tolist() == [[4]] and per.item() == 0.0
	per.sum().backward()
	assert torch.isfinite(vs.grad).all() and (vs.grad == 0).all() and off.grad.item() == 0.0
	per, cnt = plane_sections_ref(v[None], f, _plane((0, 0, 1), -1.))   # z = -1: the bottom vertex counts as above, like every other
	assert cnt.tolist() == [[0]] and per.item() == 0.0
	per, cnt = plane_sections_ref(v[None], f, _plane((0, 0, 1), 2.))    # misses
	assert cnt.tolist() == [[0]] and per.item() == 0.0


def test_cube_cut_through_a_face():
	"""Plane z = 1 through the top face: its two triangles lie in the plane and contribute nothing; each side wall has one triangle that adds
	its top edge and one that touches the plane in a single vertex (length 0)."""
	v, f = cube()
	per, cnt = plane_sections_ref(v[None], f, _plane((0, 0, 1), 1.))
	assert cnt.tolist() == [[8]] and per.item() == 4.0
	per_faces = [plane_sections_ref(v[None], f[i:i + 1], _plane((0, 0, 1), 1.)) for i in range(12)]
	assert [c.item() for _, c in per_faces[:4]] == [0, 0, 0, 0] and sum(p.item() for p, _ in per_faces[4:]) == 4.0
	per, cnt = plane_sections_ref(v[None], f, _plane((0, 0, 1), 0.5))
	assert cnt.tolist() == [[8]] and per.item() == 4.0
	# -1 rows, an index outside [0, V) and a repeated vertex contribute nothing
	more = torch.cat([f, torch.tensor([[-1, -1, -1], [0, 5, 8], [0, 6, 6]])])
	per, cnt = plane_sections_ref(v[None], more, _plane((0, 0, 1), 0.5))
	assert cnt.tolist() == [[8]] and per.item() == 4.0


def _template_cuts(v, f):
	a, b, c = AXES
	planes = torch.tensor([[1., 0., 0., 0.], [1., 0., 0., 0.3 * a], [0., 0., 1., 0.]], dtype=torch.float64)
	per, cnt = plane_sections_ref(v.double()[None], f, planes)
	k = math.sqrt(1 - 0.09)
	want = torch.tensor([ellipse_perimeter(b, c), ellipse_perimeter(b * k, c * k), ellipse_perimeter(a, b)], dtype=torch.float64)
	return per[0], cnt[0].tolist(), want


def test_template_sections_against_the_ellipse():
	from find_amd import synthetic
	assert abs(ellipse_perimeter(1.0, 1.0) - 2 * math.pi) < 1e-13 and abs(ellipse_perimeter(2.0, 0.0) - 8.0) < 1e-4
	per, cnt, want = _template_cuts(*synthetic.template(6890))
	rel = ((per - want).abs() / want).tolist()
	print('template(6890) x = 0, x = 0.3 a, z = 0: crossing faces', cnt, 'relative difference to the ellipse', [f'{r:.2e}' for r in rel])
	assert cnt == [416, 366, 164]
	assert all(r < 5e-4 for r in rel) and (per < want).all()   # (an inscribed polygon)
	_, cnt, _ = _template_cuts(*synthetic.ellipsoid_mesh(5, 8))
	assert cnt == [26, 24, 16]


def test_extents_reference():
	v = torch.tensor([[[0., 0., 0.], [2., 1., 0.], [2., -1., 0.], [-1., 1., 5.], [-1., 1., 7.]]], dtype=torch.float64)
	lo, hi, alo, ahi = extents_ref(v, [(1., 0., 0.), (0., 1., 0.)])
	assert lo.tolist() == [[-1., -1.]] and hi.tolist() == [[2., 1.]] and alo.tolist() == [[3, 2]] and ahi.tolist() == [[1, 1]]   # ties: the first
	lo, hi, alo, ahi = extents_ref(v, [(1., 0., 0.)], v_len=torch.tensor([3]))
	assert lo.tolist() == [[0.]] and hi.tolist() == [[2.]] and alo.tolist() == [[0]] and ahi.tolist() == [[1]]
	lo, hi, alo, ahi = extents_ref(v, [(1., 0., 0.)], v_len=torch.tensor([0]))
	assert lo.tolist() == [[0.]] and hi.tolist() == [[0.]] and alo.tolist() == [[-1]] and ahi.tolist() == [[-1]]


def test_gradient_of_the_reference_is_autograd():
	from find_amd import synthetic
	g = torch.Generator().manual_seed(0)
	v, f = synthetic.ellipsoid_mesh(3, 5, axes=(1.0, 0.7, 0.5))
	v = (v.double() + 0.01 * torch.randn(v.shape, generator=g, dtype=torch.float64))[None].requires_grad_()
	n = torch.nn.functional.normalize(torch.randn(3, 3, generator=g, dtype=torch.float64), dim=1)
	off = torch.tensor([0.05, -0.21, 0.33], dtype=torch.float64, requires_grad=True)
	fn = lambda vv, oo: plane_sections_ref(vv, f, torch.cat([n, oo[:, None]], 1))[0]   # noqa: E731
	per, cnt = plane_sections_ref(v, f, torch.cat([n, off[:, None]], 1))
	assert (cnt > 2).all() and (per > 1).all()
	assert torch.autograd.gradcheck(fn, (v, off), eps=1e-7, atol=1e-6)
	# a girth moves with the heel: its plane sits at a fraction of the foot's own length
	w = v.detach().clone().requires_grad_()
	m = foot_measurements_ref(w, f)
	m[0, 2].backward()
	heel = int(w.detach()[0, :, 0].argmin())
	assert m.shape == (1, 4) and w.grad[0, heel, 0] != 0


# ------------------------------------------------------------------ interface
def test_header_and_bindings_declare_the_symbols():
	from find_amd import _lib
	hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'find_hip.h')).read()
	for name in SYMBOLS:
		assert re.search(r'\bint ' + name + r'\(', hdr), name
		assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name), name
	assert re.search(r'\bint64_t find_plane_sections_ws_bytes\(', hdr) and 'find_plane_sections_ws_bytes' in _lib.PROTOTYPES
	assert {n: len(_lib.PROTOTYPES[n][1]) for n in SYMBOLS} == dict(zip(SYMBOLS, (14, 17, 11, 10)))
	assert _lib.ABI_VERSION == 3 and _lib.lib().find_abi_version() == 3 and '#define FIND_ABI_VERSION 3' in hdr
	assert 'NORMALS receive no gradient' in hdr
	assert os.path.exists(os.path.join(os.path.dirname(HERE), 'find_amd', 'csrc', 'measure.hip'))


def test_ws_bytes_and_refusals():
	from find_amd import _lib
	L = _lib.lib()
	# forward: a double and an int32 per workgroup of 256 faces and plane, each array rounded up to 256 bytes
	assert L.find_plane_sections_ws_bytes(1, 256, 1, 0) == 512 and L.find_plane_sections_ws_bytes(3, 257, 5, 0) == 512
	assert L.find_plane_sections_ws_bytes(16, 13776, 2, 0) == 16 * 54 * 2 * 12
	# backward: nine floats per face, a double per workgroup and plane
	assert L.find_plane_sections_ws_bytes(1, 256, 1, 1) == 256 * 36 + 256
	assert L.find_plane_sections_ws_bytes(16, 13776, 2, 1) == 16 * 13776 * 36 + 16 * 54 * 2 * 8
	for bad in ((0, 10, 1), (1, 0, 1), (1, 10, 0), (1, 10, 65), (65536, 10, 1)):
		L.find_image_mse_ws_bytes()
		assert L.find_plane_sections_ws_bytes(*bad, 0) == -1 and b'bad sizes' in L.find_last_error() and b'find_plane_sections_ws_bytes' in L.find_last_error(), bad
	one = torch.zeros(64)
	P = _lib.ptr
	o = P(one)
	# refused before anything is launched (host pointers are never read)
	fwd = lambda verts=o, faces=o, fb=1, planes=o, pb=1, N=2, V=4, F=3, Pn=2, per=o, cnt=o, ws=o, nb=1 << 20: L.find_plane_sections_fwd(   # noqa: E731
		verts, faces, fb, planes, pb, N, V, F, Pn, per, cnt, ws, nb, None)
	for kw in (dict(verts=None), dict(faces=None), dict(planes=None), dict(per=None), dict(cnt=None)):
		assert fwd(**kw) == -1 and b'NULL' in L.find_last_error(), kw
	for kw in (dict(Pn=0), dict(Pn=65), dict(fb=3), dict(fb=0), dict(pb=3), dict(N=0), dict(F=0), dict(V=0)):
		assert fwd(**kw) == -1 and b'bad sizes' in L.find_last_error(), kw
	assert fwd(ws=None) == -2 and fwd(nb=8) == -2 and b'workspace' in L.find_last_error()
	bwd = lambda verts=o, fb=1, off=o, items=o, pb=1, N=2, Pn=2, g=o, dv=o, ws=o, nb=1 << 20: L.find_plane_sections_bwd(   # noqa: E731
		verts, o, fb, off, items, o, pb, N, 4, 3, Pn, g, dv, None, ws, nb, None)
	for kw in (dict(verts=None), dict(off=None), dict(items=None), dict(g=None), dict(dv=None)):
		assert bwd(**kw) == -1 and b'NULL' in L.find_last_error(), kw
	for kw in (dict(Pn=0), dict(Pn=65), dict(fb=3), dict(pb=5)):
		assert bwd(**kw) == -1 and b'bad sizes' in L.find_last_error(), kw
	assert bwd(nb=8) == -2 and b'workspace' in L.find_last_error()
	ext = lambda verts=o, dirs=o, N=2, V=4, D=2, lo=o, hi=o, alo=o, ahi=o: L.find_extents_fwd(verts, None, dirs, N, V, D, lo, hi, alo, ahi, None)   # noqa: E731
	for kw in (dict(verts=None), dict(dirs=None), dict(lo=None), dict(hi=None), dict(alo=None), dict(ahi=None)):
		assert ext(**kw) == -1 and b'NULL' in L.find_last_error(), kw
	for kw in (dict(D=0), dict(D=9), dict(N=0), dict(V=0)):
		assert ext(**kw) == -1 and b'bad sizes' in L.find_last_error(), kw
	assert L.find_extents_bwd(o, o, o, o, o, 2, 4, 9, o, None) == -1 and b'bad sizes' in L.find_last_error()
	assert L.find_extents_bwd(o, o, o, o, o, 2, 4, 2, None, None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_extents_bwd(None, None, o, o, o, 2, 4, 2, o, None) == -1 and b'NULL' in L.find_last_error()


def test_argument_checks_come_before_the_device_check():
	from find_amd import eval_metrics, measure
	from find_amd.losses import MeasurementLoss
	v, f = torch.rand(2, 6, 3), torch.tensor([[0, 1, 2], [3, 4, 5]])
	pl = torch.tensor([[1., 0., 0., 0.5]])
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		measure.plane_sections(v, f, pl)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		measure.extents(v, [(1., 0., 0.)])
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		measure.foot_measurements(v, f)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		MeasurementLoss()(v, f, torch.zeros(2, 4))
	with pytest.raises(ValueError, match='verts'):
		measure.plane_sections(v[0], f, pl)
	with pytest.raises(ValueError, match='faces'):
		measure.plane_sections(v, f.float(), pl)
	with pytest.raises(ValueError, match='face lists'):
		measure.plane_sections(v, f[None].expand(3, -1, -1), pl)
	with pytest.raises(ValueError, match='planes'):
		measure.plane_sections(v, f, pl[:, :3])
	with pytest.raises(ValueError, match='planes'):
		measure.plane_sections(v, f, pl.expand(65, -1))
	with pytest.raises(ValueError, match='planes'):
		measure.plane_sections(v, f, pl[:0])
	with pytest.raises(ValueError, match='plane lists'):
		measure.plane_sections(v, f, pl[None].expand(3, -1, -1))
	with pytest.raises(ValueError, match='dirs'):
		measure.extents(v, torch.eye(3).repeat(3, 1))
	with pytest.raises(ValueError, match='v_len'):
		measure.extents(v, torch.eye(3), v_len=torch.tensor([1, 2, 3]))
	with pytest.raises(ValueError, match='FootSpec'):
		measure.foot_measurements(v, f, spec=True)
	with pytest.raises(ValueError, match='FootSpec'):
		measure.FootSpec(length_axis=(0, 0, 0))
	with pytest.raises(ValueError, match='FootSpec'):
		measure.FootSpec(girths=(('ball', 1.5),))
	with pytest.raises(ValueError, match='target'):
		MeasurementLoss()(v, f, torch.zeros(2, 3))
	with pytest.raises(ValueError, match='spec'):
		eval_metrics.eval_3d_metrics(None, None, measurements='yes')


def test_spec_signatures_and_defaults():
	from find_amd import eval_metrics, evaluate, measure
	from find_amd.losses import MeasurementLoss
	spec = measure.FootSpec()
	assert spec.length_axis == (1., 0., 0.) and spec.width_axis == (0., 1., 0.) and spec.girths == (('ball', 0.68), ('instep', 0.50))
	assert spec.names == ('length', 'width', 'ball_girth', 'instep_girth') and spec == measure.FootSpec()
	assert measure.FootSpec(length_axis=(2, 0, 0), girths=[('waist', 0.4)]).names == ('length', 'width', 'waist_girth')
	assert measure.FootSpec(length_axis=(0, 3, 4)).length_axis == (0., 0.6, 0.8)
	doc = ' '.join(measure.FootSpec.__doc__.split())
	assert "this project's convention" in doc and 'convex hull' in doc and 'ISO' in doc and 'at least the tape' in doc
	assert list(inspect.signature(measure.plane_sections).parameters) == ['verts', 'faces', 'planes', 'return_count']
	assert list(inspect.signature(measure.extents).parameters) == ['verts', 'dirs', 'v_len', 'return_index']
	sig = inspect.signature(measure.foot_measurements).parameters
	assert list(sig) == ['verts', 'faces', 'spec', 'v_len'] and sig['spec'].default == spec and sig['v_len'].default is None
	assert list(inspect.signature(measure.of_meshes).parameters) == ['meshes', 'spec']
	assert list(inspect.signature(MeasurementLoss.__init__).parameters) == ['self', 'spec', 'relative']
	assert list(inspect.signature(MeasurementLoss.forward).parameters) == ['self', 'verts', 'faces', 'target', 'v_len']
	loss = MeasurementLoss()
	assert loss.spec == spec and loss.relative is False and 'not in the reference' in MeasurementLoss.__doc__
	assert list(inspect.signature(eval_metrics.measurement_errors_mm).parameters) == ['pred_meshes', 'gt_meshes', 'spec', 'return_per_foot']
	assert eval_metrics.measurement_names(spec) == ('Length (mm)', 'Width (mm)', 'Ball girth (mm)', 'Instep girth (mm)')
	sig = inspect.signature(eval_metrics.eval_3d_metrics).parameters
	assert list(sig)[-1] == 'measurements' and sig['measurements'].default is None
	sig = inspect.signature(evaluate.eval_3d).parameters
	assert list(sig)[-1] == 'measurements' and sig['measurements'].default is False


def test_the_loss_and_the_step_are_left_alone():
	"""The measurement loss is composed by the user: no term in ModelWithLoss.forward, no option in Opts."""
	from find_amd import model_with_loss as M
	from find_amd.opts import Opts
	names = list(inspect.signature(M.ModelWithLoss.forward).parameters)
	assert not any('measure' in n for n in names) and not any('measure' in t.flag for t in M.TERMS + M.EVERY_EXTENSION_TERM)
	assert not any('measure' in k for k in vars(Opts())) and len(Opts().net_train_kwargs()) == 10


def test_wrappers_live_in_a_module_of_their_own():
	"""The poison census of tests/test_poison_host.py walks four modules; the measurement wrappers allocate and belong to none of them."""
	from test_poison_host import allocating_ops
	root = os.path.join(os.path.dirname(HERE), 'find_amd')
	assert allocating_ops(os.path.join(root, 'measure.py')) == ['_PlaneSections', '_Extents']
	for mod in ('functional.py', 'functional_render.py', 'vis.py', 'optim.py'):
		src = open(os.path.join(root, mod)).read()
		assert 'plane_sections' not in src and 'find_extents' not in src, mod
