"""The point-to-surface distance without a GPU: the torch reference the GPU tests compare against (surface_ref.py) on answers known by hand,
its gradient against the closed form the kernel uses, and the host-side plumbing (header, binding, options, signatures)."""
import inspect
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import surface_ref as SR   # noqa: E402

SYMBOLS = ('find_point_face_ws_bytes', 'find_point_face_fwd', 'find_point_face_bwd')


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_seven_regions_known_answers(dtype):
	tri, pts = SR.SEVEN_TRIANGLE.to(dtype), SR.SEVEN_POINTS.to(dtype)
	cp, bary = SR.closest_point(pts, tri[0], tri[1], tri[2])
	assert torch.equal(bary, SR.SEVEN_BARY.to(dtype))
	assert torch.equal(((pts - cp) ** 2).sum(-1), SR.SEVEN_DIST2.to(dtype))
	assert torch.equal(cp, SR.SEVEN_BARY.to(dtype) @ tri)
	# the same through the search, beside a face without area, a -1 row and a second triangle far away
	verts = torch.cat([tri, tri + torch.tensor([0., 0., 5.], dtype=dtype)])
	faces = torch.tensor([[1, 2, 2], [-1, -1, -1], [0, 1, 2], [3, 4, 5]])
	assert SR.usable_faces(verts, faces).tolist() == [False, False, True, True]
	r = SR.point_face(pts, verts, faces, chunk=3)
	assert torch.equal(r['idx'], torch.full((7,), 2)) and torch.equal(r['dist2'], SR.SEVEN_DIST2.to(dtype)) and torch.equal(r['bary'], SR.SEVEN_BARY.to(dtype))
	# equal distances: the smallest face index
	r = SR.point_face(pts, verts, torch.tensor([[0, 1, 2], [0, 1, 2]]))
	assert (r['idx'] == 0).all()
	# no usable face
	r = SR.point_face(pts, verts, faces[:2])
	assert (r['idx'] == -1).all() and (r['dist2'] == 0).all() and (r['bary'] == 0).all()


def test_autograd_gradient_is_the_envelope_formula():
	"""Differentiating through the barycentrics (autograd of the reference) gives what holding them constant gives: the closest point
	minimises the distance over the triangle.  The seven points, one per region, and random ones against a small closed mesh."""
	from find_amd import synthetic
	g = torch.Generator().manual_seed(0)
	cases = [(SR.SEVEN_POINTS.double(), SR.SEVEN_TRIANGLE.double(), torch.tensor([[0, 1, 2]]))]
	v, f = synthetic.ellipsoid_mesh(4, 9)
	cases.append(((v[torch.randint(0, 38, (200,), generator=g)] * (1 + 0.3 * torch.randn(200, 1, generator=g))).double() + 0.004 * torch.randn(200, 3, generator=g, dtype=torch.float64),
				  v.double(), f))
	for pts, verts, faces in cases:
		w = torch.randn(pts.shape[0], generator=g, dtype=torch.float64)
		r = SR.point_face(pts, verts, faces)
		p, x = pts.clone().requires_grad_(True), verts.clone().requires_grad_(True)
		(SR.dist2_to_face(p, x, faces, r['idx']) * w).sum().backward()
		d_points, d_verts = SR.gradients(pts, verts, faces, r['idx'], r['bary'], w)
		scale = max(p.grad.abs().max().item(), x.grad.abs().max().item())
		assert scale > 0.01
		assert (p.grad - d_points).abs().max().item() <= 1e-12 * scale and (x.grad - d_verts).abs().max().item() <= 1e-12 * scale


def test_header_and_binding_declare_the_entry_points():
	from find_amd import _lib
	hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'find_hip.h')).read(), flags=re.S)
	for name in SYMBOLS:
		assert re.search(r'\b' + name + r'\s*\(', hdr), name
		assert name in _lib.PROTOTYPES, name
	assert _lib.ABI_VERSION == 3 and '#define FIND_ABI_VERSION 3' in hdr
	n_args = {name: len(re.search(name + r'\s*\((.*?)\)', hdr, flags=re.S).group(1).split(',')) for name in SYMBOLS}
	assert n_args == {name: len(_lib.PROTOTYPES[name][1]) for name in SYMBOLS}
	L = _lib.lib()
	assert L.find_point_face_ws_bytes(3, 1500) >= 3 * 1500 * 8 and L.find_point_face_ws_bytes(0, 0) > 0 and L.find_point_face_ws_bytes(-1, 4) == -1
	# argument checks come before any launch
	assert L.find_point_face_fwd(None, None, None, None, 1, 2, 8, 4, 4, None, None, None, None, 0, None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_point_face_fwd(None, None, None, None, 1, 2, 0, 4, 4, None, None, None, None, 0, None) == 0   # no points: nothing to do
	assert L.find_point_face_bwd(None, None, None, 1, None, None, None, 2, 8, 4, 4, None, None, None) == -1


def test_options_and_signatures():
	from find_amd import eval_metrics, evaluate, functional, losses, vis
	from find_amd.model_with_loss import ALL_EXTENSION_TERMS, ALL_TERMS, EXTENSION_TERMS, EXTENSION_TERMS_3D, ModelWithLoss
	from find_amd.opts import Opts
	o = Opts()
	assert o.weight_p2s == 1e4 == o.weight_chamf and o.p2s_loss is False
	assert set(o.net_train_kwargs()) == {'chamf', 'smooth', 'texture', 'pix', 'sil', 'vgg_perc', 'restyle_perc_lat', 'restyle_perc_feat', 'restyle_perc_cluster', 'cont_pose'}
	assert inspect.signature(ModelWithLoss.forward).parameters['p2s'].default is False
	term = {t.flag: t for t in EXTENSION_TERMS_3D}['p2s']
	assert ALL_EXTENSION_TERMS == EXTENSION_TERMS + EXTENSION_TERMS_3D and hasattr(ModelWithLoss, term.fn)
	assert (term.key, term.weight, term.needs_3d, term.needs_render) == ('loss_p2s', 'weight_p2s', True, False) and 'p2s' not in {t.flag for t in ALL_TERMS}
	assert inspect.signature(eval_metrics.eval_3d_metrics).parameters['surface'].default is False
	assert inspect.signature(evaluate.eval_3d).parameters['surface'].default is False
	assert list(inspect.signature(functional.point_face_distance).parameters) == ['points', 'verts', 'faces', 'p_len']
	assert list(inspect.signature(losses.point_mesh_distance).parameters) == ['points', 'meshes', 'lengths']
	assert callable(vis.surface_errors) and issubclass(losses.SurfaceDistanceLoss, torch.nn.Module)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		functional.point_face_distance(torch.zeros(1, 4, 3), torch.zeros(1, 3, 3), torch.tensor([[0, 1, 2]]))


def test_eval_3d_metrics_keeps_its_keys_without_surface(monkeypatch):
	"""surface=False must not reach the new code: today's dictionary, key for key.  (The HIP calls are stood in for by torch on the CPU; the
	point-to-surface call raises if it is made.)"""
	from find_amd import eval_metrics
	from find_amd.structures import Meshes

	def chamfer(x, y, xl=None, yl=None):
		return torch.cdist(x, y).min(2).values.pow(2).mean() + torch.cdist(y, x).min(2).values.pow(2).mean(), None

	def forbidden(*a, **k):
		raise AssertionError('point_mesh_distance called without surface=True')
	monkeypatch.setattr(eval_metrics, 'sample_points_from_meshes', lambda meshes, num_samples, draws=None: meshes.verts_padded()[:, :num_samples])
	monkeypatch.setattr(eval_metrics.FN, 'chamfer_distance', chamfer)
	monkeypatch.setattr(eval_metrics, 'point_mesh_distance', forbidden)
	g = torch.Generator().manual_seed(0)
	v = torch.rand(2, 30, 3, generator=g) * 0.1
	f = torch.randint(0, 30, (40, 3), generator=g)
	a, b = Meshes(v, f), Meshes(v + 0.001, f)
	out = eval_metrics.eval_3d_metrics(a, b, samples=20)
	assert list(out) == ['Chamf z-cutoff 0.07 (μm)', 'Chamf (μm)']
	out, samples = eval_metrics.eval_3d_metrics(a, b, pred_verts=v, template_kp_idxs=(1, 2), gt_kps=v[:, [1, 2]] + 0.001, samples=20, return_samples=True)
	assert list(out) == ['Chamf z-cutoff 0.07 (μm)', 'Chamf (μm)', 'Keypoint (mm)'] and len(samples) == 2
	with pytest.raises(AssertionError, match='point_mesh_distance'):
		eval_metrics.eval_3d_metrics(a, b, samples=20, surface=True)
