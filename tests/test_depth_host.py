"""Depth on the host: the two formulas restated in torch (any dtype; the GPU tests evaluate them in float64 as the reference and in float32
for the size of an honest rounding error), the closed form of find_depth_bwd pinned to autograd through the oracle's fragments, the C
interface, and what the registry, the options and the Trainer say before any kernel runs."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import camera_ref, render_ref

HERE = os.path.dirname(os.path.abspath(__file__))

SYMBOLS = ('find_depth_bwd', 'find_depth_loss_fwd', 'find_depth_loss_bwd')


# ------------------------------------------------------------------ the formulas, in the dtype of their inputs
def depth_loss_ref(p, t, w=None, kind='l1', delta=0.005, trunc=0., per_image=False):
	"""sum w rho(p - t) / max(sum w, 1e-12) over the pixels with p > 0, t > 0 and |p - t| <= trunc (trunc <= 0: no limit); p, t, w
	(n_img, n_pix).  per_image: also (n_img, 2) [sum w rho, sum w]."""
	r = p - t
	a = r.abs()
	valid = (p > 0) & (t > 0)
	if trunc > 0:
		valid = valid & (a <= trunc)
	ww = (torch.ones_like(p) if w is None else w) * valid
	if kind == 'l1':
		rho = a
	elif kind == 'l2':
		rho = r * r
	else:
		rho = torch.where(a <= delta, r * r / (2 * delta), a - delta / 2)
	rho = torch.where(valid, rho, torch.zeros_like(rho))
	loss = (ww * rho).sum() / ww.sum().clamp(min=1e-12)
	return (loss, torch.stack([(ww * rho).sum(1), ww.sum(1)], dim=1)) if per_image else loss


def depth_closed_form(verts, faces, R, T, p2f, g, fov_deg=60.0):
	"""find_depth_bwd's formula.  verts (N, V, 3); faces (F, 3) or (N, F, 3); R (M, 3, 3), T (M, 3); p2f (N * M, H, W) packed ids
	image * F + f or -1; g (N * M, H, W).  Returns (z (P,) of the covered pixels in nonzero order, d verts (N, V, 3))."""
	N, V, _ = verts.shape
	M = R.shape[0]
	n_img, H, W = p2f.shape
	F = faces.shape[-2]
	s = 1.0 / math.tan(math.radians(fov_deg) / 2)
	img, yi, xi = torch.nonzero(p2f >= 0, as_tuple=True)
	f = p2f[img, yi, xi] - img * F
	mesh, view = img // M, img % M
	fv = faces.long()[f] if faces.dim() == 2 else faces.long()[mesh, f]          # (P, 3)
	p = torch.einsum('pki,pij->pkj', verts[mesh[:, None], fv], R[view]) + T[view][:, None, :]
	d = torch.stack([(1 - (2 * xi.to(verts.dtype) + 1) / W) / s, (1 - (2 * yi.to(verts.dtype) + 1) / H) / s, torch.ones(len(img), dtype=verts.dtype)], dim=1)
	n = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
	nd = (n * d).sum(1)
	z = (n * p[:, 0]).sum(1) / nd
	X = z[:, None] * d
	dv = torch.zeros_like(verts)
	for k in range(3):
		b = (torch.linalg.cross(p[:, (k + 1) % 3] - X, p[:, (k + 2) % 3] - X, dim=1) * n).sum(1) / (n * n).sum(1)
		dp = (g[img, yi, xi] * b / nd)[:, None] * n
		dv = dv.index_put((mesh, fv[:, k]), torch.einsum('pj,pij->pi', dp, R[view]), accumulate=True)
	return z, dv


def oracle_depth(verts, faces, R, T, p2f, fov_deg=60.0, order=None):
	"""(pz (P,) of the covered pixels, the pixels) by the oracle's fragment functions on the selection p2f (N * M, H, W)."""
	n_img, H, W = p2f.shape
	sel = p2f.long().unsqueeze(-1)
	pix = render_ref.covered_pixels(sel, order)
	vproj = render_ref.torch_project(verts, R, T, fov_deg)
	pz, _, _, _, _ = render_ref.torch_fragments(vproj, faces, sel[pix], R.shape[0], H, W, clip_bary=False, pixels=pix)
	return pz[:, 0], pix


def oracle_depth_grad(verts, faces, R, T, p2f, g, dtype, fov_deg=60.0, order=None):
	"""(pz on the covered pixels, d (sum g * pz) / d verts) by autograd through the oracle, in `dtype` on the CPU."""
	v = verts.detach().cpu().to(dtype).requires_grad_(True)
	pz, pix = oracle_depth(v, faces.cpu(), R.cpu().to(dtype), T.cpu().to(dtype), p2f.cpu(), fov_deg, order)
	(pz * g.cpu().to(dtype)[pix]).sum().backward()
	return pz.detach(), v.grad


def octahedron():
	v = torch.tensor([[1., 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
	f = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
	return v, f


def nearest_faces(verts, faces, R, T, H, W, fov_deg=60.0):
	"""Brute-force K = 1 selection for a small scene: (N * M, H, W) packed ids of the nearest face whose projection holds the pixel centre."""
	vproj = render_ref.torch_project(verts, R, T, fov_deg)
	n_img, F = vproj.shape[0], faces.shape[-2]
	every = (torch.arange(n_img).view(-1, 1, 1, 1) * F + torch.arange(F)).expand(n_img, H, W, F)
	pz, bary, _, _, _ = render_ref.torch_fragments(vproj, faces, every, R.shape[0], H, W, clip_bary=False)
	inside = (bary > 0).all(-1) & (pz > 0)
	z = torch.where(inside, pz, torch.full_like(pz, float('inf')))
	best = z.argmin(-1)
	return torch.where(inside.any(-1), torch.arange(n_img).view(-1, 1, 1) * F + best, torch.full_like(best, -1))


def octahedron_scene(H=16, W=16):
	v, f = octahedron()
	g = torch.Generator().manual_seed(11)
	verts = torch.stack([v * torch.tensor([0.11, 0.05, 0.04]), v * torch.tensor([0.09, 0.06, 0.05]) + 0.004 * torch.randn(6, 3, generator=g)]).double()
	R, T = camera_ref.look_at_view_transform(dist=np.array([0.3, 0.32, 0.28]), elev=np.array([0., 50., -70.]), azim=np.array([0., 30., -60.]), up=((1, 0, 0),))
	R, T = torch.from_numpy(R).double(), torch.from_numpy(T).double()
	p2f = nearest_faces(verts, f, R, T, H, W)
	up = torch.randn(p2f.shape, generator=g, dtype=torch.float64) * 4
	return verts, f, R, T, p2f, up


def test_closed_form_agrees_with_oracle_autograd():
	"""The formula find_depth_bwd evaluates is the derivative of the oracle's pz (K = 1, unclipped barycentrics) -- to rounding in float64."""
	for H, W in ((16, 16), (12, 20)):
		verts, f, R, T, p2f, up = octahedron_scene(H, W)
		covered = int((p2f >= 0).sum())
		assert covered >= 100 and (p2f < 0).any() and all((p2f[i] >= 0).any() for i in range(6))
		pz, want = oracle_depth_grad(verts, f, R, T, p2f, up, torch.float64)
		z, got = depth_closed_form(verts, f, R, T, p2f, up)
		scale = want.abs().max().item()
		assert scale > 1
		assert (z - pz).abs().max().item() < 1e-12 and 0.15 < z.min().item() and z.max().item() < 0.45
		assert (got - want).abs().max().item() <= 1e-12 * scale, ((got - want).abs().max().item(), scale)
		# autograd of z itself says the same
		v = verts.clone().requires_grad_(True)
		z2, _ = depth_closed_form(v, f, R, T, p2f, up)
		(auto,) = torch.autograd.grad((z2 * up[p2f >= 0]).sum(), v)
		assert (auto - want).abs().max().item() <= 1e-12 * scale
		# per-mesh faces with a padding row: the same
		fp = torch.cat([f, torch.full((1, 3), -1)])[None].expand(2, -1, -1)
		p2f_p = torch.where(p2f >= 0, p2f + torch.arange(6).view(-1, 1, 1), p2f)   # image * 9 + f
		_, got_p = depth_closed_form(verts, fp, R, T, p2f_p, up)
		assert torch.equal(got_p, got)


def test_loss_formula_on_known_answers():
	p = torch.tensor([[0.30, 0.31, -1.0, 0.35, 0.300, 0.40]], dtype=torch.float64)
	t = torch.tensor([[0.31, 0.30, 0.30, -1.0, 0.300, 0.30]], dtype=torch.float64)
	w = torch.tensor([[1.0, 2.0, 1.0, 1.0, 1.0, 0.5]], dtype=torch.float64)
	# pixels 2, 3 are background in one map; pixel 5 differs by 0.1
	assert abs(depth_loss_ref(p, t).item() - (0.01 + 0.01 + 0 + 0.1) / 4) < 1e-15
	assert abs(depth_loss_ref(p, t, trunc=0.02).item() - 0.02 / 3) < 1e-15
	assert abs(depth_loss_ref(p, t, w, 'l2').item() - (1e-4 + 2e-4 + 0.5 * 1e-2) / 4.5) < 1e-15
	hub = (1e-4 / 0.04 + 2 * 1e-4 / 0.04 + 0.5 * (0.1 - 0.01)) / 4.5
	assert abs(depth_loss_ref(p, t, w, 'huber', delta=0.02).item() - hub) < 1e-15
	loss, per = depth_loss_ref(p, t, w, per_image=True)
	assert per.shape == (1, 2) and abs(per[0, 1].item() - 4.5) < 1e-15 and abs(loss.item() - (per[0, 0] / per[0, 1]).item()) < 1e-15
	assert depth_loss_ref(-p.abs(), t).item() == 0.0
	# the stated gradient: w rho'(r) / sum w, sign(0) = 0
	x = p.clone().requires_grad_(True)
	depth_loss_ref(x, t, w, 'huber', delta=0.02).backward()
	want = torch.tensor([[-0.5, 2 * 0.5, 0, 0, 0, 0.5]], dtype=torch.float64) / 4.5
	assert (x.grad - want).abs().max().item() < 1e-15
	x = p.clone().requires_grad_(True)
	depth_loss_ref(x, t, w, 'l1').backward()
	assert (x.grad - torch.tensor([[-1, 2, 0, 0, 0, 0.5]], dtype=torch.float64) / 4.5).abs().max().item() < 1e-15


# ------------------------------------------------------------------ interface
def test_header_and_bindings_declare_the_symbols():
	from find_amd import _lib
	hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'find_hip.h')).read()
	for name in SYMBOLS:
		assert re.search(r'\bint ' + name + r'\(', hdr), name
		assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name), name
	assert re.search(r'\bint64_t find_depth_loss_ws_bytes\(', hdr)
	assert 'find_depth_loss_ws_bytes' in _lib.PROTOTYPES
	L = _lib.lib()
	# two doubles of sums and a pair per workgroup of 1024 pixels of one image
	assert L.find_depth_loss_ws_bytes(1, 1) == 32 and L.find_depth_loss_ws_bytes(1, 1025) == 48 and L.find_depth_loss_ws_bytes(3, 1025) == 112
	assert L.find_depth_loss_ws_bytes(0, 16) == -1 and L.find_depth_loss_ws_bytes(1, 0) == -1 and b'bad sizes' in L.find_last_error()
	assert len(_lib.PROTOTYPES['find_depth_bwd'][1]) == 14   # rp, verts, faces, faces_batch, R, T, four sizes, pix_to_face, d_depth, d_verts, stream


def test_ops_have_no_cpu_fallback():
	from find_amd import eval_metrics
	from find_amd import functional as FN
	from find_amd import functional_render as FR
	from find_amd.losses import DepthLoss
	v, f = octahedron()
	R, T = torch.eye(3)[None], torch.tensor([[0., 0, 0.3]])
	z = torch.zeros(1, 1, 4, 4)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.depth_map(v[None] * 0.05, f, R, T, FR.make_params(4), torch.zeros(1, 1, 4, 4, dtype=torch.int32), z)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.depth_loss(torch.ones(2, 16), torch.ones(2, 16))
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		DepthLoss('huber', 0.01, 0.02)(torch.ones(2, 16), torch.ones(2, 16), torch.ones(2, 16))
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		eval_metrics.depth_error_mm(dict(depth=z + 1), dict(depth=z + 1))
	with pytest.raises(ValueError, match='kind'):
		FN.depth_loss(torch.ones(2, 16), torch.ones(2, 16), kind='l3')
	with pytest.raises(ValueError, match='kind'):
		DepthLoss('cauchy')
	with pytest.raises(ValueError, match='delta'):
		FN.depth_loss(torch.ones(2, 16), torch.ones(2, 16), kind='huber', delta=0.)


def test_term_registry_options_and_signatures():
	from find_amd import model_with_loss as M
	from find_amd.evaluate import eval_2d
	from find_amd.opts import Opts
	from find_amd.renderer import FootRenderer
	assert len(M.EXTENSION_TERMS_DEPTH) == 1
	t = M.EXTENSION_TERMS_DEPTH[0]
	assert tuple(t)[:5] == ('depth', 'loss_depth', 'weight_depth', False, True) and hasattr(M.ModelWithLoss, t.fn)
	assert t not in M.ALL_TERMS and t not in M.ALL_EXTENSION_TERMS
	assert M.EVERY_EXTENSION_TERM == M.ALL_EXTENSION_TERMS + M.EXTENSION_TERMS_DEPTH   # walked last
	assert M.EXTENSION_WEIGHTS['weight_depth'] == 100.
	assert M.DEPTH_DEFAULTS == dict(depth_loss_kind='l1', depth_loss_delta=0.005, depth_trunc=0.02)
	names = list(inspect.signature(M.ModelWithLoss.forward).parameters)
	assert names[-3:] == ['depth', 'cont_pairs', 'normal'] and inspect.signature(M.ModelWithLoss.forward).parameters['depth'].default is False
	o = Opts()
	assert o.depth_loss is False and o.weight_depth == 100. and o.depth_loss_kind == 'l1' and o.depth_loss_delta == 0.005 and o.depth_trunc == 0.02
	assert Opts(depth_loss=True, weight_depth=10., depth_loss_kind='huber').depth_loss_kind == 'huber'
	kw = o.net_train_kwargs()
	assert len(kw) == 10 and 'depth' not in kw
	sig = inspect.signature(FootRenderer.forward).parameters
	assert list(sig)[-2:] == ['return_normals', 'normals_space'] and sig['return_depth'].default is False   # return_depth is the switch
	assert inspect.signature(eval_2d).parameters['depth'].default is False


def test_trainer_runs_the_term_eagerly():
	from find_amd import optim
	from find_amd.opts import Opts
	from find_amd.trainer import Trainer, pretty_print_loss
	p = torch.nn.Parameter(torch.zeros(3))
	kw = dict(sil=True, depth=True, render_foot=True)
	tr = Trainer([optim.Adam([p], capturable=True)], None, [], [], Opts(), device='cuda:0', graph='auto')
	assert 'depth' in tr._why_not_graph(tr.optims, kw)
	assert 'depth' in tr._why_not_graph(tr.optims, dict(depth=True, render_foot=True))
	assert tr._why_not_graph(tr.optims, dict(sil=True, render_foot=True)) is None
	assert tr._mode(tr.optims, None, kw) is None   # 'auto': eager
	tr.graph = True
	with pytest.raises(RuntimeError, match='depth'):
		tr._mode(tr.optims, None, kw)
	assert pretty_print_loss('loss_depth') == 'Depth'
