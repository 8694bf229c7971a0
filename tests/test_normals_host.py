"""Surface normals on the host: the formulas of the three ops restated in torch (any dtype; the GPU tests evaluate them in float64 as the
reference and in float32 for the size of an honest rounding error), the C interface, and what the renderer, the registry, the options and
the Trainer accept and refuse before any kernel runs."""
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

SYMBOLS = ('find_vertex_normals_fwd', 'find_vertex_normals_bwd', 'find_normal_map_fwd', 'find_normal_map_bwd', 'find_normal_loss_fwd',
		   'find_normal_loss_bwd')


# ------------------------------------------------------------------ the formulas, in the dtype of their inputs
def vertex_normals_ref(verts, faces):
	"""verts (V, 3), faces (F, 3) int64 (rows with a negative index are padding): n_v = s_v / max(|s_v|, 1e-6), s_v the sum of
	(v1 - v0) x (v2 - v0) over the faces at v."""
	f = faces[(faces >= 0).all(1)].long()
	v0, v1, v2 = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
	fn = torch.cross(v1 - v0, v2 - v0, dim=1)
	s = torch.zeros_like(verts)
	for k in range(3):
		s = s.index_add(0, f[:, k], fn)
	return s / s.norm(dim=1, keepdim=True).clamp(min=1e-6)


def normal_map_ref(raw, R, world=False):
	"""raw (N, M, H, W, 3), R (M, 3, 3): (raw / |raw|) @ R[view], 0 where |raw| <= 1e-6."""
	ln = raw.norm(dim=-1, keepdim=True)
	ok = ln > 1e-6
	n = torch.where(ok, raw / torch.where(ok, ln, torch.ones_like(ln)), torch.zeros_like(raw))
	return n if world else torch.einsum('nmhwj,mjk->nmhwk', n, R)


def normal_loss_ref(p, t, w):
	"""sum w (1 - p^ . t^) / max(sum w, 1e-12), the cosine 0 (no gradient) where |p| <= 1e-6 or |t| <= 1e-6."""
	lp, lt = p.norm(dim=-1), t.norm(dim=-1)
	ok = (lp > 1e-6) & (lt > 1e-6)
	one = torch.ones_like(lp)
	c = torch.where(ok, (p * t).sum(-1) / (torch.where(ok, lp, one) * torch.where(ok, lt, one)), torch.zeros_like(lp))
	return (w * (1 - c)).sum() / w.sum().clamp(min=1e-12)


def octahedron():
	"""Regular octahedron, outward winding: its vertex normals are the six unit axis vectors."""
	v = torch.tensor([[1., 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
	f = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
	return v, f


def test_formulas_on_known_answers():
	v, f = octahedron()
	n = vertex_normals_ref(v.double(), f)
	assert (n - v.double()).abs().max() < 1e-12
	# a padded face row and an untouched vertex change nothing / give zero
	v7 = torch.cat([v, torch.tensor([[3., 3, 3]])]).double()
	n7 = vertex_normals_ref(v7, torch.cat([f, torch.tensor([[-1, -1, -1]])]))
	assert torch.equal(n7[:6], n) and (n7[6] == 0).all()
	# the loss's stated gradient: d p = -w / sum w * (t^ - c p^) / |p|
	g = torch.Generator().manual_seed(0)
	p = torch.randn(5, 3, generator=g, dtype=torch.float64).requires_grad_(True)
	t = torch.randn(5, 3, generator=g, dtype=torch.float64) * 3
	w = torch.rand(5, generator=g, dtype=torch.float64)
	loss = normal_loss_ref(p, t, w)
	loss.backward()
	ph, th = p.detach() / p.detach().norm(dim=1, keepdim=True), t / t.norm(dim=1, keepdim=True)
	c = (ph * th).sum(1, keepdim=True)
	want = -(w / w.sum())[:, None] * (th - c * ph) / p.detach().norm(dim=1, keepdim=True)
	assert (p.grad - want).abs().max() < 1e-12
	assert abs(loss.item() - float((w * (1 - c[:, 0])).sum() / w.sum())) < 1e-12
	assert normal_loss_ref(p.detach(), t, torch.zeros(5, dtype=torch.float64)).item() == 0.0
	# the map: a rotation per view, zero vectors stay zero
	raw = torch.randn(1, 2, 2, 2, 3, generator=g, dtype=torch.float64)
	raw[0, 1, 0, 0] = 0
	R = torch.stack([torch.eye(3, dtype=torch.float64), torch.tensor([[0., 1, 0], [-1, 0, 0], [0, 0, 1]], dtype=torch.float64)])
	m = normal_map_ref(raw, R)
	assert (m[0, 1, 0, 0] == 0).all() and (m[0, 0].norm(dim=-1) - 1).abs().max() < 1e-12
	u = raw[0, 1, 1, 1] / raw[0, 1, 1, 1].norm()
	assert (m[0, 1, 1, 1] - torch.stack([-u[1], u[0], u[2]])).abs().max() < 1e-12
	assert torch.equal(normal_map_ref(raw, R, world=True)[0, 0], m[0, 0])


# ------------------------------------------------------------------ interface
def test_header_and_bindings_declare_the_symbols():
	from find_amd import _lib
	hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'find_hip.h')).read()
	for name in SYMBOLS:
		assert re.search(r'\bint ' + name + r'\(', hdr), name
		assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name), name
	assert re.search(r'\bint64_t find_normal_loss_ws_bytes\(', hdr)
	assert 'find_normal_loss_ws_bytes' in _lib.PROTOTYPES
	L = _lib.lib()
	assert L.find_normal_loss_ws_bytes(1) == 32 and L.find_normal_loss_ws_bytes(1025) == 48 and L.find_normal_loss_ws_bytes(0) == -1
	src = open(os.path.join(os.path.dirname(HERE), 'find_amd', 'csrc', 'normals.hip')).read()
	assert 'atomic' not in src.split('#include', 1)[1]   # a gather and fixed-order sums: nothing to race


def test_ops_have_no_cpu_fallback():
	from find_amd import functional as FN
	from find_amd.losses import NormalLoss
	from find_amd.structures import Meshes
	v, f = octahedron()
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.vertex_normals(v[None], f)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		Meshes(v[None], f).verts_normals_padded()
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.normal_map(torch.zeros(1, 1, 4, 4, 3), torch.eye(3)[None])
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.normal_map(torch.zeros(1, 1, 4, 4, 3), None, space='world')
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.normal_loss(torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4))
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		NormalLoss()(torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4))
	with pytest.raises(ValueError, match='space'):
		FN.normal_map(torch.zeros(1, 1, 4, 4, 3), torch.eye(3)[None], space='camera')


def test_renderer_refuses_normals_in_split_mode():
	import inspect
	from find_amd.renderer import FootRenderer
	from find_amd.structures import Meshes
	names = list(inspect.signature(FootRenderer.forward).parameters)
	assert names[-2:] == ['return_normals', 'normals_space']   # new keywords at the end
	v, f = octahedron()
	m = Meshes(v[None] * 0.05, f)
	R, T = torch.eye(3)[None], torch.tensor([[0., 0, 0.3]])
	rdr = FootRenderer(image_size=16, device='cpu', clip_faces=True)
	with pytest.raises(NotImplementedError, match='clip_faces=True') as e_n:
		rdr(m, R, T, return_images=False, return_normals=True)
	with pytest.raises(NotImplementedError, match='clip_faces=True') as e_f:
		rdr(m, R, T, return_images=False, return_features=True, features=torch.zeros(1, 6, 2))
	assert str(e_n.value) == str(e_f.value)
	with pytest.raises(ValueError, match='normals_space'):
		FootRenderer(image_size=16, device='cpu')(m, R, T, return_images=False, return_normals=True, normals_space='camera')


def test_term_registry_and_options():
	import inspect
	from find_amd import model_with_loss as M
	from find_amd.opts import Opts
	assert len(M.EXTENSION_TERMS) == 1
	t = M.EXTENSION_TERMS[0]
	assert tuple(t)[:5] == ('normal', 'loss_normal', 'weight_normal', False, True) and hasattr(M.ModelWithLoss, t.fn)
	assert [x.flag for x in M.TERMS] == ['chamf', 'smooth', 'texture', 'cont_pose', 'pix', 'sil']
	assert M.ALL_TERMS == M.TERMS + M.ENCODER_TERMS and M.ALL_TERMS[-1].flag == 'restyle_perc_cluster' and t not in M.ALL_TERMS
	names = list(inspect.signature(M.ModelWithLoss.forward).parameters)
	assert names[-2:] == ['cont_pairs', 'normal']
	o = Opts()
	assert o.normal_loss is False and o.weight_normal == 1.0
	assert Opts(normal_loss=True, weight_normal=0.5).weight_normal == 0.5
	kw = o.net_train_kwargs()
	assert len(kw) == 10 and 'normal' not in kw


def test_trainer_runs_the_term_eagerly():
	from find_amd import optim
	from find_amd.opts import Opts
	from find_amd.trainer import Trainer, pretty_print_loss
	p = torch.nn.Parameter(torch.zeros(3))
	kw = dict(sil=True, normal=True, render_foot=True)
	tr = Trainer([optim.Adam([p], capturable=True)], None, [], [], Opts(), device='cuda:0', graph='auto')
	assert 'normal' in tr._why_not_graph(tr.optims, kw)
	assert 'normal' in tr._why_not_graph(tr.optims, dict(normal=True, render_foot=True))
	assert tr._why_not_graph(tr.optims, dict(sil=True, render_foot=True)) is None
	assert tr._mode(tr.optims, None, kw) is None   # 'auto': eager
	tr.graph = True
	with pytest.raises(RuntimeError, match='normal'):
		tr._mode(tr.optims, None, kw)
	assert pretty_print_loss('loss_normal') == 'Normal'
