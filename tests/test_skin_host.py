"""The skinned foot model (model_type='skinned') on the host: the torch restatement of its definition (tests/skin_ref.py) against a literal
transcription of the published STAR / SUPR form and against central differences -- at pose = 0 too --, SkinnedModel's loader (every layout of
posedirs and J_regressor, .npz / .npy / .pth, cap loops, refusals), its tables and parameter groups, and the C-ABI's declarations.
No GPU needed."""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import skin_ref   # noqa: E402

CASES = [(chain, fj) for chain in ('line', 'star', 'tree') for fj in ('all', 'nonroot')]


def _inputs(J, B, N, seed, scale=1.0):
	g = torch.Generator().manual_seed(seed)
	return (torch.randn(N, 3 * J, generator=g, dtype=torch.float64) * scale, torch.randn(N, B, generator=g, dtype=torch.float64),
			torch.randn(N, 3, generator=g, dtype=torch.float64) * 0.1)


@pytest.mark.parametrize('chain,fj', CASES)
def test_restatement_equals_the_published_form(chain, fj):
	from find_amd import synthetic
	from find_amd.model import _skin_arrays
	V, J, B, N = 57, 6, 4, 3
	data = synthetic.skinned_model(V=V, J=J, B=B + 2, chain=chain, feature_joints=fj, seed=3)   # (two more shape directions than are used)
	consts = _skin_arrays(data, B, dtype=np.float64)
	assert consts['dirs'].shape == (V, B + (4 * J if fj == 'all' else 4 * (J - 1)), 3) and consts['parent'][0] == -1
	pose, betas, trans = _inputs(J, B, N, seed=5)
	pose[1, 3:6] = 0.                                # one joint at rest
	pose[2, 6:9] *= (np.pi - 1e-3) / pose[2, 6:9].norm()
	out, joints = skin_ref.skin(consts, pose, betas, trans, torch.float64, return_joints=True)
	for n in range(N):
		want, wj = skin_ref.published(data, pose[n].numpy(), betas[n].numpy(), trans[n].numpy(), B)
		# float64 on both sides: a few hundred operations of 1e-16 on values of 0.1 .. 1
		assert np.abs(out[n].numpy() - want).max() < 1e-13, (chain, fj, n)
		assert np.abs(joints[n].numpy() - wj).max() < 1e-13, (chain, fj, n)
	# the pose moves the mesh (the case is not the rest pose)
	rest = skin_ref.skin(consts, torch.zeros_like(pose), betas, trans, torch.float64)
	assert (out - rest).abs().max() > 1e-2


def _central(f, x, h):
	g = torch.zeros_like(x)
	flat = x.reshape(-1)
	for i in range(flat.numel()):
		d = torch.zeros_like(flat)
		d[i] = h
		g.reshape(-1)[i] = (f((flat + d).reshape(x.shape)) - f((flat - d).reshape(x.shape))) / (2 * h)
	return g


@pytest.mark.parametrize('scale', [0.0, 1e-6, 1.0])
@pytest.mark.parametrize('chain,fj', [('tree', 'all'), ('line', 'nonroot')])
def test_autograd_equals_central_differences(chain, fj, scale):
	from find_amd import synthetic
	from find_amd.model import _skin_arrays
	V, J, B = 23, 4, 3
	consts = _skin_arrays(synthetic.skinned_model(V=V, J=J, B=B, chain=chain, feature_joints=fj, seed=1), B, dtype=np.float64)
	pose, betas, trans = _inputs(J, B, 1, seed=2, scale=scale)
	d_out = torch.randn(1, V, 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
	_, gp, gb, gt = skin_ref.with_grads(consts, pose, betas, trans, d_out, torch.float64)
	assert torch.isfinite(gp).all() and gp.abs().max() > 1e-3
	loss = lambda p, b, t: float((skin_ref.skin(consts, p, b, t, torch.float64) * d_out).sum())
	h = 1e-5   # central differences of a smooth function: h^2 f''' / 6 ~ 1e-10, rounding 1e-16 / h ~ 1e-11
	for name, got, fd in (('pose', gp, _central(lambda p: loss(p, betas, trans), pose, h)), ('betas', gb, _central(lambda b: loss(pose, b, trans), betas, h)),
						  ('trans', gt, _central(lambda t: loss(pose, betas, t), trans, h))):
		assert (got - fd).abs().max() < 1e-8 * max(1.0, fd.abs().max()), (name, (got - fd).abs().max())


def test_derivatives_at_zero_are_the_generators():
	th = torch.zeros(3, dtype=torch.float64, requires_grad=True)
	dR = torch.autograd.functional.jacobian(skin_ref.rotations, th)   # (3, 3, 3): d R[r, c] / d th_k
	dq = torch.autograd.functional.jacobian(skin_ref.quaternions, th)   # (4, 3)
	for k in range(3):
		e = torch.zeros(3, dtype=torch.float64)
		e[k] = 1
		assert torch.equal(dR[:, :, k], skin_ref.skew(e))
	assert torch.equal(dq[:3], 0.5 * torch.eye(3, dtype=torch.float64)) and torch.equal(dq[3], torch.zeros(3, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ loader
def _state(m):
	return {k: v.clone() for k, v in m.state_dict().items()}


def _same(a, b):
	assert list(a) == list(b)
	for k in a:
		assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_loader_layouts_give_identical_constants():
	import scipy.sparse as sp
	from find_amd import synthetic
	from find_amd.model import SkinnedModel
	V, J, B = 40, 5, 3
	data = synthetic.skinned_model(V=V, J=J, B=B, chain='tree', seed=4)
	base = _state(SkinnedModel.from_arrays(data, device='cpu', num_betas=B, train_size=2, val_size=1))
	assert base['dirs'].shape == (V, B + 4 * J, 3) and base['parent'].tolist() == [-1, 0, 0, 1, 1] and base['parent'].dtype == torch.int32
	# dirs[v, k, c]: shape directions first, then pose directions
	assert base['dirs'][7, 1, 2].item() == data['shapedirs'][7, 2, 1] and base['dirs'][7, B + 5, 0].item() == data['posedirs'][7, 0, 5]
	# the fold, in float64
	J64 = data['J_regressor'].astype(np.float64)
	assert np.array_equal(base['J0'].numpy(), (J64 @ data['v_template'].astype(np.float64)).astype(np.float32))
	assert np.array_equal(base['JS'].numpy(), np.einsum('jv,vcb->jbc', J64, data['shapedirs'].astype(np.float64)).astype(np.float32))
	variants = dict(posedirs_flat=dict(data, posedirs=data['posedirs'].reshape(3 * V, -1)),
					regressor_kron=dict(data, J_regressor=np.kron(data['J_regressor'], np.eye(3, dtype=np.float32))),
					regressor_sparse=dict(data, J_regressor=sp.csc_matrix(data['J_regressor'])),
					regressor_kron_sparse=dict(data, J_regressor=sp.csr_matrix(np.kron(data['J_regressor'], np.eye(3, dtype=np.float32)))),
					signed_root=dict(data, kintree_table=np.stack([np.array([-1, 0, 0, 1, 1]), np.arange(J)])))
	for name, d in variants.items():
		_same(base, _state(SkinnedModel.from_arrays(d, device='cpu', num_betas=B, train_size=2, val_size=1)))


def test_loader_refuses_what_it_does_not_recognise():
	from find_amd import synthetic
	from find_amd.model import SkinnedModel
	V, J, B = 40, 5, 3
	data = synthetic.skinned_model(V=V, J=J, B=B, seed=4)
	load = lambda d, **kw: SkinnedModel.from_arrays(d, device='cpu', num_betas=B, train_size=1, val_size=1, **kw)
	with pytest.raises(ValueError, match=r'`posedirs` has shape \(40, 3, 18\)'):   # rotation-matrix features would be 9 (J - 1) = 36; 18 is nothing
		load(dict(data, posedirs=data['posedirs'][:, :, :18]))
	with pytest.raises(ValueError, match=r'`posedirs` has shape \(40, 3, 36\)'):
		load(dict(data, posedirs=np.zeros((V, 3, 9 * (J - 1)), np.float32)))
	with pytest.raises(ValueError, match='parents must precede'):
		load(dict(data, kintree_table=np.stack([np.array([2 ** 32 - 1, 2, 0, 1, 3], dtype=np.uint32), np.arange(J, dtype=np.uint32)])))
	with pytest.raises(ValueError, match=r'`J_regressor` has shape \(5, 39\)'):
		load(dict(data, J_regressor=data['J_regressor'][:, :-1]))
	with pytest.raises(ValueError, match='not kron'):
		load(dict(data, J_regressor=np.kron(data['J_regressor'], np.ones((3, 3), np.float32))))
	with pytest.raises(ValueError, match=r'`shapedirs` has shape \(40, 3, 3\)'):
		SkinnedModel.from_arrays(data, device='cpu', num_betas=B + 1, train_size=1, val_size=1)
	with pytest.raises(ValueError, match=r'`weights` has shape'):
		load(dict(data, weights=data['weights'][:-1]))
	with pytest.raises(ValueError, match='no `f`'):
		load({k: v for k, v in data.items() if k != 'f'})
	with pytest.raises(ValueError, match='cap loop'):
		load(data, cap_loops=[[0, 1]])


def test_files_round_trip_and_cap_loops(tmp_path):
	from find_amd import synthetic
	from find_amd.model import SkinnedModel
	V, J, B = 1002, 3, 4
	data = synthetic.skinned_model(V=V, J=J, B=B, seed=6)
	loops = [[5, 9, 13, 20, 31], [100, 101, 102]]
	np.savez(str(tmp_path / 'm.npz'), **data)
	np.save(str(tmp_path / 'm.npy'), np.array(data, dtype=object), allow_pickle=True)
	kw = dict(device='cpu', num_betas=B, train_size=3, val_size=2, cap_loops=loops)
	a = SkinnedModel.load(str(tmp_path / 'm.npz'), **kw)
	b = SkinnedModel.load(str(tmp_path / 'm.npy'), **kw)
	_same(_state(a), _state(b))
	F = data['f'].shape[0]
	faces = a.template_faces.data[0]
	assert faces.shape == (F + 3 + 1, 3) and torch.equal(faces[:F], torch.from_numpy(data['f']))
	assert faces[F:].tolist() == [[5, 9, 13], [5, 13, 20], [5, 20, 31], [100, 101, 102]]
	with torch.no_grad():   # a fitted-looking state
		g = torch.Generator().manual_seed(1)
		for t in a.latent_vectors_train + a.latent_vectors_val:
			t.data.copy_(torch.randn(t.data.shape, generator=g))
	a.save_model(str(tmp_path), 'fit')
	c = SkinnedModel.load(str(tmp_path / 'fit.pth'), device='cpu')   # (no model file, no sizes: the checkpoint carries them)
	_same(_state(a), _state(c))
	assert c.params == a.params and [t.name for t in c.latent_vectors_val] == ['pose_val', 'betas_val', 'trans_val', 'reg_val']
	_check_groups(c)
	d = SkinnedModel.load(str(tmp_path / 'fit.pth'), device='cpu', opts=types.SimpleNamespace(dont_load_latents=True), train_size=5, val_size=1)
	assert d.pose_train.data.shape == (5, 3 * J) and torch.all(d.pose_train.data == 0) and torch.equal(d.dirs, a.dirs)
	with pytest.raises(NotImplementedError, match='not understood'):
		SkinnedModel.load(str(tmp_path / 'm.mat'), device='cpu')
	np.save(str(tmp_path / 'bad.npy'), np.zeros(3))
	with pytest.raises(ValueError, match='does not hold a dict'):
		SkinnedModel.load(str(tmp_path / 'bad.npy'), device='cpu')


# ------------------------------------------------------------------------------------------------ model
def _check_groups(m):
	ids = lambda ps: [id(p) for p in ps]
	assert ids(m.main_params) == [id(m.betas_train.data), id(m.pose_train.data)]
	assert ids(m.val_params) == [id(m.betas_val.data), id(m.pose_val.data)]
	assert ids(m.reg_params) == [id(m.reg_train.data), id(m.reg_val.data)]
	assert ids(m.latent_params) == [id(m.betas_train.data), id(m.betas_val.data), id(m.pose_train.data), id(m.pose_val.data)]
	grouped = set(ids(m.main_params + m.val_params + m.reg_params + m.latent_params))
	assert id(m.trans_train.data) not in grouped and id(m.trans_val.data) not in grouped
	torch.optim.Adam(m.main_params, lr=1e-3)


def test_tables_groups_and_template():
	from find_amd import synthetic
	from find_amd.model import SkinnedModel
	V, J, B = 1002, 5, 10
	data = synthetic.skinned_model(V=V, J=J, B=B, seed=2)
	m = SkinnedModel.from_arrays(data, device='cpu', num_betas=B, train_size=4, val_size=2)
	shapes = {t.name: tuple(t.data.shape) for t in m.latent_vectors_train + m.latent_vectors_val}
	assert shapes == dict(pose_train=(4, 3 * J), betas_train=(4, B), trans_train=(4, 3), reg_train=(4, 9), pose_val=(2, 3 * J), betas_val=(2, B),
						  trans_val=(2, 3), reg_val=(2, 9))
	assert [t.name for t in m.latent_vectors_train] == ['pose_train', 'betas_train', 'trans_train', 'reg_train']
	assert torch.all(m.pose_train.data == 0) and torch.all(m.betas_val.data == 0)
	centre = -torch.from_numpy(data['v_template']).mean(0)
	assert torch.equal(m.trans_train.data, centre.expand(4, 3)) and torch.equal(m.trans_val.data, centre.expand(2, 3))
	ident = torch.tensor([0.] * 6 + [1.] * 3)
	assert torch.equal(m.reg_train.data, ident.expand(4, 9)) and torch.equal(m.reg_val.data, ident.expand(2, 9))
	assert m.reg is m.reg_train
	_check_groups(m)
	for k in SkinnedModel.CONSTS + ('template_verts', 'template_faces'):
		assert not getattr(m, k).requires_grad, k
	# template_verts: the rest mesh as the initial tables pose it
	assert m.template_verts.shape == (1, V, 3) and torch.equal(m.template_verts.data[0], torch.from_numpy(data['v_template']) + centre)
	rest = skin_ref.skin(m.state_dict(), m.pose_train.data[:1], m.betas_train.data[:1], m.trans_train.data[:1], torch.float64)
	assert (rest[0] - m.template_verts.data[0].double()).abs().max() < 1e-7
	start = [0.01, 0, 0, -np.pi / 2, 0, -np.pi / 2, 1, 1, 1]
	m2 = SkinnedModel.from_arrays(data, device='cpu', num_betas=B, train_size=1, val_size=1, reg_init=start)
	assert torch.equal(m2.reg_val.data[0], torch.tensor(start, dtype=torch.float32)) and m2.params['reg_init'] == [float(x) for x in start]
	with pytest.raises(NotImplementedError, match='no field to query'):
		m(torch.zeros(1, 4, 3))


def test_model_zoo_and_refusals(tmp_path):
	from find_amd import functional as FN
	from find_amd import synthetic
	from find_amd.model import SkinnedModel
	from find_amd.model_with_loss import ModelWithLoss, model_class_from_opts
	from find_amd.opts import Opts
	data = synthetic.skinned_model(V=1002, J=3, B=10, seed=2)
	np.savez(str(tmp_path / 'm.npz'), **data)
	opts = Opts(model_type='skinned', load_model=str(tmp_path / 'm.npz'))
	assert model_class_from_opts(opts) is SkinnedModel
	for kind in ('supr', 'vertexfeatures'):
		with pytest.raises(NotImplementedError, match='out of scope'):
			model_class_from_opts(types.SimpleNamespace(model_type=kind))
	mwl = ModelWithLoss(opts=opts, device='cpu', train_size=3, val_size=2)
	assert isinstance(mwl.model, SkinnedModel) and mwl.model.pose_train.data.shape == (3, 9)
	_check_groups(mwl.model)
	with pytest.raises(NotImplementedError, match='texture=True'):
		mwl({'idx': torch.tensor([0])}, 0, opts, chamf=True, texture=True)
	m = mwl.model
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.linear_blend_skinning(m, m.pose_train.data, m.betas_train.data, m.trans_train.data)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		m.get_meshes(poses=m.pose_val.data, betas=m.betas_val.data, trans=m.trans_val.data, reg=m.reg_val.data)
	with pytest.raises(RuntimeError, match='bad model shapes'):
		FN.linear_blend_skinning(dict(m.state_dict(), dirs=m.dirs[:, :-1]), m.pose_train.data, m.betas_train.data, m.trans_train.data)


def test_synthetic_models_are_well_formed():
	from find_amd import synthetic
	for V, J, chain, fj in ((1, 1, 'line', 'all'), (3, 2, 'star', 'nonroot'), (65, 24, 'tree', 'all'), (1002, 65, 'line', 'nonroot')):
		d = synthetic.skinned_model(V=V, J=J, B=2, chain=chain, feature_joints=fj, seed=V)
		w, r = d['weights'], d['J_regressor']
		assert w.shape == (V, J) and (w >= 0).all() and np.abs(w.sum(1) - 1).max() < 1e-6 and ((w > 0).sum(1) <= 4).all()
		assert r.shape == (J, V) and ((r != 0).sum(1) <= 8).all() and np.abs(r.sum(1) - 1).max() < 1e-6
		assert d['posedirs'].shape == (V, 3, 4 * J if fj == 'all' else 4 * (J - 1)) and d['kintree_table'].shape == (2, J)
		par = d['kintree_table'][0].astype(np.int64)
		assert par[0] == 2 ** 32 - 1 and all(par[j] < j for j in range(1, J))
		again = synthetic.skinned_model(V=V, J=J, B=2, chain=chain, feature_joints=fj, seed=V)
		assert all(np.array_equal(d[k], again[k]) for k in d)
	with pytest.raises(ValueError):
		synthetic.skinned_model(chain='ring')


def test_c_abi_declares_the_skin_symbols():
	from find_amd import _lib
	hdr = open(os.path.join(ROOT, 'include', 'find_hip.h')).read()
	assert re.search(r'#define FIND_ABI_VERSION 3\b', hdr) and _lib.ABI_VERSION == 3
	names = ('find_skin_fwd_ws_bytes', 'find_skin_fwd', 'find_skin_bwd_ws_bytes', 'find_skin_bwd')
	code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
	for name in names:
		assert re.search(r'\b' + name + r'\s*\(', code), name
		assert name in _lib.PROTOTYPES, name
	L = _lib.lib()   # (raises when the library lacks a symbol the bindings declare)
	assert all(hasattr(L, name) for name in names) and L.find_abi_version() == 3
	# the size rules need no device
	assert L.find_skin_fwd_ws_bytes(2, 100, 5, 3, 20) > 0 and L.find_skin_bwd_ws_bytes(2, 100, 5, 3, 20) > L.find_skin_fwd_ws_bytes(2, 100, 5, 3, 20)
	for bad in ((2, 100, 5, 3, 19), (2, 100, 129, 3, 516), (2, 0, 5, 3, 20), (0, 100, 5, 3, 20), (2, 100, 5, 0, 20), (2, 100, 5, 3000, 20)):
		assert L.find_skin_fwd_ws_bytes(*bad) == -1 and L.find_skin_bwd_ws_bytes(*bad) == -1, bad
