"""The PCA baseline (model_type='pca') on the host: tests/golden/pca.npz -- the reference's PCAModel.load_from_mat, get_meshes and
ModelWithLoss.forward, run by tests/golden/make_golden_pca.py -- against a float64 restatement of the decode and the registration, the port's
.mat / .pth loading and parameter groups, and the errors of what stays out of scope.  No GPU needed."""
import os
import types

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def z():
	return np.load(os.path.join(GOLD, 'pca.npz'))


def write_mat(z, path):
	from scipy.io import savemat
	savemat(path, {k: z['mat/' + k] for k in ('pcaMean', 'mesh', 'pcaCoefs', 'pcaVar')})
	return path


def euler_xyz64(e):
	"""R = Rx(e0) Ry(e1) Rz(e2), float64, (N, 3, 3)."""
	c, s = np.cos(e), np.sin(e)
	one, zero = np.ones(len(e)), np.zeros(len(e))
	Rx = np.stack([one, zero, zero, zero, c[:, 0], -s[:, 0], zero, s[:, 0], c[:, 0]], 1).reshape(-1, 3, 3)
	Ry = np.stack([c[:, 1], zero, s[:, 1], zero, one, zero, -s[:, 1], zero, c[:, 1]], 1).reshape(-1, 3, 3)
	Rz = np.stack([c[:, 2], -s[:, 2], zero, s[:, 2], c[:, 2], zero, zero, zero, one], 1).reshape(-1, 3, 3)
	return Rx @ Ry @ Rz


def decode64(coefs, template, shapevec, reg=None):
	"""offsets[n,v,c] = sum_b coefs[v,b,c] shapevec[n,b]; X = ((template + offsets) * S) @ R + t (row vectors)."""
	off = np.einsum('vbc,nb->nvc', coefs.astype(np.float64), shapevec.astype(np.float64))
	X = template.astype(np.float64) + off
	if reg is not None:
		reg = reg.astype(np.float64)
		X = (X * reg[:, None, 6:9]) @ euler_xyz64(reg[:, 3:6]) + reg[:, None, 0:3]
	return off, X


def test_float64_decode_and_registration_match_the_reference(z):
	coefs, tv, sv, rg = z['sd/pca_coefs'], z['sd/template_verts'], z['sd/shapevec.data'], z['sd/reg.data']
	for tag, r in (('reg', rg), ('noreg', None)):
		off, X = decode64(coefs, tv, sv, r)
		scale = np.abs(X).max()
		assert np.abs(off - z[f'get_meshes/{tag}/offsets']).max() < 1e-6 * max(np.abs(off).max(), 1e-3), tag
		assert np.abs(X - z[f'get_meshes/{tag}/verts']).max() < 1e-6 * scale, tag
		assert np.all(z[f'get_meshes/{tag}/colours'] == 0.5) and z[f'get_meshes/{tag}/colours'].shape == X.shape
	# the registration really moved the feet (the case is not the identity)
	assert np.abs(z['get_meshes/reg/verts'] - z['get_meshes/noreg/verts']).max() > 1e-3


def test_mat_loading_reproduces_the_reference_tensors(z, tmp_path):
	from find_amd.model import PCAModel
	m = PCAModel.load(write_mat(z, str(tmp_path / 'pca.mat')), device='cpu', train_size=3, val_size=3)
	sd = m.state_dict()
	assert list(sd) == [str(k) for k in z['loaded/keys']]
	for k, v in sd.items():
		want = z['loaded/' + k]
		assert v.dtype == torch.from_numpy(want).dtype and tuple(v.shape) == want.shape, k
		assert np.array_equal(v.numpy(), want), k
	# the (V, B, 3) permutation of pcaCoefs (3V, B), rows 3v + c; faces 1-based in the file
	V, B = sd['template_verts'].shape[1], z['mat/pcaCoefs'].shape[1]
	assert tuple(sd['pca_coefs'].shape) == (V, B, 3)
	v, b, c = V - 2, B - 1, 2
	assert sd['pca_coefs'][v, b, c].item() == np.float32(z['mat/pcaCoefs'][3 * v + c, b])
	assert sd['template_faces'].min().item() == 0 and sd['template_faces'].dtype == torch.int64
	assert [t.name for t in m.latent_vectors_train] == [str(s) for s in z['loaded/latent_train']] == ['reg_train', 'shapevec_train']
	assert [t.name for t in m.latent_vectors_val] == [str(s) for s in z['loaded/latent_val']]
	assert not m.pca_coefs.requires_grad and not m.pca_var.requires_grad and not m.template_verts.requires_grad


def _check_groups(m):
	assert [id(p) for p in m.main_params] == [id(m.shapevec.data)]
	assert [id(p) for p in m.val_params] == [id(m.shapevec_val.data)]
	assert [id(p) for p in m.reg_params] == [id(m.reg.data), id(m.reg_val.data)]
	assert [id(p) for p in m.latent_params] == [id(m.shapevec.data), id(m.shapevec_val.data)]
	torch.optim.Adam(m.main_params, lr=1e-3)   # (upstream raises here after a .pth load: empty parameter list)


def test_param_groups_after_mat_and_pth_loads(z, tmp_path):
	from find_amd.model import PCAModel
	m = PCAModel.load(write_mat(z, str(tmp_path / 'pca.mat')), device='cpu', train_size=3, val_size=3)
	_check_groups(m)
	m.save_model(str(tmp_path), 'pca_fit')
	m2 = PCAModel.load(str(tmp_path / 'pca_fit.pth'), device='cpu')
	_check_groups(m2)
	for k, v in m.state_dict().items():
		assert torch.equal(v, m2.state_dict()[k]), k
	# a checkpoint in the reference's format ({'state_dict', 'params'} as its save_model writes it), with the fixture's fitted tables
	sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
	torch.save({'state_dict': sd, 'params': dict(train_size=3, val_size=3)}, str(tmp_path / 'ref.pth'))
	m3 = PCAModel.load(str(tmp_path / 'ref.pth'), device='cpu')
	_check_groups(m3)
	for k, v in sd.items():
		assert torch.equal(m3.state_dict()[k], v), k
	# dont_load_latents: fresh tables of the requested sizes, B wide
	m4 = PCAModel.load(str(tmp_path / 'ref.pth'), device='cpu', opts=types.SimpleNamespace(dont_load_latents=True), train_size=5, val_size=2)
	_check_groups(m4)
	assert tuple(m4.shapevec.data.shape) == (5, sd['pca_coefs'].shape[1]) and torch.all(m4.shapevec.data == 0)
	assert tuple(m4.reg_val.data.shape) == (2, 9)
	with pytest.raises(NotImplementedError, match='not understood'):
		PCAModel.load(str(tmp_path / 'pca.obj'), device='cpu')


def test_model_with_loss_builds_pca_and_refuses_the_texture_loss(z, tmp_path):
	from find_amd.model import PCAModel
	from find_amd.model_with_loss import ModelWithLoss, model_class_from_opts
	from find_amd.opts import Opts
	opts = Opts(model_type='pca', load_model=write_mat(z, str(tmp_path / 'pca.mat')))
	assert model_class_from_opts(opts) is PCAModel
	mwl = ModelWithLoss(opts=opts, device='cpu', train_size=3, val_size=3)
	assert isinstance(mwl.model, PCAModel)
	_check_groups(mwl.model)
	with pytest.raises(NotImplementedError, match='texture=True'):
		mwl({'idx': torch.tensor([0])}, 0, opts, chamf=True, texture=True)


@pytest.mark.parametrize('kind', ['supr', 'vertexfeatures'])
def test_other_baselines_stay_out_of_scope(kind):
	from find_amd.model_with_loss import model_class_from_opts
	with pytest.raises(NotImplementedError, match='out of scope'):
		model_class_from_opts(types.SimpleNamespace(model_type=kind))


def test_pca_keypoints_are_the_reference_config():
	from find_amd.eval_metrics import PCA_KEYPOINTS
	assert list(PCA_KEYPOINTS) == [1308, 1270, 1271, 1113, 1033, 489]


def test_decode_refuses_cpu_tensors(z):
	from find_amd import functional as FN
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.pca_offsets(torch.from_numpy(z['sd/pca_coefs']), torch.from_numpy(z['sd/shapevec.data']))
