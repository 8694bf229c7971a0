"""The contrastive pose loss on the host: the pair draw against the reference's own (tests/golden/contrastive.npz, written by
make_golden_contrastive.py from src/model/losses.py:305-333), the arithmetic restated in float64 against the reference's values, and
the checks ModelWithLoss.forward makes before any kernel runs (model.py:1042-1049)."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def z():
	return np.load(os.path.join(GOLD, 'contrastive.npz'))


def contrastive_f64(vecs, codes, pairs, margin=0.5):
	"""ContrastiveLoss.forward over given pairs, in float64: (loss, d loss / d vecs)."""
	v = np.asarray(vecs, np.float64)
	c = np.asarray(codes, np.float64)
	a, b = pairs[:, 0], pairs[:, 1]
	y = (c[a] * c[b]).sum(1)
	diff = v[a] - v[b]
	d2 = (diff ** 2).sum(1)
	h = np.maximum(margin - d2, 0.0)
	P = len(pairs)
	loss = (y * d2 + (1.0 - y) * h ** 2).sum() / P
	coef = (y - 2.0 * (1.0 - y) * h) / P
	grad = np.zeros_like(v)
	np.add.at(grad, a, 2.0 * coef[:, None] * diff)
	np.add.at(grad, b, -2.0 * coef[:, None] * diff)
	return loss, grad


def test_draw_pairs_is_the_reference_draw(z):
	from find_amd.losses import draw_pairs
	for name in z['cases']:
		name = str(name)
		N = z[f'case/{name}/vecs'].shape[0]
		np.random.seed(int(z[f'case/{name}/seed']))
		pairs = draw_pairs(N, int(z[f'case/{name}/npairs']))
		assert pairs.dtype == np.int32 and pairs.shape == z[f'case/{name}/pairs'].shape, name
		np.testing.assert_array_equal(pairs, z[f'case/{name}/pairs'], err_msg=name)
		state = np.random.get_state()
		np.testing.assert_array_equal(state[1], z[f'case/{name}/state_keys'], err_msg=name)
		assert state[2] == int(z[f'case/{name}/state_pos']), name
	# ordered pairs of distinct rows, capped at N(N-1)/2
	np.random.seed(0)
	p = draw_pairs(16, 10_000)
	assert len(p) == 120 and (p[:, 0] != p[:, 1]).all() and len({tuple(r) for r in p.tolist()}) == 120


def test_float64_restatement_matches_the_reference(z):
	for name in z['cases']:
		name = str(name)
		loss, grad = contrastive_f64(z[f'case/{name}/vecs'], z[f'case/{name}/codes'], z[f'case/{name}/pairs'])
		want = float(z[f'case/{name}/loss'])
		assert abs(loss - want) < 1e-5 * max(1.0, abs(want)), (name, loss, want)
		gw = z[f'case/{name}/d_vecs']
		assert np.abs(grad - gw).max() <= 1e-5 * max(1e-6, np.abs(gw).max()), name
	# what the cases cover: both hinge states, y in {-1, 0, 1, 2}, a duplicated row
	assert any(z[f'case/{n}/hinge_active'] for n in z['cases']) and any(z[f'case/{n}/hinge_inactive'] for n in z['cases'])
	ys = set()
	for n in z['cases']:
		c, p = z[f'case/{n}/codes'], z[f'case/{n}/pairs']
		ys |= set((c[p[:, 0]] * c[p[:, 1]]).sum(1).tolist())
	assert {-1.0, 0.0, 1.0, 2.0} <= ys
	v, p = z['case/n3_dup/vecs'], z['case/n3_dup/pairs']
	assert any(np.array_equal(v[a], v[b]) for a, b in p)


def test_upstream_loss_is_float64(z):
	# (the deviation DESIGN 7.1 records: upstream's term is float64 because the pose codes are; the port keeps its fp32 loss path)
	assert str(z['case/n3_k256/loss_dtype']) == 'torch.float64' and str(z['compose/loss_dtype']) == 'torch.float64'


def _cpu_model_with_loss():
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	opts = Opts(chamf_loss=True, smooth_loss=True, use_pose_code=True, cont_pose_loss=True)
	mwl = ModelWithLoss(opts=opts, device='cpu', use_shapevec=True, use_texvec=True, use_posevec=True, train_size=2, val_size=1,
						shapevec_size=100, texvec_size=100, posevec_size=100, template_mesh_loc=None)
	return mwl, opts


@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('is_train', [True, False])
def test_missing_pose_rows_raise_the_reference_error_before_any_kernel(n, is_train):
	mwl, opts = _cpu_model_with_loss()
	batch = dict(idx=torch.arange(n), pose_code=torch.zeros(n, 8, dtype=torch.float64),
				 shapevec_train=torch.zeros(n, 100), texvec_train=torch.zeros(n, 100))
	if not is_train:   # (the train rows do not count for a validation step)
		batch['posevec_train'] = torch.zeros(n, 100)
	state = np.random.get_state()
	with pytest.raises(ValueError, match='Contrastive pose loss used, but no pose found'):
		mwl(batch, 0, opts, chamf=True, smooth=True, cont_pose=True, is_train=is_train)
	assert np.array_equal(np.random.get_state()[1], state[1])   # (nothing drawn)


def test_cont_pose_is_no_longer_out_of_scope():
	from find_amd import model_with_loss as M
	assert 'cont_pose' not in M.OUT_OF_SCOPE_FLAGS
	keys = [t.key for t in M.TERMS]
	assert keys == ['loss_chamf', 'loss_smooth', 'loss_tex', 'loss_cont_pose', 'loss_pix', 'loss_sil']
	t = M.TERMS[keys.index('loss_cont_pose')]
	assert t.flag == 'cont_pose' and t.weight == 'weight_cont_pose' and not t.needs_3d and not t.needs_render


def test_trainer_counts_cont_pose_as_a_term():
	from find_amd import optim
	from find_amd.opts import Opts
	from find_amd.trainer import Trainer
	p = torch.nn.Parameter(torch.zeros(3))
	tr = Trainer([optim.Adam([p], capturable=True)], None, [], [], Opts(), device='cuda:0', graph=True)
	assert tr._why_not_graph(tr.optims, dict(cont_pose=True)) is None
	assert tr._why_not_graph(tr.optims, dict(cont_pose=False)) == 'no loss term enabled'


def test_contrastive_op_has_no_cpu_fallback_and_the_library_exports_it():
	from find_amd import _lib
	from find_amd import functional as FN
	v, c = torch.randn(3, 4), torch.zeros(3, 8)
	pairs = torch.tensor([[0, 1], [2, 0]], dtype=torch.int32)
	with pytest.raises(RuntimeError, match='ROCm device'):
		FN.contrastive_pose(v, c, pairs)
	L = _lib.lib()
	for name in ('find_contrastive_fwd', 'find_contrastive_bwd'):
		assert name in _lib.PROTOTYPES and hasattr(L, name)
