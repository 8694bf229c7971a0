"""The 2-D part loss on the host: the formulas restated in float64 against what the REFERENCE's RestylePerceptualLoss.forward(mode='cluster')
returned (tests/golden/part_loss.npz, written by make_golden_part_loss.py from src/model/losses.py:251-302), the C interface, and what
the model, ModelWithLoss and the Trainer accept and refuse before any kernel runs."""
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')


@pytest.fixture(scope='module')
def z():
	return np.load(os.path.join(GOLD, 'part_loss.npz'))


def part_labels_f64(gt_logits, size):
	"""argmax_c of F.interpolate(gt_logits (B, C, h, w), size, mode='bilinear') (align_corners=False), in float64; first index on ties."""
	g = np.asarray(gt_logits, np.float64)
	h, w = g.shape[-2:]
	H, W = size

	def axis(n_in, n_out):
		src = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
		i0 = np.minimum(src.astype(np.int64), n_in - 1)
		i1 = i0 + (i0 < n_in - 1)
		l1 = src - i0
		return i0, i1, 1.0 - l1, l1
	y0, y1, ly0, ly1 = axis(h, H)
	x0, x1, lx0, lx1 = axis(w, W)
	top = g[..., y0, :][..., x0] * lx0 + g[..., y0, :][..., x1] * lx1
	bot = g[..., y1, :][..., x0] * lx0 + g[..., y1, :][..., x1] * lx1
	return (top * ly0[:, None] + bot * ly1[:, None]).argmax(1).astype(np.int32)


def part_ce_f64(logits, labels, mask, gl=1.0):
	"""The cluster loss on channel-last logits (..., C), in float64: (loss, ce * mask, d loss / d logits, d loss / d mask)."""
	x = np.asarray(logits, np.float64)
	m = np.asarray(mask, np.float64)
	lab = np.asarray(labels, np.int64)
	zz = x.copy()
	zz[..., 0] = np.where(m == 0, 100.0, 0.0)
	mx = zz.max(-1, keepdims=True)
	e = np.exp(zz - mx)
	s = e.sum(-1, keepdims=True)
	lse = (mx + np.log(s))[..., 0]
	ce = lse - np.take_along_axis(zz, lab[..., None], -1)[..., 0]
	n = m.size
	onehot = np.zeros_like(zz)
	np.put_along_axis(onehot, lab[..., None], 1.0, -1)
	d = gl / n * m[..., None] * (e / s - onehot)
	d[..., 0] = 0.0
	return (ce * m).sum() / n, ce * m, d, gl / n * ce


def test_float64_restatement_matches_the_reference(z):
	for name in z['ce_cases']:
		name = str(name)
		x, m, lab = z[f'ce/{name}/logits'], z[f'ce/{name}/mask'], z[f'ce/{name}/gt_labels']
		loss, ce, d, dm = part_ce_f64(x, lab, m)
		want = float(z[f'ce/{name}/loss'])
		assert abs(loss - want) <= 1e-6 * max(1.0, abs(want)), (name, loss, want)
		for got, key in ((d, 'd_logits'), (dm, 'd_mask'), (ce, 'CE_loss')):
			w = z[f'ce/{name}/{key}']
			assert got.shape == w.shape, (name, key)
			assert np.abs(got - w).max() <= 1e-6 * (max(1.0, np.abs(w).max()) if key == 'CE_loss' else np.abs(w).max()), (name, key, np.abs(got - w).max(), np.abs(w).max())
		assert (z[f'ce/{name}/d_logits'][..., 0] == 0).all(), name
	# what the cases cover
	assert (z['ce/mask_all_zero/mask'] == 0).all() and float(z['ce/mask_all_zero/loss']) == 0.0
	tiny = z['ce/mask_zero_and_tiny/mask']
	assert set(np.unique(tiny).tolist()) == {0.0, float(np.float32(1e-30))}
	inside = z['ce/labels_zero_inside/mask'] > 0
	assert inside.any() and (z['ce/labels_zero_inside/gt_labels'][inside] == 0).all()
	assert np.abs(z['ce/logits_pm120/logits']).min() == 120.0
	assert sorted(z[f'ce/{n}/logits'].shape[-1] for n in ('c1', 'c2', 'c33', 'c64')) == [1, 2, 33, 64]
	assert z['ce/b3_5x7_c21/mask'].size == 105
	assert all((z[f'ce/{n}/mask'] == 0).any() for n in z['ce_cases'])   # every case has background pixels: z_0 = 100 there


def test_float64_labels_match_the_reference(z):
	for name in z['label_cases']:
		name = str(name)
		got = part_labels_f64(z[f'labels/{name}/gt_logits'], tuple(z[f'labels/{name}/size']))
		np.testing.assert_array_equal(got, z[f'labels/{name}/gt_labels'], err_msg=name)
		if not name.startswith('tie_'):
			assert float(z[f'labels/{name}/gap']) >= 1e-4, name
	for name in z['ce_cases']:   # the encoder logits of the loss cases give the labels the loss used
		name = str(name)
		got = part_labels_f64(z[f'ce/{name}/gt_logits'], z[f'ce/{name}/mask'].shape[1:])
		np.testing.assert_array_equal(got, z[f'ce/{name}/gt_labels'], err_msg=name)
	assert (z['labels/tie_all_equal/gt_labels'] == 0).all() and (z['labels/tie_two_maxima/gt_labels'] == 2).all()
	sizes = {(tuple(z[f'labels/{n}/gt_logits'].shape[2:]), tuple(z[f'labels/{n}/size'])) for n in z['label_cases']}
	assert {((12, 12), (24, 24)), ((5, 5), (13, 13)), ((16, 16), (16, 16)), ((24, 24), (12, 12)), ((7, 5), (9, 14))} <= sizes


def test_header_and_bindings_declare_the_symbols():
	from find_amd import _lib
	hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'find_hip.h')).read()
	for name in ('find_part_labels', 'find_part_ce_fwd', 'find_part_ce_bwd'):
		assert re.search(r'\bint ' + name + r'\(', hdr), name
		assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name), name
	assert int(re.search(r'#define FIND_ABI_VERSION (\d+)', hdr).group(1)) == _lib.ABI_VERSION >= 3


def test_ops_have_no_cpu_fallback():
	from find_amd import functional as FN
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.part_labels(torch.zeros(1, 3, 4, 4), (8, 8))
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.part_cross_entropy(torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, dtype=torch.int32), torch.ones(1, 4, 4))


def test_loss_object_refuses_what_is_not_built():
	from find_amd.losses import RestylePerceptualLoss
	called = []
	crit = RestylePerceptualLoss(lambda *a, **k: called.append(1))
	img = torch.zeros(1, 4, 4, 3)
	ok = dict(pred_logit=torch.zeros(1, 4, 4, 3), pred_masks=torch.ones(1, 4, 4), feature_maps=[8])
	for mode in ('feat', 'latent'):
		with pytest.raises(NotImplementedError, match=mode):
			crit(img, img, mode=mode, **ok)
	with pytest.raises(NotImplementedError, match='predicted image'):
		crit(img, img, mode='cluster', **dict(ok, pred_logit=None))
	with pytest.raises(NotImplementedError, match='Clustering loss requires masking'):
		crit(img, img, mode='cluster', **dict(ok, pred_masks=None))
	with pytest.raises(NotImplementedError, match='feat map 8'):
		crit(img, img, mode='cluster', **dict(ok, feature_maps=None))
	assert not called


KW = dict(use_shapevec=True, use_texvec=True, use_posevec=True, train_size=2, val_size=1, shapevec_size=100, texvec_size=100, posevec_size=100)


def _features_file(tmp_path, V, C=21):
	path = str(tmp_path / f'classes_{V}.pth')
	torch.save({'state_dict': {'features': torch.randn(V, C, generator=torch.Generator().manual_seed(V))}}, path)
	return path


def test_neural_model_loads_per_vertex_classes(tmp_path):
	from find_amd import synthetic
	from find_amd.model import NeuralDisplacementField
	from find_amd.opts import Opts
	m = NeuralDisplacementField(**KW, device='cpu', restyle_cluster_per_vertex=True, opts=Opts())
	assert m.per_vertex_features is None and m.params['restyle_cluster_per_vertex'] is True
	with pytest.raises(NotImplementedError, match='fpv'):
		NeuralDisplacementField(**KW, device='cpu', restyle_features_per_vertex=True)
	v, f = synthetic.template(1002)
	opts = Opts(restyle_cluster_per_vertex=True, template_features_pth=_features_file(tmp_path, v.shape[0]))
	m = NeuralDisplacementField(**KW, device='cpu', restyle_cluster_per_vertex=True, opts=opts)
	m.set_template(v, f)
	p = m.per_vertex_features
	assert isinstance(p, torch.nn.Parameter) and p.requires_grad and tuple(p.shape) == (1, v.shape[0], 21)
	assert torch.equal(p.data[0], torch.load(opts.template_features_pth)['state_dict']['features'])
	assert 'per_vertex_features' in m.state_dict()
	for group in (m.main_params, m.templ_params, m.val_params, m.reg_params, m.latent_params):
		assert all(q is not p for q in group)
	m._check_per_vertex_features()
	# a V that is not the template's: refused when the template arrives, and again by get_meshes
	bad = Opts(restyle_cluster_per_vertex=True, template_features_pth=_features_file(tmp_path, 17))
	m = NeuralDisplacementField(**KW, device='cpu', opts=bad)
	with pytest.raises(ValueError, match='17'):
		m.set_template(v, f)
	with pytest.raises(ValueError, match='17'):
		m.get_meshes(shapevec=torch.zeros(1, 100), texvec=torch.zeros(1, 100), posevec=torch.zeros(1, 100))


def test_model_with_loss_needs_the_encoder(tmp_path):
	from find_amd import model_with_loss as M
	from find_amd.opts import Opts
	opts = Opts(sil_loss=True, restyle_perc_cluster_loss=True, restyle_cluster_per_vertex=True, template_features_pth=_features_file(tmp_path, 1))
	with pytest.raises(NotImplementedError, match='restyle_encoder'):
		M.ModelWithLoss(opts=opts, device='cpu', template_mesh_loc=None, **KW)
	mwl = M.ModelWithLoss(opts=opts, device='cpu', template_mesh_loc=None, restyle_encoder=lambda *a, **k: None, **KW)
	assert isinstance(mwl.restyle_perc_loss, M.RestylePerceptualLoss) and mwl.model.per_vertex_features is not None
	# the flag on a model built without the encoder, and without rendered per-vertex classes
	plain = M.ModelWithLoss(opts=Opts(sil_loss=True), device='cpu', template_mesh_loc=None, **KW)
	with pytest.raises(NotImplementedError, match='restyle_encoder'):
		plain({}, 0, Opts(restyle_cluster_per_vertex=True), restyle_perc_cluster=True, render_foot=True)
	with pytest.raises(NotImplementedError, match='restyle_cluster_per_vertex'):
		mwl({}, 0, Opts(), restyle_perc_cluster=True, render_foot=True)
	with pytest.raises(NotImplementedError, match='Clustering loss requires masking'):
		mwl({}, 0, Opts(restyle_cluster_per_vertex=True, restyle_no_masking=True), restyle_perc_cluster=True, render_foot=True)
	# the other perceptual terms are refused as before, encoder or not
	for o in (Opts(vgg_perc_loss=True), Opts(restyle_perc_feat_loss=True), Opts(restyle_perc_lat_loss=True)):
		with pytest.raises(NotImplementedError, match='out of scope'):
			M.ModelWithLoss(opts=o, device='cpu', template_mesh_loc=None, restyle_encoder=lambda *a, **k: None, **KW)
	for flag in ('vgg_perc', 'restyle_perc_feat', 'restyle_perc_lat'):
		with pytest.raises(NotImplementedError, match='out of scope'):
			mwl({}, 0, opts, **{flag: True})


def test_term_registry():
	from find_amd import model_with_loss as M
	assert 'restyle_perc_cluster' not in M.OUT_OF_SCOPE_FLAGS and {'vgg_perc', 'restyle_perc_lat', 'restyle_perc_feat'} <= set(M.OUT_OF_SCOPE_FLAGS)
	t = M.ALL_TERMS[-1]   # last: upstream's insertion order
	assert t == M.Term('restyle_perc_cluster', 'loss_restyle_perc_cluster', 'weight_restyle_perc_cluster', False, True, '_raw_restyle_perc_cluster')
	assert M.ALL_TERMS[:-1] == M.TERMS and hasattr(M.ModelWithLoss, t.fn)


def test_trainer_runs_the_term_eagerly():
	from find_amd import optim
	from find_amd.opts import Opts
	from find_amd.trainer import Trainer, pretty_print_loss
	p = torch.nn.Parameter(torch.zeros(3))
	kw = dict(sil=True, restyle_perc_cluster=True, render_foot=True)
	tr = Trainer([optim.Adam([p], capturable=True)], None, [], [], Opts(), device='cuda:0', graph='auto')
	assert 'restyle_perc_cluster' in tr._why_not_graph(tr.optims, kw)
	assert tr._why_not_graph(tr.optims, dict(sil=True, render_foot=True)) is None
	assert tr._mode(tr.optims, None, kw) is None   # 'auto': eager
	tr.graph = True
	with pytest.raises(RuntimeError, match='restyle_perc_cluster'):
		tr._mode(tr.optims, None, kw)
	assert pretty_print_loss('loss_restyle_perc_cluster') == 'Restyle Perc Cluster'
