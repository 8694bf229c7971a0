"""The 2-D part loss on the MI355X (find_part_labels, find_part_ce_fwd / _bwd) against what the REFERENCE's
RestylePerceptualLoss.forward(mode='cluster') returned (tests/golden/part_loss.npz, make_golden_part_loss.py ran src/model/losses.py:251-302
for real), against the float64 restatement at a size with many workgroups, and its place in a step: ModelWithLoss and the Trainer.

Margins: the kernels' per-pixel arithmetic is fp32 (unit roundoff 6e-8, a few operations per channel) and the sum over pixels is double;
the reference's own fp32 sits 1e-7 from float64.  1e-5 relative, the margin test_gpu_contrastive.py uses for such a kernel, leaves two
orders of magnitude; a case that needs more is summing in the wrong precision."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
sys.path.insert(0, HERE)

FORMS = ('auto', 'direct', 'staged')


@pytest.fixture(scope='module')
def z():
	return np.load(os.path.join(GOLD, 'part_loss.npz'))


def _run(x, lab, m, form='auto'):
	from find_amd import functional as FN
	xt = torch.as_tensor(x).cuda().requires_grad_(True)
	mt = torch.as_tensor(m).cuda().requires_grad_(True)
	loss, ce = FN.part_cross_entropy(xt, torch.as_tensor(lab).cuda(), mt, return_ce=True, form=form)
	assert not ce.requires_grad and loss.dtype == torch.float32 and loss.dim() == 0 and ce.shape == mt.shape
	loss.backward()
	torch.cuda.synchronize()
	return loss.detach(), ce, xt.grad, mt.grad


@pytest.mark.parametrize('form', FORMS)
def test_loss_and_gradients_equal_the_reference(z, form):
	for name in z['ce_cases']:
		name = str(name)
		loss, ce, dx, dm = _run(z[f'ce/{name}/logits'], z[f'ce/{name}/gt_labels'], z[f'ce/{name}/mask'], form)
		want = float(z[f'ce/{name}/loss'])
		print(name, form, 'loss', loss.item(), want)
		for t in (loss, ce, dx, dm):
			assert torch.isfinite(t).all(), name
		assert abs(loss.item() - want) <= 1e-5 * max(1.0, abs(want)), (name, loss.item(), want)
		for got, key in ((dx, 'd_logits'), (dm, 'd_mask')):
			w = z[f'ce/{name}/{key}']
			err = np.abs(got.cpu().numpy().astype(np.float64) - w).max()
			print(name, form, key, err, np.abs(w).max())
			assert err <= 1e-5 * np.abs(w).max(), (name, key, err, np.abs(w).max())
		w = z[f'ce/{name}/CE_loss']
		err = np.abs(ce.cpu().numpy().astype(np.float64) - w).max()
		assert err <= 1e-5 * max(1.0, np.abs(w).max()), (name, err)
		assert (dx[..., 0] == 0).all(), name


def test_labels_equal_the_reference(z):
	from find_amd import functional as FN
	for name in z['label_cases']:
		name = str(name)
		got = FN.part_labels(torch.from_numpy(z[f'labels/{name}/gt_logits']).cuda(), tuple(int(s) for s in z[f'labels/{name}/size']))
		assert got.dtype == torch.int32
		np.testing.assert_array_equal(got.cpu().numpy(), z[f'labels/{name}/gt_labels'], err_msg=name)
	for name in z['ce_cases']:
		name = str(name)
		got = FN.part_labels(torch.from_numpy(z[f'ce/{name}/gt_logits']).cuda(), z[f'ce/{name}/mask'].shape[1:])
		np.testing.assert_array_equal(got.cpu().numpy(), z[f'ce/{name}/gt_labels'], err_msg=name)


@pytest.fixture(scope='module')
def large():
	"""B = 2, 96 x 96, C = 21: 18 432 pixels = 72 tiles of 256 -- many workgroups, and the final pass adds 72 partials."""
	from test_part_loss_host import part_ce_f64
	rng = np.random.default_rng(11)
	x = rng.standard_normal((2, 96, 96, 21)).astype(np.float32) * 3
	m = rng.uniform(0, 1, (2, 96, 96)).astype(np.float32)
	m[m < 0.3] = 0
	lab = rng.integers(0, 21, (2, 96, 96)).astype(np.int32)
	return x, lab, m, part_ce_f64(x, lab, m, gl=1.0)


@pytest.mark.parametrize('form', FORMS)
def test_many_workgroups_against_float64(large, form):
	x, lab, m, (l64, ce64, d64, dm64) = large
	loss, ce, dx, dm = _run(x, lab, m, form)
	print(form, loss.item(), l64)
	assert abs(loss.item() - l64) <= 1e-5 * max(1.0, abs(l64))
	assert np.abs(dx.cpu().numpy() - d64).max() <= 1e-5 * np.abs(d64).max()
	assert np.abs(dm.cpu().numpy() - dm64).max() <= 1e-5 * np.abs(dm64).max()
	assert np.abs(ce.cpu().numpy() - ce64).max() <= 1e-5 * max(1.0, np.abs(ce64).max())
	assert (dx[..., 0] == 0).all()


@pytest.mark.parametrize('form', FORMS)
def test_two_runs_are_bit_identical(large, form):
	x, lab, m, _ = large
	a, b = _run(x, lab, m, form), _run(x, lab, m, form)
	for s, t in zip(a, b):
		assert torch.equal(s, t)


@pytest.mark.parametrize('form', FORMS)
def test_out_of_range_label_gives_nan_not_a_fault(form):
	"""Label C at pixel 0: a kernel without the guard would read the next pixel's channel 0 -- inside the buffer -- and fail here."""
	rng = np.random.default_rng(3)
	C = 5
	x = rng.standard_normal((1, 4, 4, C)).astype(np.float32)
	m = np.full((1, 4, 4), 0.5, np.float32)
	lab = rng.integers(0, C, (1, 4, 4)).astype(np.int32)
	lab[0, 0, 0] = C
	loss, ce, dx, dm = _run(x, lab, m, form)
	assert torch.isnan(loss).item()
	assert torch.isnan(dx[0, 0, 0]).all() and torch.isnan(dm[0, 0, 0]).item() and torch.isnan(ce[0, 0, 0]).item()
	rest = dx.reshape(-1, C)[1:]
	assert torch.isfinite(rest).all() and torch.isfinite(dm.reshape(-1)[1:]).all()


def test_c_interface_refuses_bad_arguments():
	from find_amd import _lib
	from find_amd import functional as FN
	x = torch.zeros(2, 4, 4, 200, device='cuda')
	lab = torch.zeros(2, 4, 4, dtype=torch.int32, device='cuda')
	m = torch.ones(2, 4, 4, device='cuda')
	with pytest.raises(RuntimeError, match='staged form'):   # 64 pixels of 201 floats do not fit the tile
		FN.part_cross_entropy(x, lab, m, form='staged')
	loss = FN.part_cross_entropy(x, lab, m)   # auto: the direct form
	assert abs(loss.item() - np.log(200.0)) < 1e-5 * np.log(200.0)
	L = _lib.lib()
	assert L.find_part_ce_fwd(None, _lib.ptr(lab), _lib.ptr(m), 32, 200, None, None, None, 0, None) == -1
	assert L.find_part_labels(_lib.ptr(x), 1, 0, 4, 4, 8, 8, _lib.ptr(lab), None) == -1
	with pytest.raises(RuntimeError, match='int32 labels'):
		FN.part_cross_entropy(x, lab.long(), m)


# ------------------------------------------------------------------ ModelWithLoss, Trainer
class StubEncoder:
	"""A fixed stand-in for the frozen image encoder: average-pool by 2, then a seeded 1 x 1 convolution to C class logits."""

	def __init__(self, C=21, device='cuda'):
		g = torch.Generator().manual_seed(0)
		self.w, self.b = (4 * torch.randn(C, 3, generator=g)).to(device), torch.randn(C, generator=g).to(device)
		self.calls = []

	def __call__(self, images, return_features=False, target_feature_maps=None):
		assert return_features and not torch.is_grad_enabled()
		self.calls.append((tuple(images.shape), target_feature_maps))
		x = torch.nn.functional.avg_pool2d(images, 2)
		return {'class_logits': torch.einsum('kc,bchw->bkhw', self.w, x) + self.b[None, :, None, None]}


@pytest.fixture(scope='module')
def step(tmp_path_factory):
	from find_amd import optim, synthetic
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	from find_amd.structures import Meshes, TexturesVertex
	n, C = 2, 21
	v, f = synthetic.template(1002)
	path = str(tmp_path_factory.mktemp('part') / 'classes.pth')
	torch.save({'state_dict': {'features': torch.randn(v.shape[0], C, generator=torch.Generator().manual_seed(1))}}, path)
	opts = Opts(sil_loss=True, restyle_perc_cluster_loss=True, restyle_cluster_per_vertex=True, template_features_pth=path, num_views=2,
				restyle_feature_maps=[8])
	enc = StubEncoder(C)
	mwl = ModelWithLoss(opts=opts, device='cpu', restyle_encoder=enc, use_shapevec=True, use_texvec=True, use_posevec=True, train_size=n, val_size=1,
						shapevec_size=100, texvec_size=100, posevec_size=100, template_mesh_loc=None, restyle_cluster_per_vertex=True)
	mwl = mwl.to('cuda')
	mwl.model.set_template(v.cuda(), f.cuda())
	lat = synthetic.latents(n, seed=3, device='cuda')
	with torch.no_grad():
		for k in ('shapevec', 'texvec', 'posevec', 'reg'):
			getattr(mwl.model, k).data.copy_(lat[k])
	gv, gf, gc = synthetic.gt_feet(n, 1002, seed=3, device='cuda')
	batch = dict(mesh=Meshes(gv, gf, TexturesVertex(gc.clamp(0.05, 0.95))), idx=torch.arange(n, device='cuda'), name=[f'{i:04d}' for i in range(n)])
	opt = optim.Adam(mwl.model.main_params, lr=1e-4, capturable=True)
	return mwl, opts, batch, opt, enc


def test_model_with_loss_equals_the_reference_composition(step):
	from find_amd.train_utils import sample_latent_vectors
	mwl, opts, batch, opt, enc = step
	b = dict(batch)
	b.update(sample_latent_vectors(b, mwl.model.latent_vectors_train))
	flags = dict(sil=True, render_foot=True, return_renders=True, restyle_feature_maps=[8])
	np.random.seed(5)
	del enc.calls[:]
	loss, losses, rdr = mwl(b, 0, opts, restyle_perc_cluster=True, **flags)
	assert list(losses) == ['loss_sil', 'loss_restyle_perc_cluster'] and list(losses)[-1] == 'loss_restyle_perc_cluster'
	assert enc.calls == [((4, 3, 256, 256), [8])]   # the GT images only, once
	feats, mask, gt_img = rdr['pred']['features'], rdr['pred']['mask'], rdr['gt']['image']
	assert feats.shape == (2, 2, 256, 256, 21) and rdr['gt_labels'].shape == (4, 256, 256) and rdr['CE_loss'].shape == (4, 256, 256)
	assert rdr['gt_logits'].shape == (4, 21, 256, 256)
	# upstream's lines (losses.py:262-276, 302) in float64 on what the step returned
	F = torch.nn.functional
	with torch.no_grad():
		g = enc(gt_img.reshape(4, 256, 256, 3).permute(0, 3, 1, 2), return_features=True)['class_logits']
		assert g.shape == (4, 21, 128, 128)
		up = F.interpolate(feats.detach().reshape(4, 256, 256, 21).permute(0, 3, 1, 2).double(), size=(256, 256), mode='bilinear')
		labels = torch.argmax(F.interpolate(g.double(), size=(256, 256), mode='bilinear'), dim=1)
		m = mask.detach().reshape(4, 256, 256).double()
		up[:, 0] = (m == 0) * 100
		want = (torch.nn.CrossEntropyLoss(reduction='none')(up, labels) * m).mean().item() * opts.weight_restyle_perc_cluster
	got = losses['loss_restyle_perc_cluster'].item()
	print('part loss', got, want, 'labels differing from float64:', int((labels != rdr['gt_labels']).sum()))
	assert (m == 0).any() and (m > 0).any() and want > 0
	assert abs(got - want) <= 1e-5 * abs(want), (got, want)
	mwl.zero_grad()
	loss.backward()
	torch.cuda.synchronize()
	grads = [p.grad for p in mwl.model.main_params if p.grad is not None]
	assert grads and all(torch.isfinite(q).all() for q in grads) and any(q.abs().max().item() > 0 for q in grads)
	pg = mwl.model.per_vertex_features.grad
	assert pg is not None and pg.shape == (1, mwl.model.template_verts.shape[1], 21) and torch.isfinite(pg).all() and pg.abs().max().item() > 0
	# the same step without the term: the other terms bit for bit, no feature render, no encoder call
	np.random.seed(5)
	del enc.calls[:]
	loss0, losses0, rdr0 = mwl(b, 0, opts, **flags)
	assert list(losses0) == ['loss_sil'] and torch.equal(losses0['loss_sil'], losses['loss_sil'])
	assert not enc.calls and 'features' not in rdr0['pred'] and 'gt_labels' not in rdr0


def test_trainer_runs_the_term_eagerly(step):
	from find_amd.trainer import Trainer
	mwl, opts, batch, opt, enc = step
	tr = Trainer([opt], mwl, [batch, batch], [], opts, latent_vectors_train=mwl.model.latent_vectors_train, device='cuda', graph='auto')
	np.random.seed(3)
	msg = tr.train_epoch(0, model_kwargs=dict(sil=True, restyle_perc_cluster=True, render_foot=True, restyle_feature_maps=[8]))
	assert tr.last_mode == 'eager', msg
	vals = tr.log[0]['train_loss']['Restyle Perc Cluster']
	assert len(vals) == 2 and all(np.isfinite(vals)) and all(np.isfinite(tr.log[0]['train_loss']['Sil']))
