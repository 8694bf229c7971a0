"""The contrastive pose loss on the MI355X (find_contrastive_fwd / _bwd) against what the REFERENCE's ContrastiveLoss and ModelWithLoss.forward
returned (tests/golden/contrastive.npz, make_golden_contrastive.py ran src/model/losses.py:305-333 and model.py:1001-1163 for real), and
its place in a step: the draw order against the camera poses, the HIP-graph replay with fresh pairs per call, the Trainer."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
sys.path.insert(0, HERE)


@pytest.fixture(scope='module')
def z():
	return np.load(os.path.join(GOLD, 'contrastive.npz'))


def _case(z, name):
	from find_amd import functional as FN
	v = torch.from_numpy(z[f'case/{name}/vecs']).cuda().requires_grad_(True)
	c = torch.from_numpy(z[f'case/{name}/codes']).float().cuda()
	p = torch.from_numpy(z[f'case/{name}/pairs']).cuda()
	loss = FN.contrastive_pose(v, c, p)
	loss.backward()
	torch.cuda.synchronize()
	return loss.detach(), v.grad.detach()


def test_loss_and_gradient_equal_the_reference(z):
	for name in z['cases']:
		name = str(name)
		loss, g = _case(z, name)
		assert loss.dtype == torch.float32 and loss.dim() == 0
		want = float(z[f'case/{name}/loss'])
		assert abs(loss.item() - want) < 1e-5 * max(1.0, abs(want)), (name, loss.item(), want)
		gw = z[f'case/{name}/d_vecs']
		err = np.abs(g.cpu().numpy().astype(np.float64) - gw).max()
		assert err <= 1e-5 * max(1e-6, np.abs(gw).max()), (name, err, np.abs(gw).max())


def test_duplicated_row_gives_finite_zero_gradient(z):
	loss, g = _case(z, 'n3_dup')
	assert torch.isfinite(loss) and torch.isfinite(g).all()
	# rows 0 and 2 are equal: the pair between them contributes nothing; alone it gives exactly zero
	from find_amd import functional as FN
	v = torch.from_numpy(z['case/n3_dup/vecs']).cuda().requires_grad_(True)
	c = torch.from_numpy(z['case/n3_dup/codes']).float().cuda()
	FN.contrastive_pose(v, c, torch.tensor([[0, 2], [2, 0]], dtype=torch.int32, device='cuda')).backward()
	assert torch.isfinite(v.grad).all() and v.grad.abs().max().item() == 0.0


def test_two_runs_are_bit_identical(z):
	for name in ('n16_k256', 'n24_k3_chunked'):
		a, ga = _case(z, name)
		b, gb = _case(z, name)
		assert torch.equal(a, b) and torch.equal(ga, gb), name


def test_out_of_range_pair_gives_nan_not_a_fault():
	from find_amd import functional as FN
	v = torch.randn(3, 8, device='cuda', requires_grad=True)
	c = torch.ones(3, 2, device='cuda')
	loss = FN.contrastive_pose(v, c, torch.tensor([[0, 1], [1, 3]], dtype=torch.int32, device='cuda'))
	loss.backward()
	torch.cuda.synchronize()
	assert torch.isnan(loss).item() and torch.isnan(v.grad).all()


def test_gradient_reaches_label_shared_posevec_rows(z):
	"""Two scans with the same pose label share one posevec row (use_latent_labels): the pair between them has d = 0, and the rows'
	gradients arrive in the table through latent_gather's backward -- the sum of the gathered rows' gradients."""
	from find_amd import functional as FN
	from find_amd.losses import ContrastiveLoss
	table = torch.from_numpy(z['case/n5_k37/vecs']).cuda().requires_grad_(True)
	idx = torch.tensor([0, 1, 1, 3, 4, 0], device='cuda')   # batch rows 1, 2 and 0, 5 share a table row
	codes = torch.tensor(np.stack([z['case/n5_k37/codes'][i] for i in idx.tolist()]), device='cuda')   # (float64, as collated)
	rows = FN.latent_gather(table, idx)
	rows.retain_grad()
	pairs = torch.tensor([[1, 2], [0, 3], [5, 0], [2, 4], [3, 5], [4, 1]], dtype=torch.int32, device='cuda')
	loss = ContrastiveLoss()(rows, codes, pairs=pairs)
	loss.backward()
	torch.cuda.synchronize()
	assert torch.isfinite(table.grad).all()
	want = torch.zeros_like(table)
	want.index_add_(0, idx, rows.grad)
	assert torch.equal(table.grad, want)
	assert table.grad[2].abs().max().item() == 0 and table.grad[1].abs().max().item() > 0
	# and the value against the float64 restatement on the gathered rows
	from test_contrastive_host import contrastive_f64
	l64, _ = contrastive_f64(rows.detach().cpu().numpy(), codes.cpu().numpy(), pairs.cpu().numpy())
	assert abs(loss.item() - l64) < 1e-5 * max(1.0, abs(l64))


# ------------------------------------------------------------------ ModelWithLoss
def _composition_model():
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	c = np.load(os.path.join(GOLD, 'composition.npz'))
	lab = {k[len('labels/'):]: [str(s) for s in c[k]] for k in c.files if k.startswith('labels/')}
	opts = Opts(chamf_loss=True, smooth_loss=True, use_pose_code=True, use_latent_labels=True, cont_pose_loss=True)
	mwl = ModelWithLoss(opts=opts, device='cpu', use_shapevec=True, use_texvec=True, use_posevec=True, train_size=3, val_size=3, shapevec_size=100,
						texvec_size=100, posevec_size=100, template_mesh_loc=None, latent_labels=lab)
	m = mwl.model
	m.set_template(torch.from_numpy(c['sd/template_verts'])[0], torch.from_numpy(c['sd/template_faces'])[0])
	m.load_state_dict({k[3:]: torch.from_numpy(c[k]) for k in c.files if k.startswith('sd/')}, strict=True)
	return mwl.to('cuda'), opts, c


def _composition_batch(mwl, c, idx, pose_code):
	from find_amd.structures import Meshes, TexturesVertex
	from find_amd.train_utils import sample_latent_vectors
	dev = torch.device('cuda')
	gv, gf, gc = (torch.from_numpy(c[f'gt/{k}']).to(dev) for k in ('verts', 'faces', 'colours'))
	feet, names = [str(s) for s in c['batch/feet']], [str(s) for s in c['batch/names']]
	b = dict(mesh=Meshes(gv[idx].contiguous(), gf, TexturesVertex(gc[idx].contiguous())), idx=torch.tensor(idx, device=dev), name=[names[i] for i in idx],
			 shape=[feet[i] for i in idx], tex=[feet[i] for i in idx], pose=[names[i] for i in idx], reg=[names[i] for i in idx],
			 pose_code=torch.as_tensor(pose_code, device=dev))
	b.update(sample_latent_vectors(b, mwl.model.latent_vectors_train))
	return b


class PairRecorder:
	"""Keeps the pairs every contrastive_pose call received."""

	def __enter__(self):
		from find_amd import functional as FN
		self.FN, self.orig, self.pairs = FN, FN.contrastive_pose, []

		def wrapped(vecs, codes, pairs, margin=0.5):
			self.pairs.append(pairs.cpu().numpy().copy())
			return self.orig(vecs, codes, pairs, margin)
		FN.contrastive_pose = wrapped
		return self

	def __exit__(self, *a):
		self.FN.contrastive_pose = self.orig


def test_model_with_loss_equals_the_reference_composition(z):
	from test_gpu_train3d import FixedDraws
	mwl, opts, c = _composition_model()
	idx = [int(i) for i in z['compose/idx']]
	b = _composition_batch(mwl, c, idx, z['compose/pose_code'])
	dr = [(torch.from_numpy(z[f'compose/draw/{i}/face_idx']).cuda(), torch.from_numpy(z[f'compose/draw/{i}/uv']).cuda()) for i in range(int(z['compose/n_draws']))]
	assert len(dr) == 2
	np.random.seed(int(z['compose/seed']))
	with FixedDraws([dr[0], dr[1], None]), PairRecorder() as rec:
		loss, losses = mwl(b, 0, opts, chamf=True, smooth=True, cont_pose=True)
	np.testing.assert_array_equal(rec.pairs[0], z['compose/pairs'])
	assert list(losses) == [str(s) for s in z['compose/loss_keys']] == ['loss_chamf', 'loss_smooth', 'loss_cont_pose']
	for k, v in losses.items():
		want = float(z[f'compose/losses/{k}'])
		assert v.dtype == torch.float32 and abs(v.item() - want) < 1e-4 * max(1.0, abs(want)), (k, v.item(), want)
	assert abs(loss.item() - float(z['compose/loss'])) < 1e-4 * max(1.0, abs(float(z['compose/loss'])))
	loss.backward()
	g = mwl.model.posevec.data.grad
	assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0
	# the same step without the term: the other terms are the same numbers
	with FixedDraws([dr[0], dr[1], None]):
		loss0, losses0 = mwl(b, 0, opts, chamf=True, smooth=True)
	assert list(losses0) == ['loss_chamf', 'loss_smooth']
	for k, v in losses0.items():
		assert v.item() == losses[k].item(), k
		assert abs(v.item() - float(z[f'compose/without/losses/{k}'])) < 1e-4 * max(1.0, abs(v.item()))


def test_one_scan_gives_no_term_and_missing_pose_rows_raise(z):
	mwl, opts, c = _composition_model()
	b = _composition_batch(mwl, c, [1], z['compose/pose_code'][:1])
	state = np.random.get_state()
	loss, losses = mwl(b, 0, opts, smooth=True, cont_pose=True)
	assert list(losses) == ['loss_smooth']
	assert np.array_equal(np.random.get_state()[1], state[1])   # nothing drawn
	_, only = mwl(b, 0, opts, cont_pose=True)
	assert only == {}
	del b['posevec_train']
	with pytest.raises(ValueError, match='Contrastive pose loss used, but no pose found'):
		mwl(b, 0, opts, smooth=True, cont_pose=True)


def test_pairs_are_drawn_before_the_camera_poses(z):
	"""With the same seed a rendering step uses the reference's pairs AND the reference's views: upstream shuffles the pairs before
	sample_views draws the poses (model.py:1042-1071), both from numpy's global generator."""
	from find_amd.losses import draw_pairs
	from find_amd.train_utils import sample_latent_vectors
	mwl, opts, b, _ = _setup16(n=3)
	b.update(sample_latent_vectors(b, mwl.model.latent_vectors_train))
	opts.num_views = 2
	seen = []
	orig = mwl._views

	def views(o):
		R, T = orig(o)
		seen.append((R.clone(), T.clone()))
		return R, T
	mwl._views = views
	np.random.seed(99)
	with PairRecorder() as rec:
		loss, losses = mwl(b, 0, opts, smooth=True, sil=True, render_foot=True, cont_pose=True)
	torch.cuda.synchronize()
	assert list(losses) == ['loss_smooth', 'loss_cont_pose', 'loss_sil']
	free = dict(dist_mean=0.3, dist_std=0, elev_min=-90, elev_max=90, azim_min=-90, azim_max=90)
	np.random.seed(99)
	want_pairs = draw_pairs(3)
	R, T = mwl.rdr.sample_views(nviews=2, **free)
	np.testing.assert_array_equal(rec.pairs[0], want_pairs)
	assert torch.equal(seen[0][0].cpu(), R.cpu()) and torch.equal(seen[0][1].cpu(), T.cpu())
	np.random.seed(99)
	R_first, _ = mwl.rdr.sample_views(nviews=2, **free)   # (poses drawn before the pairs would be these)
	assert not torch.equal(seen[0][0].cpu(), R_first.cpu())


# ------------------------------------------------------------------ graph replay
def _setup16(capturable=True, n=16):
	from find_amd import optim, synthetic
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	from find_amd.structures import Meshes, TexturesVertex
	opts = Opts(chamf_loss=True, smooth_loss=True, texture_loss=True, use_pose_code=True, cont_pose_loss=True)
	mwl = ModelWithLoss(opts=opts, device='cpu', use_shapevec=True, use_texvec=True, use_posevec=True, train_size=n, val_size=1,
						shapevec_size=100, texvec_size=100, posevec_size=100, template_mesh_loc=None)
	mwl = mwl.to('cuda')
	v, f = synthetic.template(1002)
	mwl.model.set_template(v.cuda(), f.cuda())
	lat = synthetic.latents(n, seed=3, device='cuda')
	with torch.no_grad():
		for k in ('shapevec', 'texvec', 'posevec', 'reg'):
			getattr(mwl.model, k).data.copy_(lat[k])
		mwl.model.posevec.data.mul_(0.5)   # (pairs on both sides of the hinge)
	gv, gf, gc = synthetic.gt_feet(n, 1002, seed=3, device='cuda')
	rng = np.random.default_rng(5)
	codes = np.zeros((n, 8))
	for i in range(n):
		codes[i, rng.integers(0, 4)] = rng.choice([-1.0, 1.0])
	batch = dict(mesh=Meshes(gv, gf, TexturesVertex(gc.clamp(0.05, 0.95))), idx=torch.arange(n, device='cuda'),
				 name=[f'{i:04d}' for i in range(n)], pose_code=torch.from_numpy(codes).cuda())
	opt = optim.Adam(mwl.model.main_params, lr=1e-4, capturable=capturable)
	return mwl, opts, batch, opt


def test_graphed_step_draws_fresh_pairs_per_replay():
	from find_amd.graph import GraphedStep
	mwl, opts, batch, opt = _setup16()
	flags = dict(chamf=True, smooth=True, texture=True, cont_pose=True)
	gs = GraphedStep(mwl, opts, [opt], **flags)
	np.random.seed(7)
	pairs_seen, vals = [], []
	for step in range(4):
		loss, losses = gs(batch, 0)
		st = next(iter(gs._graphs.values()))
		torch.cuda.synchronize()
		assert list(losses) == ['loss_chamf', 'loss_smooth', 'loss_tex', 'loss_cont_pose']
		p = st.pairs_dev.clone()
		assert p.shape == (10, 2)
		pairs_seen.append(p.cpu().numpy())
		vals.append(losses['loss_cont_pose'].item())
	assert gs.n_captures == 1
	for a, b in zip(pairs_seen, pairs_seen[1:]):
		assert not np.array_equal(a, b)
	# the pairs are the draws numpy's generator makes in that order (first replay: the pairs drawn at capture time)
	from find_amd.losses import draw_pairs
	np.random.seed(7)
	for p in pairs_seen:
		np.testing.assert_array_equal(p, draw_pairs(16))
	assert all(np.isfinite(vals))


def test_graphed_term_equals_the_eager_op_on_the_replays_inputs():
	"""Frozen network (lr 0): every replay's loss_cont_pose equals contrastive_pose on the table rows and that replay's pairs."""
	from find_amd import functional as FN
	from find_amd.graph import GraphedStep
	mwl, opts, batch, opt = _setup16()
	for g in opt.param_groups:
		g['lr'] = 0.0
	gs = GraphedStep(mwl, opts, [opt], cont_pose=True, smooth=True)
	np.random.seed(11)
	codes = batch['pose_code'].float()
	for _ in range(3):
		loss, losses = gs(batch, 0)
		st = next(iter(gs._graphs.values()))
		torch.cuda.synchronize()
		with torch.no_grad():
			want = FN.contrastive_pose(mwl.model.posevec.data, codes, st.pairs_dev)
		torch.cuda.synchronize()
		assert losses['loss_cont_pose'].item() == want.item()


def test_trainer_replays_a_cont_pose_step_as_a_graph():
	from find_amd.trainer import Trainer
	mwl, opts, batch, opt = _setup16()
	tr = Trainer([opt], mwl, [batch, batch], [], opts, latent_vectors_train=mwl.model.latent_vectors_train, device='cuda', graph=True)
	np.random.seed(3)
	msg = tr.train_epoch(0, model_kwargs=dict(smooth=True, cont_pose=True))
	assert tr.last_mode == 'graph', msg
	assert 'Cont Pose' in tr.log[0]['train_loss'] and len(tr.log[0]['train_loss']['Cont Pose']) == 2
	assert all(np.isfinite(tr.log[0]['train_loss']['Cont Pose']))
