"""The skinned foot model on the MI355X: find_skin_fwd / find_skin_bwd through FN.linear_blend_skinning against the float64 restatement of the
definition (tests/skin_ref.py) on the same fp32 inputs, and its place in SkinnedModel, ModelWithLoss, Trainer, evaluate and init_registration.

Margins: none is a constant of the code under test.  Every float comparison follows tests/test_gpu_measure.py's _held: the same restatement is
also evaluated in float32 on the CPU; with e32 its worst error against float64 over the case's tensor, the HIP result must lie within
max(4 e32, 2 ulp of the largest value) of the float64 one.  Each case prints its figures (DESIGN 7.11 records the worst).

Shapes, the smallest that cross each boundary: V = 1, 63, 64, 65 (below and around a wave), 257 (past a vertex tile: a tile is at most 64 rows, and
V / 256 rounded up), 1000 (several blocks, a ragged last one) and one case at (N, V, J, B) = (16, 6890, 24, 10); J = 1 (the root alone), 2, 5, 24
and 65 (past a wave: the per-foot kernels loop); the three chains and both feature layouts; B = 1, 10, 37; N = 1, 3, 33 (with J = 24 a tile
kernel holds 7 feet per pass: 33 feet take five passes, and 34 fit one pass at J = 5).  Poses: exactly zero, 1e-6 (the series branch), generic, one joint at pi - 1e-3, one at 4 rad.  Every case runs twice
and must repeat bit for bit."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import poison   # noqa: E402
import skin_ref   # noqa: E402

WORST = {}   # name of a quantity -> the worst e_hip / max(e32, ulp) seen (printed by the last test of the file)


def _ulp(x):
	return float(np.spacing(np.float32(abs(float(x)))))


def _held(name, hip, ref64, ref32, kind=None):
	hip, ref64, ref32 = hip.detach().double().cpu(), ref64.detach().double(), ref32.detach().double()
	assert hip.shape == ref64.shape, (name, hip.shape, ref64.shape)
	e_hip = (hip - ref64).abs().max().item()
	e32 = (ref32 - ref64).abs().max().item()
	ulp = _ulp(ref64.abs().max().item())
	ratio = e_hip / max(e32, ulp)
	print(f'{name}: e_hip {e_hip:.3e}  e32 {e32:.3e}  ulp {ulp:.3e}  scale {ref64.abs().max().item():.3e}  e_hip / max(e32, ulp) {ratio:.2f}')
	if kind:
		WORST[kind] = max(WORST.get(kind, 0.), ratio)
	assert np.isfinite(e_hip) and e_hip <= max(4 * e32, 2 * ulp), (name, e_hip, e32, ulp)


# ------------------------------------------------------------------ inputs
def _consts(V, J, B, chain='tree', fj='all', seed=0):
	from find_amd import synthetic
	from find_amd.model import _skin_arrays
	c = _skin_arrays(synthetic.skinned_model(V=V, J=J, B=B, chain=chain, feature_joints=fj, seed=seed), B)
	c.pop('faces')
	return c


def _inputs(N, V, J, B, kind='generic', seed=0):
	"""fp32 pose (N, 3J), betas, trans and an upstream gradient.  kind: 'zero', 'tiny' (1e-6), 'generic' (every joint below 1 rad), 'pi' / 'four'
	(generic, with the last joint of every foot at pi - 1e-3 / 4 rad about a random axis)."""
	g = torch.Generator().manual_seed(seed)
	axis = torch.randn(N, J, 3, generator=g)
	axis = axis / axis.norm(dim=-1, keepdim=True)
	angle = torch.rand(N, J, 1, generator=g)
	if kind == 'zero':
		angle = angle * 0
	elif kind == 'tiny':
		angle = angle * 1e-6
	elif kind == 'pi':
		angle[:, -1] = np.pi - 1e-3
	elif kind == 'four':
		angle[:, -1] = 4.0
	pose = (axis * angle).reshape(N, 3 * J)
	return pose, torch.randn(N, B, generator=g), torch.randn(N, 3, generator=g) * 0.1, torch.randn(N, V, 3, generator=g)


def _hip(consts, pose, betas, trans, d_out):
	from find_amd import functional as FN
	c = {k: v.cuda() for k, v in consts.items()}
	p, b, t = (x.cuda().requires_grad_(True) for x in (pose, betas, trans))
	out, joints = FN.linear_blend_skinning(c, p, b, t, return_joints=True)
	assert not joints.requires_grad
	gp, gb, gt = torch.autograd.grad(out, (p, b, t), d_out.cuda())
	torch.cuda.synchronize()
	return dict(out=out.detach(), joints=joints, d_pose=gp, d_betas=gb, d_trans=gt)


def _check(tag, consts, pose, betas, trans, d_out):
	r = _hip(consts, pose, betas, trans, d_out)
	r2 = _hip(consts, pose, betas, trans, d_out)
	for k in r:
		assert torch.equal(r[k], r2[k]), (tag, k)   # no atomics: a second run repeats bit for bit
	ref64 = skin_ref.with_grads(consts, pose, betas, trans, d_out, torch.float64)
	ref32 = skin_ref.with_grads(consts, pose, betas, trans, d_out, torch.float32)
	for k, a, b in zip(('out', 'd_pose', 'd_betas', 'd_trans'), ref64, ref32):
		_held(f'{tag} {k}', r[k], a, b, kind=k)
	j64 = skin_ref.skin(consts, pose, betas, trans, torch.float64, return_joints=True)[1]
	j32 = skin_ref.skin(consts, pose, betas, trans, torch.float32, return_joints=True)[1]
	_held(f'{tag} joints', r['joints'], j64, j32, kind='joints')
	return r


# ------------------------------------------------------------------ parity
CASES = (
	# (N, V, J, B, chain, feature joints, poses)
	[(3, V, 5, 10, 'tree', fj, 'generic') for V, fj in ((1, 'all'), (63, 'nonroot'), (64, 'all'), (65, 'nonroot'), (257, 'all'), (1000, 'nonroot'))]
	+ [(3, 65, 1, 10, 'line', 'all', 'generic'), (3, 65, 1, 10, 'line', 'nonroot', 'generic'), (3, 65, 2, 10, 'star', 'nonroot', 'generic'),
	   (3, 65, 24, 10, 'tree', 'nonroot', 'generic'), (3, 65, 24, 10, 'star', 'all', 'generic'), (3, 65, 65, 10, 'line', 'all', 'generic'),
	   (3, 65, 65, 10, 'tree', 'nonroot', 'generic')]
	+ [(3, 257, 5, 1, 'line', 'all', 'generic'), (3, 257, 5, 37, 'star', 'nonroot', 'generic')]
	+ [(1, 257, 5, 10, 'line', 'nonroot', 'generic'), (33, 257, 5, 10, 'tree', 'all', 'generic'), (33, 65, 24, 10, 'tree', 'all', 'generic')]
	+ [(3, 65, 5, 10, 'tree', 'all', kind) for kind in ('zero', 'tiny', 'pi', 'four')]
	+ [(3, 65, 5, 10, 'line', 'nonroot', kind) for kind in ('zero', 'pi')]
	+ [(16, 6890, 24, 10, 'tree', 'all', 'generic')])


@pytest.mark.parametrize('N,V,J,B,chain,fj,kind', CASES)
def test_forward_and_gradients_are_held_to_float64(N, V, J, B, chain, fj, kind):
	consts = _consts(V, J, B, chain, fj, seed=V + J)
	r = _check(f'N{N} V{V} J{J} B{B} {chain} {fj} {kind}', consts, *_inputs(N, V, J, B, kind, seed=N + V + J + B))
	if kind == 'zero':   # the derivatives at theta = 0 are finite, and the pose gradient is there
		assert torch.isfinite(r['d_pose']).all() and r['d_pose'].abs().max() > 0


def test_a_foot_does_not_depend_on_its_batch():
	N, V, J, B = 33, 257, 24, 10   # (five passes over the feet in the tile kernels; alone, a foot takes one)
	consts = _consts(V, J, B, 'tree', 'all', seed=2)
	pose, betas, trans, d_out = _inputs(N, V, J, B, seed=3)
	full = _hip(consts, pose, betas, trans, d_out)
	for n in (0, 7, 32):
		one = _hip(consts, pose[n:n + 1], betas[n:n + 1], trans[n:n + 1], d_out[n:n + 1])
		for k in full:
			assert torch.equal(full[k][n:n + 1], one[k]), (n, k)


@contextlib.contextmanager
def poisoned_skinning(byte):
	"""tests/poison.py's proxy on find_amd.skinning, as tests/test_gpu_align.py puts it on find_amd.align: every torch.empty / empty_like of the
	module (the outputs and the gradients) comes back filled with `byte`.  The workspaces are functional._ws's: poison.poisoned fills those."""
	from find_amd import skinning as mod
	if byte not in poison.PATTERNS:
		raise ValueError(byte)
	assert mod.torch is torch
	proxy = poison._TorchProxy(byte)
	try:
		mod.torch = proxy
		yield proxy
	finally:
		mod.torch = torch


def test_poisoned_allocations_change_nothing():
	from find_amd import skinning
	N, V, J, B = 9, 257, 24, 10   # (nine feet: two passes over the feet in the tile kernels)
	consts = _consts(V, J, B, 'tree', 'nonroot', seed=4)
	args = _inputs(N, V, J, B, seed=5)
	runs = []
	for byte in (None, 0xFF, 0x00):
		_hip(consts, *args)   # (what a forgotten region would hold: the right values of this call)
		if byte is None:
			runs.append(_hip(consts, *args))
		else:
			with poison.poisoned(byte) as ws_proxy, poisoned_skinning(byte) as proxy:
				runs.append(_hip(consts, *args))
			assert ws_proxy.calls == 2 and proxy.calls == 2 + 3   # the two workspaces; out and joints, three gradients
	assert skinning.torch is torch
	bad = poison.compare('skin', *runs)
	assert not bad, '\n'.join(bad)


# ------------------------------------------------------------------ the stack
def _model(V=1002, J=5, B=10, train_size=3, val_size=2, seed=1, **kw):
	from find_amd import synthetic
	from find_amd.model import SkinnedModel
	return SkinnedModel.from_arrays(synthetic.skinned_model(V=V, J=J, B=B, chain='tree', seed=seed), device='cuda', num_betas=B, train_size=train_size,
									val_size=val_size, **kw)


def _fit(model, seed):
	"""Tables of a fitted-looking model."""
	g = torch.Generator().manual_seed(seed)
	with torch.no_grad():
		for sfx in ('train', 'val'):
			pose, betas, trans, reg = (getattr(model, f'{k}_{sfx}').data for k in ('pose', 'betas', 'trans', 'reg'))
			pose.copy_((torch.randn(pose.shape, generator=g) * 0.2).cuda())
			betas.copy_(torch.randn(betas.shape, generator=g).cuda())
			trans.add_((torch.randn(trans.shape, generator=g) * 0.005).cuda())
			reg[:, 0:3] = (torch.randn(reg.shape[0], 3, generator=g) * 0.01).cuda()
			reg[:, 3:6] = (torch.randn(reg.shape[0], 3, generator=g) * 0.1).cuda()
	return model


def _draws(n, F_gt, F_pred, seed, S=5000):
	g = torch.Generator().manual_seed(seed)
	return [(torch.randint(0, F, (n, S), generator=g, dtype=torch.int32).cuda(), torch.rand(n, S, 2, generator=g).cuda()) for F in (F_gt, F_pred)] + [None]


def test_model_with_loss_equals_the_restatement_composed_with_the_ops(tmp_path):
	"""chamf + smooth of ModelWithLoss(model_type='skinned') against the same step with the model's decode replaced by the float64 restatement
	(rounded to fp32, then the same registration, sampler, Chamfer and smoothness ops).  The two sets of vertices differ by fp32 rounding
	(1e-8 m on 0.1 m); the losses are smooth in them, so 1e-4 relative -- the bound tests/test_gpu_pca.py holds its losses to -- is generous."""
	from test_gpu_train3d import FixedDraws
	from find_amd import functional as FN
	from find_amd import synthetic
	from find_amd.model import SkinnedModel
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	from find_amd.structures import Meshes, TexturesVertex, extend_template
	from find_amd.train_utils import sample_latent_vectors
	data = synthetic.skinned_model(V=1002, J=5, B=10, chain='tree', seed=1)
	np.savez(str(tmp_path / 'm.npz'), **data)
	opts = Opts(model_type='skinned', load_model=str(tmp_path / 'm.npz'))
	mwl = ModelWithLoss(opts=opts, device='cuda', train_size=3, val_size=2)
	m = _fit(mwl.model, seed=6)
	assert isinstance(m, SkinnedModel)
	gv, gf, _ = synthetic.gt_feet(3, n_verts=1002, seed=2)
	idx = [2, 0]
	b = dict(mesh=Meshes(gv[idx].contiguous(), gf, TexturesVertex(torch.full_like(gv[idx], 0.5))), idx=torch.tensor(idx, device='cuda'))
	b.update(sample_latent_vectors(b, m.latent_vectors_train))
	assert sorted(k for k in b if k.endswith('_train')) == ['betas_train', 'pose_train', 'reg_train', 'trans_train']
	dr = _draws(2, gf.shape[0], m.template_faces.shape[1], seed=7)
	with FixedDraws(dr):
		loss, losses = mwl(b, 0, opts, chamf=True, smooth=True)
	assert list(losses) == ['loss_chamf', 'loss_smooth']
	loss.backward()
	for t in (m.pose_train, m.betas_train, m.trans_train, m.reg_train):
		assert torch.isfinite(t.data.grad).all() and t.data.grad[idx].abs().max() > 0 and torch.all(t.data.grad[1] == 0), t.name
	assert m.dirs.grad is None and m.weights.grad is None

	def restated(batch, is_train=True, **kw):
		X = skin_ref.skin(m.state_dict(), batch['pose_train'].detach().cpu(), batch['betas_train'].detach().cpu(), batch['trans_train'].detach().cpu(),
						  torch.float64).float().cuda()
		X = FN.register_points(torch.zeros(1, X.shape[1], 3, device='cuda'), X, batch['reg_train'].detach())
		meshes = extend_template(m.template_mesh, N=X.shape[0]).update_padded(X)
		meshes.textures = TexturesVertex(torch.full_like(X, 0.5))
		return dict(meshes=meshes, verts=X)
	m.get_meshes_from_batch = restated
	try:
		with FixedDraws(dr):
			loss2, losses2 = mwl(b, 0, opts, chamf=True, smooth=True)
	finally:
		del m.get_meshes_from_batch
	for k in losses:
		a, w = losses[k].item(), losses2[k].item()
		print(f'{k}: model {a:.8e}  restatement {w:.8e}')
		assert w > 0 and abs(a - w) < 1e-4 * abs(w), (k, a, w)
	assert abs(loss.item() - loss2.item()) < 1e-4 * abs(loss2.item())


def _stage_run(graph, stage, path, n_steps=3):
	from test_gpu_train3d import FixedDraws
	from find_amd import optim, synthetic
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	from find_amd.structures import Meshes, TexturesVertex
	from find_amd.trainer import Trainer
	opts = Opts(model_type='skinned', load_model=path)
	mwl = ModelWithLoss(opts=opts, device='cuda', train_size=3, val_size=2)
	m = _fit(mwl.model, seed=8)
	start = {n: p.detach().clone() for n, p in m.named_parameters()}
	gv, gf, _ = synthetic.gt_feet(3, n_verts=1002, seed=2)
	loader = [dict(mesh=Meshes(gv[[i]].contiguous(), gf, TexturesVertex(torch.full_like(gv[[i]], 0.5))), idx=torch.tensor([i], device='cuda')) for i in (0, 2, 1)]
	if stage == 'reg':
		op = optim.SGD(m.reg_params, lr=1e-5, momentum=0.9)
		kw = dict(chamf=True, gt_z_cutoff=0.01)
	else:
		op = optim.Adam(m.main_params, lr=1e-3, capturable=True)
		kw = dict(chamf=True, smooth=True)
	tr = Trainer([op], mwl, loader, [], opts, latent_vectors_train=m.latent_vectors_train, latent_vectors_val=m.latent_vectors_val, device='cuda', graph=graph)
	dr = _draws(1, gf.shape[0], m.template_faces.shape[1], seed=9)
	modes = []
	with FixedDraws(dr):
		for epoch in range(n_steps):
			tr.train_epoch(epoch, model_kwargs=dict(kw))
			modes.append(tr.last_mode)
	torch.cuda.synchronize()
	return tr, start, {n: p.detach().clone() for n, p in m.named_parameters()}, modes


@pytest.mark.parametrize('stage', ['reg', 'latent'])
def test_trainer_graph_replay_equals_eager_steps(stage, tmp_path):
	"""As tests/test_gpu_pca.py holds the PCA model: three captured-and-replayed steps against three eager ones."""
	from find_amd import synthetic
	path = str(tmp_path / 'm.npz')
	np.savez(path, **synthetic.skinned_model(V=1002, J=5, B=10, chain='tree', seed=1))
	tr_g, start, p_g, modes_g = _stage_run('auto', stage, path)
	tr_e, start_e, p_e, modes_e = _stage_run(False, stage, path)
	assert modes_g == ['graph'] * 3 and modes_e == ['eager'] * 3
	moving = ('reg_train.data',) if stage == 'reg' else ('betas_train.data', 'pose_train.data')
	for n in p_e:
		assert torch.equal(start[n], start_e[n]), n
		if n in moving:
			moved = (p_e[n] - start[n]).abs().max().item()
			assert moved > 0, n
			# the two loops differ by the float-atomic noise of the sampling backward, not by flips
			assert (p_g[n] - p_e[n]).abs().max().item() < 1e-3 * moved, (n, (p_g[n] - p_e[n]).abs().max().item(), moved)
		else:
			assert torch.equal(p_g[n], start[n]) and torch.equal(p_e[n], start[n]), n
	for epoch in range(3):
		a, b = tr_g.log[epoch]['train_loss'], tr_e.log[epoch]['train_loss']
		assert set(a) == set(b)
		for k in a:
			np.testing.assert_allclose(a[k], b[k], rtol=1e-4, atol=1e-7)


def test_eval_3d_and_2d_run_on_a_fitted_model(tmp_path):
	from tests.test_gpu_eval2d import _foot3d_val
	from tests.test_gpu_points import _foot3d_val_kp
	from find_amd import evaluate
	for sub in ('kp', '2d'):
		os.makedirs(str(tmp_path / sub))
	ds3 = _foot3d_val_kp(tmp_path / 'kp')
	m = _fit(_model(val_size=len(ds3)), seed=10)
	torch.manual_seed(3)
	res, extra = evaluate.eval_3d(m, ds3, [3, 17, 40, 101], samples=500, return_per_foot=True)
	assert list(res) == ['Keypoint (mm)', 'Chamf z-cutoff 0.07 (μm)', 'Chamf (μm)']
	assert all(isinstance(v, float) and np.isfinite(v) and v > 0 for v in res.values())
	assert extra['keypoint_mm'].shape == (len(ds3), 4) and torch.isfinite(extra['keypoint_mm']).all()
	ds2 = _foot3d_val(tmp_path / '2d')
	m2 = _fit(_model(val_size=len(ds2)), seed=11)
	res2, per2 = evaluate.eval_2d(m2, ds2, image_size=48, nviews=4, batch_size=2, feet_per_call=3, return_per_image=True)
	assert list(res2) == ['MSE', 'PSNR_A', 'PSNR_B', 'PSNR_C', 'IOU'] and all(np.isfinite(v) for v in res2.values())
	assert per2['IOU'].shape == (len(ds2) * 2,) and per2['IOU'].max() > 0.05   # the feet are in view


def test_init_registration_recovers_a_known_similarity():
	"""Scans made by a known similarity of the model's own template: the written rows of reg_val, through FN.register_points, land the template
	where the float64 reference ICP on the very same samples lands it -- tests/test_gpu_align.py's check of the same call, with its bounds --
	and within the sample spacing of the scan."""
	import math
	import align_ref as ref
	import test_gpu_align as TA
	from find_amd import align
	from find_amd import functional as FN
	from find_amd.losses import sample_points_from_meshes
	from find_amd.structures import Meshes
	N, S = 2, 500
	model = _model(train_size=4, val_size=N)
	tv1 = model.template_verts.data[0].cpu()
	f = model.template_faces.data[0]
	rng = np.random.default_rng(3)
	truths = [TA._truth(rng, 6, 4 * rng.normal(size=3), 1.02 + 0.02 * n) for n in range(N)]
	scans = torch.stack([torch.from_numpy(ref.apply(tv1.double().numpy(), *tr).astype(np.float32)) for tr in truths])
	batch = dict(mesh=Meshes(scans.cuda(), f), idx=torch.arange(N))
	before = model.reg.data.clone()
	sol = align.init_registration(model, batch, val=True, samples=S, generator=torch.Generator(device='cuda').manual_seed(5), max_iterations=TA.ITERS)
	assert torch.equal(model.reg_train.data, before)
	reg = model.reg_val.data.detach()
	assert torch.isfinite(reg).all() and (reg[:, 6] == reg[:, 7]).all() and (reg[:, 6] == reg[:, 8]).all()
	g = torch.Generator(device='cuda').manual_seed(5)
	tv = model.template_verts.data.expand(N, -1, -1).contiguous()
	xs = sample_points_from_meshes(Meshes(tv, f), num_samples=S, generator=g).cpu().numpy()
	ys = sample_points_from_meshes(batch['mesh'], num_samples=S, generator=g).cpu().numpy()
	kw = dict(max_iterations=TA.ITERS, trim=0.2, estimate_scale=True)
	r64 = [ref.icp(x, y, dtype=np.float64, **kw) for x, y in zip(xs, ys)]
	r32 = [ref.icp(x, y, dtype=np.float32, **kw) for x, y in zip(xs, ys)]
	landed = FN.register_points(tv, torch.zeros_like(tv), reg)
	tv64 = tv.double().cpu().numpy()
	TA._held('init_registration (skinned): the registered template', landed,
			 np.stack([ref.apply(tv64[n], r64[n]['R'], r64[n]['t'], r64[n]['s']) for n in range(N)]),
			 np.stack([ref.apply(tv64[n].astype(np.float32), r32[n]['R'], r32[n]['t'], r32[n]['s']) for n in range(N)]))
	tri = tv[0][f].double()
	area = 0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=-1).sum().item()
	spacing = math.sqrt(area / S)
	off = (landed - scans.cuda()).norm(dim=-1).max().item()
	start = (tv - scans.cuda()).norm(dim=-1).max().item()
	print(f'init_registration (skinned): within {off * 1e3:.2f} mm of the scan (identity: {start * 1e3:.2f} mm; sample spacing {spacing * 1e3:.2f} mm)')
	assert off < spacing < start
	assert torch.equal(align.reg_from_transform(sol.RTs), reg)
	# and the model's own decode, at its initial tables and the found registration, is that registered template: at zero pose the chain adds
	# and subtracts the rest joints (one rounding per level, three levels here), the blend and the two translations round five times more, and
	# the registration passes that on at a scale of about 1 -- under 16 ulp of the largest coordinate
	with torch.no_grad():
		res = model.get_meshes(poses=model.pose_val.data, betas=model.betas_val.data, trans=model.trans_val.data, reg=reg)
	assert (res['verts'] - landed).abs().max().item() <= 16 * _ulp(landed.abs().max().item())


def test_c_abi_error_codes():
	from find_amd import _lib
	L = _lib.lib()
	P = _lib.ptr
	N, V, J, B = 2, 100, 5, 3
	consts = {k: v.cuda() for k, v in _consts(V, J, B, 'tree', 'all', seed=1).items()}
	c = [P(consts[k]) for k in ('v_template', 'dirs', 'J0', 'JS', 'weights', 'parent')]
	pose, betas, trans, d_out = (t.cuda() for t in _inputs(N, V, J, B, seed=1))
	out, d_pose, d_betas, d_trans = (torch.empty_like(t) for t in (d_out, pose, betas, trans))
	sz = (V, J, B, 4 * J)
	need_f, need_b = L.find_skin_fwd_ws_bytes(N, *sz), L.find_skin_bwd_ws_bytes(N, *sz)
	assert 0 < need_f < need_b and L.find_skin_fwd_ws_bytes(N, V, J, B, 4 * J + 1) == -1 and L.find_skin_bwd_ws_bytes(N, V, 129, B, 4 * 129) == -1
	ws = torch.empty(need_b, dtype=torch.uint8, device='cuda')
	fwd = lambda c=c, sz=sz, pose=P(pose), out=P(out), ws=P(ws), nb=need_f, n=N: L.find_skin_fwd(*c, *sz, pose, P(betas), P(trans), n, out, None, ws, nb, None)
	bwd = lambda c=c, sz=sz, g=P(d_out), dp=P(d_pose), ws=P(ws), nb=need_b, n=N: L.find_skin_bwd(*c, *sz, P(pose), P(betas), g, n, dp, P(d_betas), P(d_trans), ws, nb, None)
	for i in range(6):
		assert fwd(c=c[:i] + [None] + c[i + 1:]) == -1 and b'NULL' in L.find_last_error()
		assert bwd(c=c[:i] + [None] + c[i + 1:]) == -1 and b'NULL' in L.find_last_error()
	assert fwd(pose=None) == -1 and fwd(out=None) == -1 and fwd(ws=None) == -1 and b'NULL' in L.find_last_error()
	assert bwd(g=None) == -1 and bwd(dp=None) == -1 and bwd(ws=None) == -1 and b'NULL' in L.find_last_error()
	for bad in ((V, J, B, 4 * J - 1), (V, J, 0, 4 * J), (0, J, B, 4 * J), (V, 0, B, 0), (V, 129, B, 516), (V, J, 3000, 4 * J)):
		assert fwd(sz=bad) == -1 and b'bad sizes' in L.find_last_error(), bad
		assert bwd(sz=bad) == -1 and b'bad sizes' in L.find_last_error(), bad
	assert fwd(n=0) == -1 and bwd(n=0) == -1
	assert fwd(nb=need_f - 4) == -2 and b'workspace' in L.find_last_error()
	assert bwd(nb=need_b - 4) == -2 and b'workspace' in L.find_last_error()
	assert fwd() == 0 and bwd() == 0
	torch.cuda.synchronize()
	ref = skin_ref.with_grads({k: v.cpu() for k, v in consts.items()}, pose.cpu(), betas.cpu(), trans.cpu(), d_out.cpu(), torch.float64)
	for got, want in zip((out, d_pose, d_betas, d_trans), ref):
		assert torch.allclose(got.double().cpu(), want, rtol=1e-4, atol=1e-5 * want.abs().max().item())


def test_print_the_worst_ratios():
	"""Not a check of its own: the worst e_hip / max(e32, ulp) of the comparisons above, per quantity, for the test log."""
	print('worst e_hip / max(e32, 1 ulp) per quantity:', {k: round(v, 3) for k, v in WORST.items()})
