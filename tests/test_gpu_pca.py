"""The PCA baseline on the GPU: find_pca_fwd / find_pca_bwd against float64 (odd B, vertex tails, more than 32 feet) and from run to run,
find_amd.ModelWithLoss(model_type='pca') against the reference's own results (tests/golden/pca.npz, tests/golden/make_golden_pca.py),
checkpoints in both formats, the registration and latent stages through Trainer (graph replay against eager steps), eval_3d_metrics and
eval_2d on a fitted PCA model, and the C-ABI's error codes."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
TOL = 1e-4


def _decode_inputs(N, V, B, seed):
	g = torch.Generator().manual_seed(seed)
	coefs = (torch.randn(V, B, 3, generator=g) * 0.01).cuda()
	sv = torch.randn(N, B, generator=g).cuda().requires_grad_(True)
	dout = torch.randn(N, V, 3, generator=g).cuda()
	return coefs, sv, dout


@pytest.mark.parametrize('N,V,B', [(1, 98, 1), (3, 6890, 7), (16, 6890, 100), (33, 50002, 37)])
def test_decode_matches_float64(N, V, B):
	from find_amd import functional as FN
	coefs, sv, dout = _decode_inputs(N, V, B, seed=N + V + B)
	off = FN.pca_offsets(coefs, sv)
	(d_sv,) = torch.autograd.grad(off, sv, dout)
	off64 = torch.einsum('vbc,nb->nvc', coefs.double(), sv.detach().double())
	d64 = torch.einsum('nvc,vbc->nb', dout.double(), coefs.double())
	err = (off.double() - off64).abs().max().item() / off64.abs().max().item()
	derr = (d_sv.double() - d64).abs().max().item() / d64.abs().max().item()
	assert err < 1e-5, err
	assert derr < 1e-4, derr
	# repeated calls are bit-identical (no atomics; the split depends on the sizes only)
	for _ in range(2):
		off2 = FN.pca_offsets(coefs, sv)
		(d2,) = torch.autograd.grad(off2, sv, dout)
		assert torch.equal(off2, off) and torch.equal(d2, d_sv)


def _write_mat(z, tmp_path):
	sys.path.insert(0, HERE)
	from test_pca_host import write_mat
	return write_mat(z, str(tmp_path / 'pca.mat'))


def _fixture_mwl(z, tmp_path):
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	opts = Opts(model_type='pca', load_model=_write_mat(z, tmp_path))
	mwl = ModelWithLoss(opts=opts, device='cuda', train_size=3, val_size=3)
	mwl.model.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}, strict=True)
	return mwl, opts


def test_model_with_loss_equals_the_reference(tmp_path):
	sys.path.insert(0, HERE)
	from test_gpu_train3d import FixedDraws
	from find_amd.structures import Meshes, TexturesVertex
	from find_amd.train_utils import sample_latent_vectors
	z = np.load(os.path.join(GOLD, 'pca.npz'))
	mwl, opts = _fixture_mwl(z, tmp_path)
	m = mwl.model
	dev = torch.device('cuda')
	gv, gf = (torch.from_numpy(z[f'gt/{k}']).to(dev) for k in ('verts', 'faces'))
	# get_meshes with and without the registration
	for tag, reg in (('reg', m.reg.data), ('noreg', None)):
		with torch.no_grad():
			res = m.get_meshes(shapevec=m.shapevec.data, reg=reg)
		for k in ('offsets', 'verts'):
			want = z[f'get_meshes/{tag}/{k}']
			assert np.abs(res[k].cpu().numpy() - want).max() < 1e-6 * max(1e-3, np.abs(want).max()), (tag, k)
		assert torch.all(res['meshes'].textures.verts_features_padded() == 0.5)
	params = dict(m.named_parameters())
	for name in z['cases']:
		flags = {}
		for f in z[f'case/{name}/flags']:
			k, v = str(f).split('=')
			flags[k] = {'True': True, 'False': False}.get(v, None if v == 'None' else v)
			if k == 'gt_z_cutoff':
				flags[k] = float(v)
		idx = [int(i) for i in z[f'case/{name}/idx']]
		b = dict(mesh=Meshes(gv[idx].contiguous(), gf, TexturesVertex(torch.full_like(gv[idx], 0.5))), idx=torch.tensor(idx, device=dev))
		b.update(sample_latent_vectors(b, m.latent_vectors_train))
		dr = [(torch.from_numpy(z[f'case/{name}/draw/{i}/face_idx']).to(dev), torch.from_numpy(z[f'case/{name}/draw/{i}/uv']).to(dev)) for i in range(2)]
		for p in mwl.parameters():
			p.grad = None
		with FixedDraws([dr[0], dr[1], None]):
			loss, losses = mwl(b, 0, opts, **flags)
		assert list(losses) == [str(s) for s in z[f'case/{name}/loss_keys']]
		for k, v in losses.items():
			want = float(z[f'case/{name}/losses/{k}'])
			assert abs(v.item() - want) < TOL * max(1.0, abs(want)), (name, k, v.item(), want)
		assert abs(loss.item() - float(z[f'case/{name}/loss'])) < TOL * max(1.0, abs(loss.item()))
		loss.backward()
		for k in ('shapevec.data', 'reg.data'):
			want = z[f'case/{name}/grad64/{k}']
			got = params[k].grad.detach().cpu().numpy().astype(np.float64)
			err = np.abs(got - want).max() / max(1e-3, np.abs(want).max())
			assert err < max(TOL, 2.0 * float(z[f'case/{name}/ref_fp32_error/{k}'])), (name, k, err)
		assert params['pca_coefs'].grad is None


def test_checkpoints_of_both_formats_give_identical_forwards(tmp_path):
	from find_amd.model import PCAModel
	z = np.load(os.path.join(GOLD, 'pca.npz'))
	sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
	torch.save({'state_dict': sd, 'params': dict(train_size=3, val_size=3)}, str(tmp_path / 'ref.pth'))
	a = PCAModel.load(str(tmp_path / 'ref.pth'), device='cuda')
	a.save_model(str(tmp_path), 'port')
	b = PCAModel.load(str(tmp_path / 'port.pth'), device='cuda')
	saved = torch.load(str(tmp_path / 'port.pth'), map_location='cpu', weights_only=False)
	assert list(saved['state_dict']) == [str(k) for k in z['loaded/keys']] and saved['params'] == dict(train_size=3, val_size=3)
	with torch.no_grad():
		ra = a.get_meshes(shapevec=a.shapevec.data, reg=a.reg.data)
		rb = b.get_meshes(shapevec=b.shapevec.data, reg=b.reg.data)
	assert torch.equal(ra['verts'], rb['verts']) and torch.equal(ra['offsets'], rb['offsets'])
	want = z['get_meshes/reg/verts']
	assert np.abs(ra['verts'].cpu().numpy() - want).max() < 1e-6 * np.abs(want).max()


def _stage_run(graph, stage, tmp_path, z, n_steps=3):
	from test_gpu_train3d import FixedDraws
	from find_amd import optim
	from find_amd.structures import Meshes, TexturesVertex
	from find_amd.trainer import Trainer
	mwl, opts = _fixture_mwl(z, tmp_path)
	m = mwl.model
	dev = torch.device('cuda')
	gv, gf = (torch.from_numpy(z[f'gt/{k}']).to(dev) for k in ('verts', 'faces'))
	loader = [dict(mesh=Meshes(gv[[i]].contiguous(), gf, TexturesVertex(torch.full_like(gv[[i]], 0.5))), idx=torch.tensor([i], device=dev)) for i in (0, 2, 1)]
	if stage == 'reg':
		op = optim.SGD(m.reg_params, lr=1e-5, momentum=0.9)
		kw = dict(chamf=True, gt_z_cutoff=0.01)
	else:
		op = optim.Adam(m.main_params, lr=1e-3, capturable=True)
		kw = dict(chamf=True, smooth=True)
	tr = Trainer([op], mwl, loader, [], opts, latent_vectors_train=m.latent_vectors_train, latent_vectors_val=m.latent_vectors_val, device='cuda', graph=graph)
	dr = [(torch.from_numpy(z[f'case/reg/draw/{i}/face_idx'][:1]).to(dev), torch.from_numpy(z[f'case/reg/draw/{i}/uv'][:1]).to(dev)) for i in range(2)]
	modes = []
	with FixedDraws([dr[0], dr[1], None]):
		for epoch in range(n_steps):
			tr.train_epoch(epoch, model_kwargs=dict(kw))
			modes.append(tr.last_mode)
	torch.cuda.synchronize()
	return tr, {n: p.detach().clone() for n, p in m.named_parameters()}, modes


@pytest.mark.parametrize('stage', ['reg', 'latent'])
def test_trainer_graph_replay_equals_eager_steps(stage, tmp_path):
	sys.path.insert(0, HERE)
	z = np.load(os.path.join(GOLD, 'pca.npz'))
	start = {k[3:]: torch.from_numpy(z[k]).cuda() for k in z.files if k.startswith('sd/')}
	tr_g, p_g, modes_g = _stage_run('auto', stage, tmp_path, z)
	tr_e, p_e, modes_e = _stage_run(False, stage, tmp_path, z)
	assert modes_g == ['graph'] * 3 and modes_e == ['eager'] * 3
	moving = 'reg.data' if stage == 'reg' else 'shapevec.data'
	for n in p_e:
		if n == moving:
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


def test_eval_3d_and_2d_on_a_fitted_pca_model(tmp_path):
	from tests.test_eval2d_host import eval_2d_group64
	from tests.test_gpu_eval2d import _foot3d_val
	from find_amd import evaluate
	from find_amd.dataset import BatchCollator
	from find_amd.eval_metrics import eval_3d_metrics
	from find_amd.model import PCAModel
	from find_amd.renderer import FootRenderer
	from find_amd.structures import Meshes
	z = np.load(os.path.join(GOLD, 'pca.npz'))
	ds = _foot3d_val(tmp_path)
	m = PCAModel.load(_write_mat(z, tmp_path), device='cuda', train_size=1, val_size=len(ds))
	g = torch.Generator().manual_seed(8)
	with torch.no_grad():   # a fitted-looking model: shape codes and registrations of its own
		m.shapevec_val.data.copy_(torch.randn(len(ds), m.shapevec_val.data.shape[1], generator=g).cuda())
		m.reg_val.data[:, 0:3] = torch.randn(len(ds), 3, generator=g).cuda() * 0.01
		m.reg_val.data[:, 3:6] = torch.randn(len(ds), 3, generator=g).cuda() * 0.1
		m.reg_val.data[:, 6:9] = 1.0
	# 3-D: eval_3d_metrics on the registered predictions against the scans, equal to a float64 torch composition of the same samples
	collate = BatchCollator(device='cuda').collate_batches
	batch = collate([ds[i] for i in range(2)])
	with torch.no_grad():
		res = m.get_meshes(shapevec=m.shapevec_val.data[:2], reg=m.reg_val.data[:2])
	kp = np.array([3, 17, 40])
	gt_kps = res['verts'][:, kp] + 0.001
	S = 2000
	gts = Meshes(batch['mesh'].verts_padded(), batch['mesh'].faces_padded())
	draws_g = (torch.randint(0, int(gts.num_faces_per_mesh().min()), (2, S), generator=g, dtype=torch.int32).cuda(), torch.rand(2, S, 2, generator=g).cuda())
	draws_p = (torch.randint(0, res['meshes'].faces_shared().shape[0], (2, S), generator=g, dtype=torch.int32).cuda(), torch.rand(2, S, 2, generator=g).cuda())
	out = eval_3d_metrics(res['meshes'], gts, pred_verts=res['verts'], template_kp_idxs=kp, gt_kps=gt_kps, samples=S, draws_gt=draws_g, draws_pred=draws_p)

	def samples64(verts, faces, draws):
		fi, uv = draws
		v = verts.double()
		tri = torch.stack([torch.stack([v[n][faces[n][fi[n].long()][:, j].long()] for j in range(3)], 1) for n in range(len(v))])
		su = uv[..., 0:1].double().sqrt()
		return (1 - su) * tri[:, :, 0] + su * (1 - uv[..., 1:2].double()) * tri[:, :, 1] + su * uv[..., 1:2].double() * tri[:, :, 2]

	pg = samples64(gts.verts_padded(), gts.faces_padded(), draws_g)
	pp = samples64(res['verts'], res['meshes'].faces_padded(), draws_p)
	d = ((pg[:, :, None] - pp[:, None]) ** 2).sum(-1)
	chamf64 = (d.min(2).values.mean(1) + d.min(1).values.mean(1)).mean() * 1e6
	assert abs(out['Chamf (μm)'].item() - chamf64.item()) < 1e-4 * chamf64.item()
	assert abs(out['Keypoint (mm)'].item() - np.sqrt(3) * 1e-3 * 1e3) < 1e-4
	# 2-D: eval_2d (renders of several feet per call) against the reference's loop, one foot and one group of views at a time
	size, nviews, bs = 48, 4, 2
	res2, per2 = evaluate.eval_2d(m, ds, image_size=size, nviews=nviews, batch_size=bs, feet_per_call=3, return_per_image=True)
	rdr = FootRenderer(image_size=size, device='cuda')
	R, T = rdr.linspace_views(nviews=nviews, dist=0.3, elev_min=-90, elev_max=90)
	ref = {k: [] for k in res2}
	with torch.no_grad():
		for i in range(len(ds)):
			b = collate([ds[i]])
			b.update({vec.name: vec.data[b['idx']] for vec in m.latent_vectors_val})
			o = m.get_meshes_from_batch(b, is_train=False)
			for j in range(nviews // bs):
				Rb, Tb = R[j * bs:(j + 1) * bs], T[j * bs:(j + 1) * bs]
				gt = rdr(b['mesh'], Rb, Tb, return_mask=True, mask_out_faces=True, return_mask_out_masks=True)
				pred = rdr(o['meshes'], Rb, Tb, return_mask=True)
				for k, v in eval_2d_group64(gt['image'], gt['mask'], gt['mask_out_masks'], pred['image'], pred['mask']).items():
					ref[k].append(v.item())
	assert max(ref['IOU']) > 0.05   # the feet are in view
	for k in res2:
		assert np.allclose(per2[k].cpu().numpy(), ref[k], rtol=1e-5, atol=1e-7, equal_nan=True), k


def test_c_abi_error_codes():
	from find_amd import _lib
	L = _lib.lib()
	P = _lib.ptr
	coefs, sv, dout = _decode_inputs(2, 100, 5, seed=1)
	sv = sv.detach()
	off = torch.empty(2, 100, 3, device='cuda')
	d_sv = torch.empty(2, 5, device='cuda')
	need = L.find_pca_bwd_ws_bytes(2, 100, 5)
	assert need > 0 and L.find_pca_bwd_ws_bytes(2, 100, 0) == -1
	ws = torch.empty(need, dtype=torch.uint8, device='cuda')
	assert L.find_pca_fwd(None, 100, 5, P(sv), 2, P(off), None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_pca_fwd(P(coefs), 100, 5, P(sv), 2, None, None) == -1
	assert L.find_pca_fwd(P(coefs), 100, 0, P(sv), 2, P(off), None) == -1 and b'bad sizes' in L.find_last_error()
	assert L.find_pca_fwd(P(coefs), 100, -3, P(sv), 2, P(off), None) == -1
	assert L.find_pca_fwd(P(coefs), 0, 5, P(sv), 2, P(off), None) == -1
	assert L.find_pca_fwd(P(coefs), 100, 5, P(sv), 0, P(off), None) == -1
	assert L.find_pca_bwd(P(coefs), 100, 5, P(dout), 2, P(d_sv), None, need, None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_pca_bwd(P(coefs), 100, 0, P(dout), 2, P(d_sv), P(ws), need, None) == -1
	assert L.find_pca_bwd(P(coefs), 100, 5, P(dout), 2, P(d_sv), P(ws), need - 4, None) == -2 and b'workspace' in L.find_last_error()
	assert L.find_pca_fwd(P(coefs), 100, 5, P(sv), 2, P(off), None) == 0
	assert L.find_pca_bwd(P(coefs), 100, 5, P(dout), 2, P(d_sv), P(ws), need, None) == 0
	torch.cuda.synchronize()
	assert torch.allclose(off, torch.einsum('vbc,nb->nvc', coefs, sv), rtol=1e-5, atol=1e-7)
	assert torch.allclose(d_sv, torch.einsum('nvc,vbc->nb', dout, coefs), rtol=1e-4, atol=1e-6)
