#!/usr/bin/env python3
"""Golden vectors for the linear PCA baseline (model_type='pca').

Runs ONLY in the build container (needs the reference checkout, as make_golden_composition.py does).  Executed for real, as written:

  * src/model/model.py:610-637   PCAModel.load_from_mat / load: pcaMean, 1-based mesh, pcaCoefs (3V, B) -> pca_coefs (V, B, 3), pcaVar
  * src/model/model.py:573-608   PCAModel.get_meshes (with and without reg) / get_meshes_from_batch
  * src/model/model.py:1001-1163 ModelWithLoss.forward with opts.model_type = 'pca' and opts.load_model = the .mat file, for the fitting
                                 stage's chamf + smooth and for the registration stage's chamf with gt_z_cutoff

The PyTorch3D names are make_golden_composition.py's oracle-backed stand-ins (imported from there); the sampler draws are recorded and
stored: they are inputs of the fixture.  The .mat file itself is synthetic: pcaMean is the 128-vertex lat-long ellipsoid of that script,
B = 7 random components.

Output (data only): tests/golden/pca.npz -- the .mat contents, the tensors load_from_mat produced, get_meshes' outputs, per case the flags,
draws, loss dict, total and the gradients of the shapevec / reg tables (fp32, and float64 from the same code on double tensors).
Checked by tests/test_pca_host.py (float64 restatement, CPU) and tests/test_gpu_pca.py (find_amd on the GPU).

Usage:  python tests/golden/make_golden_pca.py"""
import copy
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
N_B = 7
N_FEET = 3


def make_mat(path):
	"""A small PCA model in the layout of the Foot3D .mat file: pcaMean (1, 3V), mesh (F, 3) 1-based, pcaCoefs (3V, B) with row 3v + c,
	pcaVar (B, 1).  Returns the arrays written."""
	import numpy as np
	from scipy.io import savemat
	from find_amd import synthetic
	from make_golden_composition import GRID_TEMPLATE
	tv, tf = synthetic.ellipsoid_mesh(*GRID_TEMPLATE)
	rng = np.random.RandomState(11)
	V = tv.shape[0]
	data = dict(pcaMean=tv.numpy().astype(np.float64).reshape(1, -1),
				mesh=(tf.numpy().astype(np.float64) + 1),
				pcaCoefs=rng.normal(0, 0.004, (3 * V, N_B)) * (1.0 / (1 + np.arange(N_B)))[None],
				pcaVar=np.sort(rng.uniform(0.1, 2.0, (N_B, 1)), axis=0)[::-1].copy())
	savemat(path, data)
	return data


def main():
	import numpy as np
	import torch
	torch.set_num_threads(4)
	from make_golden_composition import GRID_SCAN, install_pytorch3d_stand_ins
	draws, replay = [], []
	P3D = install_pytorch3d_stand_ins(draws, replay)
	import make_golden_mlp as G
	G.import_reference()
	import src.model.model as ref_model
	from src.train.opts import Opts
	from src.train.trainer import sample_latent_vectors
	from find_amd import synthetic

	out = {}
	tmp = tempfile.mkdtemp()
	mat = os.path.join(tmp, 'pca.mat')
	for k, v in make_mat(mat).items():
		out['mat/' + k] = v

	# ------------------------------------------------------------------ load_from_mat, get_meshes
	m = ref_model.PCAModel.load(mat, device='cpu', train_size=N_FEET, val_size=N_FEET)
	for k, v in m.state_dict().items():
		out['loaded/' + k] = v.detach().numpy().copy()
	out['loaded/keys'] = np.array(list(m.state_dict()), dtype=str)
	out['loaded/latent_train'] = np.array([v.name for v in m.latent_vectors_train], dtype=str)
	out['loaded/latent_val'] = np.array([v.name for v in m.latent_vectors_val], dtype=str)
	g = torch.Generator().manual_seed(77)
	with torch.no_grad():
		for vec in m.latent_vectors_train + m.latent_vectors_val:
			t = vec.data
			if vec.name.startswith('reg'):
				t.copy_(torch.cat([torch.randn(t.shape[0], 3, generator=g) * 0.004, torch.randn(t.shape[0], 3, generator=g) * 0.05, 1 + torch.randn(t.shape[0], 3, generator=g) * 0.03], 1))
			else:
				t.copy_(torch.randn(t.shape, generator=g))
	for k, v in m.state_dict().items():
		out['sd/' + k] = v.detach().numpy().copy()
	sv, rg = m.shapevec.data.detach(), m.reg.data.detach()
	for tag, r in (('reg', rg), ('noreg', None)):
		res = m.get_meshes(shapevec=sv, reg=r)
		out[f'get_meshes/{tag}/offsets'] = res['offsets'].detach().numpy().copy()
		out[f'get_meshes/{tag}/verts'] = res['verts'].detach().numpy().copy()
		out[f'get_meshes/{tag}/colours'] = res['meshes'].textures.verts_features_padded().numpy().copy()

	# ------------------------------------------------------------------ ModelWithLoss with model_type='pca'
	opts = Opts()
	opts.model_type, opts.load_model = 'pca', mat
	mwl = ref_model.ModelWithLoss(opts=opts, device='cpu', train_size=N_FEET, val_size=N_FEET)
	mwl.model.load_state_dict(m.state_dict())
	mm = mwl.model
	mm.configure_params()   # (upstream leaves the groups of a loaded model as they were; nothing below reads them)
	rng = np.random.RandomState(3)
	base, gf = synthetic.ellipsoid_mesh(*GRID_SCAN, axes=(1.0, 1.0, 1.0))
	base = base.numpy()
	gv = []
	for _ in range(N_FEET):
		ax = np.array([0.12, 0.045, 0.04]) * rng.uniform(0.9, 1.1, 3)
		r = np.ones(len(base))
		for _k in range(3):
			r = r + (0.003 / 0.04) * np.sin(base @ rng.uniform(1.0, 3.0, 3) + rng.uniform(0, 2 * np.pi))
		gv.append((base * r[:, None] * ax[None]).astype(np.float32))
	gv = torch.from_numpy(np.stack(gv))
	gc = torch.full_like(gv, 0.5)
	out['gt/verts'], out['gt/faces'] = gv.numpy(), gf.numpy()

	def batch_of(idx, model, dtype=torch.float32):
		sel = torch.tensor(idx)
		b = dict(mesh=P3D.Meshes(gv[sel].to(dtype), gf[None].expand(len(idx), -1, -1), P3D.TexturesVertex(gc[sel].to(dtype))), idx=sel)
		b.update(sample_latent_vectors(b, model.latent_vectors_train))
		return b

	cases = {
		'fit': dict(idx=[0, 1, 2], flags=dict(chamf=True, smooth=True)),          # the latent stage: chamf + smooth on the shape codes
		'reg': dict(idx=[2, 0], flags=dict(chamf=True, gt_z_cutoff=0.01)),       # the registration stage with a GT cut-off
	}
	out['cases'] = np.array(sorted(cases))
	for name, c in cases.items():
		batch = batch_of(c['idx'], mm)
		# redrawn until no Chamfer query is near a nearest-neighbour tie (make_golden_composition.py explains why)
		for attempt in range(200):
			for p in mwl.parameters():
				p.grad = None
			del draws[:]
			torch.manual_seed(300 + len(name) + 1000 * attempt)
			loss, losses = mwl(batch, 0, opts, **c['flags'])
			a, bb = draws[1][3].double(), draws[0][3].double()
			gap = 1.0
			for q, t in ((a, bb), (bb, a)):
				two = torch.topk(((q[:, :, None, :] - t[:, None, :, :]) ** 2).sum(-1), 2, dim=-1, largest=False).values
				gap = min(gap, float(((two[..., 1] - two[..., 0]) / two[..., 1]).min()))
			if gap > 3e-6:
				break
		else:
			raise RuntimeError(f'case {name}: no tie-free draws found')
		out[f'case/{name}/nn_min_relative_gap'] = np.float64(gap)
		out[f'case/{name}/idx'] = np.array(c['idx'], np.int64)
		out[f'case/{name}/flags'] = np.array([f'{k}={v}' for k, v in sorted(c['flags'].items())])
		out[f'case/{name}/loss_keys'] = np.array(list(losses), dtype=str)
		for k, v in losses.items():
			out[f'case/{name}/losses/{k}'] = np.float64(v.item())
		out[f'case/{name}/n_draws'] = np.int64(len(draws))
		for i, (ns, fi, uv, _pts) in enumerate(draws):
			out[f'case/{name}/draw/{i}/face_idx'] = fi.numpy().astype(np.int32)
			out[f'case/{name}/draw/{i}/uv'] = uv.numpy()
		out[f'case/{name}/loss'] = np.float64(loss.item())
		loss.backward()
		for k in ('shapevec.data', 'reg.data'):
			out[f'case/{name}/grad/{k}'] = dict(mwl.model.named_parameters())[k].grad.detach().numpy().copy()
		# the same call in float64 on the same draws (the yardstick the GPU test compares gradients with, as in make_golden_composition.py)
		mwl64 = copy.deepcopy(mwl).double()
		for p in mwl64.parameters():
			p.grad = None
		m64 = mwl64.model
		m64.template_mesh = P3D.Meshes(verts=m64.template_verts, faces=m64.template_faces)
		m64.latent_vectors_train = [m64.reg, m64.shapevec]
		replay.extend(draws)
		loss64, losses64 = mwl64(batch_of(c['idx'], m64, dtype=torch.float64), 0, opts, **c['flags'])
		assert not replay and list(losses64) == list(losses)
		out[f'case/{name}/loss64'] = np.float64(loss64.item())
		for k, v in losses64.items():
			out[f'case/{name}/losses64/{k}'] = np.float64(v.item())
		loss64.backward()
		for k in ('shapevec.data', 'reg.data'):
			g64 = dict(m64.named_parameters())[k].grad.detach().numpy()
			out[f'case/{name}/grad64/{k}'] = g64.copy()
			g32 = out[f'case/{name}/grad/{k}']
			out[f'case/{name}/ref_fp32_error/{k}'] = np.float64(np.abs(g32 - g64).max() / max(1e-3, np.abs(g64).max()))
		print(name, 'loss', float(loss), {k: round(float(v), 7) for k, v in losses.items()}, 'draw calls', [d[0] for d in draws], 'gap %.1e' % gap)
	np.savez_compressed(os.path.join(HERE, 'pca.npz'), **out)
	print('pca.npz:', len(out), 'arrays,', os.path.getsize(os.path.join(HERE, 'pca.npz')) // 1024, 'KB')


if __name__ == '__main__':
	main()
