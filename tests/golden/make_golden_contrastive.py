#!/usr/bin/env python3
"""Golden vectors for the contrastive pose loss (reference src/model/losses.py:305-333, ContrastiveLoss; applied in
ModelWithLoss.forward, src/model/model.py:1042-1049) -> contrastive.npz.

Runs ONLY in the build container (needs the reference checkout).  Executed for real, as written:

  * ContrastiveLoss.forward(vecs, codes) under np.random.seed(seed): the pairs its np.random.shuffle drew (recorded by wrapping the
    shuffle), numpy's generator state right after the draw, the loss and d loss / d vecs.  vecs fp32, codes float64 (what default_collate
    makes of the dataset's np.zeros pose codes: upstream's loss is float64).  Cases: N = 2, 3, 5, 16, 24 (more than 256 pairs); K = 256
    and odd K; y = <code_a, code_b> in {-1, 0, 1, 2}; the hinge max(0.5 - d^2, 0) active and inactive, every drawn pair more than 1e-4
    from its boundary except in the case built on it (d^2 = 0.5 in exact arithmetic); a duplicated row (d = 0).
  * ModelWithLoss.forward(batch of 3 scans, chamf=True, smooth=True, cont_pose=True), with the weights, latent tables and scans of
    composition.npz and its PyTorch3D stand-ins (make_golden_composition.install_pytorch3d_stand_ins): the losses dict in its key order,
    the total, the pairs, the sampler's draws (replayed on the GPU), and the same call without cont_pose."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

MARGIN_GAP = 1e-4


def _vecs(rng, N, K, scale_lo, scale_hi):
	s = rng.uniform(scale_lo, scale_hi, (N, 1)) / (K ** 0.5)
	return (rng.standard_normal((N, K)) * s).astype('float32')


def _codes(rng, N, C=8):
	"""Pose-code-like rows: entries -1 / 0 / 1 on a few slots, so that <code_a, code_b> takes -1, 0, 1 and 2."""
	import numpy as np
	c = np.zeros((N, C))
	for i in range(N):
		for j in rng.choice(3, size=rng.integers(1, 3), replace=False):
			c[i, j] = rng.choice([-1.0, 1.0])
	return c


def main():
	import numpy as np
	import torch
	torch.set_num_threads(4)
	draws, replay = [], []
	from make_golden_composition import install_pytorch3d_stand_ins
	P3D = install_pytorch3d_stand_ins(draws, replay)
	import make_golden_mlp as G
	G.import_reference()
	import src.model.losses as ref_losses
	import src.model.model as ref_model
	from src.train.opts import Opts
	from src.train.trainer import sample_latent_vectors

	shuffled = []
	real_shuffle = np.random.shuffle

	def recording_shuffle(x):
		real_shuffle(x)
		shuffled.append([tuple(int(i) for i in p) for p in x])
	ref_losses.np.random.shuffle = recording_shuffle   # (losses.py calls np.random.shuffle: the module attribute, looked up per call)

	out = {}
	crit = ref_losses.ContrastiveLoss()
	# name -> (N, K, npairs, vec scales (low, high), special)
	cases = {
		'n2_k256': (2, 256, 10, (0.1, 0.4), None),
		'n3_k256': (3, 256, 10, (0.2, 0.8), None),
		'n5_k37': (5, 37, 10, (0.1, 1.0), None),
		'n16_k256': (16, 256, 10, (0.1, 1.0), None),
		'n16_k5_all': (16, 5, 500, (0.1, 1.0), None),
		'n24_k3_chunked': (24, 3, 1000, (0.1, 1.0), None),
		'n3_dup': (3, 256, 10, (0.2, 0.8), 'dup'),
		'n2_boundary': (2, 2, 10, None, 'boundary'),
	}
	ys = set()
	for ci, (name, (N, K, npairs, scales, special)) in enumerate(cases.items()):
		for attempt in range(500):
			rng = np.random.default_rng(1000 * ci + attempt)
			codes = _codes(rng, N)
			if special == 'boundary':
				vecs = np.array([[0.0, 0.0], [0.5, 0.5]], np.float32)   # d^2 = 0.5 exactly = margin
				codes[1] = codes[0]
				codes[1, 7] = 1.0   # keep y = <c0, c1> of c0's norm
			else:
				vecs = _vecs(rng, N, K, *scales)
			if special == 'dup':
				vecs[2] = vecs[0]
			seed = 7 + 31 * ci + attempt
			np.random.seed(seed)
			del shuffled[:]
			v = torch.from_numpy(vecs).requires_grad_(True)
			c = torch.from_numpy(codes)
			loss = crit(v, c, npairs=npairs)
			state = np.random.get_state()
			P = min(npairs, N * (N - 1) // 2)
			pairs = np.array(shuffled[0][:P], np.int32).reshape(-1, 2)
			d2 = ((vecs[pairs[:, 0]].astype(np.float64) - vecs[pairs[:, 1]]) ** 2).sum(1)
			if special == 'boundary':
				break
			if np.abs(d2 - 0.5).min() <= MARGIN_GAP:
				continue
			if special == 'dup' and not any(set(p) == {0, 2} for p in pairs.tolist()):
				continue
			break
		else:
			raise RuntimeError(f'case {name}: no admissible draw')
		loss.backward()
		y = (codes[pairs[:, 0]] * codes[pairs[:, 1]]).sum(1)
		ys |= set(y.tolist())
		out[f'case/{name}/vecs'] = vecs
		out[f'case/{name}/codes'] = codes
		out[f'case/{name}/npairs'] = np.int64(npairs)
		out[f'case/{name}/seed'] = np.int64(seed)
		out[f'case/{name}/pairs'] = pairs
		out[f'case/{name}/state_keys'] = state[1]
		out[f'case/{name}/state_pos'] = np.int64(state[2])
		out[f'case/{name}/loss'] = np.float64(loss.item())
		out[f'case/{name}/loss_dtype'] = np.array(str(loss.dtype))
		out[f'case/{name}/d_vecs'] = v.grad.numpy().copy()
		out[f'case/{name}/hinge_active'] = np.bool_((d2 < 0.5).any())
		out[f'case/{name}/hinge_inactive'] = np.bool_((d2 > 0.5).any())
		print(name, 'P', P, 'loss', loss.item(), 'y', sorted(set(y.tolist())), 'd2', d2.min(), d2.max())
	assert {-1.0, 0.0, 1.0, 2.0} <= ys, ys
	out['cases'] = np.array(list(cases))

	# ------------------------------------------------------------------ ModelWithLoss.forward with cont_pose, on composition.npz's model
	z = np.load(os.path.join(HERE, 'composition.npz'))
	lab = {k[len('labels/'):]: [str(s) for s in z[k]] for k in z.files if k.startswith('labels/')}
	opts = Opts()
	for k, v in dict(chamf_loss=True, smooth_loss=True, use_pose_code=True, use_latent_labels=True, cont_pose_loss=True).items():
		setattr(opts, k, v)
	mwl = ref_model.ModelWithLoss(opts=opts, device='cpu', use_shapevec=True, use_texvec=True, use_posevec=True, train_size=3, val_size=3,
								  shapevec_size=100, texvec_size=100, posevec_size=100, template_mesh_loc=None, latent_labels=lab)
	m = mwl.model
	m.template_verts = torch.nn.Parameter(torch.from_numpy(z['sd/template_verts']), requires_grad=False)
	m.template_faces = torch.nn.Parameter(torch.from_numpy(z['sd/template_faces']), requires_grad=False)
	m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}, strict=True)
	m.template_mesh = P3D.Meshes(verts=m.template_verts, faces=m.template_faces)
	gv, gf, gc = (torch.from_numpy(z[f'gt/{k}']) for k in ('verts', 'faces', 'colours'))
	feet, names = [str(s) for s in z['batch/feet']], [str(s) for s in z['batch/names']]
	idx = [0, 1, 2]
	pose_code = np.stack([z[f'pose/{i}/code'] for i in (0, 2, 3)])   # T-Pose / Plantarflex+Inversion / Toe Extension+Eversion+Medial
	sel = torch.tensor(idx)
	batch = dict(mesh=P3D.Meshes(gv[sel], gf[None].expand(3, -1, -1), P3D.TexturesVertex(gc[sel])), idx=sel, name=[names[i] for i in idx],
				 shape=[feet[i] for i in idx], tex=[feet[i] for i in idx], pose=[names[i] for i in idx], reg=[names[i] for i in idx],
				 pose_code=torch.from_numpy(pose_code))   # (float64, as default_collate makes it)
	batch.update(sample_latent_vectors(batch, m.latent_vectors_train))
	flags = dict(chamf=True, smooth=True, cont_pose=True)
	seed = 4242
	for attempt in range(200):   # sampler draws free of nearest-neighbour near-ties (see make_golden_composition.py)
		del draws[:], shuffled[:]
		np.random.seed(seed)
		torch.manual_seed(300 + 1000 * attempt)
		loss, losses = mwl(batch, 0, opts, **flags)
		a, bb = draws[1][3].double(), draws[0][3].double()
		gap = 1.0
		for q, t in ((a, bb), (bb, a)):
			two = torch.topk(((q[:, :, None, :] - t[:, None, :, :]) ** 2).sum(-1), 2, dim=-1, largest=False).values
			gap = min(gap, float(((two[..., 1] - two[..., 0]) / two[..., 1]).min()))
		if gap > 3e-6:
			break
	else:
		raise RuntimeError('composition: no tie-free draws found')
	pre = 'compose'
	out[f'{pre}/idx'] = np.array(idx, np.int64)
	out[f'{pre}/pose_code'] = pose_code
	out[f'{pre}/seed'] = np.int64(seed)
	out[f'{pre}/pairs'] = np.array(shuffled[0][:3], np.int32)
	out[f'{pre}/flags'] = np.array([f'{k}={v}' for k, v in sorted(flags.items())])
	out[f'{pre}/loss_keys'] = np.array(list(losses), dtype=str)
	for k, v in losses.items():
		out[f'{pre}/losses/{k}'] = np.float64(v.item())
	out[f'{pre}/loss'] = np.float64(loss.item())
	out[f'{pre}/loss_dtype'] = np.array(str(loss.dtype))
	out[f'{pre}/nn_min_relative_gap'] = np.float64(gap)
	for i, (ns, fi, uv, _pts) in enumerate(draws):
		out[f'{pre}/draw/{i}/face_idx'] = fi.numpy().astype(np.int32)
		out[f'{pre}/draw/{i}/uv'] = uv.numpy()
	out[f'{pre}/n_draws'] = np.int64(len(draws))
	print('compose', list(losses), {k: v.item() for k, v in losses.items()}, 'total', loss.item(), 'pairs', shuffled[0][:3])
	# the same step without the term, on the same draws: the other terms do not move
	replay.extend(draws)
	loss0, losses0 = mwl(batch, 0, opts, chamf=True, smooth=True)
	assert not replay
	for k, v in losses0.items():
		out[f'{pre}/without/losses/{k}'] = np.float64(v.item())
		assert v.item() == losses[k].item(), k
	out[f'{pre}/without/loss'] = np.float64(loss0.item())
	np.savez_compressed(os.path.join(HERE, 'contrastive.npz'), **out)
	print('contrastive.npz:', len(out), 'arrays,', os.path.getsize(os.path.join(HERE, 'contrastive.npz')) // 1024, 'KB')


if __name__ == '__main__':
	main()
