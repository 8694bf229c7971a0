#!/usr/bin/env python3
"""Golden vectors for the 2-D evaluation: reference src/eval/eval_metrics.py and the metric loop of src/eval/eval_2d.py, run as written.

Runs ONLY in the build container (needs /root/reference).  Stores data only: tests/golden/eval2d.npz.

(a) src/eval/eval_metrics.py imports nothing but torch and is imported for real.  Every function is called on seeded render-like
    tensors (24 x 40 images: an H / W swap changes the values): soft masks with exact zeros, a prediction with the reference's mask-out
    edit applied, identical images (PSNR inf), all-zero masks (IOU and MSE_masked nan), both MSE_masked mask shapes and a bool mask,
    IOU with one and two batch dimensions.  Stored: the inputs, the calls (`a/calls`, JSON: [function, [input names]]) and each result.

(b) src/eval/eval_2d.py:main itself, with its imports replaced by sys.modules stand-ins: init_paths; src.model.model (process_opts, and
    model_from_opts handing out a stub model with latent_vectors_val and get_meshes_from_batch); src.dataset -- the module the shipped
    script imports but which does not exist -- with Foot3DDataset / NoTextureLoading / BatchCollator; src.utils.utils.cfg;
    src.model.renderer.FootRenderer, which hands out seeded recorded renders, one GT and one prediction per foot in the metric loop
    (and plain images to the HD pass, whose output is PNGs only); pytorch3d.structures / pytorch3d.renderer.look_at_view_transform,
    trimesh, cv2, tabulate, tqdm, matplotlib.  main runs on the CPU over N_FEET feet with out_dir in a temporary directory.  Stored: the
    renders exactly as the stand-in handed them out -- before main writes into the prediction under the GT's mask-out map -- and the dict
    main returns.  That pins the mask-out copy, the `> 0` thresholds, the masked products of PSNR_B / PSNR_C, IOU on the edited mask and
    the mean over feet.

Checked by tests/test_eval2d_host.py (a float64 restatement, CPU) and tests/test_gpu_eval2d.py (find_amd.eval_metrics on the GPU).

Usage:  python tests/golden/make_golden_eval2d.py"""
import json
import os
import sys
import tempfile
import types
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
H, W = 24, 40
N_FEET = 4


def render_pair(rng, hidden):
	"""One GT render (image, soft mask, mask-out map: white / 0 under it, as the renderer leaves a GT) and one predicted render."""
	import torch
	yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing='ij')

	def silhouette(cx, cy, ax, ay):
		r2 = ((xx - cx) / ax) ** 2 + ((yy - cy) / ay) ** 2
		m = np.clip(1.0 - r2, 0.0, 1.0) * rng.uniform(0.5, 1.0, (H, W))
		m[r2 >= 0.8] = 0.0                       # exact zeros outside, soft values inside
		m[(r2 < 0.3) & (rng.rand(H, W) < 0.5)] = 1.0
		return m

	gm = silhouette(rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 0.8), rng.uniform(0.5, 0.7))
	pm = silhouette(rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 0.8), rng.uniform(0.5, 0.7))
	hide = np.zeros((H, W), bool)
	if hidden:
		r0, c0 = rng.randint(4, 10), rng.randint(6, 20)
		hide[r0:r0 + 7, c0:c0 + 12] = True
	gm[hide] = 0.0
	gi = rng.uniform(0.1, 0.9, (H, W, 3))
	gi[gm == 0] = 1.0
	pi = np.clip(gi + rng.normal(0, 0.08, (H, W, 3)), 0, 1)
	pi[pm == 0] = 1.0
	pi[hide] = rng.uniform(0.0, 0.5, (int(hide.sum()), 3))   # what the edit overwrites
	pm[hide & (rng.rand(H, W) < 0.7)] = 0.6
	f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))[None, None]
	return ({'image': f(gi), 'mask': f(gm), 'mask_out_masks': torch.from_numpy(hide)[None, None]}, {'image': f(pi), 'mask': f(pm)})


def part_a(out):
	import torch
	sys.path.insert(0, REF)
	from src.eval import eval_metrics as EM
	rng = np.random.RandomState(11)
	gt, pred = render_pair(rng, hidden=True)
	gt2, pred2 = render_pair(rng, hidden=False)
	gt3, pred3 = render_pair(rng, hidden=True)
	t = lambda a: a.clone()
	inp = {}
	inp['g'] = torch.cat([gt['image'], gt2['image'], gt3['image']], 1)[0]          # (3, H, W, 3)
	inp['p'] = torch.cat([pred['image'], pred2['image'], pred3['image']], 1)[0]
	inp['gm'] = torch.cat([gt['mask'], gt2['mask'], gt3['mask']], 1)[0]            # (3, H, W)
	inp['pm'] = torch.cat([pred['mask'], pred2['mask'], pred3['mask']], 1)[0]
	hide = torch.cat([gt['mask_out_masks'], gt2['mask_out_masks'], gt3['mask_out_masks']], 1)[0]
	ph, pmh = t(inp['p']), t(inp['pm'])
	ph[hide.unsqueeze(-1).expand_as(ph)] = 1.0                                      # eval_2d.py:92-93
	pmh[hide] = 0.0
	inp['p_hidden'], inp['pm_hidden'] = ph, pmh
	inp['union_mask'] = torch.maximum(inp['pm'], inp['gm'])
	inp['full_mask'] = torch.from_numpy(rng.uniform(0, 1, inp['g'].shape).astype(np.float32) * (rng.rand(*inp['g'].shape) < 0.6))
	inp['bool_mask'] = inp['gm'] > 0
	inp['zero_mask'] = torch.zeros_like(inp['gm'])
	inp['gm4'] = torch.cat([inp['gm'], inp['pm'][:1]]).reshape(2, 2, H, W)        # two batch dimensions
	inp['pm4'] = torch.cat([inp['pm'], inp['gm'][:1]]).reshape(2, 2, H, W)
	inp['gm_one_empty'] = torch.cat([inp['gm'][:2], torch.zeros(1, H, W)])          # one slice with union 0 -> the mean is nan
	inp['pm_one_empty'] = torch.cat([inp['pm'][:2], torch.zeros(1, H, W)])
	inp['g_flat'] = inp['g'][0, 8:15, 14:27].reshape(-1, 3)                         # 7 x 13 pixels: a length that is no multiple of 4
	inp['p_flat'] = inp['p'][0, 8:15, 14:27].reshape(-1, 3)
	calls = [
		('MSE', ['g', 'p']), ('PSNR', ['g', 'p']), ('MSE', ['g', 'p_hidden']), ('PSNR', ['g', 'p_hidden']),
		('MSE', ['g', 'g']), ('PSNR', ['g', 'g']), ('PSNR', ['g_flat', 'p_flat']),
		('MSE_masked', ['g', 'p_hidden', 'union_mask']), ('PSNR_masked', ['g', 'p_hidden', 'union_mask']),
		('MSE_masked', ['g', 'p', 'full_mask']), ('PSNR_masked', ['g', 'p', 'full_mask']),
		('MSE_masked', ['g', 'p', 'bool_mask']), ('MSE_masked', ['g', 'p', 'zero_mask']), ('PSNR_masked', ['g', 'p', 'zero_mask']),
		('PSNR_masked', ['g', 'g', 'gm']),
		('IOU', ['gm', 'pm']), ('IOU', ['gm', 'pm_hidden']), ('IOU', ['gm4', 'pm4']), ('IOU', ['zero_mask', 'zero_mask']),
		('IOU', ['gm_one_empty', 'pm_one_empty']), ('IOU', ['gm', 'gm']),
	]
	for k, v in inp.items():
		out[f'a/in/{k}'] = v.numpy()
	out['a/calls'] = np.array(json.dumps(calls))
	for i, (fn, args) in enumerate(calls):
		r = getattr(EM, fn)(*[t(inp[a]) for a in args])
		out[f'a/out/{i}'] = np.float64(r.item())
	print('[eval2d] (a)', [(fn, float(out[f'a/out/{i}'])) for i, (fn, _) in enumerate(calls)])


def part_b(out):
	import torch
	torch.cuda.is_available = lambda: False   # main picks 'cpu'
	rng = np.random.RandomState(23)
	renders = [render_pair(rng, hidden=(k % 2 == 0)) for k in range(N_FEET)]
	handed = []

	class Mesh:
		def __init__(self, foot, kind):
			self.foot, self.kind = foot, kind
		def verts_packed(self):
			return torch.zeros(10, 3)

	class FootRenderer:
		def __init__(self, image_size, device='cpu', **kw):
			self.image_size = image_size
		def linspace_views(self, nviews=1, **kw):
			return torch.eye(3).expand(nviews, 3, 3).clone(), torch.zeros(nviews, 3)
		def view_from(self, names):
			return torch.eye(3).expand(len(names), 3, 3).clone(), torch.zeros(len(names), 3)
		def __call__(self, mesh, R, T, return_mask=False, mask_out_faces=False, return_mask_out_masks=False, **kw):
			if not return_mask:   # the HD pass: its images go to PNG files only
				d = {'image': torch.ones(1, R.shape[0], H, W, 3)}
				if return_mask_out_masks:
					d['mask_out_masks'] = torch.zeros(1, R.shape[0], H, W, dtype=torch.bool)
				return d
			assert R.shape[0] == 1
			gt, pred = renders[mesh.foot]
			src = gt if mesh.kind == 'gt' else pred
			assert (mesh.kind == 'gt') == bool(mask_out_faces and return_mask_out_masks)
			handed.append((mesh.foot, mesh.kind))
			return {k: v.clone() for k, v in src.items()}

	class LatentTable:
		def __init__(self, name, n):
			self.name, self.data = name, torch.randn(n, 4)

	class Model:
		latent_vectors_val = [LatentTable('shapevec_val', N_FEET), LatentTable('texvec_val', N_FEET)]
		def eval(self):
			return self
		def to(self, device):
			return self
		def get_meshes_from_batch(self, batch, is_train=True):
			assert not is_train and batch['shapevec_val'].shape == (1, 4)
			return {'meshes': Mesh(int(batch['idx'].item()), 'pred'), 'verts': torch.zeros(1, 10, 3)}

	class Foot3DDataset:
		keypoint_labels = ['Big toe', 'Heel']
		def __init__(self, *a, **kw):
			self.n = N_FEET if not kw.get('specific_feet') else 1
		def __len__(self):
			return self.n
		def __getitem__(self, i):
			return {'idx': i, 'kp_idxs': np.array([1, 2])}

	class BatchCollator:
		def __init__(self, device='cpu'):
			pass
		def collate_batches(self, items):
			return {'idx': torch.tensor([it['idx'] for it in items]), 'kp_idxs': torch.tensor(np.stack([it['kp_idxs'] for it in items])),
					'mesh': Mesh(items[0]['idx'], 'gt')}

	class tqdm:
		def __init__(self, it):
			self.it = it
		def __enter__(self):
			return self
		def __exit__(self, *a):
			return False
		def __iter__(self):
			return iter(self.it)
		def set_description(self, s):
			pass

	def module(name, **attrs):
		m = types.ModuleType(name)
		for k, v in attrs.items():
			setattr(m, k, v)
		sys.modules[name] = m
		return m

	module('init_paths')
	module('src.model.model', model_from_opts=lambda opts: Model(), process_opts=lambda opts, eval=False: types.SimpleNamespace(model_type='neural'))
	module('src.dataset', Foot3DDataset=Foot3DDataset, NoTextureLoading=MagicMock(), BatchCollator=BatchCollator)
	module('src.utils.utils', cfg={'TEMPLATE_FEET': ['0003'], 'PCA_KEYPOINTS': [1, 2], 'SUPR_KEYPOINTS': [1, 2]})
	module('src.model.renderer', FootRenderer=FootRenderer)
	module('pytorch3d')
	module('pytorch3d.structures', join_meshes_as_batch=MagicMock())
	module('pytorch3d.renderer', look_at_view_transform=lambda **kw: (torch.eye(3)[None], torch.zeros(1, 3)))
	for name in ('trimesh', 'cv2', 'tabulate', 'matplotlib', 'matplotlib.pyplot'):
		sys.modules[name] = MagicMock(name=name)
	module('tqdm', tqdm=tqdm)
	sys.path.insert(0, REF)
	import importlib.util
	spec = importlib.util.spec_from_file_location('src.eval.eval_2d', os.path.join(REF, 'src', 'eval', 'eval_2d.py'))
	E = importlib.util.module_from_spec(spec)
	spec.loader.exec_module(E)
	with tempfile.TemporaryDirectory() as d:
		with torch.no_grad():
			res = E.main('model.pth', 'opts.yaml', exp_name='golden', out_dir=os.path.join(d, 'psnr'))
	assert [f for f, k in handed if k == 'gt'] == list(range(N_FEET)) and [f for f, k in handed if k == 'pred'] == list(range(N_FEET)), handed
	out['b/n_feet'] = np.int64(N_FEET)
	for k, (gt, pred) in enumerate(renders):
		out[f'b/{k}/gt_image'], out[f'b/{k}/gt_mask'] = gt['image'].numpy(), gt['mask'].numpy()
		out[f'b/{k}/mask_out_masks'] = gt['mask_out_masks'].numpy()
		out[f'b/{k}/pred_image'], out[f'b/{k}/pred_mask'] = pred['image'].numpy(), pred['mask'].numpy()
	out['b/keys'] = np.array(sorted(res))
	for k, v in res.items():
		out[f'b/result/{k}'] = np.float64(v)
	print('[eval2d] (b)', {k: float(v) for k, v in res.items()})


def main():
	import torch
	torch.set_num_threads(4)
	out = {}
	part_a(out)
	part_b(out)
	path = os.path.join(HERE, 'eval2d.npz')
	np.savez_compressed(path, **out)
	print('[eval2d] wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
	main()
