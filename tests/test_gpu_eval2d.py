"""2-D evaluation on the GPU: find_image_metrics against a float64 evaluation (vector and tail paths, every optional input, 64 x 512^2),
repeatability, the reference's own results (tests/golden/eval2d.npz), find_amd.evaluate.eval_2d end to end on a synthetic Foot3D folder
and the C-ABI's error codes."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests.test_eval2d_host import assert_close, eval_2d_group64, golden, golden_calls, iou64, mse64, psnr64, sums64

pytestmark = pytest.mark.gpu


def _inputs(n_img, pix, C, seed, hide=True, masks=True, weight=True):
	g = torch.Generator(device='cuda').manual_seed(seed)
	r = lambda *s: torch.rand(*s, generator=g, device='cuda')
	shape = (n_img, *pix)
	pred, gt = r(*shape, C), r(*shape, C)
	pm = (r(*shape) - 0.3).clamp_min(0) if masks else None   # soft, with exact zeros
	gm = (r(*shape) - 0.3).clamp_min(0) if masks else None
	h = (r(*shape) < 0.2) if hide else None
	w = r(*shape) if weight else None
	return pred, gt, pm, gm, h, w


def _check_sums(got, want):
	assert got.dtype == torch.float64 and got.shape == want.shape
	err = (got - want).abs()
	assert bool((err <= torch.maximum(1e-6 * want.abs(), torch.full_like(want, 1e-9))).all()), (err.max().item(), (err / want.abs()).max().item())


@pytest.mark.parametrize('n_img,pix,C', [(3, (1001,), 3), (2, (1, 1), 3), (4, (48, 64), 3), (5, (4096,), 1), (3, (37, 29), 1), (2, (100,), 2),
										  (7, (33,), 3)])
@pytest.mark.parametrize('opts', [dict(), dict(hide=False), dict(masks=False), dict(weight=False), dict(hide=False, masks=False, weight=False)])
def test_sums_match_float64(n_img, pix, C, opts):
	from find_amd import functional as FN
	pred, gt, pm, gm, h, w = _inputs(n_img, pix, C, seed=n_img * 100 + C, **opts)
	got = FN.image_metric_sums(pred, gt, pm, gm, h, w)
	_check_sums(got, sums64(pred, gt, pm, gm, h, w))


def test_sums_64_images_at_512_and_repeatable():
	from find_amd import functional as FN
	pred, gt, pm, gm, h, w = _inputs(64, (512, 512), 3, seed=7)
	a = FN.image_metric_sums(pred, gt, pm, gm, h, w)
	_check_sums(a, sums64(pred, gt, pm, gm, h, w))
	b = FN.image_metric_sums(pred, gt, pm, gm, h, w)
	assert torch.equal(a, b)
	# the scalar path (a channel count without a vector kernel) repeats as well
	x = _inputs(3, (1001,), 2, seed=3)
	assert torch.equal(FN.image_metric_sums(*x), FN.image_metric_sums(*x))


def test_hide_leaves_inputs_untouched_and_accepts_uint8():
	from find_amd import functional as FN
	pred, gt, pm, gm, h, w = _inputs(2, (16, 20), 3, seed=5)
	p0, m0 = pred.clone(), pm.clone()
	a = FN.image_metric_sums(pred, gt, pm, gm, h, w)
	assert torch.equal(pred, p0) and torch.equal(pm, m0)
	assert torch.equal(a, FN.image_metric_sums(pred, gt, pm, gm, h.to(torch.uint8), w))
	# non-contiguous inputs are read as their values
	big = torch.rand(2, 16, 20, 4, device='cuda')
	_check_sums(FN.image_metric_sums(big[..., :3], gt, pm, gm, h, w), sums64(big[..., :3], gt, pm, gm, h, w))


def test_wrappers_reject_mixed_devices():
	from find_amd import functional as FN
	pred, gt, pm, gm, h, w = _inputs(2, (8, 8), 3, seed=1)
	with pytest.raises(RuntimeError, match='ROCm device'):
		FN.image_metric_sums(pred, gt, pred_mask=pm.cpu())
	with pytest.raises(ValueError, match='bool or uint8'):
		FN.image_metric_sums(pred, gt, hide=pm)


def test_reference_metric_functions_fixture():
	"""Part (a) of the fixture: the reference's eval_metrics.py results, from find_amd.eval_metrics on CUDA tensors."""
	from find_amd import eval_metrics as EM
	G = golden()
	for i, (fn, args) in enumerate(golden_calls(G)):
		got = getattr(EM, fn)(*[torch.from_numpy(G[f'a/in/{a}']).cuda() for a in args])
		assert got.dtype == torch.float32 and got.dim() == 0
		assert_close(got.item(), G[f'a/out/{i}'], 1e-5, (i, fn, args))


def test_reference_eval_2d_main_fixture():
	"""Part (b): eval_2d_metrics fed the renders the reference's main saw gives the dict main returned -- one foot per call and all feet in
	one call -- and leaves the render dicts as they were."""
	from find_amd.eval_metrics import eval_2d_metrics
	G = golden()
	nf = int(G['b/n_feet'])
	t = lambda k, name: torch.from_numpy(G[f'b/{k}/{name}']).cuda()
	per = {k: [] for k in G['b/keys']}
	for k in range(nf):
		gt = {'image': t(k, 'gt_image'), 'mask': t(k, 'gt_mask'), 'mask_out_masks': t(k, 'mask_out_masks')}
		pred = {'image': t(k, 'pred_image'), 'mask': t(k, 'pred_mask')}
		p0 = pred['image'].clone()
		for key, v in eval_2d_metrics(pred, gt, batch_size=1).items():
			assert v.shape == (1,)
			per[key].append(v.item())
		assert torch.equal(pred['image'], p0)
	for key, vals in per.items():
		assert_close(np.mean(vals), G[f'b/result/{key}'], 1e-5, key)
	cat = lambda name: torch.cat([t(k, name) for k in range(nf)])
	gt = {'image': cat('gt_image'), 'mask': cat('gt_mask'), 'mask_out_masks': cat('mask_out_masks'), 'nothing_hidden': False}
	pred = {'image': cat('pred_image'), 'mask': cat('pred_mask')}
	for key, v in eval_2d_metrics(pred, gt, batch_size=1).items():
		assert v.shape == (nf,)
		assert_close(v.mean().item(), G[f'b/result/{key}'], 1e-5, key)


def _write_marked_scan(folder, rel_obj, rel_png, n_side, every=3):
	"""A _write_scan sheet whose OBJ ends its UV list with the mask-out marker `vt 0 0`, used for all three corners by every `every`-th face."""
	from PIL import Image
	os.makedirs(os.path.dirname(os.path.join(folder, rel_obj)), exist_ok=True)
	lines = [f'v {i * 0.01:.6f} {j * 0.01:.6f} {0.002 * ((i * j) % 3):.6f}' for i in range(n_side) for j in range(n_side)]
	lines += [f'vt {i / (n_side - 1):.6f} {j / (n_side - 1):.6f}' for i in range(n_side) for j in range(n_side)]
	lines.append('vt 0 0')
	marker = n_side * n_side + 1
	idx = lambda i, j: i * n_side + j + 1
	k = 0
	for i in range(n_side - 1):
		for j in range(n_side - 1):
			a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
			for tri in ((a, b, c), (a, c, d)):
				if k % every == 0:
					lines.append('f ' + ' '.join(f'{v}/{marker}' for v in tri))
				else:
					lines.append('f ' + ' '.join(f'{v}/{v}' for v in tri))
				k += 1
	with open(os.path.join(folder, rel_obj), 'w') as fh:
		fh.write('# synthetic scan with masked faces\n' + '\n'.join(lines) + '\n')
	img = (np.random.RandomState(n_side).rand(8, 6, 3) * 255).astype(np.uint8)
	Image.fromarray(img).save(os.path.join(folder, rel_png))


def _foot3d_val(tmp_path):
	from tests.test_host_dataset import CFG_POSE, _write_scan
	from find_amd.dataset import Foot3DDataset
	root = str(tmp_path)
	mesh_dir = os.path.join(root, 'Meshes_sliced')
	data, val = [], []
	for k, fid in enumerate(['0011', '0012', '0013', '0014']):
		rel = f'{fid}/A/{fid}-A'
		if k == 1:
			_write_marked_scan(mesh_dir, rel + '.obj', rel + '.png', 9)
		else:
			_write_scan(mesh_dir, rel + '.obj', rel + '.png', 7 + k, (0.0, 0.0, 0.0))
		data.append({'Foot ID': fid, 'Scan ID': 'A', 'footedness': 'Left', 'pose': ['T-Pose'], 'keypoints': None, 'OBJ file': rel + '.obj', 'PNG file': rel + '.png'})
		val.append(fid)
	jpath = os.path.join(root, 'index.json')
	with open(jpath, 'w') as fh:
		json.dump({'keypoint_labels': ['a'], 'data': data}, fh)
	cfg = {'DATASET_FOLDER': root, 'DATASET_JSON': jpath, 'DATASET_NAME': 'Meshes_sliced', 'LOWPOLY_DATASET_NAME': 'x', 'VAL_FEET': val, 'TEMPLATE_FEET': [],
		   'POSE_VECTOR': CFG_POSE}
	return Foot3DDataset(cfg, device='cpu', is_train=False)


def _model(n_val):
	from find_amd import synthetic
	model = synthetic.make_model(1002, train_size=2, val_size=n_val, device='cuda')
	lat = synthetic.latents(n_val, seed=4, device='cuda')
	with torch.no_grad():
		model.shapevec_val.data.copy_(lat['shapevec'])
		model.texvec_val.data.copy_(lat['texvec'])
		model.posevec_val.data.copy_(lat['posevec'])
		model.reg_val.data.copy_(lat['reg'])
	return model


def test_eval_2d_end_to_end(tmp_path):
	from find_amd import evaluate
	from find_amd.dataset import BatchCollator
	from find_amd.renderer import FootRenderer
	ds = _foot3d_val(tmp_path)
	assert len(ds) == 4
	model = _model(len(ds))
	size, nviews, bs = 48, 4, 2
	res1, per1 = evaluate.eval_2d(model, ds, image_size=size, nviews=nviews, batch_size=bs, feet_per_call=1, return_per_image=True)
	res3, per3 = evaluate.eval_2d(model, ds, image_size=size, nviews=nviews, batch_size=bs, feet_per_call=3, return_per_image=True)
	assert set(res1) == {'MSE', 'PSNR_A', 'PSNR_B', 'PSNR_C', 'IOU'} and all(isinstance(v, float) for v in res1.values())
	assert model.training   # restored
	for k in res1:
		assert per1[k].shape == (len(ds) * (nviews // bs),)
		assert_close(res3[k], res1[k], 1e-5, ('feet_per_call', k))
		assert torch.allclose(per3[k], per1[k], rtol=1e-5, atol=1e-7, equal_nan=True), k
	# the reference's loop, one foot and one group of views at a time (eval_2d.py:79-121), metrics restated in float64
	rdr = FootRenderer(image_size=size, device='cuda')
	R, T = rdr.linspace_views(nviews=nviews, dist=0.3, elev_min=-90, elev_max=90)
	collate = BatchCollator(device='cuda').collate_batches
	model.eval()
	ref = {k: [] for k in res1}
	hidden_pixels = 0
	with torch.no_grad():
		for i in range(len(ds)):
			batch = collate([ds[i]])
			batch.update({vec.name: vec.data[batch['idx']] for vec in model.latent_vectors_val})
			out = model.get_meshes_from_batch(batch, is_train=False)
			for b in range(nviews // bs):
				Rb, Tb = R[b * bs:(b + 1) * bs], T[b * bs:(b + 1) * bs]
				gt = rdr(batch['mesh'], Rb, Tb, return_mask=True, mask_out_faces=True, return_mask_out_masks=True)
				pred = rdr(out['meshes'], Rb, Tb, return_mask=True)
				hidden_pixels += int(gt['mask_out_masks'].sum())
				for k, v in eval_2d_group64(gt['image'], gt['mask'], gt['mask_out_masks'], pred['image'], pred['mask']).items():
					ref[k].append(v.item())
	model.train()
	assert hidden_pixels > 0   # the marked scan hid some of its faces
	for k in res1:
		assert_close(res1[k], np.mean(ref[k]), 1e-5, k)
		assert np.allclose(per1[k].cpu().numpy(), ref[k], rtol=1e-5, atol=1e-7, equal_nan=True), k


def test_c_abi_error_codes():
	from find_amd import _lib
	L = _lib.lib()
	pred, gt, pm, gm, h, w = _inputs(2, (10, 10), 3, seed=2)
	sums = torch.empty(2, 7, dtype=torch.float64, device='cuda')
	need = L.find_image_metrics_ws_bytes(2, 100)
	ws = torch.empty(need, dtype=torch.uint8, device='cuda')
	P = _lib.ptr
	args = lambda **kw: [kw.get('pred', P(pred)), kw.get('gt', P(gt)), P(pm), P(gm), P(h), P(w), kw.get('n_img', 2), kw.get('n_pix', 100),
						 kw.get('C', 3), kw.get('sums', P(sums)), P(ws), kw.get('ws_bytes', need), None]
	assert L.find_image_metrics(*args(pred=None)) == -1 and b'NULL' in L.find_last_error()
	assert L.find_image_metrics(*args(sums=None)) == -1
	assert L.find_image_metrics(*args(n_img=0)) == -1 and b'bad sizes' in L.find_last_error()
	assert L.find_image_metrics(*args(C=17)) == -1
	assert L.find_image_metrics(*args(ws_bytes=need - 8)) == -2 and b'workspace' in L.find_last_error()
	assert L.find_image_metrics(*args()) == 0
	_check_sums(sums, sums64(pred, gt, pm, gm, h, w))
