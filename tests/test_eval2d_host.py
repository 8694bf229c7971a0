"""2-D evaluation (find_amd.eval_metrics MSE / PSNR / MSE_masked / PSNR_masked / IOU, eval_2d_metrics, find_amd.evaluate) without a GPU:
the C-ABI's symbols and argument checks, a float64 restatement of the reference's definitions against tests/golden/eval2d.npz (made by
tests/golden/make_golden_eval2d.py from the reference's own code), and the Python wrappers' errors."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval2d.npz')


# ---------------------------------------------------------------------------------------------- float64 restatement
def sums64(pred, gt, pred_mask=None, gt_mask=None, hide=None, weight=None):
	"""The seven per-image sums of find_image_metrics in float64 (torch, any device): pred, gt (n_img, *pixels, C)."""
	n = pred.shape[0]
	p, g = pred.double().reshape(n, -1, pred.shape[-1]), gt.double().reshape(n, -1, gt.shape[-1])
	ones = torch.ones(p.shape[:2], dtype=torch.float64, device=p.device)
	pm = ones if pred_mask is None else pred_mask.double().reshape(n, -1)
	gm = ones if gt_mask is None else gt_mask.double().reshape(n, -1)
	w = ones if weight is None else weight.double().reshape(n, -1)
	if hide is not None:
		h = hide.bool().reshape(n, -1)
		p = torch.where(h[..., None], torch.ones_like(p), p)
		pm = torch.where(h, torch.zeros_like(pm), pm)
	bg, bp = (gm > 0).double()[..., None], (pm > 0).double()[..., None]
	d2 = (g - p) ** 2
	return torch.stack([d2.sum((1, 2)), ((g * bg - p * bp) ** 2).sum((1, 2)), ((g * bg * bp - p * bg * bp) ** 2).sum((1, 2)), (gm * pm).sum(1),
						torch.maximum(gm, pm).sum(1), (w[..., None] * d2).sum((1, 2)), w.sum(1)], dim=1)


def mse64(p1, p2):
	return ((p1.double() - p2.double()) ** 2).mean()


def psnr64(p1, p2):
	return -10 * torch.log10(mse64(p1, p2))


def mse_masked64(p1, p2, mask):
	m = mask.unsqueeze(-1) if mask.shape == p1.shape[:-1] else mask
	m = m.double().expand(p1.shape)
	return (m * (p1.double() - p2.double()) ** 2).sum() / m.sum()


def psnr_masked64(p1, p2, mask):
	return -10 * torch.log10(mse_masked64(p1, p2, mask))


def iou64(s1, s2):
	a, b = s1.double().reshape(-1, *s1.shape[-2:]), s2.double().reshape(-1, *s2.shape[-2:])
	return ((a * b).sum((1, 2)) / torch.maximum(a, b).sum((1, 2))).mean()


REF64 = {'MSE': mse64, 'PSNR': psnr64, 'MSE_masked': mse_masked64, 'PSNR_masked': psnr_masked64, 'IOU': iou64}


def eval_2d_group64(gt_image, gt_mask, hide, pred_image, pred_mask):
	"""One group of eval_2d.py's inner loop (the edit of the prediction, then the five metrics), float64."""
	p, pm = pred_image.double().clone(), pred_mask.double().clone()
	if hide is not None:
		p[hide.bool().unsqueeze(-1).expand_as(p)] = 1.0
		pm[hide.bool()] = 0.0
	g, gm = gt_image.double(), gt_mask.double()
	bg, bp = (gm > 0).double().unsqueeze(-1), (pm > 0).double().unsqueeze(-1)
	return {'MSE': mse64(g, p), 'PSNR_A': psnr64(g, p), 'PSNR_B': psnr64(g * bg, p * bp), 'PSNR_C': psnr64(g * bg * bp, p * bg * bp), 'IOU': iou64(gm, pm)}


def golden():
	return dict(np.load(GOLDEN))


def golden_calls(G):
	return [(fn, args) for fn, args in json.loads(str(G['a/calls']))]


def assert_close(got, want, rtol, what):
	got, want = float(got), float(want)
	if np.isnan(want) or np.isinf(want):
		assert (np.isnan(got) and np.isnan(want)) or got == want, (what, got, want)
	else:
		assert abs(got - want) <= rtol * max(abs(want), 1e-12), (what, got, want)


# ---------------------------------------------------------------------------------------------- tests
def test_library_exports_the_metric_entry_points():
	from find_amd import _lib
	L = _lib.lib()
	for name in ('find_image_metrics_ws_bytes', 'find_image_metrics'):
		assert hasattr(L, name) and name in _lib.PROTOTYPES
	assert L.find_image_metrics_ws_bytes(64, 128 * 128) > 0
	assert L.find_image_metrics_ws_bytes(0, 10) == -1 and L.find_image_metrics_ws_bytes(3, 0) == -1


def test_metric_entry_point_argument_checks():
	"""Every check comes before a launch: NULL pointers, bad sizes and a short workspace are refused on a host without a GPU."""
	from find_amd import _lib
	L = _lib.lib()
	fake = ctypes.c_void_p(4096)   # never dereferenced: the checks return first
	need = L.find_image_metrics_ws_bytes(2, 100)
	assert L.find_image_metrics(None, fake, None, None, None, None, 2, 100, 3, fake, fake, need, None) == -1
	assert b'NULL' in L.find_last_error()
	assert L.find_image_metrics(fake, fake, None, None, None, None, 2, 100, 3, None, fake, need, None) == -1
	assert L.find_image_metrics(fake, fake, None, None, None, None, 0, 100, 3, fake, fake, need, None) == -1
	assert b'bad sizes' in L.find_last_error()
	assert L.find_image_metrics(fake, fake, None, None, None, None, 2, 100, 0, fake, fake, need, None) == -1
	assert L.find_image_metrics(fake, fake, None, None, None, None, 2, 100, 3, fake, fake, need - 1, None) == -2
	assert b'workspace' in L.find_last_error()


def test_restatement_reproduces_reference_metric_functions():
	"""Part (a): every call the generator made to reference eval_metrics.py, restated in float64 (inf / nan in the same places)."""
	G = golden()
	calls = golden_calls(G)
	assert {fn for fn, _ in calls} == set(REF64)
	for i, (fn, args) in enumerate(calls):
		got = REF64[fn](*[torch.from_numpy(G[f'a/in/{a}']) for a in args])
		assert_close(got, G[f'a/out/{i}'], 1e-5, (i, fn, args))
	outs = [float(G[f'a/out/{i}']) for i in range(len(calls))]
	assert any(np.isinf(v) for v in outs) and any(np.isnan(v) for v in outs)


def test_restatement_reproduces_reference_eval_2d_main():
	"""Part (b): the dict eval_2d.main returned for the recorded renders: per-foot groups (nviews = batch_size = 1), mean over feet."""
	G = golden()
	per = {k: [] for k in G['b/keys']}
	hidden = 0
	for k in range(int(G['b/n_feet'])):
		t = lambda name: torch.from_numpy(G[f'b/{k}/{name}'])
		hidden += int(t('mask_out_masks').any())
		for key, v in eval_2d_group64(t('gt_image'), t('gt_mask'), t('mask_out_masks'), t('pred_image'), t('pred_mask')).items():
			per[key].append(float(v))
	assert 0 < hidden < int(G['b/n_feet'])
	for key, vals in per.items():
		assert_close(np.mean(vals), G[f'b/result/{key}'], 1e-5, key)


def test_sums64_compose_to_the_metrics():
	"""The sums the kernel produces, composed as eval_metrics composes them, give the restated metrics (the host half of the GPU path)."""
	G = golden()
	g, p = torch.from_numpy(G['a/in/g']), torch.from_numpy(G['a/in/p'])
	gm, pm = torch.from_numpy(G['a/in/gm']), torch.from_numpy(G['a/in/pm'])
	s = sums64(p, g, pm, gm, weight=gm)
	assert_close(s[:, 0].sum() / g.numel(), mse64(g, p), 1e-12, 'MSE')
	assert_close(s[:, 5].sum() / (3 * s[:, 6].sum()), mse_masked64(g, p, gm), 1e-12, 'MSE_masked')
	assert_close((s[:, 3] / s[:, 4]).mean(), iou64(gm, pm), 1e-12, 'IOU')


def test_wrappers_reject_bad_arguments():
	from find_amd import eval_metrics as EM
	from find_amd import functional as FN
	a, b = torch.rand(2, 5, 3), torch.rand(2, 6, 3)
	with pytest.raises(ValueError, match='differ'):
		FN.image_metric_sums(a, b)
	with pytest.raises(ValueError, match='without channels'):
		FN.image_metric_sums(a, a, pred_mask=torch.rand(2, 6))
	with pytest.raises(ValueError, match='without channels'):
		FN.image_metric_sums(a, a, hide=torch.zeros(2, 5, 3, dtype=torch.bool))
	with pytest.raises(RuntimeError, match='ROCm device'):
		FN.image_metric_sums(a, a)
	for fn in (EM.MSE, EM.PSNR):
		with pytest.raises(ValueError, match='differ'):
			fn(a, b)
		with pytest.raises(RuntimeError, match='ROCm device'):
			fn(a, a)
	with pytest.raises(ValueError, match='differ'):
		EM.MSE_masked(a, b, torch.ones(2, 5))
	with pytest.raises(ValueError, match='differ'):
		EM.IOU(torch.rand(3, 4), torch.rand(4, 3))
	with pytest.raises(RuntimeError, match='ROCm device'):
		EM.IOU(torch.rand(3, 4), torch.rand(3, 4))
	gt = {'image': torch.rand(1, 3, 4, 4, 3), 'mask': torch.rand(1, 3, 4, 4)}
	with pytest.raises(ValueError, match='groups of 2'):
		EM.eval_2d_metrics(gt, gt, batch_size=2)


def test_iou_other_reductions_raise():
	from find_amd import eval_metrics as EM
	with pytest.raises(NotImplementedError, match='sum'):
		EM.IOU(torch.rand(2, 4, 4), torch.rand(2, 4, 4), reduce='sum')


def test_evaluate_module_imports():
	from find_amd import evaluate
	assert callable(evaluate.eval_2d) and evaluate.METRICS == ('MSE', 'PSNR_A', 'PSNR_B', 'PSNR_C', 'IOU')
