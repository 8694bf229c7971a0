#!/usr/bin/env python3
"""Golden vectors for the 2-D part loss (reference src/model/losses.py:251-302, RestylePerceptualLoss.forward(mode='cluster',
pred_logit=...); call site src/model/model.py:1129-1147) -> part_loss.npz.

Runs ONLY in the build container (needs the reference checkout).  Executed for real, as written: RestylePerceptualLoss.forward on the
CPU, on an object made with __new__ + nn.Module.__init__ (the constructor loads encoder weights that do not exist) whose encoder is a
stub that returns the case's class logits, with the PyTorch3D stand-ins of make_golden_composition and make_golden_mlp.import_reference.

  * ce/<name>: rendered logits x (B, H, W, C) channel-last (handed over as upstream does, x.permute(0, 3, 1, 2)), predicted mask m
    (B, H, W), encoder logits g (B, C, h, w) -> loss, d loss / d x (channel-last), d loss / d m, encodings['gt_labels'], ['CE_loss'].
    x is unit normal unless said otherwise, m uniform with values below 0.3 set to exactly 0.
  * labels/<name>: g (B, C, h, w) and the size (H, W) -> encodings['gt_labels'].  Seeds are retried until every output pixel's top-2
    gap of the float64 resample is >= MARGIN_GAP (a label must not hang on fp32 rounding); two cases hold exact ties by construction."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

MARGIN_GAP = 1e-4


def bilinear_f64(g, H, W):
	"""F.interpolate(g, (H, W), mode='bilinear') (align_corners=False) in float64."""
	import numpy as np
	g = np.asarray(g, np.float64)
	h, w = g.shape[-2:]

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
	return top * ly0[:, None] + bot * ly1[:, None]


def top2_gap(G):
	import numpy as np
	if G.shape[1] < 2:
		return np.inf
	s = np.sort(G, axis=1)
	return float((s[:, -1] - s[:, -2]).min())


def main():
	import numpy as np
	import torch
	torch.set_num_threads(4)
	from make_golden_composition import install_pytorch3d_stand_ins
	install_pytorch3d_stand_ins([], [])
	import make_golden_mlp as G
	G.import_reference()
	import src.model.losses as ref_losses
	nn = torch.nn

	def run(x, m, g, size=None):
		"""The reference's forward on one case; x / m may be None (label cases: zeros logits, ones mask)."""
		crit = ref_losses.RestylePerceptualLoss.__new__(ref_losses.RestylePerceptualLoss)
		nn.Module.__init__(crit)
		crit._cluster_crit_full = nn.CrossEntropyLoss(reduction='none')
		gt = torch.from_numpy(g)
		crit.encoder = lambda images, return_features=False, target_feature_maps=None: {'class_logits': gt.clone()}
		B, C = g.shape[:2]
		H, W = size if size is not None else x.shape[1:3]
		xt = torch.from_numpy(x if x is not None else np.zeros((B, H, W, C), np.float32)).requires_grad_(True)
		mt = torch.from_numpy(m if m is not None else np.ones((B, H, W), np.float32)).requires_grad_(True)
		img = torch.zeros(B, H, W, 3)
		before = xt.detach().clone()
		loss, enc = crit(img, img, mode='cluster', feature_maps=[8], pred_masks=mt, pred_logit=xt.permute(0, 3, 1, 2), return_encodings=True)
		loss.backward()
		assert torch.equal(before, xt.detach())   # (the caller's logits are not modified in place)
		return dict(loss=np.float32(loss.item()), d_logits=xt.grad.numpy().copy(), d_mask=mt.grad.numpy().copy(),
					gt_labels=enc['gt_labels'].numpy().astype(np.int32), CE_loss=enc['CE_loss'].detach().numpy().copy())

	out = {}
	# ------------------------------------------------------------------ cross-entropy cases
	# name -> (B, H, W, C, (h, w) of the encoder logits, special)
	ce_cases = {
		'b3_5x7_c21': (3, 5, 7, 21, (3, 4), None),          # 105 pixels: no multiple of 64
		'c1': (2, 8, 8, 1, (4, 4), None),
		'c2': (2, 8, 8, 2, (4, 4), None),
		'c33': (2, 8, 8, 33, (4, 4), None),
		'c64': (2, 8, 8, 64, (4, 4), None),
		'mask_all_zero': (2, 8, 8, 21, (4, 4), 'zero'),
		'mask_zero_and_tiny': (2, 8, 8, 21, (4, 4), 'tiny'),   # exact zeros beside 1e-30: the `m == 0` switch
		'labels_zero_inside': (2, 8, 8, 21, (8, 8), 'label0'),
		'logits_pm120': (2, 8, 8, 21, (4, 4), 'big'),          # an exp without the maximum subtracted overflows
	}
	for ci, (name, (B, H, W, C, (h, w), special)) in enumerate(ce_cases.items()):
		for attempt in range(500):
			rng = np.random.default_rng(100 * ci + attempt)
			x = rng.standard_normal((B, H, W, C)).astype(np.float32)
			m = rng.uniform(0, 1, (B, H, W)).astype(np.float32)
			m[m < 0.3] = 0.0
			g = rng.standard_normal((B, C, h, w)).astype(np.float32)
			if special == 'zero':
				m[:] = 0.0
			elif special == 'tiny':
				m = np.where(rng.uniform(0, 1, m.shape) < 0.5, 0.0, 1e-30).astype(np.float32)
			elif special == 'label0':
				g[:, 0][m > 0] = 50.0
			elif special == 'big':
				x = (120.0 * np.sign(x)).astype(np.float32)
			if top2_gap(bilinear_f64(g, H, W)) >= MARGIN_GAP:
				break
		else:
			raise RuntimeError(f'case {name}: no admissible draw')
		r = run(x, m, g)
		assert np.isfinite(r['loss']) and np.isfinite(r['d_logits']).all() and np.isfinite(r['d_mask']).all(), name
		assert (r['d_logits'][..., 0] == 0).all(), name   # (the rendered channel 0 is discarded)
		if special == 'label0':
			assert (r['gt_labels'][m > 0] == 0).all() and (m > 0).any()
		out[f'ce/{name}/logits'], out[f'ce/{name}/mask'], out[f'ce/{name}/gt_logits'] = x, m, g
		for k, v in r.items():
			out[f'ce/{name}/{k}'] = v
	out['ce_cases'] = np.array(list(ce_cases))

	# ------------------------------------------------------------------ label cases
	# name -> (B, C, (h, w), (H, W))
	label_cases = {
		'up_12_24': (3, 21, (12, 12), (24, 24)),
		'up_5_13': (2, 21, (5, 5), (13, 13)),
		'same_16': (2, 21, (16, 16), (16, 16)),
		'down_24_12': (2, 5, (24, 24), (12, 12)),
		'up_7x5_9x14': (2, 21, (7, 5), (9, 14)),
	}
	for ci, (name, (B, C, hw, HW)) in enumerate(label_cases.items()):
		for attempt in range(500):
			g = np.random.default_rng(attempt + 1000 * ci).standard_normal((B, C, *hw)).astype(np.float32)
			gap = top2_gap(bilinear_f64(g, *HW))
			if gap >= MARGIN_GAP:
				break
		else:
			raise RuntimeError(f'label case {name}: no admissible draw')
		out[f'labels/{name}/gt_logits'], out[f'labels/{name}/size'], out[f'labels/{name}/gap'] = g, np.array(HW), np.float64(gap)
		out[f'labels/{name}/gt_labels'] = run(None, None, g, HW)['gt_labels']
		assert np.array_equal(out[f'labels/{name}/gt_labels'], bilinear_f64(g, *HW).argmax(1)), name
	# exact ties: every channel equal (label 0 everywhere), and channels 2 and 4 equal maxima (label 2 everywhere)
	plane = np.random.default_rng(77).standard_normal((2, 1, 6, 6)).astype(np.float32)
	ties = {'tie_all_equal': np.repeat(plane, 7, axis=1), 'tie_two_maxima': np.repeat(plane, 7, axis=1)}
	ties['tie_two_maxima'][:, [0, 1, 3, 5, 6]] -= np.float32(1.0)
	for name, g in ties.items():
		out[f'labels/{name}/gt_logits'], out[f'labels/{name}/size'], out[f'labels/{name}/gap'] = g, np.array((15, 15)), np.float64(0.0)
		out[f'labels/{name}/gt_labels'] = run(None, None, g, (15, 15))['gt_labels']
	assert (out['labels/tie_all_equal/gt_labels'] == 0).all() and (out['labels/tie_two_maxima/gt_labels'] == 2).all()
	out['label_cases'] = np.array(list(label_cases) + list(ties))

	dst = os.path.join(HERE, 'part_loss.npz')
	np.savez_compressed(dst, **out)
	print(dst, os.path.getsize(dst), 'bytes;', {n: float(out[f'labels/{n}/gap']) for n in label_cases})


if __name__ == '__main__':
	main()
