"""Cost of the 2-D part loss (restyle_perc_cluster) after the encoder, forward + backward, at B = 5 (one foot's views) and B = 80
(16 feet x 5 views) images of 256^2 x 21 rendered class logits with 128^2 encoder logits, timed two ways on the same device:
  built     functional.part_labels + functional.part_cross_entropy (find_part_labels, find_part_ce_fwd / _bwd), each kernel form;
  upstream  the reference's torch composition (losses.py:262-276, 302): permute, two F.interpolate, indexed write of channel 0,
            CrossEntropyLoss(reduction='none'), product, mean, and autograd's backward of it.
Host clock around work that ends in a device synchronise; one warm-up, then the median of --reps repeats with their range.  Each kernel
is also timed alone (device events around --launches launches on preallocated buffers) and the bytes it must move -- every input read
once, every output written once -- are divided by that time, to set beside the ~6.3 TB/s element-wise ceiling of the chip.
One JSON line, also written to profiles/part_loss_cost.json.

	python tools/part_loss_cost.py [--reps 5] [--launches 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
	fn()
	torch.cuda.synchronize()
	times = []
	for _ in range(reps):
		t0 = time.perf_counter()
		fn()
		torch.cuda.synchronize()
		times.append((time.perf_counter() - t0) * 1e3)
	return dict(median_ms=round(float(np.median(times)), 3), min_ms=round(min(times), 3), max_ms=round(max(times), 3))


def kernel_ms(fn, launches):
	a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	fn()
	a.record()
	for _ in range(launches):
		fn()
	b.record()
	b.synchronize()
	return a.elapsed_time(b) / launches


def upstream(x, m, g):
	"""The reference's lines on the rendered logits x (B, H, W, C), the mask m and the encoder's logits g: loss, with x.grad / m.grad filled."""
	F = torch.nn.functional
	H, W = x.shape[1:3]
	pred = F.interpolate(x.permute(0, 3, 1, 2), size=(H, W), mode='bilinear')
	gt = F.interpolate(g, size=(H, W), mode='bilinear')
	labels = torch.argmax(gt, dim=1)
	pred[:, 0] = (m == 0) * 100
	loss = (torch.nn.CrossEntropyLoss(reduction='none')(pred, labels) * m).mean()
	loss.backward()
	return loss


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--launches', type=int, default=10)
	ap.add_argument('--sizes', type=int, nargs='+', default=[5, 80])
	args = ap.parse_args()
	from find_amd import _lib, functional as FN
	from find_amd._lib import check, current_stream, ptr
	dev = torch.device('cuda', 0)
	H = W = 256
	C, h = 21, 128
	rec = dict(image=[H, W], classes=C, encoder_logits=[h, h], reps=args.reps)
	L = _lib.lib()
	for B in args.sizes:
		gen = torch.Generator(device=dev).manual_seed(B)
		x = torch.randn(B, H, W, C, device=dev, generator=gen).requires_grad_(True)
		m = torch.rand(B, H, W, device=dev, generator=gen)
		m = torch.where(m < 0.3, torch.zeros_like(m), m).requires_grad_(True)
		g = torch.randn(B, C, h, h, device=dev, generator=gen)
		P = B * H * W
		out = dict(pixels=P, logits_MB=round(P * C * 4 / 2 ** 20, 1))

		def built(form):
			x.grad = m.grad = None
			FN.part_cross_entropy(x, FN.part_labels(g, (H, W)), m, form=form).backward()
		for form in ('staged', 'direct'):
			out[f'built_{form}'] = timed(lambda: built(form), args.reps)

		def ref():
			x.grad = m.grad = None
			upstream(x, m, g)
		out['upstream_torch'] = timed(ref, args.reps)
		# the two paths agree
		built('auto')
		gx, gm = x.grad.clone(), m.grad.clone()
		ref()
		out['max_abs_diff_d_logits'] = float((gx - x.grad).abs().max())
		out['max_abs_diff_d_mask'] = float((gm - m.grad).abs().max())
		x.grad = m.grad = None
		# each kernel alone
		s = current_stream(dev)
		xd, md = x.detach(), m.detach()
		labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
		loss, ce = torch.empty((), device=dev), torch.empty(B, H, W, device=dev)
		partial = torch.empty((P + 63) // 64, dtype=torch.float64, device=dev)
		one, dx, dm = torch.ones((), device=dev), torch.empty_like(xd), torch.empty_like(md)
		ms = kernel_ms(lambda: check(L.find_part_labels(ptr(g), B, C, h, h, H, W, ptr(labels), s), 'find_part_labels'), args.launches)
		nbytes = g.numel() * 4 + P * 4
		out['labels_kernel'] = dict(ms=round(ms, 4), bytes=nbytes, TB_per_s=round(nbytes / ms / 1e9, 3))
		for form in ('staged', 'direct'):
			f = FN.PART_FORMS[form]
			ms = kernel_ms(lambda: check(L.find_part_ce_fwd(ptr(xd), ptr(labels), ptr(md), P, C, ptr(loss), ptr(ce), ptr(partial), f, s), 'find_part_ce_fwd'),
						   args.launches)
			nbytes = P * C * 4 + 3 * P * 4   # logits, labels, mask in; ce out
			out[f'ce_fwd_{form}'] = dict(ms=round(ms, 4), bytes=nbytes, TB_per_s=round(nbytes / ms / 1e9, 3))
			ms = kernel_ms(lambda: check(L.find_part_ce_bwd(ptr(xd), ptr(labels), ptr(md), P, C, ptr(one), ptr(dx), ptr(dm), f, s), 'find_part_ce_bwd'),
						   args.launches)
			nbytes = 2 * P * C * 4 + 3 * P * 4   # logits, labels, mask in; d_logits, d_mask out
			out[f'ce_bwd_{form}'] = dict(ms=round(ms, 4), bytes=nbytes, TB_per_s=round(nbytes / ms / 1e9, 3))
		rec[f'B{B}'] = out
		del x, m, g, xd, md, dx, dm, gx, gm
		torch.cuda.empty_cache()
	line = json.dumps(rec)
	print(line, flush=True)
	os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
	with open(os.path.join(ROOT, 'profiles', 'part_loss_cost.json'), 'w') as fh:
		fh.write(line + '\n')


if __name__ == '__main__':
	main()
