"""Cost of the surface-normal loss, forward + backward, at B = 5 (one foot's views) and B = 80 (16 feet x 5 views) normal maps of 256^2,
timed two ways on the same tensors and the same device:
  built  functional.normal_loss (find_normal_loss_fwd / _bwd);
  torch  the composition a user would write: F.normalize both maps, dot product, weighted mean, and autograd's backward of it.
Host clock around work that ends in a device synchronise; one warm-up, then the median of --reps repeats with their range.  Each kernel
is also timed alone (device events around --launches launches on preallocated buffers) and the bytes it must move -- pred, target and
weight read once each way, d pred written once -- are divided by that time, to set beside the ~6.3 TB/s element-wise ceiling of the chip.
One JSON line, also written to --out (default profiles/normal_loss_cost.json).

	python tools/normal_loss_cost.py [--reps 5] [--launches 10] [--out FILE]"""
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


def composition(p, t, w):
	"""The torch composition on pred p, target t (B, H, W, 3) and weight w (B, H, W): loss, with p.grad filled.  (F.normalize clamps the
	norm at 1e-6 where the built op takes the cosine as 0: the same on these inputs, which hold no such vectors.)"""
	F = torch.nn.functional
	c = (F.normalize(p, dim=-1, eps=1e-6) * F.normalize(t, dim=-1, eps=1e-6)).sum(-1)
	loss = (w * (1 - c)).sum() / w.sum().clamp(min=1e-12)
	loss.backward()
	return loss


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--launches', type=int, default=10)
	ap.add_argument('--sizes', type=int, nargs='+', default=[5, 80])
	ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'normal_loss_cost.json'))
	args = ap.parse_args()
	from find_amd import _lib, functional as FN
	from find_amd._lib import check, current_stream, ptr
	dev = torch.device('cuda', 0)
	H = W = 256
	rec = dict(image=[H, W], reps=args.reps)
	L = _lib.lib()
	for B in args.sizes:
		gen = torch.Generator(device=dev).manual_seed(B)
		p = (torch.randn(B, H, W, 3, device=dev, generator=gen) * 0.7).requires_grad_(True)
		t = torch.randn(B, H, W, 3, device=dev, generator=gen) * 2
		w = torch.rand(B, H, W, device=dev, generator=gen)
		w = torch.where(w < 0.3, torch.zeros_like(w), w)
		P = B * H * W
		out = dict(pixels=P, map_MB=round(P * 12 / 2 ** 20, 1))

		def built():
			p.grad = None
			FN.normal_loss(p, t, w).backward()
		out['built'] = timed(built, args.reps)

		def ref():
			p.grad = None
			composition(p, t, w)
		out['torch_composition'] = timed(ref, args.reps)
		out['built_over_torch'] = round(out['built']['median_ms'] / out['torch_composition']['median_ms'], 3)
		# the two paths agree
		built()
		gp, lb = p.grad.clone(), FN.normal_loss(p, t, w).item()
		p.grad = None
		out['loss_built'], out['loss_torch'] = lb, composition(p, t, w).item()
		out['max_abs_diff_d_pred'] = float((gp - p.grad).abs().max())
		out['max_abs_d_pred'] = float(gp.abs().max())
		p.grad = None
		# each kernel alone
		s = current_stream(dev)
		pd = p.detach()
		ws = torch.empty(L.find_normal_loss_ws_bytes(P) // 8, dtype=torch.float64, device=dev)
		loss, one, dp = torch.empty((), device=dev), torch.ones((), device=dev), torch.empty_like(pd)
		ms = kernel_ms(lambda: check(L.find_normal_loss_fwd(ptr(pd), ptr(t), ptr(w), P, ptr(loss), ptr(ws), ws.numel() * 8, s), 'find_normal_loss_fwd'),
					   args.launches)
		nbytes = P * 28   # pred, target, weight in
		out['fwd_kernels'] = dict(ms=round(ms, 4), bytes=nbytes, TB_per_s=round(nbytes / ms / 1e9, 3))
		ms = kernel_ms(lambda: check(L.find_normal_loss_bwd(ptr(pd), ptr(t), ptr(w), P, ptr(one), ptr(ws), ptr(dp), s), 'find_normal_loss_bwd'),
					   args.launches)
		nbytes = P * 40   # pred, target, weight in; d pred out
		out['bwd_kernel'] = dict(ms=round(ms, 4), bytes=nbytes, TB_per_s=round(nbytes / ms / 1e9, 3))
		rec[f'B{B}'] = out
		del p, t, w, pd, dp, gp
		torch.cuda.empty_cache()
	line = json.dumps(rec)
	print(line, flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as fh:
		fh.write(line + '\n')


if __name__ == '__main__':
	main()
