"""Cost of the structural term: forward + backward of find_amd.ssim.ssim (find_ssim_fwd / _bwd, one pass each way) against its restatement
in torch on the same device -- permuted copies of the masked images, F.conv2d with groups = C for the five window means (the row pass, then
the column pass), the formula as elementwise kernels, autograd for the backward -- on 64 images (16 feet x 4 views) of 256^2 and 512^2,
C = 3, both masks, border 'same', gradients to the prediction and its mask.
Device events around --launches calls, after --warmup calls of the same shape; the two paths alternate, --reps rounds each, median with
range.  Peak extra memory: torch.cuda.max_memory_allocated over one forward + backward, less what was allocated before it (the inputs).
One JSON line, also written to --out (default profiles/ssim_cost.json).

	python tools/ssim_cost.py [--reps 5] [--launches 50] [--warmup 5] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_ssim(x, y, xm, ym, window):
	"""The definition in torch ops: x, y (n, H, W, C), masks (n, H, W); border 'same', data_range 1."""
	C = x.shape[-1]
	a, b = (x * xm[..., None]).permute(0, 3, 1, 2), (y * ym[..., None]).permute(0, 3, 1, 2)
	wr, wc = window.view(1, 1, 1, -1).expand(C, 1, 1, -1), window.view(1, 1, -1, 1).expand(C, 1, -1, 1)

	def blur(t):
		return F.conv2d(F.conv2d(t, wr, padding=(0, 5), groups=C), wc, padding=(5, 0), groups=C)
	m1, m2, s11, s22, s12 = blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b)
	c1, c2 = 0.01 ** 2, 0.03 ** 2
	num = (2 * m1 * m2 + c1) * (2 * (s12 - m1 * m2) + c2)
	den = (m1 * m1 + m2 * m2 + c1) * ((s11 - m1 * m1) + (s22 - m2 * m2) + c2)
	return (num / den).mean()


def event_ms(fn, launches):
	a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	a.record()
	for _ in range(launches):
		fn()
	b.record()
	b.synchronize()
	return a.elapsed_time(b) / launches


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--launches', type=int, default=50)
	ap.add_argument('--warmup', type=int, default=5)
	ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ssim_cost.json'))
	args = ap.parse_args()
	from find_amd.ssim import ssim
	dev = torch.device('cuda', 0)
	d = torch.arange(11, dtype=torch.float64) - 5
	window = torch.exp(-d * d / 4.5)
	window = (window / window.sum()).float().to(dev)
	rec = dict(images=64, channels=3, border='same', launches=args.launches, reps=args.reps)
	for size in (256, 512):
		g = torch.Generator().manual_seed(size)
		low = torch.rand(64, 8, size // 8, size // 8, generator=g)
		full = F.interpolate(low, size=(size, size), mode='bilinear', align_corners=False).to(dev)
		x = full[:, 0:3].permute(0, 2, 3, 1).contiguous().requires_grad_()
		y = full[:, 3:6].permute(0, 2, 3, 1).contiguous()
		xm = full[:, 6].contiguous().requires_grad_()
		ym = full[:, 7].contiguous()
		del full, low

		def hip():
			x.grad = xm.grad = None
			ssim(x, y, xm, ym).backward()

		def restated():
			x.grad = xm.grad = None
			torch_ssim(x, y, xm, ym, window).backward()

		def hip_fwd():
			with torch.no_grad():
				ssim(x, y, xm, ym)
		paths = dict(hip=hip, torch=restated, hip_forward_only=hip_fwd)
		peak = {}
		for name, fn in paths.items():
			for _ in range(args.warmup):
				fn()
			x.grad = xm.grad = None
			torch.cuda.synchronize()
			torch.cuda.reset_peak_memory_stats(dev)
			before = torch.cuda.memory_allocated(dev)
			fn()
			torch.cuda.synchronize()
			peak[name] = round((torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20, 1)
		times = {name: [] for name in paths}
		for _ in range(args.reps):
			for name, fn in paths.items():
				times[name].append(event_ms(fn, args.launches))
		with torch.no_grad():
			agree = abs(float(ssim(x, y, xm, ym)) - float(torch_ssim(x, y, xm, ym, window)))
		r = {name: dict(median_ms=round(float(np.median(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4), peak_extra_MB=peak[name]) for name, t in times.items()}
		r['torch_over_hip'] = round(r['torch']['median_ms'] / r['hip']['median_ms'], 2)
		r['input_MB'] = round(64 * size * size * 8 * 4 / 2 ** 20, 1)
		r['dmaps_MB'] = round(64 * size * size * 9 * 4 / 2 ** 20, 1)
		r['abs_difference_of_the_means'] = agree
		rec[f'{size}x{size}'] = r
	line = json.dumps(rec)
	print(line, flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as fh:
		fh.write(line + '\n')


if __name__ == '__main__':
	main()
