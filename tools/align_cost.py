"""Cost of the alignment: find_amd.align.iterative_closest_point (one find_icp_run call: max_iterations + 1 rounds of apply, find_nn_fwd,
moments and solve, nothing read back) against the same loop restated in torch on the same device in fp32 -- torch.cdist + argmin for the
match, the centred cross-covariance and torch.linalg.svd for the solve (on the device; on the host if ROCm's batched SVD is unavailable,
which the record says), the same number of rounds and no convergence test, so neither path reads anything back either -- on 1 x 5000 and
16 x 5000 samples of a moved copy of a cloud in a foot-sized box, untrimmed and with trim 0.2 (torch: kthvalue).
Device events around --launches calls, after --warmup calls of the same shape; the two paths alternate, --reps rounds each, median with
range.  One JSON line, also written to --out (default profiles/align_cost.json).

	python tools/align_cost.py [--reps 5] [--launches 5] [--warmup 2] [--iterations 20] [--out FILE]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SVD_ON_HOST = False


def _svd(H):
	global SVD_ON_HOST
	if not SVD_ON_HOST:
		try:
			return torch.linalg.svd(H)
		except RuntimeError:
			SVD_ON_HOST = True
	U, D, Vt = torch.linalg.svd(H.cpu())
	return U.to(H.device), D.to(H.device), Vt.to(H.device)


def torch_icp(X, Y, rounds, estimate_scale=False, trim=0.):
	"""rounds updates of the absolute transform, then one more match; returns (R, T, s, rmse)."""
	N, P, _ = X.shape
	R = torch.eye(3, device=X.device).expand(N, 3, 3).contiguous()
	T = torch.zeros(N, 3, device=X.device)
	s = torch.ones(N, device=X.device)
	k = P - int(math.floor(trim * P))
	for rnd in range(rounds + 1):
		Xt = s[:, None, None] * torch.bmm(X, R) + T[:, None]
		d2, idx = (torch.cdist(Xt, Y) ** 2).min(dim=2)
		w = torch.ones_like(d2) if trim == 0 else (d2 <= d2.kthvalue(k, dim=1, keepdim=True).values).float()
		rmse = ((w * d2).sum(1) / w.sum(1)).sqrt()
		if rnd == rounds:
			break
		Ym = torch.gather(Y, 1, idx[..., None].expand(-1, -1, 3))
		sw = w.sum(1, keepdim=True)
		mx, my = (w[..., None] * X).sum(1) / sw, (w[..., None] * Ym).sum(1) / sw
		Xc, Yc = X - mx[:, None], Ym - my[:, None]
		U, D, Vt = _svd(torch.bmm((w[..., None] * Xc).transpose(1, 2), Yc))
		E = torch.ones(N, 3, device=X.device)
		E[:, 2] = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
		R = torch.bmm(U * E[:, None], Vt)
		if estimate_scale:
			s = (D * E).sum(1) / (w * (Xc * Xc).sum(-1)).sum(1)
		T = my - s[:, None] * torch.bmm(mx[:, None], R)[:, 0]
	return R, T, s, rmse


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
	ap.add_argument('--launches', type=int, default=5)
	ap.add_argument('--warmup', type=int, default=2)
	ap.add_argument('--iterations', type=int, default=20)
	ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'align_cost.json'))
	args = ap.parse_args()
	from find_amd.align import iterative_closest_point
	dev = torch.device('cuda', 0)
	P = 5000
	rec = dict(samples=P, iterations=args.iterations, launches=args.launches, reps=args.reps)
	g = torch.Generator().manual_seed(5)
	for n_feet in (1, 16):
		X = (torch.rand(n_feet, P, 3, generator=g) * torch.tensor([0.25, 0.10, 0.08])).to(dev)
		ang = math.radians(6)
		R0 = torch.tensor([[math.cos(ang), math.sin(ang), 0.], [-math.sin(ang), math.cos(ang), 0.], [0., 0., 1.]], device=dev)
		Y = ((X @ R0) + torch.tensor([0.004, -0.003, 0.002], device=dev))[:, torch.randperm(P, generator=g).to(dev)].contiguous()
		for tag, kw in (('rigid', {}), ('trim0.2_scale', dict(trim=0.2, estimate_scale=True))):
			# relative_rmse_thr 0 never stops before the rmse repeats to the bit; both paths run every round either way
			paths = dict(hip=lambda kw=kw: iterative_closest_point(X, Y, max_iterations=args.iterations, relative_rmse_thr=0., **kw),
						 torch=lambda kw=kw: torch_icp(X, Y, args.iterations, **kw))
			for fn in paths.values():
				for _ in range(args.warmup):
					fn()
			torch.cuda.synchronize()
			times = {name: [] for name in paths}
			for _ in range(args.reps):
				for name, fn in paths.items():
					times[name].append(event_ms(fn, args.launches))
			a, b = paths['hip'](), paths['torch']()
			r = {name: dict(median_ms=round(float(np.median(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4)) for name, t in times.items()}
			r['torch_over_hip'] = round(r['torch']['median_ms'] / r['hip']['median_ms'], 2)
			r['hip_ms_per_round'] = round(r['hip']['median_ms'] / (args.iterations + 1), 4)
			r['largest_difference_R'] = float((a.RTs.R - b[0]).abs().max())
			r['rmse_hip'], r['rmse_torch'] = float(a.rmse.max()), float(b[3].max())
			rec[f'N{n_feet}_{tag}'] = r
	rec['torch_svd_on_host'] = SVD_ON_HOST
	line = json.dumps(rec)
	print(line, flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as fh:
		fh.write(line + '\n')


if __name__ == '__main__':
	main()
