"""Cost of fitting to depth, forward + backward, at B = 5 (one foot x five views) and B = 80 (16 feet x 5 views) depth maps of 256^2 of the
6890-vertex template, timed two ways on the same tensors and the same device:
  built  FootRenderer(..., return_depth=True) (functional.depth_map) + functional.depth_loss -- find_depth_bwd, find_depth_loss_fwd / _bwd;
  torch  the composition a user would write on the same raster pass: the ray-plane depth of every covered pixel by a torch gather of its
         face's corners (the formula of find_depth_bwd's forward), a masked l1 mean on the two maps, and autograd's backward of both.
Both include the raster pass (render_no_grad times it alone).  Host clock around work that ends in a device synchronise; one warm-up, then
the median of --reps repeats with their range.  The kernels are also timed alone (device events around --launches launches on preallocated
buffers): find_depth_bwd with its atomic bytes per second (36 bytes per covered pixel) beside the chip-wide float-atomic rate of ~1.3 TB/s
(DESIGN 7.6), the loss kernels with the bytes they must move.  One JSON line, also written to --out (default profiles/depth_loss_cost.json).

	python tools/depth_loss_cost.py [--reps 5] [--launches 10] [--out FILE]"""
import argparse
import ctypes
import json
import math
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


def torch_depth(verts, faces, R, T, p2f, fov_deg=60.0):
	"""(N, M, H, W) depth from the selection p2f by torch ops: z = (n . p0) / (n . d) on the covered pixels, -1 elsewhere."""
	N, M, H, W = p2f.shape
	F = faces.shape[0]
	s = 1.0 / math.tan(math.radians(fov_deg) / 2)
	flat = p2f.reshape(N * M, H, W)
	img, yi, xi = torch.nonzero(flat >= 0, as_tuple=True)
	f = (flat[img, yi, xi] - img * F).long()
	mesh, view = img // M, img % M
	fv = faces.long()[f]
	p = torch.einsum('pki,pij->pkj', verts[mesh[:, None], fv], R[view]) + T[view][:, None, :]
	d = torch.stack([(1 - (2 * xi.float() + 1) / W) / s, (1 - (2 * yi.float() + 1) / H) / s, torch.ones_like(xi, dtype=torch.float32)], dim=1)
	n = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
	z = (n * p[:, 0]).sum(1) / (n * d).sum(1)
	return torch.full((N * M, H, W), -1.0, device=verts.device).index_put((img, yi, xi), z).reshape(N, M, H, W)


def masked_l1(p, t, trunc):
	r = p - t
	valid = ((p > 0) & (t > 0) & (r.abs() <= trunc)).float()
	return (valid * r.abs()).sum() / valid.sum().clamp(min=1e-12)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--launches', type=int, default=10)
	ap.add_argument('--feet', type=int, nargs='+', default=[1, 16])
	ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'depth_loss_cost.json'))
	args = ap.parse_args()
	from find_amd import _lib, functional as FN, functional_render as FR, synthetic
	from find_amd._lib import check, current_stream, ptr
	from find_amd.renderer import FootRenderer
	from find_amd.structures import Meshes
	dev = torch.device('cuda', 0)
	size, M, trunc = 256, 5, 0.02
	rdr = FootRenderer(image_size=size, device=dev)
	R, T = rdr.sample_views(nviews=M, dist_mean=0.3, dist_std=0, elev_min=-90, elev_max=90, azim_min=-90, azim_max=90, seed=5)
	R, T = R.to(dev).float().contiguous(), T.to(dev).float().contiguous()
	v, f = synthetic.template(6890)
	f = f.to(dev).to(torch.int32).contiguous()
	rec = dict(image=[size, size], views=M, verts=v.shape[0], faces=f.shape[0], reps=args.reps, atomic_rate_TB_per_s_guide=1.3)
	L = _lib.lib()
	for N in args.feet:
		B = N * M
		g = torch.Generator().manual_seed(N)
		gt_v = (v[None] * (1 + 0.08 * torch.rand(N, 1, 3, generator=g))).to(dev)
		x = (gt_v + 0.002 * torch.randn(gt_v.shape, generator=g).to(dev)).requires_grad_(True)
		with torch.no_grad():
			gt = rdr(Meshes(gt_v, f), R, T, return_images=False, return_depth=True)['depth']
		out = dict(maps=B, pixels=B * size * size)

		def built():
			x.grad = None
			depth = rdr(Meshes(x, f), R, T, return_images=False, return_depth=True)['depth']
			loss = FN.depth_loss(depth.reshape(B, -1), gt.reshape(B, -1), kind='l1', trunc=trunc)
			loss.backward()
			return loss
		out['built'] = timed(built, args.reps)

		def ref():
			x.grad = None
			with torch.no_grad():
				_, _, p2f, _ = FR.render(x, None, f, R, T, rdr.params, want_mask=False, want_image=False, want_frags=True)
			loss = masked_l1(torch_depth(x, f, R, T, p2f), gt, trunc)
			loss.backward()
			return loss
		out['torch_composition'] = timed(ref, args.reps)
		out['built_over_torch'] = round(out['built']['median_ms'] / out['torch_composition']['median_ms'], 3)

		def render_only():
			with torch.no_grad():
				rdr(Meshes(x, f), R, T, return_images=False, return_depth=True)
		out['render_no_grad'] = timed(render_only, args.reps)
		# the two paths agree
		lb = built().item()
		gb = x.grad.clone()
		lt = ref().item()
		out['loss_built'], out['loss_torch'] = lb, lt
		out['max_abs_diff_d_verts'] = float((gb - x.grad).abs().max())
		out['max_abs_d_verts'] = float(gb.abs().max())
		x.grad = None
		# each kernel alone
		s = current_stream(dev)
		xd = x.detach()
		_, _, p2f, zbuf = FR.render(xd, None, f, R, T, rdr.params, want_mask=False, want_image=False, want_frags=True)
		covered = int((p2f >= 0).sum())
		out['covered_pixels'] = covered
		up, dv = torch.randn(zbuf.shape, device=dev), torch.empty_like(xd)
		ms = kernel_ms(lambda: check(L.find_depth_bwd(ctypes.byref(rdr.params), ptr(xd), ptr(f), 1, ptr(R), ptr(T), N, M, xd.shape[1], f.shape[0],
													  ptr(p2f), ptr(up), ptr(dv), s), 'find_depth_bwd'), args.launches)
		out['depth_bwd'] = dict(ms=round(ms, 4), atomic_bytes=covered * 36, atomic_TB_per_s=round(covered * 36 / ms / 1e9, 4))
		P = size * size
		pr, tg = zbuf.reshape(B, P), gt.reshape(B, P)
		ws = torch.empty(L.find_depth_loss_ws_bytes(B, P) // 8, dtype=torch.float64, device=dev)
		loss, one, dp = torch.empty((), device=dev), torch.ones((), device=dev), torch.empty_like(pr)
		ms = kernel_ms(lambda: check(L.find_depth_loss_fwd(ptr(pr), ptr(tg), None, B, P, 0, 0.005, trunc, ptr(loss), None, ptr(ws), ws.numel() * 8, s),
									 'find_depth_loss_fwd'), args.launches)
		out['loss_fwd_kernels'] = dict(ms=round(ms, 4), bytes=B * P * 8, TB_per_s=round(B * P * 8 / ms / 1e9, 3))
		ms = kernel_ms(lambda: check(L.find_depth_loss_bwd(ptr(pr), ptr(tg), None, B, P, 0, 0.005, trunc, ptr(one), ptr(ws), ptr(dp), s),
									 'find_depth_loss_bwd'), args.launches)
		out['loss_bwd_kernel'] = dict(ms=round(ms, 4), bytes=B * P * 12, TB_per_s=round(B * P * 12 / ms / 1e9, 3))
		rec[f'B{B}'] = out
		del x, gt_v, gt, gb, p2f, zbuf, up, dv, pr, tg, dp
		torch.cuda.empty_cache()
	line = json.dumps(rec)
	print(line, flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as fh:
		fh.write(line + '\n')


if __name__ == '__main__':
	main()
