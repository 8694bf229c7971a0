"""Cost of the skinned model's decode: find_skin_fwd + find_skin_bwd (through FN.linear_blend_skinning and autograd) against the torch
restatement of the same definition (tests/skin_ref.py, fp32, on the GPU: the kinematic tree as a Python loop, (N, V, 3, 3) temporaries,
einsums -- what the op would be without a kernel), forward + backward, on a synthetic model of 6890 vertices and 24 joints with 10 shape
directions, 16 feet.  The two C calls are also timed alone.  Median of --reps timings of --iters iterations each, HIP events on the current
stream.  One JSON line.  Run by hand; nothing gates on it.

	python tools/skin_cost.py [--iters 20] [--reps 5] [--feet 16] [--verts 6890] [--joints 24] [--betas 10]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def timed(fn, iters, reps):
	for _ in range(3):
		fn()
	torch.cuda.synchronize()
	times = []
	for _ in range(reps):
		a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		a.record()
		for _ in range(iters):
			fn()
		b.record()
		b.synchronize()
		times.append(a.elapsed_time(b) / iters)
	return float(np.median(times))


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--iters', type=int, default=20)
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--feet', type=int, default=16)
	ap.add_argument('--verts', type=int, default=6890)
	ap.add_argument('--joints', type=int, default=24)
	ap.add_argument('--betas', type=int, default=10)
	args = ap.parse_args()
	import skin_ref
	from find_amd import functional as FN
	from find_amd import skinning as SK
	from find_amd import synthetic
	from find_amd._lib import current_stream, lib, ptr
	from find_amd.model import _skin_arrays
	dev = torch.device('cuda', 0)
	N, V, J, B = args.feet, args.verts, args.joints, args.betas
	consts = {k: v.to(dev) for k, v in _skin_arrays(synthetic.skinned_model(V=V, J=J, B=B, chain='tree', seed=0), B).items() if k != 'faces'}
	P = consts['dirs'].shape[1] - B
	g = torch.Generator().manual_seed(1)
	pose = (torch.randn(N, 3 * J, generator=g) * 0.3).to(dev).requires_grad_(True)
	betas = torch.randn(N, B, generator=g).to(dev).requires_grad_(True)
	trans = (torch.randn(N, 3, generator=g) * 0.1).to(dev).requires_grad_(True)
	d_out = torch.randn(N, V, 3, generator=g).to(dev)

	def hip():
		torch.autograd.grad(FN.linear_blend_skinning(consts, pose, betas, trans), (pose, betas, trans), d_out)

	def restated():
		torch.autograd.grad(skin_ref.skin(consts, pose, betas, trans, torch.float32), (pose, betas, trans), d_out)

	a = torch.autograd.grad(FN.linear_blend_skinning(consts, pose, betas, trans), (pose, betas, trans), d_out)
	b = torch.autograd.grad(skin_ref.skin(consts, pose, betas, trans, torch.float32), (pose, betas, trans), d_out)
	agree = max(((x - y).abs().max() / y.abs().max()).item() for x, y in zip(a, b))
	L = lib()
	c = [ptr(consts[k]) for k in SK.SKIN_CONSTS]
	out, d_pose, d_betas, d_trans = (torch.empty_like(t) for t in (d_out, pose, betas, trans))
	ws = torch.empty(L.find_skin_bwd_ws_bytes(N, V, J, B, P), dtype=torch.uint8, device=dev)
	s = current_stream(dev)
	fwd = lambda: L.find_skin_fwd(*c, V, J, B, P, ptr(pose), ptr(betas), ptr(trans), N, ptr(out), None, ptr(ws), ws.numel(), s)
	bwd = lambda: L.find_skin_bwd(*c, V, J, B, P, ptr(pose), ptr(betas), ptr(d_out), N, ptr(d_pose), ptr(d_betas), ptr(d_trans), ptr(ws), ws.numel(), s)
	assert fwd() == 0 and bwd() == 0
	t_hip = timed(hip, args.iters, args.reps)
	t_ref = timed(restated, args.iters, args.reps)
	t_fwd = timed(fwd, args.iters * 10, args.reps)
	t_bwd = timed(bwd, args.iters * 10, args.reps)
	print(json.dumps(dict(feet=N, verts=V, joints=J, betas=B, pose_features=P, hip_fwd_bwd_us=round(t_hip * 1e3, 1), torch_fwd_bwd_us=round(t_ref * 1e3, 1),
						  speedup=round(t_ref / t_hip, 2), skin_fwd_us=round(t_fwd * 1e3, 2), skin_bwd_us=round(t_bwd * 1e3, 2),
						  worst_relative_gradient_difference=float(f'{agree:.3e}'))), flush=True)


if __name__ == '__main__':
	main()
