"""Cost of the PCA baseline's step and the share of it that the decode kernels take: 16 feet x 6890 vertices (synthetic template) x B in
{10, 100}.  The step is the latent / registration stage's forward + backward through find_amd.ModelWithLoss(model_type='pca'): decode,
registration, Chamfer (5000 samples per foot) and smoothness, eagerly, without an optimiser step.  find_pca_fwd and find_pca_bwd are
timed alone on the same sizes.  Median of --reps timings of --iters iterations each, HIP events on the current stream.  One JSON line per B.

	python tools/pca_cost.py [--iters 20] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
	args = ap.parse_args()
	from find_amd import synthetic
	from find_amd._lib import current_stream, lib, ptr
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	from find_amd.structures import Meshes, TexturesVertex
	from find_amd.train_utils import sample_latent_vectors
	dev = torch.device('cuda', 0)
	N = args.feet
	v, f = synthetic.template(6890)
	V = v.shape[0]
	gv, gf = synthetic.ellipsoid_mesh(40, 60)
	L = lib()
	for B in (10, 100):
		g = torch.Generator().manual_seed(B)
		sd = dict(template_verts=v[None].float(), template_faces=f[None].long(), pca_var=torch.ones(B, 1),
				  pca_coefs=torch.randn(V, B, 3, generator=g) * 0.002)
		mwl = ModelWithLoss(opts=Opts(model_type='pca'), device=dev, train_size=N, val_size=1)
		m = mwl.model
		m.configure_template(sd, device=dev)
		m.load_state_dict(sd, strict=False)
		m.configure_params()
		with torch.no_grad():
			m.shapevec.data.copy_(torch.randn(N, B, generator=g).to(dev))
		opts = Opts(model_type='pca')
		scan = gv[None].expand(N, -1, -1).contiguous().to(dev)
		batch = dict(mesh=Meshes(scan, gf.to(dev), TexturesVertex(torch.full_like(scan, 0.5))), idx=torch.arange(N, device=dev))

		def step():
			b = dict(batch)
			b.update(sample_latent_vectors(b, m.latent_vectors_train))
			loss, _ = mwl(b, 0, opts, chamf=True, smooth=True)
			loss.backward()

		coefs, sv = m.pca_coefs.data, m.shapevec.data
		off = torch.empty(N, V, 3, device=dev)
		d_sv = torch.empty(N, B, device=dev)
		d_off = torch.randn(N, V, 3, device=dev)
		ws = torch.empty(L.find_pca_bwd_ws_bytes(N, V, B), dtype=torch.uint8, device=dev)
		s = current_stream(dev)
		fwd = lambda: L.find_pca_fwd(ptr(coefs), V, B, ptr(sv), N, ptr(off), s)
		bwd = lambda: L.find_pca_bwd(ptr(coefs), V, B, ptr(d_off), N, ptr(d_sv), ptr(ws), ws.numel(), s)
		assert fwd() == 0 and bwd() == 0
		t_step = timed(step, args.iters, args.reps)
		t_fwd = timed(fwd, args.iters * 10, args.reps)
		t_bwd = timed(bwd, args.iters * 10, args.reps)
		floor_us = 12.0 * V * B / 8e12 * 1e6   # coefficient bytes once at a nominal 8 TB/s
		print(json.dumps(dict(feet=N, verts=V, B=B, step_ms=round(t_step, 4), pca_fwd_us=round(t_fwd * 1e3, 2), pca_bwd_us=round(t_bwd * 1e3, 2),
							  decode_share_of_step=round((t_fwd + t_bwd) / t_step, 4), coef_bytes=12 * V * B, coef_read_floor_us=round(floor_us, 2))), flush=True)


if __name__ == '__main__':
	main()
