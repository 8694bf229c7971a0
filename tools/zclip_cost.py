"""Cost of the z-clip split mode (make_params(clip_faces=True)): render forward + backward (mask and image losses) at the C3 shape
(16 feet x 4 views @256^2) and the C4 shape (@512^2) on the 6890-vertex template, default mode against split mode, once with no face
crossing the plane (cameras 0.3 m out) and once with half the views inside the mesh (0.02 m).  Median of --reps timings of --iters
iterations each, HIP events on the current stream.  One JSON line per (shape, scene, mode).

	python tools/zclip_cost.py [--iters 20] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--iters', type=int, default=20)
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--feet', type=int, default=16)
	args = ap.parse_args()
	from find_amd import functional_render as FR
	from find_amd import synthetic
	from find_amd.cameras import look_at_view_transform
	dev = torch.device('cuda', 0)
	v, f = synthetic.template(6890)
	g = torch.Generator().manual_seed(0)
	verts = (v[None] * (1 + 0.05 * torch.rand(args.feet, 1, 3, generator=g))).to(dev).requires_grad_(True)
	cols = torch.rand(args.feet, v.shape[0], 3, generator=g).to(dev).requires_grad_(True)
	faces = f.to(dev)
	elev, azim = np.array([0.0, 30.0, -45.0, 60.0]), np.array([0.0, 90.0, 180.0, 270.0])
	scenes = {'clean': np.full(4, 0.3), 'inside': np.array([0.3, 0.02, 0.3, 0.02])}
	for size, shape in ((256, 'C3'), (512, 'C4')):
		for scene, dist in scenes.items():
			R, T = look_at_view_transform(dist=dist, elev=elev, azim=azim, up=((1, 0, 0),))
			R, T = R.to(dev).float(), T.to(dev).float()
			res = {}
			for clip in (False, True):
				params = FR.make_params(size, clip_faces=clip)

				def step():
					mask, image, _, _ = FR.render(verts, cols, faces, R, T, params)
					(mask.sum() + image.sum()).backward()
				with FR.flag_policy('ignore'):
					for _ in range(3):
						step()
					torch.cuda.synchronize()
					times = []
					for _ in range(args.reps):
						a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
						a.record()
						for _ in range(args.iters):
							step()
						b.record()
						b.synchronize()
						times.append(a.elapsed_time(b) / args.iters)
				res['split' if clip else 'default'] = times
			md, ms = float(np.median(res['default'])), float(np.median(res['split']))
			print(json.dumps({'shape': shape, 'size': size, 'feet': args.feet, 'views': 4, 'scene': scene, 'default_ms': round(md, 4),
							  'split_ms': round(ms, 4), 'overhead': round(ms / md - 1.0, 4), 'default_all': [round(t, 4) for t in res['default']],
							  'split_all': [round(t, 4) for t in res['split']]}), flush=True)


if __name__ == '__main__':
	main()
