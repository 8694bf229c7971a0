"""Cost of the foot measurements: forward + backward of find_amd.measure.foot_measurements (one find_extents_fwd, one
find_plane_sections_fwd, their backward passes and the torch glue between them) against the same measurements restated in torch on the same
device in fp32 -- max / min for the extents, tests/measure_ref.py's vectorised `where` formulation over (N, P, F) for the sections, autograd
for the backward -- on 16 feet of the 6 890- and the 50 002-vertex templates (13 776 and 100 000 faces), with 2 and 16 girth planes.
Device events around --launches calls, after --warmup calls of the same shape; the two paths alternate, --reps rounds each, median with
range.  Peak extra memory: torch.cuda.max_memory_allocated over one forward + backward, less what was allocated before it.
One JSON line, also written to --out (default profiles/measure_cost.json).

	python tools/measure_cost.py [--reps 5] [--launches 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def torch_foot_measurements(verts, faces, spec):
	"""foot_measurements in torch ops, in the dtype and on the device of verts."""
	from measure_ref import plane_sections_ref
	dirs = torch.tensor([spec.length_axis, spec.width_axis], device=verts.device, dtype=verts.dtype)
	s = verts @ dirs.T
	lo, hi = s.amin(1), s.amax(1)
	size = hi - lo
	frac = torch.tensor([f for _, f in spec.girths], device=verts.device, dtype=verts.dtype)
	d = lo[:, :1] + frac[None] * size[:, :1]
	planes = torch.cat([dirs[0].expand(verts.shape[0], frac.shape[0], 3), d[..., None]], -1)
	return torch.cat([size, plane_sections_ref(verts, faces, planes)[0]], 1)


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
	ap.add_argument('--launches', type=int, default=20)
	ap.add_argument('--warmup', type=int, default=3)
	ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'measure_cost.json'))
	args = ap.parse_args()
	from find_amd import synthetic
	from find_amd.measure import FootSpec, foot_measurements
	dev = torch.device('cuda', 0)
	n_feet = 16
	rec = dict(feet=n_feet, launches=args.launches, reps=args.reps)
	for n_verts in (6890, 50002):
		v, f = synthetic.template(n_verts)
		g = torch.Generator().manual_seed(n_verts)
		verts = (v[None] * (0.9 + 0.2 * torch.rand(n_feet, 1, 3, generator=g))).to(dev).requires_grad_()
		faces = f.to(dev)
		for n_planes in (2, 16):
			spec = FootSpec() if n_planes == 2 else FootSpec(girths=tuple((f'g{k}', float(x)) for k, x in enumerate(np.linspace(0.2, 0.8, n_planes))))
			weight = torch.rand(n_feet, 2 + n_planes, generator=g).to(dev) + 0.5

			def hip():
				verts.grad = None
				(foot_measurements(verts, faces, spec)[0] * weight).sum().backward()

			def restated():
				verts.grad = None
				(torch_foot_measurements(verts, faces, spec) * weight).sum().backward()

			def hip_fwd():
				with torch.no_grad():
					foot_measurements(verts, faces, spec)
			paths = dict(hip=hip, torch=restated, hip_forward_only=hip_fwd)
			peak = {}
			for name, fn in paths.items():
				for _ in range(args.warmup):
					fn()
				verts.grad = None
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
				a, b = foot_measurements(verts, faces, spec)[0], torch_foot_measurements(verts, faces, spec)
				agree = float(((a - b).abs() / b.abs()).max())
			r = {name: dict(median_ms=round(float(np.median(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4), peak_extra_MB=peak[name]) for name, t in times.items()}
			r['torch_over_hip'] = round(r['torch']['median_ms'] / r['hip']['median_ms'], 2)
			r['mesh_MB'] = round((n_feet * n_verts * 12 + f.shape[0] * 12) / 2 ** 20, 2)
			r['largest_relative_difference'] = agree
			rec[f'V{n_verts}_P{n_planes}'] = r
	line = json.dumps(rec)
	print(line, flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as fh:
		fh.write(line + '\n')


if __name__ == '__main__':
	main()
