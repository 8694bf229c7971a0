"""Cost of the tape girths: find_amd.girth.section_hulls (forward, and forward + backward to the vertices and the planes) against
find_amd.measure.plane_sections at the same shapes -- the same pass over the faces, without the hull -- and against what a user did before:
the crossing points computed in torch on the device, downloaded, and hulled on the host by scipy.spatial.ConvexHull, section by section.
16 feet of the arched 6 890-vertex template (13 776 faces), jittered as in tests/test_gpu_girth.py, with 2 and with 64 planes normal to the
length axis.  Device events around --launches calls after --warmup calls of the same shape; the device paths alternate, --reps rounds each,
median with range.  The host path is timed by the host clock around whole calls that end with the data on the host (--host-reps of them).
One JSON line, also written to --out (default profiles/girth_cost.json).

	python tools/girth_cost.py [--reps 5] [--launches 20] [--warmup 3] [--host-reps 2] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def event_ms(fn, launches):
	a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	a.record()
	for _ in range(launches):
		fn()
	b.record()
	b.synchronize()
	return a.elapsed_time(b) / launches


def host_hulls(verts, faces, planes):
	"""Every section's hull perimeter by the host: crossing points in torch on the device (tests/girth_ref.py's formulation), one download per
	section, scipy's Qhull on the plane's 2-D coordinates."""
	from girth_ref import basis, crossing_points
	from scipy.spatial import ConvexHull
	out = np.zeros(planes.shape[:2])
	for n in range(verts.shape[0]):
		for k in range(planes.shape[1]):
			p = crossing_points(verts[n], faces, planes[n, k])[0].cpu()
			if p.shape[0] < 3:
				continue
			e1, e2 = basis(planes[n, k, :3].cpu())
			xy = torch.stack([p @ e1, p @ e2], 1).numpy()
			h = p[torch.from_numpy(ConvexHull(xy).vertices.astype(np.int64))]
			out[n, k] = float((h - h.roll(-1, 0)).norm(dim=1).sum())
	return out


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--launches', type=int, default=20)
	ap.add_argument('--warmup', type=int, default=3)
	ap.add_argument('--host-reps', type=int, default=2)
	ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'girth_cost.json'))
	args = ap.parse_args()
	from girth_ref import arched
	from find_amd import synthetic
	from find_amd.girth import section_hulls
	from find_amd.measure import plane_sections
	dev = torch.device('cuda', 0)
	n_feet = 16
	v, f = synthetic.template(6890)
	v = arched(v)
	g = torch.Generator().manual_seed(6890)
	verts = v[None] * (0.8 + 0.4 * torch.rand(n_feet, 1, 3, generator=g)) + 0.002 * v.abs().max() * torch.randn(n_feet, v.shape[0], 3, generator=g)
	verts = verts.to(dev).requires_grad_()
	faces = f.to(dev)
	rec = dict(feet=n_feet, faces=int(f.shape[0]), launches=args.launches, reps=args.reps)
	for n_planes in (2, 64):
		frac = torch.tensor([0.68, 0.50] if n_planes == 2 else np.linspace(0.1, 0.9, n_planes).tolist())
		x = verts.detach()[:, :, 0]
		d = x.amin(1, keepdim=True) + frac.to(dev)[None] * (x.amax(1, keepdim=True) - x.amin(1, keepdim=True))
		planes = torch.cat([torch.tensor([1., 0., 0.], device=dev).expand(n_feet, n_planes, 3), d[..., None]], -1).contiguous().requires_grad_()
		weight = torch.rand(n_feet, n_planes, generator=g).to(dev) + 0.5

		def both(op, **kw):
			def fn():
				verts.grad = planes.grad = None
				(op(verts, faces, planes, **kw) * weight).sum().backward()
			return fn

		def fwd(op, **kw):
			def fn():
				with torch.no_grad():
					op(verts, faces, planes, **kw)
			return fn
		paths = dict(hulls_forward=fwd(section_hulls), hulls_forward_backward=both(section_hulls), hulls_forward_max_points_1024=fwd(section_hulls, max_points=1024),
					 sections_forward=fwd(plane_sections), sections_forward_backward=both(plane_sections))
		peak = {}
		for name, fn in paths.items():
			for _ in range(args.warmup):
				fn()
			verts.grad = planes.grad = None
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
		r = {name: dict(median_ms=round(float(np.median(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4), peak_extra_MB=peak[name]) for name, t in times.items()}
		host = []
		with torch.no_grad():
			for _ in range(args.host_reps):
				torch.cuda.synchronize()
				t0 = time.perf_counter()
				on_host = host_hulls(verts.detach(), faces, planes.detach())
				host.append((time.perf_counter() - t0) * 1e3)
			girth, n_hull, count, status, _ = section_hulls(verts, faces, planes, return_hull=True)
		r['host_scipy'] = dict(median_ms=round(float(np.median(host)), 2), min_ms=round(min(host), 2), max_ms=round(max(host), 2))
		r['hulls_over_sections_forward'] = round(r['hulls_forward']['median_ms'] / r['sections_forward']['median_ms'], 2)
		r['hulls_over_sections_forward_backward'] = round(r['hulls_forward_backward']['median_ms'] / r['sections_forward_backward']['median_ms'], 2)
		r['host_over_hulls_forward'] = round(r['host_scipy']['median_ms'] / r['hulls_forward']['median_ms'], 1)
		r['crossing_faces'] = [int(count.min()), int(count.max())]
		r['corners'] = [int(n_hull.min()), int(n_hull.max())]
		r['status_nonzero'] = int((status != 0).sum())
		r['largest_relative_difference_to_host'] = float(np.abs(girth.cpu().numpy() - on_host).max() / on_host.max())
		rec[f'P{n_planes}'] = r
	line = json.dumps(rec)
	print(line, flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as fh:
		fh.write(line + '\n')


if __name__ == '__main__':
	main()
