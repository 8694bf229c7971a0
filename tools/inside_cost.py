"""Cost of the winding-number pass (find_winding_fwd) at two sizes, beside a chunked torch restatement of the same definition and beside the
point-to-surface search (find_point_face_fwd) on the same points and meshes:
  training   16 meshes of synthetic.template(6890) (13 776 faces), 5000 box-uniform points each: 1.1 G point-face pairs;
  grid       one mesh, the 128^3 cell centres of its padded box: 2 097 152 points, 28.9 G pairs -- through the C call in one piece, and
             through inside.occupancy_grid, which generates and consumes the points a chunk at a time.
The torch restatement (float32 on the device, the per-face formula of tests/inside_ref.py, a (chunk, F) block at a time, summed in float64)
is timed on --torch-points points of each size and scaled to the whole: it is linear in the points.
Device events around --launches calls in a row (a warm-up call first), repeated --reps times: the median per call with its range, and pairs
per second.  One JSON line, also written to --out (default profiles/inside_cost.json).

	python tools/inside_cost.py [--reps 5] [--launches 5] [--feet 16] [--points 5000] [--res 128] [--out FILE]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn, launches):
	a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	a.record()
	for _ in range(launches):
		fn()
	b.record()
	b.synchronize()
	return a.elapsed_time(b) / launches


def summary(times, pairs, scale=1.):
	med = float(np.median(times)) * scale
	return dict(median_ms=round(med, 4), min_ms=round(min(times) * scale, 4), max_ms=round(max(times) * scale, 4), pairs=pairs, G_pairs_per_s=round(pairs / med / 1e6, 1))


def torch_winding(points, verts, faces, chunk):
	"""w (N, P) float32: the definition in torch, float32 per face, the faces summed in float64, `chunk` points of every mesh at a time."""
	a, b, c = (verts[:, faces[:, k]][:, None] for k in range(3))   # (N, 1, F, 3)
	out = []
	for s in range(0, points.shape[1], chunk):
		p = points[:, s:s + chunk, None]
		A, B, C = a - p, b - p, c - p
		la, lb, lc = A.norm(dim=-1), B.norm(dim=-1), C.norm(dim=-1)
		det = (A * torch.linalg.cross(B, C)).sum(-1)
		den = la * lb * lc + (A * B).sum(-1) * lc + (B * C).sum(-1) * la + (C * A).sum(-1) * lb
		om = torch.where((la == 0) | (lb == 0) | (lc == 0) | (det == 0), torch.zeros_like(det), 2 * torch.atan2(det, den))
		out.append((om.sum(-1, dtype=torch.float64) / (4 * math.pi)).float())
	return torch.cat(out, 1)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--launches', type=int, default=5)
	ap.add_argument('--feet', type=int, default=16)
	ap.add_argument('--points', type=int, default=5000)
	ap.add_argument('--res', type=int, default=128)
	ap.add_argument('--template', type=int, default=6890)
	ap.add_argument('--torch-points', type=int, default=1 << 15)
	ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'inside_cost.json'))
	args = ap.parse_args()
	from find_amd import _lib, inside, synthetic
	from find_amd import functional as FN
	from find_amd._lib import check, current_stream, ptr
	dev = torch.device('cuda', 0)
	L = _lib.lib()
	s = current_stream(dev)
	N, P, res = args.feet, args.points, args.res
	tv, tf = synthetic.template(args.template)
	gen = torch.Generator().manual_seed(0)
	verts = torch.stack([tv * (1 + 0.1 * torch.randn(3, generator=gen)) for _ in range(N)]).to(dev).contiguous()
	faces = tf.to(dev).to(torch.int32).contiguous()
	V, F = verts.shape[1], faces.shape[0]
	lo, hi = verts.amin(1) - 0.02, verts.amax(1) + 0.02
	pts = (lo[:, None] + torch.rand(N, P, 3, generator=gen).to(dev) * (hi - lo)[:, None]).contiguous()
	origin, extent = verts[:1].amin(1) - 0.005, verts[:1].amax(1) - verts[:1].amin(1) + 0.01
	grid = inside.grid_points(origin, extent / res, res, 0, res ** 3).contiguous()
	rec = dict(feet=N, points=P, verts=V, faces=F, res=res, launches=args.launches, reps=args.reps, torch_points=args.torch_points)

	def bare(points, v, n):
		"""The two C calls on preallocated buffers."""
		p = points.shape[1]
		w = torch.empty(n, p, device=dev)
		dist2, idx, bary = torch.empty(n, p, device=dev), torch.empty(n, p, dtype=torch.int32, device=dev), torch.empty(n, p, 3, device=dev)
		ws_w = torch.empty(max(L.find_winding_ws_bytes(n, p, F), 256), dtype=torch.uint8, device=dev)
		ws_p = torch.empty(max(L.find_point_face_ws_bytes(n, p), 256), dtype=torch.uint8, device=dev)

		def winding():
			check(L.find_winding_fwd(ptr(points), None, ptr(v), ptr(faces), 1, n, p, V, F, ptr(w), ptr(ws_w), ws_w.numel(), s), 'find_winding_fwd')

		def point_face():
			check(L.find_point_face_fwd(ptr(points), None, ptr(v), ptr(faces), 1, n, p, V, F, ptr(dist2), ptr(idx), ptr(bary), ptr(ws_p), ws_p.numel(), s),
				  'find_point_face_fwd')
		return winding, point_face, w

	for name, points, v, n in (('training', pts, verts, N), ('grid', grid, verts[:1], 1)):
		p = points.shape[1]
		winding, point_face, w = bare(points, v, n)
		wrapper = (lambda: inside.winding_number(points, v, faces)) if name == 'training' else (lambda: inside.occupancy_grid(v, faces, res))
		tp = min(p, args.torch_points // n if name == 'training' else args.torch_points)
		sub = points[:, :tp].contiguous()
		restated = lambda: torch_winding(sub, v, faces.long(), max(1, (1 << 23) // (n * F)))
		fns = dict(find_winding_fwd=winding, find_point_face_fwd=point_face, wrapper=wrapper, torch=restated)
		for fn in fns.values():
			fn()
		torch.cuda.synchronize()
		times = {k: [] for k in fns}
		for _ in range(args.reps):   # alternating: what disturbs one disturbs the others
			for k, fn in fns.items():
				times[k].append(event_ms(fn, 1 if k == 'torch' else args.launches))
		pairs = n * p * F
		rec[name] = {k: summary(t, pairs, p / tp if k == 'torch' else 1.) for k, t in times.items()}
		rec[name]['wrapper_is'] = 'inside.winding_number' if name == 'training' else f'inside.occupancy_grid(res={res})'
		rec[name]['torch_over_hip'] = round(rec[name]['torch']['median_ms'] / rec[name]['find_winding_fwd']['median_ms'], 1)
		rec[name]['winding_over_point_face'] = round(rec[name]['find_winding_fwd']['median_ms'] / rec[name]['find_point_face_fwd']['median_ms'], 2)
		# the values, for the record: the torch restatement against the HIP pass on the points both saw
		winding()
		rec[name]['max_abs_torch_minus_hip'] = float((torch_winding(sub, v, faces.long(), max(1, (1 << 23) // (n * F))) - w[:, :tp]).abs().max())
		rec[name]['share_inside'] = round(float((w > 0.5).float().mean()), 4)
	line = json.dumps(rec)
	print(line, flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as fh:
		fh.write(line + '\n')


if __name__ == '__main__':
	main()
