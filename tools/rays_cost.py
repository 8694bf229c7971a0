"""Cost of the ray-casting pass (find_ray_fwd) at two sizes, closest hit and any_hit side by side, beside a chunked torch restatement of the
same pair test:
  training   16 meshes of synthetic.template(6890) (13 776 faces), 5000 box rays each (the origin uniform in the mesh's box grown by 2 cm,
             aimed at a second such point): 1.1 G ray-face pairs;
  ao_bake    one AO bake of a 256^2 atlas (synthetic.face_atlas) on template(6890): the covered texels x 64 hemisphere directions, through
             bake.bake_ambient_occlusion, and the same rays through the two C calls in one piece.
Pairs are counted as rays x faces, whatever the any_hit call's early exit leaves out: its figure is what the brute-force pass would need.
The torch restatement (float32 on the device, the operations of tests/rays_ref.py, a (chunk, F) block at a time) is timed on --torch-rays
rays of each size and scaled to the whole: it is linear in the rays.
Device events around --launches calls in a row (a warm-up call first), repeated --reps times: the median per call with its range, and pairs
per second.  One JSON line, also written to --out (default profiles/rays_cost.json).

	python tools/rays_cost.py [--reps 5] [--launches 5] [--feet 16] [--rays 5000] [--atlas 256] [--out FILE]"""
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


def torch_cast(o, d, verts, faces, chunk):
	"""t (N, R) float32, +inf for a miss: the pair test in torch, float32, `chunk` rays of every mesh at a time."""
	N, R = o.shape[:2]
	kz = d.abs().argmax(-1)
	kx, ky = (kz + 1) % 3, (kz + 2) % 3
	dz = torch.gather(d, 2, kz[..., None])[..., 0]
	swap = dz < 0
	kx, ky = torch.where(swap, ky, kx), torch.where(swap, kx, ky)
	e1, e2 = torch.zeros_like(d), torch.zeros_like(d)
	e1.scatter_(2, kx[..., None], 1.)
	e1.scatter_(2, kz[..., None], -(torch.gather(d, 2, kx[..., None]) / dz[..., None]))
	e2.scatter_(2, ky[..., None], 1.)
	e2.scatter_(2, kz[..., None], -(torch.gather(d, 2, ky[..., None]) / dz[..., None]))
	dd = (d * d).sum(-1)
	out = []
	for s in range(0, R, chunk):
		P = verts[:, None] - o[:, s:s + chunk, None]   # (N, r, V, 3)
		x, y, z = (P * e1[:, s:s + chunk, None]).sum(-1), (P * e2[:, s:s + chunk, None]).sum(-1), (P * d[:, s:s + chunk, None]).sum(-1)
		ax, ay, bx, by, cx, cy = x[..., faces[:, 0]], y[..., faces[:, 0]], x[..., faces[:, 1]], y[..., faces[:, 1]], x[..., faces[:, 2]], y[..., faces[:, 2]]
		U, V, W = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
		det = U + V + W
		inside = (((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))) & (det != 0)
		t = (U * z[..., faces[:, 0]] + V * z[..., faces[:, 1]] + W * z[..., faces[:, 2]]) / (det * dd[:, s:s + chunk, None])
		out.append(torch.where(inside & (t > 0), t, torch.full_like(t, math.inf)).amin(-1))
	return torch.cat(out, 1)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--launches', type=int, default=5)
	ap.add_argument('--feet', type=int, default=16)
	ap.add_argument('--rays', type=int, default=5000)
	ap.add_argument('--atlas', type=int, default=256)
	ap.add_argument('--dirs', type=int, default=64)
	ap.add_argument('--template', type=int, default=6890)
	ap.add_argument('--torch-rays', type=int, default=1 << 12)
	ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rays_cost.json'))
	args = ap.parse_args()
	from find_amd import _lib, bake, rays, synthetic
	from find_amd._lib import check, current_stream, ptr
	dev = torch.device('cuda', 0)
	L = _lib.lib()
	s = current_stream(dev)
	N, R = args.feet, args.rays
	tv, tf = synthetic.template(args.template)
	gen = torch.Generator().manual_seed(0)
	verts = torch.stack([tv * (1 + 0.1 * torch.randn(3, generator=gen)) for _ in range(N)]).to(dev).contiguous()
	faces = tf.to(dev).to(torch.int32).contiguous()
	V, F = verts.shape[1], faces.shape[0]
	lo, hi = verts.amin(1) - 0.02, verts.amax(1) + 0.02
	o = (lo[:, None] + torch.rand(N, R, 3, generator=gen).to(dev) * (hi - lo)[:, None]).contiguous()
	d = ((lo[:, None] + torch.rand(N, R, 3, generator=gen).to(dev) * (hi - lo)[:, None]) - o).contiguous()
	# the AO bake's rays, as bake_ambient_occlusion and rays.ambient_occlusion make them
	vu, fu = synthetic.face_atlas(F)
	plan = bake.plan(vu.to(dev), fu.to(dev), args.atlas)
	T = plan.idx.numel()
	pts = plan.points(verts[:1], faces).contiguous()
	t1, t2, nrm = rays.normal_frames(bake.texel_normals(plan, verts[:1], faces))
	loc = rays.hemisphere_directions(args.dirs, dev)
	ao_d = (loc[:, 0, None] * t1[:, :, None] + loc[:, 1, None] * t2[:, :, None] + loc[:, 2, None] * nrm[:, :, None]).reshape(1, -1, 3).contiguous()
	ao_o = pts[:, :, None].expand(-1, -1, args.dirs, -1).reshape(1, -1, 3).contiguous()
	ao_skip = plan.face.reshape(-1)[plan.idx][None, :, None].expand(-1, -1, args.dirs).reshape(1, -1).contiguous()
	rec = dict(feet=N, rays=R, verts=V, faces=F, atlas=args.atlas, dirs=args.dirs, covered_texels=T, launches=args.launches, reps=args.reps, torch_rays=args.torch_rays)

	def bare(o_, d_, v, n, skip):
		"""The C call on preallocated buffers, closest hit and any_hit."""
		r = o_.shape[1]
		t, idx, bary = torch.empty(n, r, device=dev), torch.empty(n, r, dtype=torch.int32, device=dev), torch.empty(n, r, 3, device=dev)
		hit = torch.empty(n, r, dtype=torch.uint8, device=dev)
		ws = torch.empty(max(L.find_ray_ws_bytes(n, r, F), 256), dtype=torch.uint8, device=dev)

		def closest():
			check(L.find_ray_fwd(ptr(o_), ptr(d_), None, ptr(skip), ptr(v), ptr(faces), 1, n, r, V, F, 0., math.inf, 0, ptr(t), ptr(idx), ptr(bary), None, ptr(ws),
								 ws.numel(), s), 'find_ray_fwd')

		def any_hit():
			check(L.find_ray_fwd(ptr(o_), ptr(d_), None, ptr(skip), ptr(v), ptr(faces), 1, n, r, V, F, 0., math.inf, 1, None, None, None, ptr(hit), ptr(ws),
								 ws.numel(), s), 'find_ray_fwd')
		return closest, any_hit, t, hit

	for name, o_, d_, v, n, skip in (('training', o, d, verts, N, None), ('ao_bake', ao_o, ao_d, verts[:1], 1, ao_skip)):
		r = o_.shape[1]
		closest, any_hit, t, hit = bare(o_, d_, v, n, skip)
		wrapper = (lambda: rays.ray_mesh_intersect(o_, d_, v, faces)) if name == 'training' else (lambda: bake.bake_ambient_occlusion(plan, v, faces, n_dirs=args.dirs))
		tr = min(r, args.torch_rays // n if name == 'training' else args.torch_rays)
		so, sd = o_[:, :tr].contiguous(), d_[:, :tr].contiguous()
		restated = lambda: torch_cast(so, sd, v, faces.long(), max(1, (1 << 22) // (n * F)))
		fns = dict(find_ray_fwd_closest=closest, find_ray_fwd_any_hit=any_hit, wrapper=wrapper, torch=restated)
		for fn in fns.values():
			fn()
		torch.cuda.synchronize()
		times = {k: [] for k in fns}
		for _ in range(args.reps):   # alternating: what disturbs one disturbs the others
			for k, fn in fns.items():
				times[k].append(event_ms(fn, 1 if k == 'torch' else args.launches))
		pairs = n * r * F
		rec[name] = {k: summary(tm, pairs, r / tr if k == 'torch' else 1.) for k, tm in times.items()}
		rec[name]['rays'] = n * r
		rec[name]['wrapper_is'] = 'rays.ray_mesh_intersect' if name == 'training' else f'bake.bake_ambient_occlusion({args.atlas}^2, n_dirs={args.dirs})'
		rec[name]['torch_over_hip'] = round(rec[name]['torch']['median_ms'] / rec[name]['find_ray_fwd_closest']['median_ms'], 1)
		rec[name]['closest_over_any_hit'] = round(rec[name]['find_ray_fwd_closest']['median_ms'] / rec[name]['find_ray_fwd_any_hit']['median_ms'], 2)
		# the values, for the record: the two calls against each other, and the torch restatement against the HIP pass on the rays both saw
		closest(), any_hit()
		rec[name]['any_hit_equals_isfinite_t'] = bool(torch.equal(hit.bool(), torch.isfinite(t)))
		rec[name]['share_hit'] = round(float(hit.float().mean()), 4)
		if skip is None:
			tt = torch_cast(so, sd, v, faces.long(), max(1, (1 << 22) // (n * F)))
			both = torch.isfinite(tt) & torch.isfinite(t[:, :tr])
			rec[name]['torch_hits_agree'] = round(float((torch.isfinite(tt) == torch.isfinite(t[:, :tr])).float().mean()), 6)
			rec[name]['max_abs_torch_minus_hip'] = float((tt[both] - t[:, :tr][both]).abs().max())
	line = json.dumps(rec)
	print(line, flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as fh:
		fh.write(line + '\n')


if __name__ == '__main__':
	main()
