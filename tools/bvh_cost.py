"""Cost of the BVH path of the ray casts (find_ray_bvh_fwd) beside the brute-force pass (find_ray_fwd), closest hit and any_hit, and of the
structure's build and refit, at three sizes:
  training   16 meshes of synthetic.template(6890) (13 776 faces), 5000 box rays each (tools/rays_cost.py's rays);
  ao_bake    the rays of one AO bake of a 256^2 atlas on template(6890): the covered texels x 64 hemisphere directions;
  scan       one mesh of synthetic.template(50002) (about 10^5 faces), 10^6 box rays.
Device events around --launches calls in a row, the variants alternating inside --reps rounds (what disturbs one disturbs the others): the
median per call with its range.  `build` is find_bvh_keys + torch.sort + find_bvh_build, `refit` is find_bvh_refit alone.  The results of
the two paths are compared while at it (equal bits expected).  One JSON line, also written to --out (default profiles/bvh_cost.json).

	python tools/bvh_cost.py [--reps 5] [--launches 3] [--scan-rays 1000000] [--out FILE]"""
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


def summary(times):
	return dict(median_ms=round(float(np.median(times)), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def box_rays(verts, R, gen, dev):
	lo, hi = verts.amin(1) - 0.02, verts.amax(1) + 0.02
	o = (lo[:, None] + torch.rand(verts.shape[0], R, 3, generator=gen).to(dev) * (hi - lo)[:, None]).contiguous()
	return o, ((lo[:, None] + torch.rand(verts.shape[0], R, 3, generator=gen).to(dev) * (hi - lo)[:, None]) - o).contiguous()


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--launches', type=int, default=3)
	ap.add_argument('--feet', type=int, default=16)
	ap.add_argument('--rays', type=int, default=5000)
	ap.add_argument('--atlas', type=int, default=256)
	ap.add_argument('--dirs', type=int, default=64)
	ap.add_argument('--scan-verts', type=int, default=50002)
	ap.add_argument('--scan-rays', type=int, default=1000000)
	ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bvh_cost.json'))
	args = ap.parse_args()
	from find_amd import _lib, bake, rays, synthetic
	from find_amd._lib import check, current_stream, ptr
	dev = torch.device('cuda', 0)
	L = _lib.lib()
	s = current_stream(dev)
	gen = torch.Generator().manual_seed(0)
	tv, tf = synthetic.template(6890)
	verts = torch.stack([tv * (1 + 0.1 * torch.randn(3, generator=gen)) for _ in range(args.feet)]).to(dev).contiguous()
	faces = tf.to(dev).to(torch.int32).contiguous()
	o, d = box_rays(verts, args.rays, gen, dev)
	vu, fu = synthetic.face_atlas(faces.shape[0])
	plan = bake.plan(vu.to(dev), fu.to(dev), args.atlas)
	pts = plan.points(verts[:1], faces).contiguous()
	t1, t2, nrm = rays.normal_frames(bake.texel_normals(plan, verts[:1], faces))
	loc = rays.hemisphere_directions(args.dirs, dev)
	ao_d = (loc[:, 0, None] * t1[:, :, None] + loc[:, 1, None] * t2[:, :, None] + loc[:, 2, None] * nrm[:, :, None]).reshape(1, -1, 3).contiguous()
	ao_o = pts[:, :, None].expand(-1, -1, args.dirs, -1).reshape(1, -1, 3).contiguous()
	ao_skip = plan.face.reshape(-1)[plan.idx][None, :, None].expand(-1, -1, args.dirs).reshape(1, -1).to(torch.int32).contiguous()
	sv, sf = synthetic.template(args.scan_verts)
	sv, sf = sv[None].to(dev).contiguous(), sf.to(dev).to(torch.int32).contiguous()
	so, sd = box_rays(sv, args.scan_rays, gen, dev)
	rec = dict(leaf=rays.BVH_LEAF, arity=rays.BVH_ARITY, launches=args.launches, reps=args.reps)
	for name, o_, d_, v, f, skip in (('training', o, d, verts, faces, None), ('ao_bake', ao_o, ao_d, verts[:1], faces, ao_skip), ('scan', so, sd, sv, sf, None)):
		n, r, V, F = o_.shape[0], o_.shape[1], v.shape[1], f.shape[0]
		t, idx, bary = torch.empty(n, r, device=dev), torch.empty(n, r, dtype=torch.int32, device=dev), torch.empty(n, r, 3, device=dev)
		hit = torch.empty(n, r, dtype=torch.uint8, device=dev)
		ws = torch.empty(max(L.find_ray_ws_bytes(n, r, F), 256), dtype=torch.uint8, device=dev)
		bvh = rays.build_bvh(v, f)
		moved = (v * 1.01).contiguous()

		def cast(any_hit, accel):
			out = (None, None, None, ptr(hit)) if any_hit else (ptr(t), ptr(idx), ptr(bary), None)
			if accel:
				check(L.find_ray_bvh_fwd(ptr(o_), ptr(d_), None, ptr(skip), ptr(v), ptr(f), 1, n, r, V, F, 0., math.inf, any_hit, *out, ptr(bvh.data), bvh.nbytes, ptr(ws),
										 ws.numel(), s), 'find_ray_bvh_fwd')
			else:
				check(L.find_ray_fwd(ptr(o_), ptr(d_), None, ptr(skip), ptr(v), ptr(f), 1, n, r, V, F, 0., math.inf, any_hit, *out, ptr(ws), ws.numel(), s), 'find_ray_fwd')

		scratch = rays.build_bvh(v, f)   # refit and build are timed on a structure of their own: `bvh` stays the one of v
		fns = dict(brute_closest=lambda: cast(0, False), brute_any_hit=lambda: cast(1, False), bvh_closest=lambda: cast(0, True), bvh_any_hit=lambda: cast(1, True),
				   build=lambda: rays.build_bvh(v, f), refit=lambda: scratch.refit(moved))
		for fn in fns.values():
			fn()
		torch.cuda.synchronize()
		times = {k: [] for k in fns}
		for _ in range(args.reps):
			for k, fn in fns.items():
				times[k].append(event_ms(fn, 1 if (k.startswith('brute') and name == 'scan') else args.launches))
		row = {k: summary(tm) for k, tm in times.items()}
		row.update(meshes=n, rays=n * r, faces=F, pairs=n * r * F, bvh_bytes=bvh.nbytes)
		row['brute_over_bvh_closest'] = round(row['brute_closest']['median_ms'] / row['bvh_closest']['median_ms'], 2)
		row['brute_over_bvh_any_hit'] = round(row['brute_any_hit']['median_ms'] / row['bvh_any_hit']['median_ms'], 2)
		# the values, for the record
		cast(0, False)
		want = (t.clone(), idx.clone(), bary.clone())
		cast(0, True), cast(1, True)
		row['equal_bits'] = bool(torch.equal(t, want[0]) and torch.equal(idx, want[1]) and torch.equal(bary, want[2]) and torch.equal(hit.bool(), torch.isfinite(want[0])))
		row['share_hit'] = round(float(hit.float().mean()), 4)
		rec[name] = row
		print(name, json.dumps(row), flush=True)
	line = json.dumps(rec)
	print(line, flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as fh:
		fh.write(line + '\n')


if __name__ == '__main__':
	main()
