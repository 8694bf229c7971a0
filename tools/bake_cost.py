"""Cost of baking the colour field into UV textures (find_amd.bake) at the sizes a user would run: synthetic.template(6890) (13 776 faces)
with synthetic.face_atlas(13776), one right triangle per face -- the atlas with the most chart border per texel.
  raster   find_uv_raster on preallocated outputs, at 1024^2 and 2048^2;
  dilate   find_uv_dilate_map with pad = 4 on those rasters;
  bake     bake.bake_colours for 16 feet at 1024^2 on a ready plan, and its two parts alone: the colour head over the covered texels'
           points (16 x T rows, in chunks of 65 536 texels) and BakePlan.assemble (one index_select into 16 maps).
Device events around --launches calls in a row (a warm-up call first), repeated --reps times: the median per call with its range.  The
raster and the dilate map are also given as a share of the 16-foot bake (they are made once per atlas, a bake once per batch of feet).
One JSON line, also written to --out (default profiles/bake_cost.json).

	python tools/bake_cost.py [--reps 5] [--launches 10] [--feet 16] [--out FILE]"""
import argparse
import json
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


def timed(fn, launches, reps):
	fn()
	torch.cuda.synchronize()
	return summary([event_ms(fn, launches) for _ in range(reps)])


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--launches', type=int, default=10)
	ap.add_argument('--bake-launches', type=int, default=3)
	ap.add_argument('--feet', type=int, default=16)
	ap.add_argument('--template', type=int, default=6890)
	ap.add_argument('--pad', type=int, default=4)
	ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bake_cost.json'))
	args = ap.parse_args()
	from find_amd import _lib, bake, synthetic
	from find_amd._lib import check, current_stream, ptr
	dev = torch.device('cuda', 0)
	model = synthetic.make_model(args.template, train_size=args.feet, device=dev)
	lat = synthetic.latents(args.feet, seed=0, device=dev)
	F = model.template_faces.shape[1]
	vu, fu = synthetic.face_atlas(F)
	vu, fu = vu.to(dev), fu.to(dev).to(torch.int32).contiguous()
	L = _lib.lib()
	s = current_stream(dev)
	rec = dict(feet=args.feet, template_verts=args.template, faces=F, pad=args.pad, launches=args.launches, bake_launches=args.bake_launches, reps=args.reps)
	for size in (1024, 2048):
		face = torch.empty(size, size, dtype=torch.int32, device=dev)
		bary = torch.empty(size, size, 3, device=dev)
		src = torch.empty_like(face)

		def raster():
			check(L.find_uv_raster(ptr(vu), vu.shape[0], ptr(fu), F, size, size, ptr(face), ptr(bary), s), 'find_uv_raster')

		def dilate():
			check(L.find_uv_dilate_map(ptr(face), size, size, args.pad, ptr(src), s), 'find_uv_dilate_map')
		rec[f'raster_{size}'] = timed(raster, args.launches, args.reps)
		rec[f'dilate_{size}'] = timed(dilate, args.launches, args.reps)
		rec[f'covered_{size}'] = int((face >= 0).sum())
		rec[f'gutter_{size}'] = int(((src >= 0) & (face < 0)).sum())
	# the bake of --feet feet at 1024^2
	plan = bake.plan(vu, fu, 1024, pad=args.pad)
	T = plan.idx.numel()
	tv, tf = model.template_verts.data, model.template_faces.data[0]
	chunk = 65536
	cols = torch.empty(args.feet, T, 3, device=dev)

	def whole():
		return bake.bake_colours(model, plan, texvec=lat['texvec'])

	def evaluate():
		with torch.no_grad():
			pts = plan.points(tv, tf)
			for a in range(0, T, chunk):
				cols[:, a:a + chunk] = model(pts[:, a:a + chunk].contiguous(), texvec=lat['texvec'], want=('col',))['col'][..., :3]

	def assemble():
		return plan.assemble(cols)
	rec['bake_texels'] = T
	rec['bake_rows'] = args.feet * T
	rec['bake_1024'] = timed(whole, args.bake_launches, args.reps)
	rec['bake_1024_mlp'] = timed(evaluate, args.bake_launches, args.reps)
	rec['bake_1024_assemble'] = timed(assemble, args.bake_launches, args.reps)
	rec['raster_share_of_bake'] = round(rec['raster_1024']['median_ms'] / rec['bake_1024']['median_ms'], 4)
	rec['dilate_share_of_bake'] = round(rec['dilate_1024']['median_ms'] / rec['bake_1024']['median_ms'], 4)
	rec['raster_over_mlp'] = round(rec['raster_1024']['median_ms'] / rec['bake_1024_mlp']['median_ms'], 4)
	rec['dilate_over_mlp'] = round(rec['dilate_1024']['median_ms'] / rec['bake_1024_mlp']['median_ms'], 4)
	line = json.dumps(rec)
	print(line, flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as fh:
		fh.write(line + '\n')


if __name__ == '__main__':
	main()
