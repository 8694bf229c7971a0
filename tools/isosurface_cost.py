"""Cost of the surface-nets extraction (find_surface_nets_count + find_surface_nets_emit) on sphere fields of 64^3 and 128^3 samples, N = 1 and
16, beside find_amd.isosurface.extract_surface with and without the read-back of the counts and beside a torch restatement on the device
(masks, nonzero, gathers: the same vertices; the faces grouped by axis, not sorted into sample order); the backward call; and, for context,
isosurface.remesh(res) of synthetic.template(6890) split into the field (inside.signed_distance on the grid) and the extraction.
Device events around --launches calls in a row (a warm-up call first), the variants alternating, repeated --reps times: the median per call
with its range.  One JSON line, also written to --out (default profiles/isosurface_cost.json).

	python tools/isosurface_cost.py [--reps 5] [--launches 5] [--res 128] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EDGES = [(a, b) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count('1') == 1]


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


def _corner(t, c):
	nx, ny, nz = t.shape[1:]
	di, dj, dk = (c >> 2) & 1, (c >> 1) & 1, c & 1
	return t[:, di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk]


def torch_nets(values, iso):
	"""(g (V, 3) of all meshes in (mesh, cell) order, faces (F, 3) indexing it, grouped by axis) of the definition in torch, float32."""
	ins = values < iso
	cin = [_corner(ins, c) for c in range(8)]
	cnt = sum(c.to(torch.int32) for c in cin)
	active = (cnt > 0) & (cnt < 8)
	idx = active.nonzero()
	cellmap = (torch.cumsum(active.flatten(), 0) - 1).view(active.shape)
	n, i, j, k = idx.unbind(1)
	cv = [values[n, i + ((c >> 2) & 1), j + ((c >> 1) & 1), k + (c & 1)] for c in range(8)]
	ci = [v < iso for v in cv]
	s, cnt = torch.zeros(len(idx), 3, device=values.device), torch.zeros(len(idx), device=values.device)
	for a, b in EDGES:
		cross = ci[a] != ci[b]
		t = (iso - cv[a]) / (cv[b] - cv[a])
		t = torch.where(torch.isfinite(t), t, torch.full_like(t, 0.5))
		p = torch.tensor([(a >> 2) & 1, (a >> 1) & 1, a & 1], dtype=torch.float32, device=values.device).repeat(len(idx), 1)
		p[:, {4: 0, 2: 1, 1: 2}[b - a]] = t
		s += torch.where(cross[:, None], p, torch.zeros_like(p))
		cnt += cross
	g = idx[:, 1:].float() + s / cnt[:, None]
	faces = []
	shape = values.shape[1:]
	for ax in range(3):
		u, w = (ax + 1) % 3, (ax + 2) % 3
		lo, hi = [slice(None)] * 4, [slice(None)] * 4
		lo[1 + ax], hi[1 + ax] = slice(0, shape[ax] - 1), slice(1, shape[ax])
		lo[1 + u] = hi[1 + u] = slice(1, shape[u] - 1)
		lo[1 + w] = hi[1 + w] = slice(1, shape[w] - 1)
		a_in = ins[tuple(lo)]
		at = (a_in != ins[tuple(hi)]).nonzero()
		s_in = a_in[at.unbind(1)]
		at[:, 1 + u] += 1
		at[:, 1 + w] += 1
		q = []
		for du, dw in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
			c = at.clone()
			c[:, 1 + u] += du
			c[:, 1 + w] += dw
			q.append(cellmap[c.unbind(1)])
		q = torch.stack(q, 1)
		q = torch.where(s_in[:, None], q, q.flip(1))
		faces.append(torch.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3))
	return g, torch.cat(faces)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--launches', type=int, default=5)
	ap.add_argument('--res', type=int, default=128, help='remesh resolution of the context figure')
	ap.add_argument('--template', type=int, default=6890)
	ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'isosurface_cost.json'))
	args = ap.parse_args()
	from find_amd import _lib, isosurface, synthetic
	from find_amd._lib import check, current_stream, ptr
	dev = torch.device('cuda', 0)
	L = _lib.lib()
	st = current_stream(dev)
	rec = dict(launches=args.launches, reps=args.reps)
	for res in (64, 128):
		for N in (1, 16):
			ax = -0.06 + (torch.arange(res, device=dev) + 0.5) * (0.12 / res)
			x, y, z = torch.meshgrid(ax, ax, ax, indexing='ij')
			radii = 0.04 - 0.0005 * torch.arange(N, device=dev)
			values = ((x * x + y * y + z * z).sqrt()[None] - radii[:, None, None, None]).contiguous()
			origin, spacing = torch.full((N, 3), -0.06, device=dev), torch.full((N, 3), 0.12 / res, device=dev)
			verts, faces, v_len, f_len, status = isosurface.extract_surface(values, origin, spacing)
			V, F = verts.shape[1], faces.shape[1]
			ws = torch.empty(L.find_surface_nets_ws_bytes(N, res, res, res), dtype=torch.uint8, device=dev)
			g, fc = torch.empty(N, V, 3, device=dev), torch.empty(N, F, 3, dtype=torch.int32, device=dev)
			nv, nf, stt = torch.empty(N, dtype=torch.int64, device=dev), torch.empty(N, dtype=torch.int64, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
			grad_g, grad_values, grad_iso = torch.randn(N, V, 3, device=dev), torch.empty_like(values), torch.empty(N, device=dev)
			bws = torch.empty(L.find_surface_nets_bwd_ws_bytes(N, res, res, res), dtype=torch.uint8, device=dev)

			def count():
				check(L.find_surface_nets_count(ptr(values), 0., N, res, res, res, ptr(nv), ptr(nf), ptr(stt), ptr(ws), ws.numel(), st), 'count')

			def count_emit():
				count()
				check(L.find_surface_nets_emit(ptr(values), 0., N, res, res, res, ptr(nv), ptr(nf), V, F, ptr(g), ptr(fc), ptr(stt), ptr(ws), ws.numel(), st), 'emit')

			def backward():
				check(L.find_surface_nets_bwd(ptr(values), 0., N, res, res, res, ptr(ws), ptr(grad_g), V, ptr(grad_values), ptr(grad_iso), ptr(bws), bws.numel(), st), 'bwd')
			fns = dict(count=count, count_emit=count_emit, backward=backward, extract_read_back=lambda: isosurface.extract_surface(values, origin, spacing),
					   extract_capacities=lambda: isosurface.extract_surface(values, origin, spacing, 0., V, F), torch=lambda: torch_nets(values, 0.))
			for fn in fns.values():
				fn()
			torch.cuda.synchronize()
			times = {k: [] for k in fns}
			for _ in range(args.reps):   # alternating: what disturbs one disturbs the others
				for k, fn in fns.items():
					times[k].append(event_ms(fn, args.launches))
			case = {k: summary(t) for k, t in times.items()}
			tg, tf = torch_nets(values, 0.)
			count_emit()
			keep = torch.arange(V, device=dev)[None] < v_len[:, None]
			case.update(verts=[int(v) for v in v_len], faces=[int(f) for f in f_len], max_abs_torch_minus_hip=float((tg - g[keep]).abs().max()),
						torch_faces=int(len(tf)), torch_over_hip=round(case['torch']['median_ms'] / case['count_emit']['median_ms'], 1),
						M_samples_per_s=round(N * res ** 3 / case['count_emit']['median_ms'] / 1e3, 1))
			assert len(tg) == int(v_len.sum()) and len(tf) == int(f_len.sum())
			rec[f'{res}^3 x {N}'] = case
	# context: the remesh of a template, field and extraction apart
	tv, tf = synthetic.template(args.template)
	tv, tf = tv[None].to(dev).contiguous(), tf.to(dev)
	sdf, origin, spacing = isosurface.field_grid(tv, tf, args.res)
	fns = dict(field_grid=lambda: isosurface.field_grid(tv, tf, args.res), extract_surface=lambda: isosurface.extract_surface(sdf, origin, spacing),
			   remesh=lambda: isosurface.remesh(tv, tf, args.res))
	for fn in fns.values():
		fn()
	times = {k: [] for k in fns}
	for _ in range(args.reps):
		for k, fn in fns.items():
			times[k].append(event_ms(fn, 1))
	out = isosurface.remesh(tv, tf, args.res)
	rec['remesh'] = dict(res=args.res, template=args.template, faces_in=int(tf.shape[0]), verts_out=int(out[2][0]), faces_out=int(out[3][0]), status=int(out[4][0]),
						 **{k: summary(t) for k, t in times.items()})
	line = json.dumps(rec)
	print(line, flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as fh:
		fh.write(line + '\n')


if __name__ == '__main__':
	main()
