"""Cost of a full-size turntable spin (find_amd.vis.turntable: 250 frames at 512^2, azim 70, dist 0.35) for the 6890-vertex template
prediction (TexturesVertex) and a scan-sized TexturesUV mesh (10 002 vertices), each timed two ways through the SAME renderer:
  built     vis.turntable: rotated cameras, `views_per_call` views per render call, bytes made on the device (find_frames_u8);
  upstream  the reference's call pattern (mesh_turntable.py:46-62): 250 calls of one view each on rotated vertices, per frame
            .cpu().numpy(), (255 * x).astype(uint8) and the 180 degree turn on the host.
Per views_per_call in {25, 50, 125, 250}: the spin's time, the time per render call and the peak device memory.  find_frames_u8 is timed
alone on one chunk for its share of a spin.  Host clock around work that ends in a device synchronise; one warm-up, then the median of
--reps repeats with their range.  One JSON line per mesh.

	python tools/spin_cost.py [--reps 5] [--frames 250] [--size 512]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
	fn()
	torch.cuda.synchronize()
	times = []
	for _ in range(reps):
		t0 = time.perf_counter()
		fn()
		torch.cuda.synchronize()
		times.append((time.perf_counter() - t0) * 1e3)
	return dict(median_ms=round(float(np.median(times)), 2), min_ms=round(min(times), 2), max_ms=round(max(times), 2))


def upstream_spin(mesh, renderer, nframes, azim, dist):
	R, T = renderer.linspace_views(nviews=1, dist=dist, azim_min=azim, azim_max=azim)
	verts = mesh.verts_padded()
	theta = torch.linspace(0, 2 * math.pi, nframes)
	frames = []
	with torch.no_grad():
		for i in range(nframes):
			c, s = math.cos(float(theta[i])), math.sin(float(theta[i]))
			Rz = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], device=verts.device)
			image = renderer(mesh.update_padded(verts @ Rz), R, T)['image']
			rdr = (255 * image[0, 0].cpu().numpy()).astype(np.uint8)
			frames.append(np.ascontiguousarray(rdr[::-1, ::-1]))
	return frames


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--frames', type=int, default=250)
	ap.add_argument('--size', type=int, default=512)
	args = ap.parse_args()
	from find_amd import functional as FN, synthetic, vis
	from find_amd.renderer import FootRenderer
	from find_amd.structures import Meshes, TexturesUV, TexturesVertex
	dev = torch.device('cuda', 0)
	g = torch.Generator().manual_seed(0)
	tv, tf = synthetic.template(6890)
	pred = Meshes(tv[None].to(dev), tf.to(dev), TexturesVertex(torch.rand(1, tv.shape[0], 3, generator=g).to(dev)))
	gv, gf, _ = synthetic.gt_feet(1, 10002, seed=0, device=dev)
	lo, hi = gv.amin(1, keepdim=True), gv.amax(1, keepdim=True)
	uv = ((gv - lo) / (hi - lo))[..., :2].contiguous()
	scan = Meshes(gv, gf[None], TexturesUV(torch.rand(1, 1024, 1024, 3, generator=g).to(dev), gf[None], uv))
	n, size = args.frames, args.size
	renderer = FootRenderer(image_size=size, device=dev)
	chunk = torch.rand(min(50, n), size, size, 3, device=dev)
	for name, mesh in (('template_6890_vertex_colours', pred), ('scan_10002_uv', scan)):
		rec = dict(mesh=name, frames=n, image_size=size)
		for per_call in (25, 50, 125, 250):
			if per_call > n:
				continue
			torch.cuda.reset_peak_memory_stats(dev)
			t = timed(lambda: vis.turntable(mesh, None, image_size=size, nframes=n, azim=70, dist=0.35, silent=True, views_per_call=per_call), args.reps)
			t['per_call_ms'] = round(t['median_ms'] / math.ceil(n / per_call), 2)
			t['peak_MB'] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 20)
			rec[f'built_{per_call}_views_per_call'] = t
		rec['upstream_pattern'] = timed(lambda: upstream_spin(mesh, renderer, n, 70, 0.35), args.reps)
		a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		FN.frames_u8(chunk)
		a.record()
		for _ in range(20):
			FN.frames_u8(chunk)
		b.record()
		b.synchronize()
		per_chunk_ms = a.elapsed_time(b) / 20
		rec['frames_u8_ms_per_chunk'] = round(per_chunk_ms, 4)
		rec['frames_u8_chunk'] = list(chunk.shape)
		rec['frames_u8_GB_per_s'] = round(chunk.numel() * 5 / per_chunk_ms / 1e6, 1)
		key = 'built_50_views_per_call' if 'built_50_views_per_call' in rec else next(k for k in rec if k.startswith('built_'))
		rec['frames_u8_share_of_spin'] = round(per_chunk_ms * (n / chunk.shape[0]) / rec[key]['median_ms'], 4)
		print(json.dumps(rec), flush=True)


if __name__ == '__main__':
	main()
