"""Timing of the per-vertex feature render against the raster pass it follows (find_render_features_fwd / _bwd vs find_render_fwd /
find_render_bwd's silhouette part): 16 feet x 4 views of the 6890-vertex synthetic template at 256^2 (C3 shape) and 512^2 (C4 rank share),
C in {3, 21, 64}.  Device events around each call, warm-up, median of repeats; prints one JSON line per configuration with the times
(ms) and the algorithmic bytes of the feature passes (output write, d_out read).  `python tools/prof_features.py [--repeats R]`."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from find_amd import _lib, functional_render as FR, synthetic   # noqa: E402
from find_amd._lib import check, current_stream, ptr   # noqa: E402
from find_amd.cameras import look_at_view_transform   # noqa: E402
from find_amd.functional import _ws   # noqa: E402


def _timed(fn, warmup, repeats):
	for _ in range(warmup):
		fn()
	ts = []
	for _ in range(repeats):
		a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		a.record()
		fn()
		b.record()
		b.synchronize()
		ts.append(a.elapsed_time(b))
	return float(np.median(ts))


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--repeats', type=int, default=9)
	ap.add_argument('--warmup', type=int, default=3)
	ap.add_argument('--sizes', default='256,512')
	ap.add_argument('--channels', default='3,21,64')
	args = ap.parse_args()
	L = _lib.lib()
	dev = torch.device('cuda')
	v, f = synthetic.template(6890)
	g = torch.Generator().manual_seed(0)
	N, M = 16, 4
	verts = (v[None] * (1 + 0.1 * torch.rand(N, 1, 3, generator=g))).to(dev).contiguous()
	faces = f.to(dev).to(torch.int32).contiguous()
	rng = np.random.RandomState(1)
	R, T = look_at_view_transform(dist=np.full(M, 0.3), elev=rng.uniform(-90, 90, M), azim=rng.uniform(-90, 90, M), up=((1, 0, 0),))
	R, T = R.to(dev).float().contiguous(), T.to(dev).float().contiguous()
	V, F = verts.shape[1], faces.shape[0]
	s = current_stream(dev)
	for size in [int(x) for x in args.sizes.split(',')]:
		p = FR.make_params(size)
		H = W = size
		ws = _ws(L.find_render_ws_bytes(ctypes.byref(p), N, M, V, F), dev)
		mask = torch.empty(N, M, H, W, device=dev)
		d_mask = torch.randn(N, M, H, W, device=dev)
		d_verts = torch.empty_like(verts)

		def raster():
			check(L.find_render_fwd(ctypes.byref(p), ptr(verts), ptr(faces), 1, None, ptr(R), ptr(T), N, M, V, F, ptr(mask), None, None, None,
									ptr(ws), ws.numel(), s), 'find_render_fwd')

		def sil_bwd():
			check(L.find_render_bwd(ctypes.byref(p), ptr(verts), ptr(faces), 1, None, ptr(R), ptr(T), N, M, V, F, ptr(mask), ptr(d_mask), None,
									ptr(d_verts), None, ptr(ws), ws.numel(), s), 'find_render_bwd')
		t_raster = _timed(raster, args.warmup, args.repeats)
		t_sil_bwd = _timed(sil_bwd, args.warmup, args.repeats)
		raster()
		for C in [int(x) for x in args.channels.split(',')]:
			feats = torch.randn(N, V, C, device=dev)
			fws = _ws(L.find_render_features_ws_bytes(ctypes.byref(p), N, M, C), dev)
			out = torch.empty(N, M, H, W, C, device=dev)
			d_out = torch.randn_like(out)
			d_feat = torch.empty_like(feats)

			def ffwd():
				check(L.find_render_features_fwd(ctypes.byref(p), ptr(verts), ptr(faces), 1, ptr(R), ptr(T), N, M, V, F, ptr(feats), C, ptr(out),
												  ptr(ws), ws.numel(), ptr(fws), fws.numel(), s), 'find_render_features_fwd')

			def fbwd():
				check(L.find_render_features_bwd(ctypes.byref(p), ptr(verts), ptr(faces), 1, ptr(R), ptr(T), N, M, V, F, ptr(feats), C, ptr(out),
												  ptr(d_out), ptr(d_verts), ptr(d_feat), ptr(ws), ws.numel(), ptr(fws), fws.numel(), s),
					  'find_render_features_bwd')
			t_ffwd = _timed(ffwd, args.warmup, args.repeats)
			t_fbwd = _timed(fbwd, args.warmup, args.repeats)
			nbytes = N * M * H * W * C * 4
			print(json.dumps(dict(size=size, feet=N, views=M, C=C, raster_fwd_ms=round(t_raster, 4), sil_bwd_ms=round(t_sil_bwd, 4),
								  feat_fwd_ms=round(t_ffwd, 4), feat_bwd_ms=round(t_fbwd, 4), feat_fwd_over_raster=round(t_ffwd / t_raster, 3),
								  feat_bwd_over_sil_bwd=round(t_fbwd / t_sil_bwd, 3), out_write_bytes=nbytes, d_out_read_bytes=nbytes,
								  feat_fwd_gbps=round(nbytes / t_ffwd / 1e6, 1))), flush=True)


if __name__ == '__main__':
	main()
