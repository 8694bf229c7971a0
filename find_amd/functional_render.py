"""torch.autograd binding of the HIP renderer (find_render_fwd / find_render_bwd), of the per-vertex feature render on its raster pass
(find_render_features_fwd / _bwd) and of the keypoint splat render (find_points_render, forward only).  GPU only, no fallback."""
import atexit
import contextlib
import ctypes
import math
import os
import warnings

import torch

from . import _lib
from ._lib import PointsParams, RenderParams, check, current_stream, ptr
from .functional import _c, _faces_i32, _require_gpu, _ws


def make_params(image_size=256, faces_per_pixel=100, background=(1., 1., 1.), light_pos=(0., 0., 100.), znear=0.02, zfar=100.0,
				fov_deg=60.0, sil_sigma=1e-4, z_clip=None, clip_faces=False):
	"""FootRenderer's fixed settings (renderer.py:113-128, 274) + PyTorch3D defaults for BlendParams / PointLights / Materials.
	clip_faces: faces that straddle the z-clip plane are clipped into one or two triangles as PyTorch3D does (close-up views, a camera
	inside the mesh); off (the default), they are rasterised whole and reported by the render watchdog below."""
	p = RenderParams()
	if isinstance(image_size, (tuple, list)):
		p.image_h, p.image_w = int(image_size[0]), int(image_size[1])
	else:
		p.image_h = p.image_w = int(image_size)
	p.fov_deg, p.znear, p.zfar = fov_deg, znear, zfar
	p.sil_sigma = sil_sigma
	p.sil_blur_radius = float(math.log(1. / 1e-4 - 1.) * sil_sigma)
	if not 1 <= int(faces_per_pixel) <= 32767:   # (int16 in find_render_params: it shares its four bytes with clip_faces)
		raise ValueError(f'make_params: faces_per_pixel {faces_per_pixel} outside 1 .. 32767')
	p.sil_faces_per_pixel = faces_per_pixel
	p.rgb_sigma, p.rgb_gamma = 1e-4, 1e-4
	p.background[:] = list(background)
	p.light_pos[:] = list(light_pos)
	p.ambient, p.diffuse, p.specular, p.shininess = 0.5, 0.3, 0.2, 64.0
	p.z_clip = znear / 2 if z_clip is None else z_clip
	p.clip_faces = 1 if clip_faces else 0
	return p


# ---------------------------------------------------------------------------------------------- render watchdog
# PyTorch3D clips faces that straddle the z-clip plane (znear / 2, renderer.py:231-234) into 1-2 triangles; this rasteriser does so only
# with make_params(clip_faces=True) (FootRenderer(..., clip_faces=True)).  By default it counts them (find_render_flags) and, like the pixels that collect more than 4096 silhouette candidates, they make the result differ
# from the reference.  Neither occurs with FIND's cameras (0.3 m from a <= 0.15 m object; view_from('toes') leaves 0.06 m).  A render
# that hits either case is REPORTED: the two counters travel to a pinned host slot behind the launch and are looked at when they have
# arrived -- at the next render call, in check_render_flags(), at an epoch boundary of find_amd.trainer.Trainer, or when the interpreter
# exits -- so the check costs no synchronisation.  FLAG_POLICY:
#   'strict' (default since round 6: a wrong image is an error) the look-up raises RuntimeError, in whichever later call finds the
#            counters;   'async' = 'strict' (rounds 1-2 name)
#   'warn'   warnings.warn with the description of the render -- what find_amd.trainer.Trainer runs its epochs under (flag_policy('warn')):
#            a close-up visualisation render must not end a training run at an arbitrary later call;
#   'sync'   wait for the counters and raise in the same call (tests);   'ignore' no bookkeeping at all.
FLAG_POLICY = os.environ.get('FIND_RENDER_FLAG_POLICY', 'strict')


@contextlib.contextmanager
def flag_policy(policy):
	"""Renders issued inside the block are watched under `policy` (each render carries the policy of its own call to the look-up)."""
	global FLAG_POLICY
	if policy not in ('strict', 'async', 'warn', 'sync', 'ignore'):
		raise ValueError(f'flag_policy: {policy!r}')
	prev, FLAG_POLICY = FLAG_POLICY, policy
	try:
		yield
	finally:
		FLAG_POLICY = prev
_RING = 64
_pending = []   # (event, slot, description, policy at the time of the render)
_slots = None   # one pinned int32[_RING][2] buffer, reused: slot i is free when no pending entry holds it
_free = []


def _report(vals, what, policy):
	if vals[0] <= 0 and vals[1] <= 0:
		return
	msg = (f'find_amd.render: {what}: {vals[0]} face(s) straddle the z-clip plane (PyTorch3D would clip them; this rasteriser '
		   f'does not) and {vals[1]} pixel(s) collected more than 4096 silhouette candidates (K-nearest rule not applied): the '
		   'result differs from the reference.  Move the camera; functional_render.FLAG_POLICY = "strict" / "ignore" changes this report.'
		   + ('  FootRenderer(..., clip_faces=True) / make_params(clip_faces=True) clips such faces as PyTorch3D does.' if vals[0] > 0 else ''))
	if policy == 'warn':
		warnings.warn(msg, RuntimeWarning, stacklevel=3)
	else:
		raise RuntimeError(msg)


_cap_flags = {}     # device -> int32[2]: the counters of renders replayed from a HIP graph, summed on the device
_cap_used = set()


def _check_captured():
	"""Renders inside a captured step cannot hand their counters to a pinned slot per call; they ADD them to one static device slot
	(part of the graph, so every replay adds), read back here -- one device-to-host copy, at an epoch boundary (Trainer._epoch_done) or
	an explicit check_render_flags(wait=True).  A device stays registered once a capture has used its slot (`_watch` runs only
	while a stream CAPTURES, so a device taken off the list after the first check was never looked at again and the watchdog of the
	Trainer's default mode ended with epoch 0).  The read and the reset are ordered against whatever stream replays the graphs by
	synchronising the device on both sides -- once per epoch."""
	bad = None
	for dev in list(_cap_used):
		t = _cap_flags[dev]
		torch.cuda.synchronize(dev)
		vals = t.tolist()
		if vals[0] > 0 or vals[1] > 0:
			t.zero_()
			torch.cuda.synchronize(dev)
			bad = bad or vals
	if bad is not None:
		_report(bad, 'renders replayed from a HIP graph since the last check', 'warn' if FLAG_POLICY == 'warn' else 'strict')


def check_render_flags(wait=False):
	"""Look at the counters of earlier renders that have arrived (all of them with wait=True): a warning per bad render under the
	'warn' policy, RuntimeError on the first bad one under 'strict' / 'sync'."""
	global _pending
	if wait and _cap_used and FLAG_POLICY != 'ignore':
		_check_captured()
	keep = []
	i = -1
	try:
		for i, (ev, slot, what, policy) in enumerate(_pending):
			if wait:
				ev.synchronize()
			if ev.query():
				vals = _slots[slot].tolist()
				_free.append(slot)
				_report(vals, what, policy)
			else:
				keep.append((ev, slot, what, policy))
	except RuntimeError:
		keep += _pending[i + 1:]
		raise
	finally:
		_pending = keep


def _watch(ws, what):
	global _slots
	if FLAG_POLICY == 'ignore':
		return
	dev = ws.device
	if torch.cuda.is_current_stream_capturing():
		t = _cap_flags.get(dev)   # (allocated by the eager warm-up step that precedes every capture; nothing may be allocated for good in here)
		if t is not None:
			t.add_(ws[:8].view(torch.int32))
			_cap_used.add(dev)
		return
	if dev not in _cap_flags:
		_cap_flags[dev] = torch.zeros(2, dtype=torch.int32, device=dev)
	check_render_flags()
	if not _free and _slots is not None:   # nobody ever looked and the ring is full: do it now rather than grow without bound
		check_render_flags(wait=True)
	if _slots is None:
		_slots = torch.zeros(_RING, 2, dtype=torch.int32).pin_memory()
		_free.extend(range(_RING))
		atexit.register(_flush_at_exit)
	slot = _free.pop()
	_slots[slot].copy_(ws[:8].view(torch.int32), non_blocking=True)
	ev = torch.cuda.Event()
	ev.record()
	_pending.append((ev, slot, what, 'strict' if FLAG_POLICY == 'async' else FLAG_POLICY))
	if FLAG_POLICY == 'sync':
		check_render_flags(wait=True)


def _flush_at_exit():
	"""The renders nobody looked at again: report them before the interpreter goes (a bad last render used to pass unseen)."""
	try:
		check_render_flags(wait=True)
	except RuntimeError as e:   # 'strict': nothing left to abort, say it
		warnings.warn(str(e), RuntimeWarning)
	except Exception:           # (the device may be gone already)
		pass


class _Render(torch.autograd.Function):
	@staticmethod
	def forward(ctx, verts, colors, faces, R, T, params, want_mask, want_image, want_frags):
		_require_gpu(verts, colors, R, T)
		L = _lib.lib()
		verts, colors, R, T = _c(verts), _c(colors), _c(R), _c(T)
		faces = _faces_i32(faces)
		N, V, _ = verts.shape
		M = R.shape[0]
		fb = 1 if faces.dim() == 2 else faces.shape[0]
		F = faces.shape[-2]
		H, W = params.image_h, params.image_w
		dev = verts.device
		nbytes = L.find_render_ws_bytes(ctypes.byref(params), N, M, V, F)
		if nbytes < 0:
			check(-1, 'find_render_ws_bytes')
		ws = _ws(nbytes, dev)
		mask = torch.empty(N, M, H, W, device=dev) if want_mask else None
		image = torch.empty(N, M, H, W, 3, device=dev) if want_image else None
		p2f = torch.empty(N, M, H, W, device=dev, dtype=torch.int32) if want_frags else None
		zbuf = torch.empty(N, M, H, W, device=dev) if want_frags else None
		check(L.find_render_fwd(ctypes.byref(params), ptr(verts), ptr(faces), fb, ptr(colors), ptr(R), ptr(T), N, M, V, F, ptr(mask), ptr(image),
								ptr(p2f), ptr(zbuf), ptr(ws), ws.numel(), current_stream(dev)), 'find_render_fwd')
		_watch(ws, f'render of {N} meshes x {M} views @{H}x{W}')
		ctx.params, ctx.ws, ctx.dims = params, ws, (N, M, V, F, fb)
		ctx.save_for_backward(verts, colors, faces, R, T, mask)
		ctx.mark_non_differentiable(*[t for t in (p2f, zbuf) if t is not None])
		# an output nothing reads hands None to backward, not a tensor of zeros: with the silhouette loss alone the whole RGB backward
		# (shading, vertex normals: ~0.2 ms at C3) used to run on zeros
		ctx.set_materialize_grads(False)
		return mask, image, p2f, zbuf

	@staticmethod
	def backward(ctx, g_mask, g_image, _gp, _gz):
		L = _lib.lib()
		verts, colors, faces, R, T, mask = ctx.saved_tensors
		N, M, V, F, fb = ctx.dims
		if g_mask is None and g_image is None:
			return (None,) * 9
		g_mask, g_image = _c(g_mask), _c(g_image)
		d_verts = torch.empty_like(verts)
		d_colors = torch.empty_like(colors) if (colors is not None and g_image is not None and ctx.needs_input_grad[1]) else None
		check(L.find_render_bwd(ctypes.byref(ctx.params), ptr(verts), ptr(faces), fb, ptr(colors), ptr(R), ptr(T), N, M, V, F, ptr(mask),
								ptr(g_mask), ptr(g_image), ptr(d_verts), ptr(d_colors), ptr(ctx.ws), ctx.ws.numel(),
								current_stream(verts.device)), 'find_render_bwd')
		return d_verts, d_colors, None, None, None, None, None, None, None


class _RenderFeatures(torch.autograd.Function):
	"""_Render plus the per-vertex feature render (find_render_features_fwd / _bwd) on the same raster pass: the forward always forms the
	mask (the feature render reads its K nearest silhouette candidates) and returns it only when asked for."""
	@staticmethod
	def forward(ctx, verts, colors, features, faces, R, T, params, want_mask, want_image, want_frags):
		_require_gpu(verts, colors, features, R, T)
		if params.clip_faces:
			raise NotImplementedError('find_amd.render: per-vertex features are not rendered in split mode (clip_faces=True): the feature '
									  'shader reads the K nearest silhouette candidates of unclipped faces')
		L = _lib.lib()
		verts, colors, features, R, T = _c(verts), _c(colors), _c(features), _c(R), _c(T)
		faces = _faces_i32(faces)
		N, V, _ = verts.shape
		M = R.shape[0]
		C = features.shape[-1]
		fb = 1 if faces.dim() == 2 else faces.shape[0]
		F = faces.shape[-2]
		H, W = params.image_h, params.image_w
		dev = verts.device
		nbytes = L.find_render_ws_bytes(ctypes.byref(params), N, M, V, F)
		fbytes = L.find_render_features_ws_bytes(ctypes.byref(params), N, M, C)
		if nbytes < 0 or fbytes < 0:
			check(-1, 'find_render_ws_bytes')
		ws, fws = _ws(nbytes, dev), _ws(fbytes, dev)
		mask = torch.empty(N, M, H, W, device=dev)
		image = torch.empty(N, M, H, W, 3, device=dev) if want_image else None
		p2f = torch.empty(N, M, H, W, device=dev, dtype=torch.int32) if want_frags else None
		zbuf = torch.empty(N, M, H, W, device=dev) if want_frags else None
		feat = torch.empty(N, M, H, W, C, device=dev)
		stream = current_stream(dev)
		check(L.find_render_fwd(ctypes.byref(params), ptr(verts), ptr(faces), fb, ptr(colors), ptr(R), ptr(T), N, M, V, F, ptr(mask), ptr(image),
								ptr(p2f), ptr(zbuf), ptr(ws), ws.numel(), stream), 'find_render_fwd')
		check(L.find_render_features_fwd(ctypes.byref(params), ptr(verts), ptr(faces), fb, ptr(R), ptr(T), N, M, V, F, ptr(features), C, ptr(feat),
										 ptr(ws), ws.numel(), ptr(fws), fws.numel(), stream), 'find_render_features_fwd')
		_watch(ws, f'render of {N} meshes x {M} views @{H}x{W} with {C} feature channels')
		ctx.params, ctx.ws, ctx.fws, ctx.dims = params, ws, fws, (N, M, V, F, fb, C)
		ctx.save_for_backward(verts, colors, features, faces, R, T, mask, feat)
		ctx.mark_non_differentiable(*[t for t in (p2f, zbuf) if t is not None])
		ctx.set_materialize_grads(False)
		return (mask if want_mask else None), image, p2f, zbuf, feat

	@staticmethod
	def backward(ctx, g_mask, g_image, _gp, _gz, g_feat):
		L = _lib.lib()
		verts, colors, features, faces, R, T, mask, feat = ctx.saved_tensors
		N, M, V, F, fb, C = ctx.dims
		stream = current_stream(verts.device)
		d_verts = d_colors = d_features = None
		if g_mask is not None or g_image is not None:
			g_mask, g_image = _c(g_mask), _c(g_image)
			d_verts = torch.empty_like(verts)
			d_colors = torch.empty_like(colors) if (colors is not None and g_image is not None and ctx.needs_input_grad[1]) else None
			check(L.find_render_bwd(ctypes.byref(ctx.params), ptr(verts), ptr(faces), fb, ptr(colors), ptr(R), ptr(T), N, M, V, F, ptr(mask),
									ptr(g_mask), ptr(g_image), ptr(d_verts), ptr(d_colors), ptr(ctx.ws), ctx.ws.numel(), stream), 'find_render_bwd')
		if g_feat is not None and (ctx.needs_input_grad[0] or ctx.needs_input_grad[2]):
			g_feat = _c(g_feat)
			if d_verts is None and ctx.needs_input_grad[0]:
				d_verts = torch.zeros_like(verts)
			d_features = torch.empty_like(features) if ctx.needs_input_grad[2] else None
			check(L.find_render_features_bwd(ctypes.byref(ctx.params), ptr(verts), ptr(faces), fb, ptr(R), ptr(T), N, M, V, F, ptr(features), C,
											 ptr(feat), ptr(g_feat), ptr(d_verts), ptr(d_features), ptr(ctx.ws), ctx.ws.numel(), ptr(ctx.fws),
											 ctx.fws.numel(), stream), 'find_render_features_bwd')
		return d_verts, d_colors, d_features, None, None, None, None, None, None, None


def _check_features(features, verts):
	if not isinstance(features, torch.Tensor) or not features.is_floating_point():
		raise ValueError('find_amd.render: features must be a float tensor (N,V,C)')
	if features.dim() != 3 or features.shape[0] != verts.shape[0] or features.shape[1] != verts.shape[1] or features.shape[2] < 1:
		raise ValueError(f'find_amd.render: features must be (N,V,C) = ({verts.shape[0]},{verts.shape[1]},C >= 1), got {tuple(features.shape)}')
	if features.device != verts.device or not features.is_cuda:
		raise ValueError(f'find_amd.render: features must be on the mesh\'s ROCm device, got features on {features.device}, the mesh on {verts.device}')
	return features.float()


def render(verts, colors, faces, R, T, params, want_mask=True, want_image=True, want_frags=False, features=None):
	"""verts (N,V,3), colors (N,V,3)|None, faces (F,3)|(N,F,3), R (M,3,3), T (M,3)  ->  mask (N,M,H,W), image (N,M,H,W,3),
	pix_to_face (N,M,H,W) int32, zbuf (N,M,H,W)   (entries not requested are None).
	features (N,V,C): also the feature maps (N,M,H,W,C) as a fifth entry -- FeatureShader + softmax_blend (znear 1, zfar 100, background 0)
	on the K-nearest silhouette fragments, differentiable in the features and the vertices, from the same raster pass."""
	if want_image and colors is None:
		raise RuntimeError('find_amd.render: an RGB image needs per-vertex colours')
	if features is not None:
		features = _check_features(features, verts)
		return _RenderFeatures.apply(verts, colors, features, faces, R, T, params, want_mask, want_image, want_frags)
	return _Render.apply(verts, colors, faces, R, T, params, want_mask, want_image, want_frags)


def render_flags(ws):
	"""(faces straddling the clip plane, pixels with more than 4096 silhouette candidates -- the only ones the K-nearest rule
	leaves unresolved) of the forward that used ws."""
	L = _lib.lib()
	out = (ctypes.c_int32 * 2)()
	check(L.find_render_flags(ptr(ws), ctypes.cast(out, ctypes.c_void_p), current_stream(ws.device)), 'find_render_flags')
	return int(out[0]), int(out[1])


def uv_sample(maps, verts_uvs, faces_uvs, face_idx, bary):
	"""Colours of surface points from UV maps (TexturesUV.sample_textures): maps (Nm,H,W,3), verts_uvs (Nm,Vt,2), faces_uvs (Nm|1,F,3),
	face_idx (R,P) local face ids (-1 -> zeros), bary (R,P,3), R a multiple of Nm with the rows of one map consecutive.  No gradient
	(the reference only ever samples GT scans)."""
	_require_gpu(maps, verts_uvs, bary)
	L = _lib.lib()
	maps, verts_uvs, bary = _c(maps.detach()), _c(verts_uvs.detach()), _c(bary.detach())
	fu = _faces_i32(faces_uvs)
	fi = face_idx if face_idx.dtype == torch.int32 else face_idx.to(torch.int32)
	fi = fi.contiguous()
	fb = 1 if fu.dim() == 2 else fu.shape[0]
	Rr, P = fi.shape
	out = torch.empty(Rr, P, 3, device=maps.device, dtype=torch.float32)
	check(L.find_uv_sample(ptr(maps), maps.shape[0], maps.shape[1], maps.shape[2], ptr(verts_uvs), verts_uvs.shape[1], ptr(fu), fb, fu.shape[-2], ptr(fi), ptr(bary),
						   Rr, P, ptr(out), current_stream(maps.device)), 'find_uv_sample')
	return out


def render_frags(ws, params, n_meshes, n_views, n_verts, n_faces):
	"""(local face id (N,M,H,W) int32, perspective-correct barycentrics (N,M,H,W,3)) of the forward that used `ws`."""
	L = _lib.lib()
	H, W = params.image_h, params.image_w
	f = torch.empty(n_meshes, n_views, H, W, device=ws.device, dtype=torch.int32)
	b = torch.empty(n_meshes, n_views, H, W, 3, device=ws.device, dtype=torch.float32)
	check(L.find_render_frags(ctypes.byref(params), n_meshes, n_views, n_verts, n_faces, ptr(ws), ptr(f), ptr(b), current_stream(ws.device)), 'find_render_frags')
	return f, b


def render_uv(verts, tex, faces, R, T, params, want_mask=True, want_frags=False, features=None):
	"""FootRenderer image of UV-textured meshes (GT scans; no gradient): the Phong + softmax blend is linear in the texture colour, so
	image = o0 + (o1 - o0) * texel with o0 / o1 the renders with black / white vertex colours and texel the map read at every pixel's
	nearest fragment.  Returns (mask, image, pix_to_face, zbuf), and with features (N,V,C) the feature maps (N,M,H,W,C) as a fifth entry."""
	with torch.no_grad():
		N, V, _ = verts.shape
		M = R.shape[0]
		Fn = faces.shape[-2]
		ones = torch.ones(N, V, 3, device=verts.device)
		L = _lib.lib()
		if features is not None:
			features = _check_features(features, verts)
			mask, o1, p2f, zbuf, feat = _RenderFeatures.apply(verts, ones, features, faces, R, T, params, want_mask, True, True)
		else:
			mask, o1, p2f, zbuf = _Render.apply(verts, ones, faces, R, T, params, want_mask, True, True)
		# the fragments of that forward (its workspace is not exposed by autograd.Function: run the raster once more for the buffers)
		vv, ff = _c(verts), _faces_i32(faces)
		fb = 1 if ff.dim() == 2 else ff.shape[0]
		ws = _ws(L.find_render_ws_bytes(ctypes.byref(params), N, M, V, Fn), verts.device)
		o0 = torch.empty_like(o1)
		zeros = torch.zeros_like(ones)
		check(L.find_render_fwd(ctypes.byref(params), ptr(vv), ptr(ff), fb, ptr(zeros), ptr(_c(R)), ptr(_c(T)), N, M, V, Fn, None, ptr(o0), None, None,
								ptr(ws), ws.numel(), current_stream(verts.device)), 'find_render_fwd')
		fl, bary = render_frags(ws, params, N, M, V, Fn)
		H, W = params.image_h, params.image_w
		texel = uv_sample(tex.maps_padded(), tex.verts_uvs_padded(), tex.faces_uvs_padded(), fl.reshape(N, M * H * W), bary.reshape(N, M * H * W, 3))
		image = o0 + (o1 - o0) * texel.reshape(N, M, H, W, 3)
	out = (mask, image, (p2f if want_frags else None), (zbuf if want_frags else None))
	return out + (feat,) if features is not None else out


def render_points(points, features, R, T, image_size, radius=0.03, points_per_pixel=10, fov_deg=60.0, return_fragments=False):
	"""PyTorch3D's PointsRasterizer + PointsRenderer(AlphaCompositor()) as FootRenderer draws keypoints (renderer.py:139-142, 365-376):
	points, features (N,P,3) world space, R (M,3,3), T (M,3)  ->  image (N,M,H,W,3), cloud n drawn in each of the M views, 0 where no
	point lands.  A point covers a pixel if its NDC distance is below `radius`; each pixel composites its `points_per_pixel` (1 .. 32)
	nearest points in view-space z front to back with weight 1 - d^2 / radius^2.  return_fragments: also (idx (N,M,H,W,K) int32 point
	index within the cloud, zbuf (view-space z), dists (d^2)), -1 in empty slots.  Forward only: nothing in FIND trains through this
	render, and it raises if a gradient would be needed."""
	if torch.is_grad_enabled() and (points.requires_grad or features.requires_grad):
		raise RuntimeError('find_amd.render_points: the point render has no backward; call it under torch.no_grad() or on detached tensors')
	_require_gpu(points, features, R, T)
	if points.dim() != 3 or points.shape[-1] != 3 or features.shape != points.shape:
		raise ValueError(f'find_amd.render_points: points and features must both be (N,P,3), got {tuple(points.shape)} / {tuple(features.shape)}')
	if R.dim() != 3 or R.shape[1:] != (3, 3) or T.shape != (R.shape[0], 3):
		raise ValueError(f'find_amd.render_points: R (M,3,3) and T (M,3) expected, got {tuple(R.shape)} / {tuple(T.shape)}')
	p = PointsParams()
	if isinstance(image_size, (tuple, list)):
		p.image_h, p.image_w = int(image_size[0]), int(image_size[1])
	else:
		p.image_h = p.image_w = int(image_size)
	p.fov_deg, p.radius, p.points_per_pixel = fov_deg, radius, int(points_per_pixel)
	points, features = _c(points.detach()), _c(features.detach())
	R, T = _c(R.detach().to(points.device)), _c(T.detach().to(points.device))
	N, P, _ = points.shape
	M = R.shape[0]
	H, W, K = p.image_h, p.image_w, p.points_per_pixel
	dev = points.device
	image = torch.empty(N, M, H, W, 3, device=dev)
	frags = None
	if return_fragments:
		shape = (N, M, H, W, max(K, 1))
		frags = (torch.empty(shape, device=dev, dtype=torch.int32), torch.empty(shape, device=dev), torch.empty(shape, device=dev))
	idx, zbuf, dists = frags if frags is not None else (None, None, None)
	check(_lib.lib().find_points_render(ctypes.byref(p), ptr(points), ptr(features), ptr(R), ptr(T), N, M, P, ptr(image), ptr(idx), ptr(zbuf),
										ptr(dists), current_stream(dev)), 'find_points_render')
	return (image, frags) if return_fragments else image
