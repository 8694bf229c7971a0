"""FootRenderer on the MI355X hot path: host-side mirror of reference src/model/renderer.py (same class name, constructor
keywords, view helpers and forward() keywords / outputs); all rendering arithmetic runs in libfind_hip.so
(find_amd.functional_render).  Keypoints are drawn as PyTorch3D's point renderer draws them (functional_render.render_points, one HIP
kernel); per-vertex features (return_features=True, features=(N,V,C)) as FeatureShader draws them on the K-nearest silhouette fragments
(find_render_features_fwd / _bwd, on the same raster pass as the mask and the image)."""
from typing import Union

import numpy as np
import torch

from . import functional as FN
from . import functional_render as FR
from .cameras import look_at_view_transform
from .structures import Meshes, TexturesUV, TexturesVertex

nn = torch.nn


class FootRenderer(nn.Module):
	def __init__(self, image_size, device='cuda', background_color=(1., 1., 1.), bin_size=None, z_clip_value=None, max_faces_per_bin=None,
				 clip_faces=False):
		"""bin_size / max_faces_per_bin are accepted for signature compatibility: binning is an acceleration structure of
		PyTorch3D's CUDA rasteriser and must not change results; the HIP rasteriser tiles internally.
		clip_faces (not in the reference): faces that straddle the z-clip plane are split as PyTorch3D's rasterize_meshes does (close-up
		views, cameras inside the mesh); off, such a render is reported by functional_render's watchdog instead."""
		super().__init__()
		self.image_size = image_size
		self.device = device
		self.background_color = tuple(float(c) for c in background_color)
		self.bin_size, self.max_faces_per_bin = bin_size, max_faces_per_bin
		self.light_location = (0., 0., 100.)  # PointLights(location=[[0, 0, 100]])  (renderer.py:114)
		# PointsRasterizationSettings(image_size, radius=0.03, points_per_pixel=10) + AlphaCompositor() (renderer.py:139-142)
		self.points_radius, self.points_per_pixel = 0.03, 10
		self.params = FR.make_params(image_size, faces_per_pixel=100, background=self.background_color, light_pos=self.light_location,
									 znear=0.02, z_clip=z_clip_value, clip_faces=clip_faces)

	# ------------------------------------------------------------------ camera poses
	# Every FIND camera looks along a ray through `at` with the world x axis as "up" (the foot's long axis; renderer.py:152,171,198).
	# What the callers rely on: (i) sample_views draws distance, elevation, azimuth -- in that order, `nviews` values each -- from numpy's
	# GLOBAL generator and reseeds it only for a truthy seed (renderer.py:146-151: `if seed`, so seed=0 means "do not reseed");
	# (ii) the six named poses below (renderer.py:176-196).  Both are data that must match; the code around them is this file's own.
	UP = ((1, 0, 0),)
	NAMED_VIEWS = {   # name: (dist, elev, azim, look-at point)
		'topdown': (0.30, 0, 0, (0, 0, 0)),
		'side1': (0.35, 90, 0, (0, 0, 0)),
		'side2': (0.35, -90, 180, (0, 0, 0)),
		'toes': (0.10, 0, 0, (0.1, 0, 0)),
		'45': (0.35, -45, 0, (0, 0, 0)),
		'60': (0.35, -60, 0, (0, 0, 0)),
	}

	@classmethod
	def _poses(cls, dist, elev, azim, at=((0, 0, 0),)):
		return look_at_view_transform(dist=dist, elev=elev, azim=azim, up=cls.UP, at=at)

	def sample_views(self, nviews=1, dist_mean=.25, dist_std=0.05, elev_min=-90, elev_max=90, azim_min=0, azim_max=360, seed: int = None):
		"""Random poses: dist ~ N(dist_mean, dist_std), elev ~ U(elev_min, elev_max), azim ~ U(azim_min, azim_max), degrees."""
		if seed:
			np.random.seed(seed)
		draws = [np.random.normal(dist_mean, dist_std, nviews)]
		draws += [np.random.uniform(lo, hi, nviews) for lo, hi in ((elev_min, elev_max), (azim_min, azim_max))]
		return self._poses(*draws)

	def linspace_views(self, nviews=1, dist=.3, dist_min=None, dist_max=None, elev_min=None, elev_max=None, azim_min=None, azim_max=None,
					   at=((0, 0, 0),)):
		"""Evenly spaced poses: each of dist / elev / azim sweeps its [min, max] when a min is given, else stays at dist / 0 / 0."""
		def sweep(lo, hi, fixed):
			return fixed if lo is None else np.linspace(lo, hi, nviews)
		return self._poses(sweep(dist_min, dist_max, dist), sweep(elev_min, elev_max, 0), sweep(azim_min, azim_max, 0), at=at)

	def view_from(self, view_kw='topdown'):
		"""One pose per name in NAMED_VIEWS (a name or a list of names)."""
		names = [view_kw] if isinstance(view_kw, str) else list(view_kw)
		for v in names:
			assert v in self.NAMED_VIEWS, f'View description `{view_kw}` not understood'
		dist, elev, azim, at = zip(*(self.NAMED_VIEWS[v] for v in names))
		return self._poses(np.array(dist), np.array(elev), np.array(azim), at=np.array(at, dtype=np.float64))

	def combine_views(self, R1, T1, R2, T2):
		return torch.cat([R1, R2], dim=0), torch.cat([T1, T2], dim=0)

	# ------------------------------------------------------------------ render
	def forward(self, input_meshes: Meshes, R, T, return_images=True, return_depth=False, return_mask=False, mask_with_grad=True,
				mask_out_faces=False, masked_faces=None, keypoints=None, keypoints_blend=False, lights=None, return_mask_out_masks=False,
				return_features=False, features=None, return_normals=False, normals_space='view') -> dict:
		"""Render N meshes from M views: image [N,M,H,W,3], mask [N,M,H,W] (soft silhouette when mask_with_grad), optional
		depth and mask-out masks (reference renderer.py:247-383).  Image index = mesh*M + view.
		keypoints (N,P,3): out['keypoints'] (N,M,H,W,3), the points drawn red by PyTorch3D's point renderer (functional_render.render_points;
		no depth test against the mesh, no gradient) -- mesh n's keypoints in each of its M views, as renderer.py:367 meant (upstream's own
		line discards that expansion and works for M = 1 only); with keypoints_blend also out['keypoints_blend'], the image with the
		splats over it (~any(pcl > 0) * image + any(pcl > 0) * pcl), which needs return_images.  keypoints_blend without keypoints is
		ignored, as upstream.
		return_features with features (N,V,C): out['features'] (N,M,H,W,C), the per-vertex features blended as FeatureShader does
		(renderer.py:293-299: softmax_blend over the K = 100 silhouette fragments, znear 1, zfar 100, background 0), differentiable in the
		features and the vertices; 0 where mask_out_faces hides a pixel.  Upstream needs return_mask=True as well (fragments['sil'] only
		exists then); here the silhouette pass runs either way and out['mask'] is returned only when asked for.  Not in split mode
		(clip_faces=True).
		return_normals (not in the reference): out['normals'] (N,M,H,W,3), unit surface normals in the camera frame of each view
		(normals_space='view': n_world @ R[view]) or in world space ('world'), 0 on the background and where mask_out_faces hides a pixel:
		functional.normal_map of the feature render of the mesh's vertex normals (Meshes.verts_normals_padded), so differentiable to the
		vertices through the normals and through the blend.  Together with return_features the normals are a feature render of their own
		on a second raster pass: each output is what the call that asks for it alone returns.  Not in split mode either.
		return_depth: out['depth'] (N,M,H,W), view-space z of the nearest face, -1 on the background.  Where gradients are enabled and the
		vertices require one it is differentiable to them (functional.depth_map; PyTorch3D's fragments.zbuf), in split mode too; the values
		are the same either way.  UV-textured scans stay without gradient."""
		if keypoints is not None:
			if keypoints_blend and not return_images:   # (a NameError upstream)
				raise ValueError('FootRenderer: keypoints_blend draws the keypoints over the image: it needs return_images=True')
			if keypoints.dim() != 3 or keypoints.shape[-1] != 3 or keypoints.shape[0] != len(input_meshes):
				raise ValueError(f'FootRenderer: keypoints must be (N,P,3) with N = {len(input_meshes)} meshes, got {tuple(keypoints.shape)}')
		if (return_features or return_normals) and self.params.clip_faces:
			raise NotImplementedError('FootRenderer: per-vertex features are not rendered with clip_faces=True: the feature shader reads '
									  'the K nearest silhouette candidates of unclipped faces (split mode is out of scope for it)')
		if return_normals and normals_space not in ('view', 'world'):
			raise ValueError(f"FootRenderer: normals_space 'view' or 'world', got {normals_space!r}")
		if return_features:
			if features is None:   # (an assert upstream)
				raise ValueError('FootRenderer: return_features needs features (N,V,C)')
			nv = input_meshes.verts_padded().shape[:2]
			if (not isinstance(features, torch.Tensor) or not features.is_floating_point() or features.dim() != 3
					or tuple(features.shape[:2]) != tuple(nv) or features.shape[2] < 1):
				raise ValueError(f'FootRenderer: features must be a float tensor (N,V,C) with N = {nv[0]} meshes and V = {nv[1]} vertices, got '
								 + (f'{tuple(features.shape)} {features.dtype}' if isinstance(features, torch.Tensor) else type(features).__name__))
			if features.device != input_meshes.device or not features.is_cuda:
				raise ValueError(f'FootRenderer: features must be on the mesh\'s ROCm device ({input_meshes.device}), got {features.device}')
		if lights is not None:
			raise NotImplementedError('custom lights are not used on the FIND path; the renderer keeps PointLights((0,0,100))')
		dev = input_meshes.device
		R, T = R.to(dev).float(), T.to(dev).float()
		N, M = len(input_meshes), R.shape[0]
		verts = input_meshes.verts_padded()
		faces = input_meshes.faces_shared()
		if faces is None:
			faces = input_meshes.faces_padded()
		F = faces.shape[-2]
		colors = None
		tex = input_meshes.textures
		uv_tex = isinstance(tex, TexturesUV)
		if return_images and not uv_tex:
			if not isinstance(tex, TexturesVertex):
				raise NotImplementedError('return_images needs TexturesVertex or TexturesUV textures')
			colors = tex.verts_features_padded()[..., :3]
		want_soft = return_mask and (mask_with_grad or not return_images)
		# (pix_to_face is read below only to hide faces: when the caller names some, or for UV textures' (0,0)-UV convention)
		want_frags = (mask_out_faces and (masked_faces is not None or uv_tex)) or return_depth
		# the normals travel as three feature channels: the call's own feature render when it has no other, else one more (see above)
		vnormals = input_meshes.verts_normals_padded() if return_normals else None
		if return_normals and not return_features:
			features = vnormals
		with_feat = return_features or return_normals
		if not (return_images or want_soft or want_frags or with_feat):
			return self._keypoints(dict(), None, keypoints, keypoints_blend, R, T, dev)
		if return_images and uv_tex:
			# GT scans (dataset.py:263-271): no gradient flows to a UV-textured mesh anywhere in the reference
			if verts.requires_grad:
				raise NotImplementedError('UV-textured meshes are rendered without gradient (GT scans); use TexturesVertex for predicted meshes')
			res = FR.render_uv(verts, tex, faces, R, T, self.params, want_mask=want_soft, want_frags=want_frags,
							   features=features if with_feat else None)
		else:
			res = FR.render(verts, colors, faces, R, T, self.params, want_mask=want_soft, want_image=return_images, want_frags=want_frags,
							features=features if with_feat else None)
		mask, renders, p2f, zbuf = res[:4]
		feat = res[4] if with_feat else None
		nraw = None
		if return_normals:
			nraw = feat if not return_features else FR.render(verts, None, faces, R, T, self.params, want_mask=False, want_image=False,
															  features=vnormals)[4]
		out = dict()
		if return_depth:
			# (with a gradient to carry, the z-buffer goes through functional.depth_map: the same values, and find_depth_bwd behind them)
			with_grad = torch.is_grad_enabled() and verts.requires_grad and not (return_images and uv_tex)
			out['depth'] = FN.depth_map(verts, faces, R, T, self.params, p2f, zbuf) if with_grad else zbuf
		if return_mask and not want_soft:  # hard mask from the image render (renderer.py:313)
			mask = torch.any(renders < 1, dim=-1).float()

		# (the all-False map costs a 16-MB fill @512^2: it is made where somebody hides faces or asks for the map, and `nothing_hidden` -- not in
		# the reference -- tells ModelWithLoss that copying it into the prediction would change nothing)
		hides = mask_out_faces and (masked_faces is not None or uv_tex)
		mask_out = torch.zeros((N, M, self.params.image_h, self.params.image_w), dtype=torch.bool, device=dev) if (hides or return_mask_out_masks) else None
		nothing_hidden = not hides
		if hides:
			img = torch.arange(N * M, device=dev, dtype=torch.int32).view(N, M, 1, 1)
			local = torch.where(p2f >= 0, p2f - img * F, p2f)  # face count within the mesh (renderer.py:322-327)
			for n in range(N):
				if masked_faces is not None:
					mf = masked_faces[n] if isinstance(masked_faces, list) else masked_faces
				else:
					# TexturesUV convention (renderer.py:340-349): a final UV vertex at (0, 0) marks faces to mask out -- those whose three
					# UV indices all point at it; the first mesh without the marker ends the search, as the reference's `break`
					vu, fu = tex.verts_uvs_padded()[n], tex.faces_uvs_padded()[n]
					if not bool((vu[-1] == 0).all()):
						nothing_hidden = nothing_hidden or n == 0
						break
					mf = torch.argwhere(torch.all(fu == vu.shape[0] - 1, dim=-1)).flatten()
				mask_out[n] = torch.isin(local[n], mf.to(dev).to(local.dtype))
			if return_images:
				renders = torch.where(mask_out.unsqueeze(-1), torch.ones_like(renders), renders)
			if return_mask:
				mask = torch.where(mask_out, torch.zeros_like(mask), mask)
			if with_feat:   # (renderer.py:361-363)
				feat = torch.where(mask_out.unsqueeze(-1), torch.zeros_like(feat), feat)
			if return_normals:
				nraw = feat if not return_features else torch.where(mask_out.unsqueeze(-1), torch.zeros_like(nraw), nraw)

		self._keypoints(out, renders, keypoints, keypoints_blend, R, T, dev)
		if return_images:
			out['image'] = renders
		if return_mask:
			out['mask'] = mask
		if return_mask_out_masks:
			out['mask_out_masks'] = mask_out
			out['nothing_hidden'] = nothing_hidden
		if return_features:
			out['features'] = feat
		if return_normals:
			out['normals'] = FN.normal_map(nraw, R, space=normals_space)
		return out

	def _keypoints(self, out, renders, keypoints, keypoints_blend, R, T, dev):
		"""out['keypoints'] (and out['keypoints_blend'] over `renders`) as renderer.py:365-376 forms them."""
		if keypoints is None:
			return out
		kp = keypoints.to(dev).float()
		features = torch.zeros_like(kp)
		features[..., 0] = 1
		pcl = FR.render_points(kp, features, R, T, (self.params.image_h, self.params.image_w), radius=self.points_radius,
							   points_per_pixel=self.points_per_pixel, fov_deg=self.params.fov_deg)
		out['keypoints'] = pcl
		if keypoints_blend:
			pcl_mask = torch.any(pcl > 0, dim=-1).unsqueeze(-1)
			out['keypoints_blend'] = ~pcl_mask * renders + pcl_mask * pcl
		return out
