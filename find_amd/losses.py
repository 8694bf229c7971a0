"""FIND's 3-D and silhouette losses on the MI355X hot path: host-side mirror of reference src/model/losses.py (same class
names and forward signatures); the arithmetic runs in libfind_hip.so through find_amd.functional.

In scope: TextureLossGTSpace, DisplacementLoss (Chamfer, incl. the z-cut-off variants),
MeshSmoothnessLoss, SilhouetteLoss, ContrastiveLoss, and the cluster mode of RestylePerceptualLoss on rendered per-vertex class
logits (the encoder is the caller's).  The other perceptual / Restyle modes need absent network weights or submodules and are out of
scope."""
import itertools
import os

import numpy as np
import torch

from . import functional as FN
from . import functional_render as FR
from . import measure as _measure
from . import ssim as _ssim
from .structures import Meshes, TexturesUV, TexturesVertex

nn = torch.nn
# the Chamfer term's backward as one kernel from the neighbours to the predicted vertices (DisplacementLoss.forward) where the measured size
# rule says it pays (functional.surface_chamfer_pays); FIND_FUSED_CHAMFER_BWD=0: never -- the sampler's and the Chamfer distance's own
# backward passes, as before; 2: wherever it fits (tests, A/B runs)
FUSED_CHAMFER_BWD = int(os.environ.get('FIND_FUSED_CHAMFER_BWD', '1'))


def sample_points_from_meshes(meshes: Meshes, num_samples: int = 10000, return_textures: bool = False, generator=None, draws=None):
	"""pytorch3d.ops.sample_points_from_meshes: faces ~ multinomial(area) with replacement, (w0,w1,w2) = (1-sqrt(u),
	sqrt(u)(1-v), sqrt(u)v).  The uniform draws come from torch's generator on the mesh device; the areas, the face
	choice and the gather / lerp run in find_sample_surface_fwd.  draws=(face_idx (N,S) int, uv (N,S,2)) replays given draws for
	reproducible CPU/GPU comparisons (find_sample_points_fwd)."""
	verts = meshes.verts_padded()
	faces = meshes.faces_shared()
	if faces is None:
		faces = meshes.faces_padded()
	N = verts.shape[0]
	tex = meshes.textures if return_textures else None
	if return_textures and not isinstance(tex, (TexturesUV, TexturesVertex)):
		raise NotImplementedError('return_textures needs TexturesVertex or TexturesUV')
	attr = tex.verts_features_padded()[..., :3].contiguous() if isinstance(tex, TexturesVertex) else None
	if draws is None:
		# one launch for the draws (torch's device generator, where PyTorch3D draws), two for areas -> running sum -> search -> gather
		rnd = torch.rand(N, num_samples, 3, device=verts.device, generator=generator)
		pts, cols, face_idx, uv = FN.sample_surface(verts, faces, rnd, attr)
	else:
		face_idx, uv = draws
		r = FN.sample_points(verts, faces, face_idx, uv, attr)
		pts, cols = r if attr is not None else (r, None)
	if not return_textures:
		return pts
	if isinstance(tex, TexturesUV):
		# PyTorch3D: barycentrics of the sample (w0 = 1 - sqrt(u), w1 = sqrt(u)(1 - v), w2 = sqrt(u) v), then TexturesUV.sample_textures
		su = uv[..., 0].sqrt()
		bary = torch.stack([1.0 - su, su * (1.0 - uv[..., 1]), su * uv[..., 1]], dim=-1)
		return pts, FR.uv_sample(tex.maps_padded(), tex.verts_uvs_padded(), tex.faces_uvs_padded(), face_idx, bary)
	return pts, cols


def _compact_by_mask(points, keep):
	"""Move the kept points of every cloud to the front (stable) and return (padded points, lengths): the padded-tensor form
	of the ragged Pointclouds the reference builds for its z cut-offs (losses.py:69-85)."""
	order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)
	return torch.gather(points, 1, order.unsqueeze(-1).expand(-1, -1, 3)), keep.sum(dim=1).to(torch.int32)


def chamfer_distance(x, y, x_lengths=None, y_lengths=None):
	return FN.chamfer_distance(x, y, x_lengths, y_lengths)


def _mesh_faces(meshes):
	faces = meshes.faces_shared()
	return faces if faces is not None else meshes.faces_padded()


def point_mesh_distance(points, meshes: Meshes, lengths=None):
	"""functional.point_face_distance on a Meshes (shared or ragged, -1 padded faces): (dist2 (N,P), idx (N,P) int32, bary (N,P,3)) of
	points (N,P,3) against the surface of mesh n; lengths (N): the point counts of a padded batch.  Differentiable in the points and in the
	meshes' vertices."""
	return FN.point_face_distance(points, meshes.verts_padded(), _mesh_faces(meshes), lengths)


class TextureLossGTSpace(nn.Module):
	def forward(self, model, batch: dict, num_samples=1000, shapevec=None, texvec=None, posevec=None, gt_samples=None) -> torch.Tensor:
		"""Sample points + colours on the GT meshes, query the colour field there, masked L2 (reference losses.py:22-57).
		gt_samples (not in the reference): (points, colours) already drawn on batch['mesh'] -- ModelWithLoss draws the GT samples of a step
		before the main pass, beside it (they depend on the batch alone)."""
		mesh_gt = batch['mesh']
		sampled_verts, sampled_gt_colours = gt_samples if gt_samples is not None else sample_points_from_meshes(mesh_gt, num_samples=num_samples, return_textures=True)
		texvec = texvec if texvec is not None else batch.get('texvec', None)
		shapevec = shapevec if shapevec is not None else batch.get('shapevec', None)
		posevec = posevec if posevec is not None else batch.get('posevec', None)
		# (only the colour head is read below: a model that can skip the displacement head does)
		# (... and its weight gradients may trail behind the rest of the backward pass: nothing reads them before the pass ends)
		only_col = dict(want=('col',), defer_wgrad_join=True) if 'want' in getattr(getattr(model.forward, '__code__', None), 'co_varnames', ()) else {}
		res = model(sampled_verts.detach(), texvec=texvec, shapevec=shapevec, posevec=posevec, **only_col)
		# F.mse_loss(reduction='none') * mask, .mean() with mask = any(gt < 1) per point (losses.py:43,55-57), as one kernel
		return FN.masked_mse(res['col'], sampled_gt_colours)


class DisplacementLoss(nn.Module):
	def forward(self, model, res, batch, epoch, num_samples=5000, z_cutoff=None, gt_z_cutoff=None, gt_samples=None):
		"""Chamfer distance between surface samples of the GT and the predicted meshes (reference losses.py:59-90).
		gt_samples (not in the reference): the GT samples, already drawn (see TextureLossGTSpace.forward)."""
		if gt_samples is None:
			gt_samples = sample_points_from_meshes(batch['mesh'], num_samples=num_samples)
		pred_samples = sample_points_from_meshes(res['meshes'], num_samples=num_samples)
		src = FN.surface_of(pred_samples) if FUSED_CHAMFER_BWD and z_cutoff is None and torch.is_grad_enabled() and not gt_samples.requires_grad else None
		if (src is not None and (FUSED_CHAMFER_BWD >= 2 or FN.surface_chamfer_pays(pred_samples.shape[0], pred_samples.shape[1]))
				and FN.surface_chamfer_fits(pred_samples.shape[0], src[0].shape[1], pred_samples.shape[1])):
			# the predicted samples reach the Chamfer term as the sampler made them: the same loss, and a backward that goes from the neighbours
			# straight to the predicted vertices in one kernel (functional.surface_chamfer_distance); the sampler's own node stays unused
			g, gl = _compact_by_mask(gt_samples, gt_samples[..., 2] <= gt_z_cutoff) if gt_z_cutoff is not None else (gt_samples, None)
			return dict(loss=FN.surface_chamfer_distance(pred_samples, g, gl))
		if z_cutoff is not None:
			p, pl = _compact_by_mask(pred_samples, pred_samples[..., 2] <= z_cutoff)
			g, gl = _compact_by_mask(gt_samples, gt_samples[..., 2] <= z_cutoff)
			chamf_loss, _ = chamfer_distance(p, g, pl, gl)
		elif gt_z_cutoff is not None:
			g, gl = _compact_by_mask(gt_samples, gt_samples[..., 2] <= gt_z_cutoff)
			chamf_loss, _ = chamfer_distance(pred_samples, g, None, gl)
		else:
			chamf_loss, _ = chamfer_distance(pred_samples, gt_samples)
		return dict(loss=chamf_loss)


class MeshSmoothnessLoss(nn.Module):
	def forward(self, meshes: Meshes):
		"""0.1 * cotangent-Laplacian smoothing + 10 * edge-length loss (reference losses.py:93-99)."""
		faces = meshes.faces_shared()
		if faces is None:
			raise NotImplementedError('MeshSmoothnessLoss expects meshes sharing one topology (the template), as on the FIND path')
		verts = meshes.verts_padded()
		topo = FN.MeshTopology.get(faces, verts.shape[1])
		return FN.mesh_smoothness_loss(verts, topo, w_edge=10.0, w_lap=0.1)


class SilhouetteLoss(nn.Module):
	def forward(self, pred, gt):
		"""MSE of the soft silhouettes (reference losses.py:122-128: nn.MSELoss), one pass each way in find_image_mse_*."""
		return FN.image_mse(pred, gt)


def draw_pairs(N, npairs=10):
	"""The pairs ContrastiveLoss.forward draws (reference losses.py:326-331), with the same numpy calls on numpy's global generator --
	same pairs, same generator state afterwards: min(npairs, N(N-1)/2) ORDERED pairs of distinct rows, (P, 2) int32 on the host."""
	max_pairs = (N * (N - 1)) // 2
	npairs = min(npairs, max_pairs)
	all_pairs = list(itertools.permutations(np.arange(N), 2))
	np.random.shuffle(all_pairs)
	return np.array(all_pairs[:npairs], dtype=np.int32).reshape(-1, 2)


def pairs_to_device(pairs, device):
	"""Host (P, 2) pairs -> device int32, through pinned memory (no wait for the queue to drain)."""
	t = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32))
	if torch.device(device).type != 'cuda':
		return t
	return t.pin_memory().to(device, non_blocking=True)


class ContrastiveLoss(nn.Module):
	"""Contrastive loss of pose vectors against pose codes (reference losses.py:305-333), one HIP launch each way (functional.contrastive_pose)."""

	def crit(self, vec1, vec2, code1, code2, margin=0.5):
		"""L = y d^2 + (1 - y) max(margin - d^2, 0)^2 for one pair, y = <code1, code2>, d = ||vec1 - vec2|| (losses.py:307-319)."""
		vecs = torch.stack([vec1, vec2])
		codes = torch.stack([code1, code2]).to(device=vecs.device, dtype=torch.float32)
		return FN.contrastive_pose(vecs, codes, pairs_to_device(np.array([[0, 1]]), vecs.device), margin)

	def forward(self, vecs, codes, npairs=10, pairs=None):
		"""Mean loss over min(npairs, N(N-1)/2) random ordered pairs of the N rows of vecs (N, K) / codes (N, C) (losses.py:321-333).
		pairs (not in the reference): a device int32 (P, 2) tensor of pairs already drawn -- no draw here (the captured step's static input,
		find_amd.graph).  Codes go to the kernel as fp32 (pose codes are -1 / 0 / 1: exact); the loss is fp32 (upstream's is float64,
		DESIGN 7.1)."""
		N = vecs.shape[0]
		if pairs is None:
			pairs = pairs_to_device(draw_pairs(N, npairs), vecs.device)
		return FN.contrastive_pose(vecs, torch.as_tensor(codes).to(device=vecs.device, dtype=torch.float32), pairs)


class RestylePerceptualLoss(nn.Module):
	"""The reference's RestylePerceptualLoss (losses.py:136-302) in the one mode that needs no weights of ours: mode='cluster' on rendered
	per-vertex class logits (pred_logit).  encoder: the frozen image encoder, any callable used as
	encoder(images (B, 3, H, W), return_features=True, target_feature_maps=feature_maps)['class_logits'] -> (B, C, h, w); it sees the GT
	images only, under no_grad.  Everything after its output is two HIP launches forward and one backward (functional.part_labels,
	functional.part_cross_entropy)."""

	def __init__(self, encoder):
		super().__init__()
		if not callable(encoder):
			raise TypeError('RestylePerceptualLoss(encoder): a callable image encoder is expected')
		self.encoder = encoder

	def forward(self, pred, gt, mode='feat', feature_maps=None, pred_masks=None, gt_masks=None, debug=False, debug_dir=None, pred_feat=None,
				pred_logit=None, return_encodings=False):
		"""pred, gt: renders (B, H, W, 3); pred_logit: rendered class logits (B, H, W, C) CHANNEL-LAST, as the feature render returns them
		(upstream takes the (B, C, H, W) permutation of the same tensor, model.py:1133); pred_masks (B, H, W): the predicted soft
		silhouette.  gt_masks is accepted and unused, as upstream.  Returns (loss, encodings); with return_encodings the dictionary holds
		gt_labels (B, H, W) int32, CE_loss (B, H, W) and gt_logits, the encoder's logits resampled to (H, W) -- formed with F.interpolate
		on this path only, the loss never needs it."""
		assert mode in ['feat', 'latent', 'cluster'], f"Mode `{mode}` not understood for Restyle loss."
		if mode != 'cluster':
			raise NotImplementedError(f"RestylePerceptualLoss mode='{mode}' compares encoder activations of the predicted render: it needs the "
									  "encoder's weights and a backward through it, which are out of scope; only mode='cluster' is built")
		if pred_logit is None:
			raise NotImplementedError('pred_logit=None would run the encoder on the predicted image and differentiate through it: out of scope; '
									  'render per-vertex class logits (opts.restyle_cluster_per_vertex) and pass them as pred_logit')
		if debug:
			raise NotImplementedError('debug=True writes label images through cv2 (losses.py:283-300): visualisation, out of scope')
		if feature_maps != [8]:   # (upstream's two refusals, made before the encoder runs instead of after)
			raise NotImplementedError('Classifier only works with exactly feat map 8 currently.')
		if pred_masks is None:
			raise NotImplementedError('Clustering loss requires masking')
		with torch.no_grad():
			gt_logit = self.encoder(gt.permute(0, 3, 1, 2), return_features=True, target_feature_maps=feature_maps)['class_logits']
		H, W = pred.shape[-3], pred.shape[-2]
		if tuple(pred_logit.shape[:-1]) != (gt_logit.shape[0], H, W) or pred_logit.shape[-1] != gt_logit.shape[1]:
			raise ValueError(f'RestylePerceptualLoss: pred_logit (B, H, W, C) = {tuple(pred_logit.shape)} does not match the renders '
							 f'{tuple(pred.shape)} and the encoder\'s class logits {tuple(gt_logit.shape)}')
		gt_logit = gt_logit.float()
		gt_labels = FN.part_labels(gt_logit, (H, W))
		loss, ce = FN.part_cross_entropy(pred_logit, gt_labels, pred_masks, return_ce=True)
		encodings = {}
		if return_encodings:
			encodings['gt_labels'] = gt_labels
			encodings['gt_logits'] = nn.functional.interpolate(gt_logit, size=(H, W), mode='bilinear')
			encodings['CE_loss'] = ce
		return loss, encodings


class NormalLoss(nn.Module):
	"""Weighted cosine loss between a predicted and a target normal map (not in the reference; FOUND-style fitting to surface normals): one
	HIP pass each way (functional.normal_loss)."""

	def forward(self, pred, target, weight):
		"""pred, target (..., 3), not necessarily unit; weight (...) without gradient: sum w (1 - cos) / max(sum w, 1e-12).  The gradient
		goes to pred only."""
		return FN.normal_loss(pred, target, weight)


class SurfaceDistanceLoss(nn.Module):
	"""Symmetric point-to-surface distance between predicted and GT meshes (not in the reference, whose Chamfer term measures sample to
	sample): mean over feet [ mean_i d2(g_i -> predicted mesh) + mean_j d2(s_j -> GT mesh) ], g the surface samples of the scans and s those
	of the prediction, d2 the exact squared distance to the nearest triangle (functional.point_face_distance).  The same unit as
	chamfer_distance (m^2), without its floor from the finite sample count."""

	def forward(self, pred_meshes: Meshes, gt_meshes: Meshes, num_samples=5000, gt_samples=None, pred_samples=None):
		"""gt_samples / pred_samples: (N,S,3) surface samples already drawn (the step's Chamfer samples; pred_samples must carry the sampler's
		graph for the second term to reach the predicted vertices).  The first term's gradient reaches the predicted vertices through the
		closest points, the second's through the sampler's backward."""
		if gt_samples is None:
			gt_samples = sample_points_from_meshes(gt_meshes, num_samples=num_samples)
		if pred_samples is None:
			pred_samples = sample_points_from_meshes(pred_meshes, num_samples=num_samples)
		to_pred, _, _ = point_mesh_distance(gt_samples.detach(), pred_meshes)
		to_gt, _, _ = point_mesh_distance(pred_samples, gt_meshes)
		return (to_pred.mean(1) + to_gt.mean(1)).mean()


class PenetrationLoss(nn.Module):
	"""Penalty for points inside a mesh (not in the reference): a foot's vertices against a shoe last, or against a ground slab.  The mean
	over the points of [w > level] d2, with d2 the exact squared distance to the mesh's surface (functional.point_face_distance) and w the
	point's winding number about the mesh (find_amd.inside.winding_number): points outside cost nothing, a point inside its squared depth.
	m^2, like the Chamfer term.  The gradient reaches the points and the mesh's vertices through d2; which points are inside is a constant."""

	def __init__(self, level=0.5):
		super().__init__()
		self.level = level

	def forward(self, points, meshes: Meshes, lengths=None):
		"""points (N, P, 3) against mesh n of meshes (shared or ragged faces); lengths (N): the point counts of a padded batch, whose rows at
		or past them do not count.  sum over the inside points of d2 / the number of points that count."""
		from . import inside
		verts, faces = meshes.verts_padded(), _mesh_faces(meshes)
		dist2, _, _ = FN.point_face_distance(points, verts, faces, lengths)
		w = inside.winding_number(points, verts, faces, lengths)
		n = max(points.shape[0] * points.shape[1], 1) if lengths is None else torch.as_tensor(lengths).sum().clamp(min=1).to(dist2.device)
		return torch.where(w > self.level, dist2, torch.zeros_like(dist2)).sum() / n


class ARAPLoss(nn.Module):
	"""As-rigid-as-possible deformation energy against a rest mesh (not in the reference; Sorkine & Alexa 2007): every vertex neighbourhood
	of the deformed mesh should be a rotated copy of the rest mesh's, so bending is free and stretch and shear are not.  One HIP pass each
	way (functional.arap_energy).  rest_verts (V, 3) or (1, V, 3) and faces: the rest mesh, shared by the batch; weights 'cotangent' (of the
	rest mesh, clamped at 0) or 'uniform'.  m^2, like the Chamfer term."""

	def __init__(self, rest_verts, faces, weights='cotangent'):
		super().__init__()
		self.rest = FN.ArapRest.get(rest_verts, faces, weights)

	def forward(self, verts):
		"""verts (N, V, 3): the mean over the N meshes of E_n."""
		return FN.arap_energy(verts, self.rest).mean()


class DepthLoss(nn.Module):
	"""Masked, robust loss between a predicted and a target depth map (not in the reference; fitting to a depth sensor or a structured-light
	scan): one HIP pass each way (functional.depth_loss)."""

	def __init__(self, kind='l1', delta=0.005, trunc=0.):
		"""kind 'l1' | 'l2' | 'huber' (delta: where it turns linear, metres); trunc > 0: pixels whose depths differ by more -- occlusion
		edges, where one map sees the far side -- are left out."""
		super().__init__()
		if kind not in FN.DEPTH_LOSS_KINDS:
			raise ValueError(f"DepthLoss: kind 'l1', 'l2' or 'huber', got {kind!r}")
		self.kind, self.delta, self.trunc = kind, float(delta), float(trunc)

	def forward(self, pred, target, weight=None):
		"""pred, target (n_img, ...), positive where a surface is seen; weight of the same shape or None, without gradient:
		sum w rho(pred - target) / max(sum w, 1e-12) over the pixels valid in both maps.  The gradient goes to pred only."""
		return FN.depth_loss(pred, target, weight, kind=self.kind, delta=self.delta, trunc=self.trunc)


class SSIMLoss(nn.Module):
	"""1 - SSIM of two image batches (not in the reference, whose pixel loss is a mean squared error; the structural term of
	differentiable-rendering losses): one HIP pass each way (find_amd.ssim.ssim)."""

	def __init__(self, data_range=1.0, border='same'):
		"""data_range: the span of the values (C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2); border 'same' (zero padding, every
		pixel counts and gets a gradient) | 'valid' (only windows inside the image count)."""
		super().__init__()
		if border not in _ssim.BORDERS:
			raise ValueError(f"SSIMLoss: border 'same' or 'valid', got {border!r}")
		if not data_range > 0:
			raise ValueError(f'SSIMLoss: data_range > 0 expected, got {data_range}')
		self.data_range, self.border = float(data_range), border

	def forward(self, pred, target, pred_mask=None, target_mask=None):
		"""pred, target (..., H, W, C), C <= 4; masks (..., H, W) or None, multiplied in.  The gradient goes to pred and pred_mask only."""
		return 1. - _ssim.ssim(pred, target, pred_mask, target_mask, data_range=self.data_range, border=self.border)


class MeasurementLoss(nn.Module):
	"""Squared difference between a mesh's foot measurements (find_amd.measure.foot_measurements: length, width, girths) and given numbers
	-- a tape's, where there is no scan (not in the reference).  The mean over feet and measurements, m^2; relative: of the difference
	divided by the target, dimensionless.  The user composes it on model.get_meshes(...)['verts'] to refine latents with the existing
	optimisers; it is no term of ModelWithLoss."""

	def __init__(self, spec=None, relative=False):
		super().__init__()
		self.spec = _measure.FootSpec() if spec is None else spec
		if not isinstance(self.spec, _measure.FootSpec):
			raise ValueError(f'MeasurementLoss: spec must be a FootSpec, got {type(spec).__name__}')
		self.relative = bool(relative)

	def forward(self, verts, faces, target, v_len=None):
		"""verts (N, V, 3), faces (F, 3) or (N, F, 3); target (N, M) in metres, columns as spec.names; a NaN entry is "not measured" and is
		left out: the mean runs over the entries that count (0 when none does).  The gradient goes to the vertices."""
		M = len(self.spec.names)
		if target.dim() != 2 or target.shape != (verts.shape[0], M):
			raise ValueError(f'MeasurementLoss: target ({verts.shape[0]}, {M}) for {self.spec.names} expected, got {tuple(target.shape)}')
		values, _ = _measure.foot_measurements(verts, faces, self.spec, v_len)
		target = target.to(values.device, values.dtype)
		known = ~torch.isnan(target)
		diff = torch.where(known, values - torch.where(known, target, values.detach()), torch.zeros_like(values))
		if self.relative:
			diff = diff / torch.where(known, target, torch.ones_like(target))
		return (diff * diff).sum() / known.sum().clamp(min=1)
