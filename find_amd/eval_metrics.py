"""Metric definitions of reference src/eval/eval_3d.py on the HIP path (row a16): keypoint error in mm (eval_3d.py:142,
220-221), Chamfer over 10 000 surface samples reported x1e6 as "um" (eval_3d.py:148-151, 223 -- the reference's
scaling of a m^2 quantity is kept) and the per-foot z <= 0.07 cut-off variant (eval_3d.py:154-161).
Spins, heat maps and OBJ export of the eval script: find_amd.vis / find_amd.evaluate.eval_3d; its tables and plots are out of scope.

The 2-D half: MSE, PSNR, MSE_masked, PSNR_masked and IOU under the names and semantics of reference src/eval/eval_metrics.py (so that
`from find_amd.eval_metrics import IOU, MSE, PSNR, MSE_masked, PSNR_masked` replaces that import), and eval_2d_metrics, the per-group
metrics of eval_2d.py:86-121.  All of them are formed from the per-image sums of ONE pass over the images (FN.image_metric_sums), composed
in float64 on the device; the scalar functions return float32 0-d tensors like their torch originals (MSE 0 -> PSNR inf, a union or mask
sum of 0 -> nan)."""
import torch

from . import align as _align
from . import functional as FN
from . import inside as _inside
from . import measure as _measure
from . import ssim as _ssim
from .losses import _mesh_faces, point_mesh_distance, sample_points_from_meshes

# template vertex ids of the six keypoints on the PCA foot model's mesh (reference src/cfg.yaml:11, read by eval_3d.py:137-138 and
# eval_2d.py:155-156): eval_3d_metrics(..., template_kp_idxs=PCA_KEYPOINTS) for a PCAModel fitted to Foot3D scans
PCA_KEYPOINTS = (1308, 1270, 1271, 1113, 1033, 489)


def keypoint_error_mm(pred_verts, template_kp_idxs, gt_kps):
	"""pred_verts (N,V,3) registered predictions, template_kp_idxs (K) vertex ids, gt_kps (N,K,3) -> scalar mm."""
	idx = torch.as_tensor(template_kp_idxs, device=pred_verts.device, dtype=torch.long)
	dists = torch.norm(pred_verts[:, idx] - gt_kps, dim=-1)
	return dists.mean() * 1e3


def _foot_spec(measurements, who):
	"""measurements: True (the default FootSpec) or a FootSpec."""
	if measurements is True:
		return _measure.FootSpec()
	if not isinstance(measurements, _measure.FootSpec):
		raise ValueError(f'find_amd.{who}: measurements must be True or a FootSpec (the spec of what to measure), got {measurements!r}')
	return measurements


def measurement_names(spec):
	"""The table's keys of a FootSpec: 'Length (mm)', 'Width (mm)', 'Ball girth (mm)', ..."""
	return tuple(n.replace('_', ' ').capitalize() + ' (mm)' for n in spec.names)


def measurement_errors_mm(pred_meshes, gt_meshes, spec=None, return_per_foot=False):
	"""Foot measurements of predictions against those of the scans (not in the reference; find_amd.measure.of_meshes on both):
	{'Length (mm)', 'Width (mm)', 'Ball girth (mm)', 'Instep girth (mm)'} with the default FootSpec, each the mean over feet of
	|pred - scan| x 1e3.  return_per_foot: also the two (N, M) tables in mm, the predictions' and the scans'.  No gradient."""
	spec = _measure.FootSpec() if spec is None else _foot_spec(spec, 'eval_metrics.measurement_errors_mm')
	with torch.no_grad():
		pred = _measure.of_meshes(pred_meshes, spec)[0] * 1e3
		gt = _measure.of_meshes(gt_meshes, spec)[0] * 1e3
		out = dict(zip(measurement_names(spec), (pred - gt).abs().mean(0)))
	return (out, pred, gt) if return_per_foot else out


def _mesh_boxes(meshes):
	"""(lo (N, 3), hi (N, 3)) over each mesh's own vertices (the rows that pad a ragged batch do not count)."""
	v = meshes.verts_padded()
	own = (torch.arange(v.shape[1], device=v.device)[None] < meshes.num_verts_per_mesh().to(v.device)[:, None])[..., None]
	inf = torch.full_like(v, float('inf'))
	return torch.where(own, v, inf).amin(1), torch.where(own, v, -inf).amax(1)


def eval_3d_metrics(pred_meshes, gt_meshes, pred_verts=None, template_kp_idxs=None, gt_kps=None, samples=10000, z_cutoff=0.07,
					draws_gt=None, draws_pred=None, return_samples=False, surface=False, return_per_foot=False, align=None, volume=None, measurements=None):
	"""Returns {'Keypoint (mm)', 'Chamf z-cutoff <z> (um)', 'Chamf (um)'} as 0-d tensors (keypoints only when given); with return_samples
	also (gt_pts, pred_pts), the (N,samples,3) surface samples the Chamfer terms were taken on (the per-vertex heat maps of eval_3d.py:171-178
	read the predicted ones: no second draw).
	surface (not in the reference): three more keys, distances to the other SURFACE (losses.point_mesh_distance) instead of to its samples --
	'Scan→pred (mm)': the mean over feet of the mean unsquared distance of every scan vertex to the predicted surface, x 1e3; 'Pred→scan (mm)':
	the same for the predicted vertices against the scan's surface; 'Surf (μm)': the symmetric mean squared distance of the very samples
	'Chamf (μm)' used, x 1e6.  return_per_foot (with surface): a last value {'Scan→pred (mm)', 'Pred→scan (mm)'} of (N) tensors, a number per
	foot.
	measurements (not in the reference; True or a measure.FootSpec): the keys of measurement_errors_mm join the result, and with
	return_per_foot the last value also holds 'measure_pred_mm' and 'measure_gt_mm', the (N, M) tables.  No random number is drawn for them.
	align (not in the reference; None, 'rigid' or 'similarity'): errors after alignment, for a prediction that is right up to a rigid motion
	(or a similarity).  The prediction is moved onto the scan by find_amd.align.iterative_closest_point from the very predicted samples to
	the very scan samples the Chamfer term drew -- no further random number is drawn -- and 'Chamf aligned (μm)' is the Chamfer term of the
	moved samples; with keypoints 'Keypoint aligned (mm)' is the keypoint error of the predicted keypoints under the same transform.  With
	return_per_foot the last value also holds 'align_R' (N, 3, 3), 'align_T' (N, 3), 'align_s' (N) and 'align_rmse' (N).  None changes nothing.
	volume (not in the reference; None or a grid resolution): find_amd.inside.volume_iou of every prediction with its scan on one volume^3 grid
	over the two (5 mm of margin): 'Vol IoU (%)', the mean over feet of the volumetric IoU x 100, and 'Volume err (ml)', the mean of
	|V_pred - V_scan| x 1e6 of the two grid volumes (winding number > 0.5 at the cell centres, so a scan open at the ankle is closed about flat).
	With return_per_foot the last value also holds 'vol_iou', 'volume_pred_ml' and 'volume_gt_ml' (N).  No random number is drawn for them;
	None changes nothing."""
	if volume is not None and (not isinstance(volume, int) or isinstance(volume, bool) or volume < 1):
		raise ValueError(f'find_amd.eval_metrics.eval_3d_metrics: volume must be None or a grid resolution (an int >= 1), got {volume!r}')
	if align not in (None, 'rigid', 'similarity'):
		raise ValueError(f"find_amd.eval_metrics.eval_3d_metrics: align must be None, 'rigid' or 'similarity', got {align!r}")
	spec = None if measurements is None or measurements is False else _foot_spec(measurements, 'eval_metrics.eval_3d_metrics')
	with torch.no_grad():
		gt_pts = sample_points_from_meshes(gt_meshes, num_samples=samples, draws=draws_gt)
		pred_pts = sample_points_from_meshes(pred_meshes, num_samples=samples, draws=draws_pred)
		chamf, _ = FN.chamfer_distance(gt_pts, pred_pts)
		# per-foot cut-off clouds, each its own batch of one, then the mean over feet (eval_3d.py:154-161)
		keep_p, keep_g = pred_pts[..., 2] <= z_cutoff, gt_pts[..., 2] <= z_cutoff
		order_p = torch.argsort((~keep_p).to(torch.int8), dim=1, stable=True)
		order_g = torch.argsort((~keep_g).to(torch.int8), dim=1, stable=True)
		pp = torch.gather(pred_pts, 1, order_p.unsqueeze(-1).expand(-1, -1, 3))
		gp = torch.gather(gt_pts, 1, order_g.unsqueeze(-1).expand(-1, -1, 3))
		pl, gl = keep_p.sum(1).to(torch.int32), keep_g.sum(1).to(torch.int32)
		# batch-mean of per-cloud (mean_x + mean_y) == mean over feet of single-cloud Chamfer distances
		chamf_cut, _ = FN.chamfer_distance(gp, pp, gl, pl)
		out = {f'Chamf z-cutoff {z_cutoff} (μm)': chamf_cut * 1e6, 'Chamf (μm)': chamf * 1e6}
		if template_kp_idxs is not None:
			out['Keypoint (mm)'] = keypoint_error_mm(pred_verts, template_kp_idxs, gt_kps)
		per_foot = {}
		if surface:
			n_gt = gt_meshes.num_verts_per_mesh().to(torch.int32)
			n_pred = pred_meshes.num_verts_per_mesh().to(torch.int32)
			to_pred, _, _ = point_mesh_distance(gt_meshes.verts_padded(), pred_meshes, n_gt)      # (padded rows: 0)
			to_gt, _, _ = point_mesh_distance(pred_meshes.verts_padded(), gt_meshes, n_pred)
			per_foot['Scan→pred (mm)'] = to_pred.sqrt().sum(1) / n_gt.clamp(min=1) * 1e3
			per_foot['Pred→scan (mm)'] = to_gt.sqrt().sum(1) / n_pred.clamp(min=1) * 1e3
			out.update({k: v.mean() for k, v in per_foot.items()})
			s_pred, _, _ = point_mesh_distance(gt_pts, pred_meshes)
			s_gt, _, _ = point_mesh_distance(pred_pts, gt_meshes)
			out['Surf (μm)'] = (s_pred.mean(1) + s_gt.mean(1)).mean() * 1e6
		if spec is not None:
			errs, per_foot['measure_pred_mm'], per_foot['measure_gt_mm'] = measurement_errors_mm(pred_meshes, gt_meshes, spec, return_per_foot=True)
			out.update(errs)
		if volume is not None:
			lo_p, hi_p = _mesh_boxes(pred_meshes)
			lo_g, hi_g = _mesh_boxes(gt_meshes)
			iou, vol_p, vol_g = _inside.volume_iou(pred_meshes.verts_padded(), _mesh_faces(pred_meshes), gt_meshes.verts_padded(), _mesh_faces(gt_meshes), res=volume,
												   bounds=(torch.minimum(lo_p, lo_g) - 0.005, torch.maximum(hi_p, hi_g) + 0.005))
			per_foot.update(vol_iou=iou, volume_pred_ml=vol_p * 1e6, volume_gt_ml=vol_g * 1e6)
			out['Vol IoU (%)'] = iou.mean() * 100
			out['Volume err (ml)'] = (vol_p - vol_g).abs().mean() * 1e6
		if align is not None:
			sol = _align.iterative_closest_point(pred_pts, gt_pts, estimate_scale=align == 'similarity')
			out['Chamf aligned (μm)'] = FN.chamfer_distance(gt_pts, sol.Xt)[0] * 1e6
			if template_kp_idxs is not None:
				kp = torch.as_tensor(template_kp_idxs, device=pred_verts.device, dtype=torch.long)
				out['Keypoint aligned (mm)'] = torch.norm(sol.RTs.apply(pred_verts[:, kp]) - gt_kps, dim=-1).mean() * 1e3
			per_foot.update(align_R=sol.RTs.R, align_T=sol.RTs.T, align_s=sol.RTs.s, align_rmse=sol.rmse)
	ret = (out,) + (((gt_pts, pred_pts),) if return_samples else ()) + ((per_foot,) if (surface or spec is not None or align is not None or volume is not None) and return_per_foot else ())
	return ret if len(ret) > 1 else out


# ---------------------------------------------------------------------------------------------- 2-D (eval_2d.py, eval_metrics.py)
SQ, SQ_EACH, SQ_COMMON, INTER, UNION, WSQ, W = range(7)   # columns of FN.image_metric_sums


def _f32(t):
	return t if t.dtype == torch.float32 else t.float()


def _same_shape(what, p1, p2):
	if p1.shape != p2.shape:
		raise ValueError(f'find_amd.eval_metrics.{what}: shapes differ: {tuple(p1.shape)} / {tuple(p2.shape)}')


def _psnr(mse):
	return -10 * torch.log10(mse)


def MSE(p1, p2):
	"""nn.functional.mse_loss(p1, p2): mean of the squared differences over every element."""
	_same_shape('MSE', p1, p2)
	s = FN.image_metric_sums(p2.reshape(1, -1, 1), p1.reshape(1, -1, 1))
	return (s[0, SQ] / p1.numel()).float()


def PSNR(p1, p2):
	"""-10 log10(MSE(p1, p2))."""
	_same_shape('PSNR', p1, p2)
	s = FN.image_metric_sums(p2.reshape(1, -1, 1), p1.reshape(1, -1, 1))
	return _psnr(s[0, SQ] / p1.numel()).float()


def _mse_masked64(p1, p2, mask):
	_same_shape('MSE_masked', p1, p2)
	if mask.shape == p1.shape[:-1]:   # a weight per pixel, counted once per channel
		C = p1.shape[-1]
		s = FN.image_metric_sums(p2.reshape(1, -1, C), p1.reshape(1, -1, C), weight=_f32(mask).reshape(1, -1))
		return s[0, WSQ] / (C * s[0, W])
	w = mask.expand_as(p1)            # any other shape broadcasts to the values (expand_as raises where the reference does)
	s = FN.image_metric_sums(p2.reshape(1, -1, 1), p1.reshape(1, -1, 1), weight=_f32(w).reshape(1, -1))
	return s[0, WSQ] / s[0, W]


def MSE_masked(p1, p2, mask):
	"""sum(mask * (p1 - p2)^2) / sum(mask expanded to p1): mask of p1.shape[:-1] (one value per pixel, C channels) or of p1's shape."""
	return _mse_masked64(p1, p2, mask).float()


def PSNR_masked(p1, p2, mask):
	return _psnr(_mse_masked64(p1, p2, mask)).float()


def IOU(s1, s2, reduce='mean'):
	"""sum(s1 * s2) / sum(max(s1, s2)) per [H, W] slice (leading dimensions are batch dimensions), then the mean over the slices."""
	if reduce != 'mean':
		raise NotImplementedError(f'Reduction method `{reduce}` for IOU not implemented.')
	_same_shape('IOU', s1, s2)
	if s1.dim() < 2:
		raise ValueError(f'find_amd.eval_metrics.IOU: masks are [(batch) x H x W], got {tuple(s1.shape)}')
	n_pix = s1.shape[-2] * s1.shape[-1]
	a, b = _f32(s1).reshape(-1, n_pix), _f32(s2).reshape(-1, n_pix)
	s = FN.image_metric_sums(b.unsqueeze(-1), a.unsqueeze(-1), pred_mask=b, gt_mask=a)
	return (s[:, INTER] / s[:, UNION]).mean().float()


def eval_2d_metrics(pred_rdrs, gt_rdrs, batch_size=None):
	"""The metrics of eval_2d.py:86-121 for renders of N feet x M views (FootRenderer output dicts; gt_rdrs rendered with return_mask,
	mask_out_faces and return_mask_out_masks, pred_rdrs with return_mask).  A group is `batch_size` consecutive views of one foot (default:
	all M), as one pass of the reference's inner loop.  Returns {'MSE', 'PSNR_A', 'PSNR_B', 'PSNR_C', 'IOU'}: float64 tensors of
	N * (M // batch_size) values, foot-major.  MSE and the PSNRs are taken over the whole group, IOU is the mean of its per-image IoUs.
	The prediction is read as if 1 / 0 had been written into its image / mask under the GT's mask-out map (eval_2d.py:92-94); the dicts
	are left as they are."""
	gi, pi, gm, pm = gt_rdrs['image'], pred_rdrs['image'], gt_rdrs['mask'], pred_rdrs['mask']
	if gi.dim() != 5 or pi.shape != gi.shape:
		raise ValueError(f'find_amd.eval_2d_metrics: images must be (feet, views, H, W, C) of one shape, got {tuple(pi.shape)} / {tuple(gi.shape)}')
	N, M, H, Wd, C = gi.shape
	bs = M if batch_size is None else int(batch_size)
	if bs < 1 or M % bs:
		raise ValueError(f'find_amd.eval_2d_metrics: {M} views do not split into groups of {bs}')
	hide = None if gt_rdrs.get('nothing_hidden', False) else gt_rdrs.get('mask_out_masks')
	n_img, n_pix = N * M, H * Wd
	s = FN.image_metric_sums(pi.reshape(n_img, n_pix, C), gi.reshape(n_img, n_pix, C), pred_mask=pm.reshape(n_img, n_pix),
							 gt_mask=gm.reshape(n_img, n_pix), hide=None if hide is None else hide.reshape(n_img, n_pix))
	per = s.view(n_img // bs, bs, 7)
	S = per.sum(1)
	n = bs * n_pix * C
	mse = S[:, SQ] / n
	return {'MSE': mse, 'PSNR_A': _psnr(mse), 'PSNR_B': _psnr(S[:, SQ_EACH] / n), 'PSNR_C': _psnr(S[:, SQ_COMMON] / n),
			'IOU': (per[..., INTER] / per[..., UNION]).mean(1)}


def depth_error_mm(pred_rdrs, gt_rdrs, return_coverage=False):
	"""Mean absolute depth error per image, millimetres (not in the reference): renders of N feet x M views with return_depth (FootRenderer
	output dicts; gt_rdrs may carry mask_out_masks, whose pixels do not count).  1000 * sum w |pred - gt| / sum w over the pixels where both
	maps see a surface -- the per-image sums of functional.depth_loss (kind 'l1', no truncation), float64, N * M values, foot-major; NaN
	where the two maps share no pixel.  return_coverage: also the share of the GT's own pixels that the prediction covers, per image (NaN
	where the GT sees nothing): a prediction that misses the scan scores no depth error there, and this says how much that is."""
	pd, gd = pred_rdrs['depth'], gt_rdrs['depth']
	if gd.dim() != 4 or pd.shape != gd.shape:
		raise ValueError(f'find_amd.depth_error_mm: depth maps must be (feet, views, H, W) of one shape, got {tuple(pd.shape)} / {tuple(gd.shape)}')
	N, M, H, Wd = gd.shape
	hide = None if gt_rdrs.get('nothing_hidden', False) else gt_rdrs.get('mask_out_masks')
	weight = None if hide is None else (~hide).float().reshape(N * M, H * Wd)
	with torch.no_grad():
		_, per = FN.depth_loss(_f32(pd).detach().reshape(N * M, H * Wd), _f32(gd).detach().reshape(N * M, H * Wd), weight, kind='l1', trunc=0.,
							   return_per_image=True)
		nan = torch.full_like(per[:, 0], float('nan'))
		err = torch.where(per[:, 1] > 0, 1000. * per[:, 0] / per[:, 1].clamp(min=1e-300), nan)
		if not return_coverage:
			return err
		seen = (gd > 0).reshape(N * M, H * Wd)
		n_gt = (seen if weight is None else seen & (weight > 0)).sum(1).double()
		return err, torch.where(n_gt > 0, per[:, 1] / n_gt.clamp(min=1), nan)


def SSIM(gt, pred, gt_mask=None, pred_mask=None, border='valid'):
	"""Structural similarity per image (not in the reference; find_amd.ssim.ssim, data_range 1): gt, pred (..., H, W, C) in [0, 1], C <= 4,
	masks (..., H, W) or None, multiplied in.  Returns the float64 values of the images, leading dimensions folded; border 'valid' is
	pytorch-msssim's convention (only windows inside the image count), 'same' that of 3DGS.  No gradient."""
	_same_shape('SSIM', gt, pred)
	with torch.no_grad():
		_, per = _ssim.ssim(_f32(pred).detach(), _f32(gt).detach(), None if pred_mask is None else _f32(pred_mask).detach(),
							None if gt_mask is None else _f32(gt_mask).detach(), data_range=1.0, border=border, return_per_image=True)
	return per
