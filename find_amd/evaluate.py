"""The metric loop of reference src/eval/eval_2d.py (main, eval_2d.py:50-121) on the HIP path: every validation foot and its prediction
rendered from the same views, PSNR_A / _B / _C, MSE and IOU per group of views (eval_metrics.eval_2d_metrics), the mean over all groups of
all feet.  The HD three-view render, the PNG writes, the results table and the experiment-directory walk (run_on_exp) are visualisation
and out of scope.

eval_3d is the loop of reference src/eval/eval_3d.py (main, eval_3d.py:56-225) the same way: keypoint error, Chamfer and its z cut-off
variant (eval_metrics.eval_3d_metrics) over every validation foot, and optionally the per-foot keypoint table behind errors.png and the
top-down keypoint renders of render_correspondences (eval_3d.py:94-99); with produce_spins / export_meshes the six turntable spins per
foot with their per-vertex Chamfer heat maps (eval_3d.py:163-201) and the OBJ files (eval_3d.py:204-217), through find_amd.vis.  The PNG
writes and the matplotlib table are out of scope."""
import os

import torch
from torch.utils.data import DataLoader

from .dataset import BatchCollator
from .eval_metrics import SSIM, _foot_spec, depth_error_mm, eval_2d_metrics, eval_3d_metrics, measurement_names
from .renderer import FootRenderer
from .structures import Meshes, TexturesVertex

METRICS = ('MSE', 'PSNR_A', 'PSNR_B', 'PSNR_C', 'IOU')


def _marked_faces(textures):
	"""Faces a scan's TexturesUV marks to hide: a final UV vertex at (0, 0) that all three UV corners of the face use (the renderer's
	convention, reference renderer.py:340-349), read from the scan's own tables.  (Collated into one ragged batch, the tables are padded
	with (0, 0) rows, and the renderer's search over the padded batch would then find another answer than for the scan alone.)"""
	vu, fu = textures.verts_uvs_padded()[0], textures.faces_uvs_padded()[0]
	if not bool((vu[-1] == 0).all()):
		return torch.zeros(0, dtype=torch.int64)
	return torch.argwhere(torch.all(fu == vu.shape[0] - 1, dim=-1)).flatten()


def eval_2d(model, dataset, image_size=128, nviews=1, batch_size=1, R=None, T=None, feet_per_call=16, return_per_image=False, device='cuda', depth=False,
			ssim=False):
	"""model: a NeuralDisplacementField, a PCAModel or a SkinnedModel -- any model with latent_vectors_val and get_meshes_from_batch -- whose
	validation latent tables are indexed by the dataset's item index (batch['idx'], as eval_2d.py:28-35 samples them); dataset: the
	validation Foot3DDataset.  Views: linspace_views(nviews, dist=0.3, elev_min=-90,
	elev_max=90) unless R, T are given; groups of `batch_size` consecutive views (nviews // batch_size of them per foot, the loop bound of
	eval_2d.py:86).  Feet are rendered `feet_per_call` at a time; the metrics are per image sums composed in float64, so the result does
	not depend on that choice.  Returns {'MSE', 'PSNR_A', 'PSNR_B', 'PSNR_C', 'IOU'} as floats, and with return_per_image also the
	per-group float64 tensors (foot-major, nviews // batch_size groups per foot) as a second dict.
	depth (not in the reference): two more columns from eval_metrics.depth_error_mm -- 'Depth (mm)', the mean absolute difference of the two
	rendered depth maps where both see a surface, and 'Depth coverage', the share of the scan's pixels the prediction covers -- as means over
	the images that have a value; the per-image tensors (one value per foot and view, NaN where there is none) join the second dict.
	ssim (not in the reference): two more columns from eval_metrics.SSIM (border 'valid') -- 'SSIM_A' on the images PSNR_A compares (the
	prediction whitened under the GT's mask-out map, eval_2d.py:92-94) and 'SSIM_B' on those of PSNR_B (each image times its own mask > 0) --
	per group the mean over its images, like IOU."""
	renderer = FootRenderer(image_size=image_size, device=device)
	if R is None:
		R, T = renderer.linspace_views(nviews=nviews, dist=0.3, elev_min=-90, elev_max=90)
	n_used = (R.shape[0] // batch_size) * batch_size
	if n_used == 0:
		raise ValueError(f'find_amd.evaluate.eval_2d: {R.shape[0]} views make no group of {batch_size}')
	R, T = R[:n_used].to(device), T[:n_used].to(device)
	collate = BatchCollator(device=device).collate_batches
	loader = DataLoader(dataset, batch_size=feet_per_call, shuffle=False, collate_fn=lambda items: (collate(items), [_marked_faces(it['textures']) for it in items]))
	per = {k: [] for k in METRICS + (('Depth (mm)', 'Depth coverage') if depth else ()) + (('SSIM_A', 'SSIM_B') if ssim else ())}
	more = dict(return_depth=True) if depth else {}
	was_training = model.training
	model.eval()
	try:
		with torch.no_grad():
			for batch, marked in loader:
				idx = batch['idx'].to(device)
				batch.update({vec.name: vec[idx] for vec in model.latent_vectors_val})
				res = model.get_meshes_from_batch(batch, is_train=False)
				gt_rdrs = renderer(batch['mesh'], R, T, return_mask=True, mask_out_faces=True, masked_faces=marked, return_mask_out_masks=True, **more)
				pred_rdrs = renderer(res['meshes'], R, T, return_mask=True, **more)
				for k, v in eval_2d_metrics(pred_rdrs, gt_rdrs, batch_size).items():
					per[k].append(v)
				if depth:
					err, cover = depth_error_mm(pred_rdrs, gt_rdrs, return_coverage=True)
					per['Depth (mm)'].append(err)
					per['Depth coverage'].append(cover)
				if ssim:
					for k, v in _ssim_columns(pred_rdrs, gt_rdrs, batch_size).items():
						per[k].append(v)
	finally:
		model.train(was_training)
	per = {k: torch.cat(v) for k, v in per.items()}
	out = {k: float(v.nanmean() if k.startswith('Depth') else v.mean()) for k, v in per.items()}
	return (out, per) if return_per_image else out


def _ssim_columns(pred_rdrs, gt_rdrs, batch_size):
	"""'SSIM_A' / 'SSIM_B' of renders of N feet x M views: float64, N * (M // batch_size) values, foot-major, a group's value the mean over
	its images.  The images are those of eval_metrics.eval_2d_metrics' PSNR_A / PSNR_B, formed here (evaluation code, not a hot path)."""
	gi, pi, gm, pm = gt_rdrs['image'], pred_rdrs['image'], gt_rdrs['mask'], pred_rdrs['mask']
	hide = None if gt_rdrs.get('nothing_hidden', False) else gt_rdrs.get('mask_out_masks')
	if hide is not None:
		pi = torch.where(hide[..., None], torch.ones_like(pi), pi)
		pm = torch.where(hide, torch.zeros_like(pm), pm)
	a = SSIM(gi, pi)
	b = SSIM(gi, pi, gt_mask=(gm > 0).float(), pred_mask=(pm > 0).float())
	return {'SSIM_A': a.view(-1, batch_size).mean(1), 'SSIM_B': b.view(-1, batch_size).mean(1)}


def eval_3d(model, dataset, template_kp_idxs, samples=10000, z_cutoff=0.07, feet_per_call=16, render_correspondences=False, image_size=256,
			return_per_foot=False, device='cuda', produce_spins=False, export_meshes=False, out_dir=None, spin_frames=250, spin_image_size=512,
			spin_format='gif', surface=False, template_uvs=None, texture_size=1024, texture_pad=4, align=None, volume=None, measurements=False):
	"""model: a NeuralDisplacementField, a PCAModel or a SkinnedModel -- any model with latent_vectors_val and get_meshes_from_batch -- whose
	validation latent tables are indexed by the dataset's item index (batch['idx']);
	dataset: the validation Foot3DDataset, every foot with keypoints; template_kp_idxs: the template vertices of the keypoints (the
	template foot's kp_idxs for a neural model, eval_metrics.PCA_KEYPOINTS for a PCAModel, the caller's own ids for a SkinnedModel;
	eval_3d.py:132-138).  Ground-truth keypoints
	are the scan's vertices at its kp_idxs, predicted ones the prediction's vertices at template_kp_idxs.  Predictions are made
	`feet_per_call` at a time; the metrics are taken once over all feet, as eval_3d.py:146-161 does, so the keypoint table does not depend
	on that choice and the Chamfer terms draw their samples as one eval_3d_metrics call over all feet would.
	Returns {'Keypoint (mm)', 'Chamf z-cutoff <z> (μm)', 'Chamf (μm)'} as floats; with return_per_foot or render_correspondences a second
	dict follows, holding 'keypoint_mm' (N,K) float32 (the data of errors.png) and / or 'gt' and 'pred', the keypoint_blend images
	(N,1,H,W,3) from view_from('topdown').  A foot without keypoints raises ValueError (upstream reads vertex 0 for it).
	export_meshes writes {out_dir}/meshes/{n:02d}_gt_mesh.obj and {n:02d}_pred_mesh.obj (vis.export_obj: the prediction with its vertex
	colours, the scan's geometry).  produce_spins writes, per foot n, {out_dir}/spins/{n:02d}_{pred_rgb, pred_chamf, pred_grey, gt_rgb, gt_chamf,
	gt_grey}.<spin_format>: vis.turntable(azim=70, dist=0.35) of spin_frames frames at spin_image_size, in the mesh's own texture, as the
	per-vertex heat map vis.error_colours(vis.vertex_errors(...)) -- the GT one against the very predicted samples the Chamfer number was
	taken on -- and in grey (TexturesVertex(0.5)); each spin is written as it is made.  spin_format: an extension vis.turntable writes
	('gif', 'png', 'webp', 'npy'; 'mp4' with imageio -- upstream's format).  Either adds to the second dict 'files', the paths written, and
	produce_spins also 'pred_vertex_error' (N,V) and 'gt_vertex_error', a list of (Vg,) tensors (squared distances).  The metrics do not
	depend on these keywords: no random number is drawn for them.
	surface (not in the reference): eval_metrics.eval_3d_metrics(surface=True) -- 'Scan→pred (mm)', 'Pred→scan (mm)' and 'Surf (μm)' join the
	returned metrics, with return_per_foot the second dict also holds 'scan_to_pred_mm' and 'pred_to_scan_mm' (N), and the heat maps of
	produce_spins are coloured from vis.surface_errors (distances to the other surface) instead of vis.vertex_errors.
	template_uvs (not in the reference): (verts_uvs (Vt,2), faces_uvs (F,3)), a UV atlas of the template's faces.  With export_meshes every
	predicted foot is then also written as {n:02d}_pred_textured.obj / .mtl / .png beside the vertex-coloured one: the colour field baked
	into a texture_size map with a gutter of texture_pad texels (find_amd.bake; a NeuralDisplacementField only).  None: nothing changes.
	measurements (not in the reference; True or a find_amd.measure.FootSpec): eval_metrics.eval_3d_metrics(measurements=...) -- 'Length (mm)',
	'Width (mm)', 'Ball girth (mm)' and 'Instep girth (mm)' (the spec's names) join the returned metrics, each the mean over feet of
	|prediction - scan|; with return_per_foot the second dict also holds 'measure_pred_mm' and 'measure_gt_mm' (N, M).  False: nothing changes.
	align (not in the reference; None, 'rigid' or 'similarity'): eval_metrics.eval_3d_metrics(align=...) -- 'Chamf aligned (μm)' and 'Keypoint
	aligned (mm)', the errors after the prediction has been moved onto the scan by ICP on the Chamfer term's own samples, join the returned
	metrics; with return_per_foot the second dict also holds 'align_R', 'align_T', 'align_s' and 'align_rmse'.  None: nothing changes.
	volume (not in the reference; None or a grid resolution): eval_metrics.eval_3d_metrics(volume=...) -- 'Vol IoU (%)' and 'Volume err (ml)',
	the volumetric IoU and the volume difference of prediction and scan on a volume^3 grid (find_amd.inside), join the returned metrics; with
	return_per_foot the second dict also holds 'vol_iou', 'volume_pred_ml' and 'volume_gt_ml' (N).  None: nothing changes."""
	if align not in (None, 'rigid', 'similarity'):
		raise ValueError(f"find_amd.evaluate.eval_3d: align must be None, 'rigid' or 'similarity', got {align!r}")
	spec = _foot_spec(measurements, 'evaluate.eval_3d') if measurements is not False and measurements is not None else None
	if (produce_spins or export_meshes) and out_dir is None:
		raise ValueError('find_amd.evaluate.eval_3d: produce_spins / export_meshes need out_dir')
	keep_meshes = produce_spins or export_meshes
	gt_meshes, pred_meshes, tex_meshes = [], [], []
	bake_plan = None
	if template_uvs is not None and export_meshes:
		from . import bake
		uvs = (template_uvs[0].to(device), template_uvs[1].to(device))
		bake_plan = bake.plan(uvs[0], uvs[1], texture_size, pad=texture_pad)
	collate = BatchCollator(device=device).collate_batches
	loader = DataLoader(dataset, batch_size=feet_per_call, shuffle=False, collate_fn=collate)
	kp_t = torch.as_tensor(template_kp_idxs, dtype=torch.long, device=device)
	renderer = FootRenderer(image_size=image_size, device=device) if render_correspondences else None
	R, T = renderer.view_from('topdown') if render_correspondences else (None, None)
	gt_v, gt_f, pred_v, pred_f, gt_kps, pred_verts, images = [], [], [], [], [], [], {'gt': [], 'pred': []}
	was_training = model.training
	model.eval()
	try:
		with torch.no_grad():
			for batch in loader:
				has = [bool(h) for h in batch['has_keypoints']]
				if not all(has):
					raise ValueError(f'find_amd.evaluate.eval_3d: foot {batch["name"][has.index(False)]} has no keypoints')
				idx = batch['idx'].to(device)
				batch.update({vec.name: vec[idx] for vec in model.latent_vectors_val})
				res = model.get_meshes_from_batch(batch, is_train=False)
				gt = batch['mesh']
				kp_idxs = torch.as_tensor(batch['kp_idxs'], device=device).long()
				gkp = torch.stack([v[k] for v, k in zip(gt.verts_list(), kp_idxs)])
				pkp = res['verts'][:, kp_t]
				gt_v += gt.verts_list(); gt_f += gt.faces_list()
				pred_v += res['meshes'].verts_list(); pred_f += res['meshes'].faces_list()
				gt_kps.append(gkp)
				pred_verts.append(res['verts'])
				if keep_meshes:
					gt_meshes += [gt[i] for i in range(len(gt))]
					pred_meshes += [res['meshes'][i] for i in range(len(gt))]
				if bake_plan is not None:
					textured = bake.textured_meshes(model, bake_plan, uvs[0], uvs[1], batch, is_train=False)
					tex_meshes += [textured[i] for i in range(len(gt))]
				if render_correspondences:
					images['gt'].append(renderer(gt, R, T, return_images=True, keypoints=gkp, keypoints_blend=True)['keypoints_blend'])
					images['pred'].append(renderer(res['meshes'], R, T, return_images=True, keypoints=pkp, keypoints_blend=True)['keypoints_blend'])
			gt_kps = torch.cat(gt_kps)
			pred_verts = torch.cat(pred_verts)
			gt_all = Meshes(gt_v, gt_f)
			pred_all = Meshes(pred_v, pred_f)
			got = eval_3d_metrics(pred_all, gt_all, pred_verts=pred_verts, template_kp_idxs=kp_t, gt_kps=gt_kps, samples=samples, z_cutoff=z_cutoff,
								  return_samples=True, **(dict(surface=True) if surface else {}), **(dict(measurements=spec) if spec is not None else {}),
								  **(dict(align=align) if align is not None else {}), **(dict(volume=volume) if volume is not None else {}),
								  **(dict(return_per_foot=True) if surface or spec is not None or align is not None or volume is not None else {}))
			metrics, (_, pred_pts) = got[0], got[1]
			surf_per_foot = got[2] if surface or spec is not None or align is not None or volume is not None else {}
			per_foot = torch.norm(pred_verts[:, kp_t] - gt_kps, dim=-1) * 1e3
			written = {}
			if produce_spins:
				written = _spins(gt_meshes, pred_meshes, gt_all, pred_verts, pred_pts, os.path.join(out_dir, 'spins'), spin_frames, spin_image_size, spin_format,
								 pred_all if surface else None)
			if export_meshes:
				written.setdefault('files', []).extend(_export(gt_meshes, pred_meshes, os.path.join(out_dir, 'meshes')))
				for n, mesh in enumerate(tex_meshes):
					written['files'].extend(bake.export_textured_obj(mesh, os.path.join(out_dir, 'meshes', f'{n:02d}_pred_textured.obj')))
	finally:
		model.train(was_training)
	out = {k: float(metrics[k]) for k in ('Keypoint (mm)', f'Chamf z-cutoff {z_cutoff} (μm)', 'Chamf (μm)') + (('Scan→pred (mm)', 'Pred→scan (mm)', 'Surf (μm)') if surface else ())
		   + (measurement_names(spec) if spec is not None else ()) + (('Chamf aligned (μm)', 'Keypoint aligned (mm)') if align is not None else ()) + (('Vol IoU (%)', 'Volume err (ml)') if volume is not None else ())}
	if not (return_per_foot or render_correspondences or keep_meshes):
		return out
	extra = dict(written)
	if return_per_foot:
		extra['keypoint_mm'] = per_foot
		if surface:
			extra['scan_to_pred_mm'], extra['pred_to_scan_mm'] = surf_per_foot['Scan→pred (mm)'], surf_per_foot['Pred→scan (mm)']
		if spec is not None:
			extra['measure_pred_mm'], extra['measure_gt_mm'] = surf_per_foot['measure_pred_mm'], surf_per_foot['measure_gt_mm']
		if align is not None:
			extra.update({k: surf_per_foot[k] for k in ('align_R', 'align_T', 'align_s', 'align_rmse')})
		if volume is not None:
			extra.update({k: surf_per_foot[k] for k in ('vol_iou', 'volume_pred_ml', 'volume_gt_ml')})
	if render_correspondences:
		extra.update({k: torch.cat(v) for k, v in images.items()})
	return out, extra


def _spins(gt_meshes, pred_meshes, gt_all, pred_verts, pred_pts, spins_dir, nframes, image_size, fmt, pred_all=None):
	"""The six spins per foot of eval_3d.py:163-201; the heat maps of all feet come from one vertex_errors call -- from one surface_errors call
	when pred_all, the predictions as one batch, is given.  Returns the error tensors and the files written."""
	from . import vis
	os.makedirs(spins_dir, exist_ok=True)
	n_gt = gt_all.num_verts_per_mesh()
	pred_err, gt_err = vis.vertex_errors(pred_verts, gt_all.verts_padded(), pred_pts, n_gt) if pred_all is None else vis.surface_errors(pred_all, gt_all)
	pred_col, gt_col = vis.error_colours(pred_err), vis.error_colours(gt_err)
	files = []
	for n, (gt, pred) in enumerate(zip(gt_meshes, pred_meshes)):
		vg = gt.verts_padded().shape[1]   # (padded to the largest scan of its batch: the rows past its own vertices are in no face)
		heat_p, heat_g = pred_col[n:n + 1], gt_col[n:n + 1, :vg].contiguous()
		renders = ((pred, pred.textures, 'pred_rgb'), (pred, TexturesVertex(heat_p), 'pred_chamf'), (pred, TexturesVertex(torch.full_like(heat_p, 0.5)), 'pred_grey'),
				   (gt, gt.textures, 'gt_rgb'), (gt, TexturesVertex(heat_g), 'gt_chamf'), (gt, TexturesVertex(torch.full_like(heat_g, 0.5)), 'gt_grey'))
		for mesh, texture, name in renders:
			mesh = mesh.update_padded(mesh.verts_padded())   # (a shallow copy: the caller's mesh keeps its texture)
			mesh.textures = texture
			loc = os.path.join(spins_dir, f'{n:02d}_{name}.{fmt.lstrip(".")}')
			vis.turntable(mesh, out_loc=loc, nframes=nframes, silent=True, azim=70, dist=0.35, image_size=image_size)
			files.append(loc)
	return {'pred_vertex_error': pred_err, 'gt_vertex_error': [gt_err[n, :int(v)] for n, v in enumerate(n_gt)], 'files': files}


def _export(gt_meshes, pred_meshes, mesh_dir):
	"""{n:02d}_gt_mesh.obj and {n:02d}_pred_mesh.obj per foot (eval_3d.py:204-217).  Returns the files written."""
	from . import vis
	os.makedirs(mesh_dir, exist_ok=True)
	files = []
	for n, (gt, pred) in enumerate(zip(gt_meshes, pred_meshes)):
		for key, mesh in (('gt_mesh', gt), ('pred_mesh', pred)):
			files.append(vis.export_obj(mesh, os.path.join(mesh_dir, f'{n:02d}_{key}.obj')))
	return files
