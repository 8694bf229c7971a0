"""The metric loop of reference src/eval/eval_2d.py (main, eval_2d.py:50-121) on the HIP path: every validation foot and its prediction
rendered from the same views, PSNR_A / _B / _C, MSE and IOU per group of views (eval_metrics.eval_2d_metrics), the mean over all groups of
all feet.  The HD three-view render, the PNG writes, the results table and the experiment-directory walk (run_on_exp) are visualisation
and out of scope."""
import torch
from torch.utils.data import DataLoader

from .dataset import BatchCollator
from .eval_metrics import eval_2d_metrics
from .renderer import FootRenderer

METRICS = ('MSE', 'PSNR_A', 'PSNR_B', 'PSNR_C', 'IOU')


def _marked_faces(textures):
	"""Faces a scan's TexturesUV marks to hide: a final UV vertex at (0, 0) that all three UV corners of the face use (the renderer's
	convention, reference renderer.py:340-349), read from the scan's own tables.  (Collated into one ragged batch, the tables are padded
	with (0, 0) rows, and the renderer's search over the padded batch would then find another answer than for the scan alone.)"""
	vu, fu = textures.verts_uvs_padded()[0], textures.faces_uvs_padded()[0]
	if not bool((vu[-1] == 0).all()):
		return torch.zeros(0, dtype=torch.int64)
	return torch.argwhere(torch.all(fu == vu.shape[0] - 1, dim=-1)).flatten()


def eval_2d(model, dataset, image_size=128, nviews=1, batch_size=1, R=None, T=None, feet_per_call=16, return_per_image=False, device='cuda'):
	"""model: a NeuralDisplacementField or a PCAModel whose validation latent tables are indexed by the dataset's item index (batch['idx'], as
	eval_2d.py:28-35 samples them); dataset: the validation Foot3DDataset.  Views: linspace_views(nviews, dist=0.3, elev_min=-90,
	elev_max=90) unless R, T are given; groups of `batch_size` consecutive views (nviews // batch_size of them per foot, the loop bound of
	eval_2d.py:86).  Feet are rendered `feet_per_call` at a time; the metrics are per image sums composed in float64, so the result does
	not depend on that choice.  Returns {'MSE', 'PSNR_A', 'PSNR_B', 'PSNR_C', 'IOU'} as floats, and with return_per_image also the
	per-group float64 tensors (foot-major, nviews // batch_size groups per foot) as a second dict."""
	renderer = FootRenderer(image_size=image_size, device=device)
	if R is None:
		R, T = renderer.linspace_views(nviews=nviews, dist=0.3, elev_min=-90, elev_max=90)
	n_used = (R.shape[0] // batch_size) * batch_size
	if n_used == 0:
		raise ValueError(f'find_amd.evaluate.eval_2d: {R.shape[0]} views make no group of {batch_size}')
	R, T = R[:n_used].to(device), T[:n_used].to(device)
	collate = BatchCollator(device=device).collate_batches
	loader = DataLoader(dataset, batch_size=feet_per_call, shuffle=False, collate_fn=lambda items: (collate(items), [_marked_faces(it['textures']) for it in items]))
	per = {k: [] for k in METRICS}
	was_training = model.training
	model.eval()
	try:
		with torch.no_grad():
			for batch, marked in loader:
				idx = batch['idx'].to(device)
				batch.update({vec.name: vec[idx] for vec in model.latent_vectors_val})
				res = model.get_meshes_from_batch(batch, is_train=False)
				gt_rdrs = renderer(batch['mesh'], R, T, return_mask=True, mask_out_faces=True, masked_faces=marked, return_mask_out_masks=True)
				pred_rdrs = renderer(res['meshes'], R, T, return_mask=True)
				for k, v in eval_2d_metrics(pred_rdrs, gt_rdrs, batch_size).items():
					per[k].append(v)
	finally:
		model.train(was_training)
	per = {k: torch.cat(v) for k, v in per.items()}
	out = {k: float(v.mean()) for k, v in per.items()}
	return (out, per) if return_per_image else out
