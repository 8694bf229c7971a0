"""Structural similarity (SSIM, Wang et al. 2004) of two image batches on the HIP path (find_ssim_*, csrc/ssim.hip); not in the reference,
whose photometric signal is a mean squared error.  The definition is that of pytorch-msssim / the 3DGS `ssim` with data_range = L: a
separable Gaussian window of 11 taps, sigma 1.5, per channel, C1 = (0.01 L)^2, C2 = (0.03 L)^2,
    ssim = (2 mu_a mu_b + C1)(2 sigma_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(sigma_a^2 + sigma_b^2 + C2)),
on a = pred * pred_mask, b = target * target_mask.  border 'same': the window is zero-padded and the mean runs over every value (3DGS);
'valid': the mean runs over the values whose window lies inside the image (pytorch-msssim).  One pass each way, no atomics: two runs agree
bit for bit.  GPU only."""
import torch

from . import _lib
from ._lib import check, current_stream, ptr
from .functional import _c, _require_gpu

BORDERS = ('same', 'valid')
WINDOW = 11


class _SSIM(torch.autograd.Function):
	@staticmethod
	def forward(ctx, x, xm, y, ym, L_range, valid, want_per_image, want_grad):
		L = _lib.lib()
		x, xm, y, ym = _c(x), _c(xm), _c(y), _c(ym)
		n_img, H, W, C = x.shape
		nbytes = L.find_ssim_ws_bytes(n_img, H, W, C, 0)
		if nbytes < 0:
			check(-1, 'find_ssim_ws_bytes')
		ws = torch.empty(nbytes // 8, device=x.device, dtype=torch.float64)   # a partial sum per tile
		mean = torch.empty((), device=x.device, dtype=torch.float32)
		per_image = torch.empty(n_img, device=x.device, dtype=torch.float64) if want_per_image else None
		# what the backward gathers: d ssim / d (E[a], E[a^2], E[ab]) of every pixel and channel, 12 C bytes per pixel.  want_grad is decided
		# by the caller: in here the grad mode is always off, and needs_input_grad mirrors requires_grad whatever the caller's mode was
		dmaps = torch.empty(n_img, C, 3, H, W, device=x.device, dtype=torch.float32) if want_grad else None
		check(L.find_ssim_fwd(ptr(x), ptr(xm), ptr(y), ptr(ym), n_img, H, W, C, L_range, valid, ptr(mean), ptr(per_image), ptr(dmaps), ptr(ws),
							  ws.numel() * 8, current_stream(x.device)), 'find_ssim_fwd')
		ctx.args = (n_img, H, W, C, L_range, valid)
		ctx.has_maps = dmaps is not None
		ctx.save_for_backward(x, xm, y, ym, dmaps)
		if per_image is not None:
			ctx.mark_non_differentiable(per_image)
		return mean, per_image

	@staticmethod
	def backward(ctx, g, _gp):
		x, xm, y, ym, dmaps = ctx.saved_tensors
		n_img, H, W, C, L_range, valid = ctx.args
		d_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
		d_xm = torch.empty_like(xm) if (xm is not None and ctx.needs_input_grad[1]) else None
		if d_x is None and d_xm is None:
			return None, None, None, None, None, None, None, None
		if not ctx.has_maps:
			raise RuntimeError('find_amd.ssim: the forward ran without a gradient map (no input required a gradient)')
		check(_lib.lib().find_ssim_bwd(ptr(x), ptr(xm), ptr(y), ptr(ym), n_img, H, W, C, L_range, valid, ptr(_c(g)), ptr(dmaps), ptr(d_x), ptr(d_xm),
									   current_stream(x.device)), 'find_ssim_bwd')
		return d_x, d_xm, None, None, None, None, None, None


def ssim(pred, target, pred_mask=None, target_mask=None, data_range=1.0, border='same', return_per_image=False):
	"""Mean SSIM of pred and target (..., H, W, C) fp32, channel-last, C <= 4; leading dimensions fold into images ((N, M, H, W, C): N * M of
	them).  pred_mask, target_mask (..., H, W) or None (= 1) are multiplied in: ssim(pred * pred_mask[..., None], target * target_mask[..., None]).
	Returns an fp32 scalar, the mean over images of each image's mean; with return_per_image also the (n_img,) float64 per-image values
	(no gradient).  The gradient goes to pred and pred_mask; target and target_mask carry none.  border 'same' | 'valid' (H, W >= 11): see
	the module's docstring."""
	if border not in BORDERS:
		raise ValueError(f"find_amd.ssim: border 'same' or 'valid', got {border!r}")
	if not data_range > 0:
		raise ValueError(f'find_amd.ssim: data_range > 0 expected, got {data_range}')
	if pred.dim() < 3:
		raise ValueError(f'find_amd.ssim: images are (..., H, W, C), got {tuple(pred.shape)}')
	H, W, C = pred.shape[-3:]
	if C > 4:
		raise ValueError(f'find_amd.ssim: at most 4 channels, got {C}')
	if border == 'valid' and (H < WINDOW or W < WINDOW):
		raise ValueError(f"find_amd.ssim: border 'valid' needs H, W >= {WINDOW}, got {H} x {W}")
	_require_gpu(pred, target, pred_mask, target_mask)
	if target.shape != pred.shape or pred.numel() == 0:
		raise RuntimeError(f'find_amd.ssim: pred and target of one non-empty shape (..., H, W, C) expected, got {tuple(pred.shape)} / {tuple(target.shape)}')
	for name, m in (('pred_mask', pred_mask), ('target_mask', target_mask)):
		if m is not None and m.shape != pred.shape[:-1]:
			raise RuntimeError(f'find_amd.ssim: {name} {tuple(m.shape)} must have the images\' shape without channels {tuple(pred.shape[:-1])}')

	# the gradient maps are written only when a backward can follow: an input requires a gradient AND the grad mode is on
	want_grad = torch.is_grad_enabled() and (pred.requires_grad or (pred_mask is not None and pred_mask.requires_grad))

	def fold(t, tail):
		return None if t is None else t.reshape((-1,) + tuple(tail))
	mean, per_image = _SSIM.apply(fold(pred, (H, W, C)), fold(pred_mask, (H, W)), fold(target.detach(), (H, W, C)),
								  fold(None if target_mask is None else target_mask.detach(), (H, W)), float(data_range), int(border == 'valid'),
								  bool(return_per_image), want_grad)
	return (mean, per_image) if return_per_image else mean
