"""SSIM restated in torch on the CPU, from the definition (Wang et al. 2004 with the conventions find_hip.h names): what tests/test_ssim_host.py
checks against closed forms and tests/test_gpu_ssim.py holds the HIP path to.  Everything runs in the dtype of the inputs; float64 is the truth.

  window     11 taps of exp(-d^2 / (2 * 1.5^2)), normalised to sum 1 in double and rounded to fp32 -- the constants of the definition -- then
             taken to the working dtype
  means      F.conv2d per channel (groups = C) with zero padding, the row pass and then the column pass of the separable window
  value      ((2 m1 m2 + C1)(2 (s12 - m1 m2) + C2)) / ((m1^2 + m2^2 + C1)((s11 - m1^2) + (s22 - m2^2) + C2)), C1 = (0.01 L)^2, C2 = (0.03 L)^2
  border     'same': the mean of an image's H W C values;  'valid': of the (H - 10)(W - 10) C values whose window lies inside the image
  masks      a = x * xm[..., None], b = y * ym[..., None]
Gradients come from autograd."""
import torch
import torch.nn.functional as F

TAPS, RAD, SIGMA = 11, 5, 1.5


def window(dtype=torch.float64):
	d = torch.arange(TAPS, dtype=torch.float64) - RAD
	g = torch.exp(-d * d / (2 * SIGMA * SIGMA))
	return (g / g.sum()).float().to(dtype)


def _blur(t, w):
	"""t (n, C, H, W): the window mean around every pixel, zeros outside the image."""
	C = t.shape[1]
	t = F.conv2d(t, w.view(1, 1, 1, TAPS).expand(C, 1, 1, TAPS), padding=(0, RAD), groups=C)
	return F.conv2d(t, w.view(1, 1, TAPS, 1).expand(C, 1, TAPS, 1), padding=(RAD, 0), groups=C)


def ssim_map(a, b, data_range=1.0):
	"""a, b (n, H, W, C)  ->  the 'same' map (n, H, W, C)."""
	w = window(a.dtype)
	a, b = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)
	c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
	m1, m2, s11, s22, s12 = _blur(a, w), _blur(b, w), _blur(a * a, w), _blur(b * b, w), _blur(a * b, w)
	num = (2 * m1 * m2 + c1) * (2 * (s12 - m1 * m2) + c2)
	den = (m1 * m1 + m2 * m2 + c1) * ((s11 - m1 * m1) + (s22 - m2 * m2) + c2)
	return (num / den).permute(0, 2, 3, 1)


def ssim_ref(x, y, xm=None, ym=None, data_range=1.0, border='same', per_image=False):
	"""x, y (n, H, W, C), xm, ym (n, H, W) or None  ->  the mean over images of the per-image means (a 0-d tensor); per_image: also those (n,)."""
	if border not in ('same', 'valid'):
		raise ValueError(border)
	a = x if xm is None else x * xm[..., None]
	b = y if ym is None else y * ym[..., None]
	m = ssim_map(a, b, data_range)
	if border == 'valid':
		m = m[:, RAD:m.shape[1] - RAD, RAD:m.shape[2] - RAD]
	per = m.reshape(m.shape[0], -1).mean(1)
	return (per.mean(), per) if per_image else per.mean()
