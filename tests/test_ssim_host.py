"""SSIM on the host: the torch restatement (tests/ssim_ref.py) against closed forms, the C interface, and what the wrappers, the options and the
Trainer say before any kernel runs."""
import inspect
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ssim_ref import RAD, TAPS, ssim_map, ssim_ref, window   # noqa: E402

SYMBOLS = ('find_ssim_fwd', 'find_ssim_bwd')


# ------------------------------------------------------------------ the reference against closed forms
def test_window_is_the_normalised_gaussian():
	w = window()
	assert w.shape == (TAPS,) and w.dtype == torch.float64 and torch.equal(w, w.flip(0)) and int(w.argmax()) == RAD
	assert torch.equal(w, w.float().double())          # fp32 constants
	assert abs(float(w.sum()) - 1) < 2e-7              # (each rounded by at most 2^-25 of itself)
	assert abs(float(w[RAD + 1] / w[RAD]) - torch.exp(torch.tensor(-1 / 4.5, dtype=torch.float64)).item()) < 1e-7


def test_identical_images_give_exactly_one():
	g = torch.Generator().manual_seed(0)
	x = torch.rand(2, 17, 23, 3, generator=g, dtype=torch.float64)
	m = torch.rand(2, 17, 23, generator=g, dtype=torch.float64)
	for border in ('same', 'valid'):
		assert ssim_ref(x, x, border=border).item() == 1.0
		assert ssim_ref(x, x.clone(), m, m.clone(), border=border).item() == 1.0
		mean, per = ssim_ref(x.float(), x.float(), border=border, per_image=True)
		assert mean.item() == 1.0 and (per == 1).all() and per.shape == (2,)


@pytest.mark.parametrize('L', [1.0, 255.0])
def test_constant_images_under_valid(L):
	p, q = 0.75 * L, 0.25 * L
	a, b = torch.full((1, 13, 16, 2), p, dtype=torch.float64), torch.full((1, 13, 16, 2), q, dtype=torch.float64)
	c1 = (0.01 * L) ** 2
	# the window's fp32 constants sum to 1 within 2e-7: variances of 2e-7 p^2 against C2 = 9e-4 L^2
	assert abs(ssim_ref(a, b, data_range=L, border='valid').item() - (2 * p * q + c1) / (p * p + q * q + c1)) < 1e-3
	w = window()
	s = float(w.sum()) ** 2
	m1, m2 = p * s, q * s
	c2 = (0.03 * L) ** 2
	want = (2 * m1 * m2 + c1) * (2 * (p * q * s - m1 * m2) + c2) / ((m1 * m1 + m2 * m2 + c1) * ((p * p * s - m1 * m1) + (q * q * s - m2 * m2) + c2))
	assert abs(ssim_ref(a, b, data_range=L, border='valid').item() - want) < 1e-12


def test_valid_is_the_interior_of_same():
	g = torch.Generator().manual_seed(1)
	x, y = torch.rand(3, 14, 19, 3, generator=g, dtype=torch.float64), torch.rand(3, 14, 19, 3, generator=g, dtype=torch.float64)
	xm, ym = torch.rand(3, 14, 19, generator=g, dtype=torch.float64), torch.rand(3, 14, 19, generator=g, dtype=torch.float64)
	full = ssim_map(x * xm[..., None], y * ym[..., None])
	assert full.shape == (3, 14, 19, 3)
	inner = full[:, RAD:-RAD, RAD:-RAD]
	mean, per = ssim_ref(x, y, xm, ym, border='valid', per_image=True)
	assert torch.equal(per, inner.reshape(3, -1).mean(1)) and mean.item() == per.mean().item()
	mean_s, per_s = ssim_ref(x, y, xm, ym, border='same', per_image=True)
	assert torch.equal(per_s, full.reshape(3, -1).mean(1)) and 0 < mean_s.item() < mean.item() + 1
	# an interior value reads nothing of the padding: the same map from an image embedded in a larger one
	big_x, big_y = torch.rand(3, 24, 29, 3, generator=g, dtype=torch.float64), torch.rand(3, 24, 29, 3, generator=g, dtype=torch.float64)
	big_x[:, 5:19, 5:24], big_y[:, 5:19, 5:24] = x, y
	assert torch.allclose(ssim_map(big_x, big_y)[:, 10:14, 10:19], ssim_map(x, y)[:, RAD:-RAD, RAD:-RAD], rtol=0, atol=1e-14)


def test_gradient_of_the_reference_is_autograd():
	g = torch.Generator().manual_seed(2)
	x = torch.rand(1, 12, 13, 2, generator=g, dtype=torch.float64, requires_grad=True)
	xm = torch.rand(1, 12, 13, generator=g, dtype=torch.float64, requires_grad=True)
	y, ym = torch.rand(1, 12, 13, 2, generator=g, dtype=torch.float64), torch.rand(1, 12, 13, generator=g, dtype=torch.float64)
	assert torch.autograd.gradcheck(lambda a, m: ssim_ref(a, y, m, ym, border='valid'), (x, xm), eps=1e-6, atol=1e-6)
	ssim_ref(x, y, xm, ym, border='valid').backward()
	assert x.grad[0, 0, 0].abs().max() > 0   # a border pixel lies in a counting pixel's window


# ------------------------------------------------------------------ interface
def test_header_and_bindings_declare_the_symbols():
	from find_amd import _lib
	hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'find_hip.h')).read()
	for name in SYMBOLS:
		assert re.search(r'\bint ' + name + r'\(', hdr), name
		assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name), name
	assert re.search(r'\bint64_t find_ssim_ws_bytes\(', hdr) and 'find_ssim_ws_bytes' in _lib.PROTOTYPES
	assert len(_lib.PROTOTYPES['find_ssim_fwd'][1]) == 16 and len(_lib.PROTOTYPES['find_ssim_bwd'][1]) == 15
	assert _lib.ABI_VERSION == 3 and _lib.lib().find_abi_version() == 3
	assert os.path.exists(os.path.join(os.path.dirname(HERE), 'find_amd', 'csrc', 'ssim.hip'))


def test_ws_bytes_and_refusals():
	from find_amd import _lib
	L = _lib.lib()
	# a double per 16 x 16 tile; with want_grad the bytes of the gradient maps, 3 C floats per pixel
	assert L.find_ssim_ws_bytes(1, 16, 16, 3, 0) == 8 and L.find_ssim_ws_bytes(3, 17, 33, 4, 0) == 3 * 2 * 3 * 8
	assert L.find_ssim_ws_bytes(1, 16, 16, 3, 1) == 16 * 16 * 9 * 4 and L.find_ssim_ws_bytes(2, 7, 40, 1, 1) == 2 * 7 * 40 * 3 * 4
	for bad in ((0, 16, 16, 3), (1, 0, 16, 3), (1, 16, -1, 3), (1, 16, 16, 0), (1, 16, 16, 5)):
		L.find_image_mse_ws_bytes()
		assert L.find_ssim_ws_bytes(*bad, 0) == -1 and b'bad sizes' in L.find_last_error() and b'find_ssim_ws_bytes' in L.find_last_error(), bad
	one = torch.zeros(4)
	P = _lib.ptr
	# refused before anything is launched (host pointers are never read)
	assert L.find_ssim_fwd(None, None, P(one), None, 1, 1, 1, 1, 1.0, 0, P(one), None, None, P(one), 8, None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_ssim_fwd(P(one), None, P(one), None, 1, 1, 1, 5, 1.0, 0, P(one), None, None, P(one), 8, None) == -1 and b'bad sizes' in L.find_last_error()
	assert L.find_ssim_fwd(P(one), None, P(one), None, 1, 1, 1, 1, 0.0, 0, P(one), None, None, P(one), 8, None) == -1 and b'data_range' in L.find_last_error()
	assert L.find_ssim_fwd(P(one), None, P(one), None, 1, 10, 16, 1, 1.0, 1, P(one), None, None, P(one), 8, None) == -1 and b'valid' in L.find_last_error()
	assert L.find_ssim_fwd(P(one), None, P(one), None, 1, 17, 16, 1, 1.0, 0, P(one), None, None, P(one), 8, None) == -2 and b'workspace' in L.find_last_error()
	assert L.find_ssim_bwd(P(one), None, P(one), None, 1, 1, 1, 1, 1.0, 0, P(one), P(one), None, None, None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_ssim_bwd(P(one), None, P(one), None, 1, 1, 1, 1, 1.0, 0, P(one), P(one), None, P(one), None) == -1 and b'd_xm without xm' in L.find_last_error()


def test_argument_checks_come_before_the_device_check():
	from find_amd import eval_metrics
	from find_amd.losses import SSIMLoss
	from find_amd.ssim import ssim
	x = torch.rand(2, 12, 12, 3)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		ssim(x, x)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		SSIMLoss()(x, x, torch.ones(2, 12, 12))
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		eval_metrics.SSIM(x, x)
	with pytest.raises(ValueError, match='border'):
		ssim(x, x, border='reflect')
	with pytest.raises(ValueError, match='border'):
		SSIMLoss(border='full')
	with pytest.raises(ValueError, match='data_range'):
		ssim(x, x, data_range=0.)
	with pytest.raises(ValueError, match='data_range'):
		SSIMLoss(data_range=-1.)
	with pytest.raises(ValueError, match='4 channels'):
		ssim(torch.rand(2, 12, 12, 5), torch.rand(2, 12, 12, 5))
	with pytest.raises(ValueError, match="'valid' needs"):
		ssim(torch.rand(2, 10, 12, 3), torch.rand(2, 10, 12, 3), border='valid')
	with pytest.raises(ValueError, match="'valid' needs"):
		SSIMLoss(border='valid')(torch.rand(2, 12, 10, 3), torch.rand(2, 12, 10, 3))
	loss = SSIMLoss(data_range=2., border='valid')
	assert (loss.data_range, loss.border) == (2., 'valid') and 'not in the reference' in SSIMLoss.__doc__
	assert list(inspect.signature(ssim).parameters) == ['pred', 'target', 'pred_mask', 'target_mask', 'data_range', 'border', 'return_per_image']
	assert inspect.signature(eval_metrics.SSIM).parameters['border'].default == 'valid'


def test_wrappers_live_in_a_module_of_their_own():
	"""The poison census of tests/test_poison_host.py walks four modules; the SSIM wrappers allocate and belong to none of them."""
	from test_poison_host import allocating_ops
	root = os.path.join(os.path.dirname(HERE), 'find_amd')
	assert allocating_ops(os.path.join(root, 'ssim.py')) == ['_SSIM']
	for mod in ('functional.py', 'functional_render.py', 'vis.py', 'optim.py'):
		assert 'ssim' not in open(os.path.join(root, mod)).read().lower(), mod


def test_options_registry_and_signatures():
	from find_amd import evaluate
	from find_amd import model_with_loss as M
	from find_amd.opts import Opts
	assert Opts().pix_ssim_lambda == 0. and Opts(pix_ssim_lambda=0.2).pix_ssim_lambda == 0.2
	assert M.PIX_DEFAULTS == dict(pix_ssim_lambda=0.)
	assert len(Opts().net_train_kwargs()) == 10
	names = list(inspect.signature(M.ModelWithLoss.forward).parameters)
	assert names[-3:] == ['depth', 'cont_pairs', 'normal'] and 'ssim' not in names
	assert [t.key for t in M.TERMS].count('loss_pix') == 1 and not any('ssim' in t.flag for t in M.TERMS + M.EVERY_EXTENSION_TERM)
	sig = inspect.signature(evaluate.eval_2d).parameters
	assert list(sig)[-1] == 'ssim' and sig['ssim'].default is False
	assert evaluate.METRICS == ('MSE', 'PSNR_A', 'PSNR_B', 'PSNR_C', 'IOU')


def test_gradient_maps_are_asked_for_only_when_a_backward_can_follow(monkeypatch):
	"""want_grad is decided in ssim(): inside an autograd Function's forward the grad mode is always off, and needs_input_grad mirrors
	requires_grad whatever the caller's mode was."""
	from find_amd import ssim as mod
	seen = []

	class Stub:
		@staticmethod
		def apply(*args):
			assert len(args) == 8
			seen.append(args[-1])
			return torch.zeros(()), None
	monkeypatch.setattr(mod, '_SSIM', Stub)
	monkeypatch.setattr(mod, '_require_gpu', lambda *t: None)
	x, m = torch.rand(1, 12, 12, 3, requires_grad=True), torch.rand(1, 12, 12, requires_grad=True)
	y = torch.rand(1, 12, 12, 3)
	mod.ssim(x, y)
	mod.ssim(y, y, m)
	mod.ssim(y, y, m.detach(), m)      # (the target's mask carries no gradient)
	with torch.no_grad():
		mod.ssim(x, y, m)
	mod.ssim(y, y)
	assert seen == [True, True, False, False, False]


def test_the_share_is_a_share():
	import types
	from find_amd import model_with_loss as M
	from find_amd.opts import Opts
	for bad in (-0.1, 1.5, float('nan')):
		with pytest.raises(ValueError, match='pix_ssim_lambda'):   # before anything is launched
			M.ModelWithLoss._raw_pix(None, types.SimpleNamespace(opts=Opts(pix_ssim_lambda=bad)))


def test_trainer_runs_the_structural_share_eagerly():
	from find_amd import optim
	from find_amd.opts import Opts
	from find_amd.trainer import Trainer
	p = torch.nn.Parameter(torch.zeros(3))
	kw = dict(pix=True, sil=True, render_foot=True)

	def trainer(opts):
		return Trainer([optim.Adam([p], capturable=True)], None, [], [], opts, device='cuda:0', graph='auto')
	tr = trainer(Opts(pix_ssim_lambda=0.2))
	assert 'pix_ssim_lambda' in tr._why_not_graph(tr.optims, kw)
	assert tr._why_not_graph(tr.optims, dict(sil=True, render_foot=True)) is None   # the pixel term is off: nothing to say
	assert tr._mode(tr.optims, None, kw) is None                                    # 'auto': eager
	tr.graph = True
	with pytest.raises(RuntimeError, match='pix_ssim_lambda'):
		tr._mode(tr.optims, None, kw)
	assert 'pix_ssim_lambda' in trainer(Opts(pix_ssim_lambda=-0.2))._why_not_graph(tr.optims, kw)   # (refused by the step itself; never captured)
	tr0 = trainer(Opts())
	assert tr0._why_not_graph(tr0.optims, kw) is None

	class ReferenceOpts:   # an options object that has never heard of the option
		step_per_epoch = False
	tr1 = trainer(ReferenceOpts())
	assert tr1._why_not_graph(tr1.optims, kw) is None
