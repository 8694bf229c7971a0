"""SSIM on the MI355X: find_ssim_fwd / _bwd through find_amd.ssim.ssim against the float64 torch restatement of the definition
(tests/ssim_ref.py) on the same fp32 inputs, and its place in losses, eval_metrics, evaluate.eval_2d and ModelWithLoss.

Margins: none is a constant of the code under test.  sigma^2 = E[a^2] - mu^2 cancels in fp32 against C2 = 9e-4, so what fp32 can reach is a
property of the number format: every comparison also evaluates the same reference in float32 on the CPU; with e32 its worst error against
float64 (max-abs, for the mean, the per-image values and each gradient tensor) the HIP result must lie within 4 e32 + 1e-7 of the float64
value.  Each case prints its figures (DESIGN 7.8 records them).

Shapes: the tile is 16 x 16 with a 5-pixel halo.  (11, 11) is smaller than a tile and the smallest `valid` image (one counting pixel);
(16, 16) exactly one tile; (17, 33) one past a tile down and one past two tiles across, W C = 99 odd; (7, 40) (`same` only) lower than the
window; (48, 21) exactly three tiles down, a partial second tile across, W C = 63 odd.  C = 1, 3 and, at (17, 33), 4."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import poison   # noqa: E402
from ssim_ref import ssim_ref   # noqa: E402

SHAPES = [(11, 11, 1), (11, 11, 3), (16, 16, 1), (16, 16, 3), (17, 33, 1), (17, 33, 3), (17, 33, 4), (7, 40, 1), (7, 40, 3), (48, 21, 1), (48, 21, 3)]
MASKS = ('none', 'both', 'pred')


def _held(name, hip, ref64, ref32):
	e_hip = (hip.detach().double().cpu() - ref64).abs().max().item()
	e32 = (ref32.detach().double() - ref64).abs().max().item()
	print(f'{name}: e_hip {e_hip:.3e}  e32 {e32:.3e}  scale {ref64.abs().max().item():.3e}')
	assert np.isfinite(e_hip) and e_hip <= 4 * e32 + 1e-7, (name, e_hip, e32)


def _fields(n, H, W, C, seed):
	"""Smooth random images and masks in [0, 1] with a flat corner, as a render's background: both images white and both masks 0 there, the
	target's corner one row taller and one column narrower than the prediction's (two silhouettes never agree)."""
	g = torch.Generator().manual_seed(seed)

	def smooth(ch):
		low = torch.rand(n, ch, H // 4 + 2, W // 4 + 2, generator=g)
		return F.interpolate(low, size=(H, W), mode='bicubic', align_corners=True).clamp(0, 1).permute(0, 2, 3, 1).contiguous()
	x, y = smooth(C), smooth(C)
	y = (0.7 * x + 0.3 * y).contiguous()
	xm, ym = smooth(1)[..., 0].contiguous(), smooth(1)[..., 0].contiguous()
	h, w = max(H // 3, 1), max(W // 2, 2)
	x[:, :h, :w], xm[:, :h, :w] = 1., 0.
	y[:, :h + 1, :w - 1], ym[:, :h + 1, :w - 1] = 1., 0.
	return x, y, xm, ym


def _pick(masks, xm, ym):
	return (None, None) if masks == 'none' else (xm, ym) if masks == 'both' else (xm, None)


def _hip(x, y, xm, ym, border, L=1.0):
	from find_amd.ssim import ssim
	xs = x.cuda().requires_grad_()
	ms = None if xm is None else xm.cuda().requires_grad_()
	mean, per = ssim(xs, y.cuda(), ms, None if ym is None else ym.cuda(), data_range=L, border=border, return_per_image=True)
	assert mean.dtype == torch.float32 and mean.dim() == 0 and per.dtype == torch.float64 and not per.requires_grad
	mean.backward()
	torch.cuda.synchronize()
	return mean.detach(), per, xs.grad, None if ms is None else ms.grad


def _ref(dtype, x, y, xm, ym, border, L=1.0):
	xs = x.to(dtype).requires_grad_()
	ms = None if xm is None else xm.to(dtype).requires_grad_()
	mean, per = ssim_ref(xs, y.to(dtype), ms, None if ym is None else ym.to(dtype), data_range=L, border=border, per_image=True)
	mean.backward()
	return mean.detach(), per.detach(), xs.grad, None if ms is None else ms.grad


def _against_float64(name, x, y, xm, ym, border, L=1.0):
	got = _hip(x, y, xm, ym, border, L)
	shape = x.shape[-3:]
	fold = [t if t is None else t.reshape((-1,) + tuple(shape[:k])) for t, k in ((x, 3), (y, 3), (xm, 2), (ym, 2))]
	r64, r32 = _ref(torch.float64, *fold, border, L), _ref(torch.float32, *fold, border, L)
	for what, h, a, b in zip(('mean', 'per image', 'd_x', 'd_xm'), got, r64, r32):
		if a is None:
			assert h is None
			continue
		_held(f'{name} {what}', h.reshape(a.shape), a, b)
	return got, r64


# ------------------------------------------------------------------ the kernels against float64
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_ssim_against_float64(shape):
	H, W, C = shape
	for n in (1, 3):
		x, y, xm, ym = _fields(n, H, W, C, seed=H * W + C + n)
		for masks in MASKS:
			for border in ('same', 'valid') if min(H, W) >= 11 else ('same',):
				(mean, per, d_x, d_xm), (m64, _, g64, _) = _against_float64(f'{H}x{W}x{C} n={n} {masks} {border}', x, y, *_pick(masks, xm, ym), border)
				assert abs(mean.item()) < 1 and per.shape == (n,) and d_x.shape == x.shape and g64.abs().max() > 0


def test_data_range_255():
	x, y, xm, ym = _fields(2, 17, 33, 3, seed=11)
	_against_float64('17x33x3 L=255 both same', x * 255, y * 255, xm, ym, 'same', L=255.)
	_against_float64('17x33x3 L=255 none valid', x * 255, y * 255, None, None, 'valid', L=255.)


def test_identical_images():
	x, _, xm, _ = _fields(2, 17, 33, 3, seed=3)
	for border in ('same', 'valid'):
		for masks in ('none', 'both'):
			m = xm if masks == 'both' else None
			(mean, per, d_x, d_xm), (m64, _, g64, _) = _against_float64(f'identical {masks} {border}', x, x.clone(), m, None if m is None else m.clone(), border)
			assert m64.item() == 1.0 and g64.abs().max().item() < 1e-12   # (what the bound is held against)


def test_non_contiguous_inputs_and_folding():
	from find_amd.ssim import ssim
	x, y, xm, ym = _fields(4, 17, 33, 3, seed=5)
	want = _hip(x, y, xm, ym, 'same')
	# channel-first storage seen channel-last, masks as every second column of a wider tensor
	xs = x.permute(0, 3, 1, 2).contiguous().cuda().permute(0, 2, 3, 1).requires_grad_()
	ys = y.permute(0, 3, 1, 2).contiguous().cuda().permute(0, 2, 3, 1)
	wide = torch.zeros(4, 17, 66, device='cuda')
	wide[..., ::2] = xm.cuda()
	ms = wide[..., ::2].requires_grad_()
	assert not xs.is_contiguous() and not ys.is_contiguous() and not ms.is_contiguous()
	mean, per = ssim(xs, ys, ms, ym.cuda(), return_per_image=True)
	mean.backward()
	assert torch.equal(mean, want[0]) and torch.equal(per, want[1]) and torch.equal(xs.grad, want[2]) and torch.equal(ms.grad, want[3])
	# (2, 2, H, W, 3) folds to four images
	x5, m5 = x.reshape(2, 2, 17, 33, 3), xm.reshape(2, 2, 17, 33)
	got, _ = _against_float64('5-D fold same', x5, y.reshape(2, 2, 17, 33, 3), m5, ym.reshape(2, 2, 17, 33), 'same')
	assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2].shape == x5.shape and got[3].shape == m5.shape
	assert torch.equal(got[2].reshape(x.shape), want[2]) and torch.equal(got[3].reshape(xm.shape), want[3])
	with pytest.raises(RuntimeError, match='one non-empty shape'):
		ssim(x.cuda(), y.cuda()[:, :-1])
	with pytest.raises(RuntimeError, match='pred_mask'):
		ssim(x.cuda(), y.cuda(), xm.cuda()[:, :-1])
	# no gradient asked for: no gradient maps, the same values
	with torch.no_grad():
		assert torch.equal(ssim(x.cuda(), y.cuda(), xm.cuda(), ym.cuda()), want[0])
	assert torch.equal(ssim(x.cuda(), y.cuda(), xm.cuda(), ym.cuda()), want[0])


class _Recorder(poison._TorchProxy):
	"""tests/poison.py's proxy, keeping the shape of every torch.empty it hands out."""

	def empty(self, *args, **kwargs):
		t = super().empty(*args, **kwargs)
		self.__dict__.setdefault('shapes', []).append(tuple(t.shape))
		return t


def test_gradient_maps_are_made_only_when_a_backward_can_follow():
	"""The (n, C, 3, H, W) maps -- 12 C bytes per pixel -- are allocated and written when an input requires a gradient AND the grad mode
	is on: not under no_grad with inputs that require one (a validation step), not for inputs that require none."""
	from find_amd import ssim as mod
	x, y, xm, ym = _fields(2, 17, 33, 3, seed=17)
	maps = (2, 3, 3, 17, 33)
	xs, ms = x.cuda().requires_grad_(), xm.cuda().requires_grad_()

	def shapes(fn):
		rec = _Recorder(0xFF)
		assert mod.torch is torch
		try:
			mod.torch = rec
			out = fn()
		finally:
			mod.torch = torch
		return out, rec.__dict__.get('shapes', [])
	with_grad, made = shapes(lambda: mod.ssim(xs, y.cuda(), ms, ym.cuda()))
	assert maps in made and with_grad.requires_grad
	with torch.no_grad():
		quiet, made = shapes(lambda: mod.ssim(xs, y.cuda(), ms, ym.cuda()))
	assert maps not in made and not any(len(sh) == 5 for sh in made) and not quiet.requires_grad and torch.equal(quiet, with_grad.detach())
	plain, made = shapes(lambda: mod.ssim(x.cuda(), y.cuda(), xm.cuda(), ym.cuda()))
	assert maps not in made and torch.equal(plain, quiet)
	only_mask, made = shapes(lambda: mod.ssim(x.cuda(), y.cuda(), ms, ym.cuda()))
	assert maps in made and torch.equal(only_mask.detach(), quiet)
	only_mask.backward()
	assert ms.grad is not None and torch.isfinite(ms.grad).all()


def test_two_runs_agree_bit_for_bit():
	x, y, xm, ym = _fields(3, 48, 21, 3, seed=9)
	for border in ('same', 'valid'):
		a, b = _hip(x, y, xm, ym, border), _hip(x, y, xm, ym, border)
		assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_loss_class_and_metric():
	from find_amd import eval_metrics
	from find_amd.losses import SSIMLoss
	from find_amd.ssim import ssim
	x, y, xm, ym = _fields(3, 17, 33, 3, seed=13)
	xc, yc, xmc, ymc = (t.cuda() for t in (x, y, xm, ym))
	for border in ('same', 'valid'):
		assert torch.equal(SSIMLoss(border=border)(xc, yc, xmc, ymc), 1. - ssim(xc, yc, xmc, ymc, border=border))
	assert torch.equal(SSIMLoss(data_range=2.)(xc, yc), 1. - ssim(xc, yc, data_range=2.))
	xs = xc.clone().requires_grad_()
	SSIMLoss()(xs, yc).backward()
	assert torch.equal(xs.grad, -_hip(x, y, None, None, 'same')[2])
	# eval_metrics.SSIM(gt, pred, gt_mask, pred_mask): per image, float64, `valid` unless asked otherwise
	for kw, border, masks in ((dict(), 'valid', False), (dict(border='same'), 'same', True)):
		per = eval_metrics.SSIM(yc, xc, *((ymc, xmc) if masks else ()), **kw)
		assert per.dtype == torch.float64 and per.shape == (3,) and not per.requires_grad
		m = (xm, ym) if masks else (None, None)
		_, p64 = ssim_ref(x.double(), y.double(), *(None if t is None else t.double() for t in m), border=border, per_image=True)
		_, p32 = ssim_ref(x, y, *m, border=border, per_image=True)
		_held(f'eval_metrics.SSIM {border}', per, p64, p32)


# ------------------------------------------------------------------ evaluate.eval_2d
def test_eval_2d_reports_the_ssim_columns(tmp_path, monkeypatch):
	"""evaluate.eval_2d(ssim=True) on the four synthetic scans of test_gpu_eval2d.py (one of them hides faces).  Two image renders differ in
	the last bits (the shader's vertex normals are float-atomic sums), so the renderer is recorded in the first call and replayed in the
	second: on the same renders the five old columns are the same bit for bit, and the new ones are the reference's on those renders.
	What two plain calls differ by is measured first and printed (tests/test_gpu_render.py, test_gpu_render_features.py and
	test_gpu_depth.py::test_eval_2d_reports_the_depth_columns hold two renders to 1e-5 for the same reason)."""
	from test_gpu_eval2d import _foot3d_val, _model
	from find_amd import evaluate
	ds = _foot3d_val(tmp_path)
	model = _model(len(ds))
	size, nviews, bs = 48, 4, 2
	once = evaluate.eval_2d(model, ds, image_size=size, nviews=nviews, batch_size=bs, feet_per_call=3)
	again = evaluate.eval_2d(model, ds, image_size=size, nviews=nviews, batch_size=bs, feet_per_call=3, ssim=True)
	apart = {k: abs(again[k] - once[k]) / max(1.0, abs(once[k])) for k in once}
	print('two plain eval_2d calls, relative difference per column:', {k: f'{v:.2e}' for k, v in apart.items()}, 'bit-equal:', all(v == 0 for v in apart.values()))
	assert all(v <= 1e-5 for v in apart.values()), apart
	tape, state = [], dict(record=True, at=0)

	class Taped(evaluate.FootRenderer):
		def __call__(self, *args, **kw):
			if state['record']:
				tape.append(super().__call__(*args, **kw))
				return tape[-1]
			state['at'] += 1
			return tape[state['at'] - 1]
	monkeypatch.setattr(evaluate, 'FootRenderer', Taped)
	plain, per_plain = evaluate.eval_2d(model, ds, image_size=size, nviews=nviews, batch_size=bs, feet_per_call=3, return_per_image=True)
	state['record'] = False
	res, per = evaluate.eval_2d(model, ds, image_size=size, nviews=nviews, batch_size=bs, feet_per_call=3, return_per_image=True, ssim=True)
	assert state['at'] == len(tape) == 4 and model.training
	assert list(plain) == list(evaluate.METRICS) and list(res) == list(plain) + ['SSIM_A', 'SSIM_B']
	for k in plain:   # (bit for bit; a group without a silhouette has nan for its IOU in both)
		assert (res[k] == plain[k] or (np.isnan(res[k]) and np.isnan(plain[k]))) and torch.equal(per[k].nan_to_num(nan=-1.), per_plain[k].nan_to_num(nan=-1.)), k
	want = {k: {d: [] for d in (torch.float64, torch.float32)} for k in ('SSIM_A', 'SSIM_B')}
	hidden = 0
	gts, preds = [r for r in tape if 'mask_out_masks' in r], [r for r in tape if 'mask_out_masks' not in r]   # (only the GT render is asked for them)
	assert len(gts) == len(preds) == 2
	for gt, pred in zip(gts, preds):
		hide = gt['mask_out_masks'].cpu()
		hidden += int(hide.sum())
		gi, gm = gt['image'].cpu(), gt['mask'].cpu()
		pi = torch.where(hide[..., None], torch.ones(()), pred['image'].cpu())
		pm = torch.where(hide, torch.zeros(()), pred['mask'].cpu())
		for d in (torch.float64, torch.float32):
			fold = lambda t, tail: t.to(d).reshape((-1, size, size) + tail)   # noqa: E731
			_, a = ssim_ref(fold(pi, (3,)), fold(gi, (3,)), border='valid', per_image=True)
			_, b = ssim_ref(fold(pi, (3,)), fold(gi, (3,)), fold((pm > 0).float(), ()), fold((gm > 0).float(), ()), border='valid', per_image=True)
			want['SSIM_A'][d].append(a.view(-1, bs).mean(1))
			want['SSIM_B'][d].append(b.view(-1, bs).mean(1))
	assert hidden > 0   # the marked scan hid some of its faces
	for k in ('SSIM_A', 'SSIM_B'):
		w64, w32 = torch.cat(want[k][torch.float64]), torch.cat(want[k][torch.float32])
		assert per[k].shape == (len(ds) * (nviews // bs),) and per[k].dtype == torch.float64
		assert ((per[k] > 0) & (per[k] <= 1)).all() and 0 < res[k] <= 1
		_held(f'eval_2d {k}', per[k], w64, w32)
		assert abs(res[k] - float(per[k].mean())) < 1e-15


# ------------------------------------------------------------------ ModelWithLoss
def test_model_with_loss_mixes_the_structural_share():
	from find_amd import functional as FN
	from find_amd import synthetic
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	from find_amd.renderer import FootRenderer
	from find_amd.structures import Meshes, TexturesVertex
	from find_amd.train_utils import sample_latent_vectors
	n = 2
	v, f = synthetic.template(1002)
	opts = Opts(pix_loss=True, num_views=2)
	assert opts.pix_ssim_lambda == 0.
	mwl = ModelWithLoss(opts=opts, device='cpu', use_shapevec=True, use_texvec=True, use_posevec=True, train_size=n, val_size=1,
						shapevec_size=100, texvec_size=100, posevec_size=100, template_mesh_loc=None).to('cuda')
	mwl.model.set_template(v.cuda(), f.cuda())
	mwl.rdr = FootRenderer(image_size=32, device='cuda')
	lat = synthetic.latents(n, seed=3, device='cuda')
	with torch.no_grad():
		for k in ('shapevec', 'texvec', 'posevec', 'reg'):
			getattr(mwl.model, k).data.copy_(lat[k])
		gen = torch.Generator().manual_seed(1234)   # (a displacement head that carries gradient: synthetic.make_model)
		mwl.model.mlp_disp[-1].weight.copy_((torch.randn(mwl.model.mlp_disp[-1].weight.shape, generator=gen) * 0.01).cuda())
	gv, gf, gc = synthetic.gt_feet(n, 1002, seed=3, device='cuda')
	batch = dict(mesh=Meshes(gv, gf, TexturesVertex(gc.clamp(0.05, 0.95))), idx=torch.arange(n, device='cuda'), name=[f'{i:04d}' for i in range(n)])
	batch.update(sample_latent_vectors(batch, mwl.model.latent_vectors_train))
	flags = dict(pix=True, render_foot=True, return_renders=True)

	def parts(rdr, dtype=None):
		pi, gi, pm, gm = rdr['pred']['image'], rdr['gt']['image'], rdr['pred']['mask'], rdr['gt']['mask']
		if dtype is None:
			return pi, gi, pm, gm
		return tuple(t.detach().cpu().to(dtype).reshape((-1,) + tuple(t.shape[2:])) for t in (pi, gi, pm, gm))
	# lambda 0: the step of before, its MSE alone
	np.random.seed(5)
	_, losses0, rdr0 = mwl(batch, 0, opts, **flags)
	assert list(losses0) == ['loss_pix']
	assert torch.equal(losses0['loss_pix'], FN.image_mse(*parts(rdr0)) * opts.weight_pix)
	# lambda 0.2: 0.8 MSE + 0.2 (1 - SSIM) of the step's own renders
	o2 = Opts(pix_loss=True, num_views=2, pix_ssim_lambda=0.2)
	np.random.seed(5)
	mwl.zero_grad()
	_, losses2, rdr2 = mwl(batch, 0, o2, **flags)
	assert list(losses2) == ['loss_pix']
	want = {}
	for d in (torch.float64, torch.float32):
		pi, gi, pm, gm = parts(rdr2, d)
		mse = ((pi * pm[..., None] - gi * gm[..., None]) ** 2).mean()
		want[d] = 0.8 * mse + 0.2 * (1 - ssim_ref(pi, gi, pm, gm, border='same'))
	_held('loss_pix at lambda 0.2', losses2['loss_pix'] / o2.weight_pix, want[torch.float64], want[torch.float32])
	assert losses2['loss_pix'].item() > losses0['loss_pix'].item()
	losses2['loss_pix'].backward()
	torch.cuda.synchronize()
	grads = {k: q.grad for k, q in mwl.model.named_parameters() if q.grad is not None}
	assert grads and all(torch.isfinite(g).all() for g in grads.values())
	net = [k for k in grads if k.startswith('mlp_')]
	assert net and any(grads[k].abs().max().item() > 0 for k in net), sorted(grads)
	mwl.zero_grad()

	class Bare:   # a reference Opts has never heard of the option: the MSE alone
		pass
	bare = Bare()
	bare.__dict__.update({k: v for k, v in vars(opts).items() if k != 'pix_ssim_lambda'})
	np.random.seed(5)
	_, losses3, rdr3 = mwl(batch, 0, bare, **flags)
	assert torch.equal(losses3['loss_pix'], FN.image_mse(*parts(rdr3)) * opts.weight_pix)


# ------------------------------------------------------------------ poison
@contextlib.contextmanager
def poisoned_ssim(byte):
	"""tests/poison.py's proxy on find_amd.ssim: every torch.empty / torch.empty_like of the module comes back filled with `byte`."""
	from find_amd import ssim as mod
	if byte not in poison.PATTERNS:
		raise ValueError(byte)
	assert mod.torch is torch
	proxy = poison._TorchProxy(byte)
	try:
		mod.torch = proxy
		yield proxy
	finally:
		mod.torch = torch


def test_no_op_reads_or_leaves_unwritten_memory():
	from test_poison_host import allocating_ops
	from find_amd import ssim as mod
	x, y, xm, ym = _fields(2, 17, 33, 3, seed=21)
	ran = set()

	def run():
		out = {}
		for border in ('same', 'valid'):
			for masks in ('none', 'both'):
				got = _hip(x, y, *_pick(masks, xm, ym), border)
				for what, t in zip(('mean', 'per', 'd_x', 'd_xm'), got):
					out[f'{border} {masks} {what}'] = None if t is None else t.clone()
		ran.add('_SSIM')
		return out
	runs = []
	for byte in (None, 0xFF, 0x00):
		run()   # (what a forgotten region would hold: the right values of this call)
		with (poisoned_ssim(byte) if byte is not None else contextlib.nullcontext()) as proxy:
			runs.append(run())
			assert byte is None or proxy.calls >= 4 * 5
	assert mod.torch is torch
	bad = poison.compare('ssim', *runs)
	assert not bad, '\n'.join(bad)
	# under `valid` the border of d_x is written too, with the true values: the window of the counting pixel (5, 5) reaches (0, 0), and the
	# clean run was held to the reference above (test_ssim_against_float64[17x33x3])
	for tag, run_ in (('0xFF', runs[1]), ('0x00', runs[2])):
		d = run_['valid none d_x']
		assert torch.isfinite(d).all() and (d[:, 0, 0] != 0).any() and (d[:, -1, -1] != 0).any() and torch.equal(d, runs[0]['valid none d_x']), tag
	ops = allocating_ops(os.path.join(os.path.dirname(HERE), 'find_amd', 'ssim.py'))
	assert ops == ['_SSIM'] and set(ops) <= ran
