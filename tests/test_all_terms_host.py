"""A step with every loss term, on the host: the registry of ModelWithLoss fits functional.weighted_terms' bound, the bound is checked
before any device call, and forward() reports the terms in the registry's walk order (tests/test_gpu_all_terms.py runs the step)."""
import inspect

import pytest
import torch

TEN_KEYS = ['loss_chamf', 'loss_smooth', 'loss_tex', 'loss_cont_pose', 'loss_pix', 'loss_sil', 'loss_restyle_perc_cluster', 'loss_normal', 'loss_p2s',
			'loss_depth']
TEN_FLAGS = ['chamf', 'smooth', 'texture', 'cont_pose', 'pix', 'sil', 'restyle_perc_cluster', 'normal', 'p2s', 'depth']


def _registry():
	from find_amd import model_with_loss as MWL
	return MWL.ALL_TERMS + MWL.EVERY_EXTENSION_TERM


def test_the_registry_fits_the_bound_of_weighted_terms():
	from find_amd import functional as FN
	reg = _registry()
	assert FN.WEIGHTED_TERMS_MAX == 16
	assert len(reg) <= FN.WEIGHTED_TERMS_MAX, f'{len(reg)} loss terms, but one weighted_terms call takes {FN.WEIGHTED_TERMS_MAX}: raise TERMS_MAX (latent.hip)'
	assert [t.key for t in reg] == TEN_KEYS and [t.flag for t in reg] == TEN_FLAGS
	assert len({t.key for t in reg}) == len(reg) and len({t.weight for t in reg}) == len(reg)
	from find_amd.model_with_loss import ModelWithLoss
	params = inspect.signature(ModelWithLoss.forward).parameters
	for t in reg:
		assert t.flag in params and params[t.flag].default is False and callable(getattr(ModelWithLoss, t.fn)), t


def test_weighted_terms_checks_the_count_before_any_device_call():
	from find_amd import functional as FN
	z = torch.zeros(())   # a CPU tensor: a call that got past the count would raise RuntimeError (no fallback), not ValueError
	for n in (0, FN.WEIGHTED_TERMS_MAX + 1, 17):
		with pytest.raises(ValueError, match=r'1 \.\. 16 terms'):
			FN.weighted_terms([z] * n, [1.] * n)
	with pytest.raises(ValueError, match=r'1 \.\. 16 terms'):
		FN.weighted_terms([z] * 9, [1.] * 8)
	# 9 and 16 pass the count: what refuses them here is the device check behind it
	for n in (1, 8, 9, 16):
		with pytest.raises(Exception) as e:
			FN.weighted_terms([z] * n, [1.] * n)
		assert not isinstance(e.value, ValueError), (n, e.value)


def test_the_c_interface_states_the_new_bound():
	"""find_weighted_terms_* refuse 17 terms by their argument check (no launch, so no device is needed) and name the bound."""
	import ctypes
	from find_amd import _lib
	L = _lib.lib()
	one = ctypes.c_float(0.)
	p = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)   # never dereferenced: the count is refused first
	for n in (0, 17, -1):
		terms = (ctypes.c_void_p * 17)(*[p.value] * 17)
		w = (ctypes.c_float * 17)(*[1.] * 17)
		assert L.find_weighted_terms_fwd(n, terms, w, p, p, None) == -1, n
		assert '1 .. 16 terms' in L.find_last_error().decode()
		assert L.find_weighted_terms_bwd(n, w, p, p, p, None) == -1, n
		assert '1 .. 16 terms' in L.find_last_error().decode()


class _Opts:
	"""Weights 1, 2, 3, ... in registry order: the order of the weights handed to weighted_terms is then visible."""
	special_view_type = None
	num_views = 1

	def __init__(self):
		for i, t in enumerate(_registry()):
			setattr(self, t.weight, float(i + 1))


def _stub_step(monkeypatch, seen):
	"""A ModelWithLoss whose model, renders and raw terms are stand-ins (term i of the registry returns the CPU scalar 10 + i), and a
	weighted_terms that records what forward() hands it: what is left is forward()'s own walk."""
	from find_amd import model_with_loss as MWL
	mwl = MWL.ModelWithLoss.__new__(MWL.ModelWithLoss)
	torch.nn.Module.__init__(mwl)

	class _Model:
		def get_meshes_from_batch(self, batch, **kw):
			return {'cpv': None, 'meshes': None}

	class _Part:
		encoder = object()
	object.__setattr__(mwl, 'model', _Model())
	mwl.restyle_perc_loss = _Part()
	monkeypatch.setattr(MWL.ModelWithLoss, '_require_part_loss', staticmethod(lambda opts, enc: None))
	monkeypatch.setattr(MWL.ModelWithLoss, '_render_gt', lambda self, st, views, masked, images=True, **kw: ({}, None, None, None))
	monkeypatch.setattr(MWL.ModelWithLoss, '_render_pred', lambda self, st, gt, R, T, side, cmo, images=True, **kw: {})
	for i, t in enumerate(_registry()):
		monkeypatch.setattr(MWL.ModelWithLoss, t.fn, lambda self, st, i=i: torch.tensor(10. + i))

	def weighted(terms, weights):
		seen.append(([float(x) for x in terms], list(weights)))
		scaled = [x * w for x, w in zip(terms, weights)]
		return sum(scaled), scaled
	monkeypatch.setattr(MWL.FN, 'weighted_terms', weighted)
	batch = dict(posevec_train=torch.zeros(2, 4), pose_code=torch.zeros(2, 3), idx=torch.arange(2), name=['a', 'b'])
	return mwl, batch


def test_forward_reports_the_terms_in_the_registrys_walk_order(monkeypatch):
	seen = []
	mwl, batch = _stub_step(monkeypatch, seen)
	pairs = torch.zeros(1, 2, dtype=torch.int32)
	every = {f: True for f in TEN_FLAGS}
	loss, losses = mwl.forward(batch, 0, _Opts(), render_foot=True, cont_pairs=pairs, views=(None, None), **every)
	assert list(losses) == TEN_KEYS
	assert seen == [([10. + i for i in range(10)], [float(i + 1) for i in range(10)])]
	assert [float(losses[k]) for k in TEN_KEYS] == [(10. + i) * (i + 1) for i in range(10)]
	assert float(loss) == sum((10. + i) * (i + 1) for i in range(10))
	# whatever order the flags are given in, and with terms missing: still the registry's order
	del seen[:]
	some = dict(depth=True, p2s=True, sil=True, chamf=True, normal=True)
	_, losses = mwl.forward(batch, 0, _Opts(), render_foot=True, views=(None, None), **some)
	assert list(losses) == ['loss_chamf', 'loss_sil', 'loss_normal', 'loss_p2s', 'loss_depth']
	assert seen[0][1] == [1., 6., 8., 9., 10.]
	# without renders the render terms are left out, the others keep their places
	_, losses = mwl.forward(batch, 0, _Opts(), cont_pairs=pairs, **every)
	assert list(losses) == ['loss_chamf', 'loss_smooth', 'loss_tex', 'loss_cont_pose', 'loss_p2s']
