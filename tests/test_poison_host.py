"""The poison harness (tests/poison.py) on the CPU: the allocations of the HIP path's wrappers come back filled, the comparison the GPU
cases use reports an op that leaves part of its output unwritten, and every allocating op of functional.py / functional_render.py is
named by a case of tests/test_gpu_poison.py."""
import ast
import os

import pytest
import torch

from poison import BITS, MODULES, Rule, atomic_bound, compare, poisoned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes(t):
	return t.contiguous().view(-1).view(torch.uint8) if t.numel() else torch.empty(0, dtype=torch.uint8)


@pytest.mark.parametrize('byte', [0xFF, 0x00])
def test_the_wrappers_allocations_come_back_filled(byte):
	from find_amd import functional as FN
	from find_amd import functional_render as FR
	from find_amd import optim, vis
	dev = torch.device('cpu')
	like = [torch.zeros(5, 7), torch.zeros(3), torch.zeros(0, 4)]
	with poisoned(byte) as proxy:
		assert all(m.torch is proxy for m in (FN, FR, optim, vis))
		got = [FN._ws(1000, dev), FN._ws(0, dev), FN._grad_for((0, 0), (4, 5, 3), dev), FN._grad_for((0, 0), (0, 3), dev), FN._grad_for((0, 0), (), dev)]
		got += FN._fill_rest([None, None, None], like)
		got += FN._grads_like(like)
		got += [FN.torch.empty(3, 2, dtype=torch.float64), FN.torch.empty((2, 2), dtype=torch.int32), FN.torch.empty_like(like[0]), FR.torch.empty(0), FN.torch.empty(7, dtype=torch.int64)]
		assert proxy.calls >= 10
		assert FN.torch.zeros is torch.zeros and FN.torch.float32 is torch.float32 and FN.torch.autograd is torch.autograd   # everything else is the real torch
	for m in (FN, FR, optim, vis):
		assert m.torch is torch
	assert got[0].numel() == 1000 and got[1].numel() == 256 and got[2].shape == (4, 5, 3) and got[3].numel() == 0 and got[4].dim() == 0
	for t in got:
		assert (_bytes(t) == byte).all(), (t.shape, t.dtype)
	if byte == 0xFF:   # NaN as a float, -1 as an index, ~0 as a key
		assert torch.isnan(got[2]).all() and (got[-4] == -1).all() and (got[-1] == -1).all()
	else:
		assert (got[2] == 0).all() and (got[-4] == 0).all() and (got[-1] == 0).all()
	# views of one flat allocation, as the MLP's gradients are carved
	a, b, c = FN._fill_rest([None, None, None], like)
	assert a._base is b._base and a.shape == (5, 7) and c.numel() == 0


def test_the_real_torch_is_back_after_an_exception_and_other_patterns_are_refused():
	from find_amd import functional as FN
	with pytest.raises(KeyError):
		with poisoned(0xFF):
			assert FN.torch is not torch
			raise KeyError('inside')
	import importlib
	for m in MODULES:
		assert importlib.import_module(m).torch is torch
	for byte in (0x7F, 0xAA, -1, 256):
		with pytest.raises(ValueError):
			with poisoned(byte):
				pass
	assert float(FN._ws(16, torch.device('cpu')).sum()) >= 0   # (plain uninitialised memory again: only that the call works)


# ------------------------------------------------------------------------------------------------ the harness can fail
class _HalfWritten(torch.autograd.Function):
	"""A toy op that allocates as the wrappers do and forgets the second half of its output -- and of its gradient."""

	@staticmethod
	def forward(ctx, x):
		from find_amd import functional as FN
		out = FN.torch.empty_like(x)
		h = x.numel() // 2
		out.view(-1)[:h] = 2 * x.detach().view(-1)[:h]
		return out

	@staticmethod
	def backward(ctx, g):
		from find_amd import functional as FN
		d = FN.torch.empty_like(g)
		h = g.numel() // 2
		d.view(-1)[:h] = 2 * g.view(-1)[:h]
		return d


class _Whole(torch.autograd.Function):
	@staticmethod
	def forward(ctx, x):
		from find_amd import functional as FN
		out = FN.torch.empty_like(x)
		out.copy_(2 * x.detach())
		return out

	@staticmethod
	def backward(ctx, g):
		from find_amd import functional as FN
		d = FN.torch.empty_like(g)
		d.copy_(2 * g)
		return d


def _three_runs(run):
	"""What test_gpu_poison.run_three does, without a device: a discarded clean call, then the run -- clean, under 0xFF, under 0x00."""
	import contextlib
	out = []
	for byte in (None, 0xFF, 0x00):
		run()
		with (poisoned(byte) if byte is not None else contextlib.nullcontext()):
			out.append(run())
	return out


def _toy(fn):
	x0 = torch.linspace(-1, 1, 24).reshape(4, 6)

	def run():
		x = x0.clone().requires_grad_(True)
		y = fn.apply(x)
		y.backward(torch.ones_like(y))
		return dict(out=y.detach().clone(), d_x=x.grad.clone())
	return run


def test_an_op_that_writes_half_of_its_output_is_reported():
	r0, r1, r2 = _three_runs(_toy(_HalfWritten))
	# the clean run may hold anything in the unwritten half (often the right values of the warm-up call: that is the point); make it finite
	r0 = {k: torch.nan_to_num(v) for k, v in r0.items()}
	bad = compare('toy', r0, r1, r2)
	assert any('toy/out [0xFF]' in b and 'not finite' in b for b in bad), bad
	assert any('toy/d_x [0xFF]' in b and 'not finite' in b for b in bad), bad
	assert any('12 of 24 entries are not finite (first at flat index 12)' in b for b in bad), bad
	# 0x00 reads as a plain wrong number: reported unless the stale value happened to be 0
	r0['out'].view(-1)[12:] = 5.0
	assert any('toy/out [0x00]' in b and 'differ from the clean run' in b for b in compare('toy', r0, r1, r2)), bad
	# and an op that writes everything passes the same routine
	assert compare('whole', *_three_runs(_toy(_Whole))) == []


def test_compare_rules():
	a = dict(x=torch.tensor([1.0, 2.0, 4.0]), i=torch.tensor([0, 3, -1], dtype=torch.int32), none=None)
	same = {k: (None if v is None else v.clone()) for k, v in a.items()}
	assert compare('c', a, same, same, dict(i=Rule(irange=(0, 4)))) == []
	# bit for bit means the last bit
	off = dict(same, x=a['x'] + torch.tensor([0.0, 2.0 ** -22, 0.0]))
	assert len(compare('c', a, off, same)) == 1 and compare('c', a, same, off)[0].startswith('c/x [0x00]: 1 of 3')
	# a summation-order bound per entry, a relative and an absolute one
	assert compare('c', a, off, off, dict(x=Rule(bits=False, bound=torch.tensor([0.0, 3e-7, 0.0])))) == []
	assert len(compare('c', a, off, off, dict(x=Rule(bits=False, bound=torch.tensor([0.0, 2e-7, 0.0]))))) == 2
	assert compare('c', a, off, off, dict(x=Rule(bits=False, rel=1e-7))) == [] and len(compare('c', a, off, same, dict(x=Rule(bits=False, rel=1e-8)))) == 1
	assert compare('c', a, off, off, dict(x=Rule(bits=False, abs=3e-7))) == [] and len(compare('c', a, off, same, dict(x=Rule(bits=False, abs=1e-7)))) == 1
	# integers outside their op's range, a missing output, another shape
	wild = dict(same, i=torch.tensor([0, 4, -1], dtype=torch.int32))
	assert any('outside -1 / [0, 4)' in b for b in compare('c', a, wild, same, dict(i=Rule(irange=(0, 4)))))
	assert any('missing' in b for b in compare('c', a, dict(same, x=None), same))
	assert any('unexpected' in b for b in compare('c', a, dict(same, none=torch.zeros(1)), same))
	assert any('instead of' in b for b in compare('c', a, dict(same, x=torch.zeros(2)), same))
	with pytest.raises(ValueError):
		Rule(bits=False)
	assert BITS.bits
	# (n_row + 3) * 2^-24 * sum |addend|
	assert atomic_bound(torch.tensor([0.0, 5.0]), torch.tensor([2.0, 2.0])).tolist() == [3 * 2.0 ** -24 * 2, 8 * 2.0 ** -24 * 2]


# ------------------------------------------------------------------------------------------------ census
def _allocates(node):
	for n in ast.walk(node):
		if isinstance(n, ast.Call):
			f = n.func
			if isinstance(f, ast.Attribute) and f.attr in ('empty', 'empty_like') and isinstance(f.value, ast.Name) and f.value.id == 'torch':
				return True
			if isinstance(f, ast.Name) and f.id == '_ws':
				return True
	return False


def allocating_ops(path):
	"""Names of the autograd.Function classes and module-level functions of a wrapper module whose body calls torch.empty,
	torch.empty_like or _ws."""
	with open(path) as fh:
		tree = ast.parse(fh.read())
	names = []
	for node in tree.body:
		if isinstance(node, ast.FunctionDef) and _allocates(node):
			names.append(node.name)
		elif isinstance(node, ast.ClassDef) and _allocates(node):
			is_function = any(isinstance(b, ast.Attribute) and b.attr == 'Function' for b in node.bases)
			assert is_function or node.name in ('SGD', 'Adam'), f'{node.name}: an allocating class that is no autograd.Function'
			names.append(node.name)
	return names


def test_every_allocating_op_has_a_poison_case():
	import test_gpu_poison as T
	covered = set()
	for c in T.CASES:
		assert c.covers and c.kind in ('bits', 'atomics') and c.ref, c.name
		covered.update(c.covers)
	assert len({c.name for c in T.CASES}) == len(T.CASES)
	ops = []
	for mod, at_least in (('functional.py', 25), ('functional_render.py', 6), ('vis.py', 1), ('optim.py', 1)):
		found = allocating_ops(os.path.join(ROOT, 'find_amd', mod))
		assert len(found) >= at_least, (mod, found)
		ops += found
	for name in ('_ws', '_grad_for', '_fill_rest', '_MLP', '_NN', '_Chamfer', '_SurfaceChamfer', '_PointFace', '_DepthMap', 'face_areas', '_Render', '_RenderFeatures',
				 'render_points', 'render_uv', 'render_frags', 'uv_sample'):
		assert name in ops, f'the census no longer finds {name}'
	missing = sorted(set(ops) - covered)
	assert not missing, f'allocating ops without a case in tests/test_gpu_poison.py: {missing}'
	# the census itself can fail: an op added later without a case
	src = 'import torch\nclass _New(torch.autograd.Function):\n\t@staticmethod\n\tdef forward(ctx, x):\n\t\treturn torch.empty_like(x)\ndef helper(x):\n\treturn x\ndef fresh(n):\n\treturn _ws(n, None)\n'
	import tempfile
	with tempfile.NamedTemporaryFile('w', suffix='.py', delete=False) as fh:
		fh.write(src)
	try:
		assert allocating_ops(fh.name) == ['_New', 'fresh'] and not {'_New', 'fresh'} & covered
	finally:
		os.unlink(fh.name)
