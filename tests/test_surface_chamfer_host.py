"""The fused Chamfer backward without a GPU: the entry points are declared and bound with matching argument counts, the size function
answers before any HIP call, the argument checks come before any launch, and the Python side has its switch and its signatures."""
import inspect
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SYMBOLS = ('find_chamfer_surface_bwd_ws_bytes', 'find_chamfer_surface_bwd')


def test_header_and_binding_declare_the_entry_points():
	from find_amd import _lib
	hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'find_hip.h')).read(), flags=re.S)
	for name in SYMBOLS:
		assert re.search(r'\b' + name + r'\s*\(', hdr), name
		assert name in _lib.PROTOTYPES, name
	assert _lib.ABI_VERSION == 3 and '#define FIND_ABI_VERSION 3' in hdr
	n_args = {name: len(re.search(name + r'\s*\((.*?)\)', hdr, flags=re.S).group(1).split(',')) for name in SYMBOLS}
	assert n_args == {name: len(_lib.PROTOTYPES[name][1]) for name in SYMBOLS} == {SYMBOLS[0]: 3, SYMBOLS[1]: 19}


def test_size_function_and_argument_checks_need_no_gpu():
	from find_amd import _lib
	L = _lib.lib()
	size = L.find_chamfer_surface_bwd_ws_bytes
	assert size(16, 6890, 5000) >= 16 * 8 * 6890 * 12      # the training step: eight slices per foot, a slab each
	assert size(1, 6890, 5000) >= 8 * 6890 * 12 and size(1, 6890, 1024) == 0   # (a cloud of one round of threads is not cut)
	assert size(0, 6890, 5000) == -1 and size(1, 0, 5000) == -1 and size(1, 6890, 0) == -1
	# the image of one foot has to fit a workgroup's 160 KiB of LDS
	fits = [v for v in (13000, 13600, 13650, 13651, 13652, 13653, 13654, 14000, 20000) if size(2, v, 64) >= 0]
	assert fits and all(v * 12 <= 160 * 1024 for v in fits) and 13000 in fits and 14000 not in fits
	try:
		# a forced slice count sizes the slabs
		assert L.find_render_switches(2 << 16) == 0 and size(16, 6890, 5000) >= 16 * 2 * 6890 * 12
		assert L.find_render_switches(1 << 16) == 0 and size(1, 6890, 5000) == 0
	finally:
		assert L.find_render_switches(0) == 0
	assert L.find_render_switches(8 << 16) == -1           # (past the field)
	# argument checks come before any launch
	args = [None, None, None, 1, 8, 8, None, None, 0, None, 1, None, None, 4, 4, None, None, 0, None]
	assert L.find_chamfer_surface_bwd(*args) == -1 and b'NULL' in L.find_last_error()


def test_python_side_switch_and_signatures():
	from find_amd import functional, losses
	assert losses.FUSED_CHAMFER_BWD == int(os.environ.get('FIND_FUSED_CHAMFER_BWD', '1'))
	# the size rule: the training step's 16 x 5000 samples take the fused backward, one foot's 5000 keep the two passes
	assert functional.surface_chamfer_pays(16, 5000) and functional.surface_chamfer_pays(4, 5000)
	assert not functional.surface_chamfer_pays(1, 5000) and not functional.surface_chamfer_pays(2, 5000)
	assert list(inspect.signature(functional.surface_chamfer).parameters) == ['verts', 'faces', 'rnd', 'y', 'y_len']
	assert inspect.signature(functional.surface_chamfer).parameters['y_len'].default is None
	assert list(inspect.signature(functional.surface_chamfer_distance).parameters) == ['samples', 'y', 'y_len'] and functional.surface_of(torch.zeros(1, 4, 3)) is None
	with pytest.raises(RuntimeError, match='not the direct output'):
		functional.surface_chamfer_distance(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
	assert functional.surface_chamfer_fits(16, 6890, 5000) and not functional.surface_chamfer_fits(16, 20000, 5000)
	with pytest.raises(RuntimeError, match='do not fit'):
		functional.surface_chamfer(torch.zeros(1, 20000, 3), torch.tensor([[0, 1, 2]]), torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		functional.surface_chamfer(torch.zeros(1, 3, 3), torch.tensor([[0, 1, 2]]), torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
