"""Host-side checks of the per-vertex feature render (no GPU needed): FootRenderer's argument validation, the C-ABI refusals of
find_render_features_fwd / _bwd (reached before any launch: the pointers are never dereferenced), and the gfx950 code of its kernels."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_meshes(n=2, v=5):
	from find_amd.structures import Meshes, TexturesVertex
	verts = torch.rand(n, v, 3)
	faces = torch.tensor([[0, 1, 2], [1, 2, 3], [2, 3, 4]], dtype=torch.int32)
	return Meshes(verts, faces, TexturesVertex(torch.rand(n, v, 3))), torch.eye(3)[None], torch.tensor([[0., 0., 0.3]])


def test_foot_renderer_validates_features():
	from find_amd.renderer import FootRenderer
	meshes, R, T = _cpu_meshes()
	r = FootRenderer(16, device='cpu')
	with pytest.raises(ValueError, match='needs features'):
		r(meshes, R, T, return_features=True)
	for bad in (torch.zeros(2, 5), torch.zeros(3, 5, 4), torch.zeros(2, 6, 4), torch.zeros(2, 5, 0), torch.zeros(2, 5, 4, dtype=torch.int32)):
		with pytest.raises(ValueError, match='features must be a float tensor'):
			r(meshes, R, T, return_features=True, features=bad)
	with pytest.raises(ValueError, match='ROCm device'):   # a CPU tensor (and a CPU mesh: there is no CPU fallback)
		r(meshes, R, T, return_features=True, features=torch.zeros(2, 5, 4))
	with pytest.raises(NotImplementedError, match='clip_faces'):
		FootRenderer(16, device='cpu', clip_faces=True)(meshes, R, T, return_features=True, features=torch.zeros(2, 5, 4))


def test_c_abi_refusals():
	from find_amd import _lib
	from find_amd import functional_render as FR
	L = _lib.lib()
	fake = ctypes.c_void_p(0x1000)

	def call(params, C=3, ws=fake):
		return L.find_render_features_fwd(ctypes.byref(params), fake, fake, 1, fake, fake, 1, 1, 8, 4, fake, C, fake, ws, 1 << 30, fake, 1 << 30, None)

	def call_bwd(params, C=3):
		return L.find_render_features_bwd(ctypes.byref(params), fake, fake, 1, fake, fake, 1, 1, 8, 4, fake, C, fake, fake, fake, fake, fake, 1 << 30,
										  fake, 1 << 30, None)
	p = FR.make_params(16)
	assert call(FR.make_params(16, clip_faces=True)) == -1 and b'clip_faces = 1' in L.find_last_error()
	assert call(p, C=0) == -1 and b'n_channels 0' in L.find_last_error()
	assert call_bwd(p, C=0) == -1 and b'n_channels 0' in L.find_last_error()
	# a workspace that no find_render_fwd with a mask filled
	assert call(p) == -1 and b'does not hold a find_render_fwd with a mask' in L.find_last_error()
	assert call_bwd(p) == -1 and b'does not hold a find_render_fwd with a mask' in L.find_last_error()
	assert call(p, ws=None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_render_features_ws_bytes(ctypes.byref(p), 2, 3, 0) == -1
	assert L.find_render_features_ws_bytes(ctypes.byref(p), 2, 3, 21) == 2 * 3 * 16 * 16 * 16


def test_feature_kernels_have_no_scratch_and_no_spills():
	hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
	if not os.path.exists(hipcc):
		pytest.skip('hipcc not available')
	csrc = os.path.join(ROOT, 'find_amd', 'csrc')
	with tempfile.TemporaryDirectory() as d:
		out = os.path.join(d, 'render.s')
		r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I' + os.path.join(ROOT, 'include'), '-I' + csrc, '-S',
							'--cuda-device-only', os.path.join(csrc, 'render.hip'), '-o', out], capture_output=True, text=True)
		assert r.returncode == 0, r.stderr[-2000:]
		asm = open(out).read()
	blocks = {m.group(1): m.group(2) for m in re.finditer(r'\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel', asm, re.S)}
	feat = {k: v for k, v in blocks.items() if 'feat_' in k}
	assert len(feat) == 11, sorted(feat)   # forward, prepass, 3 lane counts x 3 (geometry, features) variants of the backward
	for k, v in feat.items():
		assert int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', v).group(1)) == 0, k
		assert int(re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', v).group(1)) <= 256, k
	# no VGPR spills; the forward parks a dozen uniform values in VGPR lanes (SGPR spills: v_writelane / v_readlane, no memory)
	spills = re.findall(r'\.name:\s+(\S*feat_\S*)\s.*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)', asm, re.S)
	assert len(spills) == 11 and all(int(s) <= 16 and v == '0' for _, s, v in spills), spills
