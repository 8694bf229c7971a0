"""FIND model API on the MI355X hot path.

Host-side mirror of reference src/model/model.py: same class names, constructor keywords, state_dict keys,
parameter groups and forward()/get_meshes()/get_meshes_from_batch() signatures, so src/train and src/eval call it
unchanged.  All arithmetic runs in libfind_hip.so (find_amd.functional); nothing here computes the
network on the CPU."""
import os

import numpy as np
import torch

from . import functional as FN
from .structures import LazyTexturesVertex, Meshes, TexturesVertex, extend_template

nn = torch.nn


def make_params_list(*params):
	"""Flatten modules / parameters / None into a list of parameters (reference model.py:47-60)."""
	out = []
	for prm in params:
		if prm is None:
			continue
		if isinstance(prm, nn.Parameter):
			out.append(prm)
		elif hasattr(prm, 'parameters'):
			out.extend(prm.parameters())
		else:
			raise ValueError(f'Param type {type(prm)} not understood.')
	return out


class FourierFeatureTransform(nn.Module):
	"""Holder of the Gaussian Fourier matrix B (reference src/utils/fourier_feature_transform.py:17-26).

	Quirks kept on purpose: construction reseeds the *global* torch RNG to 1 (so every later nn.Linear init is
	deterministic), the `num_input_channels` ROWS of B are sorted by L2 norm, and `_B` is a plain attribute --
	not a buffer, not in the state_dict.  The encoding itself is fused into the first GEMM of the HIP MLP kernel
	(csrc/mlp_kernels.h: pe_value), so this module has no forward of its own."""

	def __init__(self, num_input_channels, mapping_size=256, scale=10, exclude=0):
		super().__init__()
		self._num_input_channels = num_input_channels
		self._mapping_size = mapping_size
		self.exclude = exclude
		torch.manual_seed(1)
		B = torch.randn((num_input_channels, mapping_size)) * scale
		order = sorted(range(num_input_channels), key=lambda i: float(torch.norm(B[i], p=2)))
		self._B = torch.stack([B[i] for i in order])
		self._B_dev = {}

	def B(self, device):
		device = torch.device(device)
		t = self._B_dev.get(device)
		if t is None:
			t = self._B.to(device=device, dtype=torch.float32).contiguous()
			self._B_dev[device] = t
		return t

	def forward(self, x):
		raise NotImplementedError('FourierFeatureTransform is fused into find_amd.functional.mlp (HIP); call the model instead')


class LatentVector(nn.Module):
	"""Table of learned per-item vectors addressed by int / tensor / label / list (reference model.py:92-152)."""

	def __init__(self, dataset_size=None, vec_size=512, name='', device='cuda', key=None, labels: list = None, init_values=None):
		super().__init__()
		self.dataset_size = dataset_size
		self.vec_size = vec_size
		if labels is not None:
			dataset_size = len(labels)
		self.labels = labels
		self.key = key
		init = torch.zeros(dataset_size, vec_size)
		if init_values is not None:
			if not isinstance(init_values, np.ndarray):
				raise NotImplementedError
			init[:] = torch.from_numpy(init_values).unsqueeze(0).float()
		self.data = nn.Parameter(init.to(device))
		self.name = name
		self._label_cache = {}

	def __len__(self):
		return self.dataset_size

	def _index_of(self, label):
		assert self.labels is not None, f'Tried to access item {label} from LatentVector {self.name}, LV does not have labels'
		return self.labels.index(label)

	def _rows(self, idx):
		"""self.data[idx] for an integer index tensor; on the GPU through the gather kernel (deterministic scatter backward)."""
		if self.data.is_cuda and self.data.dtype == torch.float32 and idx.dim() == 1:
			if not idx.is_cuda and idx.numel() > 0:   # a host index can be checked for free; torch raises IndexError here as well
				lo, hi = int(idx.min()), int(idx.max())
				if lo < -self.data.shape[0] or hi >= self.data.shape[0]:
					raise IndexError(f'LatentVector {self.name}: index {lo if lo < -self.data.shape[0] else hi} is out of range for {self.data.shape[0]} rows')
			# (a device index is not read back: the gather kernel answers an out-of-range row with NaNs instead of a host synchronisation)
			return FN.latent_gather(self.data, idx.to(device=self.data.device, dtype=torch.int64))
		# a table that lives on the host (a model being built or inspected on the CPU: tests/test_host_api.py, checkpoint tools) or an index of
		# another shape: plain indexing.  Not a compute fall-back -- every kernel-backed op downstream (FN.mlp, register_points, the losses)
		# raises on CPU tensors, so a training step cannot run through here by accident.
		return self.data[idx]

	def _label_rows(self, labels):
		"""Rows for a list of label strings.  The label -> row search is the reference's host-side list.index; the resulting index
		tensor is kept per label tuple (device_index), so a batch seen before costs no host-to-device copy (a DataLoader revisits the
		same scans every epoch)."""
		idx = self.device_index(labels)
		if idx is None:   # CPU table
			idx = torch.tensor([self._index_of(o) for o in labels], dtype=torch.int64, device=self.data.device)
		return self._rows(idx)

	def device_index(self, sel):
		"""The int64 device index vector that self[sel] would gather with on the GPU path -- sel a 1-D integer tensor or a list of label
		strings -- or None when self[sel] takes another route (CPU table, scalar index, list of ints ...).  Same checks as __getitem__."""
		if not (self.data.is_cuda and self.data.dtype == torch.float32):
			return None
		if isinstance(sel, torch.Tensor) and sel.dim() == 1 and sel.dtype in (torch.int64, torch.int32):
			if not sel.is_cuda and sel.numel() > 0:
				lo, hi = int(sel.min()), int(sel.max())
				if lo < -self.data.shape[0] or hi >= self.data.shape[0]:
					raise IndexError(f'LatentVector {self.name}: index {lo if lo < -self.data.shape[0] else hi} is out of range for {self.data.shape[0]} rows')
			return sel.to(device=self.data.device, dtype=torch.int64)
		if isinstance(sel, list) and sel and isinstance(sel[0], str):
			key = tuple(sel)
			idx = self._label_cache.get(key)
			if idx is None or idx.device != self.data.device:
				if len(self._label_cache) > 4096:
					self._label_cache.clear()
				idx = torch.tensor([self._index_of(o) for o in sel], dtype=torch.int64, device=self.data.device)
				self._label_cache[key] = idx
			return idx
		return None

	def __getitem__(self, idx):
		if isinstance(idx, torch.Tensor) and idx.dim() == 1 and idx.dtype in (torch.int64, torch.int32):
			return self._rows(idx)
		if isinstance(idx, (int, torch.Tensor)):
			return self.data[idx]
		if isinstance(idx, str):
			return self.data[self._index_of(idx)]
		if isinstance(idx, list):
			if isinstance(idx[0], int):
				return self.data[idx]
			if isinstance(idx[0], str):
				return self._label_rows(idx)
			return None  # the reference falls through here as well (model.py:142-149)
		raise NotImplementedError(f"Didn't understand indexing of LatentVector {self.name}, type {type(idx)}")


class Model(nn.Module):
	"""save / load / freeze (reference model.py:155-196); checkpoints are {'state_dict', 'params'} dicts."""

	def save_model(self, out_dir='models/tmp', fname='model_tmp'):
		os.makedirs(out_dir, exist_ok=True)
		torch.save({'state_dict': self.state_dict(), 'params': self.params}, os.path.join(out_dir, fname + '.pth'))

	def freeze(self):
		for prm in self.parameters():
			prm.requires_grad = False

	@classmethod
	def load(cls, file, device='cuda', opts=None, **kwargs):
		ext = os.path.splitext(file)[-1]
		assert ext == '.pth', f'Generic models can only load from .pth files - received `{ext}` file.'
		data = torch.load(file, map_location=device, weights_only=False)
		skip_latents = opts is not None and getattr(opts, 'dont_load_latents', False)
		if skip_latents:
			data['params']['train_size'] = kwargs.get('train_size', 1)
			data['params']['val_size'] = kwargs.get('val_size', 1)
			data['params']['latent_labels'] = kwargs.get('latent_labels', None)
		state_dict = data['state_dict']
		model = cls(**data['params'], device=device, opts=opts)
		model.configure_template(state_dict, device=device)
		if skip_latents:
			latent_keys = {f + '.data' for f in ['shapevec', 'shapevec_val', 'texvec', 'texvec_val', 'posevec', 'posevec_val', 'reg', 'reg_val']}
			state_dict = {k: v for k, v in state_dict.items() if k not in latent_keys}
		model.load_state_dict(state_dict, strict=False)
		return model


def _template_texture_image(obj_path):
	"""The image behind the template OBJ's first material (`mtllib` -> `newmtl` -> `map_Kd`), as (H, W, 3) float32 in [0, 1] -- what
	pytorch3d.io.load_obj returns as props.texture_images['material_0'] in the reference (model.py:268) -- or None when there is none."""
	folder = os.path.dirname(obj_path)
	mtl = None
	with open(obj_path, 'r') as fh:
		for line in fh:
			if line.startswith('mtllib '):
				mtl = os.path.join(folder, line.split(None, 1)[1].strip())
				break
	if mtl is None or not os.path.isfile(mtl):
		return None
	with open(mtl, 'r') as fh:
		for line in fh:
			if line.strip().startswith('map_Kd'):
				img = os.path.join(folder, line.split(None, 1)[1].strip())
				if os.path.isfile(img):
					from .dataset import load_texture_png
					return load_texture_png(img)
				return None
	return None


def _average_template_colour(verts, faces, faces_uvs, verts_uvs, image, num_samples=1000):
	"""Mean colour of `num_samples` surface samples of the UV-textured template (reference model.py:266-277: sample_points_from_meshes(mesh,
	1000, return_textures=True).mean).  One-off set-up arithmetic at construction, in plain torch on the tensors' device, drawing from that
	device's default generator in PyTorch3D's order (faces ~ multinomial(area), then rand(2, 1, S) for the barycentrics)."""
	v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
	areas = 0.5 * torch.linalg.cross(v1 - v0, v2 - v0).norm(dim=1)
	fi = areas.multinomial(num_samples, replacement=True)
	uv = torch.rand(2, 1, num_samples, dtype=verts.dtype, device=verts.device)
	su = uv[0, 0].sqrt()
	w = torch.stack([1.0 - su, su * (1.0 - uv[1, 0]), su * uv[1, 0]], dim=1)               # (S, 3) barycentrics
	tri_uv = verts_uvs[faces_uvs[fi]]                                                        # (S, 3, 2)
	p = (w[:, :, None] * tri_uv).sum(dim=1)                                                  # (S, 2) texture coordinates
	grid = (p * 2.0 - 1.0).view(1, 1, num_samples, 2)
	tex = torch.flip(image, [0]).permute(2, 0, 1)[None]                                      # TexturesUV: v = 0 is the bottom row
	cols = torch.nn.functional.grid_sample(tex, grid, mode='bilinear', align_corners=True, padding_mode='border')
	return cols[0, :, 0, :].mean(dim=1)


class _Once:
	"""A value computed on the first call and kept.  The deferred colour head is ONE such cell shared by the result dict and by the meshes'
	textures: neither refers to the other, so nothing of a step -- its autograd graph and the gigabyte of activations saved in it -- waits
	in a reference cycle for the cyclic garbage collector (the first version's textures closed over the dict that holds the meshes: the
	allocator grew by a step's memory per step and the headline loop slowed from 2.2 to 3.9 ms within a hundred steps)."""

	def __init__(self, fn):
		self.fn, self.value = fn, None

	def __call__(self):
		if self.fn is not None:
			self.value = self.fn()
			self.fn = None
		return self.value


class _LazyColours(dict):
	"""get_meshes' result when the colour head is deferred: res['col'] runs the head on first access (and keeps the value)."""

	def __init__(self, res, cell):
		super().__init__(res)
		self._cell = cell

	def __missing__(self, key):
		if key != 'col' or self._cell is None:
			raise KeyError(key)
		self['col'] = self._cell()
		self._cell = None
		return dict.__getitem__(self, 'col')


def load_template_classes(file, device='cuda'):
	"""Per-vertex template classes (V, C) of a pretrained checkpoint: its state_dict['features'] (reference model.py:199-203)."""
	return torch.load(file, map_location=device, weights_only=False)['state_dict']['features'].float()


class NeuralDisplacementField(Model):
	"""Template mesh + Fourier PE + trunk MLP + displacement / colour heads + per-instance latent tables
	(reference model.py:206-534)."""

	def __init__(self, sigma=10, depth=4, width=256, encoding='gaussian', dispdepth=3, coldepth=3, normratio=0.1,
				 clamp=None, normclamp=None, niter=6000, input_dim=3, positional_encoding=True, progressive_encoding=False,
				 exclude=0,
				 use_shapevec=False, train_size=None, val_size=None, shapevec_size=256,
				 use_texvec=False, texvec_size=256, use_posevec=False, posevec_size=256,
				 template_mesh_loc=None, device='cuda',
				 restyle_features_per_vertex=False, restyle_cluster_per_vertex=False,
				 use_avg_colour=False, opts=None,
				 latent_labels: dict = None):
		super().__init__()
		self.params = dict(sigma=sigma, depth=depth, width=width, encoding=encoding, dispdepth=dispdepth, coldepth=coldepth,
						   progressive_encoding=progressive_encoding, positional_encoding=positional_encoding,
						   train_size=train_size, val_size=val_size,
						   use_shapevec=use_shapevec, shapevec_size=shapevec_size, use_texvec=use_texvec,
						   texvec_size=texvec_size, use_posevec=use_posevec, posevec_size=posevec_size,
						   restyle_features_per_vertex=restyle_features_per_vertex,
						   restyle_cluster_per_vertex=restyle_cluster_per_vertex,
						   use_avg_colour=use_avg_colour, latent_labels=latent_labels)
		if progressive_encoding:
			raise NotImplementedError('progressive_encoding is flagged untested in the reference (opts.py:49-50) and is out of scope')
		if restyle_features_per_vertex:
			# (restyle_cluster_per_vertex is only stored, as upstream: ModelWithLoss reads opts.restyle_cluster_per_vertex and res['cpv'])
			raise NotImplementedError("restyle_features_per_vertex is out of scope: upstream never produces the res['fpv'] it would render (model.py:1081)")
		if width != 256 or input_dim != 3:
			raise NotImplementedError('the HIP kernels are specialised for width=256, input_dim=3 (the reference setting, model.py:207)')
		self.clamp, self.normclamp, self.normratio = clamp, normclamp, normratio
		self.width, self.input_dim = width, input_dim

		# --- construction order matters: FFT reseeds the global RNG, then Linear layers draw from it in this order
		enc = []
		use_pe = (encoding == 'gaussian') and positional_encoding
		if use_pe:
			enc.append(FourierFeatureTransform(input_dim, width, sigma, exclude))
		input_size = width * 2 + input_dim if use_pe else input_dim
		layers = [nn.Linear(input_size, width), nn.ReLU()]
		for _ in range(depth):
			layers += [nn.Linear(width, width), nn.ReLU()]
		self.encoder = nn.ModuleList(enc)
		self.base = nn.ModuleList(layers)

		# --- template (centred at its centroid, model.py:274-275)
		if template_mesh_loc is not None:
			from .dataset import load_obj
			verts, face_dict, props = load_obj(template_mesh_loc)
			faces = face_dict.verts_idx
			image = _template_texture_image(template_mesh_loc)
			if image is not None and props.verts_uvs.numel() > 0 and bool((face_dict.textures_idx >= 0).all()):
				dev = torch.device(device)
				avg_col = _average_template_colour(verts.to(dev), faces.to(dev), face_dict.textures_idx.to(dev), props.verts_uvs.to(dev), image.to(dev)).cpu()
			elif use_avg_colour:
				raise NotImplementedError('use_avg_colour=True needs the template\'s UV texture (OBJ with vt coordinates + mtllib / map_Kd image): the reference '
										  'averages 1000 surface samples of it (model.py:266-277); a checkpoint that carries avg_col restores it without one')
			else:
				avg_col = torch.zeros(3)
			verts = verts - verts.mean(dim=0)
		else:
			verts = torch.zeros((1, 3), dtype=torch.float32)
			faces = torch.ones((1, 3), dtype=torch.int)
			avg_col = torch.zeros(3, dtype=torch.float32)
		self.template_verts = nn.Parameter(verts.unsqueeze(0).float().to(device), requires_grad=False)
		self.template_faces = nn.Parameter(faces.unsqueeze(0).to(device), requires_grad=False)
		self.avg_col = nn.Parameter(avg_col.to(device), requires_grad=False)
		self._rebuild_template_mesh()

		# --- latent tables (model.py:299-348).  NB posevec tables are sized with shapevec_size (model.py:320-322).
		self.latent_vectors_train, self.latent_vectors_val = [], []
		ll = latent_labels or {}

		def table(n, size, name, key, lab, **kw):
			return LatentVector(n, vec_size=size, name=name, key=key, labels=ll.get(lab, None), device=device, **kw)

		self.shapevec_size, self.use_shapevec = shapevec_size, use_shapevec
		self.shapevec = self.shapevec_val = None
		if use_shapevec:
			self.shapevec = table(train_size, shapevec_size, 'shapevec_train', 'shape', 'shape')
			self.shapevec_val = table(val_size, shapevec_size, 'shapevec_val', 'shape', 'shape_val')
			self.latent_vectors_train.append(self.shapevec)
			self.latent_vectors_val.append(self.shapevec_val)
		self.posevec_size, self.use_posevec = posevec_size, use_posevec
		self.posevec = self.posevec_val = None
		if use_posevec:
			self.posevec = table(train_size, shapevec_size, 'posevec_train', 'pose', 'pose')
			self.posevec_val = table(val_size, shapevec_size, 'posevec_val', 'pose', 'pose_val')
			self.latent_vectors_train.append(self.posevec)
			self.latent_vectors_val.append(self.posevec_val)
		self.texvec_size, self.use_texvec = texvec_size, use_texvec
		self.texvec = self.texvec_val = None
		if use_texvec:
			self.texvec = table(train_size, texvec_size, 'texvec_train', 'tex', 'tex')
			self.texvec_val = table(val_size, texvec_size, 'texvec_val', 'tex', 'tex_val')
			self.latent_vectors_train.append(self.texvec)
			self.latent_vectors_val.append(self.texvec_val)
		ident = np.array([0] * 6 + [1] * 3)
		self.reg = table(train_size, 9, 'reg_train', 'reg', 'reg', init_values=ident)
		self.reg_val = table(val_size, 9, 'reg_val', 'reg', 'reg_val', init_values=ident)
		self.latent_vectors_train.append(self.reg)
		self.latent_vectors_val.append(self.reg_val)

		# --- heads.  The disp-head input counts the shape code only if use_texvec (reference quirk, model.py:352).
		self._lat_disp = self.shapevec_size * self.use_texvec + self.posevec_size * self.use_posevec
		self._lat_col = self.texvec_size * self.use_texvec
		disp_layers = []
		for i in range(dispdepth):
			disp_layers += [nn.Linear(width + self._lat_disp if i == 0 else width, width), nn.ReLU()]
		disp_layers.append(nn.Linear(width, 3))
		self.mlp_disp = nn.Sequential(*disp_layers)
		col_layers = []
		for i in range(coldepth):
			col_layers += [nn.Linear(width + self._lat_col if i == 0 else width, width), nn.ReLU()]
		self.use_avg_colour = use_avg_colour
		col_layers.append(nn.Linear(width, 3))
		self.mlp_col = nn.Sequential(*col_layers)

		self.restyle_features_per_vertex = restyle_features_per_vertex
		self.per_vertex_features = None
		if opts is not None and getattr(opts, 'template_features_pth', None) is not None:
			# per-vertex class logits of the template (model.py:199-203, 377-381): a Parameter in no parameter group, as upstream
			self.per_vertex_features = nn.Parameter(load_template_classes(opts.template_features_pth, device=device).unsqueeze(0))
			if template_mesh_loc is not None:
				self._check_per_vertex_features()

		# --- parameter groups read by train.py:161-168
		self.main_params = make_params_list(self.base, self.mlp_disp, self.mlp_col, self.shapevec, self.texvec, self.posevec)
		self.templ_params = make_params_list(self.template_verts, self.reg)
		self.val_params = make_params_list(self.shapevec_val, self.texvec_val, self.posevec_val)
		self.reg_params = make_params_list(self.reg, self.reg_val)
		self.latent_params = make_params_list(self.shapevec, self.shapevec_val, self.texvec, self.texvec_val, self.posevec, self.posevec_val)

		if dispdepth < 1 or coldepth < 1:
			raise NotImplementedError('dispdepth/coldepth must be >= 1')
		self._spec = FN.MLPSpec(n_trunk=depth + 1, n_disp=dispdepth, n_col=coldepth, pe_size=width if use_pe else 0,
								lat_disp=self._lat_disp, lat_col=self._lat_col, in_dim=input_dim, width=width)
		self.reset_weights()
		self.onnx_mode = False

	# ------------------------------------------------------------------ helpers
	def set_mlp_precision(self, precision):
		"""Arithmetic of THIS model's 256 -> 256 layers: 'fp32', 'fp16' (opt-in, find_amd.functional.set_mlp_precision for what it
		means) or None = follow the process default.  Two models in one process may differ."""
		if precision not in (None, 'fp32', 'fp16', 'bf16x3'):
			raise ValueError(f"set_mlp_precision: None, 'fp32', 'bf16x3' or 'fp16', got {precision!r}")
		self._spec.precision = precision

	def _check_per_vertex_features(self):
		f = self.per_vertex_features
		if f is not None and (f.dim() != 3 or f.shape[1] != self.template_verts.shape[1]):
			raise ValueError(f'template_features_pth holds per-vertex features of shape {tuple(f.shape[1:])}, the template has '
							 f'{self.template_verts.shape[1]} vertices: (V, C) with the template\'s V expected')

	def _rebuild_template_mesh(self):
		self.template_mesh = Meshes(verts=self.template_verts.data, faces=self.template_faces.data[0])

	def _weights(self):
		"""The MLP's Parameter objects in kernel order.  Collected once (walking the three Sequentials cost 25 us per call -- twice per step
		at batch 1, where the step is bound by the host) and VALIDATED on every call by identity: each cached (container, layer, weight, bias)
		must still be what the module tree holds, so a replaced Parameter (`load_state_dict(assign=True)`, `layer.weight = nn.Parameter(...)`,
		torch.__future__.set_overwrite_module_params_on_conversion), a replaced layer or a replaced Sequential rebuilds the list instead of
		feeding the kernels tensors the optimiser no longer holds."""
		c = self.__dict__.get('_wlist')
		if c is not None:
			ws, checks, seqs = c
			mods = self._modules
			ok = mods['base'] is seqs[0] and mods['mlp_disp'] is seqs[1] and mods['mlp_col'] is seqs[2]
			if ok:
				for i, (md, key, layer, pd) in enumerate(checks):
					if md.get(key) is not layer or pd.get('weight') is not ws[2 * i] or pd.get('bias') is not ws[2 * i + 1]:
						ok = False
						break
				ok = ok and sum(len(q) for q in seqs) == self.__dict__['_wcount']
			if ok:
				return ws
		ws, checks = [], []
		seqs = (self.base, self.mlp_disp, self.mlp_col)
		for seq in seqs:
			for key, layer in seq._modules.items():
				if isinstance(layer, nn.Linear):
					ws += [layer.weight, layer.bias]
					checks.append((seq._modules, key, layer, layer._parameters))
		self.__dict__['_wlist'] = (ws, checks, seqs)
		self.__dict__['_wcount'] = sum(len(q) for q in seqs)
		return ws

	def _apply(self, fn, *args, **kwargs):
		# (one override: drops the cached weight list -- conversions may replace Parameter objects -- AND re-points the template mesh at the
		# converted template tensors; round 4 had two definitions of this method and the second silently replaced the first)
		self.__dict__.pop('_wlist', None)
		out = super()._apply(fn, *args, **kwargs)
		self._rebuild_template_mesh()
		return out

	@staticmethod
	def _cat_latents(*vecs):
		vecs = [v for v in vecs if v is not None]
		if not vecs:
			return None
		return vecs[0] if len(vecs) == 1 else torch.cat(vecs, dim=-1)

	# ------------------------------------------------------------------ reference API
	def forward(self, pos, shapevec=None, texvec=None, posevec=None, want=('disp', 'col'), defer_wgrad_join=False):
		"""pos [B|1, V, 3]; shapevec/texvec/posevec [B, L] -> dict(disp [B,V,3], col [B,V,3])   (model.py:393-453).
		A batch-1 `pos` with batched latents is evaluated once through the trunk and shared by every foot.
		`want` (not in the reference, which always evaluates both heads): the heads to evaluate -- the texture loss reads 'col' only;
		defer_wgrad_join: see find_amd.functional.mlp."""
		if self.onnx_mode:
			raise NotImplementedError('onnx_mode (web export) is out of scope')
		if pos.dim() != 3 or pos.shape[-1] != self.input_dim:
			raise ValueError(f'pos must be [B, V, {self.input_dim}], got {tuple(pos.shape)}')
		# (a head `want` leaves out reads no latents: its concatenation -- a launch on the texture pass's critical chain -- is not formed)
		lat_disp = self._cat_latents(shapevec, posevec) if 'disp' in want else None
		lat_col = self._cat_latents(texvec) if 'col' in want else None
		got_d = self._lat_disp if 'disp' not in want else (0 if lat_disp is None else lat_disp.shape[-1])
		got_c = self._lat_col if 'col' not in want else (0 if lat_col is None else lat_col.shape[-1])
		if got_d != self._lat_disp or got_c != self._lat_col:
			raise RuntimeError(f'latent widths do not match the head input sizes: disp head expects {self._lat_disp} latent columns '
							   f'(got {got_d}), col head expects {self._lat_col} (got {got_c}); cf. model.py:352,361')
		enc = self.encoder[0] if len(self.encoder) else None
		B = enc.B(pos.device) if enc is not None else None
		avg = self.avg_col if self.use_avg_colour else None
		disp, col = FN.mlp(self._spec, pos, lat_disp, lat_col, B, avg, self._weights(), want=want, defer_wgrad_join=defer_wgrad_join)
		return {k: v for k, v in (('disp', disp), ('col', col)) if v is not None}

	def get_meshes(self, shapevec=None, reg=None, texvec=None, posevec=None, no_displacement=False, include_texture=True, lazy_colours=False):
		"""Evaluate the field at every template vertex, apply the learned similarity registration and return
		dict(meshes, offsets, verts, disp, col)   (model.py:455-504).
		lazy_colours (not in the reference): the colour head is evaluated when `col` / `meshes.textures` is first READ instead of here --
		ModelWithLoss asks for this on steps that render nothing (chamf / smooth / texture read the vertices only; the texture term queries
		the field at its own samples), where the reference computes the template's colours and drops them.  Same values either way."""
		N = 0 if shapevec is None else shapevec.shape[0]
		self._check_per_vertex_features()
		meshes = extend_template(self.template_mesh, N=N)
		tv = self.template_verts.data  # (1, V, 3): the trunk is evaluated once for all N feet
		if not self.use_texvec:
			# (the reference falls back to self.template_tex here, model.py:500 -- an attribute its constructor never assigns (the lines that
			# built it are commented out, model.py:288-295): upstream raises AttributeError on this path as well)
			raise NotImplementedError('use_texvec=False: the template-texture fallback of get_meshes does not exist upstream either (model.py:288-295, 500)')
		if lazy_colours:
			cell = _Once(lambda: self(tv, shapevec=shapevec, texvec=texvec, posevec=posevec, want=('col',))['col'])
			res = _LazyColours(self(tv, shapevec=shapevec, texvec=texvec, posevec=posevec, want=('disp',)), cell)
		else:
			res = self(tv, shapevec=shapevec, texvec=texvec, posevec=posevec)
		offsets = res['disp']
		if reg is not None:
			X = FN.register_points(tv, offsets, reg)
		else:
			X = tv + offsets
		if not no_displacement:
			meshes = meshes.update_padded(X)
		if lazy_colours:
			meshes.textures = LazyTexturesVertex(lambda: cell()[..., :3])
		else:
			meshes.textures = TexturesVertex(res['col'][..., :3])
		res.update(meshes=meshes, offsets=offsets, verts=X)
		if self.per_vertex_features is not None:
			res['cpv'] = self.per_vertex_features
		return res

	def get_meshes_from_batch(self, batch, is_train=True, no_displacement=False, lazy_colours=False):
		sfx = 'train' if is_train else 'val'
		return self.get_meshes(shapevec=batch.get(f'shapevec_{sfx}', None), reg=batch.get(f'reg_{sfx}', None),
							   texvec=batch.get(f'texvec_{sfx}', None), posevec=batch.get(f'posevec_{sfx}', None),
							   include_texture=True, no_displacement=no_displacement, lazy_colours=lazy_colours)

	def reset_weights(self):
		"""Zero the last displacement layer so the initial mesh equals the template (model.py:516-518)."""
		self.mlp_disp[-1].weight.data.zero_()
		self.mlp_disp[-1].bias.data.zero_()

	def configure_template(self, state_dict, device='cuda'):
		self.template_verts = nn.Parameter(state_dict['template_verts'].float().to(device), requires_grad=False)
		self.template_faces = nn.Parameter(state_dict['template_faces'].to(device), requires_grad=False)
		self._rebuild_template_mesh()
		self._check_per_vertex_features()
		if 'avg_col' in state_dict:
			self.avg_col = nn.Parameter(state_dict['avg_col'].to(device), requires_grad=False)

	def set_template(self, verts, faces):
		"""Install an in-memory template (verts (V,3) float, faces (F,3) int); used by synthetic benchmarks/tests."""
		dev = self.template_verts.device
		self.configure_template({'template_verts': verts.reshape(1, -1, 3), 'template_faces': faces.reshape(1, -1, 3)}, device=dev)

	def to(self, device):
		out = super().to(device)
		self._rebuild_template_mesh()
		return out


class PCAModel(Model):
	"""Linear PCA foot model, the baseline FIND is compared with (reference model.py:536-655): template + sum_b coefs[:, b] * shapevec[b],
	then the learned similarity registration.  Offsets run in find_pca_fwd / find_pca_bwd, registration in find_register_fwd / bwd (the
	kernels of NeuralDisplacementField.get_meshes).  The model comes from a .mat file (load_from_mat) or a .pth checkpoint (load); state_dict
	keys are the reference's (template_verts, template_faces, pca_var, pca_coefs, reg.data, reg_val.data, shapevec.data, shapevec_val.data),
	so checkpoints move between the two in both directions."""

	def __init__(self, *args, train_size=None, val_size=None, device='cuda', **kwargs):
		super().__init__()
		self.params = dict(train_size=train_size, val_size=val_size)
		self.train_size, self.val_size = train_size, val_size
		# set by configure_template
		self.template_verts = self.template_faces = self.template_mesh = None
		self.pca_var = None     # (B,) as stored in the .mat file; never read (as upstream)
		self.pca_coefs = None   # (V, B, 3)
		self.latent_vectors_train, self.latent_vectors_val = [], []
		self.shapevec, self.shapevec_val = None, None
		ident = np.array([0] * 6 + [1] * 3)
		self.reg = LatentVector(train_size, vec_size=9, name='reg_train', device=device, init_values=ident)
		self.reg_val = LatentVector(val_size, vec_size=9, name='reg_val', device=device, init_values=ident)
		self.latent_vectors_train.append(self.reg)
		self.latent_vectors_val.append(self.reg_val)
		self.configure_params()

	def configure_params(self):
		"""Parameter groups read by train.py:161-168 (model.py:563-567)."""
		self.main_params = make_params_list(self.shapevec)
		self.val_params = make_params_list(self.shapevec_val)
		self.reg_params = make_params_list(self.reg, self.reg_val)
		self.latent_params = make_params_list(self.shapevec, self.shapevec_val)

	def _rebuild_template_mesh(self):
		if self.template_verts is not None:
			self.template_mesh = Meshes(verts=self.template_verts.data, faces=self.template_faces.data[0])

	def _apply(self, fn, *args, **kwargs):
		out = super()._apply(fn, *args, **kwargs)
		self._rebuild_template_mesh()
		return out

	def get_meshes(self, shapevec=None, reg=None, **kwargs):
		"""dict(meshes, offsets, verts) for shape codes (N, B) and registrations (N, 9) or None (model.py:573-601).  Every other keyword --
		no_displacement, lazy_colours, ... -- is accepted and ignored, as upstream.  The texture is a constant grey."""
		N = shapevec.shape[0]
		meshes = extend_template(self.template_mesh, N=N)
		tv = self.template_verts.data   # (1, V, 3), shared by the N feet
		offsets = FN.pca_offsets(self.pca_coefs, shapevec)
		X = FN.register_points(tv, offsets, reg) if reg is not None else tv + offsets
		meshes = meshes.update_padded(X)
		meshes.textures = TexturesVertex(torch.full(X.shape, 0.5, dtype=torch.float32, device=X.device))
		return dict(meshes=meshes, offsets=offsets, verts=X)

	def get_meshes_from_batch(self, batch, is_train=True, **kwargs):
		sfx = 'train' if is_train else 'val'
		return self.get_meshes(shapevec=batch.get(f'shapevec_{sfx}', None), reg=batch.get(f'reg_{sfx}', None))

	def forward(self, *args, **kwargs):
		raise NotImplementedError('PCAModel has no field to query: it is evaluated through get_meshes / get_meshes_from_batch (the texture loss, '
								  'which queries a colour field, does not apply to it)')

	@classmethod
	def load_from_mat(cls, src, device, **kwargs):
		"""pcaMean (3V) -> template_verts (1, V, 3); mesh (F, 3), 1-based -> template_faces (1, F, 3); pcaCoefs (3V, B), rows vertex-major ->
		pca_coefs (V, B, 3); pcaVar -> pca_var as stored (model.py:610-628)."""
		from scipy.io import loadmat
		data = loadmat(src)
		sd = {}
		sd['template_verts'] = torch.from_numpy(data['pcaMean'].reshape(-1, 3)).unsqueeze(0).float()
		sd['template_faces'] = torch.from_numpy(data['mesh']).unsqueeze(0).long() - 1
		V = sd['template_verts'].shape[1]
		sd['pca_coefs'] = torch.from_numpy(data['pcaCoefs']).reshape(V, 3, -1).permute(0, 2, 1).float()
		sd['pca_var'] = torch.from_numpy(data['pcaVar']).float()
		model = cls(device=device, **kwargs)
		model.configure_template(sd, device=device)
		model.load_state_dict(sd, strict=False)
		model.configure_params()
		return model

	@classmethod
	def load(cls, file, device='cuda', opts=None, **kwargs):
		if file.endswith('.pth'):
			model = super().load(file, device=device, opts=opts, **kwargs)
			# Deviation from upstream: Model.load never calls configure_params again, so there the four groups stay empty after a .pth
			# load (torch.optim raises on them).  They are filled here, on both paths.
			model.configure_params()
			return model
		if file.endswith('.mat'):
			return cls.load_from_mat(file, device=device, opts=opts, **kwargs)
		raise NotImplementedError(f'Filetype `{os.path.splitext(file)[-1]}` for PCA model not understood')

	def configure_template(self, state_dict, device='cuda'):
		"""Template, coefficients and the shape-code tables, B wide, appended after reg (model.py:639-655)."""
		self.template_verts = nn.Parameter(state_dict['template_verts'].float().to(device), requires_grad=False)
		self.template_faces = nn.Parameter(state_dict['template_faces'].to(device), requires_grad=False)
		self._rebuild_template_mesh()
		self.pca_var = nn.Parameter(state_dict['pca_var'].to(device), requires_grad=False)
		self.pca_coefs = nn.Parameter(state_dict['pca_coefs'].float().to(device), requires_grad=False)
		V, B, _ = self.pca_coefs.shape
		self.shapevec = LatentVector(self.train_size, vec_size=B, name='shapevec_train', device=device)
		self.shapevec_val = LatentVector(self.val_size, vec_size=B, name='shapevec_val', device=device)
		self.latent_vectors_train.append(self.shapevec)
		self.latent_vectors_val.append(self.shapevec_val)

	def to(self, device):
		out = super().to(device)
		self._rebuild_template_mesh()
		return out


def _skin_arrays(data, num_betas, dtype=np.float32):
	"""The constants of a skinned model from the arrays of a STAR / SUPR style file (SkinnedModel.load), as `dtype` / int tensors on the CPU:
	v_template (V, 3), dirs (V, B + P, 3), J0 (J, 3), JS (J, B, 3), weights (V, J), parent (J) int32, faces (F, 3) int64.  The joint
	regressor is folded through the template and the shape directions here, in float64: J0 = Jreg v_template, JS = Jreg shapedirs.
	Anything whose shape is not one of the layouts named in SkinnedModel.load is refused with that shape in the message."""
	def need(key):
		if key not in data:
			raise ValueError(f'SkinnedModel: the file has no `{key}` (keys: {sorted(data)})')
		a = data[key]
		return a.detach().cpu().numpy() if torch.is_tensor(a) else a

	def bad(key, a, want):
		return ValueError(f'SkinnedModel: `{key}` has shape {tuple(a.shape)}; expected {want}')

	vt = np.asarray(need('v_template'), dtype=np.float64)
	if vt.ndim != 2 or vt.shape[1] != 3 or vt.shape[0] < 1:
		raise bad('v_template', vt, '(V, 3)')
	V = vt.shape[0]
	w = np.asarray(need('weights'), dtype=np.float64)
	if w.ndim != 2 or w.shape[0] != V or w.shape[1] < 1:
		raise bad('weights', w, f'({V}, J)')
	J = w.shape[1]
	sd = np.asarray(need('shapedirs'), dtype=np.float64)
	if sd.ndim != 3 or sd.shape[:2] != (V, 3) or sd.shape[2] < num_betas or num_betas < 1:
		raise bad('shapedirs', sd, f'({V}, 3, >= num_betas = {num_betas})')
	sd = sd[:, :, :num_betas]
	pd = np.asarray(need('posedirs'), dtype=np.float64)
	if pd.ndim == 2 and pd.shape[0] == 3 * V:
		pd = pd.reshape(V, 3, -1)
	if pd.ndim != 3 or pd.shape[:2] != (V, 3) or pd.shape[2] not in (4 * J, 4 * (J - 1)):
		raise bad('posedirs', pd, f'({V}, 3, P) or ({3 * V}, P) with P = 4 J = {4 * J} or 4 (J - 1) = {4 * (J - 1)} quaternion features')
	jr = need('J_regressor')
	if hasattr(jr, 'toarray'):   # scipy.sparse
		jr = jr.toarray()
	jr = np.asarray(jr, dtype=np.float64)
	if jr.shape == (3 * J, 3 * V):
		# the regressor acting on the flattened vertices (rows 3j + c, columns 3v + c): it must be a per-coordinate copy of one (J, V) matrix
		small = jr[0::3, 0::3]
		if not np.array_equal(jr, np.kron(small, np.eye(3))):
			raise ValueError(f'SkinnedModel: `J_regressor` has shape {tuple(jr.shape)} but is not kron(R, I3) of a ({J}, {V}) regressor R')
		jr = small
	if jr.shape != (J, V):
		raise bad('J_regressor', jr, f'({J}, {V}) or ({3 * J}, {3 * V})')
	kt = np.asarray(need('kintree_table'))
	if kt.shape != (2, J):
		raise bad('kintree_table', kt, f'(2, {J})')
	parent = kt[0].astype(np.int64)
	parent[(parent < 0) | (parent >= J)] = -1   # (the published files mark the root with 2^32 - 1)
	for j in range(J):
		if parent[j] >= j or (j == 0 and parent[j] != -1):
			raise ValueError(f'SkinnedModel: `kintree_table` puts joint {j} before its parent {parent[j]}; parents must precede their children')
	f = np.asarray(need('f'))
	if f.ndim != 2 or f.shape[1] != 3 or (f.size and (f.min() < 0 or f.max() >= V)):
		raise bad('f', f, f'(F, 3) with vertex ids below {V}')
	dirs = np.concatenate([sd, pd], axis=2).transpose(0, 2, 1)   # (V, B + P, 3)
	J0 = jr @ vt
	JS = np.einsum('jv,vcb->jbc', jr, sd)
	t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))
	return dict(v_template=t32(vt), dirs=t32(dirs), J0=t32(J0), JS=t32(JS), weights=t32(w), parent=torch.from_numpy(parent.astype(np.int32)),
				faces=torch.from_numpy(f.astype(np.int64)))


class SkinnedModel(Model):
	"""Articulated foot model, the third model FIND is compared with (reference model.py:658-799, SUPRModel): SMPL-family linear blend
	skinning with quaternion pose correctives as STAR / SUPR publish it, then the learned similarity registration.  The reference calls a
	submodule for the skinning; here it is find_skin_fwd / find_skin_bwd (FN.linear_blend_skinning), the registration find_register_fwd / bwd.
	Tables, batch keys and parameter groups are upstream's: pose (3J, zeros), betas (B), trans (3, -mean(v_template)) and reg (9), each
	_train and _val; main = betas_train + pose_train, val = betas_val + pose_val, reg = both regs, latent = betas and pose of both splits,
	trans in none.  Not upstream's: reg_init defaults to the identity (upstream hard-codes a start rotation for SUPR; align.init_registration
	finds one: reg / reg_val / template_verts / template_faces are there for it), the loop that caps the open ankle is an argument of load
	(cap_loops), and a checkpoint carries the model's constants, so loading one needs no path to the model file."""
	CONSTS = ('v_template', 'dirs', 'J0', 'JS', 'weights', 'parent')
	TABLES = ('pose', 'betas', 'trans', 'reg')

	def __init__(self, *args, train_size=None, val_size=None, device='cuda', num_betas=10, reg_init=None, **kwargs):
		super().__init__()
		reg_init = [0.] * 6 + [1.] * 3 if reg_init is None else [float(x) for x in reg_init]
		if len(reg_init) != 9:
			raise ValueError(f'SkinnedModel: reg_init must have 9 entries (translation, euler XYZ, scale), got {len(reg_init)}')
		self.params = dict(train_size=train_size, val_size=val_size, num_betas=num_betas, reg_init=reg_init)
		self.train_size, self.val_size, self.num_betas, self.reg_init = train_size, val_size, num_betas, reg_init
		# set by configure_template
		self.template_verts = self.template_faces = self.template_mesh = None
		for k in self.CONSTS:
			setattr(self, k, None)
		for k in self.TABLES:
			setattr(self, f'{k}_train', None)
			setattr(self, f'{k}_val', None)
		self.latent_vectors_train, self.latent_vectors_val = [], []
		self.configure_params()

	@property
	def reg(self):
		"""reg_train under the name the other models (and align.init_registration) use; reg_val is upstream's name already."""
		return self.reg_train

	def configure_params(self):
		"""Parameter groups read by train.py:161-168 (model.py:718-722)."""
		self.main_params = make_params_list(self.betas_train, self.pose_train)
		self.val_params = make_params_list(self.betas_val, self.pose_val)
		self.reg_params = make_params_list(self.reg_train, self.reg_val)
		self.latent_params = make_params_list(self.betas_train, self.betas_val, self.pose_train, self.pose_val)

	def _rebuild_template_mesh(self):
		if self.template_verts is not None:
			self.template_mesh = Meshes(verts=self.template_verts.data, faces=self.template_faces.data[0])
			self._no_verts = torch.zeros_like(self.template_verts.data)

	def _apply(self, fn, *args, **kwargs):
		out = super()._apply(fn, *args, **kwargs)
		self._rebuild_template_mesh()
		return out

	def get_meshes(self, poses=None, betas=None, trans=None, reg=None, return_joints=False, **kwargs):
		"""dict(meshes, verts) for poses (N, 3J), betas (N, B), translations (N, 3) and registrations (N, 9) or None (model.py:726-744).  Every
		other keyword is accepted and ignored, as upstream.  The texture is a constant grey.  return_joints (not upstream): also `joints`
		(N, J, 3), the posed joints before the registration, detached."""
		X, joints = FN.linear_blend_skinning(self, poses, betas, trans, return_joints=True)
		if reg is not None:
			X = FN.register_points(self._no_verts, X, reg)
		meshes = extend_template(self.template_mesh, N=X.shape[0]).update_padded(X)
		meshes.textures = TexturesVertex(torch.full(X.shape, 0.5, dtype=torch.float32, device=X.device))
		res = dict(meshes=meshes, verts=X)
		if return_joints:
			res['joints'] = joints
		return res

	def get_meshes_from_batch(self, batch, is_train=True, **kwargs):
		sfx = 'train' if is_train else 'val'
		return self.get_meshes(poses=batch[f'pose_{sfx}'], betas=batch[f'betas_{sfx}'], trans=batch[f'trans_{sfx}'], reg=batch.get(f'reg_{sfx}', None))

	def forward(self, *args, **kwargs):
		raise NotImplementedError('SkinnedModel has no field to query: it is evaluated through get_meshes / get_meshes_from_batch (the texture loss, '
								  'which queries a colour field, does not apply to it)')

	def configure_template(self, state_dict, device='cuda'):
		"""The model's constants, the centred rest mesh as template_verts / template_faces, and the eight latent tables in upstream's order
		(model.py:690-709)."""
		for k in self.CONSTS:
			t = state_dict[k]
			setattr(self, k, nn.Parameter((t.to(torch.int32) if k == 'parent' else t.float()).to(device), requires_grad=False))
		V, J = self.weights.shape
		B = self.JS.shape[1]
		if B != self.num_betas:
			raise ValueError(f'SkinnedModel: the constants hold {B} shape directions, num_betas is {self.num_betas}')
		trans_init = -self.v_template.data.mean(dim=0)
		self.template_verts = nn.Parameter((self.v_template.data + trans_init).unsqueeze(0), requires_grad=False)
		self.template_faces = nn.Parameter(state_dict['template_faces'].to(device), requires_grad=False)
		self._rebuild_template_mesh()
		trans_init = trans_init.cpu().numpy()
		reg_init = np.array(self.reg_init)
		for sfx, size, tables in (('train', self.train_size, self.latent_vectors_train), ('val', self.val_size, self.latent_vectors_val)):
			del tables[:]
			made = dict(pose=LatentVector(size, vec_size=3 * J, name=f'pose_{sfx}', device=device),
						betas=LatentVector(size, vec_size=B, name=f'betas_{sfx}', device=device),
						trans=LatentVector(size, vec_size=3, name=f'trans_{sfx}', device=device, init_values=trans_init),
						reg=LatentVector(size, vec_size=9, name=f'reg_{sfx}', device=device, init_values=reg_init))
			for k in self.TABLES:
				setattr(self, f'{k}_{sfx}', made[k])
				tables.append(made[k])
		self.configure_params()

	@classmethod
	def from_arrays(cls, data, device='cuda', num_betas=10, cap_loops=None, **kwargs):
		"""A model from the arrays of a STAR / SUPR style file (the keys: load).  cap_loops: ordered vertex loops, each closed with a fan of
		triangles (loop[0], loop[i], loop[i + 1]) appended to the faces -- upstream's cap over the open ankle (model.py:713-716)."""
		sd = _skin_arrays(data, num_betas)
		faces = sd.pop('faces')
		V = sd['v_template'].shape[0]
		for loop in (cap_loops or []):
			loop = [int(i) for i in loop]
			if len(loop) < 3 or min(loop) < 0 or max(loop) >= V:
				raise ValueError(f'SkinnedModel: a cap loop needs at least 3 vertex ids below {V}, got {len(loop)} ids in [{min(loop, default=0)}, {max(loop, default=0)}]')
			faces = torch.cat([faces, torch.tensor([[loop[0], b, c] for b, c in zip(loop[1:], loop[2:])], dtype=torch.int64)], dim=0)
		sd['template_faces'] = faces.unsqueeze(0)
		kwargs.pop('opts', None)
		model = cls(device=device, num_betas=num_betas, **kwargs)
		model.configure_template(sd, device=device)
		return model

	@classmethod
	def load(cls, file, device='cuda', opts=None, num_betas=10, cap_loops=None, **kwargs):
		"""file: .npz (plain arrays), .npy holding a pickled dict (the format SUPR is distributed in) or a .pth checkpoint of a fitted
		SkinnedModel.  Arrays read from a model file: v_template (V, 3), shapedirs (V, 3, >= num_betas), posedirs (V, 3, P) or (3V, P)
		with P = 4J or 4(J-1), J_regressor (J, V) or (3J, 3V), dense or scipy-sparse, weights (V, J), kintree_table (2, J) with the
		parents in row 0 (any out-of-range value marks the root; parents must precede their children, else ValueError) and f (F, 3)."""
		ext = os.path.splitext(file)[-1]
		if ext == '.pth':
			data = torch.load(file, map_location=device, weights_only=False)
			params, sd = dict(data['params']), data['state_dict']
			skip_latents = opts is not None and getattr(opts, 'dont_load_latents', False)
			if skip_latents:
				params['train_size'], params['val_size'] = kwargs.get('train_size', 1), kwargs.get('val_size', 1)
				sd = {k: v for k, v in sd.items() if k not in {f'{t}_{s}.data' for t in cls.TABLES for s in ('train', 'val')}}
			model = cls(**params, device=device)
			model.configure_template(sd, device=device)
			model.load_state_dict(sd, strict=False)
			return model
		if ext == '.npz':
			with np.load(file, allow_pickle=False) as z:
				data = {k: z[k] for k in z.files}
		elif ext == '.npy':
			data = np.load(file, allow_pickle=True)   # (a pickled dict: the one place that unpickles a model file)
			if not (isinstance(data, np.ndarray) and data.dtype == object and data.shape == ()) or not isinstance(data.item(), dict):
				raise ValueError(f'SkinnedModel: {file} does not hold a dict (got {type(data).__name__} of shape {getattr(data, "shape", None)})')
			data = data.item()
		else:
			raise NotImplementedError(f'Filetype `{ext}` for a skinned model not understood')
		return cls.from_arrays(data, device=device, num_betas=num_betas, cap_loops=cap_loops, **kwargs)
