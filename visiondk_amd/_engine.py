"""What the native model wrappers share: `FlatEngine` (the flat HBM buffers of one model and their workspaces) and `FlatParamModule` (the nn.Module with timm's names whose
Parameters are views into the engine's flat fp32 buffer).  vit / swin / convnext / resnet hold what is theirs: the config struct, the ABI prefix, the derived-weight
buffers, the init rule and the reshaping of the output."""
from __future__ import annotations

import copy
import ctypes as C
from typing import Optional

import torch
import torch.nn as nn

from . import _abi, _lib

OPERANDS = {"bf16": torch.bfloat16, "fp16": torch.float16}


def check_image(x: torch.Tensor, in_chans: int, img_size: int) -> None:
    if x.dtype != torch.float32 or x.dim() != 4 or tuple(x.shape[1:]) != (in_chans, img_size, img_size):
        raise ValueError(f"expected float32 [B, {in_chans}, {img_size}, {img_size}], got {tuple(x.shape)} {x.dtype}")


def seeded_generator(seed: Optional[int]) -> torch.Generator:
    """the CPU generator reset_parameters draws from.  No explicit seed: it is drawn from torch's global generator, so that `torch.manual_seed(s)` reproduces the
    initialisation like it does for the reference's model (and data-parallel ranks seeded alike start alike even before the broadcast)"""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed if seed is not None else int(torch.randint(0, 2 ** 31 - 1, (1,)).item()))
    return gen


def pad_cast_dlogits(eng: "FlatEngine", dlogits: torch.Tensor) -> torch.Tensor:
    """dlogits f32 [B, C] -> the operand format [B, cp], zero-padded columns for the head GEMMs: one cast kernel on a padded staging buffer
    (fp16 operands: under the reference's GradScaler the incoming gradient already carries the loss scale, train.py:205)"""
    be = eng.be
    B, Cn = dlogits.shape
    stage = torch.zeros((B, eng.cp), dtype=torch.float32, device=dlogits.device)
    stage[:, :Cn].copy_(dlogits)
    dl = torch.empty((B, eng.cp), dtype=eng.op_dtype, device=dlogits.device)
    cast = be.lib.vdk_cast_f32_f16 if eng.operand == "fp16" else be.lib.vdk_cast_f32_bf16
    be.check(cast(be.ptr(stage), be.ptr(dl), stage.numel(), be.stream()), "vdk_cast_f32_16")
    return dl


class FlatEngine:
    """Owns the flat HBM buffers of one model (fp32 master params, 16-bit operand copies, grads, the family's derived-weight buffers) and its grow-only workspaces."""

    def __init__(self, spec, device=None, backend: Optional[_lib.Backend] = None, operand: str = "bf16"):
        assert operand in OPERANDS, operand
        self.spec = spec
        self.operand = operand
        self.be = backend or _lib.load()
        self.device = torch.device(device if device is not None else ("cuda" if self.be.device_only else "cpu"))
        self._derived = ()
        self._ws: Optional[torch.Tensor] = None        # the training forward's workspace (it keeps the activations for the backward)
        self._ws_batch = -1                            # what _ws was laid out for; -1 invalidates it
        self._ws32: Optional[torch.Tensor] = None      # forward_precise's
        self._ws_t32: Optional[torch.Tensor] = None    # the fp32 training arithmetic's (ConvNeXt)
        self._weights_version = None

    @property
    def op_dtype(self) -> torch.dtype:
        return OPERANDS[self.operand]

    def _read_entries(self, info_fn, cfg, n: int, *which) -> list:
        """(name, offset, numel, shape) of the n tensors a family's vdk_<family>_param_info enumerates (`which`: ResNet's parameters / buffers selector)"""
        name = C.create_string_buffer(96)
        off, numel, ndim = _abi.I64(0), _abi.I64(0), _abi.I32(0)
        shape = (_abi.I64 * 4)()
        out = []
        for i in range(n):
            self.be.check(info_fn(C.byref(cfg), *which, i, name, 96, C.byref(off), C.byref(numel), shape, C.byref(ndim)), info_fn.__name__)
            out.append((name.value.decode(), off.value, numel.value, tuple(shape[j] for j in range(ndim.value))))
        return out

    def _alloc(self, **derived) -> None:
        """params / grads / wb16 over n_floats, and the family's derived-weight buffers as name=(numel, dtype); the device move follows the same list"""
        dev = self.device
        self.params = torch.zeros(self.n_floats, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(self.n_floats, dtype=torch.float32, device=dev)
        self.wb16 = torch.zeros(self.n_floats, dtype=self.op_dtype, device=dev)
        for attr, (numel, dtype) in derived.items():
            setattr(self, attr, torch.zeros(numel, dtype=dtype, device=dev))
        self._derived = tuple(derived)

    def __deepcopy__(self, memo):   # ModelEMA deep-copies the model; the library handle is shared
        new = object.__new__(type(self))
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            setattr(new, k, v if k == "be" else copy.deepcopy(v, memo))
        return new

    def view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        """the tensor `name` (timm key) inside a flat buffer laid out like params (grads, a momentum or EMA buffer of the fused step)"""
        for n, off, numel, shape in self.entries:
            if n == name:
                return flat[off:off + numel].view(shape)
        raise KeyError(name)

    def views(self, flat: torch.Tensor) -> tuple:
        return tuple(flat[off:off + numel].view(shape) for (_, off, numel, shape) in self.entries)

    def _image(self, x: torch.Tensor) -> torch.Tensor:
        """the input of a family whose image size is fixed by its spec, checked and contiguous"""
        check_image(x, self.spec.in_chans, self.spec.img_size)
        return x.contiguous()

    def _ensure_fresh(self) -> None:
        if self._weights_version != self.params._version:
            self.refresh_weights()

    def _grow(self, attr: str, size_fn, cfg) -> torch.Tensor:
        """the workspace `attr`, at least as large as size_fn reports for cfg.  Grow-only (OHEM hands the step a different, smaller batch every iteration); the old one
        is freed before the larger one is allocated"""
        need = C.c_size_t(0)
        self.be.check(size_fn(C.byref(cfg), C.byref(need)), size_fn.__name__)
        if getattr(self, attr) is None or getattr(self, attr).numel() < need.value:
            setattr(self, attr, None)
            setattr(self, attr, torch.empty(need.value, dtype=torch.uint8, device=self.device))
        return getattr(self, attr)

    def moved_to(self, device: torch.device) -> None:
        """every buffer to `device` (.to keeps each one's dtype: fp32 masters, 16-bit operand copies); every workspace dropped"""
        self.device = device
        for attr in ("params", "grads", "wb16") + self._derived:
            setattr(self, attr, getattr(self, attr).to(device))
        self._ws = self._ws32 = self._ws_t32 = None
        self._ws_batch, self._weights_version = -1, None


class _Holder(nn.Module):
    """empty container mirroring one level of timm's module tree (patch_embed, blocks.3.attn, ...); owns Parameters / buffers only"""


class FlatParamModule(nn.Module):
    """The module tree mirrors timm's with parameter-only holder modules, so named_parameters() / state_dict() / load_state_dict() carry timm's key names at any nesting
    depth; every Parameter is a view into the engine's flat fp32 buffer.  A family sets `engine` and calls _build_tree()."""

    family = ""      # as the error messages name it

    def _holder(self, path) -> nn.Module:
        m = self
        for part in path:
            if part not in m._modules:
                m.add_module(part, _Holder())
            m = m._modules[part]
        return m

    def _build_tree(self) -> None:
        self._plist = []      # (timm name, Parameter) pairs in flat-buffer order
        eng = self.engine
        for (name, *_), v in zip(eng.entries, eng.views(eng.params)):
            parts = name.split(".")
            p = nn.Parameter(v)
            self._holder(parts[:-1]).register_parameter(parts[-1], p)
            self._plist.append((name, p))

    # keep the flat buffer authoritative even if someone re-pointed a parameter (.to(), deepcopy, p.data = ...)
    def _sync_flat(self) -> None:
        eng = self.engine
        base = eng.params.data_ptr()
        for (name, off, numel, shape), (_, p) in zip(eng.entries, self._plist):
            if p.data_ptr() != base + off * 4:
                with torch.no_grad():
                    eng.params[off:off + numel].view(shape).copy_(p.detach().to(eng.device))
                    p.data = eng.params[off:off + numel].view(shape)

    def _apply(self, fn, recurse=True):
        eng = self.engine
        probe = fn(torch.zeros(1, dtype=torch.float32, device=eng.device))
        if probe.device != eng.device or probe.dtype != torch.float32:
            if probe.dtype != torch.float32:
                raise RuntimeError(f"visiondk_amd {self.family} keeps fp32 master weights; bf16 copies are internal")
            if eng.be.device_only and probe.device.type != "cuda":
                raise RuntimeError(f"visiondk_amd {self.family} lives on the GPU (no CPU fallback)")
            eng.moved_to(probe.device)
            for (_, p), v in zip(self._plist, eng.views(eng.params)):
                p.data = v
        return self

    def _flat_grads(self, g: torch.Tensor) -> tuple:
        """what the family's autograd.Function returns for (x, module, *params): the parameter gradients as views of the flat gradient"""
        return (None, None) + self.engine.views(g)
