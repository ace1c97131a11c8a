"""The engines stay inside the workspace size they report, and never read a workspace region before writing it.

The wrappers allocate their workspaces with torch.empty and grow-only (a smaller batch runs inside the stale contents of a larger one), so a region that is read before it is
written, or a write past the reported size, lands in memory that usually happens to be harmless.  Here the wrapper's workspace is replaced by a guard-banded view (tests/extent.py)
of EXACTLY the reported number of bytes, filled with 0x00 / 0xFF (NaN) / 0x7B before the forward (never between forward and backward: that state lives there by design):
  I1  the guards around the workspace are intact after forward + backward (the reported size is sufficient);
  I2  outputs, every gradient, and for the train steps the updated parameters / momentum / EMA / loss-scale state are bit-identical across the three patterns;
  grow-only: on the NaN pattern, batch `big`, then batch `small` inside the same buffer WITHOUT a refill, then once more WITH a refill: equal bit for bit
             (stale contents of a larger batch are as good as poison).
"""
import ctypes as C

import pytest
import torch

from tests.extent import FILLS, assert_guards_intact, assert_same_bits, bits, embed, one_torch_thread
from visiondk_amd import convnext, face, resnet, swin, vit


class _Guarded:
    def __init__(self, nbytes, fill, dev, name):
        self.fill = fill
        self.reg, self.view = embed(torch.zeros(nbytes, dtype=torch.uint8), fill=fill, dev=dev, name=name)
        self.refill()

    def refill(self):
        self.reg.big.fill_(self.fill)

    def check(self):
        assert_guards_intact(self.reg, self.fill)


def _need(be, fn, cfg):
    n = C.c_size_t(0)
    be.check(fn(C.byref(cfg), C.byref(n)), fn.__name__)
    return int(n.value)


def _sync(be):
    if be.device_only:
        torch.cuda.synchronize()


def _isolation(be, dev, build, attr, need, forward, backward=None, big=5, small=3):
    """build() -> engine (same weights every time); need(eng, batch) -> bytes; forward(eng, batch) -> output; backward(eng, batch) -> flat gradient"""
    with one_torch_thread():
        _isolation_rounds(be, dev, build, attr, need, forward, backward, big, small)


def _isolation_rounds(be, dev, build, attr, need, forward, backward, big, small):
    results = []
    for fill in FILLS:
        eng = build()
        g = _Guarded(need(eng, big), fill, dev, f"{type(eng).__name__}.{attr}")
        setattr(eng, attr, g.view)
        eng._ws_batch = -1

        def rnd(batch, refill):
            if refill:
                g.refill()
            r = {"out": forward(eng, batch).clone()}
            if backward is not None:
                r["grads"] = backward(eng, batch).clone()
            _sync(be)
            g.check()
            assert getattr(eng, attr).data_ptr() == g.view.data_ptr(), "the wrapper replaced the workspace: the reported size did not suffice for its own check"
            return {k: bits(v) for k, v in r.items()}

        results.append(rnd(big, True))
        assert need(eng, small) <= need(eng, big)
        if fill == FILLS[1]:                        # grow-only, on the NaN pattern: the smaller batch inside the stale contents of the larger one ...
            stale = rnd(small, False)
            fresh = rnd(small, True)                # ... equals the run on a freshly poisoned buffer
            assert_same_bits([fresh, stale], f"batch {small} after batch {big} without a refill")
    assert_same_bits(results, "across the patterns")
    for v in results[0].values():
        assert bool(torch.isfinite(v.view(torch.float32)).all())          # (the outputs are f32: a NaN that is the same in every run would pass the comparison above)


# ---------------------------------------------------------------------------------------------------------------- ViT
_X = {}


def _x(n, shape, seed=0):
    key = (n, shape, seed)
    if key not in _X:
        _X[key] = torch.randn((n,) + shape, generator=torch.Generator().manual_seed(seed))
    return _X[key]


def _dl(n, cols, valid, dtype, seed=1):
    d = torch.randn(n, cols, generator=torch.Generator().manual_seed(seed)) * 0.1
    d[:, valid:] = 0
    return d.to(dtype)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp8", "no_cls", "pre_norm"])
def test_vit_engine_workspace(be, dev, mode):
    fp8 = mode == "fp8"
    kw = dict(img_size=32, patch_size=8, num_classes=10, dim=256 if fp8 else 64, depth=1 if fp8 else 2, heads=4 if fp8 else 1, mlp_dim=256 if fp8 else 128)
    if fp8:
        kw.update(img_size=64)                     # the fp8 GEMMs need M, N >= 256: 5 x 65 tokens, dim 256 (the smallest spec of tests/test_vit_fp8.py)
    if mode == "no_cls":
        kw.update(class_token=False, num_classes=0)
    if mode == "pre_norm":
        kw.update(pre_norm=True)
    spec = vit.VitSpec(**kw)
    operand = "fp16" if mode == "fp16" else "bf16"
    big, small = (5, 4) if fp8 else (5, 3)         # (the fp8 mode needs batch * tokens >= 256)

    def build():
        m = vit.VisionTransformer(spec, device=dev, backend=be, seed=0, operand=operand)
        if fp8:
            m.engine.enable_fp8(1)
        return m.engine

    def need(eng, b):
        return _need(be, be.lib.vdk_vit_workspace_bytes, eng._cfg(b))

    def fwd(eng, b):
        if fp8:                                    # every round starts from the same scaling state (vdk_vit_fp8_update below moves it)
            eng.fp8_state[0] = 0.0; eng.fp8_state[1:] = 1.0
        return eng.forward(_x(big, (3, spec.img_size, spec.img_size))[:b].to(dev))

    def bwd(eng, b):
        if fp8:
            g = eng.backward(_dl(big, eng.cp, spec.num_classes, eng.op_dtype)[:b].contiguous().to(dev)).clone()
            eng.fp8_update()
            return torch.cat([g, eng.fp8_state.reshape(-1)])
        if eng.cp:
            return eng.backward(_dl(big, eng.cp, spec.num_classes, eng.op_dtype)[:b].contiguous().to(dev))
        return eng.backward((_x(big * eng.tokens, (spec.dim,), 2) * 0.1)[:b * eng.tokens].contiguous().to(dev))

    _isolation(be, dev, build, "_ws", need, fwd, bwd, big=big, small=small)


@pytest.mark.parametrize("class_token", [True, False])
def test_vit_engine_precise_workspace(be, dev, class_token):
    spec = vit.VitSpec(img_size=32, patch_size=8, num_classes=10 if class_token else 0, dim=64, depth=2, heads=1, mlp_dim=128, class_token=class_token)
    _isolation(be, dev, lambda: vit.VisionTransformer(spec, device=dev, backend=be, seed=0).engine, "_ws32",
               lambda eng, b: _need(be, be.lib.vdk_vit_workspace_f32_bytes, eng._cfg(b)), lambda eng, b: eng.forward_precise(_x(5, (3, 32, 32))[:b].to(dev)))


# ---------------------------------------------------------------------------------------------------------------- Swin
_SWIN = dict(img_size=224, num_classes=5, embed_dim=32, depths=(1, 1), heads=(1, 2))


def test_swin_engine_workspace(be, dev):
    spec = swin.SwinSpec(**_SWIN)

    def build():
        return swin.SwinTransformer(spec, device=dev, backend=be, seed=0).engine

    _isolation(be, dev, build, "_ws", lambda eng, b: _need(be, be.lib.vdk_swin_workspace_bytes, eng._cfg(b)),
               lambda eng, b: eng.forward(_x(2, (3, 224, 224))[:b].to(dev), training=False),
               lambda eng, b: eng.backward(_dl(2, eng.cp, 5, eng.op_dtype)[:b].contiguous().to(dev)), big=2, small=1)


def test_swin_engine_precise_workspace(be, dev):
    spec = swin.SwinSpec(**_SWIN)
    _isolation(be, dev, lambda: swin.SwinTransformer(spec, device=dev, backend=be, seed=0).engine, "_ws32",
               lambda eng, b: _need(be, be.lib.vdk_swin_workspace_f32_bytes, eng._cfg(b)), lambda eng, b: eng.forward_precise(_x(2, (3, 224, 224))[:b].to(dev)), big=2, small=1)


# ---------------------------------------------------------------------------------------------------------------- ConvNeXt
def _convnext(be, dev, operand="bf16", num_classes=0):
    spec = convnext.ConvNeXtSpec(img_size=32, depths=(1, 1, 2, 1), dims=(8, 16, 24, 32), num_classes=num_classes)
    return convnext.ConvNeXt(spec, device=dev, backend=be, seed=0, operand=operand).engine


@pytest.mark.parametrize("operand,ncls", [("fp16", 0), ("bf16", 5)])
def test_convnext_engine_workspace(be, dev, operand, ncls):
    def bwd(eng, b):
        if ncls:
            d = torch.zeros(eng.dlogits_rows(b), eng.cp)
            d[:b] = _dl(5, eng.cp, ncls, torch.float32)[:b]
            return eng.backward(d.to(eng.dt16).to(dev))
        return eng.backward((_x(5, (eng.out_ch,), 3) * 0.1)[:b].contiguous().to(dev))         # (32 / 32 = one map row per image)

    _isolation(be, dev, lambda: _convnext(be, dev, operand, ncls), "_ws", lambda eng, b: _need(be, be.lib.vdk_convnext_workspace_bytes, eng._cfg(b)),
               lambda eng, b: eng.forward(_x(5, (3, 32, 32))[:b].to(dev)), bwd)


def test_convnext_engine_f32_workspaces(be, dev):
    """forward_f32 (precise evaluation) and forward_train_f32 / backward_train_f32 (the fp32-class training arithmetic)"""
    _isolation(be, dev, lambda: _convnext(be, dev), "_ws32", lambda eng, b: _need(be, be.lib.vdk_convnext_workspace_f32_bytes, eng._cfg(b)),
               lambda eng, b: eng.forward_precise(_x(5, (3, 32, 32))[:b].to(dev)))

    def build():
        eng = _convnext(be, dev)
        eng.precision = "fp32"
        return eng

    _isolation(be, dev, build, "_ws_t32", lambda eng, b: _need(be, be.lib.vdk_convnext_train_f32_workspace_bytes, eng._cfg(b)),
               lambda eng, b: eng.forward(_x(5, (3, 32, 32))[:b].to(dev)), lambda eng, b: eng.backward((_x(5, (eng.out_ch,), 3) * 0.1)[:b].contiguous().to(dev)))


# ---------------------------------------------------------------------------------------------------------------- ResNet
def test_resnet_engine_workspace(be, dev):      # (bf16 operands; fp16: test_resnet_train_step_workspaces)
    spec = resnet.ResNetSpec(img_size=32, widths=(8, 16, 24, 32), depths=(1, 1, 1, 1), num_classes=5)

    def build():
        eng = resnet.ResNet(spec, device=dev, backend=be, seed=0).engine
        eng._buf0 = eng.buffers.clone()
        return eng

    def fwd(eng, b):
        eng.buffers.copy_(eng._buf0)               # (training mode moves the running statistics: every round starts from the same ones)
        return eng.forward(_x(5, (3, 32, 32))[:b].to(dev), training=True)

    _isolation(be, dev, build, "_ws", lambda eng, b: _need(be, be.lib.vdk_resnet_workspace_bytes, eng._cfg(b, 32)), fwd,
               lambda eng, b: eng.backward(_dl(5, eng.cp, 5, eng.op_dtype)[:b].contiguous().to(dev)))


# ---------------------------------------------------------------------------------------------------------------- whole steps
def _step_isolation(be, dev, build, state_of, ws_attr, need_engine, batch=5):
    """build() -> (step, run); one full step with the engine workspace AND the step's sum-of-squares workspace guarded, exact and pattern-filled"""
    with one_torch_thread():
        _step_rounds(be, dev, build, state_of, ws_attr, need_engine, batch)


def _step_rounds(be, dev, build, state_of, ws_attr, need_engine, batch):
    results = []
    for fill in FILLS:
        step, run = build()
        eng = step.eng
        g = _Guarded(need_engine(eng, batch), fill, dev, "engine workspace")
        attr = "_ws_t32" if getattr(eng, "precision", "") == "fp32" else "_ws"
        setattr(eng, attr, g.view); eng._ws_batch = -1
        n = C.c_size_t(0)
        be.check(be.lib.vdk_sumsq_workspace_bytes(C.byref(n)), "vdk_sumsq_workspace_bytes")
        g2 = _Guarded(int(n.value), fill, dev, "sum-of-squares workspace")
        assert getattr(step, ws_attr).numel() == n.value
        setattr(step, ws_attr, g2.view)
        run(step)
        _sync(be)
        g.check(); g2.check()
        assert getattr(eng, attr).data_ptr() == g.view.data_ptr()
        results.append({k: bits(v) for k, v in state_of(step).items() if v is not None})
    assert_same_bits(results, "across the patterns")


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
def test_fused_train_step_workspaces(be, dev, operand):
    spec = vit.VitSpec(img_size=32, patch_size=8, num_classes=10, dim=64, depth=2, heads=1, mlp_dim=128)
    x = _x(5, (3, 32, 32)); y = torch.tensor([1, 7, 3, 0, 9])

    def build():
        m = vit.VisionTransformer(spec, device=dev, backend=be, seed=0, operand=operand)
        return vit.FusedTrainStep(m, lr=0.01, label_smoothing=0.05, max_norm=1.0, ema=True, init_scale=1024.0), lambda s: s.step(x.to(dev), y.to(dev))

    _step_isolation(be, dev, build, lambda s: {"params": s.eng.params, "grads": s.eng.grads, "momentum": s.momentum_buf, "ema": s.ema, "wb16": s.eng.wb16, "loss_state": s.loss_state,
                                                "loss": s._loss_rows}, "_sumsq_ws", lambda eng, b: _need(be, be.lib.vdk_vit_workspace_bytes, eng._cfg(b)))


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
def test_resnet_train_step_workspaces(be, dev, operand):
    spec = resnet.ResNetSpec(img_size=32, widths=(8, 16, 24, 32), depths=(1, 1, 1, 1), num_classes=5)
    x = _x(5, (3, 32, 32)); y = (torch.rand(5, 5, generator=torch.Generator().manual_seed(4)) > 0.5).float()

    def build():
        m = resnet.ResNet(spec, device=dev, backend=be, seed=0, operand=operand)
        return resnet.ResNetTrainStep(m, lr=0.05, momentum=0.9, weight_decay=5e-4, loss="bce", max_norm=1.0, ema=True, init_scale=1024.0), lambda s: s.step(x.to(dev), y.to(dev))

    _step_isolation(be, dev, build, lambda s: {"params": s.eng.params, "grads": s.eng.grads, "momentum": s.momentum_buf, "ema": s.ema, "buffers": s.eng.buffers, "ema_buffers": s.ema_buffers,
                                                "loss_state": s.loss_state, "loss": s.loss_rows}, "_ws", lambda eng, b: _need(be, be.lib.vdk_resnet_workspace_bytes, eng._cfg(b, 32)))


@pytest.mark.parametrize("operand,precision", [("bf16", "bf16"), ("fp16", "bf16"), ("bf16", "fp32")])
def test_face_train_step_workspaces(be, dev, monkeypatch, operand, precision):
    monkeypatch.setitem(convnext.TIMM_CONVNEXTS, "convnext_test", dict(depths=(1, 1, 2, 1), dims=(8, 16, 24, 32)))
    cfg = {"task": "cbir", "image_size": 32, "backbone": {"timm-convnext_test": {"pretrained": False, "image_size": 32, "feat_dim": 64, "operand": operand}},
           "head": {"arcface": {"feat_dim": 64, "num_class": 40, "margin_arc": 0.35, "margin_am": 0.0, "scale": 32}}}
    x = _x(5, (3, 32, 32)); y = torch.tensor([1, 7, 33, 0, 39])

    def build():
        torch.manual_seed(0)
        model = face.get_model(cfg, None, 0, backend=be, device=dev).model
        model.train()
        return face.FaceTrainStep(model, lr=0.05, momentum=0.9, weight_decay=5e-4, max_norm=0.5, ema=True, precision=precision, init_scale=1024.0), lambda s: s.step(x.to(dev), y.to(dev))

    def need(eng, b):
        return _need(be, be.lib.vdk_convnext_train_f32_workspace_bytes if precision == "fp32" else be.lib.vdk_convnext_workspace_bytes, eng._cfg(b))

    _step_isolation(be, dev, build, lambda s: {"params": s.eng.params, "grads": s.eng.grads, "momentum": s.mom_flat, "ema": s.ema_flat, "head": s.head.weight.detach(), "loss_state": s.loss_state,
                                                "loss": s.loss_rows, **{f"small {i}": p.detach() for i, p in enumerate(s.small)}, **{f"ema small {i}": e for i, e in enumerate(s.ema_small)}},
                    "_ws", need)
