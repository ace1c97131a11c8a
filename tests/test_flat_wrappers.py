"""The contract of visiondk_amd._engine (FlatEngine / FlatParamModule), pinned on each of the four native models that are built on it: the smallest spec of each family
that tests/test_workspace_isolation.py builds, batch 2, on the CPU emulation and on the device.  Forwards are compared bit for bit: they are the same kernels on the same
values, in the same order."""
import copy

import pytest
import torch

from visiondk_amd import convnext, resnet, swin, vit

_SPECS = {
    "vit": (vit.VisionTransformer, vit.VitSpec(img_size=32, patch_size=8, num_classes=10, dim=64, depth=2, heads=1, mlp_dim=128), 32),
    "swin": (swin.SwinTransformer, swin.SwinSpec(img_size=224, num_classes=5, embed_dim=32, depths=(1, 1), heads=(1, 2)), 224),
    "convnext": (convnext.ConvNeXt, convnext.ConvNeXtSpec(img_size=32, depths=(1, 1, 2, 1), dims=(8, 16, 24, 32), num_classes=0), 32),
    "resnet": (resnet.ResNet, resnet.ResNetSpec(img_size=32, widths=(8, 16, 24, 32), depths=(1, 1, 1, 1), num_classes=5), 32),
}
FAMILY = {"vit": "ViT", "swin": "Swin", "convnext": "ConvNeXt", "resnet": "ResNet"}
WORKSPACES = ("_ws", "_ws32", "_ws_t32")
families = pytest.mark.parametrize("family", list(_SPECS))


def _model(family, be, dev, seed=0):
    cls, spec, _ = _SPECS[family]
    return cls(spec, device=dev, backend=be, seed=seed).eval()      # eval: ResNet's forward then leaves its running statistics alone


def _x(family, dev):
    s = _SPECS[family][2]
    return torch.randn(2, 3, s, s, generator=torch.Generator().manual_seed(3)).to(dev)


def _out(model, x):
    with torch.no_grad():
        y = model(x).clone()
    if x.is_cuda:
        torch.cuda.synchronize()
    return y


def _assert_views(model):
    """every Parameter (and, for ResNet, every running statistic) is a view into the engine's flat buffer"""
    eng = model.engine
    for (name, off, numel, shape), (n2, p) in zip(eng.entries, model._plist):
        assert name == n2 and tuple(p.shape) == tuple(shape)
        assert p.data_ptr() == eng.params.data_ptr() + 4 * off, name
    for name, off, numel, shape, m, bn in getattr(model, "_blist", []):
        assert getattr(m, bn).data_ptr() == eng.buffers.data_ptr() + 4 * off, name


@families
def test_deepcopy_is_independent(be, dev, family):
    model = _model(family, be, dev)
    x = _x(family, dev)
    y = _out(model, x)
    twin = copy.deepcopy(model)              # ModelEMA does this
    assert twin.engine is not model.engine and twin.engine.be is model.engine.be
    y2 = _out(twin, x)
    assert torch.equal(y2, y)
    _assert_views(twin)
    assert twin.engine.params.data_ptr() != model.engine.params.data_ptr()
    before = model.engine.params.clone()
    with torch.no_grad():
        twin._plist[0][1].add_(1.0)
    assert torch.equal(model.engine.params, before)
    assert not torch.equal(twin.engine.params, before)
    assert torch.equal(_out(model, x), y)


@families
def test_dtype_and_device_rules(be, dev, family):
    model = _model(family, be, dev)
    ptr = model.engine.params.data_ptr()
    assert model.float() is model and model.engine.params.data_ptr() == ptr
    _assert_views(model)
    with pytest.raises(RuntimeError, match=f"visiondk_amd {FAMILY[family]} keeps fp32 master weights; bf16 copies are internal"):
        model.half()
    if be.device_only:
        with pytest.raises(RuntimeError, match=f"visiondk_amd {FAMILY[family]} lives on the GPU \\(no CPU fallback\\)"):
            model.to("cpu")
    else:
        assert model.to("cpu") is model
    assert model.engine.params.data_ptr() == ptr and model.engine.params.dtype == torch.float32
    _assert_views(model)


@families
def test_repointed_parameter_and_load_state_dict(be, dev, family):
    a, b = _model(family, be, dev), _model(family, be, dev)
    x = _x(family, dev)
    y0 = _out(a, x)
    assert torch.equal(_out(b, x), y0)
    k = 0                                      # the first tensor of the flat buffer (the stem's weight, ViT's class token): every output depends on it
    new = (a._plist[k][1].detach() + 0.05 * torch.randn(a._plist[k][1].shape, generator=torch.Generator().manual_seed(9)).to(dev)).clone()
    with torch.no_grad():
        b._plist[k][1].copy_(new)              # the plain way: written into the flat buffer
    p = a._plist[k][1]
    p.data = new.clone()                       # re-pointed: the next forward copies it back into the flat buffer
    assert p.data_ptr() != a.engine.params.data_ptr() + 4 * a.engine.entries[k][1]
    ya = _out(a, x)
    assert torch.equal(ya, _out(b, x)) and not torch.equal(ya, y0)
    _assert_views(a)
    c = _model(family, be, dev, seed=5)
    assert not torch.equal(_out(c, x), ya)
    c.load_state_dict(b.state_dict(), strict=True)
    assert torch.equal(_out(c, x), ya)
    _assert_views(c)


@families
def test_state_dict_names(be, dev, family):
    model = _model(family, be, dev)
    eng = model.engine
    names = [e[0] for e in eng.entries]
    assert [n for n, _ in model.named_parameters()] == names
    want = set(names)
    if family == "resnet":
        stats = [e[0] for e in eng.buffer_entries]
        assert stats and all(n.rsplit(".", 1)[1] in ("running_mean", "running_var") for n in stats)
        want |= set(stats) | {n.rsplit(".", 1)[0] + ".num_batches_tracked" for n in stats}
    assert set(model.state_dict()) == want
    for n in names:
        assert eng.view(eng.params, n).data_ptr() == dict(model._plist)[n].data_ptr()


def _fill_workspaces(family, model, x):
    """every workspace the family has: forward_precise's, the training forward's, and ConvNeXt's fp32-training one"""
    eng = model.engine
    model.train()
    if hasattr(model, "forward_precise"):
        model.forward_precise(x)
    model(x)
    if family == "convnext":
        eng.precision = "fp32"
        model(x)
        eng.precision = "bf16"
    held = {"vit": ("_ws", "_ws32"), "swin": ("_ws", "_ws32"), "convnext": WORKSPACES, "resnet": ("_ws",)}[family]
    for attr in WORKSPACES:
        assert (getattr(eng, attr) is not None) == (attr in held), attr
    return held


@families
def test_apply_without_a_move_keeps_the_workspaces(be, dev, family):
    """fn leaves its argument on the engine's own torch.device (on the emulation: cpu to cpu): nothing is dropped"""
    model = _model(family, be, "cuda:0" if be.device_only else "cpu")
    eng = model.engine
    x = _x(family, eng.device)
    held = _fill_workspaces(family, model, x)
    ptrs = {attr: getattr(eng, attr).data_ptr() for attr in held}
    batch, version = eng._ws_batch, eng._weights_version
    model._apply(lambda t: t.to(eng.device))
    assert {attr: getattr(eng, attr).data_ptr() for attr in held} == ptrs
    assert eng._ws_batch == batch and eng._weights_version == version and version is not None
    _assert_views(model)


def _move_and_check(family, model, x, other):
    """the engine goes to `other`: every buffer is there, every workspace is gone, and a forward on the new device gives what the old one gave"""
    _fill_workspaces(family, model, x)
    y = _out(model.eval(), x)
    model._apply(lambda t: t.to(other))
    eng = model.engine
    assert eng.device == other
    for attr in WORKSPACES:
        assert getattr(eng, attr) is None, attr
    assert eng._ws_batch == -1 and eng._weights_version is None
    for attr in ("params", "grads", "wb16") + eng._derived:
        assert getattr(eng, attr).device == other, attr
    _assert_views(model)
    with torch.cuda.device(other):
        y2 = _out(model, x.to(other))
        if hasattr(model, "forward_precise"):
            model.forward_precise(x.to(other))
        torch.cuda.synchronize()
    assert torch.equal(y2.cpu(), y.cpu())


@pytest.mark.gpu
@families
def test_move_to_another_name_of_the_device_drops_every_workspace(hip, family):
    """torch.device("cuda") -> torch.device("cuda:0"): the same GPU under another torch.device, which the wrapper treats as a move (one GPU is enough for this leg)"""
    _move_and_check(family, _model(family, hip, "cuda"), _x(family, "cuda"), torch.device("cuda:0"))


@pytest.mark.gpu
@families
def test_move_to_another_gpu_drops_every_workspace(hip, family):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs: the move is cuda:0 -> cuda:1")
    _move_and_check(family, _model(family, hip, "cuda:0"), _x(family, "cuda:0"), torch.device("cuda:1"))
