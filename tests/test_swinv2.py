"""visiondk_amd.swinv2 (SwinV2 window8_256 as autograd nodes over the kernels) against the CPU restatement tests/swinv2_ref.py, both operand formats, on the CPU SIMT
emulation and on the device.

Tiny model: img_size 64, embed 32, depths (2, 2), heads (1, 2), 10 classes, batch 2 -- maps 16 x 16 (four windows, the odd block shifted and masked) and 8 x 8 (one
window, shift forced to 0).  Every test draws norm1 / norm2 weights and biases at random, as a trained checkpoint has them: at the family's init they are zero, every
block is the identity, and a wrong attention kernel would pass.  Floor rule (as for ResNet): each quantity's relative deviation from the fp32 restatement is bounded by
2 x the deviation of the 16-bit-operand restatement from the fp32 restatement on the same weights and inputs, computed here; the 2 x covers summation order."""
import copy
import math

import pytest
import torch

from oracle import bf16ops
from tests.swinv2_ref import LOGIT_MAX, SwinV2Ref
from visiondk_amd import swinv2

TINY = dict(img_size=64, num_classes=10, embed_dim=32, depths=(2, 2), heads=(1, 2))
MODE = {"bf16": "bf16_operands", "fp16": "fp16_operands"}
LOSS_SCALE = {"bf16": 1.0, "fp16": 1024.0}
FLOOR_FACTOR = 2.0
LS_UNITS = "units of the logit_scale gradients"
F32_FLOOR = 1e-5          # quantities both sides compute in fp32 alone (the pooled head, the last norm's bias): the restatement's deviation is 0 and what is left is the
#                           summation order of fp32 sums over <= 2 x 64 x 64 terms, a few hundred 2^-24
BATCHES = 3               # every quantity is measured over three batches of two images, stacked
# A head's logit_scale gradient is ONE number per batch, tau d(tau) with d(tau) = sum dS (qn . kn) and sum_j dS_ij = 0: a sum of cancelling terms, often a hundredth of
# what went into it.  Its deviation relative to ITSELF is a draw (measured on this model, emulator, fp16: one block's three numbers 2.4e-3 in the restatement, 1.1e-3 ..
# 1.1e-2 in the engine depending only on where else in the model a tensor was rounded), so each block's logit_scale gradient is measured in units of what went into it,
# S = tau sum |dS| |qn . kn| from the fp32 restatement (tests/test_window_attention_cos.py's scale of d(tau)): e = |g - g32| / |S| over the stacked batches and the unclamped
# heads, bounded, by name, by 2 x the restatement's worst block in the same units -- tests/rowbound.py's rule (every row against the oracle's worst row).
_CACHE = {}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _trained_like(model, seed=11):
    """norms, q_bias / v_bias, logit_scale and the coordinate MLP as a trained checkpoint has them; one head's logit_scale above the clamp"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda p, s: torch.randn(p.shape, generator=g) * s
    with torch.no_grad():
        for name, p in model.named_parameters():
            if ".norm1." in name or ".norm2." in name:
                p.copy_((rn(p, 0.3) + (1.0 if name.endswith("weight") else 0.0)).to(p.device))
            elif name.endswith("q_bias") or name.endswith("v_bias"):
                p.copy_(rn(p, 0.2).to(p.device))
            elif name.endswith("logit_scale"):
                p.copy_((math.log(5.0) + torch.rand(p.shape, generator=g) * (math.log(30.0) - math.log(5.0))).to(p.device))
            elif "cpb_mlp.0" in name:
                p.copy_(rn(p, 1.0).to(p.device))
            elif "cpb_mlp.2" in name:
                p.copy_(rn(p, 0.1).to(p.device))
        model.layers[1].blocks[0].attn.logit_scale[1] = math.log(150.0)


def _ref_run(ref, x, wts, mode, scale, factors=None):
    """logits and parameter gradients (divided by the loss scale) of the restatement in `mode`"""
    ref.zero_grad()
    ref.set_drop_path(factors)
    with bf16ops.precision(mode):
        logits = ref(x)
        (logits * wts * scale).sum().backward()
    grads = {n: p.grad.detach().clone() / scale for n, p in ref.named_parameters()}
    for n, m in ref.named_modules():
        if hasattr(m, "logit_scale_grad_scale"):
            grads["scale of " + n + ".logit_scale"] = m.logit_scale_grad_scale() / scale
    return logits.detach().clone(), grads


def setup(be, dev, operand):
    key = (be.name, operand)
    if key not in _CACHE:
        model = swinv2.SwinTransformerV2(swinv2.SwinV2Spec(**TINY), device=dev, backend=be, seed=1, operand=operand)
        _trained_like(model)
        ref = SwinV2Ref(**TINY)
        ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
        g = torch.Generator().manual_seed(5)
        xs, ws = torch.randn(BATCHES, 2, 3, 64, 64, generator=g), torch.randn(BATCHES, 2, 10, generator=g)
        runs = {"fp32": [], "r16": [], "engine": []}
        model.eval()
        for x, wts in zip(xs, ws):
            runs["fp32"].append(_ref_run(ref, x, wts, "fp32", 1.0))
            runs["r16"].append(_ref_run(ref, x, wts, MODE[operand], LOSS_SCALE[operand]))
            model.zero_grad()
            logits = model(x.to(dev))
            (logits * wts.to(dev) * LOSS_SCALE[operand]).sum().backward()
            runs["engine"].append((logits.detach().cpu(), {n: p.grad.detach().cpu() / LOSS_SCALE[operand] for n, p in model.named_parameters()}))
        # one tensor per quantity: the BATCHES results stacked
        stack = lambda rs: (torch.stack([r[0] for r in rs]), {n: torch.stack([r[1][n] for r in rs]) for n in rs[0][1]})
        (l32, g32), (l16, g16), (logits, grads) = stack(runs["fp32"]), stack(runs["r16"]), stack(runs["engine"])
        scales = {n[len("scale of "):]: g32.pop(n) for n in list(g32) if n.startswith("scale of ")}
        for n in list(g16):
            if n.startswith("scale of "):
                del g16[n]
        g32[LS_UNITS] = scales
        x, wts = xs[0], ws[0]
        _CACHE[key] = (model, ref, x, wts, logits.detach().cpu(), grads, l32, g32, l16, g16)
    return _CACHE[key]


def logit_scale_errors(g, g32):
    """{name: |g - g32| / |S| over the stacked batches and the heads whose clamp passes the gradient} in units of what went into the gradient"""
    out = {}
    for n, S in g32[LS_UNITS].items():
        live = S != 0
        assert bool(live.any()), n
        out[n] = float((g[n] - g32[n])[live].double().norm() / S[live].double().norm())
    return out


def _check_logit_scales(operand, grads, g32, g16):
    e, f = logit_scale_errors(grads, g32), logit_scale_errors(g16, g32)
    worst = max(f.values())
    for n in sorted(e):
        print(f"swinv2 {operand} grad {n}: engine {e[n]:.3e} restatement {f[n]:.3e} of what went into it (restatement's worst block {worst:.3e})")
    for n in sorted(e):
        assert e[n] <= FLOOR_FACTOR * worst, (n, e[n], worst)


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
def test_swinv2_logits_and_gradients_within_twice_the_16bit_floor(be, dev, operand):
    model, ref, x, wts, logits, grads, l32, g32, l16, g16 = setup(be, dev, operand)
    e, floor = _rel(logits, l32), _rel(l16, l32)
    print(f"swinv2 {operand} logits: engine {e:.3e} floor {floor:.3e}")
    assert e <= FLOOR_FACTOR * floor, ("logits", e, floor)
    assert set(grads) == set(g16) == set(n for n, _ in model.named_parameters()) == set(g32) - {LS_UNITS}
    worst = []
    _check_logit_scales(operand, grads, g32, g16)
    for n in sorted(grads):
        if n.endswith(".logit_scale"):
            continue
        e, floor = _rel(grads[n], g32[n]), _rel(g16[n], g32[n])
        worst.append((e / max(floor, 1e-30), n, e, floor))
    worst.sort(reverse=True)
    for r, n, e, floor in worst[:8]:
        print(f"swinv2 {operand} grad {n}: engine {e:.3e} floor {floor:.3e} ratio {r:.2f}")
    for r, n, e, floor in worst:
        assert e <= FLOOR_FACTOR * floor + F32_FLOOR, (n, e, floor)


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
def test_swinv2_attention_parameter_gradients_by_name(be, dev, operand):
    """cpb_mlp.*, logit_scale, q_bias and v_bias reach the optimizer: present, finite, within the floor rule; the clamped head's logit_scale gradient exactly 0, the
    unclamped ones non-zero"""
    model, ref, x, wts, logits, grads, l32, g32, l16, g16 = setup(be, dev, operand)
    for blk in ("layers.0.blocks.0", "layers.0.blocks.1", "layers.1.blocks.0", "layers.1.blocks.1"):
        for leaf in ("cpb_mlp.0.weight", "cpb_mlp.0.bias", "cpb_mlp.2.weight", "logit_scale", "q_bias", "v_bias"):
            n = f"{blk}.attn.{leaf}"
            assert bool(torch.isfinite(grads[n]).all()) and float(grads[n].abs().max()) > 0.0, n
            if leaf != "logit_scale":
                assert _rel(grads[n], g32[n]) <= FLOOR_FACTOR * _rel(g16[n], g32[n]), n
    _check_logit_scales(operand, grads, g32, g16)
    ls = grads["layers.1.blocks.0.attn.logit_scale"].view(BATCHES, 2)
    assert float(model.layers[1].blocks[0].attn.logit_scale.detach()[1]) > LOGIT_MAX and bool((ls[:, 1] == 0.0).all()) and bool((ls[:, 0] != 0.0).all())
    assert bool((g32["layers.1.blocks.0.attn.logit_scale"].view(BATCHES, 2)[:, 1] == 0.0).all())


def test_swinv2_fp16_operands_are_closer_to_fp32_than_bf16(be, dev):
    """fp16 has 3 more mantissa bits: logits and the median gradient several times closer to the fp32 restatement (tests/test_swin.py's assertion for v1)"""
    r = {}
    for operand in ("bf16", "fp16"):
        model, ref, x, wts, logits, grads, l32, g32, l16, g16 = setup(be, dev, operand)
        errs = sorted(_rel(grads[n], g32[n]) for n in grads if not n.endswith(".logit_scale"))
        r[operand] = (_rel(logits, l32), errs[-1], errs[len(errs) // 2])
    print(r)
    assert r["fp16"][0] < 0.35 * r["bf16"][0] and r["fp16"][2] < 0.35 * r["bf16"][2], r


def test_swinv2_state_dict_round_trip_and_deepcopy(be, dev):
    model, ref = setup(be, dev, "bf16")[:2]
    sd = model.state_dict()
    assert not any(k.endswith(s) for k in sd for s in ("k_bias", "relative_coords_table", "relative_position_index", "attn_mask", "_uses"))
    fresh = SwinV2Ref(**TINY)
    fresh.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    other = swinv2.SwinTransformerV2(swinv2.SwinV2Spec(**TINY), device=dev, backend=be, seed=2)
    other.load_state_dict({k: v.to(dev) for k, v in fresh.state_dict().items()}, strict=True)
    for (n, a), (_, b) in zip(sorted(model.state_dict().items()), sorted(other.state_dict().items())):
        assert torch.equal(a.cpu(), b.cpu()), n
    ema = copy.deepcopy(model)
    assert ema.be is model.be and ema.layers[0].blocks[0].attn.qkv.weight.data_ptr() != model.layers[0].blocks[0].attn.qkv.weight.data_ptr()
    x = setup(be, dev, "bf16")[2].to(dev)
    with torch.no_grad():
        assert torch.equal(ema.eval()(x), model.eval()(x))


def test_swinv2_blocks_are_the_identity_at_init(be, dev):
    """at the reference's init (zero post-norms) forward_features = norm(downsampled patch embedding): equal to the restatement's skip path within the floor rule, and bit
    for bit independent of every block parameter"""
    spec = swinv2.SwinV2Spec(**{**TINY, "num_classes": 0})
    model = swinv2.SwinTransformerV2(spec, device=dev, backend=be, seed=3).eval()
    ref = SwinV2Ref(**{**TINY, "num_classes": 0})
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(6))

    def skip_path():
        y = ref.patch_embed(x)
        for stage in ref.layers:
            y = stage.downsample(y)
        return ref.norm(y)

    with torch.no_grad():
        f = model(x.to(dev)).cpu()
        want32 = skip_path()
        assert torch.equal(ref(x), want32)                                     # the restatement's blocks add exact zeros
        with bf16ops.precision("bf16_operands"):
            want16 = skip_path()
        assert tuple(f.shape) == (2, 8, 8, 64) and _rel(f, want32) <= FLOOR_FACTOR * _rel(want16, want32)
        for blk in model.layers[0].blocks:
            blk.attn.qkv.weight.normal_(); blk.mlp.fc1.weight.normal_(); blk.attn.logit_scale.fill_(3.0)
        assert torch.equal(model(x.to(dev)).cpu(), f)


def test_swinv2_drop_path(be, dev):
    """train mode with injected factors = the restatement with the same factors; eval ignores the rate; drawn factors are 0 or 1 / (1 - p_j), p_j = linspace(0, rate, blocks)[j]"""
    model, ref, x, wts = setup(be, dev, "fp16")[:4]
    fac = torch.tensor([[1.0, 1.0], [1.0, 0.0], [0.0, 1.25], [1.25, 1.25], [1.5, 0.0], [0.0, 0.0], [2.0, 2.0], [0.0, 2.0]])
    l32 = _ref_run(ref, x, wts, "fp32", 1.0, fac)[0]
    l16 = _ref_run(ref, x, wts, MODE["fp16"], 1.0, fac)[0]
    ref.set_drop_path(None)
    with torch.no_grad():
        model.train()
        try:
            got = model(x.to(dev), drop_path=fac.to(dev)).cpu()
            model.drop_path_rate = 0.3
            d = model.draw_drop_path(64).cpu()
        finally:
            model.eval()
        same = model(x.to(dev)).cpu()
        model.drop_path_rate = 0.0
    e, floor = _rel(got, l32), _rel(l16, l32)
    print(f"swinv2 drop-path logits: engine {e:.3e} floor {floor:.3e}")
    assert e <= FLOOR_FACTOR * floor
    assert torch.equal(same, setup(be, dev, "fp16")[4][0])                         # eval: the rate changes nothing
    p = torch.linspace(0, 0.3, 4).repeat_interleave(2)
    assert tuple(d.shape) == (8, 64) and bool((d[:2] == 1.0).all())
    for j in range(8):
        vals = set(d[j].tolist())
        assert vals <= {0.0, float(1.0 / (1.0 - p[j]))}, (j, vals)
    assert 0.0 in set(d[7].tolist())


def test_create_model_ids_and_refusals(be, dev):
    assert set(swinv2.TIMM_SWINV2S) == {"swinv2_tiny_window8_256", "swinv2_small_window8_256", "swinv2_base_window8_256"}
    for bad in ("swinv2_base_window16_256", "timm-swinv2_base_window12to16_192to256.ms_in22k_ft_in1k", "swinv2_cr_tiny_224"):
        with pytest.raises(KeyError, match="swinv2_base_window8_256"):
            swinv2.create_model(bad, device=dev, backend=be)
    with pytest.raises(RuntimeError):
        swinv2.create_model("swinv2_tiny_window8_256", pretrained=True, device=dev, backend=be)
    with pytest.raises(TypeError, match="window_size"):
        swinv2.create_model("swinv2_tiny_window8_256", window_size=16, device=dev, backend=be)
    with pytest.raises(ValueError, match="256"):
        swinv2.create_model("swinv2_tiny_window8_256", img_size=224, device=dev, backend=be)
    m = swinv2.create_model("timm-swinv2_tiny_window8_256.ms_in1k", num_classes=5, device="meta", backend=be)
    assert m.spec.embed_dim == 96 and tuple(m.spec.depths) == (2, 2, 6, 2) and tuple(m.spec.heads) == (3, 6, 12, 24) and m.drop_path_rate == 0.1
    assert m.head.fc.weight.shape == (5, 768) and [s.blocks[0].res for s in m.layers] == [64, 32, 16, 8] and m.layers[3].blocks[1].shift == 0


# ---- routing (visiondk_amd/face.py) ----------------------------------------------------------------------------------------------------------------------
def test_get_model_routes_swinv2_ids(be, dev):
    """`name: timm-swinv2_base_window8_256.ms_in1k` (an alternative the reference's yamls list) -> VisionWrapper -> swinv2.create_model; construction only, on the meta
    device; the window-16 id is a KeyError with the served list"""
    from visiondk_amd import face
    cfg = {"task": "classification", "name": "timm-swinv2_base_window8_256.ms_in1k", "image_size": 256, "num_classes": 5, "pretrained": True}
    m = face.get_model(cfg, None, 0, backend=be, device="meta").model
    assert isinstance(m, swinv2.SwinTransformerV2) and m.spec.embed_dim == 128 and tuple(m.spec.depths) == (2, 2, 18, 2) and tuple(m.spec.heads) == (4, 8, 16, 32)
    assert m.spec.img_size == 256 and m.head.fc.weight.shape == (5, 1024) and m.drop_path_rate == 0.1
    with pytest.raises(KeyError, match="swinv2_base_window8_256"):
        face.get_model({**cfg, "name": "timm-swinv2_base_window16_256.ms_in1k"}, None, 0, backend=be, device="meta")
    with pytest.raises(NotImplementedError, match="swinv2_tiny_window8_256"):
        face.TimmWrapper("swinv3_nano", feat_dim=8, image_size=256, pretrained=False, backend=be, device="meta")


def test_face_model_with_a_swinv2_backbone(be, dev, monkeypatch):
    """a cbir config with the tiny spec: FaceTrainingModel forward and backward through the neck (BatchNorm2d over the NHWC map's row index, Flatten, Linear, BatchNorm1d)
    and ArcFace; the embedding against the same module sequence in torch on the restatement's map within the floor rule; FusedTrainStep / FaceTrainStep / forward_precise
    refuse the model and name the follow-up"""
    from visiondk_amd import face, vit
    monkeypatch.setitem(swinv2.TIMM_SWINV2S, "swinv2_test_window8_256", dict(embed_dim=32, depths=(1, 1, 1, 1), heads=(1, 2, 4, 8)))
    torch.manual_seed(0)
    cfg = {"task": "cbir", "image_size": 256, "load_from": None,
           "backbone": {"timm-swinv2_test_window8_256.ms_in1k": {"pretrained": False, "image_size": 256, "feat_dim": 64}},
           "head": {"arcface": {"feat_dim": 64, "num_class": 24, "margin_arc": 0.35, "margin_am": 0.0, "scale": 32}}}
    model = face.get_model(cfg, None, 0, backend=be, device=dev).model.train()
    w = model.trainingwrapper["backbone"]
    assert isinstance(w.model, swinv2.SwinTransformerV2) and w.is_cnn and w.operand == "fp16" and w.model.operand == "fp16"
    assert isinstance(w.output_layer[0], torch.nn.BatchNorm2d) and w.output_layer[0].num_features == 8 and w.output_layer[2].weight.shape == (64, 8 * 8 * 256)
    _trained_like(w.model)
    w.model.drop_path_rate = 0.0
    ref = SwinV2Ref(img_size=256, num_classes=0, embed_dim=32, depths=(1, 1, 1, 1), heads=(1, 2, 4, 8))
    ref.load_state_dict({k: v.detach().cpu() for k, v in w.model.state_dict().items()}, strict=True)
    neck = copy.deepcopy(w.output_layer).cpu().train()
    x = torch.randn(4, 3, 256, 256, generator=torch.Generator().manual_seed(2))          # (four images: a train-mode BatchNorm over two is a sign function)
    labels = torch.tensor([1, 5, 7, 23])
    emb = w(x.to(dev))
    def neck16(f):                                   # the neck as the wrapper runs it in a 16-bit mode: BatchNorm2d, Flatten, the Linear on 16-bit operands, BatchNorm1d
        n16 = copy.deepcopy(w.output_layer).cpu().train()
        return n16[3](bf16ops.linear(n16[1](n16[0](f)), n16[2].weight, n16[2].bias))

    with torch.no_grad():
        e32 = neck(ref(x))
        with bf16ops.precision("fp16_operands"):
            e16 = neck16(ref(x))
    e, floor = _rel(emb.detach().cpu(), e32), _rel(e16, e32)
    print(f"swinv2 cbir embedding: engine {e:.3e} floor {floor:.3e}")
    assert emb.shape == (4, 64) and e <= FLOOR_FACTOR * floor
    out = model(x.to(dev), labels.to(dev))
    loss = torch.nn.functional.cross_entropy(out.float(), labels.to(dev))
    loss.backward()
    grads = [p.grad for p in w.model.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and sum(float(g.abs().sum()) for g in grads) > 0.0
    for make in (lambda: vit.FusedTrainStep(w.model, lr=0.01), lambda: face.FaceTrainStep(model, lr=0.01), lambda: w.forward_precise(x.to(dev))):
        with pytest.raises(NotImplementedError, match="vdk_swinv2"):
            make()
