"""visiondk_amd.dinov2 (DINOv2 ViT-S/B/L/14 as autograd nodes over the kernels) against the CPU restatement tests/dinov2_ref.py, both operand formats, on the CPU SIMT
emulation and on the device.

Tiny model: img_size 70 (5 x 5 patches + the class token = 26 tokens), dim 128, depth 2, heads 2, mlp 512, 10 classes, batch 2.  Weights as a trained checkpoint has them:
LayerNorms and biases random, every LayerScale gamma uniform in [0.05, 1] with a random sign -- except block 1's ls1.gamma, which stays at the family's init 1e-5, so that
the gradient of a 1e-5 gamma and of the branch behind it (whose incoming gradient is 1e-5 x the stream's, subnormal in fp16 under the loss scale of 1024) is measured too.
Floor rule (tests/test_swinv2.py's): each quantity's relative deviation from the fp32 restatement is bounded by 2 x the deviation of the 16-bit-operand restatement from the
fp32 restatement on the same weights and inputs, computed here; the 2 x covers summation order.  Whatever the restatement measures is the floor -- also for the fp16 gradients
behind the 1e-5 gamma."""
import copy

import pytest
import torch

from oracle import bf16ops
from tests.dinov2_ref import Dinov2Ref
from visiondk_amd import dinov2

TINY = dict(img_size=70, num_classes=10, dim=128, depth=2, heads=2, mlp_dim=512)
MODE = {"bf16": "bf16_operands", "fp16": "fp16_operands"}
LOSS_SCALE = {"bf16": 1.0, "fp16": 1024.0}
FLOOR_FACTOR = 2.0
F32_FLOOR = 1e-5          # quantities both sides compute in fp32 alone (the head on the normed class token, the last norm's bias): the restatement's deviation is 0 and what
#                           is left is the summation order of short fp32 sums
BATCHES = 3               # every quantity is measured over three batches of two images, stacked
TINY_GAMMA = "blocks.1.ls1.gamma"
_CACHE = {}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _trained_like(model, seed=11, keep=TINY_GAMMA):
    g = torch.Generator().manual_seed(seed)
    rn = lambda p, s: torch.randn(p.shape, generator=g) * s
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name == keep:
                continue
            if "norm" in name:
                p.copy_((rn(p, 0.3) + (1.0 if name.endswith("weight") else 0.0)).to(p.device))
            elif name.endswith(".gamma"):
                p.copy_(((0.05 + 0.95 * torch.rand(p.shape, generator=g)) * (torch.randint(0, 2, p.shape, generator=g) * 2.0 - 1.0)).to(p.device))
            elif name == "cls_token":
                p.copy_(rn(p, 0.02).to(p.device))
            elif p.dim() == 1:
                p.copy_(rn(p, 0.1).to(p.device))


def _ref_run(ref, x, wts, mode, scale):
    """logits and parameter gradients (divided by the loss scale) of the restatement in `mode`"""
    ref.zero_grad()
    with bf16ops.precision(mode):
        logits = ref(x)
        (logits * wts * scale).sum().backward()
    return logits.detach().clone(), {n: p.grad.detach().clone() / scale for n, p in ref.named_parameters()}


def setup(be, dev, operand):
    key = (be.name, operand)
    if key not in _CACHE:
        model = dinov2.DinoVisionTransformer(dinov2.Dinov2Spec(**TINY), device=dev, backend=be, seed=1, operand=operand)
        _trained_like(model)
        ref = Dinov2Ref(**TINY)
        ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
        g = torch.Generator().manual_seed(5)
        xs, ws = torch.randn(BATCHES, 2, 3, 70, 70, generator=g), torch.randn(BATCHES, 2, 10, generator=g)
        runs = {"fp32": [], "r16": [], "engine": []}
        model.eval()
        for x, wts in zip(xs, ws):
            runs["fp32"].append(_ref_run(ref, x, wts, "fp32", 1.0))
            runs["r16"].append(_ref_run(ref, x, wts, MODE[operand], LOSS_SCALE[operand]))
            model.zero_grad()
            logits = model(x.to(dev))
            (logits * wts.to(dev) * LOSS_SCALE[operand]).sum().backward()
            runs["engine"].append((logits.detach().cpu(), {n: p.grad.detach().cpu() / LOSS_SCALE[operand] for n, p in model.named_parameters()}))
        stack = lambda rs: (torch.stack([r[0] for r in rs]), {n: torch.stack([r[1][n] for r in rs]) for n in rs[0][1]})
        (l32, g32), (l16, g16), (logits, grads) = stack(runs["fp32"]), stack(runs["r16"]), stack(runs["engine"])
        _CACHE[key] = (model, ref, xs[0], ws[0], logits, grads, l32, g32, l16, g16)
    return _CACHE[key]


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
def test_dinov2_logits_and_gradients_within_twice_the_16bit_floor(be, dev, operand):
    model, ref, x, wts, logits, grads, l32, g32, l16, g16 = setup(be, dev, operand)
    e, floor = _rel(logits, l32), _rel(l16, l32)
    print(f"dinov2 {operand} logits: engine {e:.3e} floor {floor:.3e}")
    assert e <= FLOOR_FACTOR * floor, ("logits", e, floor)
    assert set(grads) == set(g16) == set(g32) == set(n for n, _ in model.named_parameters())
    worst = []
    for n in sorted(grads):
        e, floor = _rel(grads[n], g32[n]), _rel(g16[n], g32[n])
        worst.append((e / max(floor, 1e-30), n, e, floor))
    worst.sort(reverse=True)
    for r, n, e, floor in worst[:8]:
        print(f"dinov2 {operand} grad {n}: engine {e:.3e} floor {floor:.3e} ratio {r:.2f}")
    for r, n, e, floor in worst:
        assert e <= FLOOR_FACTOR * floor + F32_FLOOR, (n, e, floor)


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
def test_dinov2_gradients_of_and_behind_the_tiny_gamma(be, dev, operand):
    """block 1's ls1.gamma = 1e-5: its own gradient (sum dy h, no gamma in it: as large as any other gamma's) and those of the attention branch behind it (1e-5 x the
    stream's gradient) are present, finite, non-zero and within the floor rule, by name; every LayerScale gamma reaches the optimizer"""
    model, ref, x, wts, logits, grads, l32, g32, l16, g16 = setup(be, dev, operand)
    assert bool((model.blocks[1].ls1.gamma.detach().cpu() == 1e-5).all()) and float(model.blocks[1].ls2.gamma.detach().abs().min()) >= 0.05
    names = [TINY_GAMMA] + [f"blocks.1.{m}.{leaf}" for m in ("attn.proj", "attn.qkv", "norm1") for leaf in ("weight", "bias")]
    for n in names:
        e, floor = _rel(grads[n], g32[n]), _rel(g16[n], g32[n])
        print(f"dinov2 {operand} grad {n}: engine {e:.3e} floor {floor:.3e} |g32| {float(g32[n].norm()):.3e}")
        assert bool(torch.isfinite(grads[n]).all()) and float(grads[n].abs().max()) > 0.0, n
        assert e <= FLOOR_FACTOR * floor + F32_FLOOR, (n, e, floor)
    # behind the 1e-5 gamma the gradient is 1e-5-class: five orders below the same tensor's in block 0
    assert float(g32["blocks.1.attn.proj.weight"].norm()) < 1e-3 * float(g32["blocks.0.attn.proj.weight"].norm())
    for i in (0, 1):
        for ls in ("ls1", "ls2"):
            n = f"blocks.{i}.{ls}.gamma"
            assert float(grads[n].abs().max()) > 0.0 and _rel(grads[n], g32[n]) <= FLOOR_FACTOR * _rel(g16[n], g32[n]) + F32_FLOOR, n


def test_dinov2_fp16_operands_are_closer_to_fp32_than_bf16(be, dev):
    r = {}
    for operand in ("bf16", "fp16"):
        model, ref, x, wts, logits, grads, l32, g32, l16, g16 = setup(be, dev, operand)
        errs = sorted(_rel(grads[n], g32[n]) for n in grads if not n.startswith("blocks.1.attn") and not n.startswith("blocks.1.norm1"))
        r[operand] = (_rel(logits, l32), errs[-1], errs[len(errs) // 2])
    print(r)
    assert r["fp16"][0] < 0.35 * r["bf16"][0] and r["fp16"][2] < 0.35 * r["bf16"][2], r


def test_dinov2_state_dict_round_trip_and_deepcopy(be, dev):
    model, ref = setup(be, dev, "bf16")[:2]
    sd = model.state_dict()
    assert set(sd) == set(ref.state_dict()) and sd["pos_embed"].shape == (1, 26, 128) and sd["blocks.0.ls1.gamma"].shape == (128,)
    fresh = Dinov2Ref(**TINY)
    fresh.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    other = dinov2.DinoVisionTransformer(dinov2.Dinov2Spec(**TINY), device=dev, backend=be, seed=2)
    other.load_state_dict({k: v.to(dev) for k, v in fresh.state_dict().items()}, strict=True)
    for (n, a), (_, b) in zip(sorted(model.state_dict().items()), sorted(other.state_dict().items())):
        assert torch.equal(a.cpu(), b.cpu()), n
    ema = copy.deepcopy(model)
    assert ema.be is model.be and ema.blocks[0].attn.qkv.weight.data_ptr() != model.blocks[0].attn.qkv.weight.data_ptr()
    x = setup(be, dev, "bf16")[2].to(dev)
    with torch.no_grad():
        assert torch.equal(ema.eval()(x), model.eval()(x))


def test_dinov2_init_and_feature_modes(be, dev):
    """reset_parameters leaves every gamma at 1e-5, LayerNorms at 1 / 0, Linear biases at 0; num_classes = 0 gives the normed class token, with global_pool = '' the normed
    tokens [B, 26, D], both within the floor rule of the restatement"""
    kw = {**TINY, "num_classes": 0}
    model = dinov2.DinoVisionTransformer(dinov2.Dinov2Spec(**kw, global_pool=""), device=dev, backend=be, seed=3).eval()
    for n, p in model.named_parameters():
        if n.endswith(".gamma"):
            assert bool((p.detach().cpu() == 1e-5).all()), n
        elif "norm" in n:
            assert bool((p.detach() == (1.0 if n.endswith("weight") else 0.0)).all()), n
        elif n.endswith(".bias") and n != "patch_embed.proj.bias":          # (the Conv2d bias keeps torch's default init: the override zeroes Linear biases only)
            assert float(p.detach().abs().max()) == 0.0, n
    assert 0.015 < float(model.blocks[1].mlp.fc2.weight.detach().std()) < 0.025 and 0.0 < float(model.cls_token.detach().abs().max()) < 1e-4
    _trained_like(model, keep=None)
    ref = Dinov2Ref(**kw, global_pool="")
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    x = torch.randn(2, 3, 70, 70, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        f = model(x.to(dev)).cpu()
        want32 = ref(x)
        with bf16ops.precision("bf16_operands"):
            want16 = ref(x)
        assert tuple(f.shape) == (2, 26, 128) and _rel(f, want32) <= FLOOR_FACTOR * _rel(want16, want32)
        tok = dinov2.DinoVisionTransformer(dinov2.Dinov2Spec(**kw), device=dev, backend=be, seed=3).eval()
        tok.load_state_dict(model.state_dict(), strict=True)
        t = tok(x.to(dev)).cpu()
        assert tuple(t.shape) == (2, 128) and torch.equal(t, f[:, 0])


def test_create_model_ids_and_refusals(be, dev):
    assert set(dinov2.TIMM_DINOV2S) == {"vit_small_patch14_dinov2", "vit_base_patch14_dinov2", "vit_large_patch14_dinov2"}
    for bad in ("vit_giant_patch14_dinov2", "timm-vit_large_patch14_reg4_dinov2.lvd142m", "vit_small_patch14_reg4_dinov2", "vit_large_patch16_dinov3"):
        with pytest.raises(KeyError, match="vit_large_patch14_dinov2"):
            dinov2.create_model(bad, device=dev, backend=be)
    with pytest.raises(RuntimeError):
        dinov2.create_model("vit_small_patch14_dinov2", pretrained=True, device=dev, backend=be)
    with pytest.raises(TypeError, match="init_values"):
        dinov2.create_model("vit_small_patch14_dinov2", init_values=1.0, device=dev, backend=be)
    with pytest.raises(ValueError, match="14"):
        dinov2.create_model("vit_small_patch14_dinov2", img_size=224 + 8, device=dev, backend=be)
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        dinov2.create_model("vit_small_patch14_dinov2", drop_path_rate=0.1, device=dev, backend=be)
    with pytest.raises(ValueError, match="global_pool"):
        dinov2.create_model("vit_small_patch14_dinov2", global_pool="avg", device=dev, backend=be)
    with pytest.raises(ValueError, match="global_pool"):
        dinov2.create_model("vit_small_patch14_dinov2", global_pool="", device=dev, backend=be)
    m = dinov2.create_model("timm-vit_large_patch14_dinov2.lvd142m", num_classes=5, device="meta", backend=be)
    s = m.spec
    assert (s.dim, s.depth, s.heads, s.mlp_dim, s.img_size, s.patch_size, s.ln_eps, s.init_values) == (1024, 24, 16, 4096, 518, 14, 1e-6, 1e-5)
    assert m.pos_embed.shape == (1, 1370, 1024) and m.head.weight.shape == (5, 1024) and m.blocks[23].ls2.gamma.shape == (1024,) and m.tokens == 1370
    for name, want in (("vit_small_patch14_dinov2", (384, 12, 6, 1536)), ("vit_base_patch14_dinov2", (768, 12, 12, 3072))):
        s = dinov2.create_model(name, img_size=224, num_classes=0, global_pool="", device="meta", backend=be).spec
        assert (s.dim, s.depth, s.heads, s.mlp_dim) == want and s.global_pool == "" and s.img_size == 224


# ---- routing (visiondk_amd/face.py) ----------------------------------------------------------------------------------------------------------------------
def test_get_model_routes_dinov2_ids(be, dev):
    """`name: timm-vit_large_patch14_dinov2.lvd142m` (the drop-in backbone the reference's yamls list, imgsz 518) -> VisionWrapper -> dinov2.create_model; construction only,
    on the meta device; the giant and reg4 ids are a KeyError with the served list"""
    from visiondk_amd import face
    cfg = {"task": "classification", "name": "timm-vit_large_patch14_dinov2.lvd142m", "image_size": 518, "num_classes": 5, "pretrained": True}
    m = face.get_model(cfg, None, 0, backend=be, device="meta").model
    assert isinstance(m, dinov2.DinoVisionTransformer) and (m.spec.dim, m.spec.depth, m.spec.heads, m.spec.img_size) == (1024, 24, 16, 518)
    assert m.head.weight.shape == (5, 1024) and m.pos_embed.shape == (1, 1370, 1024)
    for bad in ("timm-vit_giant_patch14_dinov2.lvd142m", "timm-vit_base_patch14_reg4_dinov2.lvd142m"):
        with pytest.raises(KeyError, match="vit_large_patch14_dinov2"):
            face.get_model({**cfg, "name": bad}, None, 0, backend=be, device="meta")
    with pytest.raises(NotImplementedError, match="vit_small_patch14_dinov2"):
        face.TimmWrapper("vit_giant_patch14_dinov2", feat_dim=8, image_size=518, pretrained=False, backend=be, device="meta")


def test_face_model_with_a_dinov2_backbone(be, dev, monkeypatch):
    """a cbir config with the tiny spec: FaceTrainingModel forward and backward through the transformer neck (LayerNorm, Flatten, Linear(N D, feat_dim), BatchNorm1d) and
    ArcFace; the embedding against the same module sequence in torch on the restatement's tokens within the floor rule; FusedTrainStep / FaceTrainStep / forward_precise
    refuse the model and name the follow-up"""
    from visiondk_amd import face, vit
    monkeypatch.setitem(dinov2.TIMM_DINOV2S, "vit_test_patch14_dinov2", dict(dim=128, depth=2, heads=2, mlp_dim=512))
    torch.manual_seed(0)
    cfg = {"task": "cbir", "image_size": 70, "load_from": None,
           "backbone": {"timm-vit_test_patch14_dinov2.lvd142m": {"pretrained": False, "image_size": 70, "feat_dim": 64}},
           "head": {"arcface": {"feat_dim": 64, "num_class": 24, "margin_arc": 0.35, "margin_am": 0.0, "scale": 32}}}
    model = face.get_model(cfg, None, 0, backend=be, device=dev).model.train()
    w = model.trainingwrapper["backbone"]
    assert isinstance(w.model, dinov2.DinoVisionTransformer) and not w.is_cnn and w.operand == "fp16" and w.model.operand == "fp16" and w.model.spec.global_pool == ""
    assert isinstance(w.output_layer[0], torch.nn.LayerNorm) and w.output_layer[2].weight.shape == (64, 26 * 128)
    _trained_like(w.model)
    ref = Dinov2Ref(img_size=70, num_classes=0, dim=128, depth=2, heads=2, mlp_dim=512, global_pool="")
    ref.load_state_dict({k: v.detach().cpu() for k, v in w.model.state_dict().items()}, strict=True)
    neck = copy.deepcopy(w.output_layer).cpu().train()
    x = torch.randn(4, 3, 70, 70, generator=torch.Generator().manual_seed(2))          # (four images: a train-mode BatchNorm over two is a sign function)
    labels = torch.tensor([1, 5, 7, 23])
    emb = w(x.to(dev))

    def neck16(f):                                   # the neck as the wrapper runs it in a 16-bit mode: LayerNorm, Flatten, the Linear on 16-bit operands, BatchNorm1d
        n16 = copy.deepcopy(w.output_layer).cpu().train()
        return n16[3](bf16ops.linear(n16[1](n16[0](f)), n16[2].weight, n16[2].bias))

    with torch.no_grad():
        e32 = neck(ref(x))
        with bf16ops.precision("fp16_operands"):
            e16 = neck16(ref(x))
    e, floor = _rel(emb.detach().cpu(), e32), _rel(e16, e32)
    print(f"dinov2 cbir embedding: engine {e:.3e} floor {floor:.3e}")
    assert emb.shape == (4, 64) and e <= FLOOR_FACTOR * floor
    out = model(x.to(dev), labels.to(dev))
    loss = torch.nn.functional.cross_entropy(out.float(), labels.to(dev))
    loss.backward()
    grads = {n: p.grad for n, p in w.model.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values()) and all(float(grads[f"blocks.{i}.{ls}.gamma"].abs().sum()) > 0.0 for i in (0, 1)
                                                                                                 for ls in ("ls1", "ls2"))
    for make in (lambda: vit.FusedTrainStep(w.model, lr=0.01), lambda: face.FaceTrainStep(model, lr=0.01), lambda: w.forward_precise(x.to(dev))):
        with pytest.raises(NotImplementedError, match="LayerScale mode of the native vdk_vit"):
            make()
