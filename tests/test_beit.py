"""visiondk_amd.beit (BEiT / BEiT-v2 B/L patch16_224 as autograd nodes over the kernels) against the CPU restatement tests/beit_ref.py, both operand formats, on the CPU
SIMT emulation and on the device.

Tiny model: img_size 96 (6 x 6 patches + the class token = 37 tokens), dim 128, 2 heads, depth 2, 10 classes, batch 2.  Weights as a trained checkpoint has them
(tests/test_beit_ref.trained_like): random non-zero relative position tables, gammas in +-[0.1, 1], random q / v biases and norm affine -- at init the tables are zero and
an attention kernel without the bias would pass.
Floor rule (tests/test_swinv2.py's): each quantity's relative deviation from the fp32 restatement is bounded by 2 x the deviation of the 16-bit-operand restatement from
the fp32 restatement on the same weights and inputs, computed here; the 2 x covers summation order.

On the parent commit visiondk_amd.beit does not exist: the module's import fails and every test here with it."""
import copy

import pytest
import torch

from oracle import bf16ops
from tests.beit_ref import BeitRef
from tests.test_beit_ref import trained_like
from visiondk_amd import beit

TINY = dict(img_size=96, num_classes=10, dim=128, depth=2, heads=2)
MODE = {"bf16": "bf16_operands", "fp16": "fp16_operands"}
LOSS_SCALE = {"bf16": 1.0, "fp16": 1024.0}
FLOOR_FACTOR = 2.0
F32_FLOOR = 1e-5          # quantities both sides compute in fp32 alone (the head on the pooled, normed features): the restatement's deviation is 0 there
BATCHES = 3               # every quantity is measured over three batches of two images, stacked
_CACHE = {}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _ref_run(ref, x, wts, mode, scale):
    ref.zero_grad()
    with bf16ops.precision(mode):
        logits = ref(x)
        (logits * wts * scale).sum().backward()
    return logits.detach().clone(), {n: p.grad.detach().clone() / scale for n, p in ref.named_parameters()}


def setup(be, dev, operand):
    key = (be.name, operand)
    if key not in _CACHE:
        model = beit.Beit(beit.BeitSpec(**TINY), device=dev, backend=be, seed=1, operand=operand)
        trained_like(model, seed=11)
        ref = BeitRef(**TINY)
        ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
        g = torch.Generator().manual_seed(5)
        xs, ws = torch.randn(BATCHES, 2, 3, 96, 96, generator=g), torch.randn(BATCHES, 2, 10, generator=g)
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
def test_beit_logits_and_gradients_within_twice_the_16bit_floor(be, dev, operand):
    model, ref, x, wts, logits, grads, l32, g32, l16, g16 = setup(be, dev, operand)
    e, floor = _rel(logits, l32), _rel(l16, l32)
    print(f"beit {operand} logits: engine {e:.3e} floor {floor:.3e}")
    assert e <= FLOOR_FACTOR * floor, ("logits", e, floor)
    assert set(grads) == set(g16) == set(g32) == set(n for n, _ in model.named_parameters())
    worst = []
    for n in sorted(grads):
        e, floor = _rel(grads[n], g32[n]), _rel(g16[n], g32[n])
        worst.append((e / max(floor, 1e-30), n, e, floor))
    worst.sort(reverse=True)
    for r, n, e, floor in worst[:8]:
        print(f"beit {operand} grad {n}: engine {e:.3e} floor {floor:.3e} ratio {r:.2f}")
    for r, n, e, floor in worst:
        assert e <= FLOOR_FACTOR * floor + F32_FLOOR, (n, e, floor)


@pytest.mark.parametrize("operand", ["bf16", "fp16"])
def test_beit_table_gradients_by_name(be, dev, operand):
    """the relative position tables' gradients (attention backward's d(bias) through the gather's backward), the q / v biases' and the gammas': present, finite, non-zero in
    every row the index uses -- the three class-token rows included, except where the pooling cuts the class query off -- and within the floor rule"""
    model, ref, x, wts, logits, grads, l32, g32, l16, g16 = setup(be, dev, operand)
    for i in (0, 1):
        n = f"blocks.{i}.attn.relative_position_bias_table"
        e, floor = _rel(grads[n], g32[n]), _rel(g16[n], g32[n])
        print(f"beit {operand} grad {n}: engine {e:.3e} floor {floor:.3e} |g32| {float(g32[n].norm()):.3e}")
        assert grads[n].shape == (BATCHES, 11 * 11 + 3, 2) and bool(torch.isfinite(grads[n]).all())
        live = grads[n].abs().amax(dim=(0, 2)) > 0.0
        if i == 1:           # the mean pooling leaves the class token's output row of the LAST block out: its query rows of the table (R - 3 and R - 1) get exactly 0
            assert not bool(live[-3]) and not bool(live[-1]) and float(g32[n][:, -3].abs().max()) == 0.0
            live[-3] = live[-1] = True
        assert bool(live.all()), "a table row without a gradient"
        assert e <= FLOOR_FACTOR * floor + F32_FLOOR, (n, e, floor)
        for leaf in ("attn.q_bias", "attn.v_bias", "gamma_1", "gamma_2"):
            n = f"blocks.{i}.{leaf}"
            assert float(grads[n].abs().max()) > 0.0 and _rel(grads[n], g32[n]) <= FLOOR_FACTOR * _rel(g16[n], g32[n]) + F32_FLOOR, n
    assert not any("k_bias" in n or "relative_position_index" in n for n in grads)


def test_beit_sees_its_tables(be, dev):
    """with the tables zeroed in the model alone the logits leave the bound of the logits test (FLOOR_FACTOR x the floor): that test does not pass on an attention
    without the bias"""
    model, ref, x, wts, logits, grads, l32, g32, l16, g16 = setup(be, dev, "bf16")
    blind = copy.deepcopy(model).eval()
    with torch.no_grad():
        for blk in blind.blocks:
            blk.attn.relative_position_bias_table.zero_()
        e, floor = _rel(blind(x.to(dev)).cpu(), l32[0]), _rel(l16[0], l32[0])
    print(f"beit logits with zero tables: {e:.3e}, floor {floor:.3e}")
    assert e > FLOOR_FACTOR * floor


def test_beit_state_dict_round_trip_and_deepcopy(be, dev):
    model, ref = setup(be, dev, "bf16")[:2]
    sd = model.state_dict()
    assert set(sd) == set(ref.state_dict()) and sd["blocks.0.attn.relative_position_bias_table"].shape == (124, 2) and sd["blocks.1.gamma_2"].shape == (128,)
    assert not any(k.endswith(("k_bias", "relative_position_index", "_uses", "pos_embed", "qkv.bias")) for k in sd) and "fc_norm.weight" in sd and "norm.weight" not in sd
    fresh = BeitRef(**TINY)
    fresh.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    other = beit.Beit(beit.BeitSpec(**TINY), device=dev, backend=be, seed=2)
    other.load_state_dict({k: v.to(dev) for k, v in fresh.state_dict().items()}, strict=True)
    for (n, a), (_, b) in zip(sorted(model.state_dict().items()), sorted(other.state_dict().items())):
        assert torch.equal(a.cpu(), b.cpu()), n
    ema = copy.deepcopy(model)
    assert ema.be is model.be and ema.blocks[0].attn.qkv.weight.data_ptr() != model.blocks[0].attn.qkv.weight.data_ptr()
    x = setup(be, dev, "bf16")[2].to(dev)
    with torch.no_grad():
        assert torch.equal(ema.eval()(x), model.eval()(x))


def test_beit_init_reset_and_token_path(be, dev):
    """init: zero tables, gammas at init_values, zero q / v biases, LayerNorms 1 / 0; reset_parameters re-draws Conv / Linear weights and zeroes Linear biases and leaves
    gamma_*, q_bias, v_bias, the tables, cls_token and the LayerNorms alone.  num_classes = 0 with global_pool = '': norm.* and no fc_norm.*, the normed tokens [B, 37, D]
    within the floor rule of the restatement"""
    kw = {**TINY, "num_classes": 0}
    model = beit.Beit(beit.BeitSpec(**kw, global_pool="", init_values=1e-5), device=dev, backend=be, seed=3).eval()
    for n, p in model.named_parameters():
        if "gamma_" in n:
            assert bool((p.detach().cpu() == 1e-5).all()), n
        elif "norm" in n:
            assert bool((p.detach() == (1.0 if n.endswith("weight") else 0.0)).all()), n
        elif n.endswith(("relative_position_bias_table", "q_bias", "v_bias")) or (n.endswith(".bias") and n != "patch_embed.proj.bias"):
            assert float(p.detach().abs().max()) == 0.0, n
    assert 0.015 < float(model.blocks[1].mlp.fc2.weight.detach().std()) < 0.025 and 0.0 < float(model.cls_token.detach().abs().max()) < 0.1
    keys = set(model.state_dict())
    assert {"norm.weight", "norm.bias"} <= keys and not any(k.startswith(("fc_norm", "head")) for k in keys)
    trained_like(model, seed=4)
    keep = {n: p.detach().clone() for n, p in model.named_parameters()}
    with torch.no_grad():
        model.blocks[0].attn.proj.bias.fill_(0.5)
    model.reset_parameters()
    for n, p in model.named_parameters():
        left_alone = "gamma_" in n or "norm" in n or n == "cls_token" or n.endswith(("relative_position_bias_table", "q_bias", "v_bias")) or n == "patch_embed.proj.bias"
        if left_alone:
            assert torch.equal(p.detach(), keep[n]), n
        elif n.endswith(".bias"):
            assert float(p.detach().abs().max()) == 0.0, n
        else:
            assert not torch.equal(p.detach(), keep[n]) and 0.015 < float(p.detach().std()) < 0.025, n
    trained_like(model, seed=4)
    ref = BeitRef(**kw, global_pool="")
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    x = torch.randn(2, 3, 96, 96, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        f = model(x.to(dev)).cpu()
        want32 = ref(x)
        with bf16ops.precision("bf16_operands"):
            want16 = ref(x)
    e, floor = _rel(f, want32), _rel(want16, want32)
    print(f"beit tokens: engine {e:.3e} floor {floor:.3e}")
    assert tuple(f.shape) == (2, 37, 128) and e <= FLOOR_FACTOR * floor


def test_create_model_ids_and_refusals(be, dev):
    assert set(beit.TIMM_BEITS) == {"beit_base_patch16_224", "beit_large_patch16_224", "beitv2_base_patch16_224", "beitv2_large_patch16_224"}
    for bad in ("beit_base_patch16_384", "timm-beit_large_patch16_512.in22k_ft_in22k_in1k", "beitv2_huge_patch16_224"):
        with pytest.raises(KeyError, match="beit_base_patch16_224"):
            beit.create_model(bad, device=dev, backend=be)
    with pytest.raises(RuntimeError):
        beit.create_model("beit_base_patch16_224", pretrained=True, device=dev, backend=be)
    with pytest.raises(TypeError, match="init_values"):
        beit.create_model("beit_base_patch16_224", init_values=1.0, device=dev, backend=be)
    for bad_size in (224 + 8, 256):
        with pytest.raises(ValueError, match="256"):
            beit.create_model("beit_base_patch16_224", img_size=bad_size, device=dev, backend=be)
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        beit.create_model("beit_base_patch16_224", drop_path_rate=0.1, device=dev, backend=be)
    with pytest.raises(ValueError, match="global_pool"):
        beit.create_model("beit_base_patch16_224", global_pool="token", device=dev, backend=be)
    with pytest.raises(ValueError, match="global_pool"):
        beit.create_model("beit_base_patch16_224", global_pool="", device=dev, backend=be)
    m = beit.create_model("timm-beit_large_patch16_224.in22k_ft_in22k_in1k", num_classes=5, device="meta", backend=be)
    s = m.spec
    assert (s.dim, s.depth, s.heads, s.img_size, s.ln_eps, s.init_values, s.global_pool) == (1024, 24, 16, 224, 1e-6, 0.1, "avg")
    assert m.head.weight.shape == (5, 1024) and m.blocks[23].attn.relative_position_bias_table.shape == (732, 16) and m.tokens == 197 and m.fc_norm.weight.shape == (1024,)
    for name, want in (("beit_base_patch16_224", (768, 12, 12, 0.1)), ("beitv2_base_patch16_224", (768, 12, 12, 1e-5)), ("beitv2_large_patch16_224", (1024, 24, 16, 1e-5))):
        s = beit.create_model(name, img_size=240, num_classes=0, global_pool="", device="meta", backend=be).spec
        assert (s.dim, s.depth, s.heads, s.init_values) == want and s.global_pool == "" and s.img_size == 240


def test_uses_table_lists_every_position_once():
    idx = beit.relative_position_index(6)
    uses = beit._uses_table(idx, 11 * 11 + 3)
    assert uses.dtype == torch.int32 and uses.shape == (124, 36)
    flat = idx.reshape(-1)
    for r in (0, 60, 121, 122, 123):
        u = uses[r][uses[r] >= 0].long()
        assert torch.equal(u, (flat == r).nonzero().view(-1)), r
    assert int((uses >= 0).sum()) == 37 * 37


# ---- routing (visiondk_amd/face.py) ----------------------------------------------------------------------------------------------------------------------
def test_get_model_routes_beit_ids(be, dev):
    """`name: timm-beit_base_patch16_224.in22k_ft_in22k` (the first id of the reference's READMEs) -> VisionWrapper -> beit.create_model, and the same id as a cbir
    backbone -> TimmWrapper with the token neck; construction only, on the meta device; the 384 id is a KeyError with the served list"""
    from visiondk_amd import face
    cfg = {"task": "classification", "name": "timm-beit_base_patch16_224.in22k_ft_in22k", "image_size": 224, "num_classes": 5, "pretrained": True}
    m = face.get_model(cfg, None, 0, backend=be, device="meta").model
    assert isinstance(m, beit.Beit) and (m.spec.dim, m.spec.depth, m.spec.heads, m.spec.img_size, m.spec.global_pool) == (768, 12, 12, 224, "avg")
    assert m.head.weight.shape == (5, 768) and m.blocks[0].attn.relative_position_bias_table.shape == (732, 12)
    with pytest.raises(KeyError, match="beit_base_patch16_224"):
        face.get_model({**cfg, "name": "timm-beit_base_patch16_384.in22k_ft_in22k_in1k"}, None, 0, backend=be, device="meta")
    w = face.TimmWrapper("beit_base_patch16_224", feat_dim=8, image_size=224, pretrained=False, backend=be, device="meta")
    assert isinstance(w.model, beit.Beit) and not w.is_cnn and w.model.spec.global_pool == "" and w.output_layer[2].weight.shape == (8, 197 * 768)
    with pytest.raises(NotImplementedError, match="beitv2_large_patch16_224"):
        face.TimmWrapper("beit_base_patch16_384", feat_dim=8, image_size=384, pretrained=False, backend=be, device="meta")


def test_face_model_with_a_beit_backbone(be, dev, monkeypatch):
    """a cbir config with the tiny spec: FaceTrainingModel forward and backward through the transformer neck and ArcFace; the embedding against the same module sequence in
    torch on the restatement's tokens within the floor rule; FusedTrainStep / FaceTrainStep / forward_precise refuse the model and name the follow-up"""
    from visiondk_amd import face, vit
    monkeypatch.setitem(beit.TIMM_BEITS, "beit_test_patch16_224", dict(dim=128, depth=2, heads=2, init_values=0.1))
    torch.manual_seed(0)
    cfg = {"task": "cbir", "image_size": 96, "load_from": None,
           "backbone": {"timm-beit_test_patch16_224.in22k_ft_in22k": {"pretrained": False, "image_size": 96, "feat_dim": 64}},
           "head": {"arcface": {"feat_dim": 64, "num_class": 24, "margin_arc": 0.35, "margin_am": 0.0, "scale": 32}}}
    model = face.get_model(cfg, None, 0, backend=be, device=dev).model.train()
    w = model.trainingwrapper["backbone"]
    assert isinstance(w.model, beit.Beit) and not w.is_cnn and w.model.operand == w.operand and w.model.spec.global_pool == ""
    assert isinstance(w.output_layer[0], torch.nn.LayerNorm) and w.output_layer[2].weight.shape == (64, 37 * 128)
    trained_like(w.model, seed=11)
    ref = BeitRef(img_size=96, num_classes=0, dim=128, depth=2, heads=2, global_pool="")
    ref.load_state_dict({k: v.detach().cpu() for k, v in w.model.state_dict().items()}, strict=True)
    neck = copy.deepcopy(w.output_layer).cpu().train()
    x = torch.randn(4, 3, 96, 96, generator=torch.Generator().manual_seed(2))          # (four images: a train-mode BatchNorm over two is a sign function)
    labels = torch.tensor([1, 5, 7, 23])
    emb = w(x.to(dev))

    def neck16(f):                                   # the neck as the wrapper runs it in a 16-bit mode: LayerNorm, Flatten, the Linear on 16-bit operands, BatchNorm1d
        n16 = copy.deepcopy(w.output_layer).cpu().train()
        return n16[3](bf16ops.linear(n16[1](n16[0](f)), n16[2].weight, n16[2].bias))

    with torch.no_grad():
        e32 = neck(ref(x))
        with bf16ops.precision(MODE[w.operand]):
            e16 = neck16(ref(x))
    e, floor = _rel(emb.detach().cpu(), e32), _rel(e16, e32)
    print(f"beit cbir embedding: engine {e:.3e} floor {floor:.3e}")
    assert emb.shape == (4, 64) and e <= FLOOR_FACTOR * floor
    out = model(x.to(dev), labels.to(dev))
    loss = torch.nn.functional.cross_entropy(out.float(), labels.to(dev))
    loss.backward()
    grads = {n: p.grad for n, p in w.model.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    assert all(float(grads[f"blocks.{i}.attn.relative_position_bias_table"].abs().sum()) > 0.0 for i in (0, 1))
    for make in (lambda: vit.FusedTrainStep(w.model, lr=0.01), lambda: face.FaceTrainStep(model, lr=0.01), lambda: w.forward_precise(x.to(dev))):
        with pytest.raises(NotImplementedError, match="LayerScale \\+ bias mode of the native vdk_vit"):
            make()
