"""The class-token tail of the ViT engine's classifier mode (csrc/vit_engine.hip `cls_tail_on`): behind the last block's attention only the B class-token rows are
computed -- proj + residual, norm2, the MLP, and their backward -- because the head (timm global_pool='token') reads nothing else.  VDK_VIT_CLS_TAIL=0 keeps the
full-size path; the engine reads it per call, so both arms run in one process.

The model is tests/test_vit.py's (32x32 input, patch 8, 17 tokens, dim 128, 2 heads, mlp 256, 10 classes) with its weight perturbation.

Pruned against full: the two paths feed identical operands to every class row, so they can differ only in the order of fp32 accumulation (another GEMM tile shape, other
row splits of the column sums) and, through that, in an occasional last-bit flip of a 16-bit rounding: the bound is ONE unit in the last place of the operand format
(2^-10 fp16, 2^-7 bf16) on the logits and on every parameter gradient, Frobenius-relative.  A wiring error -- a non-class row read, a forgotten zero-fill, a pitch that
drifts -- shows as O(1).  Measured: logits bit-equal in every case; worst gradient 1.4e-7 on the emulator, 1.1e-7 on the MI355X (weight gradients and column sums of
the last block add B rows instead of B x N rows in another split order); three fused steps: updates bit-equal on the emulator, 4.0e-7 on the MI355X."""
import pytest
import torch

from oracle.vit_ref import VisionTransformerRef
from visiondk_amd import vit

ULP = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -7}


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def _pair(be, dev, depth=2, operand="bf16", pre_norm=False, seed=0):
    torch.manual_seed(seed)
    ref = VisionTransformerRef(32, 8, 3, 10, 128, depth, 2, 256, pre_norm=pre_norm)
    with torch.no_grad():      # tests/test_vit.py's perturbation: biases / norms / cls carry signal, 4x branch weights give O(1) activations
        for n, p in ref.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.05)
        ref.cls_token.add_(torch.randn_like(ref.cls_token) * 0.02)
        for blk in ref.blocks:
            for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
                lin.weight.mul_(4.0)
    spec = vit.VitSpec(img_size=32, patch_size=8, in_chans=3, num_classes=10, dim=128, depth=depth, heads=2, mlp_dim=256, ln_eps=1e-6, pre_norm=pre_norm)
    model = vit.VisionTransformer(spec, device=dev, backend=be, seed=1, operand=operand)
    model.load_state_dict(ref.state_dict())
    return ref, model


def _fwd_bwd(model, x, y, dev, scale=1.0):
    """logits and every parameter gradient (divided by the loss scale the backward ran under)"""
    for p in model.parameters():
        p.grad = None
    lo = model(x.to(dev))
    (torch.nn.functional.cross_entropy(lo, y.to(dev), label_smoothing=0.05) * scale).backward()
    return lo.detach().cpu().clone(), {n: p.grad.detach().cpu().clone() / scale for n, p in model.named_parameters()}


def _both_arms(monkeypatch, run):
    """run() with the tail pruned (the default) and with the full-size path"""
    monkeypatch.delenv("VDK_VIT_CLS_TAIL", raising=False)
    pruned = run()
    monkeypatch.setenv("VDK_VIT_CLS_TAIL", "0")
    full = run()
    monkeypatch.delenv("VDK_VIT_CLS_TAIL", raising=False)
    return pruned, full


# batch 3: ragged rows, the transposing weight-gradient path with padded rows; batch 64: B % 64 == 0, the TN weight-gradient path reads the class rows at pitch N * D
CASES = [(op, depth, B, False) for op in ("bf16", "fp16") for depth in (2, 1) for B in (3, 64)] + [("fp16", 2, 3, True)]


@pytest.mark.parametrize("operand,depth,B,pre_norm", CASES)
def test_pruned_tail_matches_the_full_path(be, dev, monkeypatch, operand, depth, B, pre_norm):
    """logits and every parameter gradient, tensor by tensor, within one unit in the last place of the operand format.
    Measured worst over the nine cases: logits 0 (bit-equal), gradients 1.4e-7 (emulator) / 1.1e-7 (MI355X) against 9.8e-4 (fp16) and 7.8e-3 (bf16)."""
    _, model = _pair(be, dev, depth=depth, operand=operand, pre_norm=pre_norm)
    torch.manual_seed(5)
    x = torch.randn(B, 3, 32, 32); y = torch.randint(0, 10, (B,))
    S = 1024.0 if operand == "fp16" else 1.0
    (lp, gp), (lf, gf) = _both_arms(monkeypatch, lambda: _fwd_bwd(model, x, y, dev, S))
    errs = sorted((_rel(gp[n], gf[n]), n) for n in gf)
    print(f"cls tail vs full [{operand} depth {depth} B {B} pre_norm {pre_norm}]: logits {_rel(lp, lf):.3e}, worst grad {errs[-1][0]:.3e} ({errs[-1][1]}), "
          f"bit-equal grads {sum(int(torch.equal(gp[n], gf[n])) for n in gf)} of {len(gf)}")
    assert all(torch.isfinite(g).all() for g in gp.values())
    assert _rel(lp, lf) <= ULP[operand], _rel(lp, lf)
    for r, n in errs:
        assert r <= ULP[operand], (n, r)


@pytest.mark.parametrize("operand,depth", [("bf16", 2), ("bf16", 1), ("fp16", 2), ("fp16", 1)])
def test_pruned_tail_against_the_fp32_oracle(be, dev, monkeypatch, operand, depth):
    """the pruned path (the default) against oracle/vit_ref.py in fp32: bf16 with the tolerances of tests/test_vit.py::test_forward_backward_vs_oracle (logits 2e-2,
    gradients 6e-2), fp16 with those of tests/test_fp16_operands.py (logits 1e-3, gradients 5e-3; backward under the loss scale 1024).  Depth 1: block 0 is the last block.
    Measured on the MI355X: bf16 logits 5.0e-3 / 4.7e-3 and worst gradient 9.8e-3 / 1.2e-2 (depth 2 / 1); fp16 logits 7.2e-4 / 6.5e-4, worst gradient 1.2e-3 / 1.0e-3."""
    monkeypatch.delenv("VDK_VIT_CLS_TAIL", raising=False)
    ref, model = _pair(be, dev, depth=depth, operand=operand)
    torch.manual_seed(5)
    x = torch.randn(3, 3, 32, 32); y = torch.randint(0, 10, (3,))
    lr = ref(x)
    torch.nn.functional.cross_entropy(lr, y, label_smoothing=0.05).backward()
    lo, g = _fwd_bwd(model, x, y, dev, 1024.0 if operand == "fp16" else 1.0)
    tol_l, tol_g = (1e-3, 5e-3) if operand == "fp16" else (2e-2, 6e-2)
    errs = sorted((_rel(g[n], p.grad), n) for n, p in ref.named_parameters())
    print(f"cls tail vs fp32 oracle [{operand} depth {depth}]: logits {_rel(lo, lr.detach()):.3e}, worst grad {errs[-1][0]:.3e} ({errs[-1][1]})")
    assert _rel(lo, lr.detach()) <= tol_l, _rel(lo, lr.detach())
    for r, n in errs:
        assert r <= tol_g, (n, r)


def test_fused_step_pruned_against_full(be, dev, monkeypatch):
    """three FusedTrainStep.step calls with EMA on fp16 operands: equal loss-scale state, and the UPDATE every tensor received within twice the one-pass bound
    (measured: bit-equal on the emulator, worst 4.0e-7 on the MI355X against 1.95e-3)"""
    def run():
        _, model = _pair(be, dev, operand="fp16", seed=3)
        init = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
        step = vit.FusedTrainStep(model, lr=0.01, momentum=0.937, weight_decay=5e-4, label_smoothing=0.05, max_norm=10.0, ema=True)
        torch.manual_seed(11)
        for _ in range(3):
            x = torch.randn(4, 3, 32, 32); y = torch.randint(0, 10, (4,))
            step.step(x.to(dev), y.to(dev))
        sd = model.state_dict()
        return step.loss_state.cpu().clone(), {n: sd[n].cpu() - init[n] for n in init}

    (sp, up), (sf, uf) = _both_arms(monkeypatch, run)
    assert torch.equal(sp, sf), (sp, sf)
    errs = sorted((_rel(up[n], uf[n]), n) for n in uf)
    print(f"cls tail vs full, 3 fused steps fp16: worst update {errs[-1][0]:.3e} ({errs[-1][1]}), loss state {sp.tolist()}")
    for r, n in errs:
        assert r <= 2 * ULP["fp16"], (n, r)


@pytest.mark.parametrize("class_token", [True, False])
def test_feature_mode_ignores_the_switch(be, dev, monkeypatch, class_token):
    """num_classes = 0 (every token is an output), with and without a class token: the full path either way, bit for bit"""
    spec = vit.VitSpec(img_size=32, patch_size=8, in_chans=3, num_classes=0, dim=128, depth=2, heads=2, mlp_dim=256, ln_eps=1e-6, class_token=class_token)
    model = vit.VisionTransformer(spec, device=dev, backend=be, seed=1)
    eng = model.engine
    torch.manual_seed(2)
    x = torch.randn(3, 3, 32, 32).to(dev)
    dt = (torch.randn(3 * eng.tokens, 128) * 0.1).to(dev)

    def run():
        out = eng.forward(x).detach().cpu().clone()
        return out, eng.backward(dt).detach().cpu().clone()

    (op, gp), (of, gf) = _both_arms(monkeypatch, run)
    assert torch.equal(op, of) and torch.equal(gp, gf)
    assert torch.isfinite(gp).all() and float(gp.abs().max()) > 0


def test_fp8_mode_takes_the_full_path(be, dev, monkeypatch):
    """the fp8 GEMMs want M >= 256 rows: the fp8 mode keeps the full path (smallest fp8 model of tests/test_vit_fp8.py, current scaling), bit for bit"""
    spec = vit.VitSpec(img_size=64, patch_size=8, num_classes=10, dim=256, depth=2, heads=4, mlp_dim=512)
    torch.manual_seed(2)
    x = torch.randn(4, 3, 64, 64); y = torch.randint(0, 10, (4,))

    def run():
        model = vit.VisionTransformer(spec, device=dev, backend=be, seed=1)
        model.engine.enable_fp8(2)
        return _fwd_bwd(model, x, y, dev)

    (lp, gp), (lf, gf) = _both_arms(monkeypatch, run)
    assert torch.equal(lp, lf)
    for n in gf:
        assert torch.equal(gp[n], gf[n]), n
