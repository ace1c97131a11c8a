"""Class-query attention in the last block of the ViT classifier (csrc/attention_cls.hip, csrc/vit_engine.hip `cls_attn_on`): behind the pruned tail the attention
output is read at the class rows only, so softmax(q K^T) V, the q projection, dQ and the q rows of the qkv weight gradient are computed for one query per image; K and V
of every token.  VDK_VIT_CLS_ATTN=0 keeps the full-size attention behind the pruned tail, VDK_VIT_CLS_TAIL=0 turns both off; the engine reads them per call.

Kernel tests: the two kernels through their test hooks (csrc/vdk_internal.h) beside the full-size kernels on the same inputs, dO zero outside the class rows, both against
a float64 evaluation of the same 16-bit inputs with the rounding points of oracle/bf16ops.py (P rounded once, dS rounded, D from the rounded o).  The class-query kernels
keep the arithmetic of the full-size ones and differ by fp32 summation order, so their error may be at most 1.5 x the full kernels' + 1e-5 (bench.py's rule for its
parity floor).

Engine tests: tests/test_vit_cls_tail.py's model and bounds, three arms.

Measured (emulator and MI355X alike to the digits given): at head dim 64 the class-query kernels and the full-size ones have the same error against float64 to three digits
(o bit-equal to the rounded float64 result; dq / dk / dv 1.6e-3 bf16, 2.0e-4 fp16 -- the rounding of the outputs); at head dim 80 the full-size (streaming)
kernels are 5 x further off on dq / dk and 3e-3 / 4e-4 off on o.  Engine arms: class query against full attention, worst tensor cls_token, 8.3e-4 (bf16, bound 7.8e-3) and 1.1e-4 (fp16,
bound 9.8e-4) at batch 64, where the q projection and the class rows of dh1 run on another GEMM kernel; 3e-10 .. 1e-4 at batch 3; three fused steps 1.5e-7."""
import pytest
import torch

from oracle import bf16ops
from tests.test_vit_cls_tail import CASES, ULP, _fwd_bwd, _pair, _rel
from visiondk_amd import vit

DT = {"bf16": (torch.bfloat16, 0, "bf16_operands"), "fp16": (torch.float16, 2, "fp16_operands")}
# (B, H, N, hd, extra pitch): the test model (N < 64, 6 items: not a multiple of the 4 waves of a workgroup); one key past a 64-lane pass; the flagship's N; head dim 80
# past 256 keys; pitches larger than the rows
SHAPES = [(3, 2, 17, 64, 0), (2, 3, 65, 64, 0), (1, 12, 197, 64, 0), (2, 2, 257, 80, 0), (2, 2, 33, 64, 16)]
NAN = float("nan")


def _inputs(B, H, N, hd, fmt, seed=0):
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    qkv = (torch.randn(B, N, 3 * D, generator=g) * 1.5).to(DT[fmt][0])
    dout = torch.zeros(B, N, D)
    dout[:, 0] = torch.randn(B, D, generator=g)             # random on the class rows, zero elsewhere
    return qkv, dout.to(DT[fmt][0])


_REF = {}


def _reference(B, H, N, hd, fmt):
    """float64 on the 16-bit inputs, class query only: o, lse, dq [B, D]; dk, dv [B, N, D].  Computed once per case."""
    key = (B, H, N, hd, fmt)
    if key not in _REF:
        qkv, dout = _inputs(B, H, N, hd, fmt)
        D = H * hd
        x = qkv.double().reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)          # [3, B, H, N, hd]
        q = x[0][:, :, :1].clone().requires_grad_(True)
        k = x[1].clone().requires_grad_(True)
        v = x[2].clone().requires_grad_(True)
        scale = hd ** -0.5
        with bf16ops.precision(DT[fmt][2]):
            o = bf16ops.attention(q, k, v, scale)                                # [B, H, 1, hd], rounded to the format
            o.backward(dout.double()[:, 0].reshape(B, H, 1, hd))
        lse = torch.logsumexp((q.detach() @ k.detach().transpose(-2, -1)) * scale, dim=-1)[..., 0]       # [B, H]
        flat = lambda t: t.permute(0, 2, 1, 3).reshape(B, -1, D)
        _REF[key] = {"o": flat(o.detach())[:, 0], "lse": lse, "dq": flat(q.grad)[:, 0], "dk": flat(k.grad), "dv": flat(v.grad)}
    return _REF[key]


def _pitched(t, pad, dev, fill=NAN):
    """a [B, N, C + pad] buffer on `dev` filled with `fill`, its [.., :C] view holding t (pad = 0: contiguous)"""
    B, N, C = t.shape
    buf = torch.full((B, N, C + pad), fill, dtype=t.dtype, device=dev)
    buf[..., :C] = t.to(dev)
    return buf


def _run(be, dev, which, qkv, dout, H, hd, fmt, pad=0, grid=0, poison_inputs=False):
    """forward + backward through the class-query hooks (`which` = "cls") or the full-size entry points ("full"); outputs are pre-filled with NaN.
    -> dict of CPU tensors: o [B, N, D], lse [B, H, N], dqkv [B, N, 3 D], cs [B, 3 D] (cls only)"""
    B, N, D3 = qkv.shape
    D = D3 // 3
    dt = DT[fmt][1]
    scale = hd ** -0.5
    qkv = qkv.clone(); dout = dout.clone()
    if poison_inputs:                       # what the class-query kernels must not read
        qkv[:, 1:, :D] = NAN; dout[:, 1:] = NAN
    qb = _pitched(qkv, pad, dev); gb = _pitched(dout, pad // 2, dev)
    ob = torch.full((B, N, D + pad // 2), NAN, dtype=qkv.dtype, device=dev)
    db = torch.full((B, N, D3 + pad), NAN, dtype=qkv.dtype, device=dev)
    lse = torch.full((B, H, N), NAN, dtype=torch.float32, device=dev)
    cs = torch.full((B, D3), NAN, dtype=torch.float32, device=dev)
    dvec = torch.empty((B, H, N), dtype=torch.float32, device=dev)
    ld, ldo = D3 + pad, D + pad // 2
    p = be.ptr
    if which == "cls":
        be.check(be.lib.vdk_debug_attention_cls_fwd(p(qb), ld, p(ob), ldo, p(lse), B, N, H, hd, scale, dt, grid, be.stream()), "cls fwd")
        be.check(be.lib.vdk_debug_attention_cls_bwd(p(qb), ld, p(ob), p(gb), ldo, p(lse), p(db), ld, p(cs), B, N, H, hd, scale, dt, grid, be.stream()), "cls bwd")
    else:
        be.check(be.lib.vdk_attention_fwd_dt(p(qb), ld, p(ob), ldo, p(lse), B, N, H, hd, scale, dt, be.stream()), "fwd")
        be.check(be.lib.vdk_attention_bwd_dt(p(qb), ld, p(ob), p(gb), ldo, p(lse), p(db), ld, p(dvec), B, N, H, hd, scale, dt, be.stream()), "bwd")
    if be.device_only:
        torch.cuda.synchronize()
    return {"o": ob[..., :D].cpu(), "lse": lse.cpu(), "dqkv": db[..., :D3].cpu(), "cs": cs.cpu()}


def _errors(r, ref, D):
    return {"o": _rel(r["o"][:, 0], ref["o"]), "lse": _rel(r["lse"][:, :, 0], ref["lse"]), "dq": _rel(r["dqkv"][:, 0, :D], ref["dq"]),
            "dk": _rel(r["dqkv"][..., D:2 * D], ref["dk"]), "dv": _rel(r["dqkv"][..., 2 * D:], ref["dv"])}


def _bits_equal(a, b):
    """same bits, NaNs included"""
    return all(torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)) for k in a)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,N,hd,pad", SHAPES)
def test_cls_kernels_against_the_full_kernels(be, dev, B, H, N, hd, pad, fmt):
    """o, lse, dq of the class rows, dk and dv of every row: Frobenius-relative error against float64 <= 1.5 x the full kernels' + 1e-5.  Guard rows: what the class-query
    kernels do not own (o, dq, lse of the other rows) keeps its NaN pre-fill, what they own is finite; the column-sum by-product equals the sums of the stored rows."""
    D = H * hd
    qkv, dout = _inputs(B, H, N, hd, fmt)
    ref = _reference(B, H, N, hd, fmt)
    new = _run(be, dev, "cls", qkv, dout, H, hd, fmt, pad)
    old = _run(be, dev, "full", qkv, dout, H, hd, fmt, pad)
    en, eo = _errors(new, ref, D), _errors(old, ref, D)
    print(f"cls attention [{fmt} B{B} H{H} N{N} hd{hd} pad{pad}]: " + " ".join(f"{k} {en[k]:.3e} (full {eo[k]:.3e})" for k in en))
    for k in en:
        assert en[k] <= 1.5 * eo[k] + 1e-5, (k, en[k], eo[k])
    assert torch.isnan(new["o"][:, 1:].float()).all() and torch.isnan(new["lse"][:, :, 1:]).all() and torch.isnan(new["dqkv"][:, 1:, :D].float()).all()
    assert torch.isfinite(new["o"][:, 0].float()).all() and torch.isfinite(new["lse"][:, :, 0]).all() and torch.isfinite(new["dqkv"][:, 0].float()).all()
    assert torch.isfinite(new["dqkv"][..., D:].float()).all()
    cs = torch.cat([new["dqkv"][:, 0, :D].double(), new["dqkv"][..., D:].double().sum(1)], dim=1)
    assert _rel(new["cs"], cs) <= 1e-5, _rel(new["cs"], cs)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_cls_kernels_do_not_read_the_other_rows(be, dev, fmt):
    """q, o and dO of the non-class rows given as NaN (o: the forward's own NaN pre-fill) change no bit of the result"""
    B, H, N, hd = 3, 2, 17, 64
    qkv, dout = _inputs(B, H, N, hd, fmt, seed=1)
    assert _bits_equal(_run(be, dev, "cls", qkv, dout, H, hd, fmt), _run(be, dev, "cls", qkv, dout, H, hd, fmt, poison_inputs=True))


@pytest.mark.parametrize("B,H,N,hd", [(3, 2, 17, 64), (2, 2, 257, 80)])
def test_cls_kernels_same_bits_on_any_grid(be, dev, B, H, N, hd):
    """a wave walks over several items when the grid is small; the sums have a fixed order: 1, 2 and 5 workgroups give the default grid's bits"""
    for fmt in ("bf16", "fp16"):
        qkv, dout = _inputs(B, H, N, hd, fmt, seed=2)
        base = _run(be, dev, "cls", qkv, dout, H, hd, fmt)
        for grid in (1, 2, 5):
            assert _bits_equal(base, _run(be, dev, "cls", qkv, dout, H, hd, fmt, grid=grid)), (fmt, grid)


def test_cls_kernels_unsupported_shapes(be, dev):
    """head dims other than 64 and 80, more than 1024 keys: VDK_EUNSUPPORTED, nothing launched"""
    from visiondk_amd import _abi
    z = torch.zeros(8, dtype=torch.bfloat16, device=dev)
    f = torch.zeros(8, device=dev)
    p = be.ptr
    for N, hd in ((8, 72), (1025, 64)):
        assert be.lib.vdk_debug_attention_cls_fwd(p(z), 3 * hd, p(z), hd, p(f), 1, N, 1, hd, 0.125, 0, 0, be.stream()) == _abi.EUNSUPPORTED
        assert be.lib.vdk_debug_attention_cls_bwd(p(z), 3 * hd, p(z), p(z), hd, p(f), p(z), 3 * hd, None, 1, N, 1, hd, 0.125, 0, 0, be.stream()) == _abi.EUNSUPPORTED


# ------------------------------------------------------------------------------------------------------------------ engine
ARMS = [("class query", {}), ("full attention", {"VDK_VIT_CLS_ATTN": "0"}), ("full path", {"VDK_VIT_CLS_TAIL": "0"})]


def _three_arms(monkeypatch, run):
    out = []
    for _, env in ARMS:
        for k in ("VDK_VIT_CLS_ATTN", "VDK_VIT_CLS_TAIL"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out.append(run())
    for k in ("VDK_VIT_CLS_ATTN", "VDK_VIT_CLS_TAIL"):
        monkeypatch.delenv(k, raising=False)
    return out


@pytest.mark.parametrize("operand,depth,B,pre_norm", CASES)
def test_three_arms_agree(be, dev, monkeypatch, operand, depth, B, pre_norm):
    """logits and every parameter gradient, pairwise over the three arms, within one unit in the last place of the operand format (tests/test_vit_cls_tail.py's bound:
    the arms feed the same operands to every row that is read, and differ by fp32 summation order and the odd last-bit flip that follows from it)"""
    _, model = _pair(be, dev, depth=depth, operand=operand, pre_norm=pre_norm)
    torch.manual_seed(5)
    x = torch.randn(B, 3, 32, 32); y = torch.randint(0, 10, (B,))
    S = 1024.0 if operand == "fp16" else 1.0
    res = _three_arms(monkeypatch, lambda: _fwd_bwd(model, x, y, dev, S))
    assert all(torch.isfinite(g).all() for g in res[0][1].values())
    for i in range(3):
        for j in range(i + 1, 3):
            (li, gi), (lj, gj) = res[i], res[j]
            errs = sorted((_rel(gi[n], gj[n]), n) for n in gj)
            print(f"{ARMS[i][0]} vs {ARMS[j][0]} [{operand} depth {depth} B {B} pre_norm {pre_norm}]: logits {_rel(li, lj):.3e}, worst grad {errs[-1][0]:.3e} ({errs[-1][1]})")
            assert _rel(li, lj) <= ULP[operand], (ARMS[i][0], ARMS[j][0], _rel(li, lj))
            for r, n in errs:
                assert r <= ULP[operand], (ARMS[i][0], ARMS[j][0], n, r)


@pytest.mark.parametrize("operand,depth", [("bf16", 2), ("bf16", 1), ("fp16", 2), ("fp16", 1)])
def test_class_query_path_against_the_fp32_oracle(be, dev, monkeypatch, operand, depth):
    """the default path against oracle/vit_ref.py in fp32 with tests/test_vit_cls_tail.py's tolerances: bf16 logits 2e-2, gradients 6e-2; fp16 logits 1e-3, gradients 5e-3"""
    for k in ("VDK_VIT_CLS_ATTN", "VDK_VIT_CLS_TAIL"):
        monkeypatch.delenv(k, raising=False)
    ref, model = _pair(be, dev, depth=depth, operand=operand)
    torch.manual_seed(5)
    x = torch.randn(3, 3, 32, 32); y = torch.randint(0, 10, (3,))
    lr = ref(x)
    torch.nn.functional.cross_entropy(lr, y, label_smoothing=0.05).backward()
    lo, g = _fwd_bwd(model, x, y, dev, 1024.0 if operand == "fp16" else 1.0)
    tol_l, tol_g = (1e-3, 5e-3) if operand == "fp16" else (2e-2, 6e-2)
    errs = sorted((_rel(g[n], p.grad), n) for n, p in ref.named_parameters())
    print(f"class-query path vs fp32 oracle [{operand} depth {depth}]: logits {_rel(lo, lr.detach()):.3e}, worst grad {errs[-1][0]:.3e} ({errs[-1][1]})")
    assert _rel(lo, lr.detach()) <= tol_l, _rel(lo, lr.detach())
    for r, n in errs:
        assert r <= tol_g, (n, r)


def test_fused_steps_three_arms(be, dev, monkeypatch):
    """three FusedTrainStep.step calls with EMA on fp16 operands, as tests/test_vit_cls_tail.py runs them: equal loss-scale state, every tensor's update pairwise within
    twice the one-pass bound"""
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

    res = _three_arms(monkeypatch, run)
    for i in range(3):
        for j in range(i + 1, 3):
            (si, ui), (sj, uj) = res[i], res[j]
            assert torch.equal(si, sj), (si, sj)
            errs = sorted((_rel(ui[n], uj[n]), n) for n in uj)
            print(f"{ARMS[i][0]} vs {ARMS[j][0]}, 3 fused steps fp16: worst update {errs[-1][0]:.3e} ({errs[-1][1]})")
            for r, n in errs:
                assert r <= 2 * ULP["fp16"], (ARMS[i][0], ARMS[j][0], n, r)


def _attn_switch(monkeypatch, run):
    monkeypatch.delenv("VDK_VIT_CLS_TAIL", raising=False)
    monkeypatch.delenv("VDK_VIT_CLS_ATTN", raising=False)
    a = run()
    monkeypatch.setenv("VDK_VIT_CLS_ATTN", "0")
    b = run()
    monkeypatch.delenv("VDK_VIT_CLS_ATTN", raising=False)
    return a, b


@pytest.mark.parametrize("class_token", [True, False])
def test_feature_mode_ignores_the_switch(be, dev, monkeypatch, class_token):
    """num_classes = 0 (every token is an output): the full path either way, bit for bit"""
    spec = vit.VitSpec(img_size=32, patch_size=8, in_chans=3, num_classes=0, dim=128, depth=2, heads=2, mlp_dim=256, ln_eps=1e-6, class_token=class_token)
    eng = vit.VisionTransformer(spec, device=dev, backend=be, seed=1).engine
    torch.manual_seed(2)
    x = torch.randn(3, 3, 32, 32).to(dev)
    dt = (torch.randn(3 * eng.tokens, 128) * 0.1).to(dev)

    def run():
        out = eng.forward(x).detach().cpu().clone()
        return out, eng.backward(dt).detach().cpu().clone()

    (oa, ga), (ob, gb) = _attn_switch(monkeypatch, run)
    assert torch.equal(oa, ob) and torch.equal(ga, gb)
    assert torch.isfinite(ga).all() and float(ga.abs().max()) > 0


def test_fp8_mode_ignores_the_switch(be, dev, monkeypatch):
    """the fp8 mode keeps the full path (no pruned tail, so no class-query attention): bit for bit (smallest fp8 model of tests/test_vit_fp8.py, current scaling)"""
    spec = vit.VitSpec(img_size=64, patch_size=8, num_classes=10, dim=256, depth=2, heads=4, mlp_dim=512)
    torch.manual_seed(2)
    x = torch.randn(4, 3, 64, 64); y = torch.randint(0, 10, (4,))

    def run():
        model = vit.VisionTransformer(spec, device=dev, backend=be, seed=1)
        model.engine.enable_fp8(2)
        return _fwd_bwd(model, x, y, dev)

    (la, ga), (lb, gb) = _attn_switch(monkeypatch, run)
    assert torch.equal(la, lb)
    for n in gb:
        assert torch.equal(ga[n], gb[n]), n
