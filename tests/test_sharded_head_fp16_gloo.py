"""The class-sharded margin head on fp16 operands under the GradScaler protocol, across ranks: two gloo ranks on the CPU emulation (the same workers run on the MI355X in
tests/test_sharded_head_fp16_gpu.py).  Each rank holds half of the classes and half of the batch: the sharded fp16 head equals the full fp16 head on the whole batch,
`FaceTrainStep(shard_head=True)` over an fp16 backbone equals the replicated-head step, and an overflowing step is skipped by both ranks together -- the inf / NaN of one
shard's scaled gradient reaches every rank through the all-reduced feature gradient and the all-reduced norm of the shards' gradients, no host read involved."""
import copy
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent
SCALE = 1024.0


def _init(rank, world, port, mode):
    """mode 'emu': the SIMT emulation on CPU tensors; 'hip': the product library, every rank on cuda:0"""
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    if mode == "emu":
        os.environ["VDK_EMU_THREADS"] = "2"
    else:
        torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if mode == "emu":
        from tests.emu.emu_backend import load_emu
        return load_emu(), "cpu"
    from visiondk_amd import _lib
    return _lib.load(), "cuda:0"


def _face_cfg():
    from tests.test_ddp_gloo import FACE_CFG
    cfg = copy.deepcopy(FACE_CFG)
    cfg["backbone"]["timm-convnext_test"]["operand"] = "fp16"
    return cfg


def _face_model(be, seed, dev):
    from visiondk_amd import convnext, face
    convnext.TIMM_CONVNEXTS["convnext_test"] = dict(depths=(1, 1, 1, 1), dims=(8, 16, 24, 32))
    torch.manual_seed(seed)
    model = face.get_model(_face_cfg(), None, 0, backend=be, device=dev).model.train()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("gamma"):
                p.fill_(0.4)
    return model


def _head_inputs():
    D, Cn, B = 64, 96, 6
    torch.manual_seed(21)
    W = torch.randn(D, Cn); feats = torch.randn(2 * B, D); labels = torch.randint(0, Cn, (2 * B,))
    labels[0], labels[B] = 3, 90                                  # targets on both shards for both ranks' samples
    return D, Cn, B, W, feats, labels


def _mk_head(tag, D, Cn, be, dev):
    from visiondk_amd import heads
    return heads.ArcFace(D, Cn, backend=be, device=dev) if tag == "arcface" else heads.MV_Softmax(D, Cn, is_am=False, backend=be, device=dev)


# ---- 2 ranks x (half of the classes, half of the batch) == the full fp16 head on the whole batch -------------------------------------------------------------------
def sharded_head_worker(rank, world, port, out_dir, mode):
    be, dev = _init(rank, world, port, mode)
    from visiondk_amd import heads
    D, Cn, B, W, feats, labels = _head_inputs()
    ls = torch.tensor([SCALE, 0.0, 0.0], device=dev)
    out = {}
    for tag in ("arcface", "mv_arc"):
        head = _mk_head(tag, D, Cn, be, dev)
        c0 = rank * (Cn // 2)
        loss, df, dW = heads.sharded_margin_ce(head, feats[rank * B:(rank + 1) * B].contiguous().to(dev), labels[rank * B:(rank + 1) * B].contiguous().to(dev),
                                               W[:, c0:c0 + Cn // 2].contiguous().to(dev), c0, Cn, label_smoothing=0.1, operand="fp16", loss_scale=ls)
        out[tag] = (loss.cpu(), df.cpu(), dW.cpu())
    torch.save(out, f"{out_dir}/sh{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


def check_sharded_head(tmp_path, be, dev):
    r = [torch.load(tmp_path / f"sh{i}.pt") for i in range(2)]
    D, Cn, B, W, feats, labels = _head_inputs()
    rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()
    ls = torch.tensor([SCALE, 0.0, 0.0], device=dev)
    for tag in ("arcface", "mv_arc"):
        head = _mk_head(tag, D, Cn, be, dev)
        with torch.no_grad():
            head.weight.copy_(W.to(dev))
        # the full fp16 head on the whole batch under the same loss scale, with the same per-sample gradient scale (1 / B_local)
        loss, df, dW = (t.cpu() for t in head.margin_ce(feats.to(dev), labels.to(dev), label_smoothing=0.1, grad_scale=1.0 / B, operand="fp16", loss_scale=ls))
        got_loss = torch.cat([r[0][tag][0], r[1][tag][0]]); got_df = torch.cat([r[0][tag][1], r[1][tag][1]]); got_dW = torch.cat([r[0][tag][2], r[1][tag][2]], 1)
        res = (rel(got_loss, loss), rel(got_df, df), rel(got_dW, dW))
        print(tag, res)
        assert torch.isfinite(got_df).all() and torch.isfinite(got_dW).all() and got_dW.abs().max() > 0
        assert res[0] < 1e-5, (tag, res)
        assert res[1] < 5e-3 and res[2] < 5e-3, (tag, res)      # the bounds of the bf16 form (test_ddp_gloo.py); fp16 rounds 8x finer


@pytest.mark.slow
def test_two_rank_class_sharded_fp16_head_equals_full_fp16_head(tmp_path, emu):
    port = 29500 + ((os.getpid() + 61) % 500)
    mp.start_processes(sharded_head_worker, args=(2, port, str(tmp_path), "emu"), nprocs=2, join=True, start_method="spawn")
    check_sharded_head(tmp_path, emu, "cpu")


# ---- FaceTrainStep(shard_head=True) over an fp16 backbone == the replicated-head fp16 step ------------------------------------------------------------------------------
def _step_state(step):
    return {"params": step.eng.params.detach().cpu().clone(), "neck": [p.detach().cpu().clone() for p in step.bb.output_layer.parameters()]}


def face_shard_worker(rank, world, port, out_dir, mode):
    be, dev = _init(rank, world, port, mode)
    from visiondk_amd import comm, face
    out = {}
    torch.manual_seed(7)
    x = torch.randn(8, 3, 32, 32).to(dev); y = torch.randint(0, 24, (8,)).to(dev)
    lo, hi = rank * 4, rank * 4 + 4
    init = None
    for shard in (False, True):
        model = _face_model(be, 100, dev)
        if init is None:
            init = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(init)                            # the same initial weights for both variants
        step = face.FaceTrainStep(model, lr=0.05, momentum=0.9, weight_decay=5e-4, max_norm=0.5, ema=True, comm=comm.GradAllReduce(bucket_bytes=20_000),
                                  shard_head=shard, layer_wise=True, init_scale=SCALE)
        assert step.amp and step.shard_head == shard
        before = _step_state(step)
        head0 = step.gather_head().detach().cpu().clone()
        rows = step.step(x[lo:hi], y[lo:hi])
        head_w = step.gather_head().detach().cpu().clone()
        head_ema = step.gather_head(ema=True).detach().cpu().clone() if shard else step.ema_small[-1].cpu().clone()
        out[shard] = {"rows": rows.cpu().clone(), "head": head_w, "head_ema": head_ema, "head0": head0, "before": before["params"], "neck_before": before["neck"], "skipped": step.skipped_steps(),
                      "scale": step.loss_scale(), **_step_state(step)}
    torch.save(out, f"{out_dir}/fs{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


def check_face_shard(tmp_path):
    r0 = torch.load(tmp_path / "fs0.pt"); r1 = torch.load(tmp_path / "fs1.pt")
    rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()
    for r in (r0, r1):
        a, b = r[True], r[False]
        for v in (a, b):                                       # a skipped step must not pass as agreement
            assert v["skipped"] == 0 and v["scale"] == SCALE
            assert not torch.equal(v["params"], v["before"]) and not torch.equal(v["head"], v["head0"])
            assert torch.isfinite(v["params"]).all() and torch.isfinite(v["head"]).all()
        res = (rel(a["rows"], b["rows"]), rel(a["params"], b["params"]), rel(a["head"], b["head"]), rel(a["head_ema"], b["head_ema"]),
               [rel(p, q) for p, q in zip(a["neck"], b["neck"])])
        # neck[1], the BatchNorm2d bias: a per-channel shift in front of Linear + train-mode BatchNorm1d, which removes it -- its true gradient is 0, it starts at 0, and
        # what the step leaves in it is the rounding noise of the backward chain (norm ~3e-8 where its sibling, the BatchNorm2d weight, moves by ~1e-4).  The ratio of two
        # noise vectors says nothing (measured on the emulation: 1.2e-2, from one fp16 rounding of d(loss)/d(cos) falling the other way); the bound of every other neck
        # tensor is applied to it on the scale of that sibling's update instead: same shape, same learning rate, same clip factor.
        upd = (b["neck"][0].double() - b["neck_before"][0].double()).norm().item()
        noise = ((a["neck"][1].double() - b["neck"][1].double()).norm().item(), a["neck"][1].norm().item(), b["neck"][1].norm().item(), upd)
        print(res, noise)
        assert res[0] < 1e-5                                                      # same loss rows
        assert res[1] < 1e-4 and res[2] < 1e-4 and res[3] < 1e-5
        assert all(v < 1e-3 for i, v in enumerate(res[4]) if i != 1), res[4]
        assert upd > 0 and noise[0] < 1e-3 * upd and noise[1] < 1e-2 * upd and noise[2] < 1e-2 * upd, noise
    assert torch.equal(r0[True]["head"], r1[True]["head"]) and torch.equal(r0[True]["params"], r1[True]["params"])   # replicas agree after the gather
    assert torch.equal(r0[True]["head_ema"], r1[True]["head_ema"])


@pytest.mark.slow
def test_two_rank_fp16_face_step_with_class_sharded_head(tmp_path, emu):
    port = 29500 + ((os.getpid() + 173) % 500)
    mp.start_processes(face_shard_worker, args=(2, port, str(tmp_path), "emu"), nprocs=2, join=True, start_method="spawn")
    check_face_shard(tmp_path)


# ---- an overflowing step: both ranks skip it together ------------------------------------------------------------------------------------------------------------------
def face_skip_worker(rank, world, port, out_dir, mode):
    be, dev = _init(rank, world, port, mode)
    from visiondk_amd import comm, face
    torch.manual_seed(7)
    x = torch.randn(8, 3, 32, 32).to(dev); y = torch.randint(0, 24, (8,)).to(dev)
    lo, hi = rank * 4, rank * 4 + 4
    model = _face_model(be, 100 + rank, dev)                   # ranks start different; the step object broadcasts rank 0's weights
    step = face.FaceTrainStep(model, lr=0.05, momentum=0.9, weight_decay=5e-4, max_norm=0.5, ema=True, comm=comm.GradAllReduce(bucket_bytes=20_000),
                              shard_head=True, layer_wise=True, init_scale=2.0 ** 40)
    p0, hs0, mom0 = step.eng.params.clone(), step.hs.clone(), step.hs_mom.clone()
    rows = step.step(x[lo:hi], y[lo:hi])
    out = {"rows_finite": bool(torch.isfinite(rows).all()), "skipped1": step.skipped_steps(), "scale1": step.loss_scale(),
           "unchanged": bool(torch.equal(step.eng.params, p0) and torch.equal(step.hs, hs0) and torch.equal(step.hs_mom, mom0))}
    step.loss_state[0] = SCALE                                 # (a usable scale for the second step)
    step.step(x[lo:hi], y[lo:hi])
    out.update(skipped2=step.skipped_steps(), scale2=step.loss_scale(), moved=bool(not torch.equal(step.eng.params, p0) and not torch.equal(step.hs, hs0)),
               params=step.eng.params.cpu().clone(), head=step.gather_head().detach().cpu().clone(), head_ema=step.gather_head(ema=True).detach().cpu().clone(),
               neck=[p.detach().cpu().clone() for p in step.bb.output_layer.parameters()])
    torch.save(out, f"{out_dir}/sk{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


def check_face_skip(tmp_path):
    r0 = torch.load(tmp_path / "sk0.pt"); r1 = torch.load(tmp_path / "sk1.pt")
    for r in (r0, r1):
        assert r["rows_finite"]                                # the loss is never scaled
        assert r["skipped1"] == 1 and r["scale1"] == 2.0 ** 39 and r["unchanged"]
        assert r["skipped2"] == 1 and r["scale2"] == SCALE and r["moved"]
        assert torch.isfinite(r["params"]).all() and torch.isfinite(r["head"]).all()
    assert torch.equal(r0["params"], r1["params"]) and torch.equal(r0["head"], r1["head"]) and torch.equal(r0["head_ema"], r1["head_ema"])
    for p, q in zip(r0["neck"], r1["neck"]):
        assert torch.equal(p, q)


@pytest.mark.slow
def test_two_rank_fp16_sharded_face_step_skips_in_lockstep(tmp_path, emu):
    port = 29500 + ((os.getpid() + 307) % 500)
    mp.start_processes(face_skip_worker, args=(2, port, str(tmp_path), "emu"), nprocs=2, join=True, start_method="spawn")
    check_face_skip(tmp_path)
