"""The class-sharded margin head on fp16 operands under a loss scale, on the MI355X: two processes, BOTH on cuda:0, exchanging over gloo (as in
tests/test_ddp_two_ranks_gpu.py; RCCL refuses two ranks on one device, and N > 1 on RCCL is not measured on hardware).  The workers of
tests/test_sharded_head_fp16_gloo.py on the product library, and cfg3's head at its real width -- ArcFace over 10^6 identities, two shards of 500 000 columns -- against the
fp32 oracle at north_star's tolerance.

test_arcface_one_million_identities_sharded_fp16_vs_oracle, measured on the MI355X (16 rows, loss scale 1024, cos_planes = 1): loss 2.7e-6 (rows 1.4e-5),
d(feats) 2.5e-4, dW 2.5e-4, worst of the 16 target columns of dW 3.3e-4 -- against the asserted 1e-3 / 5e-3 / 5e-3."""
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import test_sharded_head_fp16_gloo as two_rank

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_two_ranks_on_the_gpu_class_sharded_fp16_head_equals_full_fp16_head(tmp_path, hip):
    mp.start_processes(two_rank.sharded_head_worker, args=(2, _free_port(), str(tmp_path), "hip"), nprocs=2, join=True, start_method="spawn")
    two_rank.check_sharded_head(tmp_path, hip, DEV)


def test_two_ranks_on_the_gpu_fp16_face_step_with_class_sharded_head(tmp_path, hip):
    mp.start_processes(two_rank.face_shard_worker, args=(2, _free_port(), str(tmp_path), "hip"), nprocs=2, join=True, start_method="spawn")
    two_rank.check_face_shard(tmp_path)


def test_two_ranks_on_the_gpu_fp16_sharded_face_step_skips_in_lockstep(tmp_path, hip):
    mp.start_processes(two_rank.face_skip_worker, args=(2, _free_port(), str(tmp_path), "hip"), nprocs=2, join=True, start_method="spawn")
    two_rank.check_face_skip(tmp_path)


# ---- cfg3's head at its real width, sharded ------------------------------------------------------------------------------------------------------------------------------
C_TOTAL, D_FEAT, B_RANK, S_LOSS = 1_000_000, 512, 8, 1024.0


def _million_inputs():
    """the head's own initialisation (unit-norm columns, arcface.py:11-12) and 16 embeddings, from a fixed seed: every process builds the same tensors on the CPU"""
    g = torch.Generator().manual_seed(0)
    W = torch.empty(D_FEAT, C_TOTAL).uniform_(-1, 1, generator=g).renorm_(2, 1, 1e-5).mul_(1e5)
    f = torch.randn(2 * B_RANK, D_FEAT, generator=g)
    y = torch.randint(0, C_TOTAL, (2 * B_RANK,), generator=g)
    y[1], y[B_RANK] = C_TOTAL - 1, 3                              # targets on both shards for both ranks' samples
    return W, f, y


def _million_worker(rank, world, port, out_dir):
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from visiondk_amd import _lib, heads
    be = _lib.load()
    W, f, y = _million_inputs()
    cper = C_TOTAL // world
    c0 = rank * cper
    shard = W[:, c0:c0 + cper].contiguous().to(DEV)
    del W
    head = heads.ArcFace(D_FEAT, 8, margin_arc=0.35, margin_am=0.0, scale=32, backend=be, device=DEV)      # the head's configuration; the weight is the shard passed below
    ls = torch.tensor([S_LOSS, 0.0, 0.0], device=DEV)
    loss, df, dW = heads.sharded_margin_ce(head, f[rank * B_RANK:(rank + 1) * B_RANK].contiguous().to(DEV), y[rank * B_RANK:(rank + 1) * B_RANK].contiguous().to(DEV),
                                           shard, c0, C_TOTAL, operand="fp16", loss_scale=ls, cos_planes=1)
    torch.save({"loss": loss.cpu(), "df": df.cpu(), "dW": dW.cpu()}, f"{out_dir}/m{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


def test_arcface_one_million_identities_sharded_fp16_vs_oracle(tmp_path, hip):
    """ArcFace(512, C = 10^6, m .35, s 32) as two shards of 500 000 columns on two ranks, 8 rows each, fp16 operands, single-plane cosines, loss scale 1024 -- the conforming
    mode of cfg3 in its multi-GPU layout -- against the reference's arcface.py arithmetic in fp32 on the CPU over the 16 rows (the oracle of
    tests/test_parity_fullsize_gpu.py).  north_star's tolerance, asserted literally: loss <= 1e-3, d(feats) / S and dW / S (shards concatenated) <= 5e-3 as norm ratios.  The
    worst of the 16 target columns of dW is printed, not asserted (the project holds fp16 to no per-column figure at this width).  Each rank's gradient scale is
    1 / B_local, so the oracle's loss is the SUM over the two ranks of their mean losses."""
    from tests.test_parity_fullsize_gpu import _arcface_ref, _rel
    mp.start_processes(_million_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    r = [torch.load(tmp_path / f"m{i}.pt") for i in range(2)]
    W, f, y = _million_inputs()
    W.requires_grad_(True); f.requires_grad_(True)
    rows_ref = torch.nn.functional.cross_entropy(_arcface_ref(f, W, y), y, reduction="none")
    (rows_ref.sum() / B_RANK).backward()
    rows = torch.cat([r[0]["loss"], r[1]["loss"]]); df = torch.cat([r[0]["df"], r[1]["df"]]) / S_LOSS
    dW = torch.cat([r[0]["dW"], r[1]["dW"]], 1) / S_LOSS
    assert torch.isfinite(df).all() and torch.isfinite(dW).all()
    res = {"loss": abs(rows.mean().item() - rows_ref.mean().item()) / abs(rows_ref.mean().item()), "loss_rows": _rel(rows, rows_ref.detach()),
           "dfeats": _rel(df, f.grad), "dW": _rel(dW, W.grad), "dW_worst_target_col": max(_rel(dW[:, c], W.grad[:, c]) for c in y.tolist())}
    print(res)
    assert res["loss"] <= 1e-3, res
    assert res["dfeats"] <= 5e-3 and res["dW"] <= 5e-3, res
