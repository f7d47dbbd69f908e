"""batch_norm_ma under data parallelism (2 gloo ranks on the CPU): every rank moves its running
statistics with its own slice; rank 0's are authoritative and reach the other ranks before
anything reads them (evaluate / forward_to / prepare_save)."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_bn_ma_cpu import B, C1, _trainer
from test_dp_gloo import _free_port


def _batch(seed):
    from cxxnet_amd.io.data import DataBatch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C1, 2, 2, generator=g)
    x[B // 2:] = x[B // 2:] * 3 + 2  # the two ranks' slices have different statistics
    return DataBatch(x, torch.randint(0, 4, (B, 1), generator=g).float())


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = _trainer()
    tr.init_model()
    for seed in (1, 2):
        tr.update(_batch(seed))
    rec = {"before": tr.net.bn_state.clone()}
    tr.evaluate(None, "train")
    rec["after_eval"] = tr.net.bn_state.clone()
    tr.update(_batch(3))
    rec["before_save"] = tr.net.bn_state.clone()
    tr.prepare_save()
    rec["after_prepare"] = tr.net.bn_state.clone()
    if rank == 0:
        rec["model"] = tr.save_model(sync=False)
    tr.update(_batch(4))
    rec["before_fwd"] = tr.net.bn_state.clone()
    tr.forward_to([len(tr.net.nodes) - 1], _batch(5))
    rec["after_fwd"] = tr.net.bn_state.clone()
    torch.save(rec, out + ".r%d" % rank)
    dist.destroy_process_group()


def test_rank0_statistics_are_authoritative(tmp_path):
    out = str(tmp_path / "bn")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0 = torch.load(out + ".r0", weights_only=False)
    r1 = torch.load(out + ".r1", weights_only=False)
    for before, after in (("before", "after_eval"), ("before_save", "after_prepare"), ("before_fwd", "after_fwd")):
        assert not torch.equal(r0[before], r1[before]), before  # each rank followed its own slice
        assert torch.equal(r0[after], r1[after]), after
        assert torch.equal(r0[after], r0[before]), after        # ... and rank 0's values won
    # rank 0's model file holds them
    tr = _trainer()
    tr.load_model(r0["model"])
    assert torch.equal(tr.net.bn_state, r0["before_save"])
