"""One rank of tests/test_gpu_clip.py's DDP test (not collected by pytest): the tiny model of
tests/_ddp_worker.py plus one parameter nothing uses, its half of the 2-clip batch, two Trainer
steps with the gradients averaged by GradBucketer over gloo and clip_grad_norm=1e-3 (far below
the model's gradient norm: both steps clip).

    RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/_clip_ddp_worker.py OUT
Writes OUT.rank<r>.pt: {"params": {name: tensor}, "initial": the same before the first step,
"records": [(norm, coef) per step], "flags" / "unused": the last bucket's flag tail and
globally_unused() per step, read after the optimizer step and before the buckets are zeroed,
"spare_index": the unused parameter's flag, "rebuilds", "buckets", "bucketed"}.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ddp_worker as w  # noqa: E402  (sets the import paths and the gloo backend)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from vdiff.ddp import broadcast_parameters, init_from_env  # noqa: E402


def _named(m):
    return {n: p.detach().cpu().clone() for n, p in m.named_parameters()}


def main(out):
    rank, world, local = init_from_env()          # gloo: no GPU call before this point
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    from vdiff.engine import Clip, Trainer
    from vdiff.schedulers import LinearNoiseScheduler
    m = w.build(dev)
    m.register_parameter("spare", torch.nn.Parameter(torch.full((5,), 0.5, device=dev)))
    broadcast_parameters(m)
    tr = Trainer(m, LinearNoiseScheduler(100, 0.00085, 0.012), lr=1e-3, bucket_mb=0.25,
                 clip_grad_norm=1e-3)
    initial = _named(m)
    bk = tr.bucketer
    flags, unused = [], []
    zero_grad = bk.zero_grad

    def spy():  # the averaged, clipped buckets as the optimizer saw them
        flags.append(bk.flags.detach().cpu().clone())
        unused.append(bk.globally_unused())
        zero_grad()
    bk.zero_grad = spy
    x0, cond, feat, eps, t = w.batch(dev)
    T = x0.shape[2]
    sl = slice(rank, rank + 1)
    clip = Clip(x0[sl], cond[sl], feat[rank * T:(rank + 1) * T], eps[sl], t[sl])
    records = []
    for _ in range(2):
        tr.step(clip)
        records.append((tr.grad_norm.detach().cpu().clone(), tr.clip_coef.detach().cpu().clone()))
    tr.check_finite()
    torch.save({"params": _named(m), "initial": initial, "records": records, "flags": flags,
                "unused": unused, "spare_index": bk.index[m.spare],
                "rebuilds": tr.clipper.rebuilds, "buckets": len(bk.buckets),
                "bucketed": bk is not None},
               f"{out}.rank{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
