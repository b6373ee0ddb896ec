"""One rank of tests/test_gpu_ema.py's DDP test (not collected by pytest): the tiny model of
tests/_ddp_worker.py, its half of the 2-clip batch, two Trainer steps with the gradients
averaged by GradBucketer over gloo and ema_rates=(0.5, 0.9).

    RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/_ema_ddp_worker.py OUT
Writes OUT.rank<r>.pt: {"shadows": {"<rate>/<name>": tensor}, "initial": the same before the
first step, "num_updates": n, "bucketed": the trainer averaged gradients across ranks}.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ddp_worker as w  # noqa: E402  (sets the import paths and the gloo backend)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from vdiff.ddp import broadcast_parameters, init_from_env  # noqa: E402


def _named(ema):
    return {f"{r}/{n}": s.detach().cpu().clone()
            for r, sh in zip(ema.rates, ema.shadows) for n, s in zip(ema.names, sh)}


def main(out):
    rank, world, local = init_from_env()          # gloo: no GPU call before this point
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    from vdiff.engine import Clip, Trainer
    from vdiff.schedulers import LinearNoiseScheduler
    m = w.build(dev)
    broadcast_parameters(m)
    tr = Trainer(m, LinearNoiseScheduler(100, 0.00085, 0.012), lr=1e-3, bucket_mb=0.25,
                 ema_rates=(0.5, 0.9))
    initial = _named(tr.ema)
    x0, cond, feat, eps, t = w.batch(dev)
    T = x0.shape[2]
    sl = slice(rank, rank + 1)
    clip = Clip(x0[sl], cond[sl], feat[rank * T:(rank + 1) * T], eps[sl], t[sl])
    for _ in range(2):
        tr.step(clip)
    tr.check_finite()
    torch.save({"shadows": _named(tr.ema), "initial": initial,
                "num_updates": int(tr.ema.num_updates), "bucketed": tr.bucketer is not None},
               f"{out}.rank{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
